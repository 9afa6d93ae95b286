// Registry family: 2pc with its two `eventually` properties (models.hpp TwoPhaseLive; registry.hpp).
#include "registry.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_two_phase_live(const EngineArgs& a) {
    return with_two_phase_live(a.p, a.np, [&](const TwoPhaseLive& m) { return make_for<TwoPhaseLive, true>(m, a); });
}
}  // namespace sr
