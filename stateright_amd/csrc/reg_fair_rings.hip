// Registry family: FairRings, the fixture of the strong-fairness mode (models.hpp FairRings; registry.hpp).
#include "registry.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_fair_rings(const EngineArgs& a) {
    return with_fair_rings(a.p, a.np, [&](const FairRings& m) { return make_for<FairRings, true>(m, a); });
}
}  // namespace sr
