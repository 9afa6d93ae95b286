// Registry family: the Spread fixture, one, two and four words (registry.hpp).
#include "registry.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_spread(const EngineArgs& a) {
    return with_spread_model(a.p, a.np, [&](const auto& m) { return make_for(m, a); });
}
}  // namespace sr
