// Registry family: the fixtures without a reference counterpart whose shape is a parameter: Spread, one,
// two and four words, and LiveGraph (registry.hpp).
#include "registry.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_spread(const EngineArgs& a) {
    if (a.model == SR_MODEL_LIVE_GRAPH)
        return with_live_graph(a.p, a.np, [&](const auto& m) { return make_for<std::decay_t<decltype(m)>, true>(m, a); });
    return with_spread_model(a.p, a.np, [&](const auto& m) { return make_for(m, a); });
}
}  // namespace sr
