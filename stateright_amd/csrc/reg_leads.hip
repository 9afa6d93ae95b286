// Registry family: the fixtures of the leads-to check (live.hpp LEADS-TO): LeadsGraph (models.hpp) and
// LeadsDGraph (dgraph.hpp); registry.hpp.
#include "dgraph.hpp"
#include "registry.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_leads(const EngineArgs& a) {
    if (a.model == SR_MODEL_LEADS_DGRAPH) return make_for<LeadsDGraph, true>(LeadsDGraph::make(a.p, a.np, a.o->device), a);
    return with_leads_graph(a.p, a.np, [&](const auto& m) { return make_for<std::decay_t<decltype(m)>, true>(m, a); });
}
}  // namespace sr
