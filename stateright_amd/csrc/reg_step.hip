// Registry family: the models of the step pass (step.hpp): StepGraph and TwoPhaseStep (models.hpp) and
// StepDGraph (dgraph.hpp); registry.hpp.
#include "dgraph.hpp"
#include "registry.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_step(const EngineArgs& a) {
    if (a.model == SR_MODEL_STEP_DGRAPH) return make_for(StepDGraph::make(a.p, a.np, a.o->device), a);
    if (a.model == SR_MODEL_2PC_STEP)
        return with_two_phase_step(a.p, a.np, [&](const TwoPhaseStep& m) {
            // (the canonical reduction is 2pc's own; the step pass leaves its properties unchecked there)
            return a.o->symmetry ? make_for(Canon<TwoPhaseStep>(m), a) : make_for(m, a);
        });
    return with_step_graph(a.p, a.np, [&](const auto& m) { return make_for(m, a); });
}
}  // namespace sr
