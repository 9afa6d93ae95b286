// Registry family: SpinLock, the model of the weak-fairness mode (models.hpp SpinLock; registry.hpp).
#include "registry.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_spin_lock(const EngineArgs& a) {
    return with_spin_lock(a.p, a.np, [&](const SpinLock& m) { return make_for<SpinLock, true>(m, a); });
}
}  // namespace sr
