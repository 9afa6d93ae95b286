// Registry family: ReqLock of 1..4 threads, the model of the leads-to check (models.hpp ReqLockT; registry.hpp).
#include "registry.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_req_lock(const EngineArgs& a) {
    return with_req_lock_range<1>(a.p, a.np, [&](const auto& m) { return make_for<std::decay_t<decltype(m)>, true>(m, a); });
}
}  // namespace sr
