// Registry family: ReqLock of 5..8 threads (models.hpp ReqLockT; registry.hpp).
#include "registry.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_req_lock_wide(const EngineArgs& a) {
    return with_req_lock_range<5>(a.p, a.np, [&](const auto& m) { return make_for<std::decay_t<decltype(m)>, true>(m, a); });
}
}  // namespace sr
