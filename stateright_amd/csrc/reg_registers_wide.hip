// Registry family: the ABD linearizable register past the 8-slot encoding (registry.hpp,
// abd_wide.hpp): 16 network slots (W = 14) or 32 (W = 22). Its own translation unit, so the
// registers family's compile time does not grow.
#include "registry.hpp"
#include "abd_wide.hpp"

namespace sr {
std::unique_ptr<EngineBase> reg_registers_wide(const EngineArgs& a) {
    a.need(1);
    const int C = (int)a.p[0], S = a.np > 1 ? (int)a.p[1] : 2;
    if (act::abd_slots(C, S) == 16) {
        AbdRegisterWide16 m;
        static_cast<act::AbdWideSysT<16>&>(m) = act::AbdWideSysT<16>::make(C, S);
        return make_for(m, a);
    }
    AbdRegisterWide32 m;
    static_cast<act::AbdWideSysT<32>&>(m) = act::AbdWideSysT<32>::make(C, S);
    return make_for(m, a);
}
}  // namespace sr
