// A GpuModel with a STEP property, built into its own plugin library: a counter that may wrap.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I include \
//         examples/plugins/step_counter.hip -o examples/plugins/libstep_counter.so -L/opt/rocm/lib -lrccl
//
// State: the counter c in 0 ..= max (one parameter, 1 ..= 2^20), one 64-bit word. Actions, in `actions()` order:
// Inc (c < max: c + 1), Skip (c + 2 <= max: c + 2), Wrap (c == max: back to 0). One step property, "no action
// takes the counter down" (include/stateright_gpu_model.hpp, step_holds): Wrap violates it, at the one state
// c == max, whose depth is ceil(max / 2). No state property could say so without a history variable. The step
// pass decides it behind a one-GPU spawn_bfs / spawn_dfs that explored everything; the property's discovery is
// the search's tree path to c == max followed by Wrap.
#include "stateright_gpu_model.hpp"

using sr::i64;
using sr::u32;
using sr::u64;

struct StepCounter {
    static constexpr int W = 1, MW = 1, NPROPS = 1;
    u64 max = 1;

    int max_actions() const { return 3; }
    int max_out_degree() const { return 2; }
    SR_HD void enabled(const u64* s, u64* m) const { m[0] = (u64)(s[0] < max) | (u64)(s[0] + 2 <= max) << 1 | (u64)(s[0] == max) << 2; }
    SR_HD bool apply(const u64* s, int a, u64* o) const {
        o[0] = a == 0 ? s[0] + 1 : a == 1 ? s[0] + 2 : 0;
        return true;
    }
    SR_HD bool discovers(int, const u64*) const { return false; }  // (a step property: the search discovers nothing)
    u32 smask() const { return 1u; }
    SR_HD bool step_holds(int, const u64* s, int, const u64* t) const { return t[0] >= s[0]; }

    int init_states(u64* out) const {
        out[0] = 0;
        return 1;
    }
    int expectation(int) const { return sr::ALWAYS_STEP; }
    const char* prop_name(int) const { return "no action takes the counter down"; }
    int describe_width() const { return 1; }
    void describe(const u64* s, i64* d) const { d[0] = (i64)s[0]; }
    void undescribe(const i64* d, u64* s) const { s[0] = (u64)d[0]; }
    i64 action_id(const u64*, int a) const { return a; }
    std::string action_name(i64 id) const {
        static const char* names[] = {"Inc", "Skip", "Wrap"};
        return id >= 0 && id < 3 ? names[id] : "?";
    }
    i64 action_id_bound() const { return 3; }
};

static StepCounter make_counter(const int64_t* p, int32_t n, int /*device*/) {
    if (n != 1 || p[0] < 1 || p[0] > (1 << 20)) throw sr::Error(SR_ERR_ARG, "step_counter: one parameter, max in 1..=2^20");
    StepCounter m;
    m.max = (u64)p[0];
    return m;
}

SR_GPU_PLUGIN(step_counter, StepCounter, make_counter)
