"""Summary of scripts/pmc_diet.sh: expand_fast<TwoPhaseT<9>> dispatches of at least 100 us (durations
from the kernel-trace pass, matched to the counter pass by dispatch order)."""
import collections
import csv
import glob
import sys

O = sys.argv[1]
CLK = 2.4e9
SIMDS = 256 * 4


def is_k(name):
    return "expand_fast<sr::TwoPhaseT<9>" in name


for v in ("base", "new"):
    kt = glob.glob(f"{O}/kt_{v}/**/*kernel_trace.csv", recursive=True)
    pm = glob.glob(f"{O}/pmc_{v}/**/*counter_collection.csv", recursive=True)
    if not kt or not pm:
        print(v, "missing csv", kt, pm)
        continue
    rows = [r for r in csv.DictReader(open(kt[0])) if is_k(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    names = [r["Kernel_Name"] for r in rows]
    per = collections.OrderedDict()
    pts = {}
    for r in csv.DictReader(open(pm[0])):
        if not is_k(r["Kernel_Name"]):
            continue
        d = int(r["Dispatch_Id"])
        per.setdefault(d, {"name": r["Kernel_Name"]})[r["Counter_Name"]] = float(r["Counter_Value"])
        try:
            pts[d] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        except (KeyError, ValueError):
            pass
    ids = sorted(per)
    print(f"== {v}: {len(durs)} traced dispatches, {len(ids)} counted dispatches")
    big = [i for i, d in enumerate(durs) if d >= 100.0]
    print(f"   kernel-trace: {len(big)} dispatches >= 100 us, sum {sum(durs[i] for i in big):.1f} us, all {sum(durs):.1f} us")
    for i in big[:len(big) // 3 if len(big) >= 3 else len(big)]:
        print(f"     #{i} {durs[i]:.1f} us")
    if len(ids) == len(durs):
        sel = [ids[i] for i in big]
        how = "matched by dispatch order"
        dur_us = sum(durs[i] for i in big)
    else:
        sel = [d for d in ids if pts.get(d, 0) >= 100.0]
        how = "counter pass's own timestamps (dispatch counts differ)"
        dur_us = None
    tot = collections.defaultdict(float)
    for d in sel:
        for k, x in per[d].items():
            if k != "name":
                tot[k] += x
    print(f"   counters over {len(sel)} dispatches ({how}):")
    for k in sorted(tot):
        print(f"     {k} {tot[k]:.4g}")
    if tot.get("SQ_INSTS_VALU") and dur_us:
        cap = dur_us * 1e-6 * CLK * SIMDS / 4
        print(f"   VALU issue: {tot['SQ_INSTS_VALU']:.4g} wave-instructions x 4 cycles over {SIMDS} SIMDs x {dur_us:.1f} us (untraced durations) at 2.4 GHz = {tot['SQ_INSTS_VALU'] / cap:.3f} of issue capacity")
    if tot.get("SQ_ACTIVE_INST_VALU") and tot.get("SQ_BUSY_CYCLES"):
        print(f"   SQ_ACTIVE_INST_VALU * 4 / SQ_BUSY_CYCLES = {tot['SQ_ACTIVE_INST_VALU'] * 4 / tot['SQ_BUSY_CYCLES']:.3f} (per-SIMD share depends on how the SQ instances are summed)")
    if tot.get("SQ_ACTIVE_INST_VALU") and tot.get("GRBM_GUI_ACTIVE"):
        print(f"   VALUBusy = SQ_ACTIVE_INST_VALU * 4 / {SIMDS} / GRBM_GUI_ACTIVE = {tot['SQ_ACTIVE_INST_VALU'] * 4 / SIMDS / tot['GRBM_GUI_ACTIVE']:.3f}")
    if tot.get("SQ_WAVE_CYCLES"):
        print(f"   per wave-cycle: VALU-active {tot.get('SQ_ACTIVE_INST_VALU', 0) * 4 / tot['SQ_WAVE_CYCLES']:.3f}")
