#!/usr/bin/env python
"""Start and retirement of every group workgroup of an edge-pairing launch (csrc/rows_ga_multi_kernel.h, SH) at C2-L: does the
launch run in one round?

Needs a library built with -DNUTS_KTIMING (tools/build_ticks.sh -> build/libnuts_ticks.so, loaded through PYMC_AMD_LIB).  Every
group workgroup of the LAST paired launch stamps its first instruction and, behind a barrier of its own, its last one; the engine
sums the stamps up (nuts_model_debug_ticks, slots 40 .. 47).  A workgroup that starts after the earliest retirement of the launch
was not resident with the others: it waited for a slot.  100 MHz constant clock.

usage (GPU box): python tools/edge_pair_ticks.py [rows_per_group [groups]]   -- once per paired kernel: NUTS_GA_PACK=0 is the
kernel on raw tiles, without it the one on packed tiles.  (profiles/edge_pair_resident_profile.txt keeps the figures of the
three-waves-per-SIMD kernel this tool was written to examine.)
"""
import ctypes as C
import json
import os
import sys

os.environ["PYMC_AMD_HONOUR_NUTS_ENV"] = "1"   # NUTS_* variables reach the engine as schedule options (nuts_set_option)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PYMC_AMD_LIB", os.path.join(ROOT, "build", "libnuts_ticks.so"))


def main():
    from pymc_amd import _lib, models
    from pymc_amd.sampling import sample

    rpg = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 1248
    spec = models.hier_logit(G=G, D=8, rows_per_group=rpg)
    res = sample(draws=4, tune=26, chains=1, model=spec, init="adapt_diag", random_seed=3, device=0, discard_tuned_samples=False)
    f = res["step"]._logp_dlogp_func
    out = (C.c_int64 * 64)()
    _lib.check(_lib.load().nuts_model_debug_ticks(f._handle, out), "ticks")
    n, s0, e0, e1, late, late_max, late_sum, s1 = (int(v) for v in out[40:48])
    us = lambda t: round(t / 100.0, 2)
    print(json.dumps({
        "workload": f"C2 G={G} rows_per_group={rpg}",
        "options": {k: os.environ.get(k) for k in ("NUTS_GA_PACK",)},
        "edge_pair_packed": f.model_scalar("edge_pair_packed"), "edge_pair_rounds": f.model_scalar("edge_pair_rounds"),
        "rows_waves": f.model_scalar("rows_waves"), "paired_launches": f.model_scalar("edge_pair_shadows"),
        "workgroups_stamped": n,
        "launch_us_first_start_to_last_retirement": us(e1 - s0),
        "earliest_retirement_us_after_first_start": us(e0 - s0),
        "latest_start_us_after_first_start": us(s1 - s0),
        "workgroups_started_after_the_earliest_retirement": late,
        "latest_such_start_us_after_the_earliest_retirement": us(late_max - e0) if late else 0.0,
        "mean_delay_of_those_us": us(late_sum / late) if late else 0.0,
        "last_retirement_us_after_the_earliest": us(e1 - e0),
    }, indent=1))
    res["step"].close()


if __name__ == "__main__":
    main()
