#!/usr/bin/env python3
"""Host time of the unnaf text driver on the cases of tools/unnaf_plan.py (without its switch variants): the wall time of one call with
its final synchronize, 5 calls to warm up, then 30 timed -- median and quartiles in microseconds.  The driver is bound by launches on
archives this small, so host time is what a change of the driver could move.
    tools/perf_unnaf_driver.py > new.txt                      (NAF_GPU_LIB=<another libnaf_gpu.so>: that build; a fresh process each)
    tools/perf_unnaf_driver.py --compare parent1.txt new.txt parent2.txt
compares per case: the new median may be the larger of the two parent medians plus the parent's own run-to-run noise -- the larger of
the difference of its two medians and the interquartile range of its samples (profiles/unnaf_driver_perf.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def measure():
    import numpy as np
    import torch
    from naf_amd import capi
    import unnaf_plan
    ctx = capi.Context(0)
    out = torch.empty(96 << 20, dtype=torch.uint8, device=ctx.device)
    print("# %s  %s" % (torch.cuda.get_device_name(0), "the build NAF_GPU_LIB names" if os.environ.get("NAF_GPU_LIB") else "this build"))
    for case in unnaf_plan.cases(ctx, with_switches=False):
        with unnaf_plan.Env(case[2]):
            t = []
            for k in range(35):
                ctx.synchronize()
                t0 = time.perf_counter()
                unnaf_plan.run(ctx, case, out)
                ctx.synchronize()
                t.append((time.perf_counter() - t0) * 1e6)
        q1, med, q3 = np.percentile(t[5:], [25, 50, 75])
        print("%-32s median %9.1f  q1 %9.1f  q3 %9.1f" % (case[0].replace(" ", "_"), med, q1, q3), flush=True)
    ctx.close()


def read(path):
    rows = {}
    for line in open(path):
        f = line.split()
        if len(f) == 7 and f[1] == "median":
            rows[f[0]] = (float(f[2]), float(f[4]), float(f[6]))
    return rows


def compare(p1, new, p2):
    a, n, b = read(p1), read(new), read(p2)
    bad = 0
    for name in n:
        (ma, qa1, qa3), (mn, _, _), (mb, qb1, qb3) = a[name], n[name], b[name]
        margin = max(abs(ma - mb), qa3 - qa1, qb3 - qb1)
        ok = mn <= max(ma, mb) + margin
        bad += not ok
        print("%-32s parent %9.1f %9.1f  new %9.1f  margin %8.1f  %s" % (name, ma, mb, mn, margin, "ok" if ok else "OUTSIDE"))
    print("%d of %d cases outside the parent's noise" % (bad, len(n)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:]))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure()
