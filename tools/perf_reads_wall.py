#!/usr/bin/env python3
"""Wall time of the four read-filter calls -- naf_gpu_unnaf_trim, _clip, _dedup and _screen, the last three on the trim rows as their bounds --
on one archive of the benchmark's synthetic FASTQ (150-base reads): the least and the median of --reps calls after one warm-up call
(profiles/reads_shared_perf.txt holds its output beside that of the four per-kernel tools; DESIGN.md section 8s reads it).

    python tools/perf_reads_wall.py [--bytes N] [--reps N]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from naf_amd import capi, synth  # noqa: E402
from perf_screen import random_reference  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bytes", type=float, default=1e9)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
ctx = capi.Context(0)
text = synth.fastq_reads_device(int(args.bytes), seed=7, device="cuda")
naf, _ = ctx.ennaf(text)
naf = naf.clone()
del text
ref, _ = ctx.ennaf(random_reference(5000, "cuda", 23))
ref = ref.clone()
N = int(ctx.parse_header(naf).n_sequences)
r40, r48 = torch.empty(40 * N, dtype=torch.uint8, device="cuda"), torch.empty(48 * N, dtype=torch.uint8, device="cuda")
tview, _ = ctx.unnaf_trim(naf, capi.trim_limit(20), 30, capi.ee_units("1"), out=torch.empty(40 * N, dtype=torch.uint8, device="cuda"))
calls = (("trim Q20 min 30 max-ee 1", lambda: ctx.unnaf_trim(naf, capi.trim_limit(20), 30, capi.ee_units("1"), out=r40)),
         ("clip 13 letters, trim bounds", lambda: ctx.unnaf_clip(naf, ["AGATCGGAAGAGC"], rate="0.1", min_overlap=3, min_len=30, bounds=tview, out=r40)),
         ("dedup both strands, trim bounds", lambda: ctx.unnaf_dedup(naf, True, bounds=tview, bounds_kind="trim", out=r48)),
         ("screen k 27 ref 5000, trim bounds", lambda: ctx.unnaf_screen(naf, ref, k=27, bounds=tview, bounds_kind="trim", out=r40)))
for label, fn in calls:
    fn()
    ts = []
    for _ in range(args.reps):
        ctx.synchronize(); t0 = time.perf_counter(); fn(); ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    print("wall %-36s unnaf_call least %9.3f ms  median %9.3f ms  %d reads" % (label, ts[0], ts[len(ts) // 2], N), flush=True)
ctx.close()
