#!/usr/bin/env python3
"""Selection beside the whole text: tools/perf_select.py [genome bytes] [read-set bytes] -- on the realistic genome (default 4 GB) and
the read set (default 12.5 GB) of the bench configs, per-call times of (a) one whole record, (b) a 1 Mb region, (c) 1 000 scattered
10 kb regions (reads: 1 000 scattered reads), (d) find of 1 000 ids, each beside naf_gpu_unnaf of the same archive; then the kernel
list of every call.  Warm-up 3, median / min / max of 10, the host clock around calls that end in a device synchronise."""
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from naf_amd import capi, synth

g_size = int(float(sys.argv[1])) if len(sys.argv) > 1 else int(4e9)
q_size = int(float(sys.argv[2])) if len(sys.argv) > 2 else int(12.5e9)
print("box:", torch.cuda.get_device_name(0), "| torch", torch.__version__, "| hip", torch.version.hip)
ctx = capi.Context(0)


def timed(label, fn):
    for _ in range(3):
        r = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(10):
        t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ts.sort()
    print("%-44s median %9.3f ms  min %9.3f  max %9.3f" % (label, ts[5] * 1e3, ts[0] * 1e3, ts[-1] * 1e3))
    ctx.set_timing(True); fn(); torch.cuda.synchronize()
    for nm, ms, k in sorted(ctx.get_timing(), key=lambda x: -x[1])[:8]:
        print("      %-28s %8.3f ms x%d" % (nm, ms, k))
    ctx.set_timing(False)
    return r


def run(kind, text, mode):
    n = text.numel()
    ctx.reserve(int(n * 1.7) + (2 << 30))
    naf, rep = ctx.ennaf(text)
    naf = naf.clone()
    del text
    N = int(ctx.parse_header(naf).n_sequences)
    nb, off = ctx.unnaf_record_table(naf, 0, None, mode)
    out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    print("== %s: %d bytes of text, %d records, archive %d bytes" % (kind, n, N, naf.numel()))
    timed("whole text (naf_gpu_unnaf)", lambda: ctx.unnaf(naf, mode, out=out))
    rng = np.random.default_rng(1)
    r17 = min(17, N - 1)
    timed("(a) one whole record", lambda: ctx.unnaf_select(naf, [r17], mode, out=out))
    if mode == capi.OUT_FASTA:
        r3 = min(3, N - 1)
        b = int(nb[r3] // 3)
        timed("(b) a 1 Mb region", lambda: ctx.unnaf_select(naf, [(r3, b, b + 1_000_000)], mode, out=out))
        segs = []
        for k in range(1000):
            r = int(rng.integers(0, N)); s = int(rng.integers(0, max(1, nb[r] - 10_000))); segs.append((r, s, s + 10_000))
    else:
        timed("(b) 100 000 consecutive reads", lambda: ctx.unnaf_select(naf, list(range(N // 2, N // 2 + 100_000)), mode, out=out))
        segs = [int(r) for r in rng.integers(0, N, 1000)]
    timed("(c) 1 000 scattered", lambda: ctx.unnaf_select(naf, segs, mode, out=out))
    # the ids of 1 000 records, read out of the whole text
    recs = sorted(int(r) for r in rng.integers(0, N, 1000))
    ids = []
    for r in recs:
        head = ctx.unnaf_range(naf, off[r], min(off[r] + 256, off[r + 1]), mode).cpu().numpy().tobytes()
        ids.append(head[1:head.index(b"\n")].split(b" ")[0])
    got = timed("(d) find of 1 000 ids", lambda: ctx.unnaf_find(naf, ids))
    assert all(g is not None and g <= r for g, r in zip(got, recs))
    del out, naf


run("realistic genome", synth.realistic_genome_device(g_size, device="cuda"), capi.OUT_FASTA)
torch.cuda.empty_cache()
run("read set", synth.fastq_reads_device(q_size, device="cuda"), capi.OUT_FASTQ)
