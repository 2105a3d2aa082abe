#!/usr/bin/env python3
"""Selection beside the whole text: tools/perf_select.py [genome bytes] [read-set bytes] -- on the realistic genome (default 4 GB) and
the read set (default 12.5 GB) of the bench configs, per-call times of (a) one whole record, (b) a 1 Mb region, (c) 1 000 scattered
10 kb regions (reads: 1 000 scattered reads), (d) find of 1 000 ids, each beside naf_gpu_unnaf of the same archive; then the kernel
list of every call.  Rows (a), (b), (c) are followed by their reverse twins -- the same segments as their reverse complements
(naf_gpu_unnaf_select_stranded) -- with the ratio to the forward row of the same run, for the call and for the emit kernel alone.
Warm-up 3, median / min / max of 10, the host clock around calls that end in a device synchronise."""
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
    kernels = ctx.get_timing()
    for nm, ms, k in sorted(kernels, key=lambda x: -x[1])[:8]:
        print("      %-28s %8.3f ms x%d" % (nm, ms, k))
    ctx.set_timing(False)
    timed.last = (ts[5] * 1e3, sum(ms for nm, ms, k in kernels if nm.startswith("unnaf_emit_select")))
    return r


def both_strands(label, naf, segs, mode, out):
    """A row and its reverse twin: the same segments forward, then as reverse complements, and the ratios reverse / forward."""
    W = capi.WHOLE
    fwd = [(s, 0, W) if isinstance(s, int) else s for s in segs]
    timed(label, lambda: ctx.unnaf_select(naf, fwd, mode, out=out))
    f_call, f_emit = timed.last
    rev = [s + (1,) for s in fwd]
    timed(label + ", reverse", lambda: ctx.unnaf_select(naf, rev, mode, out=out))
    r_call, r_emit = timed.last
    print("      reverse / forward: call %.2f, emit kernel %.3f / %.3f ms = %.2f" % (r_call / f_call, r_emit, f_emit, r_emit / f_emit))


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
    both_strands("(a) one whole record", naf, [r17], mode, out)
    if mode == capi.OUT_FASTA:
        r3 = min(3, N - 1)
        b = int(nb[r3] // 3)
        both_strands("(b) a 1 Mb region", naf, [(r3, b, b + 1_000_000)], mode, out)
        segs = []
        for k in range(1000):
            r = int(rng.integers(0, N)); s = int(rng.integers(0, max(1, nb[r] - 10_000))); segs.append((r, s, s + 10_000))
    else:
        both_strands("(b) 100 000 consecutive reads", naf, list(range(N // 2, N // 2 + 100_000)), mode, out)
        segs = [int(r) for r in rng.integers(0, N, 1000)]
    both_strands("(c) 1 000 scattered", naf, segs, mode, out)
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
