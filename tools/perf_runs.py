#!/usr/bin/env python3
"""What the run table costs beside the decode it needs anyway and beside a composition sweep of the same stream: a synthetic repeat-masked
genome (naf_amd/synth.py: realistic_genome_device, 4 GB of FASTA) asked for its runs of N at min 1, of ^N at min 1, of ACGT with each at
min 10, and for its soft-masked intervals.  3 warm-up calls, then the median of 10: host time of the call and the kernel times of
naf_gpu_get_timing.  The yardsticks, from the same run on the same box: (a) every kernel of a NAF_OUT_4BIT unnaf of the archive -- the
decode alone --, (b) naf_gpu_unnaf_composition at window 0, mask off -- one sweep over the same packed bytes.
tools/perf_runs.py [bytes of FASTA] > profiles/runs_perf.txt   (GPU box, repo root)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from naf_amd import capi, synth

WARM, TAKE = 3, 10
genome_bytes = int(float(sys.argv[1])) if len(sys.argv) > 1 else int(4e9)
ctx = capi.Context(0)


def timed(call):
    """(result, median host ms, {kernel name: median ms} of TAKE calls after WARM warm-up calls)"""
    for _ in range(WARM):
        res = call()
    host, kern = [], {}
    for _ in range(TAKE):
        ctx.set_timing(True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize(); host.append((time.perf_counter() - t0) * 1e3)
        for n, ms, k in ctx.get_timing():
            kern.setdefault(n, []).append(ms)
        ctx.set_timing(False)
    return res, statistics.median(host), {n: statistics.median(v) for n, v in kern.items()}


def line(name, host, kern, mine="unnaf_runs"):
    own = sum(ms for n, ms in kern.items() if n.startswith(mine))
    top = "  ".join("%s %.3f" % (n, ms) for n, ms in sorted(kern.items(), key=lambda x: -x[1])[:7])
    print("%-32s host %9.3f ms   its kernels %9.3f ms   all kernels %9.3f ms   %s" % (name, host, own, sum(kern.values()), top), flush=True)
    return own


print("box %s   %d warm-up calls, median of %d" % (bench.box_id(), WARM, TAKE))
text = synth.realistic_genome_device(genome_bytes, device="cuda")
ctx.reserve(int(text.numel() * 3.0) + (1 << 30))
d_naf, rep = ctx.ennaf(text)
d_naf = d_naf.clone()
del text
torch.cuda.empty_cache()
h = ctx.parse_header(d_naf)
n_bases, packed = int(h.orig_size[4]), (int(h.orig_size[4]) + 1) // 2
print("\n== repeat-masked genome, %d B of FASTA: %d records, %d bases (packed stream %d B, sequence frame %d B, mask units %d B)" % (
    genome_bytes, h.n_sequences, n_bases, packed, h.comp_size[4], h.orig_size[3]), flush=True)
out4 = torch.empty(packed + 64, dtype=torch.uint8, device="cuda")
_, host, kern = timed(lambda: ctx.unnaf(d_naf, capi.OUT_4BIT, out=out4))
a = line("(a) unnaf --4bit", host, kern, "")
del out4
n = ctx.unnaf_composition_rows(d_naf, 0)
buf = torch.empty(168 * n + 168, dtype=torch.uint8, device="cuda")
_, host, kern = timed(lambda: ctx.unnaf_composition(d_naf, 0, False, out=buf))
b = line("(b) composition window 0", host, kern, "unnaf_comp")
del buf
for name, cls, each, masked, min_len in (("runs N min 1", "N", False, False, 1), ("runs ^N min 1", "^N", False, False, 1),
                                         ("runs ACGT each min 10", "ACGT", True, False, 10), ("masked runs min 1", None, False, True, 1)):
    n, nb = ctx.unnaf_runs_count(d_naf, cls, each, masked, min_len)
    buf = torch.empty(32 * n + 32, dtype=torch.uint8, device="cuda")
    _, host, kern = timed(lambda: ctx.unnaf_runs(d_naf, cls, each, masked, min_len, out=buf))
    own = line(name, host, kern)
    mark = kern.get("unnaf_runs_count", 0.0) + kern.get("unnaf_runs_write", 0.0)
    print("    runs %d (%.1f MB of rows)   bases in runs %d   the two mark passes %.3f ms = %.1f GB/s of packed bytes each   its kernels / (a) %.2f   / (b) %.2f" % (
        n, 32 * n / 1e6, nb, mark, 2 * packed / max(mark, 1e-9) / 1e6 if mark else 0.0, own / max(a, 1e-9), own / max(b, 1e-9)), flush=True)
    del buf
