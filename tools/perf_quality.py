#!/usr/bin/env python3
"""What the quality statistics cost beside one read of the same bytes: a synthetic read set (naf_amd/synth.py: fastq_reads_device, 150-base
reads, about 1 GB of FASTQ) through naf_gpu_unnaf_quality with the record table only, the cycle table only (W = 1) and both, with and without
the histogram.  3 warm-up calls, then the median of 10: host time of the call and the kernel times of naf_gpu_get_timing.  The yardstick, from
the same run on the same box: naf_gpu_histogram over the decoded quality bytes -- an existing kernel that reads the same bytes once.
tools/perf_quality.py [bytes of FASTQ] > profiles/quality_perf.txt   (GPU box, repo root)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from naf_amd import capi, synth

WARM, TAKE = 3, 10
reads_bytes = int(float(sys.argv[1])) if len(sys.argv) > 1 else int(1e9)
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


def line(name, host, kern):
    top = "  ".join("%s %.3f" % (n, ms) for n, ms in sorted(kern.items(), key=lambda x: -x[1])[:6])
    print("%-34s host %9.3f ms   all kernels %9.3f ms   %s" % (name, host, sum(kern.values()), top), flush=True)


print("box %s   %d warm-up calls, median of %d" % (bench.box_id(), WARM, TAKE))
text = synth.fastq_reads_device(reads_bytes, device="cuda")
ctx.reserve(int(text.numel() * 3.0) + (1 << 30))
d_naf, rep = ctx.ennaf(text)
d_naf = d_naf.clone()
del text
torch.cuda.empty_cache()
h = ctx.parse_header(d_naf)
qb = int(h.orig_size[5])
print("\n== read set, %d B of FASTQ: %d reads, %d quality bytes (quality frame %d B)" % (reads_bytes, h.n_sequences, qb, h.comp_size[5]), flush=True)
qual = ctx.zstd_decompress(d_naf[int(h.payload_off[5]):int(h.payload_off[5]) + int(h.comp_size[5])], qb, has_magic=False)
assert qual.numel() == qb
_, host, kern = timed(lambda: ctx.histogram(qual))
line("(y) naf_gpu_histogram", host, kern)
y = kern["histogram"]
print("    histogram kernel %.3f ms = %.1f GB/s = %.1f %% of 8 TB/s" % (y, qb / y / 1e6, qb / y / 1e6 / 80), flush=True)
del qual
nr, nc = ctx.unnaf_quality_rows(d_naf, 1)
b_rec = torch.empty(56 * nr + 56, dtype=torch.uint8, device="cuda")
b_cyc = torch.empty(56 * nc + 56, dtype=torch.uint8, device="cuda")
lib, ptr = ctx.L, lambda t: capi.C.c_void_p(t.data_ptr())
for title, W, rec, cyc, hist in (("record table only", 0, True, False, False), ("cycle table only, W = 1", 1, False, True, False), ("both, W = 1", 1, True, True, False),
                                 ("both, W = 1, with h_hist", 1, True, True, True), ("both, W = 100", 100, True, True, False), ("neither, total only", 0, False, False, False)):
    n1, n2, tot, hh = capi.C.c_uint64(), capi.C.c_uint64(), capi.QualRow(), (capi.C.c_uint64 * 256)()

    def call():
        ctx._check(lib.naf_gpu_unnaf_quality(ctx.h, ptr(d_naf), d_naf.numel(), W, 0, capi.WHOLE, ptr(b_rec) if rec else None, nr, ptr(b_cyc) if cyc else None, nc,
                                             capi.C.byref(n1), capi.C.byref(n2), hh if hist else None, capi.C.byref(tot)))
    _, host, kern = timed(call)
    line(title, host, kern)
    k = kern.get("unnaf_qual_count", 0.0)
    moved = qb + (56 * nr if rec else 0)
    print("    k_qual_count %.3f ms = %.1f GB/s of quality bytes = %.1f %% of 8 TB/s (bytes moved: %d read + %d of rows)   / histogram %.2f   total n %d mean %.3f" % (
        k, qb / max(k, 1e-9) / 1e6, qb / max(k, 1e-9) / 1e6 / 80, qb, moved - qb, k / y, tot.n, tot.sum / max(tot.n, 1) - 33), flush=True)
