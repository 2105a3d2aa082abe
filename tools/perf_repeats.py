#!/usr/bin/env python3
"""What the tandem-repeat table costs beside the homopolymer table of runs, which period 1 answers too: synthetic repeat-masked genomes
(naf_amd/synth.py: realistic_genome_device, 4 GB and 2 GB of FASTA) asked for their repeats with spec 1-10, misa and sixteen periods at 3
copies.  3 warm-up calls, then the median of 10: host time of the call and the kernel times of naf_gpu_get_timing, the two mark passes
with the least and the greatest of the ten samples.  The yardstick, from the same run on the same box: naf_gpu_unnaf_runs of ACGT with
each at min 10 -- the same intervals as spec 1-10.
tools/perf_repeats.py [bytes of FASTA ...] > profiles/repeats_perf.txt   (GPU box, repo root)"""
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from naf_amd import capi, synth

WARM, TAKE = 3, 10
sizes = [int(float(a)) for a in sys.argv[1:]] or [int(4e9), int(2e9)]
ctx = capi.Context(0)
ALL3 = ",".join("%d-3" % p for p in range(1, 17))


def timed(call, marks):
    """(result, median host ms, {kernel name: median ms}, the ten sums of the kernels `marks`) of TAKE calls after WARM warm-up calls"""
    for _ in range(WARM):
        res = call()
    host, kern, both = [], {}, []
    for _ in range(TAKE):
        ctx.set_timing(True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize(); host.append((time.perf_counter() - t0) * 1e3)
        one = {}
        for n, ms, k in ctx.get_timing():
            kern.setdefault(n, []).append(ms)
            one[n] = one.get(n, 0.0) + ms
        both.append(sum(one.get(n, 0.0) for n in marks))
        ctx.set_timing(False)
    return res, statistics.median(host), {n: statistics.median(v) for n, v in kern.items()}, both


def line(name, host, kern, mine):
    own = sum(ms for n, ms in kern.items() if n.startswith(mine))
    top = "  ".join("%s %.3f" % (n, ms) for n, ms in sorted(kern.items(), key=lambda x: -x[1])[:7])
    print("%-32s host %9.3f ms   its kernels %9.3f ms   all kernels %9.3f ms   %s" % (name, host, own, sum(kern.values()), top), flush=True)
    return own


def candidates(d_naf, spec):
    """the candidates of the call's trace line"""
    ctx.set_option("TRACE", "1")
    ctx.unnaf_repeats_count(d_naf, spec)
    text = capi.load().naf_gpu_get_trace(ctx.h).decode("latin1")
    capi.load().naf_gpu_clear_trace(ctx.h)
    ctx.set_option("TRACE", None)
    return int(re.search(r"\[repeats\] rows \d+ candidates (\d+)", text).group(1))


print("box %s   %d warm-up calls, median of %d" % (bench.box_id(), WARM, TAKE))
for genome_bytes in sizes:
    text = synth.realistic_genome_device(genome_bytes, device="cuda")
    ctx.reserve(int(text.numel() * 3.0) + (1 << 30))
    d_naf, rep = ctx.ennaf(text)
    d_naf = d_naf.clone()
    del text
    torch.cuda.empty_cache()
    h = ctx.parse_header(d_naf)
    n_bases, packed = int(h.orig_size[4]), (int(h.orig_size[4]) + 1) // 2
    print("\n== repeat-masked genome, %d B of FASTA: %d records, %d bases (packed stream %d B, sequence frame %d B)" % (
        genome_bytes, h.n_sequences, n_bases, packed, h.comp_size[4]), flush=True)
    n, nb = ctx.unnaf_runs_count(d_naf, "ACGT", True, False, 10)
    buf = torch.empty(32 * n + 32, dtype=torch.uint8, device="cuda")
    _, host, kern, ymarks = timed(lambda: ctx.unnaf_runs(d_naf, "ACGT", True, False, 10, out=buf), ("unnaf_runs_count", "unnaf_runs_write"))
    line("(y) runs ACGT each min 10", host, kern, "unnaf_runs")
    y = statistics.median(ymarks)
    print("    runs %d   the two mark passes %.3f ms (least %.3f, greatest %.3f of %d) = %.1f GB/s of packed bytes each" % (
        n, y, min(ymarks), max(ymarks), TAKE, 2 * packed / max(y, 1e-9) / 1e6), flush=True)
    del buf
    first = None
    for name, spec in (("repeats 1-10", "1-10"), ("repeats misa", "misa"), ("repeats 1-3 .. 16-3", ALL3)):
        n, nb, per = ctx.unnaf_repeats_count(d_naf, spec)
        buf = torch.empty(32 * n + 32, dtype=torch.uint8, device="cuda")
        _, host, kern, marks = timed(lambda: ctx.unnaf_repeats(d_naf, spec, out=buf), ("unnaf_repeats_count", "unnaf_repeats_write"))
        line(name, host, kern, "unnaf_repeats")
        m = statistics.median(marks)
        first = first or m
        print("    rows %d (%.1f MB)   candidates %d   bases in rows %d   the two mark passes %.3f ms (least %.3f, greatest %.3f of %d) = %.1f GB/s of packed bytes each" % (
            n, 32 * n / 1e6, candidates(d_naf, spec), nb, m, min(marks), max(marks), TAKE, 2 * packed / max(m, 1e-9) / 1e6), flush=True)
        print("    mark passes / (y) %.2f   / spec 1-10 %.2f   rows per period %s" % (m / max(y, 1e-9), m / max(first, 1e-9), " ".join(str(v) for v in per)), flush=True)
        del buf
    del d_naf
    torch.cuda.empty_cache()
