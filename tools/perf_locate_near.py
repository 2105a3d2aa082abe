#!/usr/bin/env python3
"""What a motif search with mismatches costs beside the exact search of the same letters: a synthetic repeat-masked genome
(naf_amd/synth.py: realistic_genome_device, 4 GB of FASTA) and a synthetic read set (fastq_reads_device, 12.5 GB of FASTQ) are searched
for (1) a guide of 20 letters taken from the text with [NGG] behind it, budgets 0 to 6, both strands, (2) a pair of 22-mer primers,
budgets 0 to 3, (3) 16 guides with [NGG] at once, budget 3.  The yardstick of every case is naf_gpu_unnaf_locate with the same letters
unbracketed in the same run -- the exact search's kernels are not touched by the near search.  3 warm-up calls, then the median of 10:
host time of the call and the kernel times of naf_gpu_get_timing.  Each timed call is the one that writes the table (count kernel,
scan, write kernel; a search in several pieces counts once more in front: two sweeps of the count kernel over the packed bytes).
tools/perf_locate_near.py [bytes of FASTA] [bytes of FASTQ] > profiles/locate_near_perf.txt   (GPU box, repo root)"""
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
reads_bytes = int(float(sys.argv[2])) if len(sys.argv) > 2 else int(12.5e9)
ctx = capi.Context(0)


def timed(call):
    """(result, median host ms, {kernel name: (median ms, launches)} of TAKE calls after WARM warm-up calls)"""
    for _ in range(WARM):
        res = call()
    host, kern, launches = [], {}, {}
    for _ in range(TAKE):
        ctx.set_timing(True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize(); host.append((time.perf_counter() - t0) * 1e3)
        for n, ms, k in ctx.get_timing():
            kern.setdefault(n, []).append(ms)
            launches[n] = k
        ctx.set_timing(False)
    return res, statistics.median(host), {n: (statistics.median(v), launches[n]) for n, v in kern.items()}


def archive(text):
    ctx.reserve(int(text.numel() * 3.0) + (1 << 30))
    d_naf, rep = ctx.ennaf(text)
    return d_naf.clone()


def pieces_of(d_naf, n, length, seed):
    """n substrings of `length` bases of the text itself, upper case, made of ACGT only: from places spread over the first record of a
    genome, from the start of reads spread over a read set"""
    h = ctx.parse_header(d_naf)
    lens, _ = ctx.unnaf_record_table(d_naf, 0, 1, capi.OUT_SEQUENCES)
    genome = lens[0] >= 100000
    out, k = [], 0
    while len(out) < n:
        i = len(out) + 1
        rec, at = (0, (lens[0] // (n + 1)) * i + 977 * k + seed) if genome else ((h.n_sequences // (n + 1)) * i + k, seed)
        s = ctx.unnaf_select(d_naf, [(rec, at, at + length)], capi.OUT_SEQ, use_mask=False).cpu().numpy().tobytes().decode().upper()
        k += 1
        if len(s) == length and set(s) <= set("ACGT") and len(set(s)) > 2:
            out.append(s)
            k = 0
    return out


def run_exact(d_naf, letters):
    total, _ = ctx.unnaf_locate_count(d_naf, letters, 3)
    buf = torch.empty(24 * total + 24, dtype=torch.uint8, device="cuda")
    (_, n), host, kern = timed(lambda: ctx.unnaf_locate(d_naf, letters, 3, out=buf))
    assert n == total
    return total, host, kern


def run_near(d_naf, patterns, budget):
    total, per = ctx.unnaf_locate_near_count(d_naf, patterns, budget, 3)
    buf = torch.empty(32 * total + 32, dtype=torch.uint8, device="cuda")
    (_, n), host, kern = timed(lambda: ctx.unnaf_locate_near(d_naf, patterns, budget, 3, out=buf))
    assert n == total
    by_distance = [sum(per[k][s][d] for k in range(len(patterns)) for s in (0, 1)) for d in range(9)]
    return total, by_distance, host, kern


def ms(kern, name):
    return kern.get(name, (0.0, 0))


def measure(title, d_naf, seed):
    h = ctx.parse_header(d_naf)
    n_bases, packed = int(h.orig_size[4]), (int(h.orig_size[4]) + 1) // 2
    print("\n== %s: %d records, %d bases (packed stream %d B, sequence frame %d B)" % (title, h.n_sequences, n_bases, packed, h.comp_size[4]), flush=True)
    guides = pieces_of(d_naf, 16, 20, seed)
    primers = pieces_of(d_naf, 2, 22, seed + 5)
    cases = [("guide 20 + [NGG]", [guides[0] + "[NGG]"], range(0, 7)), ("primer pair 22 + 22", primers, range(0, 4)), ("16 guides 20 + [NGG]", [g + "[NGG]" for g in guides], (0, 3))]
    for name, patterns, budgets in cases:
        letters = [capi.motif_letters(p) for p in patterns]
        print("-- %s: %s%s, both strands" % (name, " ".join(patterns[:2]), " ..." if len(patterns) > 2 else ""), flush=True)
        hits, host, kern = run_exact(d_naf, letters)
        ec, ew = ms(kern, "unnaf_locate_count"), ms(kern, "unnaf_locate_write")
        sweeps = 2 if ec[1] > 1 else 1                                             # several pieces: a counting sweep in front of the one that writes
        print("   exact             hits %10d   host %9.3f ms   count %9.3f ms (%d launches, %d sweeps)   write %8.3f ms   all kernels %9.3f ms   count: %.1f GB/s of packed bytes" % (
            hits, host, ec[0], ec[1], sweeps, ew[0], sum(v for v, _ in kern.values()), sweeps * packed / max(ec[0], 1e-9) / 1e6), flush=True)
        for b in budgets:
            hits, by_d, host, kern = run_near(d_naf, patterns, b)
            nc, nw = ms(kern, "unnaf_locate_near_count"), ms(kern, "unnaf_locate_near_write")
            print("   near budget %d     hits %10d   host %9.3f ms   count %9.3f ms (%d launches)   write %8.3f ms   all kernels %9.3f ms   count: %.1f GB/s   near / exact: count %.2f  write %s   by mismatches %s" % (
                b, hits, host, nc[0], nc[1], nw[0], sum(v for v, _ in kern.values()), sweeps * packed / max(nc[0], 1e-9) / 1e6, nc[0] / max(ec[0], 1e-9),
                "%.2f" % (nw[0] / ew[0]) if ew[0] else "-", by_d), flush=True)


print("box %s   %d warm-up calls, median of %d" % (bench.box_id(), WARM, TAKE), flush=True)
if genome_bytes:
    text = synth.realistic_genome_device(genome_bytes, device="cuda")
    d_naf = archive(text)
    del text
    torch.cuda.empty_cache()
    measure("repeat-masked genome, %d B of FASTA" % genome_bytes, d_naf, 11)
    del d_naf
    torch.cuda.empty_cache()
if reads_bytes:
    text = synth.fastq_reads_device(reads_bytes, device="cuda")
    d_naf = archive(text)
    del text
    torch.cuda.empty_cache()
    measure("read set, %d B of FASTQ" % reads_bytes, d_naf, 3)
