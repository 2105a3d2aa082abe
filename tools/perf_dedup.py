#!/usr/bin/env python3
"""Kernel times of naf_gpu_unnaf_dedup beside its yardstick, k_clip_mark with one adapter of 13 letters, which reads the same packed bytes
once with the same record walk, on the same archive in the same process (profiles/dedup_perf.txt is this script's output on one MI355X;
DESIGN.md section 8q reads it).

    python tools/perf_dedup.py [--short-bytes N] [--long-bytes N]

Three texts: (a) the benchmark's synthetic FASTQ (150-base reads, 12.5 GB by default: the FASTQ leg's size), which has no duplicates;
(b) reads of the same kind and number in which a quarter of the reads copy an earlier read that is no copy itself, a tenth of those as
its reverse complement; (c) reads of 20 000 bases (2000 distinct reads, repeated to the size asked for: every read has many copies).
Every call is made once to warm up and then three times with kernel timing on (HIP events around each launch, naf_gpu_get_timing); a
line is the least of the three sums over a call's launches, the whole call the least wall time of the three beside the sum of its
kernels."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from naf_amd import capi, synth  # noqa: E402
from perf_trim import long_reads  # noqa: E402

A13 = "AGATCGGAAGAGC"
KERNELS = ("unnaf_dedup_stage", "unnaf_dedup_preset", "unnaf_dedup_hash", "unnaf_dedup_join", "unnaf_dedup_insert", "unnaf_dedup_verify", "unnaf_dedup_count", "unnaf_dedup_finish", "unnaf_row_copy")
SHARE, REVERSED = 4, 10                         # one read in SHARE is a copy, one copy in REVERSED its reverse complement


def duplicated_reads(total_bytes, dev, read_len=150, seed=11):
    """FASTQ of ~total_bytes: fixed-width records "@r%010d", uniform ACGT; row k > 0 with k % SHARE == 0 takes the bases of a random earlier
    row that is no copy, every REVERSED-th of them reversed and complemented"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    width = 2 + 10 + 1 + read_len + 3 + read_len + 1
    n = max(SHARE + 1, total_bytes // width)
    m = torch.empty((n, width), dtype=torch.uint8, device=dev)
    m[:, 0:2] = torch.tensor(list(b"@r"), dtype=torch.uint8, device=dev)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    for d in range(10):
        m[:, 2 + d] = ((ids // (10 ** (9 - d))) % 10 + 48).to(torch.uint8)
    m[:, 12] = 10
    p = 13
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    step = 1 << 22
    for a in range(0, n, step):
        b = min(n, a + step)
        m[a:b, p:p + read_len] = lut[torch.randint(0, 4, (b - a, read_len), dtype=torch.int64, device=dev, generator=g)]
        m[a:b, p + read_len + 3:p + 2 * read_len + 3] = torch.randint(33, 74, (b - a, read_len), dtype=torch.int64, device=dev, generator=g).to(torch.uint8)
    m[:, p + read_len:p + read_len + 3] = torch.tensor(list(b"\n+\n"), dtype=torch.uint8, device=dev)
    m[:, width - 1] = 10
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)
    comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    copies = torch.arange(SHARE, n, SHARE, dtype=torch.int64, device=dev)
    for a in range(0, copies.numel(), step):
        c = copies[a:a + step]
        src = (torch.rand(c.numel(), device=dev, generator=g, dtype=torch.float64) * (c - 1).double()).long()      # an earlier row, 0 <= src < c - 1 ...
        src = src + (src % SHARE == 0).long() * (src > 0).long()                                                 # ... that is no copy itself (row 0 is none)
        bases = m[src, p:p + read_len]
        rev = (torch.arange(c.numel(), device=dev) % REVERSED == 0)
        bases[rev] = comp[bases[rev].long()].flip(1)
        m[c, p:p + read_len] = bases
    return m.reshape(-1), int(copies.numel())


def timed(ctx, label, fn, names, bases, reps=3):
    """the least time per kernel name and the least wall time of the call; returns ({name: ms}, wall ms)"""
    fn()
    best, wall = {}, None
    for _ in range(reps):
        ctx.set_timing(True)
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        w = (time.perf_counter() - t0) * 1e3
        wall = w if wall is None or w < wall else wall
        t = {n: (ms, k) for n, ms, k in ctx.get_timing()}
        ctx.set_timing(False)
        for n in names:
            if n in t and (n not in best or t[n][0] < best[n][0]):
                best[n] = t[n]
    for n in names:
        if n in best:
            print("%-34s %-24s %9.3f ms  %3d launches  %8.1f Gbases/s" % (label, n, best[n][0], best[n][1], bases / best[n][0] / 1e6), flush=True)
    return {n: v[0] for n, v in best.items()}, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short-bytes", type=float, default=12.5e9)
    ap.add_argument("--long-bytes", type=float, default=1e9)
    args = ap.parse_args()
    dev = "cuda"
    ctx = capi.Context(0)
    print("# %s, %s" % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d")), flush=True)
    texts = (("(a) 150-base reads, no copies", lambda: (synth.fastq_reads_device(int(args.short_bytes), seed=7, device=dev), 0)),
             ("(b) 150-base reads, 1/%d copies" % SHARE, lambda: duplicated_reads(int(args.short_bytes), dev)),
             ("(c) 20 kb reads", lambda: (long_reads(int(args.long_bytes), dev), None)))
    for label, make in texts:
        t0 = time.time()
        text, planted = make()
        naf, _ = ctx.ennaf(text)
        naf = naf.clone()
        n_text = text.numel()
        del text
        torch.cuda.empty_cache()
        h = ctx.parse_header(naf)
        bases, N = int(h.orig_size[4]), int(h.n_sequences)                              # (the header counts the sequence section in bases)
        print("# %s: text %d bytes, %d reads, %d bases (packed stream %d bytes), archive %d bytes (made in %.1f s)" % (label, n_text, N, bases, (bases + 1) // 2, naf.numel(), time.time() - t0), flush=True)
        rows = torch.empty(48 * N, dtype=torch.uint8, device=dev)
        crows = torch.empty(40 * N, dtype=torch.uint8, device=dev)
        clip, _ = timed(ctx, label + " clip 13 letters", lambda: ctx.unnaf_clip(naf, [A13], rate="0.1", min_overlap=3, min_len=30, out=crows), ("unnaf_clip_mark",), bases)
        del crows
        for both in (False, True):
            tag = label + (" both strands" if both else " as stored")
            dd, wall = timed(ctx, tag, lambda: ctx.unnaf_dedup(naf, both, out=rows), KERNELS, bases)
            _, tot, levels = ctx.unnaf_dedup(naf, both, out=False)
            print("# %s: hash / clip_mark = %.2f; the call %.3f ms, the sum of its kernels %.3f ms" % (tag, dd["unnaf_dedup_hash"] / clip["unnaf_clip_mark"], wall, sum(dd.values())), flush=True)
            print("# %s: %d reads, %d classes, %d duplicates%s, largest class %d, levels %s" % (tag, tot.reads, tot.classes, tot.duplicates,
                                                                                               "" if planted is None else " (%d planted)" % planted, tot.largest, levels), flush=True)
        del naf, rows
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
