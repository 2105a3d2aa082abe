#!/usr/bin/env python3
"""Kernel times of naf_gpu_unnaf_clip beside its yardstick, naf_gpu_unnaf_locate_near's count kernel for the same patterns on the forward
strand with budget floor(m / 10), on the same archive in the same process (profiles/clip_perf.txt is this script's output on one MI355X;
DESIGN.md section 8p reads it).

    python tools/perf_clip.py [--short-bytes N] [--long-bytes N]

Two texts: the benchmark's synthetic FASTQ (150-base reads, 12.5 GB by default: the FASTQ leg's size) and reads of 20 000 bases (2000
distinct reads, repeated to the size asked for).  Three questions: one adapter of 13 letters, one of 32, four adapters at once, all at rate
1/10 and min_overlap 3.  Every call is made once to warm up and then three times with kernel timing on (HIP events around each launch,
naf_gpu_get_timing); a line is the least of the three sums over a call's launches -- one launch a piece of 2^31 bases."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from naf_amd import capi, synth  # noqa: E402
from perf_trim import long_reads  # noqa: E402

A13, A32 = "AGATCGGAAGAGC", "AGATCGGAAGAGCACACGTCTGAACTCCAGTC"
FOUR = [A32, "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTG", "CTGTCTCTTATACACATCT", "TGGAATTCTCGGGTGCCAAGG"]


def timed(ctx, label, fn, names, bases, reps=3):
    """the least time per kernel name; returns {name: ms}"""
    fn()
    best = {}
    for _ in range(reps):
        ctx.set_timing(True)
        fn()
        ctx.synchronize()
        t = {n: (ms, k) for n, ms, k in ctx.get_timing()}
        ctx.set_timing(False)
        for n in names:
            if n in t and (n not in best or t[n][0] < best[n][0]):
                best[n] = t[n]
    for n in names:
        if n in best:
            print("%-34s %-24s %9.3f ms  %3d launches  %8.1f Gbases/s" % (label, n, best[n][0], best[n][1], bases / best[n][0] / 1e6), flush=True)
    return {n: v[0] for n, v in best.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short-bytes", type=float, default=12.5e9)
    ap.add_argument("--long-bytes", type=float, default=1e9)
    args = ap.parse_args()
    dev = "cuda"
    ctx = capi.Context(0)
    texts = (("150-base reads", lambda: synth.fastq_reads_device(int(args.short_bytes), seed=7, device=dev)), ("20 kb reads", lambda: long_reads(int(args.long_bytes), dev)))
    for label, make in texts:
        t0 = time.time()
        text = make()
        naf, _ = ctx.ennaf(text)
        naf = naf.clone()
        n_text = text.numel()
        del text
        torch.cuda.empty_cache()
        h = ctx.parse_header(naf)
        bases, N = int(h.orig_size[4]), int(h.n_sequences)                              # (the header counts the sequence section in bases)
        print("# %s: text %d bytes, %d reads, %d bases (packed stream %d bytes), archive %d bytes (made in %.1f s)" % (label, n_text, N, bases, (bases + 1) // 2, naf.numel(), time.time() - t0), flush=True)
        rows = torch.empty(40 * N, dtype=torch.uint8, device=dev)
        for qn, adapters in (("13 letters", [A13]), ("32 letters", [A32]), ("four adapters", FOUR)):
            clip = timed(ctx, label + " clip " + qn, lambda: ctx.unnaf_clip(naf, adapters, rate="0.1", min_overlap=3, min_len=30, out=rows),
                         ("unnaf_clip_stage", "unnaf_clip_mark", "unnaf_clip_finish", "unnaf_clip_copy"), bases)
            near = timed(ctx, label + " locate-near " + qn, lambda: ctx.unnaf_locate_near_count(naf, adapters, [len(a) // 10 for a in adapters], strands=1),
                         ("unnaf_locate_near_count",), bases)
            print("# %s, %s: clip_mark / locate_near_count = %.2f" % (label, qn, clip["unnaf_clip_mark"] / near["unnaf_locate_near_count"]), flush=True)
        timed(ctx, label + " clip 13 letters, totals only", lambda: ctx.unnaf_clip(naf, [A13], out=False), ("unnaf_clip_stage", "unnaf_clip_mark", "unnaf_clip_finish"), bases)
        _, tot, per = ctx.unnaf_clip(naf, FOUR, min_len=30, out=False)
        print("# %s, four adapters min 30: clipped %d of %d reads, kept %d, %d of %d bases" % (label, tot.clipped, tot.reads, tot.kept, tot.kept_bases, tot.bases), flush=True)
        del naf, rows
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
