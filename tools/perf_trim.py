#!/usr/bin/env python3
"""Kernel times of naf_gpu_unnaf_trim beside its yardstick, naf_gpu_unnaf_quality's count kernel, on the same archive in the same process
(profiles/trim_perf.txt is this script's output on one MI355X; DESIGN.md section 8o reads it).

    python tools/perf_trim.py [--short-bytes N] [--long-bytes N]

Two texts: the benchmark's synthetic FASTQ (150-base reads, quality uniform Phred 0-40, 12.5 GB by default: the FASTQ leg's size) and reads
of 20 000 bases (2000 distinct reads, repeated to the size asked for).  Every call is made once to warm up and then three times with kernel
timing on (HIP events around each launch, naf_gpu_get_timing); a line is the least of the three sums over a call's launches -- one launch
a piece of 2^31 quality bytes."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from naf_amd import capi, synth  # noqa: E402


def long_reads(total, dev, read_len=20000, distinct=2000, seed=5):
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(distinct):
        parts += [b"@long%d\n" % k, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, read_len)].tobytes(), b"\n+\n",
                  rng.integers(33, 74, read_len, dtype=np.uint8).tobytes(), b"\n"]
    block = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).to(dev)
    return block.repeat(max(1, total // block.numel()))


def timed(ctx, label, fn, names, qbytes, reps=3):
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
            print("%-42s %-18s %9.3f ms  %3d launches  %8.1f GB/s of quality bytes" % (label, n, best[n][0], best[n][1], qbytes / best[n][0] / 1e6), flush=True)


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
        q, N = int(h.orig_size[5]), int(h.n_sequences)
        print("# %s: text %d bytes, %d reads, quality stream %d bytes, archive %d bytes (made in %.1f s)" % (label, n_text, N, q, naf.numel(), time.time() - t0), flush=True)
        rows = torch.empty(40 * N, dtype=torch.uint8, device=dev)
        qrows = torch.empty(56 * N, dtype=torch.uint8, device=dev)
        for qn, lim in (("Q20", capi.trim_limit(20)), ("Q2", capi.trim_limit(2)), ("none", capi.TRIM_NONE)):
            timed(ctx, label + " trim " + qn + " min 30 max-ee 1", lambda: ctx.unnaf_trim(naf, lim, 30, capi.ee_units("1"), out=rows), ("unnaf_trim_mark", "unnaf_trim_join", "unnaf_row_copy"), q)
        timed(ctx, label + " trim Q20, totals only", lambda: ctx.unnaf_trim(naf, capi.trim_limit(20), out=False), ("unnaf_trim_mark", "unnaf_trim_join"), q)
        timed(ctx, label + " quality, record rows", lambda: ctx.unnaf_quality(naf, 0, out_records=qrows), ("unnaf_qual_count", "unnaf_qual_rows", "unnaf_row_copy"), q)
        _, tot = ctx.unnaf_trim(naf, capi.trim_limit(20), 30, capi.ee_units("1"), out=False)
        print("# %s, Q20 min 30 max-ee 1: kept %d of %d reads, %d of %d bases" % (label, tot.kept, tot.reads, tot.kept_bases, tot.bases), flush=True)
        del naf, rows, qrows
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
