#!/usr/bin/env python3
"""Kernel times of naf_gpu_unnaf_screen beside its yardstick, k_clip_mark with one adapter of 13 letters, which reads the same packed bytes
once with the same record walk, on the same archive in the same process (profiles/screen_perf.txt is this script's output on one MI355X;
DESIGN.md section 8r reads it).

    python tools/perf_screen.py [--reads-bytes N] [--reps N]

The reads are the benchmark's synthetic FASTQ (150-base reads, 12.5 GB by default: the FASTQ leg's size); the references are uniform
random ACGT of 5 kb (a spike-in: the prefilter's bitmap is nearly empty) and of 5 Mb (a bacterial genome: more keys than the bitmap has
bits, so it is full and every position probes the table).  The reads share no 27-mer with either, which is the case the kernel is built
for: a clean read set.  K = 27 and 31; the prefilter as the call chooses (no lever: 2^18 bits, none when the set has more than half as many
keys as that), forced to 2^18 bits (NAF_GPU_SCREEN_FILTER_BITS=262144) and switched off (=0).  Every call is
made once to warm up and then --reps times (default 5) with kernel timing on (HIP events around each launch, naf_gpu_get_timing); a
line gives the least and the median of the sums over a call's launches and the spread (largest - least) / least."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from naf_amd import capi, synth  # noqa: E402

A13 = "AGATCGGAAGAGC"
KERNELS = ("unnaf_screen_insert", "unnaf_screen_stage", "unnaf_screen_mark", "unnaf_screen_finish", "unnaf_row_copy")


def random_reference(n, dev, seed, line=100):
    """FASTA of one record of n uniform ACGT (n: whole lines)"""
    assert n % line == 0
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    m = torch.full((n // line, line + 1), 10, dtype=torch.uint8, device=dev)
    m[:, :line] = lut[torch.randint(0, 4, (n // line, line), dtype=torch.int64, device=dev, generator=g)]
    head = torch.tensor(list(b">reference %d\n" % n), dtype=torch.uint8, device=dev)
    return torch.cat([head, m.reshape(-1)])


def timed(ctx, label, fn, names, bases, reps):
    """per kernel name the sums over a call's launches in `reps` calls, sorted; prints least, median and spread"""
    fn()
    seen = {}
    for _ in range(reps):
        ctx.set_timing(True)
        ctx.synchronize()
        fn()
        ctx.synchronize()
        t = {n: (ms, k) for n, ms, k in ctx.get_timing()}
        ctx.set_timing(False)
        for n in names:
            if n in t:
                seen.setdefault(n, []).append(t[n])
    out = {}
    for n in names:
        if n in seen:
            ms = sorted(v[0] for v in seen[n])
            out[n] = ms
            print("%-44s %-22s least %9.3f ms  median %9.3f ms  spread %5.1f %%  %3d launches  %8.1f Gbases/s" % (label, n, ms[0], ms[len(ms) // 2], 100 * (ms[-1] - ms[0]) / ms[0], seen[n][0][1],
                                                                                                             bases / ms[0] / 1e6), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads-bytes", type=float, default=12.5e9)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda"
    ctx = capi.Context(0)
    print("# %s, %s" % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d")), flush=True)
    t0 = time.time()
    text = synth.fastq_reads_device(int(args.reads_bytes), seed=7, device=dev)
    naf, _ = ctx.ennaf(text)
    naf = naf.clone()
    n_text = text.numel()
    del text
    torch.cuda.empty_cache()
    h = ctx.parse_header(naf)
    bases, N = int(h.orig_size[4]), int(h.n_sequences)                                  # (the header counts the sequence section in bases)
    print("# reads: text %d bytes, %d reads, %d bases (packed stream %d bytes), archive %d bytes (made in %.1f s)" % (n_text, N, bases, (bases + 1) // 2, naf.numel(), time.time() - t0), flush=True)
    crows = torch.empty(40 * N, dtype=torch.uint8, device=dev)
    clip = timed(ctx, "clip 13 letters", lambda: ctx.unnaf_clip(naf, [A13], rate="0.1", min_overlap=3, min_len=30, out=crows), ("unnaf_clip_mark",), bases, args.reps)["unnaf_clip_mark"]
    del crows
    rows = torch.empty(40 * N, dtype=torch.uint8, device=dev)
    for ref_bases in (5000, 5000000):
        ref, _ = ctx.ennaf(random_reference(ref_bases, dev, 23))
        ref = ref.clone()
        for K in (27, 31):
            got = {}
            for fbits in (None, 1 << 18, 0):
                if fbits is None:
                    os.environ.pop("NAF_GPU_SCREEN_FILTER_BITS", None)
                else:
                    os.environ["NAF_GPU_SCREEN_FILTER_BITS"] = str(fbits)
                tag = "ref %d k %d prefilter %s" % (ref_bases, K, "default" if fbits is None else "2^18 bits" if fbits else "off")
                got[fbits] = timed(ctx, tag, lambda: ctx.unnaf_screen(naf, ref, k=K, out=rows), KERNELS, bases, args.reps)["unnaf_screen_mark"]
                os.environ["NAF_GPU_TRACE"] = "1"
                _, tot = ctx.unnaf_screen(naf, ref, k=K, out=False)                      # (its trace line goes to stderr: filtered and probed)
                os.environ.pop("NAF_GPU_TRACE")
                print("# %s: mark / clip_mark = %.2f (least), %.2f (median); %d reads, %d matched, %d of %d k-mers hit; reference %d positions, %d keys" % (
                    tag, got[fbits][0] / clip[0], got[fbits][len(got[fbits]) // 2] / clip[len(clip) // 2], tot.reads, tot.matched, tot.hit_kmers, tot.kmers, tot.ref_positions, tot.ref_kmers), flush=True)
            os.environ.pop("NAF_GPU_SCREEN_FILTER_BITS", None)
            on, off, dflt = got[1 << 18], got[0], got[None]
            print("# ref %d k %d: prefilter off / 2^18 bits = %.2f (least), %.2f (median); spread with it %.1f %%, without %.1f %%; off / default = %.2f (least)" % (
                ref_bases, K, off[0] / on[0], off[len(off) // 2] / on[len(on) // 2], 100 * (on[-1] - on[0]) / on[0], 100 * (off[-1] - off[0]) / off[0], off[0] / dflt[0]), flush=True)
        del ref
    ctx.close()


if __name__ == "__main__":
    main()
