#!/usr/bin/env python3
"""What the table of open reading frames costs beside the decode it needs anyway, beside a composition sweep of the same stream and beside
the nearest thing there was before it: a synthetic repeat-masked genome (naf_amd/synth.py: realistic_genome_device; 2 GB of FASTA, so
that its bases are fewer than 2^31 -- one piece, and a call has exactly the two mark passes whose rate is printed) asked for its ORFs at
the command line's defaults (TAA,TAG,TGA / ATG, 75 bases, both strands), from stop to stop at 3 bases (the densest table) and at 300 bases.  3 warm-up calls, then the median of 10: host time of the call and the kernel times of naf_gpu_get_timing.  The
yardsticks, from the same run on the same box: (a) every kernel of a NAF_OUT_4BIT unnaf of the archive -- the decode alone --, (b)
naf_gpu_unnaf_composition at window 0, mask off -- one sweep over the same packed bytes --, (c) naf_gpu_unnaf_locate of TAA, TAG and TGA
on both strands -- unpaired hits, no frames, no ORFs.
tools/perf_orfs.py [bytes of FASTA] > profiles/orfs_perf.txt   (GPU box, repo root)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from naf_amd import capi, synth

WARM, TAKE = 3, 10
genome_bytes = int(float(sys.argv[1])) if len(sys.argv) > 1 else int(2e9)
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


def line(name, host, kern, mine="unnaf_orfs"):
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
print("\n== repeat-masked genome, %d B of FASTA: %d records, %d bases (packed stream %d B, sequence frame %d B)" % (
    genome_bytes, h.n_sequences, n_bases, packed, h.comp_size[4]), flush=True)
out4 = torch.empty(packed + 64, dtype=torch.uint8, device="cuda")
_, host, kern = timed(lambda: ctx.unnaf(d_naf, capi.OUT_4BIT, out=out4))
a = line("(a) unnaf --4bit", host, kern, "")
del out4
n = ctx.unnaf_composition_rows(d_naf, 0)
buf = torch.empty(168 * n + 168, dtype=torch.uint8, device="cuda")
_, host, kern = timed(lambda: ctx.unnaf_composition(d_naf, 0, False, out=buf))
b = line("(b) composition window 0", host, kern, "unnaf_comp")
del buf
stops = ["TAA", "TAG", "TGA"]
n, _ = ctx.unnaf_locate_count(d_naf, stops, 3)
buf = torch.empty(24 * n + 24, dtype=torch.uint8, device="cuda")
_, host, kern = timed(lambda: ctx.unnaf_locate(d_naf, stops, 3, out=buf))
c = line("(c) locate TAA TAG TGA both", host, kern, "unnaf_loc")
print("    hits %d (%.1f MB of rows)" % (n, 24 * n / 1e6), flush=True)
del buf
torch.cuda.empty_cache()
for name, starts, min_len in (("orfs defaults (ATG, min 75)", "ATG", 75), ("orfs stop-to-stop min 3", None, 3), ("orfs ATG min 300", "ATG", 300)):
    n, nb, pf = ctx.unnaf_orfs_count(d_naf, "TAA,TAG,TGA", starts, min_len)
    buf = torch.empty(32 * n + 32, dtype=torch.uint8, device="cuda")
    _, host, kern = timed(lambda: ctx.unnaf_orfs(d_naf, "TAA,TAG,TGA", starts, min_len, out=buf))
    own = line(name, host, kern)
    mark = kern.get("unnaf_orfs_count", 0.0) + kern.get("unnaf_orfs_write", 0.0)
    print("    orfs %d (%.1f MB of rows)   bases in orfs %d   per strand and frame %s   the two mark passes %.3f ms = %.1f GB/s of packed bytes each   "
          "its kernels / (a) %.2f   / (b) %.2f   / (c) %.2f" % (n, 32 * n / 1e6, nb, pf, mark, 2 * packed / max(mark, 1e-9) / 1e6 if mark else 0.0,
                                                              own / max(a, 1e-9), own / max(b, 1e-9), own / max(c, 1e-9)), flush=True)
    del buf
    torch.cuda.empty_cache()
