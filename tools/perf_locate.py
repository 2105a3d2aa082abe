#!/usr/bin/env python3
"""What a motif search costs beside the decode it needs anyway: a synthetic repeat-masked genome (naf_amd/synth.py:
realistic_genome_device) is searched for NGG on both strands, GAATTC and a 32-mer taken from its own text, and naf_gpu_get_timing
gives (a) the two locate kernels, (b) the zstd decode of the same call, (c) a NAF_OUT_4BIT unnaf of the same archive -- the decode
alone, which a build without the search runs identically.  Prints the three, (a) / (c), and the bytes per second of the scan
(two passes over 0.5 B per base) against the 8 TB/s of HBM.   tools/perf_locate.py [bytes of FASTA]   (GPU box, repo root)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from naf_amd import capi, synth

size = int(float(sys.argv[1])) if len(sys.argv) > 1 else int(4e9)
ctx = capi.Context(0)
text = synth.realistic_genome_device(size, device="cuda")
ctx.reserve(int(text.numel() * 3.0) + (1 << 30))
d_naf, rep = ctx.ennaf(text)
d_naf = d_naf.clone()
del text
h = ctx.parse_header(d_naf)
n_bases, packed = int(h.orig_size[4]), (int(h.orig_size[4]) + 1) // 2
# a 32-mer of the text itself: 32 bases from the middle of the first record, upper case
lens, _ = ctx.unnaf_record_table(d_naf, 0, 1, capi.OUT_SEQUENCES)
mid = lens[0] // 2
mer = ctx.unnaf_select(d_naf, [(0, mid, mid + 32)], capi.OUT_SEQ, use_mask=False).cpu().numpy().tobytes().decode()
patterns = ["NGG", "GAATTC", mer]
print("box %s   FASTA %d B, %d records, %d bases (packed stream %d B, sequence frame %d B)" % (bench.box_id(), size, h.n_sequences, n_bases, packed, h.comp_size[4]))
print("patterns %s, both strands" % " ".join(patterns), flush=True)


def timed(call, repeat=3):
    """kernel times (naf_gpu_get_timing) and host time of the last of `repeat` calls"""
    for it in range(repeat):
        ctx.set_timing(it == repeat - 1)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    tm = ctx.get_timing()
    ctx.set_timing(False)
    return res, tm, dt * 1e3


(total, per), tm, ms_count = timed(lambda: ctx.unnaf_locate_count(d_naf, patterns, 3))
hit_buf = torch.empty(24 * total + 24, dtype=torch.uint8, device="cuda")
(_, total2), tm2, ms_locate = timed(lambda: ctx.unnaf_locate(d_naf, patterns, 3, out=hit_buf))
assert total2 == total
out4 = torch.empty(packed + 64, dtype=torch.uint8, device="cuda")
_, tm4, ms_4bit = timed(lambda: ctx.unnaf(d_naf, capi.OUT_4BIT, out=out4))


def split(tm):
    """(the locate kernels, every kernel of the call)"""
    return sum(ms for n, ms, k in tm if n.startswith("unnaf_locate")), sum(ms for n, ms, k in tm)


for name, t, ms in (("locate_count", tm, ms_count), ("locate", tm2, ms_locate), ("unnaf --4bit", tm4, ms_4bit)):
    print("%-13s host %8.3f ms   kernels: %s" % (name, ms, "  ".join("%s %.3f (%d)" % (n, x, k) for n, x, k in sorted(t, key=lambda x: -x[1])[:8])))
a_count, _ = split(tm)
a, all_loc = split(tm2)
c = sum(ms for n, ms, k in tm4)
print("hits %d   per pattern [forward, reverse] %s" % (total, per))
print("(a) locate kernels: count call %.3f ms, locate call %.3f ms (count + write)" % (a_count, a))
print("(b) the other kernels of the locate call -- the zstd decode of the stream, the record tables, the scan -- %.3f ms (all its kernels %.3f ms)" % (all_loc - a, all_loc))
print("(c) NAF_OUT_4BIT unnaf of the archive, all kernels %.3f ms" % c)
print("(a)/(c) %.3f   scan: %d B read twice in %.3f ms = %.1f GB/s, %.3f of the 8 TB/s roofline" % (a / c, packed, a, 2 * packed / a / 1e6, 2 * packed / a / 1e6 / 8000))
