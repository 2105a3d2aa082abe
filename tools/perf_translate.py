#!/usr/bin/env python3
"""What the translation costs beside the selection of the same segments -- the call its users had to make before it, which decodes the
same blocks, reads the same bases and writes three times the bytes: the synthetic repeat-masked genome of tools/perf_orfs.py (2 GB of
FASTA) asked for (1) the proteins of its ORF rows at the command line's defaults (TAA,TAG,TGA / ATG, 75 bases, both strands) and (2) the
six frames of its whole records.  3 warm-up calls, then the median of 10: host time of the call and the kernel times of
naf_gpu_get_timing (HIP events).  Per question: naf_gpu_unnaf_select_stranded (FASTA, mask off, lines of 60) and naf_gpu_unnaf_translate
(code 1, lines of 60) of the same segments, the emit kernel of each alone, and the rate of that kernel in bases read and in bytes written.
tools/perf_translate.py [bytes of FASTA] [--select-only] > profiles/translate_perf.txt   (GPU box, repo root)
--select-only: the yardstick alone, for a build of the library from before the translation (the same segments, made the same way)."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from naf_amd import capi, synth

WARM, TAKE = 3, 10
SELECT_ONLY = "--select-only" in sys.argv
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
genome_bytes = int(float(ARGS[0])) if ARGS else int(2e9)
ctx = capi.Context(0)
SEG = np.dtype([("record", "<u8"), ("begin", "<u8"), ("end", "<u8")])


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


def line(name, host, kern, mine, bases, written):
    own = sum(ms for n, ms in kern.items() if n.startswith(mine))
    top = "  ".join("%s %.3f" % (n, ms) for n, ms in sorted(kern.items(), key=lambda x: -x[1])[:6])
    print("%-30s host %9.3f ms   emit kernel %8.3f ms = %7.1f Gbases/s read, %7.1f GB/s written   all kernels %9.3f ms   %s" % (
        name, host, own, bases / max(own, 1e-9) / 1e6, written / max(own, 1e-9) / 1e6, sum(kern.values()), top), flush=True)
    return own


def ask(name, segs, strand, bases):
    """both calls on the same host arrays of segments (numpy: a Python list of millions of tuples is no measurement)"""
    n_segs = len(segs)
    ps, pt = segs.ctypes.data_as(C.POINTER(capi.Segment)), strand.ctypes.data_as(C.POINTER(C.c_uint8))
    o = capi.UnnafOpts(capi.OUT_FASTA, 0, 60)
    g = None if SELECT_ONLY else capi.genetic_code(1)
    need_s, need_t = C.c_size_t(), C.c_size_t()
    ctx._check(ctx.L.naf_gpu_unnaf_select_stranded_size(ctx.h, capi._ptr(d_naf), d_naf.numel(), C.byref(o), ps, pt, n_segs, C.byref(need_s)))
    if not SELECT_ONLY:
        ctx._check(ctx.L.naf_gpu_unnaf_translate_size(ctx.h, capi._ptr(d_naf), d_naf.numel(), C.byref(o), C.byref(g), ps, pt, n_segs, C.byref(need_t)))
    buf = torch.empty(need_s.value + 64, dtype=torch.uint8, device="cuda")
    got = C.c_size_t()
    print("\n-- %s: %d segments, %d bases (%d B of packed stream); selection %d B of text, translation %d B" % (name, n_segs, bases, bases // 2, need_s.value, need_t.value), flush=True)

    def select():
        ctx._check(ctx.L.naf_gpu_unnaf_select_stranded(ctx.h, capi._ptr(d_naf), d_naf.numel(), C.byref(o), ps, pt, n_segs, capi._ptr(buf), buf.numel(), C.byref(got)))

    def translate():
        ctx._check(ctx.L.naf_gpu_unnaf_translate(ctx.h, capi._ptr(d_naf), d_naf.numel(), C.byref(o), C.byref(g), ps, pt, n_segs, capi._ptr(buf), buf.numel(), C.byref(got)))

    _, host, kern = timed(select)
    a = line("select_stranded (yardstick)", host, kern, "unnaf_emit_select", bases, need_s.value)
    host_a = host
    if SELECT_ONLY:
        return
    _, host, kern = timed(translate)
    b = line("translate", host, kern, "unnaf_emit_translate", bases, need_t.value)
    print("   translate / select: emit kernel %.2f   host time of the call %.2f" % (b / max(a, 1e-9), host / max(host_a, 1e-9)), flush=True)
    del buf
    torch.cuda.empty_cache()


print("box %s   %d warm-up calls, median of %d" % (bench.box_id(), WARM, TAKE))
text = synth.realistic_genome_device(genome_bytes, device="cuda")
ctx.reserve(int(text.numel() * 3.0) + (1 << 30))
d_naf, rep = ctx.ennaf(text)
d_naf = d_naf.clone()
del text
torch.cuda.empty_cache()
h = ctx.parse_header(d_naf)
print("\n== repeat-masked genome, %d B of FASTA: %d records, %d bases (packed stream %d B, sequence frame %d B)" % (
    genome_bytes, h.n_sequences, int(h.orig_size[4]), (int(h.orig_size[4]) + 1) // 2, h.comp_size[4]), flush=True)

rows, nb = ctx.unnaf_orfs(d_naf)                                                     # the command line's defaults
segs = np.zeros(len(rows), dtype=SEG)
segs["record"], segs["begin"], segs["end"] = rows["record"], rows["begin"], rows["end"]
ask("ORF rows at the defaults", segs, np.ascontiguousarray(rows["strand"].astype(np.uint8)), int(nb))
del rows, segs

lengths, _ = ctx.unnaf_record_table(d_naf, out_type=capi.OUT_FASTA)
six = [seg for r, n in enumerate(lengths) for seg in ((r, 0, capi.WHOLE, 0), (r, 1, n, 0), (r, 2, n, 0), (r, 0, capi.WHOLE, 1), (r, 0, n - 1, 1), (r, 0, n - 2, 1))]   # (every record has three bases: capi.frames_to_segments)
segs = np.array([x[:3] for x in six], dtype=np.uint64).view(SEG).reshape(-1)
strand = np.array([x[3] for x in six], dtype=np.uint8)
bases = sum((min(e, lengths[r]) - b) for r, b, e, _ in six)
ask("six frames of every record", segs, strand, int(bases))
