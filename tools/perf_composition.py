#!/usr/bin/env python3
"""What the base composition costs beside the decode it needs anyway and beside a motif search of the same stream: a synthetic
repeat-masked genome (naf_amd/synth.py: realistic_genome_device, 4 GB of FASTA) at window 0, 100, 10 000 and 1 000 000, and a read set
(fastq_reads_device, 12.5 GB of FASTQ) at window 0.  3 warm-up calls, then the median of 10: host time of the call and the kernel times
of naf_gpu_get_timing.  The yardsticks, from the same run on the same box: (a) every kernel of a NAF_OUT_4BIT unnaf of the archive -- the
decode alone --, (b) one counting sweep of naf_gpu_unnaf_locate_count with NGG, GAATTC and a 32-mer of the text.
tools/perf_composition.py [bytes of FASTA] [bytes of FASTQ] > profiles/composition_perf.txt   (GPU box, repo root; 0 skips a data set)"""
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


def line(name, host, kern, mine="unnaf_comp"):
    own = sum(ms for n, ms in kern.items() if n.startswith(mine))
    top = "  ".join("%s %.3f" % (n, ms) for n, ms in sorted(kern.items(), key=lambda x: -x[1])[:7])
    print("%-28s host %9.3f ms   its kernels %9.3f ms   all kernels %9.3f ms   %s" % (name, host, own, sum(kern.values()), top), flush=True)
    return own


def measure(title, text, windows, fmt_note):
    ctx.reserve(int(text.numel() * 3.0) + (1 << 30))
    d_naf, rep = ctx.ennaf(text)
    d_naf = d_naf.clone()
    del text
    torch.cuda.empty_cache()
    h = ctx.parse_header(d_naf)
    n_bases, packed = int(h.orig_size[4]), (int(h.orig_size[4]) + 1) // 2
    print("\n== %s: %d records, %d bases (packed stream %d B, sequence frame %d B)%s" % (title, h.n_sequences, n_bases, packed, h.comp_size[4], fmt_note), flush=True)
    out4 = torch.empty(packed + 64, dtype=torch.uint8, device="cuda")
    _, host, kern = timed(lambda: ctx.unnaf(d_naf, capi.OUT_4BIT, out=out4))
    a = line("(a) unnaf --4bit", host, kern, "")
    del out4
    lens, _ = ctx.unnaf_record_table(d_naf, 0, 1, capi.OUT_SEQUENCES)
    mid = lens[0] // 2
    mer = ctx.unnaf_select(d_naf, [(0, mid, mid + min(32, lens[0] - mid))], capi.OUT_SEQ, use_mask=False).cpu().numpy().tobytes().decode()
    pats = ["NGG", "GAATTC", mer]
    (hits, _), host, kern = timed(lambda: ctx.unnaf_locate_count(d_naf, pats, 3))
    b = line("(b) locate_count %s" % " ".join(pats[:2] + ["%d-mer" % len(mer)]), host, kern, "unnaf_locate")
    for w in windows:
        for mask in (True, False):
            n = ctx.unnaf_composition_rows(d_naf, w)
            buf = torch.empty(168 * n + 168, dtype=torch.uint8, device="cuda")
            (_, tot), host, kern = timed(lambda: ctx.unnaf_composition(d_naf, w, mask, out=buf))
            own = line("composition window %d mask %d" % (w, mask), host, kern)
            acgt = tot.n[8] + tot.n[4] + tot.n[2] + tot.n[1]
            print("    rows %d (%.1f MB)   bases %d  N %d  masked %d  CpG %d  GC %.4f   count kernel %.3f ms = %.1f GB/s of packed bytes   its kernels / (a) %.2f   / (b) %.2f" % (
                n, 168 * n / 1e6, tot.end, tot.n[15], tot.masked, tot.cpg, (tot.n[4] + tot.n[2]) / max(acgt, 1), kern.get("unnaf_comp_count", 0.0),
                packed / max(kern.get("unnaf_comp_count", 0.0), 1e-9) / 1e6, own / max(a, 1e-9), own / max(b, 1e-9)), flush=True)
            del buf
    del d_naf
    torch.cuda.empty_cache()
    ctx.release_scratch()


print("box %s   %d warm-up calls, median of %d" % (bench.box_id(), WARM, TAKE))
if genome_bytes:
    measure("repeat-masked genome, %d B of FASTA" % genome_bytes, synth.realistic_genome_device(genome_bytes, device="cuda"), (0, 100, 10000, 1000000), "")
if reads_bytes:
    measure("read set, %d B of FASTQ" % reads_bytes, synth.fastq_reads_device(reads_bytes, device="cuda"), (0,), "")
