#!/usr/bin/env python3
"""What the k-mer counts cost beside the decode they need anyway and beside a composition sweep of the same stream: a synthetic repeat-masked
genome (naf_amd/synth.py: realistic_genome_device, 4 GB of FASTA) counted as one table at K = 4, 6, 7, 8 and 12, plain and canonical, and
per record at K = 4; a synthetic read set (fastq_reads_device, 12.5 GB of FASTQ) as one table at K = 6 and 10.  K = 7 is counted with both
LDS limits (NAF_GPU_KMERS_LDS_K = 6: global atomics, 7: 64 KiB of bins), K = 2 and 3 show the bins of the small K.  3 warm-up calls, then
the median of 10: host time of the call and the kernel times of naf_gpu_get_timing.  The yardsticks, from the same run on the same box:
(a) every kernel of a NAF_OUT_4BIT unnaf of the archive -- the decode alone --, (b) naf_gpu_unnaf_composition at window 0, mask off --
one sweep over the same packed bytes.
tools/perf_kmers.py [bytes of FASTA] [bytes of FASTQ] > profiles/kmers_perf.txt   (GPU box, repo root)"""
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


def line(name, host, kern, mine="unnaf_kmer"):
    own = sum(ms for n, ms in kern.items() if n.startswith(mine))
    top = "  ".join("%s %.3f" % (n, ms) for n, ms in sorted(kern.items(), key=lambda x: -x[1])[:6])
    print("%-34s host %9.3f ms   its kernels %9.3f ms   all kernels %9.3f ms   %s" % (name, host, own, sum(kern.values()), top), flush=True)
    return own


def archive(text):
    ctx.reserve(int(text.numel() * 3.0) + (1 << 30))
    d_naf, rep = ctx.ennaf(text)
    return d_naf.clone()


def measure(title, d_naf, queries):
    h = ctx.parse_header(d_naf)
    n_bases, packed = int(h.orig_size[4]), (int(h.orig_size[4]) + 1) // 2
    print("\n== %s: %d records, %d bases (packed stream %d B, sequence frame %d B)" % (title, h.n_sequences, n_bases, packed, h.comp_size[4]), flush=True)
    out4 = torch.empty(packed + 64, dtype=torch.uint8, device="cuda")
    _, host, kern = timed(lambda: ctx.unnaf(d_naf, capi.OUT_4BIT, out=out4))
    a = line("(a) unnaf --4bit", host, kern, "")
    del out4
    n = ctx.unnaf_composition_rows(d_naf, 0)
    buf = torch.empty(168 * n + 168, dtype=torch.uint8, device="cuda")
    _, host, kern = timed(lambda: ctx.unnaf_composition(d_naf, 0, False, out=buf))
    b = line("(b) composition window 0", host, kern, "unnaf_comp")
    del buf
    for k, canonical, per, lds_k in queries:
        if lds_k is None:
            os.environ.pop("NAF_GPU_KMERS_LDS_K", None)
        else:
            os.environ["NAF_GPU_KMERS_LDS_K"] = str(lds_k)
        n_rows, n_counters = ctx.unnaf_kmers_rows(d_naf, k, canonical, per)
        out = torch.empty(n_counters + 8, dtype=torch.int64, device="cuda")
        rows = torch.empty(40 * n_rows + 40, dtype=torch.uint8, device="cuda") if per else None
        (counts, _, tot), host, kern = timed(lambda: ctx.unnaf_kmers(d_naf, k, canonical, per, out=out, out_rows=rows))
        name = "kmers K %d%s%s%s" % (k, " canonical" if canonical else "", " per record" if per else "", "" if lds_k is None else " LDS_K=%d" % lds_k)
        own = line(name, host, kern)
        count = kern.get("unnaf_kmer_count", 0.0)
        print("    tables %d   counted %d of %d positions   count kernel %.3f ms = %.1f GB/s of packed bytes, %.2f G k-mers/s   its kernels / (a) %.2f   / (b) %.2f" % (
            n_rows, tot.counted, tot.positions, count, packed / max(count, 1e-9) / 1e6, tot.counted / max(count, 1e-9) / 1e6, own / max(a, 1e-9), own / max(b, 1e-9)), flush=True)
        assert int(counts.sum()) == tot.counted
        del out, rows, counts
    os.environ.pop("NAF_GPU_KMERS_LDS_K", None)


print("box %s   %d warm-up calls, median of %d" % (bench.box_id(), WARM, TAKE))
if genome_bytes:
    text = synth.realistic_genome_device(genome_bytes, device="cuda")
    d_naf = archive(text)
    del text
    torch.cuda.empty_cache()
    measure("repeat-masked genome, %d B of FASTA" % genome_bytes, d_naf,
            [(4, False, False, None), (4, True, False, None), (6, False, False, None), (6, True, False, None), (7, False, False, 6), (7, True, False, 6), (7, False, False, 7),
             (7, True, False, 7), (8, False, False, None), (8, True, False, None), (12, False, False, None), (12, True, False, None), (4, False, True, None),
             (2, False, False, None), (3, False, False, None), (3, False, False, 0), (6, False, False, 0)])
    del d_naf
    torch.cuda.empty_cache()
if reads_bytes:
    text = synth.fastq_reads_device(reads_bytes, device="cuda")
    d_naf = archive(text)
    del text
    torch.cuda.empty_cache()
    measure("read set, %d B of FASTQ" % reads_bytes, d_naf, [(6, False, False, None), (6, True, False, None), (10, False, False, None), (10, True, False, None)])
