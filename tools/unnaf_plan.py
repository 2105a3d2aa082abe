#!/usr/bin/env python3
"""The launch plan of the unnaf text driver (emit.hip: unnaf_run, unnaf_sections) on the smallest archive that takes each of its
branches: per case the kernels with their launch counts, which of the five streams ran anything, the trace text and the SHA-256 of
the output.  Two builds that claim the same driver print the same text: tools/unnaf_plan.py > a.txt, then once more with
NAF_GPU_LIB=<the other libnaf_gpu.so> (run on the GPU box from the repo root, a fresh process each; profiles/unnaf_driver_plan.txt).
tools/perf_unnaf_driver.py times the same cases."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from naf_amd import capi, synth

FASTA, FASTQ, SEQ, SEQUENCES, FOURBIT = capi.OUT_FASTA, capi.OUT_FASTQ, capi.OUT_SEQ, capi.OUT_SEQUENCES, capi.OUT_4BIT
SWITCHES = [("EMIT", "span"), ("EMIT", "short"), ("EMIT", "long"), ("EMIT_WAVE", "0"), ("FORCE_SLOW", "1"), ("FUSE", "1"), ("FLAT_FUSE", "0"),
            ("SIDE_FUSED", "0"), ("SPLIT", "0"), ("SPLIT", "2"), ("MASK_RLE", "0")]


def archives(ctx):
    """name -> (archive on the device, its default mode, switches the archive needs to take its branch)."""
    from oracle import oracle as O
    from test_gpu_decode import _mostly_flat_fasta
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def own(text):
        return ctx.ennaf(ctx.to_device(text))[0].clone()

    a = {}
    one = acgt[rng.integers(0, 4, 65536)]
    a["decoded_64k"] = (own(b">one record\n" + synth.wrap_lines(one, 60)), FASTA, {})               # a one-block frame is decoded: the tile kernels over a decoded stream
    # uniform ACGT, every block one flat 4-bit tree: read in place from SPEC_MIN blocks up (512; lowered as the tests lower it) -- the flat emit
    flat = acgt[rng.integers(0, 4, 2 << 20)]
    a["flat_2m"] = (own(b">one record\n" + synth.wrap_lines(flat, 60)), FASTA, {"SPEC_MIN": "8"})    # two tiles a wavefront
    low = flat.copy()
    for p in range(0, len(low), 1500):                                                            # a toggle per tile or more: one tile a wavefront
        low[p:p + 700] |= 0x20
    a["flat_2m_toggles"] = (own(b">one record\n" + synth.wrap_lines(low, 60)), FASTA, {"SPEC_MIN": "8"})
    a["mostly_flat"] = (own(_mostly_flat_fasta(np.random.default_rng(15), 2_400_011, 0.01, width=61, n_rec=3)), FASTA, {"SPEC_MIN": "8"})
    # Huffman literals only.  The split decode -> emit pipeline needs 256 blocks a part (zstd_dec.hip: 16 workgroups of HUF_BLOCKS_PER_WG) whatever
    # SPLIT_MIN says: 72 Mi bases are the 1024 blocks of the default four parts, and a 4 MiB genome never splits
    skew = acgt[rng.choice(4, 4 << 20, p=[0.4, 0.1, 0.1, 0.4])]
    a["skewed_4m"] = (own(b">skewed\n" + synth.wrap_lines(skew, 60)), FASTA, {"SPLIT_MIN": "32"})
    skew = acgt[rng.choice(4, 72 << 20, p=[0.4, 0.1, 0.1, 0.4]).astype(np.uint8)]
    a["skewed_72m"] = (own(b">skewed\n" + synth.wrap_lines(skew, 60)), FASTA, {"SPLIT_MIN": "32"})
    del skew
    for n, ln in ((1000, 150), (130, 300), (33, 700)):                                            # 4, 8 and 16 lanes a read
        a["fastq_%d" % ln] = (ctx.to_device(O.ennaf(synth.fastq_reads(n, ln, seed=n + ln, var_len=ln == 150))), FASTQ, {})
    a["short_many"] = (own(synth.fasta_mixed(4000, 300, 60, seed=102, empty_every=7)), FASTA, {})
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacdxX*", dtype=np.uint8)
    prot = b"".join(b">p%d some protein\n" % k + synth.wrap_lines(aa[rng.integers(0, len(aa), int(rng.integers(1, 600)))], 60) for k in range(400))
    a["protein"] = (ctx.to_device(O.ennaf(prot, O.PROTEIN)), FASTA, {})
    # a control byte inside an id puts a base into the stream that no length accounts for: bases behind the last record
    sur = b">big\x01\x02 c\n" + synth.wrap_lines(acgt[rng.integers(0, 4, 60_000)], 60) + b">third" + b"\x01" * 130 + b" x\n" + synth.wrap_lines(acgt[rng.integers(0, 4, 7)], 60)
    a["surplus"] = (ctx.to_device(O.ennaf(sur)), FASTA, {})
    a["ids_names_1m"] = (own(synth.fastq_reads(200_000, 100, seed=5, var_len=True)), FASTQ, {})       # names on a context of their own
    return a


def cases(ctx, with_switches=True):
    """(name, archive, env, what, mode, line_length, range or None); what: "whole", "size", "range"."""
    arcs = archives(ctx)
    out = []
    for name, (d, mode, env) in arcs.items():
        dna = name not in ("protein",)
        out.append((name, d, env, "whole", mode, -1, None))
        if name == "ids_names_1m":
            if with_switches:
                out.append((name + " NAMES_BESIDE=0", d, dict(env, NAMES_BESIDE="0"), "whole", mode, -1, None))
            continue
        for ll in (0, 13, 60):
            out.append(("%s fasta ll=%d" % (name, ll), d, env, "whole", FASTA, ll, None))
        for m, mn in ((SEQ, "seq"), (SEQUENCES, "sequences")) + (((FOURBIT, "4bit"),) if dna else ()):
            out.append(("%s %s" % (name, mn), d, env, "whole", m, -1, None))
        out.append((name + " size", d, env, "size", mode, -1, None))
    if with_switches:
        for name in ("decoded_64k", "flat_2m", "flat_2m_toggles", "mostly_flat", "skewed_72m", "fastq_150", "short_many"):
            d, mode, env = arcs[name]
            for k, v in SWITCHES:
                out.append(("%s %s=%s" % (name, k, v), d, dict(env, **{k: v}), "whole", mode, -1, None))
    for name in ("flat_2m", "short_many", "fastq_150"):
        d, mode, env = arcs[name]
        n = ctx.unnaf_size(d, mode)
        for k in range(8):
            out.append(("%s range %d/8" % (name, k), d, env, "range", mode, -1, (n * k // 8, n * (k + 1) // 8)))
    d, mode, env = arcs["surplus"]
    n = ctx.unnaf_size(d, mode)
    out.append(("surplus range in the tail", d, env, "range", mode, -1, (n - 20, n - 3)))
    return out


class Env:
    """NAF_GPU_<k> = v for the calls inside."""
    def __init__(self, env):
        self.env = {"NAF_GPU_" + k: v for k, v in env.items()}

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k in self.env:
            os.environ.pop(k, None)


def run(ctx, case, out):
    name, d, env, what, mode, ll, rng = case
    if what == "size":
        return ctx.unnaf_size(d, mode, line_length=ll)
    if what == "range":
        return ctx.unnaf_range(d, rng[0], rng[1], mode, line_length=ll, out=out)
    return ctx.unnaf(d, mode, line_length=ll, out=out)


def main():
    import torch
    ctx = capi.Context(0)
    lib = capi.load()
    cs = cases(ctx)
    out = torch.empty(96 << 20, dtype=torch.uint8, device=ctx.device)
    for case in cs:
        with Env(case[2]):
            try:
                run(ctx, case, out)                                   # (arenas grown, side contexts made: not part of the plan)
                ctx.set_option("TRACE", "1"); lib.naf_gpu_clear_trace(ctx.h)
                ctx.set_timing(True)
                r = run(ctx, case, out)
                kernels = sorted((n, k) for n, ms, k in ctx.get_timing())
                streams = "".join("x" if ms > 0 else "." for ms in ctx.get_timing_streams())
                ctx.set_timing(False)
                trace = (lib.naf_gpu_get_trace(ctx.h) or b"").decode("latin1")
                ctx.set_option("TRACE", None); lib.naf_gpu_clear_trace(ctx.h)
                res = "size %d" % r if case[3] == "size" else "%d bytes sha256 %s" % (r.numel(), hashlib.sha256(r.cpu().numpy().tobytes()).hexdigest())
            except capi.NafGpuError as e:
                ctx.set_timing(False); ctx.set_option("TRACE", None)
                kernels, streams, trace, res = [], "", "", "error %d %s" % (e.code, e.msg.strip())
        print("== %s" % case[0])
        print("   streams %s  %s" % (streams, res))
        print("   " + " ".join("%s x%d" % nk for nk in kernels))
        for line in sorted(trace.splitlines()):                       # (sorted: the lines of the host threads come in any order)
            print("   | " + line)
    ctx.close()


if __name__ == "__main__":
    main()
