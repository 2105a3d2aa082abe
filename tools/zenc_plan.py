#!/usr/bin/env python3
"""The launch plan of the zstd encoder's frame driver (zstd_enc.hip: zstd_encode_begin, zenc_finish) on the
smallest inputs that take each of its branches: one line per case with the launches of the call and their counts (Context.get_timing)
and the SHA-256 of what it wrote.  Two builds that claim the same driver print the same text: tools/zenc_plan.py > a.txt, then once
more with NAF_GPU_LIB=<the other libnaf_gpu.so> (on the GPU box from the repo root, a fresh process each; profiles/zenc_driver_plan.txt).

    tools/zenc_plan.py --time [--bytes N]          host time of the driver: the least wall time, in ms, of the timed calls per row
    tools/zenc_plan.py --compare P1 .. P5 -- B1 .. B5      the five processes of the parent's build against this build's
(profiles/zenc_driver_perf.txt; the rows: naf_gpu_zstd_compress of 64 KiB and 16 MiB at levels 1 and 3, ennaf at level 1 of the four
texts of tools/perf_enc.py at its default size)."""
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# thresholds of zstd_encode_begin and enc.hip, by the names the code gives them (or the phase that holds the number)
ZENC_CACHE_ENTRIES = 256
SAMPLE_BLOCKS = 16 * ZENC_CACHE_ENTRIES            # plan_buffers: sample_stride, the cache -- and with it the frame's tree
TREE_DEFER_BLOCKS = 256                            # plan_blocks: wt_defer
LZ_LINES_BLOCKS = 64                               # lz_buffers: k_lz_parse_lines
SMALL = (0, 1, 63, 64, 2047, 2048)                 # nothing; less than a match (lz_on); the flat scan's 2048
FUSED_TEXT = 256 << 17                             # enc.hip: the one-pass split (`fused`) from 256 times 128 KiB of text up
SMALL_BLOCKS = {"BLOCK_LOG": "10"}                 # blocks of 1 KiB: the block counts above in a few MiB


def stream(n, seed, names=False):
    """n bytes a level-1 planner has something to do with: skewed symbols, a stretch of them once more; names: zero-terminated lines."""
    import numpy as np
    rng = np.random.default_rng(seed)
    if names:
        rows = [b"read.%d.%d length=%d\0" % (seed, k, 100 + k % 7) for k in range(n // 16 + 1)]
        return b"".join(rows)[:n]
    p = np.array([0.7 ** k for k in range(24)])
    b = (rng.choice(24, n, p=p / p.sum()) + 40).astype(np.uint8)
    if n >= 4096:
        b[n // 2:n // 2 + n // 8] = b[n // 16:n // 16 + n // 8]
    return b.tobytes()


def cases(ctx):
    """(name, env, what, argument): what "z" -> (bytes, level) for naf_gpu_zstd_compress; "ennaf" -> (text, keyword arguments);
    "shard" -> (text, rank): that rank's pieces of a two-shard ennaf, the other shard's record from the CPU stand-in."""
    import numpy as np
    import huf_plan as P
    from naf_amd import synth
    out = []
    for n in SMALL:
        for level in (1, 3, 19):
            out.append(("z%d %d bytes" % (level, n), {}, "z", (stream(n, n), level)))
    for nblk in (TREE_DEFER_BLOCKS - 1, TREE_DEFER_BLOCKS, SAMPLE_BLOCKS - 1, SAMPLE_BLOCKS + 1):
        out.append(("z1 %d blocks" % nblk, SMALL_BLOCKS, "z", (stream(nblk << 10, nblk), 1)))
    out.append(("z1 %d blocks TREE_DEFER=0" % TREE_DEFER_BLOCKS, dict(SMALL_BLOCKS, TREE_DEFER="0"), "z", (stream(TREE_DEFER_BLOCKS << 10, TREE_DEFER_BLOCKS), 1)))
    for nblk in (LZ_LINES_BLOCKS - 1, LZ_LINES_BLOCKS):                          # the match finder without a window: level 1 with NAF_GPU_LZ=all
        out.append(("z1 LZ=all %d blocks of names" % nblk, dict(SMALL_BLOCKS, LZ="all"), "z", (stream(nblk << 10, nblk, names=True), 1)))
    out.append(("z1 LZ=all %d blocks of names LZ_LINES=0" % LZ_LINES_BLOCKS, dict(SMALL_BLOCKS, LZ="all", LZ_LINES="0"), "z", (stream(LZ_LINES_BLOCKS << 10, LZ_LINES_BLOCKS, names=True), 1)))
    for level in (3, 19):                                                        # zenc_level_window: the window of a level, 64 KiB blocks
        out.append(("z%d %d blocks in a window" % (level, TREE_DEFER_BLOCKS), {}, "z", (stream(TREE_DEFER_BLOCKS << 16, level), level)))
    out.append(("z3 LZ=0", {"LZ": "0"}, "z", (stream(300_000, 33), 3)))
    # a frame with a frame's tree: the quality and sequence carriers of the literals-planner tests, SAMPLE_BLOCKS blocks
    for carrier in ("qual", "seq"):
        c = P.big_case(P.SEED, carrier, P.FRAME_BLOCKS)
        env = {k[8:]: v for k, v in c.env.items()}
        text = P.text_of(c)
        out.append(("ennaf %s" % c.name, env, "ennaf", (text, {})))
        if carrier == "qual":
            for lever in ("FRAME_TREE", "FRAME_QUICK", "FRAME_WRITE"):
                out.append(("ennaf %s %s=0" % (c.name, lever), dict(env, **{lever: "0"}), "ennaf", (text, {})))
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    flat = b">flat\n" + synth.wrap_lines(acgt[rng.integers(0, 4, 300_000)], 80)
    out.append(("ennaf flat fasta", {}, "ennaf", (flat, {})))
    out.append(("ennaf flat fasta PREFER_FLAT=0", {"PREFER_FLAT": "0"}, "ennaf", (flat, {})))
    # a direct frame: a 4-bit FASTA just large enough for the one-pass split at level 1; and from two passes
    big = synth.fasta_acgt_device(FUSED_TEXT + 4096, n_records=3, width=80, seed=11, device="cuda")
    assert big.numel() >> 17 >= 256
    out.append(("ennaf direct frame", {}, "ennaf", (big, {})))
    out.append(("ennaf direct frame ONEPASS=0", {"ONEPASS": "0"}, "ennaf", (big, {})))
    # a ragged tail: an odd number of bases behind whole direct blocks (the tail is a part of its own), and without direct blocks
    odd = b">odd\n" + synth.wrap_lines(acgt[rng.integers(0, 4, 65536 * 6 + 1001)], 80)
    out.append(("ennaf ragged tail behind direct blocks", {"DIRECT": "2", "PROBE": "0"}, "ennaf", (odd, {})))
    out.append(("ennaf ragged tail", {}, "ennaf", (odd, {})))
    mixed, reads, rep = synth.fasta_mixed(40, 3000, 60, seed=5), synth.fastq_reads(2000, 150, seed=9, var_len=True), synth.repeat_genome(seed=4, unit=20000, copies=8)
    for level in (1, 3):
        out.append(("ennaf -%d mixed fasta" % level, {}, "ennaf", (mixed, {"level": level})))
        out.append(("ennaf -%d fastq" % level, {}, "ennaf", (reads, {"level": level})))
    out.append(("ennaf --long 10 repeats", {}, "ennaf", (rep, {"long_log": 10})))
    for rank in (0, 1):
        out.append(("ennaf shard %d of 2" % rank, {}, "shard", (mixed, rank)))
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


def run(ctx, what, arg):
    import torch
    if what == "z":
        return ctx.zstd_compress(ctx.to_device(arg[0]), level=arg[1])
    if what == "ennaf":
        text = arg[0] if isinstance(arg[0], torch.Tensor) else ctx.to_device(arg[0])
        return ctx.ennaf(text, **arg[1])[0]
    from naf_amd import shard
    from oracle import oracle as O
    from shard_standin import StandInCtx
    text, rank = arg
    opts, d = shard.make_opts(), ctx.to_device(text)
    fmt, p0 = ctx.ennaf_sniff(d)
    cuts = shard.cuts_local(ctx, d, fmt, p0, 2)
    infos = [ctx.ennaf_shard_begin(d[cuts[k]:cuts[k + 1]], opts, fmt, k, 2) if k == rank else StandInCtx(O).ennaf_shard_begin(text[cuts[k]:cuts[k + 1]], opts, fmt, k, 2) for k in range(2)]
    buf, pc = ctx.ennaf_shard_finish(opts, infos, cuts[rank + 1] - cuts[rank])
    return buf[:pc.total]


def plan():
    from naf_amd import capi
    ctx = capi.Context(0)
    for name, env, what, arg in cases(ctx):
        with Env(env):
            ctx.set_timing(True)
            try:
                r = run(ctx, what, arg)
                kernels = " ".join("%s x%d" % (n, k) for n, k in sorted((n, k) for n, ms, k in ctx.get_timing()))
                res = "%d bytes sha256 %s" % (r.numel(), hashlib.sha256(r.cpu().numpy().tobytes()).hexdigest())
            except capi.NafGpuError as e:
                kernels, res = "", "error %d %s" % (e.code, e.msg.strip())
            ctx.set_timing(False)
        print("%s: %s | %s" % (name, kernels, res), flush=True)
    ctx.close()


# ---- host time ----------------------------------------------------------------------------------------------------------------------------
def measure(size):
    import torch
    from naf_amd import capi, synth
    ctx = capi.Context(0)
    print("# %s  %s" % (torch.cuda.get_device_name(0), "the build NAF_GPU_LIB names" if os.environ.get("NAF_GPU_LIB") else "this build"))

    def timed(name, call, reps, warm):
        t = []
        for k in range(warm + reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            call()
            torch.cuda.synchronize(); t.append((time.perf_counter() - t0) * 1e3)
        print("%-28s least %10.4f ms of %d calls" % (name, min(t[warm:]), reps), flush=True)

    for n, nm in ((64 << 10, "64KiB"), (16 << 20, "16MiB")):
        d = ctx.to_device(stream(n, 5))
        cap = ctx.L.naf_gpu_zstd_compress_bound(n)
        out, got = torch.empty(cap, dtype=torch.uint8, device=ctx.device), capi.C.c_size_t()
        for level in (1, 3):
            timed("zstd_compress_%s_level_%d" % (nm, level), lambda: ctx._check(ctx.L.naf_gpu_zstd_compress(ctx.h, capi._ptr(d), n, level, capi._ptr(out), cap, capi.C.byref(got))), 40, 5)
        del d, out
    for which in ("uniform", "fastq", "realistic", "softmasked"):                 # the texts of tools/perf_enc.py
        if which == "fastq":
            text = synth.fastq_reads_device(size, seed=7, device="cuda")
        elif which == "realistic":
            text = synth.realistic_genome_device(size, device="cuda")
        elif which == "uniform":
            text = synth.fasta_acgt_device(size, n_records=100, width=80, seed=2024, device="cuda")
        else:
            text = synth.softmask_device(synth.fasta_acgt_device(size, n_records=24, width=60, seed=7, device="cuda"))
        n = text.numel()
        ctx.reserve(int(n * 2.0) + (1 << 30))
        buf = torch.empty(int(ctx.L.naf_gpu_ennaf_bound(n)), dtype=torch.uint8, device="cuda")
        timed("ennaf_%s_%d" % (which, n), lambda: ctx.ennaf(text, out=buf), 7, 2)
        del text, buf
        torch.cuda.empty_cache()
    ctx.close()


def read(path):
    rows = {}
    for line in open(path):
        f = line.split()
        if len(f) >= 4 and f[1] == "least":
            rows[f[0]] = float(f[2])
    return rows


def compare(parent, branch):
    P, B = [read(p) for p in parent], [read(p) for p in branch]
    print("least wall time of a process's timed calls, ms; one column a process, the builds alternating; spread = the parent against itself, max - min;")
    print("within = the difference of the means is no larger than that spread")
    bad = 0
    for name in P[0]:
        a, b = [r[name] for r in P], [r[name] for r in B]
        ma, mb, spread = sum(a) / len(a), sum(b) / len(b), max(a) - min(a)
        verdict = "within" if abs(mb - ma) <= spread else "faster" if mb < ma else "NOT within"
        bad += verdict == "NOT within"
        print("%-28s parent %s  mean %10.4f  min .. max %10.4f .. %10.4f (%.4f)" % (name, " ".join("%10.4f" % x for x in a), ma, min(a), max(a), spread))
        print("%-28s branch %s  mean %10.4f  min .. max %10.4f .. %10.4f  branch - parent %+.4f, %s" % ("", " ".join("%10.4f" % x for x in b), mb, min(b), max(b), mb - ma, verdict))
    print("%d of %d rows not within the parent's spread" % (bad, len(P[0])))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--compare":
        k = a.index("--")
        compare(a[1:k], a[k + 1:])
    elif a and a[0] == "--time":
        measure(int(float(a[2])) if len(a) > 2 and a[1] == "--bytes" else int(10e9))
    else:
        plan()
