"""Where the bytes land and what they are made from: every C-ABI entry point that takes device buffers, with its buffers inside a
fenced arena (tests/fenced.py) at every address phase, and with capacities of exactly the size the library asks for.

(a) destination and source phase: the content equals the oracle's (or numpy's), out_len is right, no byte outside the output changed;
(b) the calls whose input sits at phase 0, 1, 16 or 65 run a second time in an arena of another salt with the complement of the bait
    around the input -- both runs equal the one reference, so no result depends on a byte outside [d_src, d_src + len);
(c) too small a capacity is NAF_GPU_ECAP with the arena behind the capacity untouched, the size of the whole result where the header
    promises it, and a context that makes the exact-capacity call correctly afterwards.
The judge is never a second call of the library.  NAF_TEST_TALLY=<file> writes how many calls of each kind every entry point got."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import golden_bytes
from fenced import BIG_PHASES, PHASES, Arena, address, combos, fenced_runs, stream_bait, text_bait

pytestmark = pytest.mark.gpu
FASTA, FASTQ, SEQ, SEQUENCES, FOURBIT = 0, 1, 2, 3, 4
E_CAP = -6
ARENA_BYTES = 3 << 20
TALLY = {}


def tally(entry, kind, n=1):
    TALLY.setdefault(entry, {"a": 0, "b": 0, "c": 0})[kind] += n


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()
    if os.environ.get("NAF_TEST_TALLY"):
        with open(os.environ["NAF_TEST_TALLY"], "w") as f:
            json.dump(TALLY, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def arenas(gpu):
    return [Arena("cuda", 0x3C, ARENA_BYTES), Arena("cuda", 0xD7, ARENA_BYTES)]


def host(t):
    return t.cpu().numpy().tobytes()


def ptr(view):
    return C.c_void_p(address(view))


def dev(gpu, data):
    return gpu.to_device(data)


# ---- inputs, made once -----------------------------------------------------------------------------------------------------------
def unwrapped(text):
    out = []
    for rec in text.split(b">")[1:]:
        head, _, body = rec.partition(b"\n")
        out.append(b">" + head + b"\n" + (body.replace(b"\n", b"") + b"\n" if body else b""))
    return b"".join(out)


@pytest.fixture(scope="module")
def data(gpu):
    from naf_amd import synth
    rng = np.random.default_rng(77)
    d = {"fasta": synth.fasta_mixed(7, 2100, 60, seed=22), "fastq": synth.fastq_reads(100, 120, seed=3, var_len=True),
         "protein": b">p1 protein\n" + bytes(rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY*", dtype=np.uint8), 5000)) + b"\n",
         "header": b">only a header\n", "empty": b"", "big": synth.fasta_mixed(120, 3000, 60, seed=22)}
    d["nowrap"] = unwrapped(d["fasta"])
    assert 3 * 4096 < len(d["fasta"]) < 4 * 4096 and len(d["fasta"]) % 16, len(d["fasta"])          # three tiles and an odd tail
    assert 280_000 < len(d["big"]) < 400_000, len(d["big"])                                          # the sequence stream crosses a 128 KiB block
    naf = {k: host(gpu.ennaf(dev(gpu, d[k]))[0]) for k in ("fasta", "nowrap", "fastq", "big")}       # (inputs of the decoders; judged by the oracle there)
    naf["ref_fasta"], naf["ref_fastq"] = golden_bytes("naf", "mixed_60.naf"), golden_bytes("naf", "fastq_var.naf")    # libzstd's block shapes
    return d, naf


def is_big(b):
    return len(b) > 200_000


def phases_for(*buffers):
    return BIG_PHASES if any(is_big(b) for b in buffers) else PHASES


def sweep(arenas, entry, src, cap, bait, call, judge, phases):
    """(a) and (b): every combination of phases; each result judged, the results of the two fills equal."""
    import torch
    t = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).cuda() if len(src) else src
    for pi, po in combos(phases) if cap is not None else [(p, 0) for p in phases]:
        res = fenced_runs(arenas, t, cap, pi, po, bait, call)
        for r in res:
            judge(r)
        assert all(r == res[0] for r in res), (entry, pi, po)
        tally(entry, "a")
        tally(entry, "b", len(res) - 1)


def capacity(arenas, entry, src, need, bait, call, judge, promised, caps=None):
    """(c): NAF_GPU_ECAP, nothing written outside [0, cap), the whole size reported where promised, the context good afterwards."""
    import torch
    A = arenas[0]
    for po in (0, 5):
        for cap in sorted(set(caps or ()) | {0, 1, need - 1}):
            if not 0 <= cap < need:
                continue
            A.reset()
            d_in, d_out = A.put(src, 0, *bait(0)), A.out(cap, po)
            r = call(d_in, d_out)
            torch.cuda.synchronize()
            assert r[0] == E_CAP, (entry, cap, r[0])
            A.check()
            if promised:
                assert r[1] == need, (entry, cap, r[1], need)
            A.reset()
            d_in, d_out = A.put(src, 0, *bait(0)), A.out(need, po)
            r = call(d_in, d_out)
            torch.cuda.synchronize()
            A.check()
            judge(r)
            tally(entry, "c")


# ---- zstd --------------------------------------------------------------------------------------------------------------------------
def payloads(n):
    rng = np.random.default_rng(1000 + n)
    syms = np.array([0x88, 0x84, 0x82, 0x81, 0x48, 0x44, 0x42, 0x41, 0x28, 0x24, 0x22, 0x21, 0x18, 0x14, 0x12, 0x11], dtype=np.uint8)
    p2 = np.array([2.0 ** -(i + 1) for i in range(12)])
    return [("nibbles", syms[rng.integers(0, 16, n)].tobytes()), ("rle", b"\x07" * n),
            ("skew", rng.choice(np.arange(12, dtype=np.uint8) + 60, n, p=p2 / p2.sum()).tobytes())]


def zstd_dec_call(gpu, has_magic):
    def call(d_in, d_out):
        n = C.c_size_t(1 << 40)
        rc = gpu.L.naf_gpu_zstd_decompress(gpu.h, ptr(d_in), d_in.numel(), has_magic, ptr(d_out), d_out.numel(), C.byref(n))
        return rc, n.value, host(d_out[:n.value]) if rc == 0 else None
    return call


def equals(want):
    def judge(r):
        assert r[0] == 0 and r[1] == len(want) and r[2] == want, (r[0], r[1], len(want))
    return judge


SIZES = (0, 1, 15, 16, 17, 4095, 32767, 32768, 32769, 131073)


@pytest.mark.parametrize("n", SIZES)
def test_zstd_decompress_of_this_build_s_frames(gpu, oracle, arenas, n):
    frames = []
    for name, p in payloads(n):
        for level in (1, 3):
            f = host(gpu.zstd_compress(dev(gpu, p), level))
            assert oracle.zstd_decompress(f, len(p) + 16) == p          # the input of this test is a frame the oracle reads
            frames.append((f, p))
    frames.append((frames[0][0] + frames[3][0], frames[0][1] + frames[3][1]))      # two frames laid end to end
    frames.append((frames[4][0] + frames[1][0], frames[4][1] + frames[1][1]))
    for f, p in frames:
        for has_magic in (1, 0):
            src = f if has_magic else f[4:]
            sweep(arenas, "naf_gpu_zstd_decompress", src, len(p), lambda run: stream_bait(src, run), zstd_dec_call(gpu, has_magic), equals(p), phases_for(p))
    # (c), two frames: the needed size is the sum over both, also when it is the second that does not fit
    f, p = frames[6]
    n1 = len(frames[0][1])
    if len(p):
        capacity(arenas, "naf_gpu_zstd_decompress", f, len(p), lambda run: stream_bait(f, run), zstd_dec_call(gpu, 1), equals(p), True,
                 caps=[n1 - 1, n1, n1 + 1, len(p) - 1])
        capacity(arenas, "naf_gpu_zstd_decompress", frames[1][0][4:], n, lambda run: stream_bait(f, run), zstd_dec_call(gpu, 0), equals(frames[1][1]), True)


@pytest.mark.parametrize("name", ["empty", "one", "lens_l1", "ids_l3", "two_frames", "rep_l19"])
def test_zstd_decompress_of_libzstd_s_frames(gpu, oracle, arenas, name):
    f = golden_bytes("zstd", name + ".zst")
    p = oracle.zstd_decompress(f)
    for has_magic in (1, 0):
        src = f if has_magic else f[4:]
        sweep(arenas, "naf_gpu_zstd_decompress", src, len(p), lambda run: stream_bait(src, run), zstd_dec_call(gpu, has_magic), equals(p), phases_for(p))
    if len(p):
        capacity(arenas, "naf_gpu_zstd_decompress", f, len(p), lambda run: stream_bait(f, run), zstd_dec_call(gpu, 1), equals(p), True,
                 caps=[len(p) // 2, len(p) - 7])


@pytest.mark.parametrize("n", (1, 32767, 32768, 32769))
def test_zstd_decompress_on_either_side_of_the_capacity_switch(gpu, oracle, arenas, n):
    """The decoder picks its kernel from the capacity: a buffer of exactly the decoded size and a roomy one, both fenced, both right."""
    import torch
    A = arenas[0]
    for name, p in payloads(n):
        for level in (1, 3):
            f = host(gpu.zstd_compress(dev(gpu, p), level))
            for cap in (n, n + (1 << 20)):
                for po in (0, 5):
                    A.reset()
                    d_in, d_out = A.put(f, 1, *stream_bait(f, 0)), A.out(cap, po)
                    r = zstd_dec_call(gpu, 1)(d_in, d_out)
                    torch.cuda.synchronize()
                    A.check()
                    equals(p)(r)
                    at = address(d_out) - address(A.buf)
                    assert torch.equal(d_out[n:], A.pattern[at + n:at + cap]), "bytes of the buffer behind out_len were written"
                    tally("naf_gpu_zstd_decompress", "a")


@pytest.mark.parametrize("n", SIZES)
def test_zstd_compress(gpu, oracle, arenas, n):
    bound = gpu.L.naf_gpu_zstd_compress_bound(n)
    for name, p in payloads(n):
        for level in (1, 3):
            def call(d_in, d_out):
                m = C.c_size_t(1 << 40)
                rc = gpu.L.naf_gpu_zstd_compress(gpu.h, ptr(d_in), d_in.numel(), level, ptr(d_out), d_out.numel(), C.byref(m))
                return rc, m.value, host(d_out[:m.value]) if rc == 0 else None

            seen = set()

            def judge(r):
                assert r[0] == 0 and r[1] <= bound
                if r[2] not in seen:                                   # (the oracle's verdict on these very bytes is kept)
                    assert oracle.zstd_decompress(r[2], len(p) + 16) == p, name
                    seen.add(r[2])
            sweep(arenas, "naf_gpu_zstd_compress", p, bound, lambda run: stream_bait(p, run), call, judge, phases_for(p))
            if name == "nibbles":
                capacity(arenas, "naf_gpu_zstd_compress", p, bound, lambda run: stream_bait(p, run), call, judge, False)


# ---- unnaf -------------------------------------------------------------------------------------------------------------------------
def unnaf_call(gpu, mode, use_mask, ll, begin=None, end=None):
    from naf_amd import capi

    def call(d_in, d_out):
        o = capi.UnnafOpts(mode, int(use_mask), ll)
        n = C.c_size_t(1 << 40)
        if d_out is None:
            rc = gpu.L.naf_gpu_unnaf_size(gpu.h, ptr(d_in), d_in.numel(), C.byref(o), C.byref(n))
            return rc, n.value, None
        if begin is None:
            rc = gpu.L.naf_gpu_unnaf(gpu.h, ptr(d_in), d_in.numel(), C.byref(o), ptr(d_out), d_out.numel(), C.byref(n))
        else:
            rc = gpu.L.naf_gpu_unnaf_range(gpu.h, ptr(d_in), d_in.numel(), C.byref(o), begin, end, ptr(d_out), d_out.numel(), C.byref(n))
        return rc, n.value, host(d_out[:n.value]) if rc == 0 else None
    return call


DNA_ARCHIVES = ["fasta", "nowrap", "ref_fasta", "big"]


# FASTA, SEQ, SEQUENCES and 4BIT of the DNA archives, FASTQ of the reads
@pytest.mark.parametrize("which, mode", [(w, m) for w in DNA_ARCHIVES for m in (FASTA, SEQ, SEQUENCES, FOURBIT)] + [("fastq", FASTQ), ("ref_fastq", FASTQ)])
def test_unnaf_and_unnaf_size(gpu, oracle, arenas, data, which, mode):
    naf = data[1][which]
    for use_mask in (True, False):
        for ll in (-1, 0, 7):
            want = oracle.unnaf(naf, mode, use_mask, ll)
            bait = lambda run: stream_bait(naf, run)
            sweep(arenas, "naf_gpu_unnaf", naf, len(want), bait, unnaf_call(gpu, mode, use_mask, ll), equals(want), phases_for(naf, want))

            def size_is(r):
                assert r[0] == 0 and r[1] == len(want)
            sweep(arenas, "naf_gpu_unnaf_size", naf, None, bait, unnaf_call(gpu, mode, use_mask, ll), size_is, phases_for(naf, want))
    if which in ("fasta", "ref_fastq", "big") and mode in (FASTA, FASTQ, SEQ):
        want = oracle.unnaf(naf, mode, True, -1)
        capacity(arenas, "naf_gpu_unnaf", naf, len(want), lambda run: stream_bait(naf, run), unnaf_call(gpu, mode, True, -1), equals(want), True)


@pytest.mark.parametrize("which", DNA_ARCHIVES + ["fastq", "ref_fastq"])
def test_unnaf_range(gpu, oracle, arenas, data, which):
    naf = data[1][which]
    mode = FASTQ if "fastq" in which else FASTA
    text = oracle.unnaf(naf, mode, True, -1)
    line = 0
    while text.index(b"\n", line) - line < 40:                        # the first line of 40 bytes or more that is no header
        line = text.index(b"\n", line) + 1
    line = line if text[line:line + 1] not in b">@" else text.index(b"\n", line) + 1
    ranges = [(2, min(len(text), 1003)), (line + 17, min(len(text), line + 17 + 4097)), (len(text) - 5, len(text))]     # from inside a header, from inside a line, the last 5 bytes
    assert text[0:1] in b">@" and text[line + 16:line + 18].isalpha()
    for b, e in ranges:
        want = text[b:e]
        sweep(arenas, "naf_gpu_unnaf_range", naf, e - b, lambda run: stream_bait(naf, run), unnaf_call(gpu, mode, True, -1, b, e), equals(want), phases_for(naf))
    b, e = ranges[1]
    capacity(arenas, "naf_gpu_unnaf_range", naf, e - b, lambda run: stream_bait(naf, run), unnaf_call(gpu, mode, True, -1, b, e), equals(text[b:e]), True)


def select_call(gpu, mode, segs, stranded):
    from naf_amd import capi

    def call(d_in, d_out):
        o = capi.UnnafOpts(mode, 1, -1)
        n = C.c_size_t(1 << 40)
        sa = gpu._segments([(r, b, capi.WHOLE if e is None else e) for r, b, e, _ in segs])
        if stranded:
            st = (C.c_uint8 * max(len(segs), 1))(*[rv for _, _, _, rv in segs])
            rc = gpu.L.naf_gpu_unnaf_select_stranded(gpu.h, ptr(d_in), d_in.numel(), C.byref(o), sa, st, len(segs), ptr(d_out), d_out.numel(), C.byref(n))
        else:
            rc = gpu.L.naf_gpu_unnaf_select(gpu.h, ptr(d_in), d_in.numel(), C.byref(o), sa, len(segs), ptr(d_out), d_out.numel(), C.byref(n))
        return rc, n.value, host(d_out[:n.value]) if rc == 0 else None
    return call


@pytest.mark.parametrize("which", ["fasta", "ref_fasta", "fastq"])
def test_unnaf_select_and_select_stranded(gpu, oracle, arenas, data, which):
    from test_gpu_select_strand import Records
    naf = data[1][which]
    mode = FASTQ if which == "fastq" else FASTA
    R = Records(oracle, naf, mode)
    rec = next(r for r in range(1, R.n) if len(R.bases[r]) > (400 if mode == FASTA else 50))
    forward = [[(rec, 0, None, 0)]] + ([[(rec, 7, 7 + 333, 0)]] if mode == FASTA else [])         # a whole record, an odd-begin sub-range
    bait = lambda run: stream_bait(naf, run)
    for segs in forward:
        sweep(arenas, "naf_gpu_unnaf_select", naf, len(R.expect(segs)), bait, select_call(gpu, mode, segs, False), equals(R.expect(segs)), PHASES)
        rc_segs = [(r, b, e, 1) for r, b, e, _ in segs]
        for s in (segs, rc_segs, segs + rc_segs):
            sweep(arenas, "naf_gpu_unnaf_select_stranded", naf, len(R.expect(s)), bait, select_call(gpu, mode, s, True), equals(R.expect(s)), PHASES)
    for stranded in (False, True):                                     # n_segs = 0 into a view of no bytes
        sweep(arenas, "naf_gpu_unnaf_select" + ("_stranded" if stranded else ""), naf, 0, bait, select_call(gpu, mode, [], stranded), equals(b""), PHASES)
    segs = forward[-1] + [(rec, 0, None, 1)]
    capacity(arenas, "naf_gpu_unnaf_select", naf, len(R.expect(forward[-1])), bait, select_call(gpu, mode, forward[-1], False), equals(R.expect(forward[-1])), True)
    capacity(arenas, "naf_gpu_unnaf_select_stranded", naf, len(R.expect(segs)), bait, select_call(gpu, mode, segs, True), equals(R.expect(segs)), True)


# ---- ennaf -------------------------------------------------------------------------------------------------------------------------
def report_fields(rep):
    return (rep.n_sequences, rep.n_bases, rep.longest_line, tuple(rep.unexpected_id), tuple(rep.unexpected_comment), tuple(rep.unexpected_seq), tuple(rep.unexpected_qual))


def header_fields(h):
    return (h.version, h.seq_type, h.flags, h.separator, h.line_length, h.n_sequences, h.title_off, h.title_len, tuple(h.orig_size), tuple(h.comp_size), tuple(h.payload_off))


class JudgedEnnaf:
    """What test_gpu_encode.check_ennaf takes for its `gpu`: ennaf() hands it the archive a fenced call made, everything else is the context."""

    def __init__(self, gpu, d_naf, rep):
        self.gpu, self.d_naf, self.rep = gpu, d_naf, rep

    def to_device(self, text):
        return text

    def ennaf(self, text, **kw):
        return self.d_naf, self.rep

    def unnaf(self, d_naf, mode):
        return self.gpu.unnaf(d_naf.clone(), mode)


def ennaf_call(gpu, oracle, text, seq_type, level, judged):
    from naf_amd import capi
    from test_gpu_encode import check_ennaf

    def call(d_in, d_out):
        o = capi.EnnafOpts(capi.FMT_AUTO, seq_type, 0, 0, level, -1, None, 0)
        n, rep = C.c_size_t(1 << 40), capi.EnnafReport()
        rc = gpu.L.naf_gpu_ennaf(gpu.h, ptr(d_in), d_in.numel(), C.byref(o), ptr(d_out), d_out.numel(), C.byref(n), C.byref(rep))
        if rc:
            return rc, n.value, None
        mine, fields = host(d_out[:n.value]), report_fields(rep)
        if (mine, fields) not in judged:                               # (the oracle's verdict on these very bytes is kept)
            assert check_ennaf(JudgedEnnaf(gpu, d_out[:n.value], rep), oracle, text, seq_type=seq_type) == mine
            judged.add((mine, fields))
        return rc, n.value, mine, fields, header_fields(gpu.parse_header(d_out[:n.value]))
    return call


def ok(r):
    assert r[0] == 0


@pytest.mark.parametrize("overlap", [None, "2"])
@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("which", ["fasta", "nowrap", "fastq", "protein", "header", "empty", "big"])
def test_ennaf(gpu, oracle, arenas, data, which, level, overlap, monkeypatch):
    if overlap:
        monkeypatch.setenv("NAF_GPU_ENC_OVERLAP", overlap)
    text = data[0][which]
    seq_type = 2 if which == "protein" else 0
    judged = set()
    call = ennaf_call(gpu, oracle, text, seq_type, level, judged)
    sweep(arenas, "naf_gpu_ennaf", text, gpu.L.naf_gpu_ennaf_bound(len(text)), text_bait, call, ok, phases_for(text))
    if which in ("fasta", "fastq", "protein", "big"):
        assert len(judged) == 1                                        # the archive depends on nothing but the text
        need = len(next(iter(judged))[0])
        capacity(arenas, "naf_gpu_ennaf", text, need, text_bait, call, ok, False)      # and the actual archive length is enough


def test_ennaf_shards_with_slices_and_pieces_at_odd_phases(gpu, oracle, arenas, data):
    """Three shards, a context each on the one device: slices at phases 1, 16 and 65, every piece buffer exactly its bound, the
    stitched archive exactly the planned length."""
    import torch
    from naf_amd import capi, shard
    from test_shard_cpu import check_against_whole
    text = data[0]["fasta"]
    ctxs = [gpu, capi.Context(0), capi.Context(0)]
    try:
        got = []
        for run, A in enumerate(arenas):
            A.reset()
            opts = shard.make_opts()
            whole = A.put(text, 0, *text_bait(run))
            fmt, p0 = gpu.ennaf_sniff(whole, opts.format)
            cuts = shard.cuts_local(gpu, whole, fmt, p0, 3)            # naf_gpu_ennaf_find_cut on views that start one byte in front of a nominal cut
            assert p0 == 0 and cuts[0] == 0 and cuts[3] == len(text) and cuts[0] < cuts[1] < cuts[2] < cuts[3]
            slices = [A.put(text[cuts[k]:cuts[k + 1]], (1, 16, 65)[k], *text_bait(run)) for k in range(3)]
            infos = [ctxs[k].ennaf_shard_begin(slices[k], opts, fmt, k, 3) for k in range(3)]
            arr = (capi.ShardInfo * 3)(*infos)
            bufs, pieces = [], []
            for k in range(3):
                buf = A.out(ctxs[k].L.naf_gpu_ennaf_shard_bound(slices[k].numel()), (65, 1, 16)[k])
                pc = capi.ShardPieces()
                assert ctxs[k].L.naf_gpu_ennaf_shard_finish(ctxs[k].h, C.byref(opts), arr, ptr(buf), buf.numel(), C.byref(pc)) == 0
                bufs.append(buf); pieces.append(pc)
            segs, lit, naf_len, rep = capi.stitch_plan(opts, infos, pieces)
            out = A.out(naf_len, 5)
            for c in ctxs:
                c.synchronize()
            gpu.ennaf_stitch(segs, lit, bufs, out)
            torch.cuda.synchronize()
            A.check()
            naf = host(out)
            check_against_whole(oracle, text, naf, rep, 0, False)
            assert oracle.unnaf(naf, FASTA) == oracle.unnaf(oracle.ennaf(text), FASTA)
            got.append((naf, report_fields(rep)))
            for e in ("naf_gpu_ennaf_shard_begin", "naf_gpu_ennaf_shard_finish"):
                tally(e, "a", 3); tally(e, "b", 3 * run)
            tally("naf_gpu_ennaf_find_cut", "a", 2); tally("naf_gpu_ennaf_stitch", "a"); tally("naf_gpu_ennaf_stitch", "b", run)
        assert got[0] == got[1]
    finally:
        for c in ctxs[1:]:
            c.close()


# ---- histogram, copy, gather -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 15, 16, 17, 4095, 4097))
def test_histogram(gpu, arenas, n):
    p = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    want = np.bincount(np.frombuffer(p, dtype=np.uint8), minlength=256).tolist()

    def call(d_in, d_out):
        cnt = (C.c_uint64 * 256)()
        return gpu.L.naf_gpu_histogram(gpu.h, ptr(d_in), d_in.numel(), cnt), list(cnt)

    def judge(r):
        assert r[0] == 0 and r[1] == want
    sweep(arenas, "naf_gpu_histogram", p, None, lambda run: stream_bait(p or b"\x00\xff", run), call, judge, PHASES)


def test_copy_and_gather_ranges(gpu, arenas):
    import torch
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, 256, 1001, dtype=np.uint8).tobytes(), rng.integers(0, 256, 4099, dtype=np.uint8).tobytes()
    A = arenas[0]
    for p in PHASES:
        q = (7 * p + 3) % 128
        for ps, pd in ((0, p), (p, 0), (p, q)):
            A.reset()
            src, dst = A.put(a, ps, *stream_bait(a, 0)), A.out(len(a), pd)
            assert gpu.L.naf_gpu_copy(gpu.h, ptr(dst), ptr(src), len(a)) == 0
            torch.cuda.synchronize()
            A.check()
            assert host(dst) == a
            tally("naf_gpu_copy", "a")
            A.reset()
            s1, s2 = A.put(a, ps, *stream_bait(a, 0)), A.put(b, q, *stream_bait(b, 0))
            total = 1 + len(a) + 2 + len(b) + 3
            dst = A.out(total, pd)
            at = address(dst) - address(A.buf)
            want = bytearray(host(A.pattern[at:at + total]))           # what no part covers keeps the pattern
            want[1:1 + len(a)] = a
            want[3 + len(a):3 + len(a) + len(b)] = b
            gpu.gather_ranges(dst, [(gpu, s1, 1), (gpu, s2, 3 + len(a))])          # odd offsets, odd lengths
            torch.cuda.synchronize()
            A.check()
            assert host(dst) == bytes(want)
            tally("naf_gpu_gather_ranges", "a")
