"""The encoder's match finders (k_lz_parse, k_lz_parse_lines, k_ldm_insert + k_lzx_parse + k_lzx_seqenc) on the streams of
tests/lz_plan.py: copies planted on every round, block, window, epoch and code seam (run with -m gpu on an MI355X).

Every frame this build makes of a planned stream is decoded by the from-spec oracle, by this machine's libzstd where it loads, and by
the HIP decoder with either sequence executor; its offsets are held to the window its header announces and, for the in-block stage,
to its own block; it is no larger than the frame the same call makes without the match finder; its blocks are the plan's split ("plan
out of date" otherwise: the plants would sit beside the seams, not on them).  The sequences of the frame, listed by the oracle, say
which plants were found; what is asserted about that is a floor (lz_plan.Tally.floor), and the table is printed."""
import ctypes
import os
import time
from contextlib import contextmanager

import pytest

import lz_plan as P

pytestmark = pytest.mark.gpu
CLASSES = ("round", "length", "literal", "end", "overlap", "distance", "count", "independent", "lines", "window", "epoch", "blockseam",
           "streamend", "rep", "cap", "tables")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def libzstd():
    for cand in ("/opt/conda/lib/libzstd.so", "libzstd.so.1"):
        try:
            z = ctypes.CDLL(cand)
        except OSError:
            continue
        z.ZSTD_decompress.restype = ctypes.c_size_t
        z.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        return z
    return None


def host(t):
    return t.cpu().numpy().tobytes()


@contextmanager
def switches(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


_PLANS, _TALLY, _RAN = {}, P.Tally(), {}


def cases_of(seed, cls):
    if seed not in _PLANS:
        _PLANS[seed] = P.all_cases(seed, "even")
    return [c for c in _PLANS[seed] if c.cls == cls]


def make(gpu, oracle, c, **extra):
    """(frame with magic, archive or None) of a case by its route."""
    from naf_amd import capi
    with switches(**dict(c.env, **extra)):
        if c.route == "direct":
            return host(gpu.zstd_compress(gpu.to_device(c.data), level=c.level)), None
        naf = host(gpu.ennaf(gpu.to_device(P.text_of(c)), seq_type=capi.SEQ_TEXT, long_log=c.long_log)[0])
        return oracle.parse_naf(naf).frame(naf, oracle.SEQ), naf


def run_case(gpu, oracle, libzstd, c):
    """Checks 1 to 7 of one case; returns the reasons it failed for."""
    bad = []
    frame, naf = make(gpu, oracle, c)
    # the literal-only twin, cut into the same blocks (as test_zstd_compress_lz_roundtrip states the invariant: one NAF_GPU_BLOCK_LOG for
    # both calls): the cross-block stage cuts blocks of min(2^16, window) bytes, and without the match finder the same call would announce
    # 2^19 and cut 32 KiB blocks -- three Huffman trees fewer on a stream of 12 KiB, 100 to 190 bytes that are not the match finder's
    same_blocks = {"NAF_GPU_BLOCK_LOG": str(min(P.LZX_BLOCK_LOG, c.wlog))} if c.stage == "lzx" else {}
    plain, _ = make(gpu, oracle, c, NAF_GPU_LZ="0", **same_blocks)
    if same_blocks:
        _TALLY.add_plain(c, frame, make(gpu, oracle, c, NAF_GPU_LZ="0")[0])       # the unqualified difference: printed, not asserted
    try:
        P.check_decodes(oracle, frame, c.data)                               # 1
    except P.Reject as e:
        return [str(e)]
    if libzstd is not None:                                                  # 2
        out = ctypes.create_string_buffer(len(c.data) + 64)
        r = libzstd.ZSTD_decompress(out, len(c.data) + 64, frame, len(frame))
        if r != len(c.data) or out.raw[:len(c.data)] != c.data:
            bad.append("libzstd: %d" % r)
    d_frame = gpu.to_device(frame)
    for lds in ("1", "0"):                                                   # 3
        with switches(NAF_GPU_EXEC_LDS=lds):
            if host(gpu.zstd_decompress(d_frame, len(c.data) + 64)) != c.data:
                bad.append("HIP decoder, NAF_GPU_EXEC_LDS=%s" % lds)
    if naf is not None:
        if host(gpu.unnaf(gpu.to_device(naf))) != P.text_of(c):
            bad.append("unnaf of the archive")
        if oracle.have_ref() and oracle.ref_unnaf(naf) != P.text_of(c):
            bad.append("the reference's unnaf of the archive")
    seqs, info = oracle.zstd_sequences(frame), oracle.zstd_frame_info(frame)
    checks = [lambda: P.check_window(frame, seqs, c.wlog if c.stage == "lzx" else None),                 # 4
              lambda: P.check_size(frame, plain),                                                        # 5
              lambda: P.check_split(seqs, c.seams)]                                                      # 6
    if c.stage == "lzx":
        checks.append(lambda: P.check_first_offsets(seqs))
    else:
        checks += [lambda: P.check_independent(seqs), lambda: P.check_independent(seqs, c.seams), lambda: P.check_probes(c, seqs)]
    if info.max_offset > (1 << info.window_log):
        bad.append("max_offset %d under a window of 2^%d" % (info.max_offset, info.window_log))
    for chk in checks:
        try:
            chk()
        except P.Reject as e:
            bad.append(str(e))
    _TALLY.add(c, seqs, info)                                                # 7
    return bad


def run_class(gpu, oracle, libzstd, cls):
    if cls not in _RAN:
        t0, bad, n = time.perf_counter(), [], 0
        for seed in P.SEEDS:
            for c in cases_of(seed, cls):
                n += 1
                bad += ["%s seed %d: %s" % (c.name, seed, b) for b in run_case(gpu, oracle, libzstd, c)]
        _RAN[cls] = (bad, n, time.perf_counter() - t0)
    return _RAN[cls]


@pytest.mark.parametrize("cls", CLASSES)
def test_planted_streams(gpu, oracle, libzstd, cls, capsys):
    bad, n, dt = run_class(gpu, oracle, libzstd, cls)
    with capsys.disabled():
        print("\n  %s: %d cases over seeds %s, %.1f s, %d failures" % (cls, n, list(P.SEEDS), dt, len(bad)))
    assert n > 0
    assert not bad, "\n".join(bad[:20])


def test_coverage_floor(gpu, oracle, libzstd, capsys):
    """Every cell has a found plant over the three seeds (but for the cells the plan lists as out of the finders' reach), each of the
    six repeat variants was written, a match reached the 16-bit cap, a block began with a match.  The found share itself is printed,
    not asserted: it is the hash tables' to decide."""
    for cls in CLASSES:
        run_class(gpu, oracle, libzstd, cls)
    with capsys.disabled():
        print("\n" + _TALLY.table("kernels (the even split)"))
        print("  seconds per class: " + ", ".join("%s %.1f" % (k, _RAN[k][2]) for k in CLASSES))
    _TALLY.floor()
