"""Host tests of the conformance corpus (tests/zstd_corpus.py, composed by tests/zstd_compose.py from RFC 8878): every frame
decodes to the composer's content under libzstd (the independent judge), the from-spec oracle and the host emulation of the GPU
decoder's kernel core; the features the frames use cover the checklist below; the corpus is pinned by one digest."""
import ctypes
import hashlib
import os

import pytest

from conftest import ROOT

import zstd_compose as Z
import zstd_corpus as K

# one SHA-256 over every frame and its content, in corpus order (the corpus is deterministic: a change to it changes this)
CORPUS_SHA256 = "3b682b8a2719c35d4ca8d032a4b3aa30c810badf75fe04123ef6890eb91bcd86"

# the checklist: every choice of RFC 8878 the corpus must make on purpose
REQUIRED = (
    ["hdr:fcs%d" % w for w in (0, 1, 2, 4, 8)] + ["fcs:edge:%d" % n for n in (255, 256, 65791, 65792)]
    + ["hdr:single_segment", "hdr:window", "hdr:window:mantissa", "hdr:checksum", "frame:skippable", "frame:concat"]
    + ["block:raw", "block:rle", "block:comp", "block:raw:empty_last", "block:comp:empty", "block:window_capped"]
    + ["lit:%s:h%s" % (k, f) for k in ("raw", "rle") for f in ("1:00", "1:10", "2", "3")]
    + ["huf:streams:1", "huf:streams:4", "huf:size:10", "huf:size:14", "huf:size:18", "huf:tree:direct", "huf:tree:fse",
       "huf:symbols:2", "huf:symbols:256"] + ["huf:maxbits:%d" % b for b in range(1, 12)]
    + ["lit:treeless"] + ["lit:treeless_after:" + k for k in ("raw_lits", "rle_lits", "raw_block", "rle_block", "huf")]
    + ["nseq:1byte", "nseq:2byte", "nseq:3byte", "nseq:2byte_small"] + ["nseq:edge:%d" % n for n in (127, 128, 0x7EFF, 0x7F00)]
    + ["mode:%s:%s" % (k, m) for k in ("ll", "of", "ml") for m in ("pre", "rle", "fse", "rep", "rep_of_rle", "rep_of_table")]
    + ["mode:rep_after_nseq0", "fse:lt1", "fse:zero_run", "fse:zero_run_ext"]
    + ["fse:log:ll:%d" % g for g in range(5, 10)] + ["fse:log:of:%d" % g for g in range(5, 9)] + ["fse:log:ml:%d" % g for g in range(5, 10)]
    + ["code:ll:%d" % c for c in range(36)] + ["code:ml:%d" % c for c in range(53)]
    + ["rep:%s:ov%d" % (k, v) for k in ("ll", "ll0") for v in (1, 2, 3)]
    + ["match:overlap_off:%d" % o for o in range(1, 17)] + ["match:ml_max", "match:window_back"]
    + ["huf:tree_repeat:nonadjacent", "huf:tree_repeat:prev:other_streams", "match:into_raw_block", "match:into_rle_block"]
    + ["size:full", "size:small", "size:mid", "size:big"]
    + ["look:control", "look:short_last", "look:seq_blocks:eighth", "look:seq_blocks:over_eighth"]
    + ["look:variant:" + v for v in K.LOOK_VARIANTS]
    # block positions: 0, 1, the middle, a tail of STRIDE_TAIL + 1, STRIDE_TAIL and STRIDE_TAIL - 1 blocks behind, the last two
    + ["look:pos:%d" % p for p in (0, 1, K.LOOK_N // 2, K.LOOK_N - K.STRIDE_TAIL - 2, K.LOOK_N - K.STRIDE_TAIL - 1,
                                   K.LOOK_N - K.STRIDE_TAIL, K.LOOK_N - 2, K.LOOK_N - 1)]
)


@pytest.fixture(scope="module")
def frames():
    return list(K.corpus())


def _libzstd():
    for cand in ("/opt/conda/lib/libzstd.so", "libzstd.so.1"):
        try:
            L = ctypes.CDLL(cand)
        except OSError:
            continue
        L.ZSTD_decompress.restype = ctypes.c_size_t
        L.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        L.ZSTD_isError.restype = ctypes.c_uint
        L.ZSTD_isError.argtypes = [ctypes.c_size_t]
        L.ZSTD_getErrorName.restype = ctypes.c_char_p
        L.ZSTD_getErrorName.argtypes = [ctypes.c_size_t]
        return L
    return None


def test_xxh64_matches_the_xxhash_module():
    xxhash = pytest.importorskip("xxhash")
    import numpy as np
    r = np.random.default_rng(1)
    for n in list(range(0, 70)) + [255, 1000, 4096 + 7, 100003]:
        d = r.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert Z.xxh64(d) == xxhash.xxh64_intdigest(d), n
        assert Z.xxh64(d, 12345) == xxhash.xxh64_intdigest(d, 12345), n


def test_corpus_decodes_under_libzstd(frames):
    L = _libzstd()
    if L is None:
        pytest.skip("libzstd is not on this machine")
    for name, fr, content, feat in frames:
        out = ctypes.create_string_buffer(len(content) + 64)
        r = L.ZSTD_decompress(out, len(content) + 64, fr, len(fr))
        assert not L.ZSTD_isError(r), (name, L.ZSTD_getErrorName(r))
        assert r == len(content) and out.raw[:r] == content, name


def test_corpus_decodes_under_the_oracle(frames, oracle):
    for name, fr, content, feat in frames:
        assert oracle.zstd_decompress(fr, len(content) + 64) == content, name


def test_corpus_decodes_under_the_kernel_core_emulation(frames):
    emul = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "libzstd_emul.so"))
    emul.emul_zstd_decompress_frame.restype = ctypes.c_longlong
    emul.emul_zstd_decompress_frame.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    for name, fr, content, feat in frames:
        got = b""
        for f in (Z.split_frames(fr) if "frame:concat" in feat else [fr]):
            out = ctypes.create_string_buffer(len(content) + 64)
            n = emul.emul_zstd_decompress_frame(f, len(f), out, len(content) + 64)
            assert n >= 0, (name, n)
            got += out.raw[:n]
        assert got == content, name


def test_census_covers_the_checklist(frames):
    union = set()
    for name, fr, content, feat in frames:
        union |= feat
    missing = [f for f in REQUIRED if f not in union]
    assert not missing, missing
    # every format and state family at all three sizes: the small ones within the small-frame decoder's limits, the mid ones past
    # them and under 4 MiB, the big ones over 4 MiB of frame
    fams = {}
    for name, fr, content, feat in frames:
        if "size:small" in feat:
            assert len(fr) <= K.SMALL_SRC and len(content) + 64 <= K.SMALL_OUT, name
        if "@" in name and not name.startswith("look_"):
            fams.setdefault(name.split("@")[0], set()).add(name.split("@")[1].split(".")[0])
    assert all(v == {"full", "mid", "big"} | (set() if n in K.NOT_SMALL else {"small"}) for n, v in fams.items()), fams
    for name, fr, content, feat in frames:
        if "size:big" in feat:
            assert len(fr) > 4 << 20, name
        if "size:mid" in feat:
            assert 16 << 10 < len(fr) < 4 << 20, name
        if name.startswith("look_") and not name.startswith("look_seq_blocks"):
            assert len(fr) > 4 << 20, name
    # the lookalikes all hold the same bytes: any of them can stand in for the sequence section of one archive (GPU tests)
    look = K.lookalike_content()
    assert all(content == look for name, fr, content, feat in frames if name.startswith("look_"))


def test_corpus_digest_is_pinned(frames):
    h = hashlib.sha256()
    for name, fr, content, feat in frames:
        h.update(name.encode() + b"\0" + hashlib.sha256(fr).digest() + hashlib.sha256(content).digest())
    assert h.hexdigest() == CORPUS_SHA256
