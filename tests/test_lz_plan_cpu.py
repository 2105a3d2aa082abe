"""The plan of the match-finder tests (tests/lz_plan.py) held to its own claims, run through the serial models of the two stages
(tests/emul: emul_zstd_compress_lz, emul_zstd_compress_lzx -- the kernels' sequence writers behind a parse of their own), and its checks
shown to reject frames composed to be wrong in exactly the ways test_gpu_lz_plan.py looks for.  No GPU.

The models cut a stream on multiples of the block size, so every case is built a second time for that split: the same plants on the
models' seams.  That the floor holds there shows that a floor missed on the GPU is missed for the kernels' reasons, not the inputs'.
The lines parser has no model; its cases are held to their claims only.  Where the models reach a cell by other means than the kernels
(a serial parse sees the positions of its own round, takes matches of four bytes, and never weighs a block against its literals) the
table says so below it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lz_plan as P
import zstd_compose as Z
from conftest import ROOT


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(ROOT, "tests", "emul", "libzstd_emul.so")
    if not os.path.exists(so):
        env = dict(os.environ, PATH="/opt/rocm/bin:" + os.environ.get("PATH", ""))
        subprocess.check_call(["make", "-s", "-C", ROOT, "emul"], env=env)
    L = ctypes.CDLL(so)
    L.emul_zstd_compress_lz.restype = ctypes.c_longlong
    L.emul_zstd_compress_lz.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
    L.emul_zstd_compress_lzx.restype = ctypes.c_longlong
    L.emul_zstd_compress_lzx.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.POINTER(ctypes.c_uint32)]
    return L


@pytest.fixture(scope="module")
def plans():
    return {seed: P.all_cases(seed, "even") for seed in P.SEEDS}


def test_every_case_is_what_the_plan_says(plans, oracle):
    """Every plant is a copy of its source, the guard bytes differ, every cell lies where it says relative to the seam of the even
    split, the archive route's stream comes back from the oracle's split of the text as planned, nothing is above 3 MB."""
    names = None
    for seed, cases in plans.items():
        for c in cases:
            P.verify_case(c, "even")
            assert len(c.data) <= P.MAX_STREAM
            assert c.plants or c.probes, c.name
            if c.route == "archive":
                s = oracle.split_text(P.text_of(c), oracle.TEXT)
                assert s.seq == c.data and s.n_sequences == 1, c.name
            else:
                assert c.env.get("NAF_GPU_LZ") == "all" or c.level >= 2, c.name
        assert names is None or names == [c.name for c in cases]           # the same cases at every seed
        names = [c.name for c in cases]
    assert len(set(names)) == len(names)


def test_no_cell_is_without_a_case(plans):
    cells = P.coverage_cells(plans[P.SEEDS[0]])
    planted = {(c.cls, cell) for c in plans[P.SEEDS[0]] for cell in c.cells}
    assert not [k for k in cells if k not in planted], "cells without a plant"
    for cls in ("round", "length", "literal", "end", "overlap", "distance", "count", "independent", "lines", "window", "epoch", "blockseam",
                "streamend", "rep", "cap", "tables"):
        assert any(k[0] == cls for k in cells), cls
    for (cls, cell), why in cells.items():
        assert why is None or (why in P.EXEMPT_KINDS and cls not in P.NEVER_EXEMPT), (cls, cell, why)
    # the streaks of the issue, by count
    assert sum(k[0] == "length" for k in cells) == len(P.LENGTHS) and sum(k[0] == "literal" for k in cells) == len(P.LITERALS) + 1
    assert sum(k[0] == "overlap" for k in cells) == len(P.PERIODS) * len(P.PERIOD_RUNS) and sum(k[0] == "distance" for k in cells) == len(P.DISTANCES) + 1
    assert sum(k[0] == "lines" for k in cells) == len(P.LINE_CELLS)


def test_the_split_restated_here_is_the_even_one():
    for n, bs in ((0, 1024), (1, 1024), (1024, 1024), (1025, 1024), (3 * 1024 - 5, 1024), (138000, 65536), (4 * 65536, 65536)):
        s = P.split_even(n, bs)
        nblk = max(1, -(-n // bs))
        assert len(s) == nblk + 1 and s[0] == 0 and s[-1] == n
        assert [s[b] for b in range(nblk)] == [b * (n // nblk) + min(b, n % nblk) for b in range(nblk)]
        assert max(np.diff(s)) <= bs and max(np.diff(s)) - min(np.diff(s)) <= 1


def run_model(emul, c):
    cap = len(c.data) + len(c.data) // 64 + 4096
    out = ctypes.create_string_buffer(cap)
    if c.stage == "lz":
        n = emul.emul_zstd_compress_lz(c.data, len(c.data), c.bs, out, cap)
    else:
        n = emul.emul_zstd_compress_lzx(c.data, len(c.data), c.bs, c.wlog, out, cap, None)
    assert n > 0, (c.name, n)
    return out.raw[:n]


def test_the_inputs_alone_reach_the_floor(emul, oracle, capsys):
    """Every case of the two stages that have a model, through that model: the round trip, the checks of the GPU test, the same floor."""
    tally = P.Tally()
    for seed in P.SEEDS:
        for c in P.all_cases(seed, "multiple", lines=False):
            P.verify_case(c, "multiple")
            frame = run_model(emul, c)
            P.check_decodes(oracle, frame, c.data)
            seqs = oracle.zstd_sequences(frame)
            assert seqs.size == len(c.data)
            P.check_split(seqs, c.seams)
            P.check_window(frame, seqs, c.wlog if c.stage == "lzx" else None)
            if c.stage == "lz":
                P.check_independent(seqs, c.seams)
                P.check_independent(seqs)
            else:
                P.check_first_offsets(seqs)
            tally.add(c, seqs, oracle.zstd_frame_info(frame))
    with capsys.disabled():
        print("\n" + tally.table("serial models (blocks on multiples of the block size)"))
        print("  (the models see the positions of their own round and take matches of four bytes; they code a block with its sequences\n"
              "   whenever that is smaller than the block itself, so short plants need no ballast there; the lines parser has no model)")
        empty = sorted(k for k, (f, n) in tally.cell.items() if f == 0)
        print("  cells the models leave empty: " + ("; ".join("%s %s (%s)" % (k[0], k[1], tally.exempt.get(k) or "NOT exempt: the kernels' design reaches it")
                                                                  for k in empty) or "none"))
        print("  every cell left empty is one the plan exempts for the kernels too; the probes (lz_plan.PROBE_CELLS) are held on the kernels' frames\n"
              "   only: a model takes the four bytes at bn - 4 and writes sequences into streams of under 128 bytes")
    tally.floor()


# ---- frames composed to be wrong ------------------------------------------------------------------------------------------------------------
def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def test_the_checks_reject_composed_bad_frames(oracle, capsys):
    seen = {}

    def rejected(name, fn):
        with pytest.raises(P.Reject) as e:
            fn()
        seen[name] = e.value.reason
        return e.value.reason

    # 1. an offset of W + 1 under an announced window W: composed under a wider window, then the descriptor says 2^10
    W = 1024
    blocks = [Z.raw(_rand(W, 1)), Z.raw(_rand(100, 2)), Z.comp(lits=_rand(20, 3), seqs=[(10, 16, W + 1 + 3)])]
    frame, content, _ = Z.compose(blocks, window_log=12)
    good = frame
    frame = frame[:5] + bytes([(10 - 10) << 3]) + frame[6:]
    P.check_decodes(oracle, frame, content)                                    # the from-spec oracle does not look at the window: the gap this closes
    seqs = oracle.zstd_sequences(frame)
    assert oracle.zstd_frame_info(frame).max_offset == W + 1 and int(seqs.distance.max()) == W + 1
    assert rejected("offset W + 1 under a window of W", lambda: P.check_window(frame, seqs, 10)) == "window"
    P.check_window(good, oracle.zstd_sequences(good), 12)                      # the same sequences under the window they were composed for
    fine, content2, _ = Z.compose([Z.raw(_rand(W, 1)), Z.raw(_rand(100, 2)), Z.comp(lits=_rand(20, 3), seqs=[(10, 16, W + 3)])], window_log=10)
    P.check_window(fine, oracle.zstd_sequences(fine), 10)                      # an offset of exactly W is legal

    # 2. a match whose source begins in the block in front
    blocks = [Z.raw(_rand(200, 4)), Z.comp(lits=_rand(50, 5), seqs=[(10, 8, 30 + 3)])]
    frame, content, _ = Z.compose(blocks, window_log=10)
    P.check_decodes(oracle, frame, content)
    seqs = oracle.zstd_sequences(frame)
    assert list(seqs.block_size) == [200, 58] and list(seqs.block_type) == [0, 2]
    assert rejected("a source in the block in front", lambda: P.check_independent(seqs)) == "dependent"
    assert rejected("a source in the block in front, the plan's seams", lambda: P.check_independent(seqs, [0, 200, 258])) == "dependent"
    inside, _, _ = Z.compose([Z.raw(_rand(200, 4)), Z.comp(lits=_rand(50, 5), seqs=[(10, 8, 10 + 3)])], window_log=10)
    P.check_independent(oracle.zstd_sequences(inside))                         # a source at the block's first byte is the block's own

    # 3. a repeat code that names the wrong slot: a valid frame of other bytes
    lits = _rand(12, 6)
    right = [Z.raw(_rand(300, 7)), Z.comp(lits=lits, seqs=[(4, 8, 100 + 3), (4, 8, 200 + 3), (4, 8, 1)])]      # ll > 0, value 1: the last offset
    wrong = [Z.raw(_rand(300, 7)), Z.comp(lits=lits, seqs=[(4, 8, 100 + 3), (4, 8, 200 + 3), (4, 8, 2)])]      # value 2: the one before it
    f_right, content, _ = Z.compose(right, window_log=10)
    f_wrong, other, _ = Z.compose(wrong, window_log=10)
    assert other != content and len(other) == len(content)
    P.check_decodes(oracle, f_right, content)
    assert rejected("a repeat code of the wrong slot", lambda: P.check_decodes(oracle, f_wrong, content)) == "decode"
    s = oracle.zstd_sequences(f_wrong)
    assert list(s.offset_value) == [103, 203, 2] and list(s.distance) == [100, 200, 100] and list(s.pos) == [304, 316, 328] and list(s.ll) == [4, 4, 4]
    first = [Z.raw(_rand(300, 7)), Z.comp(lits=lits, seqs=[(4, 8, 1)])]        # a block that begins with a repeat code: the frame's initial offsets
    f_first, _, _ = Z.compose(first, window_log=10)
    assert rejected("a block that begins with a repeat code", lambda: P.check_first_offsets(oracle.zstd_sequences(f_first))) == "repeat"

    # 4. a frame of valid shape, one byte larger than its literal-only twin
    data = _rand(100, 8)
    twin, content, _ = Z.compose([Z.comp(lits=data)], window_log=10)
    fat, content_fat, _ = Z.compose([Z.comp(lits=data, lit_fmt=3)], window_log=10)
    assert content == content_fat == data and len(fat) == len(twin) + 1
    P.check_decodes(oracle, fat, data)
    assert rejected("one byte larger than the literal-only frame", lambda: P.check_size(fat, twin)) == "larger"
    P.check_size(twin, twin)

    # 5. a sequence that begins in the four bytes a block has left behind its last valid start (what check_probes holds a probe to)
    blocks = [Z.raw(_rand(200, 11)), Z.comp(lits=_rand(96, 12), seqs=[(96, 4, 50 + 3)])]
    f5, content5, _ = Z.compose(blocks, window_log=10)
    c5 = P.Case("lz.end.begins_bn-4", "lz", "end", "begins_bn-4", "direct", content5, 1, {}, 0, 0, 1024, [0, 200, 300], [], [], {}, [(296, 20, 50)], [], None, [], [])
    assert rejected("a sequence in the last four bytes of a block", lambda: P.check_probes(c5, oracle.zstd_sequences(f5))) == "probe"
    P.check_probes(c5, oracle.zstd_sequences(frame))                           # a frame without a sequence there

    # and a frame whose blocks are not the plan's
    assert rejected("blocks that are not the plan's split", lambda: P.check_split(oracle.zstd_sequences(frame), P.split_even(1144, 1024))) == "plan out of date"
    with capsys.disabled():
        print("\ncomposed bad frames, and what rejected them:")
        for k, v in seen.items():
            print("  %-52s %s" % (k, v))
    assert sorted(set(seen.values())) == ["decode", "dependent", "larger", "plan out of date", "probe", "repeat", "window"]


def test_found_counts_what_the_issue_calls_found(oracle):
    """A plant is found when a sequence of its distance covers it from target_begin + 3 on; another distance, a late start or a short
    match do not count."""
    back = _rand(400, 9)
    for ll_extra, ml, dist, want in ((0, 40, 100, True), (3, 37, 100, True), (4, 36, 100, False), (0, 39, 100, False), (0, 40, 101, False)):
        frame, content, _ = Z.compose([Z.raw(back), Z.comp(lits=_rand(20 + ll_extra, 10), seqs=[(10 + ll_extra, ml, dist + 3)])], window_log=10)
        c = P.Case("t", "lz", "x", "y", "direct", content, 1, {}, 0, 0, 1024, [0, len(content)], [(410, 40, 100)], ["y"], {}, [], [], None, [], [])
        assert bool(P.found(c, oracle.zstd_sequences(frame))[0]) == want, (ll_extra, ml, dist)
