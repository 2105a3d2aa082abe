"""The plan and the model of the sequence-table tests (tests/seq_plan.py) held to their claims, the host build of the two sequence
writers (tests/emul: emul_write_sequences_x around zenc_write_sequences_x, emul_write_sequences around zenc_write_sequences) driven
through every cell -- those no kernel can reach included -- and the checks shown to reject sections composed to be wrong in the ways
test_gpu_seq_plan.py looks for.  No GPU.

Every section the host build writes is wrapped in a frame with Raw literals, decoded by the from-spec oracle and by this machine's
libzstd where it loads, listed by oracle.zstd_seq_tables and held to the model: planner, form, size.  The planned streams run through
the serial models of the two stages (emul_zstd_compress_lzx, emul_zstd_compress_lz) with the same checks and the parity check."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lz_plan as P
import seq_plan as Q
import zstd_compose as Z
from conftest import ROOT


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(ROOT, "tests", "emul", "libzstd_emul.so")
    env = dict(os.environ, PATH="/opt/rocm/bin:" + os.environ.get("PATH", ""))
    subprocess.check_call(["make", "-s", "-C", ROOT, "emul"], env=env)       # (a library from before the two drivers is made again)
    return Q.load_emul(so)


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


_TALLY = Q.Tally()


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def test_every_stream_is_what_the_plan_says(oracle):
    """Every plant is a copy of its source, every guard differs, every claimed position lies on its seam of the even split, the archive
    route's stream comes back from the oracle's split of the text, nothing is above lz_plan.MAX_STREAM; the same streams at every seed."""
    names = None
    for seed in Q.SEEDS:
        cases = Q.seq_cases(seed)
        for c in cases:
            P.verify_case(c, "even")
            assert c.plants and c.guards and c.claims, c.name
            assert len(c.guards) >= len(c.plants), c.name
            if c.route == "archive":
                s = oracle.split_text(P.text_of(c), oracle.TEXT)
                assert s.seq == c.data and s.n_sequences == 1, c.name
                assert c.long_log in (0, 10, 12, 16)
        assert names is None or names == [c.name for c in cases]
        names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert Q.split_even is P.split_even and Q.Stream is P.Stream and Q.Reject is P.Reject and Q.SEEDS is P.SEEDS       # shared, not copied
    assert {c.long_log for c in cases if c.route == "archive" and c.stage == "lzx"} == {10, 12, 16}


# ---- the model's pieces against the composer's, which is written from the RFC by other hands ------------------------------------------------
def test_the_model_restates_the_rfc():
    rng = np.random.default_rng([Q.SEED, 11])
    assert [Q.log2_256(1 << k) for k in range(12)] == [256 * k for k in range(12)]
    assert Q.log2_256(3) == 256 + 128 and Q.log2_256(5) == 512 + 64 and Q.log2_256(767) == 9 * 256 + 127
    assert all(Q.log2_256(v) <= Q.log2_256(v + 1) for v in range(1, 2000))
    ll = np.arange(0, 65536); ml = np.arange(3, 65536)
    c = Q.codes_of(ll, np.full(len(ll), 3), np.full(len(ll), 1))[0]
    assert [int(v) for v in c[:17]] == list(range(17)) and all(c[f] == c[f - 1] + 1 for f in Q.LL_FIRST) and c[-1] == 34
    assert [Z.ll_code(int(v)) for v in ll[::97]] == c[::97].tolist()
    c = Q.codes_of(np.zeros(len(ml), dtype=int), ml, np.full(len(ml), 1))[2]
    assert all(c[f - 3] == c[f - 4] + 1 for f in Q.ML_FIRST) and c[0] == 0 and c[-1] == 51
    assert [Z.ml_code(int(v)) for v in ml[::89]] == c[::89].tolist()
    ofv = np.array([1, 2, 3, 4, 7, 8, (1 << 20) - 1, 1 << 20, (1 << 31) + 5])
    assert Q.codes_of(np.zeros(9, dtype=int), np.full(9, 3), ofv)[1].tolist() == [0, 1, 1, 2, 2, 3, 19, 20, 31]
    for _ in range(300):
        k = int(rng.integers(0, 3))
        present = int(rng.integers(2, Q.ALPHABET[k] + 1))
        nseq = int(rng.integers(present, 5000))
        h = np.zeros(64, dtype=np.int64)
        syms = rng.choice(Q.ALPHABET[k], present, replace=False)
        h[syms] = 1
        np.add.at(h, rng.choice(syms, nseq - present, p=(lambda w: w / w.sum())(rng.random(present) ** 4)), 1)
        log = Q.accuracy_log(k, nseq, present)
        norm, repair = Q.normalise(h, nseq, log)
        assert sum(norm) == 1 << log and all((norm[s] > 0) == (h[s] > 0) for s in range(64)) and repair in ("exact", "topup", "takedown")
        last = max(s for s in range(64) if norm[s])
        assert Q.describe(norm, log) == Z.fse_describe(norm[:last + 1], log)
        sym, nb, base, prev = Q.decode_table(norm, log)
        assert list(zip(sym, nb, base)) == Z.fse_decode_table(norm[:last + 1], log)
    for k in range(3):
        norm, log, n = Q.PRE[k]
        assert sum(abs(v) for v in norm) == 1 << log and n == (36, 29, 53)[k]


# ---- the listing ---------------------------------------------------------------------------------------------------------------------------
def test_the_listing_reads_what_was_composed(oracle):
    """oracle.zstd_seq_tables on frames of tests/zstd_compose.py: every field is what the composer was told to write."""
    rng = np.random.default_rng([Q.SEED, 16])
    lits = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    seqs = [(int(rng.integers(0, 12)), int(rng.integers(3, 12)), int(rng.integers(4, 200))) for _ in range(200)]
    llc = Q.codes_of(*zip(*seqs))[0]
    counts = Z.normalize({int(c): int((llc == c).sum()) for c in set(llc.tolist())}, 7)
    same = [(4, 6, 50)] * 5
    blocks = [Z.raw(lits[:700]), Z.comp(lits=lits, seqs=seqs, modes=(("fse", counts, 7), "pre", "pre")), Z.rle(65, 40), Z.comp(lits=lits[:10]),
              Z.comp(lits=lits[:100], seqs=seqs[:9], modes=("rep", "pre", "rep")), Z.comp(lits=lits[:100], seqs=same, modes=("rle",) * 3, nseq_form=2)]
    frame, content, _ = Z.compose(blocks, window_log=17)
    t, q = oracle.zstd_seq_tables(frame, with_sequences=True)
    ref = oracle.zstd_sequences(frame)
    assert t.size == len(content) == ref.size and all(np.array_equal(getattr(q, k), getattr(ref, k)) for k in ("block", "pos", "ll", "ml", "distance", "offset_value"))
    assert np.array_equal(oracle.zstd_seq_tables(frame).mode, t.mode)
    assert t.block_type.tolist() == [0, 2, 1, 2, 2, 2] and t.n_sequences.tolist() == [0, 200, 0, 0, 9, 5]
    assert t.nseq_header_bytes.tolist() == [0, 2, 0, 1, 1, 2] and t.section_bytes[3] == 1 and t.bitstream_bytes[3] == 0
    assert t.mode.tolist() == [[0] * 3, [2, 0, 0], [0] * 3, [0] * 3, [3, 0, 3], [1, 1, 1]]
    desc = Z.fse_describe(counts, 7)
    assert t.desc_bytes.tolist() == [[0] * 3, [len(desc), 0, 0], [0] * 3, [0] * 3, [0] * 3, [1, 1, 1]]
    assert t.accuracy_log.tolist()[1] == [7, 5, 6] and t.accuracy_log.tolist()[4] == [7, 5, 6] and t.accuracy_log.tolist()[5] == [0, 0, 0]
    for b in (1, 4):                                                   # Repeat_Mode lists the table it repeats
        assert t.norm[b][0].tolist() == list(counts) + [0] * (64 - len(counts))
        assert t.norm[b][1].tolist() == list(Q.PRE[1][0]) and t.norm[b][2].tolist() == list(Q.PRE[2][0])
    assert t.rle_symbol[5].tolist() == [4, 5, 3] and not t.norm[5].any()
    o = int(t.section_offset[1])
    assert frame[o:o + 3] == bytes([128, 200, 2 << 6]) and frame[o + 3:o + 3 + len(desc)] == desc
    assert frame[int(t.section_offset[5]):][:6] == bytes([128, 5, 0x54, 4, 5, 3]) and t.section_offset[5] + t.section_bytes[5] == len(frame)
    for b in (1, 4, 5):
        assert t.nseq_header_bytes[b] + 1 + t.desc_bytes[b].sum() + t.bitstream_bytes[b] == t.section_bytes[b]
        assert t.bits_consumed[b] == t.marker_bit[b] and 8 * (t.bitstream_bytes[b] - 1) <= t.marker_bit[b] < 8 * t.bitstream_bytes[b]
        blk = [x for x in Q.blocks_of(oracle, frame) if x.b == b][0]
        for k in range(3):                                            # the final states decode the last sequence's codes
            if t.accuracy_log[b][k]:
                assert Q.decode_table(t.norm[b][k].tolist(), int(t.accuracy_log[b][k]))[0][int(t.final_state[b][k])] == blk.codes[k][-1]
        assert sum(Q.model_bits(blk)[0]) + Q.model_bits(blk)[1] == t.marker_bit[b]


# ---- the host build, cell by cell -------------------------------------------------------------------------------------------------------------
def _sections(rng):
    """(name, ll, ml, ofv, decodes): sequence lists whose histograms sit in every cell."""
    out = []
    sp, lf = Q.spread, Q.lists_from

    def add(name, llc, ofc, mlc, decodes=True):
        out.append((name, *lf(rng, llc, ofc, mlc), decodes))

    def drawn(n, lls, ofs, mls, skew=2.0):
        pick = lambda a: np.asarray(a)[np.minimum((rng.random(n) ** skew * len(a)).astype(int), len(a) - 1)]
        return pick(lls), pick(ofs), pick(mls)
    for n in Q.COUNTS + (3000,):
        add("count n%d" % n, *drawn(n, range(0, 21), range(2, 13), range(0, 41)))
    for n in (0x7EFF, 0x7F00, 0x7F01):                                 # (three bytes and a little more a sequence: the block is 128 KiB at most)
        add("count %#x" % n, *drawn(n, (0, 1), (2, 3, 4, 5), (0, 1), skew=3.0))
    one = lambda n, v: np.full(n, v, dtype=np.int64)
    add("codes 1 / all three RLE", one(40, 7), one(40, 9), one(40, 12))
    add("codes 2 equal / exact sum", sp(rng, {3: 16, 9: 16}), sp(rng, {6: 16, 7: 16}), sp(rng, {5: 16, 30: 16}))
    add("codes 2 skewed", sp(rng, {3: 60, 9: 4}), sp(rng, {6: 61, 7: 3}), sp(rng, {5: 63, 30: 1}))
    add("codes 3 to 8", sp(rng, {0: 30, 1: 20, 2: 10, 20: 4}), sp(rng, {4: 40, 5: 20, 12: 4}), sp(rng, {1: 20, 2: 20, 3: 10, 4: 5, 5: 5, 40: 4}))
    add("codes over 16 / largest", sp(rng, {c: 2 + c % 3 for c in range(0, 30)}), sp(rng, {c: 5 for c in range(2, 20)}),
        sp(rng, {c: 2 for c in range(0, 45)}))
    add("norm topup, a tie", sp(rng, {2: 20, 5: 20, 9: 10}), sp(rng, {3: 20, 4: 20, 8: 10}), sp(rng, {4: 20, 6: 20, 33: 10}))
    add("norm takedown", sp(rng, {1: 2040, 17: 1, 18: 1, 20: 1, 22: 1, 23: 1, 24: 1, 25: 1, 26: 1}), sp(rng, {5: 2044, 2: 1, 9: 1, 11: 1, 13: 1}),
        sp(rng, {5: 2040, 33: 1, 34: 1, 35: 1, 36: 1, 37: 1, 38: 1, 39: 1, 40: 1}))
    add("outcome predefined kept", np.array([0, 5, 9]), np.array([4, 5, 6]), np.array([2, 3, 7]))
    add("range LL", sp(rng, {c: 1 for c in [0] + list(range(16, 35))}), one(20, 8), one(20, 4))
    add("range ML 31..50", one(20, 2), one(20, 8), sp(rng, {c: 1 for c in range(31, 51)}))
    add("range ML 51", one(2, 2), one(2, 8), np.array([51, 50]))
    add("range OF 2..19", one(36, 3), sp(rng, {c: 2 for c in range(2, 20)}), one(36, 4))
    # the repeat codes, with and without literals in front (the offsets they stand for stay far from 1)
    seqs = [(5, 10, 103), (2, 10, 203), (2, 10, 303), (0, 10, 1), (3, 10, 1), (0, 10, 2), (3, 10, 2), (0, 10, 3), (3, 10, 3)]
    out.append(("range OF 0 and 1",) + tuple(np.array(v) for v in zip(*seqs)) + (True,))
    add("range OF 20..28 (not decoded: a gigabyte of history)", one(18, 3), sp(rng, {c: 2 for c in range(20, 29)}), one(18, 4), decodes=False)
    add("outcome predefined impossible: OF 29..31", one(12, 3), sp(rng, {29: 4, 30: 4, 31: 4}), one(12, 4), decodes=False)
    add("outcome predefined impossible, one code: OF 30", one(12, 3), one(12, 30), one(12, 4), decodes=False)
    return out


def _cost_tie(rng):
    """A histogram whose FSE cost equals its predefined cost, by search with the model."""
    for _ in range(200000):
        k = int(rng.integers(0, 3))
        n = int(rng.integers(8, 400))
        syms = rng.choice(Q.PRE[k][2] - 8, int(rng.integers(2, 5)), replace=False)
        codes = rng.choice(syms, n)
        h = np.bincount(codes, minlength=64)
        if (h > 0).sum() < 2:
            continue
        p = Q.plan_table(k, h, n)
        if p.cost_fse is not None and p.cost_fse == p.cost_pre:
            return k, codes, p
    raise AssertionError("no cost tie in 200000 draws")


def test_the_host_build_in_every_cell(emul, oracle, libzstd, capsys):
    rng = np.random.default_rng([Q.SEED, 12])
    modes_seen, rows = set(), []
    for name, ll, ml, ofv, decodes in _sections(rng):
        n = len(ll)
        cap = 64 * n + 1024
        out = ctypes.create_string_buffer(cap)
        got = emul.emul_write_sequences_x(ll.astype(np.uint16).tobytes(), ml.astype(np.uint16).tobytes(), ofv.astype(np.uint32).tobytes(), n, out, cap)
        prefix, plans = Q.model_prefix(ll, ml, ofv)
        assert prefix is not None and got > len(prefix), name
        section = out.raw[:got]
        modes_seen.add(section[1 if n < 128 else 2 if n < 0x7F00 else 3])
        if not decodes:
            assert section[:len(prefix)] == prefix, "%s: %s, the model's %s" % (name, section[:len(prefix)].hex(), prefix.hex())
            rows.append("%s: %d bytes, its %d of header and tables are the model's" % (name, got, len(prefix)))
            continue
        frame, content = Q.wrap_section(section, ll, ml, ofv, rng)
        P.check_decodes(oracle, frame, content)
        if libzstd is not None:
            buf = ctypes.create_string_buffer(len(content) + 64)
            r = libzstd.ZSTD_decompress(buf, len(content) + 64, frame, len(frame))
            assert r == len(content) and buf.raw[:r] == content, (name, r)
        blocks = Q.blocks_of(oracle, frame)
        assert len(blocks) == 1 and blocks[0].section == section, name
        blk = blocks[0]
        assert np.array_equal(blk.ll, ll) and np.array_equal(blk.ml, ml) and np.array_equal(blk.ofv, ofv), name
        Q.check_planner(blk, "lzx", plans)                           # 1 (its message names the table's cells)
        assert section[:len(prefix)] == prefix, name
        Q.check_form(blk)                                             # 2
        bits = Q.check_size(blk)                                      # 3
        _TALLY.add(blk, "lzx", plans, bits, name)
        # the in-block stage's writer on the same lists, where they are its kind: new offsets within 16 bits
        if (ofv > 3).all() and (ofv - 3 < 65536).all():
            got = emul.emul_write_sequences(ll.astype(np.uint16).tobytes(), ml.astype(np.uint16).tobytes(), (ofv - 3).astype(np.uint16).tobytes(), n, out, cap)
            assert got > 0, name
            frame1, content1 = Q.wrap_section(out.raw[:got], ll, ml, ofv, np.random.default_rng([Q.SEED, 13]))
            P.check_decodes(oracle, frame1, content1)
            b1 = Q.blocks_of(oracle, frame1)[0]
            assert b1.section[b1.hdr] == 0
            Q.check_planner(b1, "lz"); Q.check_form(b1); Q.check_size(b1)
            _TALLY.add(b1, "lz", [Q.plan_table(k, b1.hist[k], b1.nseq, "lz") for k in range(3)], None, name)
    # a cost tie keeps predefined
    k, codes, p = _cost_tie(rng)
    n = len(codes)
    cols = [np.full(n, 3), np.full(n, 8), np.full(n, 4)]
    cols[k] = codes
    ll, ml, ofv = Q.lists_from(rng, *cols)
    out = ctypes.create_string_buffer(64 * n + 1024)
    got = emul.emul_write_sequences_x(ll.astype(np.uint16).tobytes(), ml.astype(np.uint16).tobytes(), ofv.astype(np.uint32).tobytes(), n, out, 64 * n + 1024)
    assert p.mode == 0 and got > 0 and (out.raw[1 if n < 128 else 2] >> (6 - 2 * k)) & 3 == 0, "a cost tie (%d / 256 bit either way) did not keep predefined" % p.cost_pre
    assert out.raw[:got][:len(Q.model_prefix(ll, ml, ofv)[0])] == Q.model_prefix(ll, ml, ofv)[0]
    rows.append("cost tie: %s of %d sequences, %d / 256 bit by either mode: predefined kept" % (Q.KIND[k], n, p.cost_pre))
    # a cap too short returns 0: below the writer's floor, and where the bitstream runs out of room
    ll, ml, ofv = Q.lists_from(rng, np.full(1000, 20), rng.integers(8, 15, 1000), np.full(1000, 40))
    args = (ll.astype(np.uint16).tobytes(), ml.astype(np.uint16).tobytes(), ofv.astype(np.uint32).tobytes(), 1000)
    big = ctypes.create_string_buffer(70000)
    full = emul.emul_write_sequences_x(*args, big, 70000)
    assert full > 1000
    for cap in (0, 255, 256, 300, full - 40):
        assert emul.emul_write_sequences_x(*args, big, cap) == 0, cap
    assert emul.emul_write_sequences(ll.astype(np.uint16).tobytes(), ml.astype(np.uint16).tobytes(), np.full(1000, 300, np.uint16).tobytes(), 1000, big, 63) == 0
    assert emul.emul_write_sequences(ll.astype(np.uint16).tobytes(), ml.astype(np.uint16).tobytes(), np.full(1000, 300, np.uint16).tobytes(), 1000, big, 500) == 0
    assert len(modes_seen) >= 8
    with capsys.disabled():
        print("\nthe host build of the writers, cell by cell: %d sections, %d values of the modes byte" % (len(rows) + _TALLY.blocks["lzx"], len(modes_seen)))
        for r in rows:
            print("  " + r)


def test_no_histogram_reaches_the_second_repair():
    """400 000 histograms drawn under the planner's log rule: the round-robin repair of fse_normalize is reached by none (EXEMPT)."""
    _TALLY.searched = Q.search_round_robin(np.random.default_rng([Q.SEED, 14]), 400000)
    assert _TALLY.searched == (400000, 0)


# ---- the planned streams through the serial models ------------------------------------------------------------------------------------------------
def _model_frame(emul, c):
    cap = len(c.data) + len(c.data) // 64 + 4096
    out = ctypes.create_string_buffer(cap)
    if c.stage == "lz":
        n = emul.emul_zstd_compress_lz(c.data, len(c.data), min(c.bs, 32768), out, cap)
    else:
        even = len(set(np.diff(c.seams))) == 1 and c.seams[1] <= 65535     # the even split is the models' where the blocks are of one size
        n = emul.emul_zstd_compress_lzx(c.data, len(c.data), c.seams[1] if even else min(c.bs, 65535), c.wlog, out, cap, None)
    assert n > 0, (c.name, n)
    return out.raw[:n]


def test_the_planned_streams_through_the_serial_models(emul, oracle, capsys):
    """The three `tables` cases of lz_plan.py, the repeat-code and cap cases and the new streams through emul_zstd_compress_lzx, the
    in-block cases through emul_zstd_compress_lz: every frame decodes, every block passes checks 1 to 4."""
    bad, n, names = [], 0, set()
    for seed in Q.SEEDS:
        for c in Q.all_cases(seed):
            if c.stage == "lz" and seed != Q.SEEDS[0] and c.cls != "seq":
                continue                                              # (the in-block stage has no planner to vary with the seed)
            frame = _model_frame(emul, c)
            P.check_decodes(oracle, frame, c.data)
            bad += ["%s seed %d: %s" % (c.name, seed, b) for b in Q.check_frame(oracle, emul, frame, c.stage, _TALLY, c.name)]
            n += 1; names.add(c.name)
    assert {"lzx.tables.one_code_each", "lzx.tables.few_sequences", "lzx.tables.varied_thousands"} <= names
    with capsys.disabled():
        print("\n  %d frames of the serial models, %d failures" % (n, len(bad)))
    assert not bad, "\n".join(bad[:20])


# ---- sections composed to be wrong ----------------------------------------------------------------------------------------------------------------------
def test_the_checks_reject_composed_bad_sections(oracle, capsys):
    rng = np.random.default_rng([Q.SEED, 15])
    seen = {}

    def rejected(name, fn):
        with pytest.raises(Q.Reject) as e:
            fn()
        seen[name] = e.value.reason
        return e.value.reason

    def one_block(**kw):
        frame, content, _ = Z.compose([Z.raw(rng.integers(0, 256, 600, dtype=np.uint8).tobytes()), Z.comp(**kw)], window_log=17)
        P.check_decodes(oracle, frame, content)
        return frame, Q.blocks_of(oracle, frame)[0]

    def all_checks(blk, stage="lzx"):
        Q.check_planner(blk, stage); Q.check_form(blk); Q.check_size(blk)

    lits = rng.integers(0, 256, 400, dtype=np.uint8).tobytes()
    # a section the model agrees with, composed from the model's own plan: every check passes
    seqs = [(3, 8, 200 + 3)] * 36 + [(3, 8, 20 + 3)] * 4
    rng.shuffle(seqs)
    seqs = [tuple(s) for s in seqs]
    hist = Q.hists_of(Q.codes_of(*zip(*[(a, b, c) for a, b, c in seqs])))
    plans = [Q.plan_table(k, hist[k], 40) for k in range(3)]
    assert [p.mode for p in plans] == [1, 2, 1] and plans[1].log == 6
    cut = lambda norm: list(norm[:max(s for s in range(64) if norm[s]) + 1])
    mode_of = lambda p: "pre" if p.mode == 0 else "rle" if p.mode == 1 else ("fse", cut(p.norm), p.log)
    good, blk = one_block(lits=lits, seqs=seqs, modes=tuple(mode_of(p) for p in plans))
    all_checks(blk)
    # 1. a long-form count below 128
    _, blk = one_block(lits=lits, seqs=seqs, modes=tuple(mode_of(p) for p in plans), nseq_form=2)
    assert rejected("a two-byte Number_of_Sequences of 40", lambda: all_checks(blk)) == "form: count form"
    # 2. FSE where predefined is cheaper by the model
    few = [(3, 8, 200 + 3), (3, 8, 20 + 3), (3, 8, 200 + 3)]
    p = Q.plan_table(1, Q.hists_of(Q.codes_of(*zip(*few)))[1], 3)
    assert p.mode == 0 and p.cost_fse > p.cost_pre
    _, blk = one_block(lits=lits, seqs=few, modes=("rle", ("fse", cut(p.fse_norm), p.fse_log), "rle"))
    assert rejected("FSE_Compressed where predefined is cheaper", lambda: all_checks(blk)) == "planner: mode"
    # 3. an Accuracy_Log one too high
    up, _ = Q.normalise(hist[1], 40, 7)
    _, blk = one_block(lits=lits, seqs=seqs, modes=("rle", ("fse", cut(up), 7), "rle"))
    assert rejected("an Accuracy_Log of 7 for 40 sequences", lambda: all_checks(blk)) == "planner: accuracy log"
    # 4. a spare byte in front of the bitstream
    _, blk = one_block(lits=lits, seqs=seqs, modes=tuple(mode_of(pp) for pp in plans))
    at = blk.off + blk.hdr + 1 + sum(blk.desc_bytes)
    start = blk.off - (len(lits) + 2) - 3                              # the block header: 3 bytes in front of a two-byte Raw literals header
    size = int.from_bytes(good[start:start + 3], "little") >> 3
    assert size == 2 + len(lits) + blk.size
    fat = good[:start] + (1 | (2 << 1) | ((size + 1) << 3)).to_bytes(3, "little") + good[start + 3:at] + b"\x00" + good[at:]
    fblk = Q.blocks_of(oracle, fat)[0]
    assert fblk.size == blk.size + 1
    assert rejected("a spare byte in front of the bitstream", lambda: all_checks(fblk)) == "form: unread bits"
    assert rejected("the same, by its size", lambda: Q.check_size(fblk)) == "size"
    # 5. a block larger than its literal-only twin
    data = rng.integers(0, 256, 100, dtype=np.uint8).tobytes()
    twin, _, _ = Z.compose([Z.comp(lits=data)], window_log=10)
    fatter, _, _ = Z.compose([Z.comp(lits=data, lit_fmt=3)], window_log=10)
    assert rejected("a block one byte larger than its literal-only twin", lambda: Q.check_economy(oracle.zstd_literals(fatter), oracle.zstd_literals(twin))) == "larger block"
    Q.check_economy(oracle.zstd_literals(twin), oracle.zstd_literals(twin))
    # and what the model does not look at: a table repeated from the block in front, a table in the in-block stage's frame
    f2, c2, _ = Z.compose([Z.raw(lits), Z.comp(lits=lits, seqs=seqs, modes=tuple(mode_of(pp) for pp in plans)), Z.comp(lits=lits, seqs=seqs, modes=("rep",) * 3)], window_log=17)
    P.check_decodes(oracle, f2, c2)
    assert rejected("Repeat_Mode", lambda: Q.check_form(Q.blocks_of(oracle, f2)[1])) == "form: repeat mode"
    assert rejected("a table of its own in the in-block stage", lambda: Q.check_planner(Q.blocks_of(oracle, good)[0], "lz")) == "planner: mode"
    with capsys.disabled():
        print("\ncomposed bad sections, and what rejected them:")
        for k, v in seen.items():
            print("  %-52s %s" % (k, v))
    assert len(set(seen.values())) == 7


def test_coverage_table(emul, oracle, libzstd, capsys):
    """Printed last: what the host build and the serial models reached.  The floor here is the host build's: every cell, but for the
    three no sequence list can show (lengths beyond 16 bits, the second repair)."""
    with capsys.disabled():
        print("\n" + _TALLY.table("host build and serial models"))
    if _TALLY.blocks["lzx"]:
        left = [c for c in _TALLY.empty_cells()]
        assert not left, left
        shown = [c for c in Q.EXEMPT if _TALLY.cell[c][0]]
        assert shown == [("count", "three_byte_form")], shown      # (what is not decoded is not listed: Offset codes of 20 and more)
