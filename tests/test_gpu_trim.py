"""GPU tests of quality trimming (naf_gpu_unnaf_trim, naf_gpu_unnaf_select_reads, unnaf --trim).  Expected rows never come from the code
under test: they are what trim_plan.model gives for the quality lines of the oracle's --fastq text of the same archive, and the expected
texts are cut out of that text.  Every planned text is swept in the oracle's archive and, without the reads the tolerant parser does
not take (empty ones, codes outside 33..126), in this library's own ennaf at level 1."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import trim_plan as TP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_FORMAT, E_CAP, E_ARG = -4, -6, -8
CASES = [c.name for c in TP.planned(0)]
TRACE = re.compile(r"\[trim\] records (\d+) kept (\d+) pieces (\d+) quality bytes decoded (\d+) of (\d+) open tiles (\d+)\n")
Q20, Q13 = TP.LIMITS["Q20"], TP.LIMITS["Q13"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


class Archive:
    def __init__(self, oracle, gpu, naf, ids):
        self.naf, self.ids = naf, ids
        self.h = oracle.parse_naf(naf)
        self.N = self.h.n_sequences
        self.text = oracle.unnaf(naf, oracle.MODE_FASTQ)
        self.quals = TP.quals_of(self.text, self.N)
        self.lens = [len(q) for q in self.quals]
        self.d_naf = gpu.to_device(naf)
        self._want = {}

    def want(self, limit, min_len=1, max_ee=TP.NO_MAX):
        """(rows, total) of the whole archive, computed once per question and left unchanged"""
        key = (limit, min_len, max_ee)
        if key not in self._want:
            rows, total = TP.model(self.quals, limit, min_len, max_ee)
            rows.setflags(write=False)
            self._want[key] = (rows, total)
        return self._want[key]

    def window(self, limit, first, count, min_len=1, max_ee=TP.NO_MAX):
        rows = self.want(limit, min_len, max_ee)[0][first:self.N if count is None else first + count]
        return rows, total_of(rows, self.lens)

    def expected(self, segments, fmt, line_length=0, strands=None):
        return TP.expected_text(self.text, self.N, segments, fmt, line_length, strands)


def total_of(rows, lens):
    kept = rows[rows["flags"] == TP.KEPT]
    return (len(rows), len(kept), sum(lens[int(r)] for r in rows["record"]), int((kept["end"] - kept["begin"]).sum()), int(kept["ee"].sum(dtype=np.uint64)),
            int((rows["flags"] & TP.SHORT != 0).sum()), int((rows["flags"] & TP.ERRORS != 0).sum()))


def total_tuple(t):
    return (int(t.reads), int(t.kept), int(t.bases), int(t.kept_bases), int(t.kept_ee), int(t.n_short), int(t.n_errors))


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive})"""
    out = {}
    for c in TP.planned(SEED):
        arc = {"oracle": Archive(oracle, gpu, oracle.ennaf(c.text, well_formed=True), c.ids)}
        assert arc["oracle"].quals == c.quals, c.name
        own, _ = gpu.ennaf(gpu.to_device(c.own_text), level=1)
        arc["own"] = Archive(oracle, gpu, own.cpu().numpy().tobytes(), [c.ids[k] for k in c.own_keep])
        assert arc["own"].quals == c.own_quals, c.name
        out[c.name] = (c, arc)
    return out


def differ(what, got, want, where):
    if got.tobytes() != want.tobytes():
        k = next((i for i in range(min(len(got), len(want))) if got[i].tobytes() != want[i].tobytes()), min(len(got), len(want)))
        raise AssertionError("%s %s: first difference at row %d of %d / %d: got %s, expected %s" % (what, where, k, len(got), len(want), got[k:k + 2].tolist(), want[k:k + 2].tolist()))


def check(gpu, A, limit, min_len=1, max_ee=None, first=0, count=None):
    rows_w, total_w = A.window(limit, first, count, min_len, TP.NO_MAX if max_ee is None else max_ee)
    where = "limit %d min_len %d max_ee %s records %d+%s" % (limit, min_len, max_ee, first, count)
    rows, total = gpu.unnaf_trim(A.d_naf, limit, min_len, max_ee, first, count)
    differ("rows", rows, rows_w, where)
    assert total_tuple(total) == total_w, where
    return rows


# ---- 1. the rows of the planned texts at every limit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_rows_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    A = arc[which]
    for lname, limit in TP.LIMITS.items():
        rows = check(gpu, A, limit)
        assert len(rows) == A.N and (rows["reserved"] == 0).all()
        if limit == TP.DESIGN and which == "oracle":                                    # the plants have the stretch they were planted to have
            for (cls, cell), v in c.cells.items():
                for r, claim in v:
                    assert claim is None or (int(rows[r]["begin"]), int(rows[r]["end"])) == claim, (cls, cell)
    check(gpu, A, Q20, 30, TP.ee_units("0.5"))
    check(gpu, A, TP.NONE, 100, TP.ee_units("2"))


def test_the_filters_at_the_planted_stretch(gpu, planned):
    c, arc = planned["seams"]
    A = arc["oracle"]
    r = c.filters
    b, e, ee = TP.stretch(A.quals[r], Q13)
    assert e - b == 50
    for min_len, max_ee, want in ((49, ee + 1, TP.KEPT), (50, ee, TP.KEPT), (51, ee, TP.SHORT), (50, ee - 1, TP.ERRORS), (51, ee - 1, TP.SHORT | TP.ERRORS), (50, 0, TP.ERRORS)):
        rows = check(gpu, A, Q13, min_len, max_ee, r - 2, 5)
        assert int(rows[2]["flags"]) == want and (int(rows[2]["begin"]), int(rows[2]["end"]), int(rows[2]["ee"])) == (b, e, ee)


# ---- 2. first and count: every record seam is the end of one sweep and the start of another -------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    c, arc = planned["seams"]
    A = arc[which]
    ends = c.ends if which == "oracle" else [c.own_keep.index(e) for e in c.ends]
    N = A.N
    runs = [(0, 1), (N - 1, 1), (N, 0), (N, None), (5, 0), (N // 2, None), (0, 2), (N - 2, 2)]
    for e in ends:
        runs += [(e - 1, 1), (e, 1), (e - 2, 2), (e, 3)]
    runs += [(0, ends[0]), (ends[-1], None)]
    empty = [r for r in range(N) if not A.quals[r]]
    assert bool(empty) == (which == "oracle")
    runs += [(r, 1) for r in empty] + ([(empty[1], 2), (empty[1] - 1, 4)] if empty else [])
    for first, count in runs:
        for limit in (Q13, TP.NONE):
            check(gpu, A, limit, 1, None, first, count)


# ---- 3. the piece size does not show ------------------------------------------------------------------------------------------------------
CHILD = """
import hashlib, sys
from naf_amd import capi
ctx = capi.Context(0)
for path in sys.argv[1:]:
    d = ctx.to_device(open(path, "rb").read())
    for limit, min_len, max_ee in ((%d, 1, None), (%d, 30, 1 << 31), (capi.TRIM_NONE, 1, None)):
        rows, t = ctx.unnaf_trim(d, limit, min_len, max_ee)
        print(len(rows), hashlib.sha256(rows.tobytes()).hexdigest(), t.reads, t.kept, t.bases, t.kept_bases, t.kept_ee, t.n_short, t.n_errors)
ctx.close()
""" % (Q13, Q20)


@pytest.mark.parametrize("piece", [1, 5000, 300000])
def test_the_result_does_not_depend_on_the_piece_size(planned, piece, tmp_path):
    """NAF_GPU_TRIM_PIECE is read when the library starts: a fresh process per value.  At 1 every read is a piece of its own (the short
    archives), at 5000 and 300000 the pieces end at reads in the middle of tiles."""
    env = dict(os.environ, NAF_GPU_TRIM_PIECE=str(piece), NAF_GPU_TRACE="1", PYTHONPATH=ROOT)
    arcs = [planned["long"][1]["own"], planned["bytes"][1]["oracle"]] + ([planned["seams"][1]["own"], planned["seams"][1]["oracle"]] if piece > 1 else [])
    for k, A in enumerate(arcs):
        (tmp_path / ("%d.naf" % k)).write_bytes(A.naf)
    p = subprocess.run([sys.executable, "-c", CHILD] + [str(tmp_path / ("%d.naf" % k)) for k in range(len(arcs))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().split("\n")
    tr = TRACE.findall(p.stderr.decode())
    assert len(tr) == 3 * len(arcs), p.stderr.decode()
    for k, A in enumerate(arcs):
        for j, (limit, min_len, max_ee) in enumerate(((Q13, 1, TP.NO_MAX), (Q20, 30, 1 << 31), (TP.NONE, 1, TP.NO_MAX))):
            rows, total = A.want(limit, min_len, max_ee)
            assert out[3 * k + j].split() == [str(x) for x in (len(rows), hashlib.sha256(rows.tobytes()).hexdigest()) + total], (k, j)
            R, K, pieces, dec, of, joined = (int(x) for x in tr[3 * k + j])
            assert (R, K, of) == (A.N, total[1], A.h.orig[5])
            assert (pieces == 1) if sum(A.lens) <= piece else (pieces >= 2), (k, piece, pieces)
            assert piece != 1 or pieces == A.N
    assert any(int(t[5]) > 0 for t in tr)                                              # reads that cross tiles were joined


# ---- 4. buffers ---------------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, limit, min_len, max_ee, first, count, d_rows, cap, total=True):
    from naf_amd import capi
    n, tot = C.c_uint64(12345), capi.TrimTotal()
    o = capi.TrimOpts(limit, min_len, max_ee)
    rc = gpu.L.naf_gpu_unnaf_trim(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), C.byref(o), first, capi.WHOLE if count is None else count,
                                  C.c_void_p(d_rows.data_ptr()) if d_rows is not None else None, cap, C.byref(n), C.byref(tot) if total else None)
    return rc, n.value, tot


def test_totals_only(gpu, planned):
    for name in CASES:
        A = planned[name][1]["own"]
        for limit in (Q13, TP.NONE):
            rows, total = gpu.unnaf_trim(A.d_naf, limit, 20, TP.ee_units("1"), out=False)
            assert rows is None and total_tuple(total) == A.want(limit, 20, TP.ee_units("1"))[1]
        rc, n, tot = raw(gpu, A.d_naf, Q13, 1, TP.NO_MAX, 0, 2, None, 0, total=False)
        assert rc == 0 and n == 2


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    arena = fenced.Arena("cuda", salt=0x77, size=8 << 20)
    for name in ("seams", "long"):
        A = planned[name][1][which]
        rows_w, total_w = A.want(Q13)
        n = len(rows_w)
        for phase in (0, 1, 31):
            arena.reset()
            d_rows = arena.out(40 * n, phase)                                            # exactly enough: 40 bytes a row and nothing outside them
            rc, got, tot = raw(gpu, A.d_naf, Q13, 1, TP.NO_MAX, 0, None, d_rows, n, total=phase != 1)
            torch.cuda.synchronize()
            assert rc == 0 and got == n
            arena.check()
            assert d_rows.cpu().numpy().tobytes() == rows_w.tobytes(), (name, phase)
            assert phase == 1 or total_tuple(tot) == total_w
        arena.reset()                                                                   # one row too few: the whole count, nothing written
        d_rows = arena.out(40 * (n - 1), 5)
        before = d_rows.clone()
        rc, got, tot = raw(gpu, A.d_naf, Q13, 1, TP.NO_MAX, 0, None, d_rows, n - 1)
        torch.cuda.synchronize()
        assert rc == E_CAP and got == n and torch.equal(d_rows, before) and "rows" in gpu.L.naf_gpu_last_error(gpu.h).decode()
        arena.check()
        arena.reset()                                                                   # a window into a table of its own size
        d_rows = arena.out(40 * 7, 31)
        rc, got, tot = raw(gpu, A.d_naf, Q13, 1, TP.NO_MAX, 3, 7, d_rows, 7)
        torch.cuda.synchronize()
        assert rc == 0 and got == 7 and d_rows.cpu().numpy().tobytes() == rows_w[3:10].tobytes()
        arena.check()
    A = planned["bytes"][1]["oracle"]                                                   # the archive in an arena, other bytes around it
    for run, in_phase in ((0, 0), (1, 1), (0, 65)):
        arena.reset()
        before, after = fenced.stream_bait(A.naf, run)
        d_in = arena.put(A.naf, in_phase, before, after)
        d_rows = arena.out(40 * A.N, 9)
        rc, got, tot = raw(gpu, d_in, Q20, 1, TP.NO_MAX, 0, None, d_rows, A.N)
        torch.cuda.synchronize()
        assert rc == 0 and d_rows.cpu().numpy().tobytes() == A.want(Q20)[0].tobytes()
        arena.check()
    from naf_amd import capi                                                            # the binding's own form with the caller's buffer
    A = planned["long"][1][which]
    buf = torch.zeros(40 * A.N + 40, dtype=torch.uint8, device="cuda")
    view, tot = gpu.unnaf_trim(A.d_naf, Q13, out=buf)
    assert view.numel() == 40 * A.N and not bool(buf[40 * A.N:].any()) and view.cpu().numpy().tobytes() == A.want(Q13)[0].tobytes()
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_trim(A.d_naf, Q13, out=buf[:40 * (A.N - 1)])
    assert e.value.code == E_CAP


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    import torch
    A = planned["long"][1]["own"]
    N = A.N

    def fails(d_naf, code, limit=Q20, min_len=1, first=0, count=None, words=()):
        buf = torch.zeros(40 * 64, dtype=torch.uint8, device="cuda")
        rc, n, tot = raw(gpu, d_naf, limit, min_len, TP.NO_MAX, first, count, buf, 64)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == code and n == 0 and not bool(buf.any()) and total_tuple(tot) == (0,) * 7, (rc, msg)
        for w in words:
            assert w in msg, msg

    fails(A.d_naf, E_ARG, limit=0, words=("limit",))
    fails(A.d_naf, E_ARG, limit=2 ** 32 + 1, words=("limit", str(2 ** 32 + 1)))
    fails(A.d_naf, E_ARG, limit=2 ** 64 - 2, words=("limit",))
    fails(A.d_naf, E_ARG, min_len=0, words=("min_len",))
    fails(A.d_naf, E_ARG, first=N + 1, words=("record", str(N + 1)))
    fails(A.d_naf, E_ARG, first=1, count=N, words=("records", str(N)))
    for name in ("acgt_10k", "protein_small"):
        fails(gpu.to_device(golden_bytes("naf", name + ".naf")), E_ARG, words=("no quality",))
    fails(gpu.to_device(short_quality_archive(oracle)), E_FORMAT, words=("corrupted quality",))
    check(gpu, A, 2 ** 32)                                                              # the largest limit there is
    check(gpu, A, 1)


def short_quality_archive(oracle):
    """An archive whose quality section is three codes shorter than its bases: the oracle's archive of a small FASTQ with its last
    section -- the quality: its two sizes, then its frame without the magic -- written again from fewer bytes."""
    naf = oracle.ennaf(b"@a x\nACGTAC\n+\nIIIIII\n@b\nACGT\n+\n5555\n")
    h = oracle.parse_naf(naf)
    assert h.flags & 1 and h.orig[5] == 10 == h.orig[4]
    start = h.payload_off[5] - len(vle(oracle, h.orig[5])) - len(vle(oracle, h.comp[5]))
    assert h.payload_off[5] + h.comp[5] == len(naf) and naf[start:h.payload_off[5]] == vle(oracle, h.orig[5]) + vle(oracle, h.comp[5])
    frame = oracle.zstd_store_raw(b"IIIIII5")
    out = naf[:start] + vle(oracle, 7) + vle(oracle, len(frame) - 4) + frame[4:]
    h2 = oracle.parse_naf(out)
    assert h2.n_sequences == 2 and h2.orig[5] == 7 and h2.orig[4] == 10
    return out


def vle(oracle, v):
    buf = C.create_string_buffer(16)
    n = oracle.lib().nafo_vle_write(v, buf)
    return buf.raw[:n]


# ---- 6. against the quality statistics, and the same bytes on every run ------------------------------------------------------------------------
def test_untrimmed_rows_carry_the_ee_of_the_quality_rows(gpu, planned):
    from naf_amd import capi
    for name in CASES:
        for which, A in planned[name][1].items():
            rows, total = gpu.unnaf_trim(A.d_naf, capi.TRIM_NONE)
            rec, _, _, qt = gpu.unnaf_quality(A.d_naf)
            assert (rows["ee"] == rec["ee"]).all() and (rows["end"] == rec["n"]).all() and not rows["begin"].any() and (rows["record"] == rec["key"]).all()
            assert int(total.kept_ee) == int(qt.ee) and int(total.bases) == int(qt.n) == int(total.kept_bases)


def test_two_calls_give_identical_bytes(gpu, planned, monkeypatch, capfd):
    from naf_amd import capi
    A = planned["seams"][1]["own"]
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    a, ta = gpu.unnaf_trim(A.d_naf, Q13)
    tr = TRACE.findall(capfd.readouterr().err)
    monkeypatch.delenv("NAF_GPU_TRACE")
    gpu.unnaf(planned["bytes"][1]["oracle"].d_naf, capi.OUT_FASTQ)                      # an unrelated call on the same context in between
    b, tb = gpu.unnaf_trim(A.d_naf, Q13)
    want, total = A.want(Q13)
    assert a.tobytes() == b.tobytes() == want.tobytes() and total_tuple(ta) == total_tuple(tb) == total
    assert len(tr) == 1 and (int(tr[0][0]), int(tr[0][1]), int(tr[0][2])) == (A.N, total[1], 1) and int(tr[0][3]) == int(tr[0][4]) == A.h.orig[5] and int(tr[0][5]) > 0


# ---- 7. the trimmed reads -------------------------------------------------------------------------------------------------------------------
def text_of(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_select_reads_writes_the_kept_stretches(gpu, planned, which):
    from naf_amd import capi
    for name, limit, min_len in (("seams", Q13, 1), ("long", Q20, 1000), ("bytes", Q20, 1)):
        A = planned[name][1][which]
        rows, _ = gpu.unnaf_trim(A.d_naf, limit, min_len)
        segs = capi.trim_to_segments(rows)
        assert segs == TP.kept_segments(A.want(limit, min_len)[0]) and len(segs) >= 2 and any(b > 0 or e < A.lens[r] for r, b, e in segs)
        for fmt, out_type, L in (("fastq", capi.OUT_FASTQ, -1), ("fasta", capi.OUT_FASTA, 0), ("fasta", capi.OUT_FASTA, 1), ("fasta", capi.OUT_FASTA, 60),
                                 ("sequences", capi.OUT_SEQUENCES, -1), ("seq", capi.OUT_SEQ, -1)):
            if name == "long" and L == 1:
                continue
            want = A.expected(segs, fmt, max(L, 0))
            got = text_of(gpu.unnaf_select_reads(A.d_naf, segs, out_type, line_length=L))
            assert got == want, (name, fmt, L, len(got), len(want))
            assert gpu.unnaf_select_reads_size(A.d_naf, segs, out_type, line_length=L) == len(want)


def test_select_reads_on_the_reverse_strand(gpu, planned):
    from naf_amd import capi
    A = planned["seams"][1]["own"]
    segs = TP.kept_segments(A.want(Q13)[0])
    pick = segs[::7] + segs[:40]
    strands = [k % 3 != 1 for k in range(len(pick))]
    four = [(r, b, e, int(s)) for (r, b, e), s in zip(pick, strands)]
    for fmt, out_type, L in (("fastq", capi.OUT_FASTQ, -1), ("fasta", capi.OUT_FASTA, 60), ("sequences", capi.OUT_SEQUENCES, -1), ("seq", capi.OUT_SEQ, -1)):
        assert text_of(gpu.unnaf_select_reads(A.d_naf, four, out_type, line_length=L)) == A.expected(pick, fmt, max(L, 0), strands), fmt
    got = text_of(gpu.unnaf_select_reads(A.d_naf, [(pick[0][0], pick[0][1], pick[0][2], 1)], capi.OUT_FASTQ)).split(b"\n")
    r, b, e = pick[0]
    assert got[0] == b"@%s/rc w" % A.ids[r].encode() and got[3] == A.quals[r][b:e][::-1] and len(got[1]) == e - b


def test_whole_records_are_the_selection_s_bytes(gpu, planned):
    from naf_amd import capi
    A = planned["long"][1]["own"]
    recs = [0, 3, A.N - 1, 3, 7]
    for out_type in (capi.OUT_FASTQ, capi.OUT_FASTA, capi.OUT_SEQUENCES, capi.OUT_SEQ):
        for segs in (recs, [(r, 0, capi.WHOLE) for r in recs], [(r, 0, capi.WHOLE, k % 2) for k, r in enumerate(recs)]):
            assert text_of(gpu.unnaf_select_reads(A.d_naf, segs, out_type)) == text_of(gpu.unnaf_select(A.d_naf, segs, out_type)), (out_type, segs[:2])
    explicit = [(r, 0, A.lens[r]) for r in recs]                                        # begin and end spelled out: the same read
    assert text_of(gpu.unnaf_select_reads(A.d_naf, explicit, capi.OUT_FASTQ)) == text_of(gpu.unnaf_select(A.d_naf, recs, capi.OUT_FASTQ))
    assert text_of(gpu.unnaf_select_reads(A.d_naf, [], capi.OUT_FASTQ)) == b""


def test_the_other_selections_keep_their_refusals(gpu, planned):
    from naf_amd import capi
    A = planned["long"][1]["own"]
    for segs in ([(1, 2, 9)], [(1, 2, 9, 1)], [0, (1, 2, 9)]):
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_select(A.d_naf, segs, capi.OUT_FASTQ)
        assert e.value.code == E_ARG and "no FASTQ form" in e.value.msg
    assert text_of(gpu.unnaf_select(A.d_naf, [(1, 2, 9)], capi.OUT_FASTA, line_length=0)).startswith(b">%s:3-9\n" % A.ids[1].encode())
    for segs, word in (([(1, 9, 9)], "select nothing"), ([(1, A.lens[1], capi.WHOLE - 1)], "select nothing"), ([(A.N, 0, 5)], "not in the archive")):
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_select_reads(A.d_naf, segs, capi.OUT_FASTQ)
        assert e.value.code == E_ARG and word in e.value.msg
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_select_reads(A.d_naf, [(1, 2, 9)], capi.OUT_4BIT)
    assert e.value.code == E_ARG


def test_five_thousand_one_base_reads_in_one_call(gpu, planned):
    from naf_amd import capi
    A = planned["seams"][1]["own"]
    rng = np.random.default_rng(77 + SEED)
    full = [r for r in range(A.N) if A.lens[r]]
    segs = []
    for r in rng.choice(full, 5000):
        b = int(rng.integers(0, A.lens[int(r)]))
        segs.append((int(r), b, b + 1))
    assert text_of(gpu.unnaf_select_reads(A.d_naf, segs, capi.OUT_FASTQ)) == A.expected(segs, "fastq")
    assert text_of(gpu.unnaf_select_reads(A.d_naf, segs, capi.OUT_SEQ)) == A.expected(segs, "seq")


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_trim_writes_the_reads_and_the_table(gpu, planned):
    A = planned["seams"][1]["own"]
    p = unnaf_cli(["--trim", "13"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == A.expected(TP.kept_segments(A.want(Q13)[0]), "fastq")
    half, one = TP.ee_units("0.5"), TP.ee_units("1")
    p = unnaf_cli(["--trim", "20", "--min-length", "30", "--max-ee", "0.5", "--fasta", "--line-length", "60"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == A.expected(TP.kept_segments(A.want(Q20, 30, half)[0]), "fasta", 60)
    p = unnaf_cli(["--trim", "none", "--max-ee", "1", "--sequences"], A.naf)
    assert p.returncode == 0 and p.stdout == A.expected(TP.kept_segments(A.want(TP.NONE, 1, one)[0]), "sequences")
    p = unnaf_cli(["--trim", "30", "--seq", "--records", "10-400"], A.naf)
    assert p.returncode == 0 and p.stdout == A.expected(TP.kept_segments(A.want(TP.LIMITS["Q30"])[0][9:400]), "seq")
    p = unnaf_cli(["--trim", "13", "--trim-table"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.table(A.want(Q13)[0], A.ids, A.lens)
    p = unnaf_cli(["--trim", "13", "--trim-table", "--min-length", "30", "--max-ee", "0.5", "--records", "3-900"], A.naf)
    assert p.returncode == 0 and p.stdout == TP.table(A.want(Q13, 30, half)[0][2:900], A.ids, A.lens)
    statuses = set(line.split(b"\t")[-1] for line in p.stdout.split(b"\n")[1:-1])
    assert statuses == {b"kept", b"short", b"errors", b"short,errors"}
    r = 17
    p = unnaf_cli(["--trim", "13", "--trim-table", "--region", A.ids[r]], A.naf)
    assert p.returncode == 0 and p.stdout == TP.table(A.want(Q13)[0][r:r + 1], A.ids, A.lens)
    for args in (["--trim", "20", "--region", "nosuch"], ["--trim", "20", "--records", "1-99999"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    O = planned["bytes"][1]["oracle"]                                                   # the read of all byte values, under its own header
    p = unnaf_cli(["--trim", "2"], O.naf)
    assert p.returncode == 0 and p.stdout == O.expected(TP.kept_segments(O.want(TP.LIMITS["Q2"])[0]), "fastq")
    p = unnaf_cli(["--trim", "20"], golden_bytes("naf", "acgt_10k.naf"))
    assert p.returncode == 1 and b"no quality" in p.stderr and p.stdout == b""
