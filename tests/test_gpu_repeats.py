"""GPU tests of the tandem-repeat table (naf_gpu_unnaf_repeats_count, naf_gpu_unnaf_repeats, unnaf --repeats).  Expected rows never come from
the code under test: they are what repeats_plan.expected_repeats -- numpy over the oracle's --sequences text of the same archive -- gives.
Every planned text is asked in two archives, the oracle's and this library's own ennaf at level 1 (the empty text: the oracle's only); the
reference-made golden archives repeat_l19 and repeat_long27 (frames whose blocks depend on each other) take the whole-decode fallback."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import repeats_plan as RP
import runs_plan
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
CASES = [c.name for c in RP.planned(0)]
GOLDEN_REPEATS = ("repeat_l19", "repeat_long27")
TRACE = re.compile(r"\[repeats\] rows (\d+) candidates (\d+) periods (\d+) pieces (\d+) sequence bytes decoded (\d+) of (\d+)\n")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


class Archive:
    def __init__(self, oracle, gpu, naf):
        self.naf = naf
        self.h = oracle.parse_naf(naf)
        self.lines = RP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), self.h.n_sequences)
        self.d_naf = gpu.to_device(naf)
        self._base, self._want = {}, {}

    def want(self, spec, min_len=1, whole=False, first=0, count=None):
        """expected rows, computed once per question and left unchanged"""
        key = (tuple(spec), min_len, whole, first, count)
        if key not in self._want:
            bk = (tuple(spec), first, count)
            if bk not in self._base:
                self._base[bk] = RP.base_rows(self.lines, spec, first, count)
            rows = RP.filter_rows(self._base[bk], min_len, whole)
            rows.setflags(write=False)
            self._want[key] = rows
        return self._want[key]


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive}); the two archives of a text hold the same lines"""
    out = {}
    for c in RP.planned(SEED):
        arc = {"oracle": Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type, well_formed=c.well_formed))}
        assert arc["oracle"].lines == c.lines, c.name
        if c.text:
            own, _ = gpu.ennaf(gpu.to_device(c.own_text), seq_type=c.seq_type, level=1)
            arc["own"] = Archive(oracle, gpu, own.cpu().numpy().tobytes())
            if c.own_text is c.text:
                assert arc["own"].lines == arc["oracle"].lines, c.name
                arc["own"]._base, arc["own"]._want = arc["oracle"]._base, arc["oracle"]._want
            else:
                assert arc["own"].lines == [ln for ln in c.lines if ln], c.name     # (the read of no bases is not in it)
        out[c.name] = (c, arc)
    return out


@pytest.fixture(scope="module")
def golden(oracle, gpu):
    return {name: Archive(oracle, gpu, golden_bytes("naf", name + ".naf")) for name in GOLDEN_REPEATS}


def per_period_of(want):
    return [int((want["period"] == p).sum()) for p in range(1, 17)]


def check(gpu, A, spec, min_len=1, whole=False, first=0, count=None, counts=True):
    """the rows byte for byte, the sum of their lengths, the rows per period, and the counting call"""
    want = A.want(spec, min_len, whole, first, count)
    rows, n_bases, per = gpu.unnaf_repeats(A.d_naf, list(spec), min_len, whole, first, count)
    if rows.tobytes() != want.tobytes():
        k = next((i for i in range(min(len(rows), len(want))) if rows[i].tobytes() != want[i].tobytes()), min(len(rows), len(want)))
        raise AssertionError("%s min_len %d whole %s records %d+%s: first difference at row %d of %d / %d: got %s, expected %s" % (
            RP.spec_text(spec), min_len, whole, first, count, k, len(rows), len(want), RP.as_tuples(rows[k:k + 2]), RP.as_tuples(want[k:k + 2])))
    total = int((want["end"] - want["begin"]).sum())
    assert n_bases == total and per == per_period_of(want)
    if counts:
        assert gpu.unnaf_repeats_count(A.d_naf, list(spec), min_len, whole, first, count) == (len(want), total, per_period_of(want))
    return rows


# ---- 1. the rows and the counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_rows_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    if which not in arc:
        assert name == "no_records"
        return
    A = arc[which]
    n = 0
    for spec in c.specs:
        for m in RP.MIN_LENS:
            for whole in (False, True):
                n += len(check(gpu, A, spec, m, whole))
    assert (n > 0) == (name != "no_records")
    have = {t[:3] + (t[4],) for t in RP.as_tuples(arc["oracle"].want(RP.ALL2))}
    assert all(x in have for x in c.plants) and not any(x in have for x in c.absent)


# ---- 2. first and count ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    for name in ("lengths", "seams"):
        c, arc = planned[name]
        A = arc[which]
        N = len(A.lines)
        empty = [r for r in range(N) if not A.lines[r]]
        assert len(empty) >= 5
        allrows = A.want(RP.ALL2)
        for r in range(N):                                                          # every record alone: its two ends are the sweep's
            rows = check(gpu, A, RP.ALL2, 1, False, r, 1, counts=False)
            assert rows.tobytes() == allrows[allrows["record"] == r].tobytes()
        for spec, m, whole in ((RP.ALL2, 1, False), (RP.MISA, 12, True)):
            allrows = A.want(spec, m, whole)
            # windows that begin and end at empty records, single records around them, and empty windows
            for first, count in ((empty[0], empty[-1] + 1 - empty[0]), (empty[1], empty[2] - empty[1]), (empty[1], 1), (empty[1], empty[3] + 1 - empty[1]), (empty[1] - 1, 2),
                                 (empty[2] + 1, 1), (3, 9), (N - 1, 1), (5, 0), (N, 0), (N, None), (0, None)):
                rows = check(gpu, A, spec, m, whole, first, count)
                last = N if count is None else first + count
                assert rows.tobytes() == allrows[(allrows["record"] >= first) & (allrows["record"] < last)].tobytes()


# ---- 3. the whole-decode fallback -------------------------------------------------------------------------------------------------------
def traced(gpu, A, spec, min_len, whole, first, count, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    import torch
    n = len(A.want(spec, min_len, whole, first, count))
    buf = torch.zeros(max(32 * n, 1), dtype=torch.uint8, device="cuda")
    view, n_bases, per = gpu.unnaf_repeats(A.d_naf, list(spec), min_len, whole, first, count, out=buf)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = TRACE.findall(err)
    assert len(m) == 1, err
    return np.frombuffer(view.cpu().numpy().tobytes(), dtype=RP.REPEAT_DTYPE), [int(x) for x in m[0]]


@pytest.mark.parametrize("name", GOLDEN_REPEATS)
def test_rows_of_the_reference_made_archives(gpu, golden, name, monkeypatch, capfd):
    A = golden[name]
    for spec, m, whole in ((RP.ALL2, 1, False), (RP.ALL3, 12, True), (RP.MISA, 1, False), (RP.single(1, 3), 1, False)):
        check(gpu, A, spec, m, whole)
    assert len(A.want(RP.ALL2)) > 0
    last = max(r for r in range(len(A.lines)) if A.lines[r])
    got, tr = traced(gpu, A, RP.ALL2, 1, False, last, 1, monkeypatch, capfd)
    assert got.tobytes() == A.want(RP.ALL2, 1, False, last, 1).tobytes()
    assert tr[2] == 16 and tr[4] == tr[5] == (A.h.orig[4] + 1) // 2                  # dependent blocks: the whole stream, once


def test_a_restricted_query_decodes_only_the_blocks_behind_its_records(gpu, planned, monkeypatch, capfd):
    A = planned["seams"][1]["own"]
    T = (A.h.orig[4] + 1) // 2
    N = len(A.lines)
    for first, count in ((0, 3), (N // 2, 2), (N - 3, 3)):
        got, (R, K, P, pieces, D, Tt) = traced(gpu, A, RP.ALL3, 1, False, first, count, monkeypatch, capfd)
        assert got.tobytes() == A.want(RP.ALL3, 1, False, first, count).tobytes()
        assert (R, P, pieces, Tt) == (len(got), 16, 1, T) and 0 < D < T and K >= R > 0, (first, count, D, T)
    got, tr = traced(gpu, A, RP.MISA, 1, False, 0, None, monkeypatch, capfd)
    assert tr[2] == 6 and tr[4] == T


# ---- 4. the piece size does not show ----------------------------------------------------------------------------------------------------
CHILD = """
import hashlib, sys
from naf_amd import capi
ctx = capi.Context(0)
for path in sys.argv[2:]:
    d = ctx.to_device(open(path, "rb").read())
    for spec, m, whole in ((sys.argv[1], 1, False), ("misa", 12, True)):
        rows, nb, per = ctx.unnaf_repeats(d, spec, m, whole)
        print(len(rows), nb, hashlib.sha256(rows.tobytes()).hexdigest(), *per)
ctx.close()
"""


@pytest.mark.parametrize("piece", [1, 5000, 300000])
def test_the_result_does_not_depend_on_the_piece_size(planned, golden, piece, tmp_path):
    """NAF_GPU_REPEATS_PIECE is read when the library starts: a fresh process per value, which sweeps three archives."""
    env = dict(os.environ, NAF_GPU_REPEATS_PIECE=str(piece), NAF_GPU_TRACE="1", PYTHONPATH=ROOT)
    arcs = (planned["seams"][1]["own"], planned["lengths"][1]["oracle"], golden["repeat_l19"])
    for k, A in enumerate(arcs):
        (tmp_path / ("%d.naf" % k)).write_bytes(A.naf)
    p = subprocess.run([sys.executable, "-c", CHILD, RP.spec_text(RP.ALL2)] + [str(tmp_path / ("%d.naf" % k)) for k in range(len(arcs))], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().split("\n")
    tr = TRACE.findall(p.stderr.decode())
    assert len(tr) == 2 * len(arcs), p.stderr.decode()
    for k, A in enumerate(arcs):
        for j, (spec, m, whole) in enumerate(((RP.ALL2, 1, False), (RP.MISA, 12, True))):
            want = A.want(spec, m, whole)
            assert out[2 * k + j].split() == [str(x) for x in [len(want), int((want["end"] - want["begin"]).sum()), hashlib.sha256(want.tobytes()).hexdigest()] + per_period_of(want)]
            assert int(tr[2 * k + j][0]) == len(want)
        # the trace's piece count: one piece when the bases fit it, else several -- at piece = 1 one a record (the empty ones, too, are pieces)
        bases, pieces = sum(len(ln) for ln in A.lines), int(tr[2 * k][3])
        assert (pieces == 1) if bases <= piece else (pieces >= 2), (k, piece, pieces)
        assert piece != 1 or pieces >= sum(1 for ln in A.lines if ln)
    assert piece == 300000 or all(int(t[3]) >= 2 for t in tr)


def test_two_calls_give_identical_bytes(gpu, planned):
    for name, spec in (("seams", RP.ALL2), ("dense", RP.ALL2), ("fastq", RP.MISA)):
        A = planned[name][1]["own"]
        a = gpu.unnaf_repeats(A.d_naf, list(spec))[0]
        b = gpu.unnaf_repeats(A.d_naf, list(spec))[0]
        assert a.tobytes() == b.tobytes() == A.want(spec).tobytes()


# ---- 5. period 1 is the homopolymer table of runs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 10])
def test_period_one_lists_the_homopolymers_of_runs(gpu, planned, k):
    for name in ("seams", "unknown", "rna", "fastq", "dense"):
        A = planned[name][1]["own"]
        rows = check(gpu, A, RP.single(1, k), counts=False)
        runs, nb = gpu.unnaf_runs(A.d_naf, "ACGT", each=True, min_len=k)
        model = runs_plan.expected_runs(A.lines, runs_plan.set_of("ACGT"), True, k)
        for other in (runs, model):
            assert len(other) == len(rows) and all(np.array_equal(rows[f], other[f]) for f in ("record", "begin", "end")), name
        code_of = np.array([0, 3, 2, 0, 1, 0, 0, 0, 0], dtype=np.uint32)             # codes 1 T, 2 G, 4 C, 8 A -> the motif's two bits
        assert np.array_equal(code_of[runs["code"]], rows["motif"]) and nb == int((rows["end"] - rows["begin"]).sum())
        assert len(rows) > 0 or (k == 10 and name != "dense")                        # (a random background has hardly a homopolymer of ten)


# ---- 6. buffers ---------------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, spec, flags, min_len, first, count, d_rows, cap, extras=True):
    from naf_amd import capi
    sp = capi.RepeatSpec((C.c_uint32 * 16)(*spec)) if spec is not None else None
    n, nb, per = C.c_uint64(12345), C.c_uint64(777), (C.c_uint64 * 16)(*[99] * 16)
    rc = gpu.L.naf_gpu_unnaf_repeats(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), C.byref(sp) if sp is not None else None, flags, min_len, first,
                                     capi.WHOLE if count is None else count, C.c_void_p(d_rows.data_ptr() if d_rows is not None and d_rows.numel() else 0), cap,
                                     C.byref(n), C.byref(nb) if extras else None, per if extras else None)
    return rc, n.value, nb.value, [int(v) for v in per]


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x5B, size=8 << 20)
    for name, spec, m, whole in (("overlap", RP.ALL2, 1, False), ("seams", RP.ALL3, 1, True), ("dense", RP.ALL3, 12, False), ("fastq", RP.ALL2, 1, False)):
        A = planned[name][1][which]
        want = A.want(spec, m, whole)
        n = len(want)
        total = int((want["end"] - want["begin"]).sum())
        assert n >= 2
        for phase in (0, 1, 31):
            # exactly enough: 32 n bytes and nothing outside them
            arena.reset()
            out = arena.out(32 * n, phase)
            rc, got, nb, per = raw(gpu, A.d_naf, spec, 1 if whole else 0, m, 0, None, out, n, extras=phase != 1)
            torch.cuda.synchronize()
            assert rc == 0 and got == n
            arena.check()
            assert out.cpu().numpy().tobytes() == want.tobytes(), (name, phase)
            assert (nb, per) == ((total, per_period_of(want)) if phase != 1 else (777, [99] * 16))
            # one row too few: the whole count, and nothing written
            arena.reset()
            out = arena.out(32 * (n - 1), phase)
            before = out.clone()
            rc, got, _, _ = raw(gpu, A.d_naf, spec, 1 if whole else 0, m, 0, None, out, n - 1)
            torch.cuda.synchronize()
            assert rc == E_CAP and got == n and torch.equal(out, before)
            arena.check()
            assert "repeats" in gpu.L.naf_gpu_last_error(gpu.h).decode()
    # the archive in an arena, other bytes around it: the same rows
    A = planned["unknown"][1][which]
    want = A.want(RP.ALL2)
    for run, in_phase in ((0, 0), (1, 1), (0, 65)):
        arena.reset()
        before, after = fenced.stream_bait(A.naf, run)
        d_in = arena.put(A.naf, in_phase, before, after)
        out = arena.out(32 * len(want), 5)
        rc, got, _, _ = raw(gpu, d_in, RP.ALL2, 0, 1, 0, None, out, len(want))
        torch.cuda.synchronize()
        assert rc == 0 and got == len(want) and out.cpu().numpy().tobytes() == want.tobytes()
        arena.check()
    # the binding's own form with a caller's buffer
    buf = torch.zeros(32 * len(want) + 32, dtype=torch.uint8, device="cuda")
    view, nb, per = gpu.unnaf_repeats(A.d_naf, RP.spec_text(RP.ALL2), out=buf)
    assert view.numel() == 32 * len(want) and not bool(buf[32 * len(want):].any()) and view.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_repeats(A.d_naf, list(RP.ALL2), out=buf[:32 * (len(want) - 1)])
    assert e.value.code == E_CAP


def test_capacity_is_checked_before_anything_is_written_in_pieces_too(gpu, planned, monkeypatch):
    import torch
    monkeypatch.setenv("NAF_GPU_REPEATS_PIECE", "5000")
    A = planned["seams"][1]["own"]
    want = A.want(RP.ALL3)
    n = len(want)
    assert n > 1000
    out = torch.full((32 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    rc, got, _, _ = raw(gpu, A.d_naf, RP.ALL3, 0, 1, 0, None, out, n - 1)
    assert rc == E_CAP and got == n and bool((out == 0xEE).all())
    rc, got, nb, per = raw(gpu, A.d_naf, RP.ALL3, 0, 1, 0, None, out, n)
    assert rc == 0 and got == n and out.cpu().numpy().tobytes() == want.tobytes() and per == per_period_of(want)
    monkeypatch.delenv("NAF_GPU_REPEATS_PIECE")


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    from naf_amd import capi
    A = planned["overlap"][1]["own"]
    N = A.h.n_sequences

    def fails(d_naf, spec=RP.MISA, flags=0, min_len=1, first=0, count=None, words=()):
        import torch
        buf = torch.zeros(32 * 64, dtype=torch.uint8, device="cuda")
        rc, n, nb, per = raw(gpu, d_naf, spec, flags, min_len, first, count, buf, 64)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == E_ARG and n == 0 and nb == 0 and per == [0] * 16 and not bool(buf.any()), (rc, msg)
        for w in words:
            assert w in msg, msg
        sp = capi.RepeatSpec((C.c_uint32 * 16)(*spec))
        n2, nb2, per2 = C.c_uint64(5), C.c_uint64(5), (C.c_uint64 * 16)(*[5] * 16)
        rc = gpu.L.naf_gpu_unnaf_repeats_count(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), C.byref(sp), flags, min_len, first, capi.WHOLE if count is None else count,
                                               C.byref(n2), C.byref(nb2), per2)
        assert rc == E_ARG and n2.value == 0 and nb2.value == 0 and list(per2) == [0] * 16
        assert all(w in gpu.L.naf_gpu_last_error(gpu.h).decode("latin1") for w in words)

    fails(A.d_naf, spec=(0,) * 16, words=("no period",))
    fails(A.d_naf, spec=(10, 1) + (0,) * 14, words=("min_copies[1]", "is 1"))
    fails(A.d_naf, min_len=0, words=("min_len",))
    fails(A.d_naf, flags=2, words=("flags",))
    fails(A.d_naf, flags=9, words=("flags",))
    fails(A.d_naf, first=N + 1, words=("record", str(N + 1)))
    fails(A.d_naf, first=1, count=N, words=("records", str(N)))
    for name, word in (("protein_small", "protein"), ("text_small", "text")):
        fails(gpu.to_device(golden_bytes("naf", name + ".naf")), words=(word,))
    fails(gpu.to_device(no_sequence_archive(oracle)), words=("no sequence",))
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_repeats_count(A.d_naf, [0] * 16)
    assert e.value.code == E_ARG
    for bad in ("1-1", "", [2] * 15, [2] * 15 + [2 ** 32]):
        with pytest.raises(ValueError):
            gpu.unnaf_repeats(A.d_naf, bad)
    # an archive without records: no rows
    E = planned["no_records"][1]["oracle"]
    assert gpu.unnaf_repeats_count(E.d_naf, "misa") == (0, 0, [0] * 16)
    rows, nb, per = gpu.unnaf_repeats(E.d_naf, "misa")
    assert len(rows) == 0 and nb == 0


def varnum(v):
    out = [v & 127]
    v >>= 7
    while v:
        out.append(128 | (v & 127))
        v >>= 7
    return bytes(reversed(out))


def no_sequence_archive(oracle):
    """An archive of two records without mask and sequence sections: the oracle's archive of a small text with the sequence section -- the
    last one -- cut off and its flag bit cleared (format 1: the flags follow the version)."""
    naf = oracle.ennaf(b">a x\nACGT\n>b\nAC\n", no_mask=True)
    h = oracle.parse_naf(naf)
    assert (h.flags >> 1) & 1 and not (h.flags >> 2) & 1 and h.payload_off[5] is None
    start = h.payload_off[4] - len(varnum(h.orig[4])) - len(varnum(h.comp[4]))
    assert naf[start:h.payload_off[4]] == varnum(h.orig[4]) + varnum(h.comp[4]) and h.payload_off[4] + h.comp[4] == len(naf)
    out = bytearray(naf[:start])
    assert out[:4] == b"\x01\xf9\xec\x01" and out[4] == h.flags
    out[4] &= ~0x02 & 0xFF
    h2 = oracle.parse_naf(bytes(out))
    assert h2.n_sequences == 2 and not (h2.flags >> 1) & 1
    return bytes(out)


# ---- 8. the rows, selected ----------------------------------------------------------------------------------------------------------------
def test_the_selected_text_of_a_row_is_its_motif_repeated(gpu, planned):
    from naf_amd import capi
    for name, rna in (("overlap", False), ("lengths", False), ("rna", True)):
        A = planned[name][1]["own"]
        rows, _, _ = gpu.unnaf_repeats(A.d_naf, list(RP.ALL2))
        segs = capi.repeats_to_segments(rows)
        got = gpu.unnaf_select(A.d_naf, segs, capi.OUT_SEQUENCES, use_mask=False).cpu().numpy().tobytes()
        want = []
        for x in rows:
            w, n = capi.repeat_motif_text(int(x["motif"]), int(x["period"]), rna), int(x["end"] - x["begin"])
            want.append((w * (n // len(w) + 1))[:n])
        assert len(segs) == len(rows) > 20 and got == "".join(t + "\n" for t in want).encode()
    lengths = [len(ln) for ln in A.lines]
    assert capi.repeats_to_segments(rows[:3], 5, lengths) == [(int(x["record"]), max(0, int(x["begin"]) - 5), min(int(x["end"]) + 5, lengths[int(x["record"])])) for x in rows[:3]]


# ---- 9. the command line ------------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_repeats_write_the_table(gpu, oracle, planned):
    """(every call starts a process that opens the device: one call per option, not their product)"""
    A = planned["lengths"][1]["own"]
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    assert len(ids) == A.h.n_sequences
    r = next(k for k in range(len(A.lines)) if len(A.want(RP.ALL2, 1, False, k, 1)) > 2)
    for args, spec, m, whole, first, count in ((["--repeats", "misa"], RP.MISA, 1, False, 0, None),
                                               (["--repeats", RP.spec_text(RP.ALL3), "--min-repeat", "12", "--records", "2-9"], RP.ALL3, 12, False, 1, 8),
                                               (["--repeats", RP.spec_text(RP.ALL2), "--whole-units", "--min-repeat", "12", "--region", ids[r]], RP.ALL2, 12, True, r, 1),
                                               (["--repeats", "2-2,3-2", "--whole-units"], (0, 2, 2) + (0,) * 13, 1, True, 0, None)):
        p = unnaf_cli(args, A.naf)
        want = A.want(spec, m, whole, first, count)
        assert p.returncode == 0 and p.stderr == b"" and p.stdout == RP.table_lines(want, ids), args
        assert len(want) > 0
    # RNA: U in the motif and in the class
    R = planned["rna"][1]["own"]
    rids = oracle.zstd_decompress(R.h.frame(R.naf, 0)).decode("latin1").split("\0")[:-1]
    p = unnaf_cli(["--repeats", RP.spec_text(RP.ALL2)], R.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == RP.table_lines(R.want(RP.ALL2), rids, rna=True) and b"U" in p.stdout and b"T" not in p.stdout.replace(b"\t", b"")
    p = unnaf_cli(["--repeats", "misa", "--region", "nosuch"], A.naf)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ")
    p = unnaf_cli(["--repeats", "misa"], golden_bytes("naf", "protein_small.naf"))
    assert p.returncode == 1 and p.stdout == b"" and b"protein" in p.stderr
