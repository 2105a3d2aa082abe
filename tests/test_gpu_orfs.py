"""GPU tests of the table of open reading frames (naf_gpu_unnaf_orfs_count, naf_gpu_unnaf_orfs, unnaf --orfs).  Expected rows never come from
the code under test: they are what orfs_plan.expected_rows -- numpy over the oracle's --sequences text of the same archive -- gives.  Every
planned text is asked in two archives, the oracle's and this library's own ennaf at level 1 (the empty text: the oracle's only); the
reference-made golden archive repeat_l19 (a frame whose blocks depend on each other) takes the whole-decode fallback.  A table is always
compared WHOLE, byte for byte: no exclusions, no tolerance."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orfs_plan as OP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
CASES = [c.name for c in OP.planned(0)]
TRACE = re.compile(r"\[orfs\] orfs (\d+) stretches (\d+) stops (\d+) pieces (\d+) sequence bytes decoded (\d+) of (\d+)\n")


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
        self.lines = OP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), self.h.n_sequences)
        self.d_naf = gpu.to_device(naf)
        self._want = {}

    def rows(self, q, first=0, count=None):
        """the model's table, computed once per question and left unchanged"""
        key = q.key + (first, count)
        if key not in self._want:
            st, sa = q.sets()
            v = OP.expected_rows(self.lines, st, sa, q.min_len, q.strands, q.flags, first, count)
            v.setflags(write=False)
            self._want[key] = v
        return self._want[key]


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive}); the two archives of a text hold the same lines (the reads: but for the empty ones)"""
    out = {}
    for c in OP.planned(SEED):
        arc = {"oracle": Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type, well_formed=c.well_formed))}
        if c.text:
            own, _ = gpu.ennaf(gpu.to_device(c.own_text or c.text), seq_type=c.seq_type, level=1)
            arc["own"] = Archive(oracle, gpu, own.cpu().numpy().tobytes())
            if c.own_text:
                assert arc["own"].lines == [x for x in arc["oracle"].lines if x] and len(arc["own"].lines) < len(arc["oracle"].lines), c.name
            else:
                assert arc["own"].lines == arc["oracle"].lines, c.name
                arc["own"]._want = arc["oracle"]._want
        out[c.name] = (c, arc)
    return out


@pytest.fixture(scope="module")
def repeat(oracle, gpu):
    return Archive(oracle, gpu, golden_bytes("naf", "repeat_l19.naf"))


def ask(gpu, A, q, first=0, count=None):
    return gpu.unnaf_orfs(A.d_naf, q.stops, q.starts, q.min_len, q.strands, bool(q.flags & OP.SPLIT_UNKNOWN), bool(q.flags & OP.CLOSED), first, count)


def check(gpu, A, q, first=0, count=None, counts=True):
    """the whole table byte for byte, the sum, and the counting call"""
    want = A.rows(q, first, count)
    rows, n_bases = ask(gpu, A, q, first, count)
    if rows.tobytes() != want.tobytes():
        got = set(tuple(int(v) for v in x) for x in rows)
        exp = set(tuple(int(v) for v in x) for x in want)
        raise AssertionError("%r records %d+%s: %d rows, %d expected; only got: %s; only expected: %s; in order: %s" % (
            q, first, count, len(rows), len(want), sorted(got - exp)[:6], sorted(exp - got)[:6], got == exp))
    n, nb, pf = OP.totals(want)
    assert n_bases == nb
    if counts:
        assert gpu.unnaf_orfs_count(A.d_naf, q.stops, q.starts, q.min_len, q.strands, bool(q.flags & OP.SPLIT_UNKNOWN), bool(q.flags & OP.CLOSED), first, count) == (n, nb, pf), q
    return rows


# ---- 1. the planned texts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_tables_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    if which not in arc:
        assert name == "no_records"
        return
    A = arc[which]
    total = 0
    for q in c.qs:
        total += len(check(gpu, A, q))
    if name == "no_records":
        assert total == 0 and len(A.lines) == 0
    else:
        assert total > 0


def test_the_seams_text_has_the_rows_of_its_plants(gpu, planned):
    """what the plants must give, said without the model: the stop planted d bases from a seam ends a stretch there or, where another stop
    lies directly in front of it (the two plants of a block seam), begins one behind it"""
    c, arc = planned["seams0"]
    rows = check(gpu, arc["own"], OP.DENSEST)
    base = np.cumsum([0] + [len(x) for x in arc["own"].lines])
    right, left = (OP.STOP3, OP.STOP5), (OP.STOP5, OP.STOP3)                        # the flag of a stop behind `end` / in front of `begin`, by strand
    ends = {(int(x["strand"]), int(base[int(x["record"])] + x["end"])) for x in rows if x["flags"] & right[int(x["strand"])]}
    begins = {(int(x["strand"]), int(base[int(x["record"])] + x["begin"])) for x in rows if x["flags"] & left[int(x["strand"])]}
    seen = 0
    for kind, d, strand, what, p, n in c.plants:
        if what == "stop":
            assert (strand, p) in ends or (strand, p + 3) in begins, (kind, d, strand, p)
            seen += (strand, p) in ends
    assert seen >= 3 * 12 + 1


def test_the_reference_made_archive(gpu, repeat, monkeypatch, capfd):
    for q in (OP.DEFAULTS, OP.DENSEST, OP.Q(OP.STD_STOPS, OP.STD_STARTS, 30, 3, OP.SPLIT_UNKNOWN | OP.CLOSED)):
        assert len(check(gpu, repeat, q)) > 0
    last = max(r for r in range(len(repeat.lines)) if repeat.lines[r])
    _, tr = traced(gpu, repeat, OP.DENSEST, last, 1, monkeypatch, capfd)
    assert tr[3] == 1 and tr[4] == tr[5] == (repeat.h.orig[4] + 1) // 2             # dependent blocks: the whole stream, once


# ---- 2. first and count, and what is decoded ----------------------------------------------------------------------------------------------
def traced(gpu, A, q, first, count, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    rows, _ = ask(gpu, A, q, first, count)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = TRACE.findall(err)
    assert len(m) == 1, err
    assert rows.tobytes() == A.rows(q, first, count).tobytes()
    return rows, [int(x) for x in m[0]]


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    A = planned["records"][1][which]
    N = len(A.lines)
    for q in (OP.DENSEST, OP.Q(OP.STD_STOPS, OP.STD_STARTS, 3, 3, OP.SPLIT_UNKNOWN)):
        whole = check(gpu, A, q)
        for first, count in ((0, 1), (N - 1, 1), (N, 0), (N, None), (5, 0), (3, 9), (0, None), (N // 2, 30), (1, N - 1), (0, N - 1), (2, 1), (100, 60)):
            last = N if count is None else first + count
            part = check(gpu, A, q, first, count)
            assert part.tobytes() == whole[(whole["record"] >= first) & (whole["record"] < last)].tobytes()
    S = planned["seams0"][1][which]
    M = len(S.lines)
    for first, count in ((0, 2), (M - 2, 2), (2, 3), (M, 0), (4, 1)):
        check(gpu, S, OP.DENSEST, first, count)
    B = planned["bounds"][1][which]
    for first, count in ((3, 2), (23, 2), (0, 1)):
        check(gpu, B, OP.Q(OP.STD_STOPS, OP.STD_STARTS, 3), first, count)


def test_a_restricted_query_decodes_only_the_blocks_behind_its_records(gpu, planned, monkeypatch, capfd):
    for which in ("oracle", "own"):
        A = planned["seams0"][1][which]
        T = (A.h.orig[4] + 1) // 2
        rows, (n, stretches, stops, pieces, D, Tt) = traced(gpu, A, OP.DENSEST, 0, None, monkeypatch, capfd)
        assert (n, pieces, D, Tt) == (len(rows), 1, T, T) and stretches >= n and stops > 0
        for first, count in ((1, 1), (len(A.lines) - 2, 1)):                        # the first 100000 bases; the last 10001
            rows, (n, stretches, stops, pieces, D, Tt) = traced(gpu, A, OP.DENSEST, first, count, monkeypatch, capfd)
            assert (n, pieces, Tt) == (len(rows), 1, T) and 0 < D < T, (which, first, count, D, T)


# ---- 3. the piece size does not show, and two runs agree ------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [OP.PIECE, 100000, None])
def test_the_result_does_not_depend_on_the_piece_size(gpu, planned, repeat, piece, monkeypatch, capfd):
    if piece:
        monkeypatch.setenv("NAF_GPU_ORFS_PIECE", str(piece))
    for which in ("oracle", "own"):
        for name in ("seams0", "bounds", "records", "dense", "reads", "r7"):
            c, arc = planned[name]
            for q in c.qs[:4]:
                check(gpu, arc[which], q, counts=False)
        check(gpu, planned["records"][1][which], OP.DENSEST, 7, 150)
    check(gpu, repeat, OP.DEFAULTS, counts=False)
    B = planned["bounds"][1]["own"]
    _, tr = traced(gpu, B, OP.DENSEST, 0, None, monkeypatch, capfd)
    assert tr[3] == (len(B.lines) if piece == OP.PIECE else 2 if piece == 100000 else 1), tr      # at PIECE every record boundary is a piece boundary
    if piece:
        monkeypatch.delenv("NAF_GPU_ORFS_PIECE")


def test_two_calls_give_identical_bytes(gpu, planned):
    for name in ("seams0", "dense", "reads", "records"):
        A = planned[name][1]["own"]
        for q in (OP.DENSEST, OP.DEFAULTS):
            a, _ = ask(gpu, A, q)
            b, _ = ask(gpu, A, q)
            assert a.tobytes() == b.tobytes() == A.rows(q).tobytes()


# ---- 4. buffers ----------------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, stops, starts, min_len, strands, flags, first, count, d_rows, cap):
    from naf_amd import capi
    n, nb = C.c_uint64(12345), C.c_uint64(777)
    rc = gpu.L.naf_gpu_unnaf_orfs(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), stops, starts, min_len, strands, flags, first, capi.WHOLE if count is None else count,
                                  C.c_void_p(d_rows.data_ptr() if d_rows is not None and d_rows.numel() else 0), cap, C.byref(n), C.byref(nb))
    return rc, n.value, nb.value


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x5D, size=8 << 20)
    for name, q in (("records", OP.DENSEST), ("dense", OP.DEFAULTS), ("bounds", OP.Q(OP.STD_STOPS, OP.STD_STARTS, 3))):
        A = planned[name][1][which]
        want = A.rows(q)
        n, nb, _ = OP.totals(want)
        st, sa = q.sets()
        assert n > 1
        for phase in fenced.PHASES:
            # exactly enough: 32 n bytes and nothing outside them, at every address phase
            arena.reset()
            out = arena.out(32 * n, phase)
            rc, got, gotb = raw(gpu, A.d_naf, st, sa, q.min_len, q.strands, q.flags, 0, None, out, n)
            torch.cuda.synchronize()
            assert (rc, got, gotb) == (0, n, nb), (name, phase, rc)
            arena.check()
            assert out.cpu().numpy().tobytes() == want.tobytes(), (name, phase)
            # one row too few: the whole count, and nothing written
            arena.reset()
            out = arena.out(32 * (n - 1), phase)
            before = out.clone()
            rc, got, gotb = raw(gpu, A.d_naf, st, sa, q.min_len, q.strands, q.flags, 0, None, out, n - 1)
            torch.cuda.synchronize()
            assert rc == E_CAP and got == n and torch.equal(out, before), (name, phase, rc, got)
            arena.check()
            assert "orfs" in gpu.L.naf_gpu_last_error(gpu.h).decode()
    # several pieces: the capacity is found too small before anything is written
    A = planned["bounds"][1][which]
    q = OP.DENSEST
    want = A.rows(q)
    st, sa = q.sets()
    os.environ["NAF_GPU_ORFS_PIECE"] = str(OP.PIECE)
    try:
        for cap in (len(want) - 1, len(want) // 2, 0):
            arena.reset()
            out = arena.out(32 * cap, 3)
            before = out.clone()
            rc, got, _ = raw(gpu, A.d_naf, st, sa, q.min_len, q.strands, q.flags, 0, None, out, cap)
            torch.cuda.synchronize()
            assert rc == E_CAP and got == len(want) and torch.equal(out, before)
            arena.check()
        arena.reset()
        out = arena.out(32 * len(want), 5)
        rc, got, _ = raw(gpu, A.d_naf, st, sa, q.min_len, q.strands, q.flags, 0, None, out, len(want))
        torch.cuda.synchronize()
        assert rc == 0 and got == len(want) and out.cpu().numpy().tobytes() == want.tobytes()
        arena.check()
    finally:
        del os.environ["NAF_GPU_ORFS_PIECE"]
    # the binding's own form with a caller's buffer
    A = planned["records"][1][which]
    want = A.rows(OP.DEFAULTS)
    buf = torch.zeros(32 * len(want) + 32, dtype=torch.uint8, device="cuda")
    rows, nb = gpu.unnaf_orfs(A.d_naf, out=buf)
    assert rows.data_ptr() == buf.data_ptr() and rows.cpu().numpy().tobytes() == want.tobytes() and not bool(buf[32 * len(want):].any())
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_orfs(A.d_naf, out=buf[:32 * len(want) - 1])
    assert e.value.code == E_CAP


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------------
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
    return bytes(out)


def test_errors_of_the_contract(gpu, planned, oracle):
    import torch
    from naf_amd import capi
    A = planned["records"][1]["own"]
    N = A.h.n_sequences
    STOPS, ATG = OP.codon_set(OP.STD_STOPS), OP.codon_set("ATG")

    def fails(d_naf, stops=STOPS, starts=ATG, min_len=75, strands=3, flags=0, first=0, count=None, words=()):
        buf = torch.zeros(32 * 64, dtype=torch.uint8, device="cuda")
        rc, n, nb = raw(gpu, d_naf, stops, starts, min_len, strands, flags, first, count, buf, 64)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == E_ARG and (n, nb) == (0, 0) and not bool(buf.any()), (rc, msg)
        for w in words:
            assert w in msg, msg
        n2, nb2, pf = C.c_uint64(5), C.c_uint64(5), (C.c_uint64 * 6)(*([9] * 6))
        rc = gpu.L.naf_gpu_unnaf_orfs_count(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), stops, starts, min_len, strands, flags, first, capi.WHOLE if count is None else count,
                                            C.byref(n2), C.byref(nb2), pf)
        assert rc == E_ARG and (n2.value, nb2.value) == (0, 0) and list(pf) == [0] * 6
        assert all(w in gpu.L.naf_gpu_last_error(gpu.h).decode("latin1") for w in words)

    fails(A.d_naf, stops=0, words=("orfs", "stops"))
    fails(A.d_naf, stops=STOPS, starts=STOPS, words=("starts", "stops"))
    fails(A.d_naf, stops=STOPS | ATG, words=("starts", "stops"))
    fails(A.d_naf, min_len=0, words=("min_len",))
    for s in (0, 4, -1, 7):
        fails(A.d_naf, strands=s, words=("strands",))
    for f in (4, 8, 7, -1):
        fails(A.d_naf, flags=f, words=("flags",))
    fails(A.d_naf, first=N + 1, words=("record", str(N + 1)))
    fails(A.d_naf, first=1, count=N, words=("records", str(N)))
    for name, word in (("protein_small", "protein"), ("text_small", "text")):
        d = gpu.to_device(golden_bytes("naf", name + ".naf"))
        fails(d, words=(word,))
    fails(gpu.to_device(no_sequence_archive(oracle)), words=("no sequence",))
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_orfs(A.d_naf, min_len=0)
    assert e.value.code == E_ARG
    with pytest.raises(ValueError):
        gpu.unnaf_orfs(A.d_naf, stops="TA")
    # an archive without records: 0 rows, and first = 0 = n_sequences is in range
    E = planned["no_records"][1]["oracle"]
    assert gpu.unnaf_orfs_count(E.d_naf) == (0, 0, [0] * 6)


# ---- 6. the cross-check through the archive itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [OP.DEFAULTS, OP.DENSEST, OP.Q("TAA,TAG", "ATG,GTG,TTG", 30), OP.Q(OP.STD_STOPS, OP.STD_STARTS, 30, 3, OP.SPLIT_UNKNOWN)], ids=repr)
def test_the_rows_selected_are_coding_texts(gpu, planned, q):
    from naf_amd import capi
    A = planned["dense"][1]["own"]
    rows, _ = ask(gpu, A, q)
    assert len(rows) > 100
    stops, starts = set(q.stops.split(",")), set(q.starts.split(",")) if q.starts else None
    for include_stop in (False, True):
        segs = capi.orfs_to_segments(rows, include_stop)
        text = gpu.unnaf_select(A.d_naf, segs, capi.OUT_SEQ, use_mask=False).cpu().numpy().tobytes().decode()
        assert len(text) == sum(e - b for _, b, e, _ in segs)
        at = 0
        for x, (_, b, e, _) in zip(rows, segs):
            t = text[at:at + e - b]
            at += e - b
            assert len(t) % 3 == 0
            codons = [t[i:i + 3] for i in range(0, len(t), 3)]
            body = codons[:-1] if include_stop and x["flags"] & OP.STOP3 else codons
            assert not stops & set(body), (x, t)                                    # no stop in frame
            if starts:
                assert codons[0] in starts, (x, t)
            if include_stop:
                assert (codons[-1] in stops) == bool(x["flags"] & OP.STOP3), (x, t)
            if q.flags & OP.SPLIT_UNKNOWN:
                assert not set(t) - set("ACGT")


# ---- 7. the command line -------------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def ids_of(oracle, A):
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    assert len(ids) == A.h.n_sequences
    return ids


def test_cli_orfs_writes_the_lines(gpu, oracle, planned):
    A = planned["dense"][1]["own"]
    ids = ids_of(oracle, A)
    for args, q, first, count in (([], OP.DEFAULTS, 0, None), (["--stop-to-stop", "--min-orf", "3"], OP.DENSEST, 0, None),
                                  (["--min-orf", "300", "--strand", "-", "--closed"], OP.Q(OP.STD_STOPS, OP.STD_STARTS, 300, 2, OP.CLOSED), 0, None),
                                  (["--stops", "TAA,TAG", "--starts", "ATG,GTG,TTG", "--min-orf", "30", "--split-unknown", "--strand", "+"],
                                   OP.Q("TAA,TAG", "ATG,GTG,TTG", 30, 1, OP.SPLIT_UNKNOWN), 0, None),
                                  (["--stops", "tar,uga", "--records", "2-9"], OP.DEFAULTS, 1, 8), (["--region", ids[4], "--strand", "both"], OP.DEFAULTS, 4, 1)):
        p = unnaf_cli(["--orfs"] + args, A.naf)
        want = OP.cli_lines(A.rows(q, first, count), ids)
        assert p.returncode == 0 and p.stderr == b"" and p.stdout == want and want, args
    F = planned["reads"][1]["own"]                                                  # FASTQ
    fids = ids_of(oracle, F)
    q = OP.Q(OP.STD_STOPS, None, 12, 3, OP.CLOSED)
    p = unnaf_cli(["--orfs", "--stop-to-stop", "--min-orf", "12", "--closed"], F.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == OP.cli_lines(F.rows(q), fids) and p.stdout.count(b"\n") > 20
    for args in (["--orfs", "--region", "nosuch"], ["--orfs", "--records", "1-9999"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    p = unnaf_cli(["--orfs"], golden_bytes("naf", "protein_small.naf"))
    assert p.returncode == 1 and p.stdout == b"" and b"protein" in p.stderr
    p = unnaf_cli(["--orfs"], planned["no_records"][1]["oracle"].naf)
    assert p.returncode == 0 and p.stdout == b""
