"""GPU tests of the run table (naf_gpu_unnaf_runs_count, naf_gpu_unnaf_runs, unnaf --runs / --masked-runs).  Expected rows never come from the
code under test: they are what runs_plan.expected_runs / expected_masked -- regexes over the oracle's --sequences text of the same
archive, mask on -- give.  Every planned text is asked in two archives, the oracle's and this library's own ennaf at level 1 (the empty
text: the oracle's only); the reference-made golden archives repeat_l19 and repeat_long27 (frames whose blocks depend on each other) take
the whole-decode fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import runs_plan as RP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
CASES = [c.name for c in RP.planned(0)]
GOLDEN_REPEATS = ("repeat_l19", "repeat_long27")
TRACE = re.compile(r"\[runs\] runs (\d+) candidates (\d+) pieces (\d+) sequence bytes decoded (\d+) of (\d+) mask toggles (\d+)\n")
Q_N, Q_NOT_N, Q_GAP, Q_HOMO, Q_MASK = (("N", 0x8000, False, False), ("^N", 0x7FFF, False, False), ("-", 0x0001, False, False), ("ACGT", 0x0116, True, False),
                                       (None, 0, False, True))


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
        self.has_mask = bool((self.h.flags >> 2) & 1)
        self.lines = RP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), self.h.n_sequences)
        self.d_naf = gpu.to_device(naf)
        self._want = {}

    def want(self, q, min_len=1, first=0, count=None):
        """expected rows, computed once per question and left unchanged"""
        _, s, each, masked = q[:4]
        key = (s, each, masked, min_len, first, count)
        if key not in self._want:
            rows = RP.expected_masked(self.lines, min_len, first, count) if masked else RP.expected_runs(self.lines, s, each, min_len, first, count)
            rows.setflags(write=False)
            self._want[key] = rows
        return self._want[key]


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive}); the two archives of a text hold the same lines"""
    out = {}
    for c in RP.planned(SEED):
        arc = {"oracle": Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type, no_mask=c.no_mask))}
        if c.text:
            own, _ = gpu.ennaf(gpu.to_device(c.text), seq_type=c.seq_type, level=1, no_mask=c.no_mask)
            arc["own"] = Archive(oracle, gpu, own.cpu().numpy().tobytes())
            assert arc["own"].lines == arc["oracle"].lines, c.name
            arc["own"]._want = arc["oracle"]._want
        out[c.name] = (c, arc)
    return out


@pytest.fixture(scope="module")
def repeats(oracle, gpu):
    return {name: Archive(oracle, gpu, golden_bytes("naf", name + ".naf")) for name in GOLDEN_REPEATS}


def ask(gpu, A, q, min_len=1, first=0, count=None, **kw):
    text, s, each, masked = q[:4]
    return gpu.unnaf_runs(A.d_naf, None if masked else (text if text is not None else s), each, masked, min_len, first, count, **kw)


def check(gpu, A, q, min_len=1, first=0, count=None, counts=True):
    """the rows byte for byte, the sum of their lengths, and the counting call"""
    want = A.want(q, min_len, first, count)
    rows, n_bases = ask(gpu, A, q, min_len, first, count)
    if rows.tobytes() != want.tobytes():
        k = next((i for i in range(min(len(rows), len(want))) if rows[i].tobytes() != want[i].tobytes()), min(len(rows), len(want)))
        raise AssertionError("%r min_len %d records %d+%s: first difference at row %d of %d / %d: got %s, expected %s" % (
            q[:4], min_len, first, count, k, len(rows), len(want), RP.as_tuples(rows[k:k + 2]), RP.as_tuples(want[k:k + 2])))
    total = int((want["end"] - want["begin"]).sum())
    assert n_bases == total
    if counts:
        text, s, each, masked = q[:4]
        assert gpu.unnaf_runs_count(A.d_naf, None if masked else s, each, masked, min_len, first, count) == (len(want), total)
    return rows


# ---- 1, 2. the rows and the counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_rows_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    if which not in arc:
        assert name == "no_records"
        return
    A = arc[which]
    assert A.has_mask or name == "nomask"
    n = {}
    for q in c.queries:
        for m in q[4]:
            n[q[:4]] = n.get(q[:4], 0) + len(check(gpu, A, q, m))
    if name == "no_records":
        assert not any(n.values())
    else:
        assert n[Q_NOT_N] > 0 and n[Q_HOMO] > 0
        assert (n[Q_MASK] > 0) == (name not in ("nomask", "fastq")), name
        assert n[Q_N] > 0
    if name in ("record_ends", "all16"):
        assert n[Q_GAP] > 0


# ---- 3. the whole-decode fallback -------------------------------------------------------------------------------------------------------
def traced(gpu, A, q, min_len, first, count, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    import torch
    n = len(A.want(q, min_len, first, count))
    buf = torch.zeros(max(32 * n, 1), dtype=torch.uint8, device="cuda")
    view, n_bases = ask(gpu, A, q, min_len, first, count, out=buf)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = TRACE.findall(err)
    assert len(m) == 1, err
    return np.frombuffer(view.cpu().numpy().tobytes(), dtype=RP.RUN_DTYPE), [int(x) for x in m[0]]


@pytest.mark.parametrize("name", GOLDEN_REPEATS)
def test_rows_of_the_reference_made_archives(gpu, repeats, name, monkeypatch, capfd):
    A = repeats[name]
    for q, m in ((Q_NOT_N, 1), (Q_HOMO, 3), (Q_HOMO, 1), (Q_N, 1), (Q_MASK, 1)):
        check(gpu, A, q, m)
    assert len(A.want(Q_HOMO, 3)) > 0
    last = max(r for r in range(len(A.lines)) if A.lines[r])
    got, tr = traced(gpu, A, Q_HOMO, 3, last, 1, monkeypatch, capfd)
    assert got.tobytes() == A.want(Q_HOMO, 3, last, 1).tobytes()
    assert tr[3] == tr[4] == (A.h.orig[4] + 1) // 2                                  # dependent blocks: the whole stream, once


# ---- 4. first and count -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    for name in ("seams", "record_ends"):
        c, arc = planned[name]
        A = arc[which]
        N = len(A.lines)
        empty = [r for r in range(N) if not A.lines[r]]
        assert len(empty) >= 5
        for q, m in ((Q_N, 1), (Q_NOT_N, 2), (Q_MASK, 1), (Q_HOMO, 3)):
            whole = A.want(q, m)
            for r in range(N):
                rows = check(gpu, A, q, m, r, 1, counts=False)
                assert rows.tobytes() == whole[whole["record"] == r].tobytes()
            # ranges that begin and end at empty records, and empty ranges
            for first, count in ((empty[0], empty[-1] + 1 - empty[0]), (empty[1], empty[2] - empty[1]), (empty[1], 1), (empty[1], empty[3] + 1 - empty[1]), (3, 9), (N - 1, 1),
                                 (5, 0), (N, 0), (N, None), (0, None)):
                rows = check(gpu, A, q, m, first, count)
                last = N if count is None else first + count
                assert rows.tobytes() == whole[(whole["record"] >= first) & (whole["record"] < last)].tobytes()


# ---- 5. the trace: what was decoded ---------------------------------------------------------------------------------------------------------
def test_a_restricted_query_decodes_only_the_blocks_behind_its_records(gpu, oracle, monkeypatch, capfd):
    rng = np.random.default_rng(9700 + SEED)
    recs = [RP._random(rng, n, "ACGTNacgtn") for n in (5000, 300000, 700000, 3001)]
    own, _ = gpu.ennaf(gpu.to_device(RP.fasta(recs, 80)), level=1)
    A = Archive(oracle, gpu, own.cpu().numpy().tobytes())
    assert [x.decode() for x in A.lines] == recs and A.has_mask
    T = (A.h.orig[4] + 1) // 2
    for first, count in ((0, 1), (1, 1), (3, 1)):
        got, (R, K, pieces, D, Tt, M) = traced(gpu, A, Q_N, 2, first, count, monkeypatch, capfd)
        assert got.tobytes() == A.want(Q_N, 2, first, count).tobytes()
        assert (R, pieces, Tt, M) == (len(got), 1, T, 0) and 0 < D < T and K >= R, (first, count, D, T)
    got, tr = traced(gpu, A, Q_N, 2, 0, None, monkeypatch, capfd)
    assert tr[3] == T
    # the soft mask: no sequence byte at all
    for first, count in ((0, None), (2, 1)):
        got, (R, K, pieces, D, Tt, M) = traced(gpu, A, Q_MASK, 2, first, count, monkeypatch, capfd)
        assert got.tobytes() == A.want(Q_MASK, 2, first, count).tobytes() and len(got) > 0
        assert (R, pieces, D, Tt) == (len(got), 0, 0, T) and M > 0 and K >= R


# ---- 6. the piece size does not show -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [5000, 1])
def test_the_result_does_not_depend_on_the_piece_size(gpu, planned, repeats, piece, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_RUNS_PIECE", str(piece))
    for name, qs in (("seams", ((Q_N, 1), (Q_NOT_N, 64), (Q_HOMO, 4), (Q_MASK, 255))), ("record_ends", ((Q_N, 1), (Q_NOT_N, 1), (Q_GAP, 1), (Q_HOMO, 1), (Q_MASK, 1))),
                     ("fastq", ((Q_N, 1), (Q_HOMO, 4))), ("all16", (((None, RP.ALL, True, False), 1), (Q_NOT_N, 1))), ("r7", ((Q_N, 1), (Q_NOT_N, 2), (Q_MASK, 1)))):
        c, arc = planned[name]
        if name == "fastq" and piece == 1:
            continue                                                                # (2000 pieces of one read each: the other texts cover piece = 1)
        for which in ("oracle", "own"):
            for q, m in qs:
                check(gpu, arc[which], q, m)
                N = len(arc[which].lines)
                check(gpu, arc[which], q, m, min(2, N - 1), min(5, N - min(2, N - 1)), counts=False)
    A = planned["seams"][1]["own"]
    got, tr = traced(gpu, A, Q_N, 1, 0, None, monkeypatch, capfd)
    assert got.tobytes() == A.want(Q_N, 1).tobytes() and tr[2] > 1                   # it was swept in pieces
    check(gpu, repeats["repeat_l19"], Q_HOMO, 3)
    monkeypatch.delenv("NAF_GPU_RUNS_PIECE")


def test_two_calls_give_identical_bytes(gpu, planned):
    for name, q, m in (("seams", Q_NOT_N, 1), ("fastq", Q_N, 1), ("all16", (None, RP.ALL, True, False), 1), ("seams", Q_MASK, 1)):
        A = planned[name][1]["own"]
        a, _ = ask(gpu, A, q, m)
        b, _ = ask(gpu, A, q, m)
        assert a.tobytes() == b.tobytes() == A.want(q, m).tobytes()


# ---- 7. equal toggles -----------------------------------------------------------------------------------------------------------------------
def varnum(v):
    out = [v & 127]
    v >>= 7
    while v:
        out.append(128 | (v & 127))
        v >>= 7
    return bytes(reversed(out))


def test_equal_toggles_of_a_foreign_archive_cancel(gpu, oracle):
    """A mask whose units hold zeros in the middle -- stretches of no bases: equal toggles -- as another writer may leave them.  Two of
    them cancel (the stretches on either side are one run), three are one; a zero behind a 255 is the unit encoding's own."""
    rng = np.random.default_rng(9800 + SEED)
    recs = [RP._random(rng, n, "ACGTN") for n in (700, 0, 1300, 255, 2000)]
    naf = oracle.ennaf(RP.fasta(recs, 60))
    h = oracle.parse_naf(naf)
    total = sum(len(r) for r in recs)
    units = [10, 5, 0, 0, 7, 0, 3, 255, 0, 255, 255, 0, 0, 20, 0, 0, 0, 30, 0, 0, 0, 0, 40, 65, 12, 0, 8]
    rest = total - sum(units)
    units += [255] * (rest // 255) + [rest % 255]
    frame = oracle.zstd_store_raw(bytes(units))[4:]
    o = h.payload_off[3]
    start = o - len(varnum(h.orig[3])) - len(varnum(h.comp[3]))
    assert naf[start:o] == varnum(h.orig[3]) + varnum(h.comp[3])
    crafted = naf[:start] + varnum(len(units)) + varnum(len(frame)) + frame + naf[o + h.comp[3]:]
    A = Archive(oracle, gpu, crafted)
    assert A.has_mask and [x.decode().upper() for x in A.lines] == recs
    low = "".join(x.decode() for x in A.lines)
    assert low == oracle.mask_apply("".join(recs).encode(), bytes(units)).decode()
    want = A.want(Q_MASK)
    # (the units alternate between upper and lower case: 5 lower; 255 lower as "255, 0"; 40 lower; and "12, 0, 8" -- 12 lower, no upper, 8 lower -- is ONE run of 20)
    assert RP.as_tuples(want) == [(0, 10, 15, 0), (0, 25, 280, 0), (2, 140, 180, 0), (2, 245, 265, 0)]
    for m in (1, 2, 5, 8, 9, 255, 256):
        check(gpu, A, Q_MASK, m)
    check(gpu, A, Q_MASK, 1, 2, 2)
    check(gpu, A, Q_N, 1)


# ---- 8. buffers ----------------------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, s, flags, min_len, first, count, d_runs, cap, bases=True):
    from naf_amd import capi
    n, nb = C.c_uint64(12345), C.c_uint64(777)
    rc = gpu.L.naf_gpu_unnaf_runs(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), s, flags, min_len, first, capi.WHOLE if count is None else count,
                                  C.c_void_p(d_runs.data_ptr() if d_runs is not None and d_runs.numel() else 0), cap, C.byref(n), C.byref(nb) if bases else None)
    return rc, n.value, nb.value


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x5A, size=8 << 20)
    for name, q, m in (("all16", (None, RP.ALL, True, False), 1), ("seams", Q_NOT_N, 1), ("seams", Q_MASK, 1), ("fastq", Q_N, 2)):
        A = planned[name][1][which]
        _, s, each, masked = q
        flags = (1 if each else 0) | (2 if masked else 0)
        want = A.want(q, m)
        n = len(want)
        total = int((want["end"] - want["begin"]).sum())
        assert n >= 2
        for phase in range(8):
            # exactly enough: 32 n bytes and nothing outside them
            arena.reset()
            out = arena.out(32 * n, phase)
            rc, got, nb = raw(gpu, A.d_naf, s, flags, m, 0, None, out, n, bases=phase % 2 == 0)
            torch.cuda.synchronize()
            assert rc == 0 and got == n
            arena.check()
            assert out.cpu().numpy().tobytes() == want.tobytes(), (name, phase)
            assert nb == (total if phase % 2 == 0 else 777)
            # one row too few: the whole count, and nothing written
            arena.reset()
            out = arena.out(32 * (n - 1), phase)
            before = out.clone()
            rc, got, _ = raw(gpu, A.d_naf, s, flags, m, 0, None, out, n - 1)
            torch.cuda.synchronize()
            assert rc == E_CAP and got == n and torch.equal(out, before)
            arena.check()
            assert "runs" in gpu.L.naf_gpu_last_error(gpu.h).decode()
    # the archive in an arena, other bytes around it: the same rows
    A = planned["all16"][1][which]
    want = A.want(Q_NOT_N, 2)
    for run, in_phase in ((0, 0), (1, 1), (0, 65)):
        arena.reset()
        before, after = fenced.stream_bait(A.naf, run)
        d_in = arena.put(A.naf, in_phase, before, after)
        out = arena.out(32 * len(want), 5)
        rc, got, _ = raw(gpu, d_in, 0x7FFF, 0, 2, 0, None, out, len(want))
        torch.cuda.synchronize()
        assert rc == 0 and got == len(want) and out.cpu().numpy().tobytes() == want.tobytes()
        arena.check()
    # the binding's own form with a caller's buffer
    buf = torch.zeros(32 * len(want) + 32, dtype=torch.uint8, device="cuda")
    view, nb = gpu.unnaf_runs(A.d_naf, "^N", min_len=2, out=buf)
    assert view.numel() == 32 * len(want) and not bool(buf[32 * len(want):].any()) and view.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_runs(A.d_naf, "^N", min_len=2, out=buf[:32 * (len(want) - 1)])
    assert e.value.code == E_CAP


def test_capacity_is_checked_before_anything_is_written_in_pieces_too(gpu, planned, monkeypatch):
    import torch
    monkeypatch.setenv("NAF_GPU_RUNS_PIECE", "5000")
    A = planned["seams"][1]["own"]
    want = A.want(Q_N, 1)
    n = len(want)
    out = torch.full((32 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    rc, got, _ = raw(gpu, A.d_naf, 0x8000, 0, 1, 0, None, out, n - 1)
    assert rc == E_CAP and got == n and bool((out == 0xEE).all())
    rc, got, nb = raw(gpu, A.d_naf, 0x8000, 0, 1, 0, None, out, n)
    assert rc == 0 and got == n and out.cpu().numpy().tobytes() == want.tobytes()
    monkeypatch.delenv("NAF_GPU_RUNS_PIECE")


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    from naf_amd import capi
    A = planned["all16"][1]["own"]
    N = A.h.n_sequences

    def fails(d_naf, s=0x8000, flags=0, min_len=1, first=0, count=None, words=()):
        import torch
        buf = torch.zeros(32 * 64, dtype=torch.uint8, device="cuda")
        rc, n, nb = raw(gpu, d_naf, s, flags, min_len, first, count, buf, 64)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == E_ARG and n == 0 and nb == 0 and not bool(buf.any()), (rc, msg)
        for w in words:
            assert w in msg, msg
        n2, nb2 = C.c_uint64(5), C.c_uint64(5)
        rc = gpu.L.naf_gpu_unnaf_runs_count(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), s, flags, min_len, first, capi.WHOLE if count is None else count,
                                            C.byref(n2), C.byref(nb2))
        assert rc == E_ARG and n2.value == 0 and nb2.value == 0
        assert all(w in gpu.L.naf_gpu_last_error(gpu.h).decode("latin1") for w in words)

    fails(A.d_naf, s=0, words=("class", "empty"))
    fails(A.d_naf, min_len=0, words=("min_len",))
    fails(A.d_naf, flags=4, words=("flags",))
    fails(A.d_naf, flags=9, words=("flags",))
    fails(A.d_naf, s=0x8000, flags=2, words=("MASKED",))
    fails(A.d_naf, s=0, flags=3, words=("MASKED",))
    fails(A.d_naf, first=N + 1, words=("record", str(N + 1)))
    fails(A.d_naf, first=1, count=N, words=("records", str(N)))
    fails(A.d_naf, s=0, flags=2, first=N + 1, words=("record", str(N + 1)))
    for name, word in (("protein_small", "protein"), ("text_small", "text")):
        d = gpu.to_device(golden_bytes("naf", name + ".naf"))
        fails(d, words=(word,))
        fails(d, s=0, flags=2, words=(word,))
    d = gpu.to_device(no_sequence_archive(oracle))
    fails(d, words=("no sequence",))
    fails(d, s=0, flags=2, words=("no sequence",))
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_runs_count(A.d_naf, 0)
    assert e.value.code == E_ARG
    with pytest.raises(ValueError):
        gpu.unnaf_runs(A.d_naf, "NX")
    # an archive without records, an archive without a mask section: no runs
    E = planned["no_records"][1]["oracle"]
    assert gpu.unnaf_runs_count(E.d_naf, "N") == (0, 0) and gpu.unnaf_runs_count(E.d_naf, None, masked=True) == (0, 0)
    M = planned["nomask"][1]["own"]
    assert not M.has_mask and gpu.unnaf_runs_count(M.d_naf, None, masked=True) == (0, 0) and gpu.unnaf_runs_count(M.d_naf, "N")[0] > 0


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


# ---- 10. the command line ---------------------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_runs_write_bed_lines(gpu, oracle, planned):
    c, arc = planned["seams"]
    A = arc["own"]
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    assert len(ids) == A.h.n_sequences
    r = next(k for k in range(len(A.lines)) if len(A.want(Q_N, 1, k, 1)) > 2)
    for args, q, m, name in ((["--runs", "N"], Q_N, 1, "N"), (["--runs", "^N", "--min-run", "100"], Q_NOT_N, 100, "^N"),
                             (["--runs", "ACGT", "--each", "--min-run", "10"], Q_HOMO, 10, None), (["--masked-runs"], Q_MASK, 1, "mask"),
                             (["--masked-runs", "--min-run", "255"], Q_MASK, 255, "mask")):
        if q == Q_HOMO:
            p = unnaf_cli(args, A.naf)
            assert p.returncode == 0 and p.stderr == b"" and p.stdout == RP.bed(A.want(q, m), ids, name)
        p = unnaf_cli(args + ["--region", ids[r]], A.naf)
        assert p.returncode == 0 and p.stderr == b"" and p.stdout == RP.bed(A.want(q, m, r, 1), ids, name), args
        p = unnaf_cli(args + ["--records", "2-9"], A.naf)
        assert p.returncode == 0 and p.stdout == RP.bed(A.want(q, m, 1, 8), ids, name), args
        assert q == Q_HOMO or len(A.want(q, m, 1, 8)) > 0
    for args in (["--runs", "N", "--region", "nosuch"], ["--masked-runs", "--records", "1-99"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    p = unnaf_cli(["--runs", "N"], golden_bytes("naf", "protein_small.naf"))
    assert p.returncode == 1 and p.stdout == b"" and b"protein" in p.stderr
    # RNA: the letter of code 1 is U
    R = planned["rna"][1]["own"]
    rids = oracle.zstd_decompress(R.h.frame(R.naf, 0)).decode("latin1").split("\0")[:-1]
    p = unnaf_cli(["--runs", "acgu", "--each", "--min-run", "2"], R.naf)
    want = R.want(Q_HOMO, 2)
    assert p.returncode == 0 and p.stdout == RP.bed(want, rids, None, rna=True) and b"\tU\n" in p.stdout


def test_the_contigs_of_a_scaffold_are_the_selected_runs_of_not_n(gpu, planned):
    from naf_amd import capi
    for name in ("lengths", "record_ends"):
        A = planned[name][1]["own"]
        runs, _ = gpu.unnaf_runs(A.d_naf, "^N")
        segs = capi.runs_to_segments(runs)
        got = gpu.unnaf_select(A.d_naf, segs, capi.OUT_SEQUENCES, use_mask=False).cpu().numpy().tobytes()
        contigs = [x for ln in A.lines for x in re.split(b"N+", ln.upper()) if x]
        assert len(contigs) == len(segs) > 3
        assert got == b"".join(x + b"\n" for x in contigs)


def test_cli_runs_table_longer_than_a_download_chunk(gpu, oracle):
    """--runs ACGT --each on one record of 2^20 + 3 bases of ACGT repeated: no two neighbours are equal, so every base is a run; the rows
    are downloaded 2^20 at a time, so the table takes a second download, of 3 rows"""
    n = (1 << 20) + 3
    line = (b"ACGT" * (n // 4 + 1))[:n]
    naf = oracle.ennaf(b">r\n" + line + b"\n")
    assert oracle.unnaf(naf, oracle.MODE_SEQUENCES, True) == line + b"\n"
    p = unnaf_cli(["--runs", "ACGT", "--each"], naf)
    assert p.returncode == 0 and p.stderr == b""
    assert p.stdout == b"".join(b"r\t%d\t%d\t%c\n" % (i, i + 1, line[i]) for i in range(n))
