"""GPU tests of the base composition (naf_gpu_unnaf_composition_rows, naf_gpu_unnaf_composition, unnaf --composition).  Expected rows never
come from the code under test: they are what composition_plan.expected_rows -- numpy over the oracle's --sequences text of the same
archive, mask on -- gives.  Every planned text is counted in two archives, the oracle's and this library's own ennaf at level 1 (the
empty text: the oracle's only); the reference-made golden archives repeat_l19 and repeat_long27 (frames whose blocks depend on each
other) take the whole-decode fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import composition_plan as CP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
CASES = [c.name for c in CP.planned(0)]
GOLDEN_REPEATS = ("repeat_l19", "repeat_long27")
TRACE = re.compile(r"\[composition\] rows (\d+) window (\d+) pieces (\d+) sequence bytes decoded (\d+) of (\d+) mask (\d+) tiles nucleotide (\d+) general (\d+)\n")


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
        self.lines = CP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), self.h.n_sequences)
        self.d_naf = gpu.to_device(naf)
        self._want = {}

    def want(self, window, mask=True, first=0, count=None):
        """expected rows and total, computed once per question and left unchanged"""
        key = (window, first, count)
        if key not in self._want:
            rows = CP.expected_rows(self.lines, window, first, count)
            rows.setflags(write=False)
            self._want[key] = rows
        rows = self._want[key]
        if not mask:
            rows = rows.copy()
            rows["masked"] = 0
        return rows, CP.expected_total(self.lines, rows, first, count)


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive}); the two archives of a text hold the same lines"""
    out = {}
    for c in CP.planned(SEED):
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


def total_tuple(t):
    return (int(t.record), int(t.begin), int(t.end), [int(v) for v in t.n], int(t.masked), int(t.cpg))


def check(gpu, A, window, mask=True, first=0, count=None):
    want, want_total = A.want(window, mask, first, count)
    rows, total = gpu.unnaf_composition(A.d_naf, window, mask, first, count)
    if rows.tobytes() != want.tobytes():
        k = next((i for i in range(min(len(rows), len(want))) if rows[i].tobytes() != want[i].tobytes()), min(len(rows), len(want)))
        raise AssertionError("window %d mask %d records %d+%s: first difference at row %d of %d / %d: got %s, expected %s" % (
            window, mask, first, count, k, len(rows), len(want), CP.as_tuples(rows[k:k + 2]), CP.as_tuples(want[k:k + 2])))
    assert total_tuple(total) == want_total
    assert gpu.unnaf_composition_rows(A.d_naf, window, first, count) == len(want)
    return rows


# ---- 1, 2. the rows, their number and the total --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_rows_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    if which not in arc:
        assert name == "no_records"
        return
    A = arc[which]
    assert A.has_mask or name not in ("seams", "all16", "rna", "r7")
    assert not (A.has_mask and name == "nomask")
    n = 0
    for w in c.windows:
        for mask in (True, False):
            n += len(check(gpu, A, w, mask))
    assert (n > 0) == (name != "no_records")


# ---- 3. the whole-decode fallback -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_REPEATS)
def test_rows_of_the_reference_made_archives(gpu, repeats, name, monkeypatch, capfd):
    A = repeats[name]
    for w in (0, 1000):
        assert len(check(gpu, A, w)) > 0
    last = max(r for r in range(len(A.lines)) if A.lines[r])
    got, tr = traced(gpu, A, 1000, True, last, 1, monkeypatch, capfd)
    assert got.tobytes() == A.want(1000, True, last, 1)[0].tobytes()
    assert tr[3] == tr[4] == (A.h.orig[4] + 1) // 2                                  # dependent blocks: the whole stream, once


# ---- 4. first and count -----------------------------------------------------------------------------------------------------------------
def traced(gpu, A, window, mask, first, count, monkeypatch, capfd, out=None):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    n = gpu.unnaf_composition_rows(A.d_naf, window, first, count)
    import torch
    buf = torch.zeros(max(168 * n, 1), dtype=torch.uint8, device="cuda")
    view, total = gpu.unnaf_composition(A.d_naf, window, mask, first, count, out=buf)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = TRACE.findall(err)
    assert len(m) == (1 if n else 0), err                                            # (the row count decodes nothing and says nothing; no rows: nothing is counted)
    return np.frombuffer(view.cpu().numpy().tobytes(), dtype=CP.ROW_DTYPE), [int(x) for x in m[0]] if m else None


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    c, arc = planned["seams"]
    A = arc[which]
    N = len(A.lines)
    for w in (0, 100):
        whole, _ = A.want(w)
        for r in range(N):
            rows = check(gpu, A, w, True, r, 1)
            assert rows.tobytes() == whole[whole["record"] == r].tobytes()
    for w in (0, 65, 4096):
        whole, _ = A.want(w)
        rows = check(gpu, A, w, True, 3, 9)
        assert rows.tobytes() == whole[(whole["record"] >= 3) & (whole["record"] < 12)].tobytes()
        assert len(check(gpu, A, w, True, 5, 0)) == 0 and len(check(gpu, A, w, True, N, 0)) == 0 and len(check(gpu, A, w, True, N, None)) == 0


def test_a_restricted_count_decodes_only_the_blocks_behind_its_records(gpu, oracle, monkeypatch, capfd):
    rng = np.random.default_rng(8600 + SEED)
    recs = [CP._random(rng, n, "ACGTN") for n in (5000, 300000, 700000, 3001)]
    own, _ = gpu.ennaf(gpu.to_device(CP.fasta(recs, 80)), level=1)
    A = Archive(oracle, gpu, own.cpu().numpy().tobytes())
    assert [x.decode() for x in A.lines] == recs
    T = (A.h.orig[4] + 1) // 2
    for first, count in ((0, 1), (1, 1), (3, 1)):
        got, (R, W, pieces, D, Tt, M, fast, general) = traced(gpu, A, 1000, True, first, count, monkeypatch, capfd)
        assert got.tobytes() == A.want(1000, True, first, count)[0].tobytes()
        assert (R, W, pieces, Tt) == (len(got), 1000, 1, T) and D < T, (first, count, D, T)
    got, tr = traced(gpu, A, 1000, True, 0, None, monkeypatch, capfd)
    assert tr[3] == T


# ---- 5. the piece size does not show -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [5000, 1])
def test_the_result_does_not_depend_on_the_piece_size(gpu, planned, repeats, piece, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_COMPOSITION_PIECE", str(piece))
    for name, windows in (("seams", (0, 100, 4097)), ("fastq", (0, 7)), ("all16", (0, 3)), ("r7", (0, 100))):
        c, arc = planned[name]
        if name == "fastq" and piece == 1:
            continue                                                                # (3000 pieces of one read each: the seams text covers piece = 1)
        for which in ("oracle", "own"):
            for w in windows:
                check(gpu, arc[which], w)
                N = len(arc[which].lines)
                check(gpu, arc[which], w, False, min(2, N - 1), min(5, N - min(2, N - 1)))
    A = planned["seams"][1]["own"]
    got, tr = traced(gpu, A, 100, True, 0, None, monkeypatch, capfd)
    assert got.tobytes() == A.want(100)[0].tobytes() and tr[2] > 1                   # it was counted in pieces
    check(gpu, repeats["repeat_l19"], 1000)
    monkeypatch.delenv("NAF_GPU_COMPOSITION_PIECE")


# ---- 6. the same bytes on every run -------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(gpu, planned):
    for name, w in (("seams", 100), ("fastq", 0), ("all16", 3)):
        A = planned[name][1]["own"]
        a, _ = gpu.unnaf_composition(A.d_naf, w)
        b, _ = gpu.unnaf_composition(A.d_naf, w)
        assert a.tobytes() == b.tobytes() == A.want(w)[0].tobytes()


# ---- 7. buffers ----------------------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, window, flags, first, count, d_rows, cap, total=True):
    from naf_amd import capi
    n, tot = C.c_uint64(12345), capi.CompRow()
    rc = gpu.L.naf_gpu_unnaf_composition(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), window, flags, first, capi.WHOLE if count is None else count,
                                         C.c_void_p(d_rows.data_ptr() if d_rows is not None and d_rows.numel() else 0), cap, C.byref(n), C.byref(tot) if total else None)
    return rc, n.value, tot


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x3C, size=8 << 20)
    for name, w, phases in (("all16", 7, range(16)), ("seams", 4097, (0, 1, 8, 65)), ("fastq", 0, (0, 3, 127))):
        A = planned[name][1][which]
        want, want_total = A.want(w)
        n = len(want)
        assert n >= 2
        for phase in phases:
            # exactly enough: 168 n bytes and nothing outside them
            arena.reset()
            out = arena.out(168 * n, phase)
            rc, total, tot = raw(gpu, A.d_naf, w, 1, 0, None, out, n, total=phase % 2 == 0)
            torch.cuda.synchronize()
            assert rc == 0 and total == n
            arena.check()
            assert out.cpu().numpy().tobytes() == want.tobytes(), (name, phase)
            if phase % 2 == 0:
                assert total_tuple(tot) == want_total
        # one row too few: the whole count, and nothing written
        arena.reset()
        out = arena.out(168 * (n - 1), 5)
        before = out.clone()
        rc, total, _ = raw(gpu, A.d_naf, w, 1, 0, None, out, n - 1)
        torch.cuda.synchronize()
        assert rc == E_CAP and total == n and torch.equal(out, before)
        arena.check()
        assert "rows" in gpu.L.naf_gpu_last_error(gpu.h).decode()
    # the archive in an arena, other bytes around it: the same rows
    A = planned["all16"][1][which]
    want, _ = A.want(16)
    for run, in_phase in ((0, 0), (1, 1), (0, 65)):
        arena.reset()
        before, after = fenced.stream_bait(A.naf, run)
        d_in = arena.put(A.naf, in_phase, before, after)
        out = arena.out(168 * len(want), 16)
        rc, total, _ = raw(gpu, d_in, 16, 1, 0, None, out, len(want))
        torch.cuda.synchronize()
        assert rc == 0 and total == len(want) and out.cpu().numpy().tobytes() == want.tobytes()
        arena.check()
    # the binding's own form with a caller's buffer
    buf = torch.zeros(168 * len(want) + 168, dtype=torch.uint8, device="cuda")
    view, tot = gpu.unnaf_composition(A.d_naf, 16, out=buf)
    assert view.numel() == 168 * len(want) and not bool(buf[168 * len(want):].any()) and view.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_composition(A.d_naf, 16, out=buf[:168 * (len(want) - 1)])
    assert e.value.code == E_CAP


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    from naf_amd import capi
    A = planned["all16"][1]["own"]
    N = A.h.n_sequences

    def fails(d_naf, first=0, count=None, flags=1, words=()):
        import torch
        buf = torch.zeros(168 * 64, dtype=torch.uint8, device="cuda")
        rc, n, _ = raw(gpu, d_naf, 0, flags, first, count, buf, 64)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == E_ARG and n == 0 and not bool(buf.any()), (rc, msg)
        for w in words:
            assert w in msg, msg
        if flags == 1:
            with pytest.raises(capi.NafGpuError) as e:
                gpu.unnaf_composition_rows(d_naf, 0, first, count)
            assert e.value.code == E_ARG and all(w in e.value.msg for w in words)

    fails(A.d_naf, first=N + 1, words=("record", str(N + 1)))
    fails(A.d_naf, first=1, count=N, words=("records", str(N)))
    fails(A.d_naf, flags=2, words=("flags",))
    fails(A.d_naf, flags=3, words=("flags",))
    for name, word in (("protein_small", "protein"), ("text_small", "text")):
        fails(gpu.to_device(golden_bytes("naf", name + ".naf")), words=(word,))
    # an archive that stores no sequence: records whose lengths are all there is (the oracle's archive of a text, cut down to ids and lengths)
    naf = no_sequence_archive(oracle)
    fails(gpu.to_device(naf), words=("no sequence",))


def no_sequence_archive(oracle):
    """An archive of two records without mask and sequence sections: the oracle's archive of a small text with those two sections cut
    out and their flag bits cleared (format: header bytes, then the sections in order, each with its sizes in front)."""
    naf = oracle.ennaf(b">a x\nACGT\n>b\nAC\n", no_mask=True)
    h = oracle.parse_naf(naf)
    assert (h.flags >> 1) & 1 and not (h.flags >> 2) & 1 and h.payload_off[5] is None
    # the sequence section is the last one: it starts at its two size fields, in front of its payload
    o = h.payload_off[4]
    start = o - varlen(h.orig[4]) - varlen(h.comp[4])
    assert start + varlen(h.orig[4]) + varlen(h.comp[4]) + h.comp[4] == len(naf)
    out = bytearray(naf[:start])
    assert out[:4] == b"\x01\xf9\xec\x01" and out[4] == h.flags                      # format 1: the flags follow the version
    out[4] &= ~0x02 & 0xFF
    h2 = oracle.parse_naf(bytes(out))
    assert h2.n_sequences == 2 and not (h2.flags >> 1) & 1
    return bytes(out)


def varlen(v):
    n = 1
    while v >= 128:
        v >>= 7
        n += 1
    return n


# ---- 9. which path counted -----------------------------------------------------------------------------------------------------------------------
def test_the_two_paths_of_the_count_kernel(gpu, planned, monkeypatch, capfd):
    for name, check_paths in (("plain", lambda f, g: f > 0 and g == 0), ("all16", lambda f, g: f == 0 and g > 0), ("sparse_iupac", lambda f, g: f > 10 and g > 10)):
        for which in ("oracle", "own"):
            A = planned[name][1][which]
            for w in (0, 100):
                got, tr = traced(gpu, A, w, True, 0, None, monkeypatch, capfd)
                assert got.tobytes() == A.want(w)[0].tobytes()
                assert check_paths(tr[6], tr[7]), (name, which, w, tr)
                bases = sum(len(x) for x in A.lines)
                assert tr[6] + tr[7] == -(-bases // 4096)


# ---- 10. the command line ---------------------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("name", ["seams", "rna"])
def test_cli_composition_writes_the_table(gpu, oracle, planned, name):
    c, arc = planned[name]
    A = arc["own"]
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    assert len(ids) == A.h.n_sequences
    rna = name == "rna"
    p = unnaf_cli(["--composition"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == CP.table(A.want(0)[0], ids, rna)
    assert p.stdout.count(b"\n") == 1 + len(A.lines) and (b"\tU\t" if rna else b"\tT\t") in p.stdout.split(b"\n")[0]
    p = unnaf_cli(["--composition", "--window", "100"], A.naf)
    assert p.returncode == 0 and p.stdout == CP.table(A.want(100)[0], ids, rna)
    p = unnaf_cli(["--composition", "--window", "4,097", "--records", "2-4"], A.naf)
    assert p.returncode == 0 and p.stdout == CP.table(A.want(4097, True, 1, 3)[0], ids, rna)
    r = 3
    p = unnaf_cli(["--composition", "--region", ids[r]], A.naf)
    assert p.returncode == 0 and p.stdout == CP.table(A.want(0, True, r, 1)[0], ids, rna)
    p = unnaf_cli(["--composition", "--window", "100", "--no-mask"], A.naf)
    assert p.returncode == 0 and p.stdout == CP.table(A.want(100, False)[0], ids, rna)
    assert any(ln.split(b"\t")[10] != b"0" for ln in CP.table(A.want(100)[0], ids, rna).split(b"\n")[1:-1])     # (the masked column is not 0 anyway)
    for args in (["--composition", "--region", "nosuch"], ["--composition", "--records", "1-99"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    if name == "seams":
        p = unnaf_cli(["--composition"], golden_bytes("naf", "protein_small.naf"))
        assert p.returncode == 1 and p.stdout == b"" and b"protein" in p.stderr


def test_cli_composition_table_longer_than_a_download_chunk(gpu, oracle):
    """--window 1 on one record of 2^18 + 3 bases: the rows are downloaded 2^18 at a time, so the table takes a second download, of 3 rows"""
    n = (1 << 18) + 3
    rng = np.random.default_rng(SEED + 77)
    seq = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), n, p=[0.24, 0.24, 0.24, 0.24, 0.04])
    for at in rng.integers(0, n - 64, 200):                          # soft-masked runs of 1 to 63 letters
        seq[at:at + rng.integers(1, 64)] |= 0x20
    seq[(1 << 18) - 3:(1 << 18) + 3] = np.frombuffer(b"nNcGcg", dtype=np.uint8)      # a CpG and the end of a masked run across the chunks' seam
    line = seq.tobytes()
    naf = oracle.ennaf(b">long one\n" + line + b"\n")
    lines = CP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), 1)
    assert lines == [line] and b"n" in line and b"N" in line
    want = CP.table(CP.expected_rows(lines, 1), ["long"])
    p = unnaf_cli(["--composition", "--window", "1"], naf)
    assert p.returncode == 0 and p.stderr == b""
    assert p.stdout.count(b"\n") == n + 1 and p.stdout == want
