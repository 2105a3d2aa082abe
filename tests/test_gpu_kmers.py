"""GPU tests of the k-mer counts (naf_gpu_unnaf_kmers_rows, naf_gpu_unnaf_kmers, unnaf --kmers).  Expected tables never come from the code
under test: they are what kmers_plan.expected_counts / expected_sparse -- numpy over the oracle's --sequences text of the same archive --
give.  Every planned text is asked in two archives, the oracle's and this library's own ennaf at level 1 (the empty text: the oracle's
only); the reference-made golden archives repeat_l19 and repeat_long27 (frames whose blocks depend on each other) take the whole-decode
fallback.  A table is always compared WHOLE: shape, the places of its non-zero counters and their values (and byte for byte where it is
small), so a k-mer missed or counted twice at a seam shows."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kmers_plan as KP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
CASES = [c.name for c in KP.planned(0)]
PER_RECORD_CASES = [c.name for c in KP.planned(0) if c.per_record_ks]
GOLDEN_REPEATS = ("repeat_l19", "repeat_long27")
TRACE = re.compile(r"\[kmers\] k (\d+) rows (\d+) pieces (\d+) sequence bytes decoded (\d+) of (\d+) lds tiles (\d+) global tiles (\d+)\n")
DENSE = 1 << 20                                                                     # tables up to this many counters are compared byte for byte too


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
        self.lines = KP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), self.h.n_sequences)
        self.d_naf = gpu.to_device(naf)
        self._want = {}

    def _cached(self, key, make):
        """expected values, computed once per question and left unchanged"""
        if key not in self._want:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._want[key] = v
        return self._want[key]

    def sparse(self, k, canonical=False, per=False, first=0, count=None):
        return self._cached(("sparse", k, canonical, per, first, count), lambda: KP.expected_sparse(self.lines, k, canonical, per, first, count))

    def dense(self, k, canonical=False, per=False, first=0, count=None):
        return self._cached(("dense", k, canonical, per, first, count), lambda: KP.expected_counts(self.lines, k, canonical, per, first, count))

    def rows(self, k, first=0, count=None):
        return self._cached(("rows", k, first, count), lambda: KP.expected_rows(self.lines, k, first, count))

    def total(self, k, first=0, count=None):
        return self._cached(("total", k, first, count), lambda: KP.expected_total(self.lines, k, first, count))

    def n_records(self, first=0, count=None):
        return (len(self.lines) - first) if count is None else count


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive}); the two archives of a text hold the same lines (the reads: but for the empty ones)"""
    out = {}
    for c in KP.planned(SEED):
        arc = {"oracle": Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type, well_formed=c.well_formed))}
        if c.text:
            own, _ = gpu.ennaf(gpu.to_device(c.own_text or c.text), seq_type=c.seq_type, level=1)
            arc["own"] = Archive(oracle, gpu, own.cpu().numpy().tobytes())
            if c.own_text:                                                          # (the reads: this build's archive is without the empty ones)
                assert arc["own"].lines == [x for x in arc["oracle"].lines if x] and len(arc["own"].lines) < len(arc["oracle"].lines), c.name
            else:
                assert arc["own"].lines == arc["oracle"].lines, c.name
                arc["own"]._want = arc["oracle"]._want
        out[c.name] = (c, arc)
    return out


@pytest.fixture(scope="module")
def repeats(oracle, gpu):
    return {name: Archive(oracle, gpu, golden_bytes("naf", name + ".naf")) for name in GOLDEN_REPEATS}


def tot_tuple(t):
    return (t.record, t.begin, t.end, t.positions, t.counted)


def same_table(counts, A, k, canonical, per, first, count):
    """the whole table: its shape, the places and values of its non-zero counters, and its bytes where it is small"""
    import torch
    n_rows = A.n_records(first, count) if per else 1
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (n_rows, 4 ** k), (counts.shape, n_rows, k)
    flat = counts.reshape(-1)
    nz = torch.nonzero(flat).flatten()
    places, values = nz.cpu().numpy(), flat[nz].cpu().numpy().view(np.uint64)
    wp, wv = A.sparse(k, canonical, per, first, count)
    if not (np.array_equal(places, wp) and np.array_equal(values, wv)):
        got, want = dict(zip(places.tolist(), values.tolist())), dict(zip(wp.tolist(), wv.tolist()))
        diff = sorted(p for p in set(got) | set(want) if got.get(p, 0) != want.get(p, 0))
        raise AssertionError("k %d canonical %s per-record %s records %d+%s: %d counters differ of %d expected; the first: %s" % (
            k, canonical, per, first, count, len(diff), len(want),
            [(p // 4 ** k, KP.kmer_names(k)[p % 4 ** k][1] if k <= 8 else p % 4 ** k, got.get(p, 0), want.get(p, 0)) for p in diff[:6]]))
    if n_rows * 4 ** k <= DENSE:
        assert counts.cpu().numpy().tobytes() == A.dense(k, canonical, per, first, count).tobytes()


def check(gpu, A, k, canonical=False, per=False, first=0, count=None, sizes=True):
    """the tables, the rows, the total and the sizes call"""
    counts, rows, tot = gpu.unnaf_kmers(A.d_naf, k, canonical, per, first, count)
    same_table(counts, A, k, canonical, per, first, count)
    assert tot_tuple(tot) == A.total(k, first, count), (k, canonical, per, first, count, tot_tuple(tot), A.total(k, first, count))
    if per:
        want = A.rows(k, first, count)
        assert rows.tobytes() == want.tobytes(), (k, first, count, rows[:3], want[:3])
        assert np.array_equal(counts.sum(dim=1).cpu().numpy().view(np.uint64), rows["counted"])        # counted == table.sum() in every row
    else:
        assert rows is None
        assert int(counts.sum()) == tot.counted
    if sizes:
        assert gpu.unnaf_kmers_rows(A.d_naf, k, canonical, per, first, count) == (counts.shape[0], counts.shape[0] * 4 ** k)
    return counts


# ---- 1. one table for the selection -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_tables_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    if which not in arc:
        assert name == "no_records"
        return
    A = arc[which]
    for k in c.ks:
        for canonical in (False, True):
            if name == "no_records":
                counts, rows, tot = gpu.unnaf_kmers(A.d_naf, k, canonical)
                assert tuple(counts.shape) == (0, 4 ** k) and rows is None and tot_tuple(tot) == (0, 0, 0, 0, 0)
                assert gpu.unnaf_kmers_rows(A.d_naf, k, canonical) == (0, 0) and gpu.unnaf_kmers_rows(A.d_naf, k, canonical, True) == (0, 0)
            else:
                counts = check(gpu, A, k, canonical)
                assert int(counts.sum()) > 0


# ---- 2. one table per record -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", PER_RECORD_CASES)
def test_tables_per_record(gpu, planned, name, which):
    c, arc = planned[name]
    A = arc[which]
    N = len(A.lines)
    for k in c.per_record_ks:
        first, count = (100, 200) if N * 4 ** k > (1 << 25) else (0, None)          # (the reads at K = 7 and 8: 200 of them)
        for canonical in (False, True) if k <= 6 or name == "two_records" else (k == 7,):
            counts = check(gpu, A, k, canonical, True, first, count)
            assert int(counts.sum()) > 0
    if name == "records":
        short = [r for r in range(N) if len(A.lines[r]) < 4]
        counts = check(gpu, A, 4, False, True)
        assert len(short) >= 6 and not bool(counts[short].any())                    # empty and too-short records: tables of zeros


# ---- 3. the whole-decode fallback -------------------------------------------------------------------------------------------------------
def traced(gpu, A, k, canonical, per, first, count, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    counts, rows, tot = gpu.unnaf_kmers(A.d_naf, k, canonical, per, first, count)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = TRACE.findall(err)
    assert len(m) == 1, err
    same_table(counts, A, k, canonical, per, first, count)
    assert tot_tuple(tot) == A.total(k, first, count)
    return counts, rows, [int(x) for x in m[0]]


@pytest.mark.parametrize("name", GOLDEN_REPEATS)
def test_tables_of_the_reference_made_archives(gpu, repeats, name, monkeypatch, capfd):
    A = repeats[name]
    for k, canonical in ((4, False), (6, True), (7, False), (11, True)):
        assert int(check(gpu, A, k, canonical).sum()) > 0
    check(gpu, A, 3, True, True)
    last = max(r for r in range(len(A.lines)) if A.lines[r])
    _, _, tr = traced(gpu, A, 5, False, False, last, 1, monkeypatch, capfd)
    assert tr[0] == 5 and tr[1] == 1 and tr[3] == tr[4] == (A.h.orig[4] + 1) // 2    # dependent blocks: the whole stream, once


# ---- 4. first and count -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    import torch
    c, arc = planned["records"]
    A = arc[which]
    N = len(A.lines)
    for k, canonical in ((4, True), (7, False)):
        whole = check(gpu, A, k, canonical, True)
        for first, count in ((0, 1), (N - 1, 1), (N, 0), (N, None), (5, 0), (3, 9), (0, None), (N // 2, 3), (1, N - 1), (0, N - 1), (2, 1)):
            last = N if count is None else first + count
            part = check(gpu, A, k, canonical, True, first, count)
            assert torch.equal(part, whole[first:last])
            one = check(gpu, A, k, canonical, False, first, count)
            assert tuple(one.shape) == (1, 4 ** k) and torch.equal(one[0], whole[first:last].sum(dim=0))      # an empty selection: one table of zeros
    S = planned["seams"][1][which]
    M = len(S.lines)
    for first, count in ((0, 1), (M - 2, 2), (7, 30), (M, 0)):
        check(gpu, S, 6, True, False, first, count)
        check(gpu, S, 12, False, False, first, count)


# ---- 5. the trace: what was decoded, and by which path ---------------------------------------------------------------------------------------
def test_a_restricted_query_decodes_only_the_blocks_behind_its_records(gpu, planned, monkeypatch, capfd):
    A = planned["seams"][1]["own"]
    T = (A.h.orig[4] + 1) // 2
    ntiles = (sum(len(x) for x in A.lines) + KP.TILE - 1) // KP.TILE
    _, _, (k, R, pieces, D, Tt, lds, glob) = traced(gpu, A, 6, False, False, 0, None, monkeypatch, capfd)
    assert (k, R, pieces, D, Tt) == (6, 1, 1, T, T) and lds == ntiles and glob == 0  # one row: every tile in LDS bins
    _, _, (k, R, pieces, D, Tt, lds, glob) = traced(gpu, A, 8, True, False, 0, None, monkeypatch, capfd)
    assert (k, R, pieces, D, Tt) == (8, 1, 1, T, T) and lds == 0 and glob == ntiles  # above the LDS limit
    for first, count in ((3, 3), (len(A.lines) - 3, 2)):
        _, _, (k, R, pieces, D, Tt, lds, glob) = traced(gpu, A, 6, False, True, first, count, monkeypatch, capfd)
        assert (k, R, pieces, Tt) == (6, count, 1, T) and 0 < D < T, (first, count, D, T)
    # a tile that holds a record boundary goes to the tables directly, one that lies in one record to the bins
    _, _, (k, R, pieces, D, Tt, lds, glob) = traced(gpu, A, 4, False, True, 0, None, monkeypatch, capfd)
    assert R == len(A.lines) and lds > 0 and glob >= 25 and lds + glob == ntiles
    B = planned["reads"][1]["own"]
    _, _, tr = traced(gpu, B, 4, False, True, 0, None, monkeypatch, capfd)
    assert tr[5] == 0 and tr[6] == (sum(len(x) for x in B.lines) + KP.TILE - 1) // KP.TILE      # reads: a boundary in every tile


# ---- 6. the piece size and the LDS limit do not show ----------------------------------------------------------------------------------------
def pieces_of(lines, first, count, piece):
    """pieces of whole records within `piece` bases, a longer record a piece of its own"""
    lens = [len(x) for x in lines[first:first + count]]
    if sum(lens) <= piece:
        return 1
    n, a = 0, 0
    while a < len(lens):
        b, s = a, 0
        while b < len(lens) and s + lens[b] <= piece:
            s += lens[b]; b += 1
        a = max(b, a + 1)
        n += 1
    return n


@pytest.mark.parametrize("piece", [10 ** 9, 400000, 5000])
def test_the_result_does_not_depend_on_the_piece_size(gpu, planned, repeats, piece, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_KMERS_PIECE", str(piece))
    for which in ("oracle", "own"):
        S, R, F = planned["seams"][1][which], planned["records"][1][which], planned["reads"][1][which]
        for k, canonical in ((6, False), (12, True), (2, True), (7, False)):
            check(gpu, S, k, canonical, sizes=False)                                # the one table accumulates across the pieces
        check(gpu, S, 3, False, True, sizes=False)
        for k in (4, 7):
            check(gpu, R, k, True, True, sizes=False)
            check(gpu, R, k, False, False, 2, len(R.lines) - 5, sizes=False)
        check(gpu, F, 5, False, True, sizes=False)
        check(gpu, planned["r7"][1][which], 4, False, True, sizes=False)
    A = planned["seams"][1]["own"]
    _, _, tr = traced(gpu, A, 6, True, False, 0, None, monkeypatch, capfd)
    want = pieces_of(A.lines, 0, len(A.lines), piece)
    assert tr[2] == want and (want == 1) == (piece == 10 ** 9) and (want == 2) == (piece == 400000), (tr, want)
    check(gpu, repeats["repeat_l19"], 6, True, sizes=False)
    monkeypatch.delenv("NAF_GPU_KMERS_PIECE")


@pytest.mark.parametrize("lds_k", [0, 6])
def test_the_result_does_not_depend_on_the_lds_limit(gpu, planned, lds_k, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_KMERS_LDS_K", str(lds_k))
    for which in ("oracle", "own"):
        S, R = planned["seams"][1][which], planned["records"][1][which]
        for k in (1, 3, 4, 6, 7):
            check(gpu, S, k, k % 2 == 0, sizes=False)
            check(gpu, R, k, k % 2 == 1, True, sizes=False)
        check(gpu, planned["lowk"][1][which], 2, True, True, sizes=False)
    A = planned["seams"][1]["own"]
    _, _, tr = traced(gpu, A, 7, False, False, 0, None, monkeypatch, capfd)
    assert tr[5] == 0 and tr[6] > 0                                                 # K = 7 above either limit: one global atomic per k-mer
    _, _, tr = traced(gpu, A, 6, True, False, 0, None, monkeypatch, capfd)
    assert (tr[5] > 0 and tr[6] == 0) if lds_k == 6 else (tr[5] == 0 and tr[6] > 0)
    monkeypatch.delenv("NAF_GPU_KMERS_LDS_K")
    _, _, tr = traced(gpu, A, 7, False, False, 0, None, monkeypatch, capfd)
    assert tr[5] > 0 and tr[6] == 0                                                 # the default limit is 7: 64 KiB of bins


def test_two_calls_give_identical_bytes(gpu, planned):
    import torch
    for name, k, canonical, per in (("seams", 6, False, False), ("seams", 8, True, False), ("reads", 4, True, True), ("records", 7, False, True), ("lowk", 1, False, False)):
        A = planned[name][1]["own"]
        a, ra, _ = gpu.unnaf_kmers(A.d_naf, k, canonical, per)
        b, rb, _ = gpu.unnaf_kmers(A.d_naf, k, canonical, per)
        assert torch.equal(a, b) and (ra is None or ra.tobytes() == rb.tobytes())
        same_table(a, A, k, canonical, per, 0, None)


# ---- 7. buffers ----------------------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, k, flags, first, count, d_counts, count_cap, d_rows, row_cap, total=True, counts_at=None):
    from naf_amd import capi
    n, nc, tot = C.c_uint64(12345), C.c_uint64(777), capi.KmerRow(9, 9, 9, 9, 9)
    at = counts_at if counts_at is not None else (d_counts.data_ptr() if d_counts is not None and d_counts.numel() else 0)
    rc = gpu.L.naf_gpu_unnaf_kmers(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), k, flags, first, capi.WHOLE if count is None else count,
                                   C.c_void_p(at), count_cap, C.c_void_p(d_rows.data_ptr() if d_rows is not None and d_rows.numel() else 0), row_cap,
                                   C.byref(n), C.byref(nc), C.byref(tot) if total else None)
    return rc, n.value, nc.value, tot_tuple(tot)


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x3C, size=8 << 20)
    for name, k, flags in (("records", 4, 2), ("records", 3, 3), ("lowk", 7, 2), ("palindromes", 6, 1), ("two_records", 2, 0)):
        A = planned[name][1][which]
        per, canonical = bool(flags & 2), bool(flags & 1)
        n = len(A.lines) if per else 1
        nk = 4 ** k
        want = A.dense(k, canonical, per).tobytes()
        want_rows = A.rows(k).tobytes()
        for phase in range(8):
            # exactly enough: 8 n 4^K and 40 n bytes and nothing outside them; the rows at every address phase, the counts at every multiple of 8
            arena.reset()
            out = arena.out(8 * n * nk, 8 * phase)
            rows = arena.out(40 * n, phase) if per else None
            rc, got, gotc, tot = raw(gpu, A.d_naf, k, flags, 0, None, out, n * nk, rows, n, total=phase % 2 == 0)
            torch.cuda.synchronize()
            assert rc == 0 and (got, gotc) == (n, n * nk), (name, phase, rc)
            arena.check()
            assert out.cpu().numpy().tobytes() == want, (name, phase)
            assert tot == (A.total(k) if phase % 2 == 0 else (9, 9, 9, 9, 9))
            if per:
                assert rows.cpu().numpy().tobytes() == want_rows, (name, phase)
            # one counter too few, one row too few: the whole sizes, and nothing written
            for short_counts, short_rows in ((1, 0), (0, 1)) if per else ((1, 0),):
                arena.reset()
                out = arena.out(8 * (n * nk - short_counts), 8 * phase)
                rows = arena.out(40 * (n - short_rows), phase) if per else None
                before, before_rows = out.clone(), rows.clone() if per else None
                rc, got, gotc, tot = raw(gpu, A.d_naf, k, flags, 0, None, out, n * nk - short_counts, rows, n - short_rows)
                torch.cuda.synchronize()
                assert rc == E_CAP and (got, gotc) == (n, n * nk) and torch.equal(out, before) and tot == (0, 0, 0, 0, 0)
                assert not per or torch.equal(rows, before_rows)
                arena.check()
                assert "kmers" in gpu.L.naf_gpu_last_error(gpu.h).decode()
        if per:                                                                     # rows that are not wanted: d_rows NULL, its capacity ignored
            arena.reset()
            out = arena.out(8 * n * nk, 0)
            rc, got, gotc, tot = raw(gpu, A.d_naf, k, flags, 0, None, out, n * nk, None, 0)
            torch.cuda.synchronize()
            assert rc == 0 and (got, gotc) == (n, n * nk) and out.cpu().numpy().tobytes() == want
            arena.check()
    # a d_counts off by 4 bytes
    A = planned["two_records"][1][which]
    arena.reset()
    out = arena.out(8 * 16 + 8, 0)
    before = out.clone()
    rc, got, gotc, tot = raw(gpu, A.d_naf, 2, 0, 0, None, out, 16, None, 0, counts_at=out.data_ptr() + 4)
    torch.cuda.synchronize()
    assert rc == E_ARG and (got, gotc) == (0, 0) and torch.equal(out, before) and "aligned" in gpu.L.naf_gpu_last_error(gpu.h).decode()
    arena.check()
    # the archive in an arena, other bytes around it: the same table
    A = planned["records"][1][which]
    want = A.dense(5, True).tobytes()
    for run, in_phase in ((0, 0), (1, 1), (0, 65)):
        arena.reset()
        before, after = fenced.stream_bait(A.naf, run)
        d_in = arena.put(A.naf, in_phase, before, after)
        out = arena.out(8 * 4 ** 5, 16)
        rc, got, gotc, _ = raw(gpu, d_in, 5, 1, 0, None, out, 4 ** 5, None, 0)
        torch.cuda.synchronize()
        assert rc == 0 and (got, gotc) == (1, 4 ** 5) and out.cpu().numpy().tobytes() == want
        arena.check()
    # the binding's own form with a caller's buffers
    n = len(A.lines)
    buf = torch.full((n * 256 + 7,), -1, dtype=torch.int64, device="cuda")
    rbuf = torch.zeros(40 * n + 40, dtype=torch.uint8, device="cuda")
    counts, rows, tot = gpu.unnaf_kmers(A.d_naf, 4, per_record=True, out=buf, out_rows=rbuf)
    assert counts.data_ptr() == buf.data_ptr() and tuple(counts.shape) == (n, 256) and bool((buf[n * 256:] == -1).all())
    assert counts.cpu().numpy().tobytes() == A.dense(4, False, True).tobytes()
    assert rows.numel() == 40 * n and rows.cpu().numpy().tobytes() == A.rows(4).tobytes() and not bool(rbuf[40 * n:].any())
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_kmers(A.d_naf, 4, per_record=True, out=buf[:n * 256 - 1], out_rows=rbuf)
    assert e.value.code == E_CAP
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_kmers(A.d_naf, 4, per_record=True, out=buf, out_rows=rbuf[:40 * n - 1])
    assert e.value.code == E_CAP


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------------------
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

    def fails(d_naf, k=4, flags=0, first=0, count=None, words=()):
        buf = torch.zeros(8 * 256 * 64, dtype=torch.uint8, device="cuda")
        rows = torch.zeros(40 * 64, dtype=torch.uint8, device="cuda")
        rc, n, nc, tot = raw(gpu, d_naf, k, flags, first, count, buf, 256 * 64, rows, 64)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == E_ARG and (n, nc) == (0, 0) and tot == (0, 0, 0, 0, 0) and not bool(buf.any()) and not bool(rows.any()), (rc, msg)
        for w in words:
            assert w in msg, msg
        n2, nc2 = C.c_uint64(5), C.c_uint64(5)
        rc = gpu.L.naf_gpu_unnaf_kmers_rows(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), k, flags, first, capi.WHOLE if count is None else count,
                                            C.byref(n2), C.byref(nc2))
        assert rc == E_ARG and (n2.value, nc2.value) == (0, 0)
        assert all(w in gpu.L.naf_gpu_last_error(gpu.h).decode("latin1") for w in words)

    fails(A.d_naf, k=0, words=("kmers", "k 0"))
    fails(A.d_naf, k=13, words=("kmers", "k 13"))
    fails(A.d_naf, k=4096, words=("kmers", "k 4096"))
    fails(A.d_naf, flags=4, words=("flags",))
    fails(A.d_naf, flags=9, words=("flags",))
    fails(A.d_naf, flags=-1, words=("flags",))
    fails(A.d_naf, first=N + 1, words=("record", str(N + 1)))
    fails(A.d_naf, first=1, count=N, words=("records", str(N)))
    fails(A.d_naf, flags=2, first=N + 1, words=("record", str(N + 1)))
    for name, word in (("protein_small", "protein"), ("text_small", "text")):
        d = gpu.to_device(golden_bytes("naf", name + ".naf"))
        fails(d, words=(word,))
        fails(d, flags=3, words=(word,))
    d = gpu.to_device(no_sequence_archive(oracle))
    fails(d, words=("no sequence",))
    for k in (0, 13):
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_kmers(A.d_naf, k)
        assert e.value.code == E_ARG
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_kmers_rows(A.d_naf, k)
        assert e.value.code == E_ARG


# ---- 9. the command line ---------------------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def ids_of(oracle, A):
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    assert len(ids) == A.h.n_sequences
    return ids


def test_cli_kmers_write_both_tables(gpu, oracle, planned):
    A = planned["records"][1]["own"]
    ids = ids_of(oracle, A)
    N = len(ids)
    r = next(k for k in range(N) if len(A.lines[k]) == 4097)
    for k, canonical in ((1, False), (3, True), (6, False), (8, True), (12, False)):
        args = ["--kmers", str(k)] + (["--canonical"] if canonical else [])
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 0 and p.stderr == b"" and p.stdout == KP.cli_total(A.dense(k, canonical) if k < 12 else KP.expected_counts(A.lines, k, canonical), k), args
        p = unnaf_cli(args + ["--region", ids[r]], A.naf)
        assert p.returncode == 0 and p.stderr == b"" and p.stdout == KP.cli_total(KP.expected_counts(A.lines, k, canonical, False, r, 1), k), args
        p = unnaf_cli(args + ["--records", "2-30"], A.naf)
        assert p.returncode == 0 and p.stdout == KP.cli_total(KP.expected_counts(A.lines, k, canonical, False, 1, 29), k) and p.stdout, args
    for k, canonical in ((1, True), (2, False), (4, True), (6, True)):
        args = ["--kmers", str(k), "--per-record"] + (["--canonical"] if canonical else [])
        p = unnaf_cli(args, A.naf)
        want = KP.cli_per_record(A.dense(k, canonical, True), A.rows(k), ids, k, canonical)
        assert p.returncode == 0 and p.stderr == b"" and p.stdout == want and p.stdout.count(b"\n") == N + 1, args
        p = unnaf_cli(args + ["--records", "3-20"], A.naf)
        assert p.returncode == 0 and p.stdout == KP.cli_per_record(KP.expected_counts(A.lines, k, canonical, True, 2, 18), A.rows(k, 2, 18), ids, k, canonical), args
        p = unnaf_cli(args + ["--region", ids[r]], A.naf)
        assert p.returncode == 0 and p.stdout == KP.cli_per_record(KP.expected_counts(A.lines, k, canonical, True, r, 1), A.rows(k, r, 1), ids, k, canonical), args
    assert len(KP.kmer_names(4, True)) == 136 and len(KP.kmer_names(3, True)) == 32 # only the canonical names appear
    # many calls of a few records each: the reads at K = 6 (1024 records a call, two calls)
    F = planned["reads"][1]["own"]
    fids = ids_of(oracle, F)
    p = unnaf_cli(["--kmers", "6", "--per-record", "--canonical", "--records", "1-1100"], F.naf)
    assert p.returncode == 0 and p.stdout == KP.cli_per_record(KP.expected_counts(F.lines, 6, True, True, 0, 1100), F.rows(6, 0, 1100), fids, 6, True)
    for args in (["--kmers", "4", "--region", "nosuch"], ["--kmers", "4", "--per-record", "--records", "1-99"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    p = unnaf_cli(["--kmers", "4"], golden_bytes("naf", "protein_small.naf"))
    assert p.returncode == 1 and p.stdout == b"" and b"protein" in p.stderr
    # RNA: the letter of index 3 is U
    R = planned["rna"][1]["own"]
    rids = ids_of(oracle, R)
    p = unnaf_cli(["--kmers", "3"], R.naf)
    assert p.returncode == 0 and p.stdout == KP.cli_total(R.dense(3), 3, rna=True) and b"UUU\t" in p.stdout and b"T" not in p.stdout
    p = unnaf_cli(["--kmers", "2", "--per-record", "--canonical"], R.naf)
    assert p.returncode == 0 and p.stdout == KP.cli_per_record(R.dense(2, True, True), R.rows(2), rids, 2, True, rna=True) and b"\tAU\t" in p.stdout.split(b"\n")[0]
    # an archive without records: no line, and the header line alone
    E = planned["no_records"][1]["oracle"]
    p = unnaf_cli(["--kmers", "5"], E.naf)
    assert p.returncode == 0 and p.stdout == b""
    p = unnaf_cli(["--kmers", "1", "--per-record"], E.naf)
    assert p.returncode == 0 and p.stdout == b"#seq\tlength\tcounted\tA\tC\tG\tT\n"
