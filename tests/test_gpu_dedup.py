"""GPU tests of duplicate collapsing (naf_gpu_unnaf_dedup, unnaf --dedup).  Expected rows never come from the code under test: they are
what dedup_plan.model gives for the records of the oracle's text of the same archive, and the expected texts are cut out of that text.
Every planned text is swept in the oracle's archive (raw 128 KiB blocks) and in this library's own ennaf at level 1."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import clip_plan as CP
import dedup_plan as DP
import trim_plan as TP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
CASES = [c.name for c in DP.planned(0)]
TRACE = re.compile(r"\[dedup\] records (\d+) considered (\d+) classes (\d+) rounds (\d+) verified (\d+) sequence bytes decoded (\d+) of (\d+)\n")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


class Archive:
    def __init__(self, oracle, gpu, naf, case, shared=None):
        self.naf, self.case = naf, case
        self.h = oracle.parse_naf(naf)
        self.N = self.h.n_sequences
        self.records = oracle.unnaf(naf, oracle.MODE_SEQUENCES, True).decode("latin1").split("\n")[:-1] if self.N else []
        self.lens = [len(r) for r in self.records]
        self.ids = case.ids
        self.d_naf = gpu.to_device(naf)
        self._want = shared._want if shared is not None else {}
        self.oracle = oracle

    def want(self, both=False, bset=None):
        """(rows, total, levels) of the whole archive, computed once per question and left unchanged"""
        key = (both, bset)
        if key not in self._want:
            rows, total, levels = DP.model(self.records, both, self.case.bounds(bset) if bset else None)
            rows.setflags(write=False)
            self._want[key] = (rows, total, levels)
        return self._want[key]

    def fastq(self):
        return self.oracle.unnaf(self.naf, self.oracle.MODE_FASTQ)


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive})"""
    out = {}
    for c in DP.planned(SEED):
        a = Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type, well_formed=c.fmt == "fastq"), c)
        assert [DP.canon(r) for r in a.records] == [DP.canon(r) for r in c.records], c.name
        own, _ = gpu.ennaf(gpu.to_device(c.text), seq_type=c.seq_type, level=1)
        b = Archive(oracle, gpu, own.cpu().numpy().tobytes(), c, a)
        assert b.records == a.records, c.name
        out[c.name] = (c, {"oracle": a, "own": b})
    return out


def differ(what, got, want, where):
    if got.tobytes() != want.tobytes():
        k = next((i for i in range(min(len(got), len(want))) if got[i].tobytes() != want[i].tobytes()), min(len(got), len(want)))
        raise AssertionError("%s %s: first difference at row %d of %d / %d: got %s, expected %s" % (what, where, k, len(got), len(want), got[k:k + 2].tolist(), want[k:k + 2].tolist()))


def total_tuple(t):
    return (int(t.reads), int(t.considered), int(t.classes), int(t.duplicates), int(t.singletons), int(t.largest), int(t.bases), int(t.kept_bases))


def check(gpu, A, both=False, bset=None, kind="trim", first=0, count=None):
    if (first, count) == (0, None):
        rows_w, total_w, levels_w = A.want(both, bset)
    else:                                                                               # classes form inside the window only
        rows_w, total_w, levels_w = DP.model(A.records, both, A.case.bounds(bset) if bset else None, first, count)
    last = A.N if count is None else first + count
    bounds = gpu.to_device(DP.bounds_rows(A.case.bounds(bset)[first:last], kind, first)) if bset and last > first else None
    where = "%s both %s bounds %s %s records %d+%s" % (A.case.name, both, bset, kind, first, count)
    rows, total, levels = gpu.unnaf_dedup(A.d_naf, both, bounds=bounds, bounds_kind=kind, first=first, count=count)
    differ("rows", rows, rows_w, where)
    assert total_tuple(total) == total_w, where
    assert levels == levels_w, where
    return rows


# ---- 1. the rows of the planned texts, with and without both strands ------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_rows_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    A = arc[which]
    for both in (False, True):
        got = {None: check(gpu, A, both)}
        assert len(got[None]) == A.N
        for k, bs in enumerate(sorted(c.bsets)):
            got[bs] = check(gpu, A, both, bs, ("trim", "clip")[(k + both) % 2])
            check(gpu, A, both, bs, ("clip", "trim")[(k + both) % 2])
        for p in c.plants:                                                              # the plants have the rows they were planted to have
            assert DP.holds(p, got[p.bset], both), (p.cell, p.kind, p.off, p.name, p.rel, both)


# ---- 2. the lever: the same tables whatever the hashes are cut to ----------------------------------------------------------------------
CHILD = """
import hashlib, sys
from naf_amd import capi
ctx = capi.Context(0)
for path in sys.argv[1:]:
    d = ctx.to_device(open(path, "rb").read())
    for both in (False, True):
        rows, t, levels = ctx.unnaf_dedup(d, both)
        print(len(rows), hashlib.sha256(rows.tobytes()).hexdigest(), t.reads, t.considered, t.classes, t.duplicates, t.singletons, t.largest, t.bases, t.kept_bases, *levels)
ctx.close()
"""


@pytest.mark.parametrize("bits", [64, 6, 2, 0])
def test_the_result_does_not_depend_on_the_hash_bits(planned, bits, tmp_path):
    """NAF_GPU_DEDUP_HASH_BITS is read when the library starts: a fresh process per value.  At 2 and 0 different sequences share a hash:
    the comparison of the codes and the later rounds decide, and the trace shows that they ran."""
    env = dict(os.environ, NAF_GPU_DEDUP_HASH_BITS=str(bits), NAF_GPU_TRACE="1", PYTHONPATH=ROOT)
    names = list(DP.SMALL_CASES) + (["seams0", "long", "classes", "fastq"] if bits >= 6 else []) + (["ones"] if bits == 64 else [])
    use = [planned[n][1]["own" if k % 2 else "oracle"] for k, n in enumerate(names)]
    for k, A in enumerate(use):
        (tmp_path / ("%d.naf" % k)).write_bytes(A.naf)
    p = subprocess.run([sys.executable, "-c", CHILD] + [str(tmp_path / ("%d.naf" % k)) for k in range(len(use))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().split("\n")
    tr = TRACE.findall(p.stderr.decode())
    assert len(tr) == 2 * len(use), p.stderr.decode()
    for k, A in enumerate(use):
        for j, both in enumerate((False, True)):
            rows, total, levels = A.want(both)
            assert out[2 * k + j].split() == [str(x) for x in (len(rows), hashlib.sha256(rows.tobytes()).hexdigest()) + total + tuple(levels)], (A.case.name, both, bits)
            R, considered, classes, rounds, verified, dec, of = (int(x) for x in tr[2 * k + j])
            assert (R, considered, classes, dec, of) == (A.N, total[1], total[2], (sum(A.lens) + 1) // 2, (sum(A.lens) + 1) // 2), (A.case.name, both, bits)
            assert rounds >= 1 and (verified >= total[3])                                # every duplicate was confirmed by its codes
            if bits <= 2 and total[2] > 16:
                assert rounds > 1 and verified > total[3], (A.case.name, both, bits, rounds, verified)
            if bits == 64:
                assert rounds == 1 and verified == total[3], (A.case.name, both, rounds, verified)


# ---- 3. first and count: classes form inside the window only ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    for name, bset in (("seams0", None), ("seams0", "win"), ("classes", None), ("bounds", "cut"), ("strand", None)):
        c, arc = planned[name]
        A = arc[which]
        N = A.N
        plants = [p.b for p in c.plants]
        runs = [(0, 1), (N - 1, 1), (N, 0), (N, None), (5, 0), (N // 2, None), (0, 2), (N - 2, 2), (1, 1), (plants[3], 1), (plants[3] - 1, 3), (plants[len(plants) // 2], None), (0, plants[len(plants) // 2])]
        empty = [r for r in range(N) if not A.lens[r]]
        runs += [(r, 1) for r in empty[:3]] + ([(empty[-1] - 1, 2)] if empty else [])
        for k, (first, count) in enumerate(runs):
            check(gpu, A, bool(k % 2), bset, ("trim", "clip")[k % 2], first, count)


def test_a_window_at_the_far_end_decodes_only_its_blocks(gpu, planned, monkeypatch, capfd):
    A = planned["seams0"][1]["oracle"]
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    check(gpu, A, False, None, "trim", A.N - 6, 6)
    check(gpu, A)
    tr = TRACE.findall(capfd.readouterr().err)
    monkeypatch.delenv("NAF_GPU_TRACE")
    assert len(tr) == 2 and int(tr[0][0]) == 6
    assert 0 < int(tr[0][5]) < int(tr[0][6]) == (sum(A.lens) + 1) // 2 == int(tr[1][5]) and int(tr[1][2]) == A.want()[1][2]


# ---- 4. bounds that never leave the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_bounds_from_unnaf_trim_and_unnaf_clip(gpu, planned, which):
    import torch
    c, arc = planned["fastq"]
    A = arc[which]
    quals = TP.quals_of(A.fastq(), A.N)
    assert quals == c.quals
    q = CP.Query([c.adapter])
    for limit, min_len, max_ee in ((TP.LIMITS["Q20"], 1, TP.NO_MAX), (TP.LIMITS["Q20"], 100, TP.ee_units("0.06"))):
        trows, _ = TP.model(quals, limit, min_len, max_ee)
        tb = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in trows]
        tbuf = torch.zeros(40 * A.N, dtype=torch.uint8, device="cuda")
        tview, _ = gpu.unnaf_trim(A.d_naf, limit, min_len, None if max_ee == TP.NO_MAX else max_ee, out=tbuf)
        assert tview.cpu().numpy().tobytes() == trows.tobytes()
        crows, _, _ = CP.model(A.records, q, min_len, tb)
        cb = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in crows]
        cbuf = torch.zeros(40 * A.N, dtype=torch.uint8, device="cuda")
        cview, _, _ = gpu.unnaf_clip(A.d_naf, q.adapters, budgets=q.budgets, min_overlap=q.min_overlap, min_len=min_len, bounds=tview, out=cbuf)
        assert cview.cpu().numpy().tobytes() == crows.tobytes()
        for both in (False, True):
            for view, bounds, kind in ((tview, tb, "trim"), (cview, cb, "clip")):
                want, total_w, levels_w = DP.model(A.records, both, bounds)
                rows, total, levels = gpu.unnaf_dedup(A.d_naf, both, bounds=view, bounds_kind=kind)
                differ("rows", rows, want, "limit %d min_len %d both %s %s" % (limit, min_len, both, kind))
                assert total_tuple(total) == total_w and levels == levels_w
                assert total_w[3] > 20 and (kind == "trim" or (rows["flags"] & DP.CLIPPED != 0).sum() > 50)
                assert min_len == 1 or ((rows["flags"] & DP.ERRORS != 0).any() and (rows["flags"] & DP.SHORT != 0).any() and total_w[1] < A.N)


# ---- 5. buffers -----------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, flags, kind, first, count, d_bounds, d_rows, cap, total=True, levels=True):
    from naf_amd import capi
    n, tot, lev = C.c_uint64(12345), capi.DedupTotal(), (C.c_uint64 * 16)(*([77] * 16))
    o = capi.DedupOpts(flags, kind)
    rc = gpu.L.naf_gpu_unnaf_dedup(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), C.byref(o), first, capi.WHOLE if count is None else count,
                                   C.c_void_p(d_bounds.data_ptr()) if d_bounds is not None else None, C.c_void_p(d_rows.data_ptr()) if d_rows is not None else None, cap,
                                   C.byref(n), C.byref(tot) if total else None, lev if levels else None)
    return rc, n.value, tot, [int(v) for v in lev]


def test_totals_only(gpu, planned):
    for name in ("seams1", "long", "ones"):
        A = planned[name][1]["own"]
        rows, total, levels = gpu.unnaf_dedup(A.d_naf, True, out=False)
        assert rows is None and total_tuple(total) == A.want(True)[1] and levels == A.want(True)[2]
        rc, n, tot, lev = raw(gpu, A.d_naf, 0, 0, 0, 2, None, None, 0, total=False, levels=False)
        assert rc == 0 and n == 2 and lev == [77] * 16


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x7A, size=8 << 20)
    for name, bset, kind in (("seams1", "win", "clip"), ("bounds", "cut", "trim"), ("strand", None, "trim")):
        A = planned[name][1][which]
        rows_w, total_w, levels_w = A.want(True, bset)
        n = len(rows_w)
        bt = DP.bounds_rows(A.case.bounds(bset), kind) if bset else None
        for phase in (0, 1, 31):
            arena.reset()
            d_bounds = arena.put(bt, (phase * 7 + 1) % 128) if bt is not None else None  # the bounds at a phase of their own
            d_rows = arena.out(48 * n, phase)                                            # exactly enough: 48 bytes a row and nothing outside them
            rc, got, tot, lev = raw(gpu, A.d_naf, 1, kind == "clip", 0, None, d_bounds, d_rows, n, total=phase != 1, levels=phase != 31)
            torch.cuda.synchronize()
            assert rc == 0 and got == n
            arena.check()
            assert d_rows.cpu().numpy().tobytes() == rows_w.tobytes(), (name, phase)
            assert phase == 1 or total_tuple(tot) == total_w
            assert phase == 31 or lev == levels_w
        arena.reset()                                                                   # one row too few: the whole count, nothing written
        d_rows = arena.out(48 * (n - 1), 5)
        before = d_rows.clone()
        rc, got, tot, lev = raw(gpu, A.d_naf, 1, 0, 0, None, None, d_rows, n - 1)
        torch.cuda.synchronize()
        assert rc == E_CAP and got == n and torch.equal(d_rows, before) and "rows" in gpu.L.naf_gpu_last_error(gpu.h).decode()
        arena.check()
        arena.reset()                                                                   # a window into a table of its own size
        d_rows = arena.out(48 * 7, 31)
        rc, got, tot, lev = raw(gpu, A.d_naf, 0, 0, 3, 7, None, d_rows, 7)
        torch.cuda.synchronize()
        assert rc == 0 and got == 7 and d_rows.cpu().numpy().tobytes() == DP.model(A.records, False, None, 3, 7)[0].tobytes()
        arena.check()
    A = planned["tail0"][1]["oracle"]                                                   # the archive in an arena, other bytes around it
    for run, in_phase in ((0, 0), (1, 1), (0, 65)):
        arena.reset()
        before, after = fenced.stream_bait(A.naf, run)
        d_in = arena.put(A.naf, in_phase, before, after)
        d_rows = arena.out(48 * A.N, 9)
        rc, got, tot, lev = raw(gpu, d_in, 1, 0, 0, None, None, d_rows, A.N)
        torch.cuda.synchronize()
        assert rc == 0 and d_rows.cpu().numpy().tobytes() == A.want(True)[0].tobytes()
        arena.check()
    A = planned["long"][1][which]                                                       # the binding's own form with the caller's buffer
    buf = torch.zeros(48 * A.N + 48, dtype=torch.uint8, device="cuda")
    view, tot, lev = gpu.unnaf_dedup(A.d_naf, True, out=buf)
    assert view.numel() == 48 * A.N and not bool(buf[48 * A.N:].any()) and view.cpu().numpy().tobytes() == A.want(True)[0].tobytes()
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_dedup(A.d_naf, out=buf[:48 * (A.N - 1)])
    assert e.value.code == E_CAP


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    import torch
    A = planned["seams1"][1]["own"]
    N = A.N

    def fails(d_naf=A.d_naf, words=(), flags=0, kind=0, first=0, count=None, d_bounds=None):
        buf = torch.zeros(48 * 64, dtype=torch.uint8, device="cuda")
        rc, n, tot, lev = raw(gpu, d_naf, flags, kind, first, count, d_bounds, buf, 64)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == E_ARG and n == 0 and not bool(buf.any()) and total_tuple(tot) == (0,) * 8 and lev == [0] * 16, (rc, n, msg)
        for w in words:
            assert w in msg, msg

    fails(flags=2, words=("flags 2",))
    fails(flags=1 | 4, words=("flags 5",))
    fails(kind=2, words=("bounds_kind 2",))
    fails(first=N + 1, words=("record", str(N + 1)))
    fails(first=1, count=N, words=("records", str(N)))
    fails(d_naf=gpu.to_device(golden_bytes("naf", "protein_small.naf")), words=("duplicates cannot be collapsed in protein sequences",))
    # bounds rows that are none: found on the device, nothing written
    for kind in ("trim", "clip"):
        good = [(0, A.lens[r], 1) for r in range(5, 69)]
        for k, field, value, word in ((9, "record", 15, "its record"), (3, "begin", A.lens[8] + 1, "begin > end"), (60, "end", A.lens[65] + 1, "behind the record's last base")):
            t = np.frombuffer(DP.bounds_rows(good, kind, 5), dtype=TP.ROW_DTYPE if kind == "trim" else CP.ROW_DTYPE).copy(); t[field][k] = value
            fails(first=5, count=64, kind=kind == "clip", d_bounds=gpu.to_device(t.tobytes()), words=("bounds row %d" % k, word))
        t = np.frombuffer(DP.bounds_rows(good, kind, 5), dtype=TP.ROW_DTYPE if kind == "trim" else CP.ROW_DTYPE).copy(); t["end"][60] += 1; t["record"][9] = 0
        fails(first=5, count=64, kind=kind == "clip", d_bounds=gpu.to_device(t.tobytes()), words=("bounds row 9",))      # two of them: the first is named
        buf = torch.zeros(48 * 64, dtype=torch.uint8, device="cuda")                      # and the rows as they stand are fine
        rc, n, tot, lev = raw(gpu, A.d_naf, 0, kind == "clip", 5, 64, gpu.to_device(DP.bounds_rows(good, kind, 5)), buf, 64)
        assert rc == 0 and n == 64 and buf.cpu().numpy().tobytes() == DP.model(A.records, False, None, 5, 64)[0].tobytes()
    # after an error return the same table
    check(gpu, A, True)


def test_archives_without_records_and_without_quality(gpu, planned, oracle):
    empty = gpu.to_device(oracle.ennaf(b""))
    rows, total, levels = gpu.unnaf_dedup(empty, True)
    assert len(rows) == 0 and total_tuple(total) == (0,) * 8 and levels == [0] * 16
    d = gpu.to_device(golden_bytes("naf", "acgt_10k.naf"))                              # FASTA: no quality section
    assert not oracle.parse_naf(golden_bytes("naf", "acgt_10k.naf")).flags & 1
    recs = oracle.unnaf(golden_bytes("naf", "acgt_10k.naf"), oracle.MODE_SEQUENCES, True).decode("latin1").split("\n")[:-1]
    for both in (False, True):
        want, total_w, levels_w = DP.model(recs, both)
        rows, total, levels = gpu.unnaf_dedup(d, both)
        differ("rows", rows, want, "acgt_10k")
        assert total_tuple(total) == total_w and levels == levels_w


def test_the_same_table_on_a_fresh_context_and_after_release_scratch(gpu, planned):
    from naf_amd import capi
    A = planned["seams0"][1]["own"]
    want, total, levels = A.want(True)
    a, ta, la = gpu.unnaf_dedup(A.d_naf, True)
    gpu.unnaf(planned["rna"][1]["oracle"].d_naf, capi.OUT_FASTA)                        # an unrelated call on the same context in between
    b, tb, lb = gpu.unnaf_dedup(A.d_naf, True)
    assert a.tobytes() == b.tobytes() == want.tobytes() and total_tuple(ta) == total_tuple(tb) == total and la == lb == levels
    assert gpu.L.naf_gpu_release_scratch(gpu.h) == 0
    c, tc, lc = gpu.unnaf_dedup(A.d_naf, True)                                          # directly after the scratch was given back
    assert c.tobytes() == want.tobytes() and total_tuple(tc) == total and lc == levels
    fresh = capi.Context(0)
    try:
        d, td, ld = fresh.unnaf_dedup(fresh.to_device(A.naf), True)
        assert d.tobytes() == want.tobytes() and total_tuple(td) == total and ld == levels
    finally:
        fresh.close()


# ---- 7. the firsts as reads -----------------------------------------------------------------------------------------------------------
def text_of(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_select_reads_writes_the_firsts(gpu, planned, which):
    from naf_amd import capi
    A = planned["fastq"][1][which]
    text = A.fastq()
    rows = check(gpu, A, True)
    segs = capi.dedup_to_segments(rows)
    assert segs == DP.kept_segments(A.want(True)[0]) and 500 < len(segs) < A.N - 100
    for fmt, out_type, L in (("fastq", capi.OUT_FASTQ, -1), ("fasta", capi.OUT_FASTA, 0), ("fasta", capi.OUT_FASTA, 1), ("fasta", capi.OUT_FASTA, 60),
                             ("sequences", capi.OUT_SEQUENCES, -1), ("seq", capi.OUT_SEQ, -1)):
        want = TP.expected_text(text, A.N, segs, fmt, max(L, 0))
        got = text_of(gpu.unnaf_select_reads(A.d_naf, segs, out_type, line_length=L))
        assert got == want, (fmt, L, len(got), len(want))


def fasta_reads(A, segs, line_length):
    """the reads of a FASTA archive cut out of the oracle's --fasta text"""
    recs = A.oracle.unnaf(A.naf, A.oracle.MODE_FASTA, True).split(b">")[1:]
    out = []
    for r, b, e in segs:
        head, _, body = recs[r].partition(b"\n")
        seq = body.replace(b"\n", b"")[b:e]
        W = line_length or len(seq)
        out += [b">", head, b"\n"] + [seq[i:i + W] + b"\n" for i in range(0, len(seq), W or 1)]
    return b"".join(out)


# ---- 8. the command line --------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_dedup_writes_the_reads_and_the_table(gpu, planned):
    c, arc = planned["fastq"]
    A = arc["own"]
    text = A.fastq()
    p = unnaf_cli(["--dedup"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, DP.kept_segments(A.want(False)[0]), "fastq")
    p = unnaf_cli(["--dedup", "--either-strand", "--fasta", "--line-length", "60"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, DP.kept_segments(A.want(True)[0]), "fasta", 60)
    p = unnaf_cli(["--dedup", "--dedup-table"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == DP.table(A.want(False)[0], A.ids, A.lens)
    p = unnaf_cli(["--dedup", "--dedup-table", "--either-strand", "--records", "3-700"], A.naf)
    assert p.returncode == 0 and p.stdout == DP.table(DP.model(A.records, True, None, 2, 698)[0], A.ids, A.lens)
    assert {line.split(b"\t")[-2] for line in p.stdout.split(b"\n")[1:-1]} == {b"+", b"-"}
    # quality trimming and adapter clipping first, on the device: the dedup call's bounds
    quals = TP.quals_of(text, A.N)
    trows, _ = TP.model(quals, TP.LIMITS["Q20"], 100, TP.ee_units("0.06"))
    tb = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in trows]
    crows = CP.model(A.records, CP.Query([c.adapter]), 100, tb)[0]
    cb = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in crows]
    want = DP.model(A.records, True, cb)[0]
    p = unnaf_cli(["--dedup", "--either-strand", "--trim", "20", "--adapter", c.adapter, "--min-length", "100", "--max-ee", "0.06"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, DP.kept_segments(want), "fastq")
    p = unnaf_cli(["--adapter", c.adapter, "--trim", "20", "--dedup", "--either-strand", "--min-length", "100", "--max-ee", "0.06", "--dedup-table"], A.naf)
    assert p.returncode == 0 and p.stdout == DP.table(want, A.ids, A.lens)
    assert {line.split(b"\t")[-1] for line in p.stdout.split(b"\n")[1:-1]} == {b"first", b"duplicate", b"short", b"errors", b"short,errors"}
    want = DP.model(A.records, False, tb)[0]
    p = unnaf_cli(["--dedup", "--trim", "20", "--min-length", "100", "--max-ee", "0.06", "--seq"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, DP.kept_segments(want), "seq")
    F = planned["classes"][1]["own"]                                                    # a FASTA archive with empty records: FASTA reads by default
    segs = DP.kept_segments(F.want(False)[0])
    p = unnaf_cli(["--dedup", "--line-length", "0"], F.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == fasta_reads(F, segs, 0) and len(segs) == 10
    p = unnaf_cli(["--dedup", "--dedup-table"], F.naf)
    assert p.returncode == 0 and p.stdout == DP.table(F.want(False)[0], F.ids, F.lens)
    p = unnaf_cli(["--dedup", "--trim", "20"], F.naf)
    assert p.returncode == 1 and b"no quality" in p.stderr and p.stdout == b""
    for args in (["--dedup", "--region", "nosuch"], ["--dedup", "--records", "1-99999"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args


# ---- 13. who takes part, at the wave and workgroup seams of a launch with a lane per record ------------------------------------------------
def test_considered_and_who_takes_part_at_the_seams_of_a_launch(oracle, gpu):
    """513 reads of 8 to 12 bases, a third of them copies; the bounds rows carry NAF_GPU_TRIM_KEPT for exactly the first n, the last n and
    every n-th record, n at 1, the wavefront's 64 and the workgroup's 256 and beside them, and 513.  `considered` is the number of set
    bits, and a read that takes no part has its row as it went in."""
    B = DP.Builder(7300 + SEED)
    for k in range(513):
        B.add(B.reads[int(B.rng.integers(0, k))] if k % 3 == 2 else B.bg(int(B.rng.integers(8, 13))))
    c = DP.Case("short", B, lower=False)
    A = Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type), c)
    assert A.N == 513 and A.records == c.records and min(A.lens) >= 8 and max(A.lens) <= 12
    for k, (name, takes) in enumerate(DP.part_sets(A.N)):
        bounds = DP.part_bounds(A.lens, takes)
        both = bool(k % 2)
        want, total_w, levels_w = DP.model(A.records, both, bounds)
        rows, total, levels = gpu.unnaf_dedup(A.d_naf, both, bounds=gpu.to_device(DP.bounds_rows(bounds, "trim")), bounds_kind="trim")
        differ("rows", rows, want, name)
        print(name, "considered", int(total.considered), "of", sum(takes))
        assert total_tuple(total) == total_w and levels == levels_w, name
        assert int(total.considered) == sum(takes), name
        out = [r for r, on in enumerate(takes) if not on]
        assert [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in rows[out]] == [bounds[r] for r in out], name
        assert (rows["first"][out] == out).all() and not rows["copies"][out].any() and not rows["strand"][out].any(), name
