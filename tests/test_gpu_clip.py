"""GPU tests of adapter clipping (naf_gpu_unnaf_clip, unnaf --adapter).  Expected rows never come from the code under test: they are what
clip_plan.model gives for the records of the oracle's text of the same archive, and the expected texts are cut out of that text.  Every
planned text is swept in the oracle's archive (raw 128 KiB blocks) and in this library's own ennaf at level 1."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import clip_plan as CP
import trim_plan as TP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
CASES = [c.name for c in CP.planned(0)[1]]
TRACE = re.compile(r"\[clip\] adapters (\d+) records (\d+) clipped (\d+) pieces (\d+) sequence bytes decoded (\d+) of (\d+)\n")
# the queries a case is swept with beside those its plants claim
EXTRA = {"seams0": ("o13", "tbl", "four"), "seams1": ("four", "o1"), "seams2": ("o1", "lower", "four1"), "long": ("four", "m13"), "rna": ("rna", "o1"),
         "ones": ("o1", "four1", "m3"), "fastq": ("m32", "m13", "four", "tbl", "o1"), "tail_first": ("four1",), "tail_bounds": ("o1",)}


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

    def want(self, P, qn, min_len=1, bset=None):
        """(rows, total, per_adapter) of the whole archive, computed once per question and left unchanged"""
        key = (qn, min_len, bset)
        if key not in self._want:
            rows, total, per = CP.model(self.records, P.q[qn], min_len, self.case.bounds(bset) if bset else None)
            rows.setflags(write=False)
            self._want[key] = (rows, total, per)
        return self._want[key]

    def fastq(self):
        return self.oracle.unnaf(self.naf, self.oracle.MODE_FASTQ)


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """(plan, name -> (case, {"oracle": Archive, "own": Archive}))"""
    P, cases = CP.planned(SEED)
    out = {}
    for c in cases:
        a = Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type, well_formed=c.fmt == "fastq"), c)
        assert a.records == c.records, c.name
        own, _ = gpu.ennaf(gpu.to_device(c.text), seq_type=c.seq_type, level=1)
        b = Archive(oracle, gpu, own.cpu().numpy().tobytes(), c, a)
        assert b.records == c.records, c.name
        out[c.name] = (c, {"oracle": a, "own": b})
    return P, out


def differ(what, got, want, where):
    if got.tobytes() != want.tobytes():
        k = next((i for i in range(min(len(got), len(want))) if got[i].tobytes() != want[i].tobytes()), min(len(got), len(want)))
        raise AssertionError("%s %s: first difference at row %d of %d / %d: got %s, expected %s" % (what, where, k, len(got), len(want), got[k:k + 2].tolist(), want[k:k + 2].tolist()))


def total_tuple(t):
    return (int(t.reads), int(t.clipped), int(t.kept), int(t.bases), int(t.kept_bases), int(t.removed_bases), int(t.n_short), int(t.n_errors))


def total_of(rows, bounds):
    """the totals of a window of rows; bounds: its (begin, end, flags) rows"""
    kept = rows[rows["flags"] & CP.KEPT != 0]
    return (len(rows), int((rows["flags"] & CP.CLIPPED != 0).sum()), len(kept), sum(b[1] - b[0] for b in bounds), int((kept["end"] - kept["begin"]).sum()),
            sum(b[1] for b in bounds) - int(rows["end"].sum()), int((rows["flags"] & CP.SHORT != 0).sum()), int((rows["flags"] & CP.ERRORS != 0).sum()))


def per_of(rows, n_adapters):
    per = [[0] * 33 for _ in range(n_adapters)]
    for x in rows[rows["flags"] & CP.CLIPPED != 0]:
        per[int(x["adapter"])][int(x["overlap"])] += 1
    return per


def bounds_tensor(gpu, bounds, first=0):
    """trim rows on the device: (begin, end, flags) of records first .."""
    t = np.zeros(len(bounds), dtype=TP.ROW_DTYPE)
    t["record"] = np.arange(first, first + len(bounds)); t["begin"] = [b[0] for b in bounds]; t["end"] = [b[1] for b in bounds]; t["flags"] = [b[2] or TP.KEPT for b in bounds]
    t["ee"] = 12345
    return gpu.to_device(t.tobytes()) if len(bounds) else None


def check(gpu, P, A, qn, min_len=1, bset=None, first=0, count=None):
    q = P.q[qn]
    rows_w, total_w, per_w = A.want(P, qn, min_len, bset)
    last = A.N if count is None else first + count
    bounds = A.case.bounds(bset)[first:last] if bset else None
    if (first, count) != (0, None):
        rows_w = rows_w[first:last]
        total_w, per_w = total_of(rows_w, bounds if bounds is not None else [(0, n, 0) for n in A.lens[first:last]]), per_of(rows_w, len(q.adapters))
    where = "%s query %s min_len %d bounds %s records %d+%s" % (A.case.name, qn, min_len, bset, first, count)
    rows, total, per = gpu.unnaf_clip(A.d_naf, q.adapters, budgets=q.budgets, min_overlap=q.min_overlap, min_len=min_len,
                                      bounds=bounds_tensor(gpu, bounds, first) if bounds is not None else None, first=first, count=count)
    differ("rows", rows, rows_w, where)
    assert total_tuple(total) == total_w, where
    assert per == per_w, where
    return rows


def questions(P, c):
    keys = sorted({(qn, ml, bs) for p in c.plants for qn, bs, ml, _ in p.claims}, key=str)
    return keys + [(qn, 1, None) for qn in EXTRA[c.name] if (qn, 1, None) not in keys]


# ---- 1. the rows of the planned texts under every query -------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_rows_of_the_planned_texts(gpu, planned, name, which):
    P, arcs = planned
    c, arc = arcs[name]
    A = arc[which]
    n = 0
    for qn, min_len, bset in questions(P, c):
        rows = check(gpu, P, A, qn, min_len, bset)
        assert len(rows) == A.N
        n += int((rows["flags"] & CP.CLIPPED != 0).sum())
        for p in c.plants:                                                              # the plants have the rows they were planted to have
            for cq, cb, cm, claim in p.claims:
                if (cq, cm, cb) == (qn, min_len, bset):
                    assert tuple(int(rows[p.record][f]) for f in ("begin", "end", "adapter", "mismatches", "overlap", "flags")) == claim, (p.cell, p.name, p.kind, p.off)
    assert n > 0


def test_the_default_rate_is_one_tenth(gpu, planned):
    P, arcs = planned
    A = arcs["seams1"][1]["own"]
    rows, total, per = gpu.unnaf_clip(A.d_naf, [P.A])
    differ("rows", rows, A.want(P, "m32")[0], "defaults")
    rows, total, per = gpu.unnaf_clip(A.d_naf, [P.A, P.B, P.C, P.A[:16]], rate="0.1", min_overlap=3)
    differ("rows", rows, A.want(P, "four")[0], "rate as text")
    assert total_tuple(total) == A.want(P, "four")[1] and per == A.want(P, "four")[2]


# ---- 2. bounds made by unnaf_trim stay on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_bounds_from_unnaf_trim(gpu, planned, which):
    import torch
    P, arcs = planned
    c, arc = arcs["fastq"]
    A = arc[which]
    quals = TP.quals_of(A.fastq(), A.N)
    assert quals == c.quals
    for limit, min_len, max_ee in ((TP.LIMITS["Q20"], 1, TP.NO_MAX), (TP.NONE, 1, TP.NO_MAX), (TP.LIMITS["Q20"], 30, TP.ee_units("0.05"))):
        trows, _ = TP.model(quals, limit, min_len, max_ee)
        bounds = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in trows]
        buf = torch.zeros(40 * A.N, dtype=torch.uint8, device="cuda")
        view, _ = gpu.unnaf_trim(A.d_naf, limit, min_len, None if max_ee == TP.NO_MAX else max_ee, out=buf)
        assert view.cpu().numpy().tobytes() == trows.tobytes()
        for qn in ("m32", "four"):
            want, total_w, per_w = CP.model(A.records, P.q[qn], min_len, bounds)
            q = P.q[qn]
            rows, total, per = gpu.unnaf_clip(A.d_naf, q.adapters, budgets=q.budgets, min_overlap=q.min_overlap, min_len=min_len, bounds=view)
            differ("rows", rows, want, "trim limit %d min_len %d %s" % (limit, min_len, qn))
            assert total_tuple(total) == total_w and per == per_w
            assert (rows["flags"] & CP.CLIPPED != 0).sum() > 100 and (min_len == 1 or ((rows["flags"] & CP.ERRORS != 0).any() and (rows["flags"] & CP.SHORT != 0).any()))


# ---- 3. first and count ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    P, arcs = planned
    for name, qn, bset in (("seams0", "m32", None), ("seams0", "m32", "end9"), ("seams1", "m32", "errors"), ("seams2", "o1", None)):
        c, arc = arcs[name]
        A = arc[which]
        N = A.N
        plants = [p.record for p in c.plants]
        runs = [(0, 1), (N - 1, 1), (N, 0), (N, None), (5, 0), (N // 2, None), (0, 2), (N - 2, 2), (1, 1), (plants[7], 1), (plants[7] - 1, 3), (plants[50], None), (0, plants[50])]
        empty = [r for r in range(N) if not A.lens[r]]
        runs += [(r, 1) for r in empty[:3]] + [(empty[-1] - 1, 4)]
        for first, count in runs:
            check(gpu, P, A, qn, 1, bset, first, count)


# ---- 4. the piece size does not show --------------------------------------------------------------------------------------------------
CHILD = """
import hashlib, json, sys
from naf_amd import capi
ctx = capi.Context(0)
qs = json.loads(sys.argv[1])
for path in sys.argv[2:]:
    d = ctx.to_device(open(path, "rb").read())
    for adapters, budgets, mo in qs:
        rows, t, per = ctx.unnaf_clip(d, adapters, budgets=budgets, min_overlap=mo)
        print(len(rows), hashlib.sha256(rows.tobytes()).hexdigest(), t.reads, t.clipped, t.kept, t.bases, t.kept_bases, t.removed_bases, t.n_short, t.n_errors, hashlib.sha256(json.dumps(per).encode()).hexdigest())
ctx.close()
"""


@pytest.mark.parametrize("piece", [1, 5000, 300000])
def test_the_result_does_not_depend_on_the_piece_size(planned, piece, tmp_path):
    """NAF_GPU_CLIP_PIECE is read when the library starts: a fresh process per value.  At 1 every read is a piece of its own (the short
    archives), at 5000 and 300000 the pieces end at reads in the middle of tiles."""
    import json
    P, arcs = planned
    env = dict(os.environ, NAF_GPU_CLIP_PIECE=str(piece), NAF_GPU_TRACE="1", PYTHONPATH=ROOT)
    use = [arcs["long"][1]["own"], arcs["rna"][1]["oracle"], arcs["tail_first"][1]["own"]] + ([arcs["seams1"][1]["own"], arcs["seams0"][1]["oracle"]] if piece > 1 else [])
    qns = ("m32", "four")
    for k, A in enumerate(use):
        (tmp_path / ("%d.naf" % k)).write_bytes(A.naf)
    p = subprocess.run([sys.executable, "-c", CHILD, json.dumps([[P.q[qn].adapters, P.q[qn].budgets, P.q[qn].min_overlap] for qn in qns])] + [str(tmp_path / ("%d.naf" % k)) for k in range(len(use))],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().split("\n")
    tr = TRACE.findall(p.stderr.decode())
    assert len(tr) == len(qns) * len(use), p.stderr.decode()
    for k, A in enumerate(use):
        for j, qn in enumerate(qns):
            rows, total, per = A.want(P, qn)
            assert out[len(qns) * k + j].split() == [str(x) for x in (len(rows), hashlib.sha256(rows.tobytes()).hexdigest()) + total + (hashlib.sha256(json.dumps(per).encode()).hexdigest(),)], (k, qn)
            n_ad, R, clipped, pieces, dec, of = (int(x) for x in tr[len(qns) * k + j])
            assert (n_ad, R, clipped, of) == (len(P.q[qn].adapters), A.N, total[1], (sum(A.lens) + 1) // 2)
            assert (pieces == 1) if sum(A.lens) <= piece else (pieces >= 2), (k, piece, pieces)
            assert piece != 1 or pieces > A.N // 2                                    # (reads of one base share a piece with the next)


def test_a_window_at_the_far_end_decodes_only_its_blocks(gpu, planned, monkeypatch, capfd):
    P, arcs = planned
    A = arcs["seams0"][1]["oracle"]
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    check(gpu, P, A, "m32", 1, None, A.N - 6, 6)
    check(gpu, P, A, "m32")
    tr = TRACE.findall(capfd.readouterr().err)
    monkeypatch.delenv("NAF_GPU_TRACE")
    assert len(tr) == 2 and int(tr[0][1]) == 6 and int(tr[0][3]) == 1
    assert 0 < int(tr[0][4]) < int(tr[0][5]) == (sum(A.lens) + 1) // 2 == int(tr[1][4]) and int(tr[1][2]) == A.want(P, "m32")[1][1]


# ---- 5. buffers -----------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, q, min_len, first, count, d_bounds, d_rows, cap, total=True, per=True, adapters=None, n_adapters=None, budgets=True, min_overlap=None):
    from naf_amd import capi
    ads = q.adapters if adapters is None else adapters
    blob = b"".join((a.encode("latin1") if isinstance(a, str) else a) + b"\0" for a in ads)
    na = len(ads) if n_adapters is None else n_adapters
    flat = [v for b in q.budgets for v in b] if budgets is True else budgets
    tab = (C.c_uint8 * max(len(flat), 1))(*flat) if flat is not None else None
    n, tot, pa = C.c_uint64(12345), capi.ClipTotal(), (C.c_uint64 * (33 * 16))()
    o = capi.ClipOpts(q.min_overlap if min_overlap is None else min_overlap, min_len)
    rc = gpu.L.naf_gpu_unnaf_clip(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), blob, len(blob), na, tab, C.byref(o), first, capi.WHOLE if count is None else count,
                                  C.c_void_p(d_bounds.data_ptr()) if d_bounds is not None else None, C.c_void_p(d_rows.data_ptr()) if d_rows is not None else None, cap,
                                  C.byref(n), C.byref(tot) if total else None, pa if per else None)
    return rc, n.value, tot, [[int(pa[33 * k + L]) for L in range(33)] for k in range(min(len(q.adapters), 16))]


def test_totals_only(gpu, planned):
    P, arcs = planned
    for name in ("seams1", "long", "ones"):
        A = arcs[name][1]["own"]
        qn = "o1" if name == "ones" else "m32"
        q = P.q[qn]
        rows, total, per = gpu.unnaf_clip(A.d_naf, q.adapters, budgets=q.budgets, min_overlap=q.min_overlap, out=False)
        assert rows is None and total_tuple(total) == A.want(P, qn)[1] and per == A.want(P, qn)[2]
        rc, n, tot, per = raw(gpu, A.d_naf, q, 1, 0, 2, None, None, 0, total=False, per=False)
        assert rc == 0 and n == 2


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    P, arcs = planned
    arena = fenced.Arena("cuda", salt=0x79, size=8 << 20)
    q = P.q["m32"]
    for name, bset in (("seams1", "errors"), ("long", "late"), ("seams0", None)):
        A = arcs[name][1][which]
        rows_w, total_w, per_w = A.want(P, "m32", 1, bset)
        n = len(rows_w)
        bt = bounds_tensor(gpu, A.case.bounds(bset)) if bset else None
        for phase in (0, 1, 31):
            arena.reset()
            d_bounds = arena.put(bt, (phase * 7 + 1) % 128) if bt is not None else None      # the bounds at a phase of their own
            d_rows = arena.out(40 * n, phase)                                            # exactly enough: 40 bytes a row and nothing outside them
            rc, got, tot, per = raw(gpu, A.d_naf, q, 1, 0, None, d_bounds, d_rows, n, total=phase != 1, per=phase != 31)
            torch.cuda.synchronize()
            assert rc == 0 and got == n
            arena.check()
            assert d_rows.cpu().numpy().tobytes() == rows_w.tobytes(), (name, phase)
            assert phase == 1 or total_tuple(tot) == total_w
            assert phase == 31 or per == per_w
        arena.reset()                                                                   # one row too few: the whole count, nothing written
        d_rows = arena.out(40 * (n - 1), 5)
        before = d_rows.clone()
        rc, got, tot, per = raw(gpu, A.d_naf, q, 1, 0, None, None, d_rows, n - 1)
        torch.cuda.synchronize()
        assert rc == E_CAP and got == n and torch.equal(d_rows, before) and "rows" in gpu.L.naf_gpu_last_error(gpu.h).decode()
        arena.check()
        arena.reset()                                                                   # a window into a table of its own size
        d_rows = arena.out(40 * 7, 31)
        rc, got, tot, per = raw(gpu, A.d_naf, q, 1, 3, 7, None, d_rows, 7)
        torch.cuda.synchronize()
        assert rc == 0 and got == 7 and d_rows.cpu().numpy().tobytes() == A.want(P, "m32")[0][3:10].tobytes()
        arena.check()
    A = arcs["tail_bounds"][1]["oracle"]                                                # the archive in an arena, other bytes around it
    for run, in_phase in ((0, 0), (1, 1), (0, 65)):
        arena.reset()
        before, after = fenced.stream_bait(A.naf, run)
        d_in = arena.put(A.naf, in_phase, before, after)
        d_rows = arena.out(40 * A.N, 9)
        rc, got, tot, per = raw(gpu, d_in, q, 1, 0, None, None, d_rows, A.N)
        torch.cuda.synchronize()
        assert rc == 0 and d_rows.cpu().numpy().tobytes() == A.want(P, "m32")[0].tobytes()
        arena.check()
    A = arcs["long"][1][which]                                                          # the binding's own form with the caller's buffer
    buf = torch.zeros(40 * A.N + 40, dtype=torch.uint8, device="cuda")
    view, tot, per = gpu.unnaf_clip(A.d_naf, q.adapters, out=buf)
    assert view.numel() == 40 * A.N and not bool(buf[40 * A.N:].any()) and view.cpu().numpy().tobytes() == A.want(P, "m32")[0].tobytes()
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_clip(A.d_naf, q.adapters, out=buf[:40 * (A.N - 1)])
    assert e.value.code == E_CAP


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    import torch
    P, arcs = planned
    A = arcs["seams1"][1]["own"]
    N = A.N
    q = P.q["m32"]

    def fails(d_naf=A.d_naf, words=(), min_len=1, first=0, count=None, d_bounds=None, **kw):
        buf = torch.zeros(40 * 64, dtype=torch.uint8, device="cuda")
        rc, n, tot, per = raw(gpu, d_naf, kw.pop("q", q), min_len, first, count, d_bounds, buf, 64, **kw)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == E_ARG and n == 0 and not bool(buf.any()) and total_tuple(tot) == (0,) * 8, (rc, n, msg)
        for w in words:
            assert w in msg, msg

    fails(adapters=[], words=("0 adapters",))
    fails(adapters=["ACGT"] * 17, q=CP.Query(["ACGT"] * 17), words=("17 adapters", "16"))
    fails(adapters=["ACGTXCGT"], words=("adapter 0", "'X'", "position 5"))
    fails(adapters=["AC[GT]A"], words=("'['", "position 3"))
    fails(adapters=["ACGT", "AC-T"], q=CP.Query(["ACGT", "ACGT"]), words=("adapter 1", "'-'", "position 3"))
    fails(adapters=["ACGT" * 8 + "A"], words=("33 letters", "first 32 letters decide the same clip points"))
    fails(adapters=[""], words=("no letters",))
    fails(adapters=["ACGT", "ACGT"], n_adapters=3, q=CP.Query(["ACGT"] * 3), words=("3 patterns announced",))
    fails(min_overlap=0, words=("min_overlap 0",))
    fails(min_overlap=33, words=("min_overlap 33",))
    fails(min_len=0, words=("min_len",))
    fails(budgets=None, words=("h_budget",))
    bad = list(q.budgets[0]); bad[7] = 7
    fails(budgets=bad, words=("adapter 0", "7 mismatches", "7 letters", "every place would be a hit"))
    fails(first=N + 1, words=("record", str(N + 1)))
    fails(first=1, count=N, words=("records", str(N)))
    fails(d_naf=gpu.to_device(golden_bytes("naf", "protein_small.naf")), words=("adapters cannot be clipped", "protein"))
    # bounds rows that are none: found on the device, nothing written
    rows = np.zeros(64, dtype=TP.ROW_DTYPE)
    rows["record"] = np.arange(5, 69); rows["end"] = A.lens[5:69]; rows["flags"] = 1
    for k, field, value, word in ((9, "record", 15, "its record"), (3, "begin", A.lens[8] + 1, "begin > end"), (60, "end", A.lens[65] + 1, "behind the record's last base")):
        t = rows.copy(); t[field][k] = value
        fails(first=5, count=64, d_bounds=gpu.to_device(t.tobytes()), words=("bounds row %d" % k, word))
    t = rows.copy(); t["end"][60] += 1; t["record"][9] = 0                               # two of them: the first is named
    fails(first=5, count=64, d_bounds=gpu.to_device(t.tobytes()), words=("bounds row 9",))
    buf = torch.zeros(40 * 64, dtype=torch.uint8, device="cuda")                          # and the rows as they stand are fine
    rc, n, tot, per = raw(gpu, A.d_naf, q, 1, 5, 64, gpu.to_device(rows.tobytes()), buf, 64)
    assert rc == 0 and n == 64 and buf.cpu().numpy().tobytes() == A.want(P, "m32")[0][5:69].tobytes()
    ok = list(q.budgets[0]); ok[2] = 200                                                 # below min_overlap the table is not looked at
    rc, n, tot, per = raw(gpu, A.d_naf, q, 1, 0, None, None, None, 0, budgets=ok)
    assert rc == 0 and total_tuple(tot) == A.want(P, "m32")[1]


def test_archives_without_records_and_without_quality(gpu, planned, oracle):
    P, arcs = planned
    empty = gpu.to_device(oracle.ennaf(b""))
    rows, total, per = gpu.unnaf_clip(empty, [P.A])
    assert len(rows) == 0 and total_tuple(total) == (0,) * 8 and per == [[0] * 33]
    d = gpu.to_device(golden_bytes("naf", "acgt_10k.naf"))                              # FASTA: no quality section
    h = oracle.parse_naf(golden_bytes("naf", "acgt_10k.naf"))
    assert not h.flags & 1
    recs = oracle.unnaf(golden_bytes("naf", "acgt_10k.naf"), oracle.MODE_SEQUENCES, True).decode("latin1").split("\n")[:-1]
    q = CP.Query(["ACGTAC", "GGNCC"], 3)
    want, total_w, per_w = CP.model(recs, q)
    rows, total, per = gpu.unnaf_clip(d, q.adapters, budgets=q.budgets, min_overlap=3)
    differ("rows", rows, want, "acgt_10k")
    assert total_tuple(total) == total_w and per == per_w and total_w[1] > 0


def test_two_calls_give_identical_bytes(gpu, planned):
    from naf_amd import capi
    P, arcs = planned
    A = arcs["seams0"][1]["own"]
    q = P.q["four"]
    a, ta, pa = gpu.unnaf_clip(A.d_naf, q.adapters)
    gpu.unnaf(arcs["rna"][1]["oracle"].d_naf, capi.OUT_FASTA)                           # an unrelated call on the same context in between
    b, tb, pb = gpu.unnaf_clip(A.d_naf, q.adapters)
    want, total, per = A.want(P, "four")
    assert a.tobytes() == b.tobytes() == want.tobytes() and total_tuple(ta) == total_tuple(tb) == total and pa == pb == per


# ---- 7. the clipped reads -------------------------------------------------------------------------------------------------------------
def text_of(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_select_reads_writes_the_clipped_reads(gpu, planned, which):
    from naf_amd import capi
    P, arcs = planned
    A = arcs["fastq"][1][which]
    text = A.fastq()
    rows = check(gpu, P, A, "m32", 30)
    segs = capi.clip_to_segments(rows)
    assert segs == CP.kept_segments(A.want(P, "m32", 30)[0]) and len(segs) > 500 and sum(e < A.lens[r] for r, b, e in segs) > 100
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
        out += [b">", head, b"\n"] + [seq[i:i + W] + b"\n" for i in range(0, len(seq), W)]
    return b"".join(out)


# ---- 8. the command line --------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_adapter_writes_the_reads_and_the_table(gpu, planned):
    P, arcs = planned
    A = arcs["fastq"][1]["own"]
    text = A.fastq()
    p = unnaf_cli(["--adapter", P.A], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, CP.kept_segments(A.want(P, "m32")[0]), "fastq")
    p = unnaf_cli(["--adapter", P.A, "--adapter", P.B, "--adapter", P.C, "--adapter", P.A[:16], "--min-length", "30", "--fasta", "--line-length", "60"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, CP.kept_segments(A.want(P, "four", 30)[0]), "fasta", 60)
    p = unnaf_cli(["--adapter", P.A.lower(), "--clip-table"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == CP.table(A.want(P, "m32")[0], A.ids, A.lens)
    p = unnaf_cli(["--adapter", P.A, "--clip-table", "--min-overlap", "1", "--records", "3-700"], A.naf)
    assert p.returncode == 0 and p.stdout == CP.table(A.want(P, "o1")[0][2:700], A.ids, A.lens)
    p = unnaf_cli(["--adapter", P.A[:13], "--adapter-errors", "0.1", "--seq", "--region", A.ids[3]], A.naf)
    assert p.returncode == 0 and p.stdout == TP.expected_text(text, A.N, CP.kept_segments(A.want(P, "m13")[0][3:4]), "seq")
    # quality trimming first, on the device: the clip call's bounds
    quals = TP.quals_of(text, A.N)
    trows, _ = TP.model(quals, TP.LIMITS["Q20"], 30, TP.ee_units("0.05"))
    bounds = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in trows]
    want = CP.model(A.records, P.q["m32"], 30, bounds)[0]
    p = unnaf_cli(["--trim", "20", "--adapter", P.A, "--min-length", "30", "--max-ee", "0.05"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, CP.kept_segments(want), "fastq")
    p = unnaf_cli(["--adapter", P.A, "--trim", "20", "--min-length", "30", "--max-ee", "0.05", "--clip-table"], A.naf)
    assert p.returncode == 0 and p.stdout == CP.table(want, A.ids, A.lens)
    assert set(line.split(b"\t")[-1] for line in p.stdout.split(b"\n")[1:-1]) == {b"kept", b"short", b"errors", b"short,errors"}
    F = arcs["seams1"][1]["own"]                                                        # a FASTA archive: FASTA reads by default
    segs = CP.kept_segments(F.want(P, "m32")[0])
    p = unnaf_cli(["--adapter", P.A, "--line-length", "0"], F.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == fasta_reads(F, segs, 0)
    p = unnaf_cli(["--adapter", P.A, "--trim", "20"], F.naf)
    assert p.returncode == 1 and b"no quality" in p.stderr and p.stdout == b""
    for args in (["--adapter", P.A, "--region", "nosuch"], ["--adapter", P.A, "--records", "1-99999"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args


# ---- 9. against the search with mismatches (extra, not the yardstick) -----------------------------------------------------------------
def test_full_overlaps_are_the_first_near_hits(gpu, planned):
    P, arcs = planned
    for name in ("seams0", "fastq"):
        A = arcs[name][1]["own"]
        rows = A.want(P, "m32")[0]
        hits, _ = gpu.unnaf_locate_near(A.d_naf, [P.A], 3, strands=1)
        first = {}
        for h in hits:
            first.setdefault(int(h["record"]), (int(h["begin"]), int(h["mismatches"])))
        full = rows[(rows["flags"] & CP.CLIPPED != 0) & (rows["overlap"] == 32)]
        assert len(full) > 30
        for x in full:
            assert first[int(x["record"])] == (int(x["end"]), int(x["mismatches"]))
