"""GPU tests of k-mer screening (naf_gpu_unnaf_screen, unnaf --screen).  Expected rows never come from the code under test: they are
what screen_plan.model gives for the records of the oracle's text of the same archives, and the expected texts are cut out of that text.
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
import screen_plan as SP
import trim_plan as TP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
CASES = [c.name for c in SP.planned(0) if not c.name.startswith("end")]
TRACE = re.compile(r"\[screen\] k (\d+) ref records (\d+) ref kmers (\d+) of (\d+) slots (\d+) filter bits (\d+) reads (\d+) considered (\d+) matched (\d+) filtered (\d+) probed (\d+) "
                   r"sequence bytes decoded (\d+) of (\d+)\n")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


class Archive:
    """a planned text or a reference as an archive on the device, with the records the oracle reads out of it"""

    def __init__(self, oracle, gpu, naf, shared=None):
        self.naf = naf
        self.N = oracle.parse_naf(naf).n_sequences
        if shared is None:
            self.records = oracle.unnaf(naf, oracle.MODE_SEQUENCES, True).decode("latin1").split("\n")[:-1] if self.N else []
            self.stream = SP.Stream(self.records)
        else:
            self.records, self.stream = shared.records, shared.stream
        self.lens = [len(r) for r in self.records]
        self.d_naf = gpu.to_device(naf)
        self.oracle = oracle


def archives(oracle, gpu, text, seq_type, fmt, records):
    a = Archive(oracle, gpu, oracle.ennaf(text, seq_type, well_formed=fmt == "fastq"))
    assert [SP.canon(r) for r in a.records] == [SP.canon(r) for r in records]
    if not text:                                                                        # (no text: no archive of this build's own)
        return {"oracle": a, "own": a}
    own, _ = gpu.ennaf(gpu.to_device(text), seq_type=seq_type, level=1)
    b = Archive(oracle, gpu, own.cpu().numpy().tobytes(), a)
    assert oracle.unnaf(b.naf, oracle.MODE_SEQUENCES, True).decode("latin1").split("\n")[:-1] == a.records if a.N else b.N == 0
    return {"oracle": a, "own": b}


class Planned:
    """the cases of one seed: name -> (case, reads archives, reference archives), made when first asked for; the model's answers are kept"""

    def __init__(self, oracle, gpu, seed):
        self.oracle, self.gpu, self.cases = oracle, gpu, {c.name: c for c in SP.planned(seed)}
        self.made, self.refs, self.wanted, self.bsets = {}, {}, {}, {}

    def __getitem__(self, name):
        if name not in self.made:
            c = self.cases[name]
            if id(c.ref) not in self.refs:
                self.refs[id(c.ref)] = archives(self.oracle, self.gpu, c.ref.text, c.ref.seq_type, c.ref.fmt, c.ref.records)
            self.made[name] = (c, archives(self.oracle, self.gpu, c.text, c.seq_type, c.fmt, c.records), self.refs[id(c.ref)])
        return self.made[name]

    def bounds(self, name, bset):
        if (name, bset) not in self.bsets:
            self.bsets[(name, bset)] = self.cases[name].bounds(bset)
        return self.bsets[(name, bset)]

    def want(self, name, K, **kw):
        """(rows, total) of the whole text, computed once per question and left unchanged"""
        key = (name, K, tuple(sorted((k, v if not isinstance(v, list) else id(v)) for k, v in kw.items())))
        if key not in self.wanted:
            c, arc, ref = self[name]
            rows, total = SP.model(arc["oracle"].stream, ref["oracle"].stream, K, **kw)
            rows.setflags(write=False)
            self.wanted[key] = (rows, total)
        return self.wanted[key]


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    return Planned(oracle, gpu, SEED)


def differ(what, got, want, where):
    if got.tobytes() != want.tobytes():
        k = next((i for i in range(min(len(got), len(want))) if got[i].tobytes() != want[i].tobytes()), min(len(got), len(want)))
        raise AssertionError("%s %s: first difference at row %d of %d / %d: got %s, expected %s" % (what, where, k, len(got), len(want), got[k:k + 2].tolist(), want[k:k + 2].tolist()))


def total_tuple(t):
    return (int(t.reads), int(t.considered), int(t.matched), int(t.kept), int(t.bases), int(t.kept_bases), int(t.kmers), int(t.hit_kmers), int(t.ref_records), int(t.ref_bases),
            int(t.ref_positions), int(t.ref_kmers))


def check(gpu, P, name, K, which="oracle", ref_which=None, bset=None, kind="trim", first=0, count=None, **kw):
    c, arc, ref = P[name]
    A, R = arc[which], ref[ref_which or which]
    bounds = P.bounds(name, bset) if bset else None
    if (first, count) == (0, None):
        rows_w, total_w = P.want(name, K, bounds=bounds, **kw) if bounds else P.want(name, K, **kw)
    else:
        rows_w, total_w = SP.model(A.stream, R.stream, K, bounds=bounds, first=first, count=count, **kw)
    last = A.N if count is None else first + count
    d_bounds = gpu.to_device(SP.bounds_rows(bounds[first:last], kind, first)) if bset and last > first else None
    where = "%s k %d %s bounds %s %s records %d+%s %s" % (name, K, which, bset, kind, first, count, kw)
    rows, total = gpu.unnaf_screen(A.d_naf, R.d_naf, k=K, bounds=d_bounds, bounds_kind=kind, first=first, count=count, **kw)
    differ("rows", rows, rows_w, where)
    assert total_tuple(total) == total_w, (where, total_tuple(total), total_w)
    return rows


# ---- 1. the rows of the planned texts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_rows_of_the_planned_texts(gpu, planned, name, which):
    c = planned[name][0]
    for K in c.ks:
        for fwd in (False, True):
            rows = check(gpu, planned, name, K, which, forward_only=fwd)
            assert len(rows) == len(c.records) and SP.claims_hold(c, K, rows, fwd), (name, K, fwd)
        for k, bs in enumerate(sorted(c.bsets)):
            for kind in ("trim", "clip", "dedup"):
                rows = check(gpu, planned, name, K, which, bset=bs, kind=kind, forward_only=bool(k % 2))
            assert SP.claims_hold(c, K, rows, bool(k % 2), bs), (name, K, bs)
        # the other archive of the reference answers the same
        check(gpu, planned, name, K, which, ref_which="own" if which == "oracle" else "oracle")


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_the_streams_end_at_every_offset(gpu, planned, which):
    """one tiny text per offset of a plant's first base from the stream's end"""
    n = 0
    for name, c in planned.cases.items():
        if name.startswith("end"):
            rows = check(gpu, planned, name, c.ks[0], which)
            assert SP.claims_hold(c, c.ks[0], rows), name
            n += 1
    assert n == 3 * sum(K + 1 for K in SP.KS)


@pytest.mark.parametrize("seed", [1, 2])
def test_other_seeds(oracle, gpu, seed):
    P = Planned(oracle, gpu, seed)
    for name in ("place1", "place17", "place31", "end15-7j0", "end31-32j5", "end2-1j1", "dna_rna", "chain"):
        c = P[name][0]
        for K in c.ks:
            rows = check(gpu, P, name, K, "own" if (seed + K) % 2 else "oracle", forward_only=bool(seed % 2))
            assert SP.claims_hold(c, K, rows, bool(seed % 2)), (name, seed)
            for bs in c.bsets:
                check(gpu, P, name, K, "oracle", bset=bs, kind="clip")


def test_the_verdict_cells(gpu, planned):
    c = planned["place27"][0]
    r = c.verdict_read
    for min_hits in (5, 6, 7):
        for keep in (False, True):
            rows = check(gpu, planned, "place27", 27, "own", min_hits=min_hits, keep_matched=keep)
            assert int(rows[r]["hits"]) == 6 and bool(int(rows[r]["flags"]) & SP.MATCHED) == (min_hits <= 6) and bool(int(rows[r]["flags"]) & SP.KEPT) == ((min_hits <= 6) == keep)
    check(gpu, planned, "ones", 1, "oracle", keep_matched=True, forward_only=True)
    check(gpu, planned, "chain", 27, "own", min_hits=124, keep_matched=True)              # a whole read of 150 bases has 124 k-mers


# ---- 2. the levers: the same tables whatever the hash is cut to and however large the prefilter is ---------------------------------------
CHILD = """
import hashlib, sys
from naf_amd import capi
ctx = capi.Context(0)
args = sys.argv[1:]
for k in range(0, len(args), 4):
    d, r = ctx.to_device(open(args[k], "rb").read()), ctx.to_device(open(args[k + 1], "rb").read())
    rows, t = ctx.unnaf_screen(d, r, k=int(args[k + 2]), forward_only=args[k + 3] == "1")
    print(len(rows), hashlib.sha256(rows.tobytes()).hexdigest(), t.reads, t.considered, t.matched, t.kept, t.bases, t.kept_bases, t.kmers, t.hit_kmers, t.ref_records, t.ref_bases, t.ref_positions, t.ref_kmers)
ctx.close()
"""


def run_child(planned, jobs, env, tmp_path):
    """jobs: (case name, which, K, forward_only); the child's lines and its trace lines, held to the model"""
    args = []
    for k, (name, which, K, fwd) in enumerate(jobs):
        c, arc, ref = planned[name]
        (tmp_path / ("%d.naf" % k)).write_bytes(arc[which].naf); (tmp_path / ("%d.ref" % k)).write_bytes(ref[which].naf)
        args += [str(tmp_path / ("%d.naf" % k)), str(tmp_path / ("%d.ref" % k)), str(K), "1" if fwd else "0"]
    p = subprocess.run([sys.executable, "-c", CHILD] + args, env=dict(os.environ, NAF_GPU_TRACE="1", PYTHONPATH=ROOT, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    out, tr = p.stdout.decode().split("\n"), TRACE.findall(p.stderr.decode())
    assert len(tr) == len(jobs), p.stderr.decode()
    for k, (name, which, K, fwd) in enumerate(jobs):
        rows, total = planned.want(name, K, forward_only=fwd)
        assert out[k].split() == [str(x) for x in (len(rows), hashlib.sha256(rows.tobytes()).hexdigest()) + total], (name, K, fwd, env)
        t = [int(x) for x in tr[k]]
        assert (t[0], t[1], t[2], t[3], t[6], t[7], t[8]) == (K, total[8], total[11], total[10], total[0], total[1], total[2]), (name, env, t)
        assert t[9] + t[10] == total[6] and t[10] >= total[7] and t[4] >= max(64, 2 * total[9]) and t[4] & (t[4] - 1) == 0, (name, env, t)      # filtered + probed: the valid positions; every hit was probed
    return [[int(x) for x in t] for t in tr]


@pytest.mark.parametrize("bits", [64, 6, 2, 0])
def test_the_result_does_not_depend_on_the_hash_bits(planned, bits, tmp_path):
    """A fresh process per value of NAF_GPU_SCREEN_HASH_BITS, so that the lever is what the library finds when it starts, as a user sets it
    (the binding would also hand a changed os.environ to a living context).  At 0 bits every key shares one chain and
    insertion is quadratic: the small references only."""
    jobs = [("dna_none", "own", 15, False), ("dna_empty", "oracle", 27, True)]
    small = ("dna_rna", "oracle", 15, False), ("rna_dna", "own", 31, True), ("dna_fastq", "own", 17, False)
    if bits:
        jobs += list(small) + [("place15", "own", 15, False), ("place31", "oracle", 31, True), ("end27-5j1", "own", 27, False), ("chain", "own", 27, False)]
    else:
        jobs += [("chain", "oracle", 27, False), ("chain", "own", 27, True)]              # (a reference of 1800 bases)
    run_child(planned, jobs, {"NAF_GPU_SCREEN_HASH_BITS": str(bits)}, tmp_path)


@pytest.mark.parametrize("fbits", [None, 0, 64, 4096, 1 << 19])
def test_the_result_does_not_depend_on_the_prefilter(planned, fbits, tmp_path):
    jobs = [("place27", "own", 27, False), ("place1", "oracle", 1, False), ("place16", "own", 16, True), ("ones", "oracle", 15, False), ("chain", "own", 27, False), ("dna_empty", "own", 15, False)]
    tr = run_child(planned, jobs, {} if fbits is None else {"NAF_GPU_SCREEN_FILTER_BITS": str(fbits)}, tmp_path)
    for (name, which, K, fwd), t in zip(jobs, tr):
        total = planned.want(name, K, forward_only=fwd)[1]
        assert t[5] == (1 << 18 if fbits is None else fbits)
        if fbits == 0:
            assert t[9] == 0 and t[10] == total[6], (name, t)                            # no prefilter: every valid position probes the table
        elif name in ("place27", "place16", "chain") and fbits != 64:
            assert t[9] > 0 and t[10] < total[6], (name, t)                              # the clean background never reaches the table
        if name == "dna_empty" and fbits:
            assert t[9] == total[6] and t[10] == 0                                       # an empty set: no bit is set
    if fbits is None:
        assert tr[0][9] > 0.8 * planned.want("place27", 27, forward_only=False)[1][6]


def test_a_large_reference_goes_without_the_prefilter_by_default(planned, tmp_path):
    """with no lever set a set of more than 2^17 keys is swept without the bitmap (insert with it, mark without it and without LDS); the
    lever's value is obeyed whatever the set"""
    jobs = [("big_ref", "own", 27, False), ("big_ref", "oracle", 15, True)]
    for env, bits in (({}, 0), ({"NAF_GPU_SCREEN_FILTER_BITS": str(1 << 18)}, 1 << 18)):
        tr = run_child(planned, jobs, env, tmp_path)
        for (name, which, K, fwd), t in zip(jobs, tr):
            total = planned.want(name, K, forward_only=fwd)[1]
            assert total[11] > 1 << 17 and total[7] > 0 and t[5] == bits, (env, t)
            assert (t[9] == 0 and t[10] == total[6]) if not bits else (0 < t[9] < total[6]), (env, t)


def test_levers_with_values_they_do_not_have(planned, tmp_path):
    c, arc, ref = planned["dna_none"]
    (tmp_path / "a.naf").write_bytes(arc["own"].naf); (tmp_path / "r.naf").write_bytes(ref["own"].naf)
    for env, word in (({"NAF_GPU_SCREEN_HASH_BITS": "65"}, "NAF_GPU_SCREEN_HASH_BITS 65 (0 to 64)"), ({"NAF_GPU_SCREEN_FILTER_BITS": "100"}, "NAF_GPU_SCREEN_FILTER_BITS 100 (0, or a power of two"),
                      ({"NAF_GPU_SCREEN_FILTER_BITS": "32"}, "NAF_GPU_SCREEN_FILTER_BITS 32"), ({"NAF_GPU_SCREEN_FILTER_BITS": str(1 << 20)}, "NAF_GPU_SCREEN_FILTER_BITS 1048576")):
        p = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "a.naf"), str(tmp_path / "r.naf"), "15", "0"], env=dict(os.environ, PYTHONPATH=ROOT, **env), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert p.returncode != 0 and word in p.stderr.decode() and "error -8" in p.stderr.decode(), p.stderr.decode()


# ---- 3. pieces, first and count ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [1, 5000, 300000])
def test_the_result_does_not_depend_on_the_piece_size(planned, piece, tmp_path):
    """NAF_GPU_SCREEN_PIECE cuts the reference's sweep and the reads' alike; a piece of one base is a piece per record"""
    jobs = [("dna_fastq", "own", 17, False), ("chain", "oracle", 27, True), ("end31-1j5", "own", 31, False)] + ([("place31", "own", 31, False)] if piece > 1 else [("ones", "own", 1, False)])
    run_child(planned, jobs, {"NAF_GPU_SCREEN_PIECE": str(piece)}, tmp_path)


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    for name, K, bset in (("dna_fastq", 17, None), ("place15", 15, "win"), ("chain", 27, None), ("ones", 1, None)):
        c, arc, ref = planned[name]
        N = arc[which].N
        plants = [p.rec for p in c.plants] or [N // 3, N // 2]
        runs = [(0, 1), (N - 1, 1), (N, 0), (N, None), (5, 0), (N // 2, None), (0, 2), (N - 2, 2), (1, 1), (plants[3 % len(plants)], 1), (plants[-1] - 1, 3), (plants[len(plants) // 2], None),
                (0, plants[len(plants) // 2])]
        if name == "place15":                                                            # (a long text: the runs that cut it at a plant)
            runs = runs[-4:]
        for k, (first, count) in enumerate(runs):
            check(gpu, planned, name, K, which, bset=bset, kind=("trim", "clip", "dedup")[k % 3], first=first, count=count, forward_only=bool(k % 2))


def test_a_window_at_the_far_end_decodes_only_its_blocks(gpu, planned, monkeypatch, capfd):
    A = planned["place31"][1]["oracle"]
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    check(gpu, planned, "place31", 31, first=A.N - 6, count=6)
    check(gpu, planned, "place31", 31)
    tr = TRACE.findall(capfd.readouterr().err)
    monkeypatch.delenv("NAF_GPU_TRACE")
    assert len(tr) == 2 and int(tr[0][6]) == 6
    assert 0 < int(tr[0][11]) < int(tr[0][12]) == (sum(A.lens) + 1) // 2 == int(tr[1][11])


# ---- 4. bounds that never leave the device, and the chain to dedup -----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_bounds_from_trim_clip_and_dedup_and_the_chain_to_dedup(gpu, planned, which):
    import torch
    c, arc, ref = planned["chain"]
    A, R = arc[which], ref[which]
    quals = TP.quals_of(A.oracle.unnaf(A.naf, A.oracle.MODE_FASTQ), A.N)
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
        drows, _, _ = DP.model(A.records, True, cb)
        db = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in drows]
        dbuf = torch.zeros(48 * A.N, dtype=torch.uint8, device="cuda")
        dview, _, _ = gpu.unnaf_dedup(A.d_naf, True, bounds=cview, bounds_kind="clip", out=dbuf)
        assert dview.cpu().numpy().tobytes() == drows.tobytes()
        for keep in (False, True):
            for view, bounds, kind in ((tview, tb, "trim"), (cview, cb, "clip"), (dview, db, "dedup")):
                want, total_w = SP.model(A.stream, R.stream, 27, keep_matched=keep, bounds=bounds)
                sbuf = torch.zeros(40 * A.N, dtype=torch.uint8, device="cuda")
                sview, total = gpu.unnaf_screen(A.d_naf, R.d_naf, k=27, keep_matched=keep, bounds=view, bounds_kind=kind, out=sbuf)
                rows = np.frombuffer(sview.cpu().numpy().tobytes(), dtype=SP.ROW_DTYPE)
                differ("rows", rows, want, "limit %d min_len %d keep %s %s" % (limit, min_len, keep, kind))
                assert total_tuple(total) == total_w and 0 < total_w[2] < total_w[1] and (kind == "trim" or (rows["flags"] & SP.CLIPPED != 0).sum() > 50)
                assert min_len == 1 or ((rows["flags"] & SP.ERRORS != 0).any() and (rows["flags"] & SP.SHORT != 0).any() and total_w[1] < A.N)
                if kind == "dedup":
                    assert (rows["flags"] == SP.DUPLICATE).any() or (rows["flags"] == SP.DUPLICATE | SP.CLIPPED).any()      # a duplicate took no part: its flags as they came
                    continue
                # trim, clip, screen, dedup: the screen rows are dedup's bounds as trim rows, and never left the device
                sb = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in want]
                for both in (False, True):
                    want_d, total_d, levels_d = DP.model(A.records, both, sb)
                    got_d, t, lev = gpu.unnaf_dedup(A.d_naf, both, bounds=sview, bounds_kind="trim")
                    assert got_d.tobytes() == want_d.tobytes() and lev == levels_d and int(t.considered) == total_d[1] == total_w[3]
                    assert (got_d["flags"] & SP.MATCHED != 0).sum() == (0 if keep else total_w[2])      # a dropped read's flags as they came


# ---- 5. buffers -----------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, d_ref, K, flags, kind, min_hits, first, count, d_bounds, d_rows, cap, total=True):
    from naf_amd import capi
    n, tot = C.c_uint64(12345), capi.ScreenTotal(*([77] * 12))
    o = capi.ScreenOpts(K, flags, kind, min_hits)
    rc = gpu.L.naf_gpu_unnaf_screen(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), C.c_void_p(d_ref.data_ptr()), d_ref.numel(), C.byref(o), first, capi.WHOLE if count is None else count,
                                    C.c_void_p(d_bounds.data_ptr()) if d_bounds is not None else None, C.c_void_p(d_rows.data_ptr()) if d_rows is not None else None, cap,
                                    C.byref(n), C.byref(tot) if total else None)
    return rc, n.value, tot


def test_totals_only(gpu, planned):
    for name, K in (("place16", 16), ("ones", 1), ("chain", 27)):
        c, arc, ref = planned[name]
        rows, total = gpu.unnaf_screen(arc["own"].d_naf, ref["own"].d_naf, k=K, out=False)
        assert rows is None and total_tuple(total) == planned.want(name, K)[1]
        rc, n, tot = raw(gpu, arc["own"].d_naf, ref["own"].d_naf, K, 0, 0, 1, 0, 2, None, None, 0, total=False)
        assert rc == 0 and n == 2


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x5C, size=8 << 20)
    for name, K, bset, kind in (("place15", 15, "win", "clip"), ("place2", 2, "win", "dedup"), ("chain", 27, None, "trim")):
        c, arc, ref = planned[name]
        A, R = arc[which], ref[which]
        bounds = planned.bounds(name, bset) if bset else None
        rows_w, total_w = planned.want(name, K, bounds=bounds) if bounds else planned.want(name, K)
        n = len(rows_w)
        bt = SP.bounds_rows(bounds, kind) if bset else None
        for phase in (0, 1, 31):
            arena.reset()
            d_bounds = arena.put(bt, (phase * 7 + 1) % 128) if bt is not None else None  # the bounds at a phase of their own
            d_rows = arena.out(40 * n, phase)                                            # exactly enough: 40 bytes a row and nothing outside them
            rc, got, tot = raw(gpu, A.d_naf, R.d_naf, K, 0, ("trim", "clip", "dedup").index(kind), 1, 0, None, d_bounds, d_rows, n, total=phase != 1)
            torch.cuda.synchronize()
            assert rc == 0 and got == n
            arena.check()
            assert d_rows.cpu().numpy().tobytes() == rows_w.tobytes(), (name, phase)
            assert phase == 1 or total_tuple(tot) == total_w
        arena.reset()                                                                   # one row too few: the whole count, nothing written
        d_rows = arena.out(40 * (n - 1), 5)
        before = d_rows.clone()
        rc, got, tot = raw(gpu, A.d_naf, R.d_naf, K, 0, 0, 1, 0, None, None, d_rows, n - 1)
        torch.cuda.synchronize()
        assert rc == E_CAP and got == n and torch.equal(d_rows, before) and "rows" in gpu.L.naf_gpu_last_error(gpu.h).decode() and total_tuple(tot) == (0,) * 12
        arena.check()
        arena.reset()                                                                   # a window into a table of its own size
        d_rows = arena.out(40 * 7, 31)
        rc, got, tot = raw(gpu, A.d_naf, R.d_naf, K, 0, 0, 1, 3, 7, None, d_rows, 7)
        torch.cuda.synchronize()
        assert rc == 0 and got == 7 and d_rows.cpu().numpy().tobytes() == SP.model(A.stream, R.stream, K, first=3, count=7)[0].tobytes()
        arena.check()
    c, arc, ref = planned["end17-4j0"]                                                    # both archives in an arena, other bytes around them
    A, R = arc["oracle"], ref[which]
    for run, in_phase in ((0, 0), (1, 1), (0, 65)):
        arena.reset()
        before, after = fenced.stream_bait(A.naf, run)
        d_in = arena.put(A.naf, in_phase, before, after)
        before, after = fenced.stream_bait(R.naf, run)
        d_ref = arena.put(R.naf, (in_phase + 3) % 128, before, after)
        d_rows = arena.out(40 * A.N, 9)
        rc, got, tot = raw(gpu, d_in, d_ref, 17, 0, 0, 1, 0, None, None, d_rows, A.N)
        torch.cuda.synchronize()
        assert rc == 0 and d_rows.cpu().numpy().tobytes() == planned.want("end17-4j0", 17)[0].tobytes()
        arena.check()
    c, arc, ref = planned["place16"]                                                    # the binding's own form with the caller's buffer
    A, R = arc[which], ref[which]
    buf = torch.zeros(40 * A.N + 40, dtype=torch.uint8, device="cuda")
    view, tot = gpu.unnaf_screen(A.d_naf, R.d_naf, k=16, out=buf)
    assert view.numel() == 40 * A.N and not bool(buf[40 * A.N:].any()) and view.cpu().numpy().tobytes() == planned.want("place16", 16)[0].tobytes()
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_screen(A.d_naf, R.d_naf, k=16, out=buf[:40 * (A.N - 1)])
    assert e.value.code == E_CAP


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    import torch
    c, arc, ref = planned["place15"]
    A, R = arc["own"], ref["own"]
    N = A.N
    protein = gpu.to_device(golden_bytes("naf", "protein_small.naf"))

    def fails(d_naf=A.d_naf, d_ref=R.d_naf, words=(), K=15, flags=0, kind=0, min_hits=1, first=0, count=None, d_bounds=None):
        buf = torch.zeros(40 * 64, dtype=torch.uint8, device="cuda")
        rc, n, tot = raw(gpu, d_naf, d_ref, K, flags, kind, min_hits, first, count, d_bounds, buf, 64)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == E_ARG and n == 0 and not bool(buf.any()) and total_tuple(tot) == (0,) * 12, (rc, n, msg)
        for w in words:
            assert w in msg, msg

    fails(K=0, words=("k 0", "1 to 31"))
    fails(K=32, words=("k 32", "1 to 31"))
    fails(min_hits=0, words=("min_hits 0",))
    fails(flags=4, words=("flags 4",))
    fails(flags=1 | 8, words=("flags 9",))
    fails(kind=3, words=("bounds_kind 3",))
    fails(first=N + 1, words=("record", str(N + 1)))
    fails(first=1, count=N, words=("records", str(N)))
    fails(d_naf=protein, words=("screen: reads cannot be screened in protein sequences",))
    fails(d_ref=protein, count=3, words=("screen reference: reads cannot be screened in protein sequences",))
    from test_gpu_orfs import no_sequence_archive
    no_seq = gpu.to_device(no_sequence_archive(oracle))                                  # two records, no sequence section
    fails(d_naf=no_seq, words=("screen: the archive stores no sequence",))
    fails(d_naf=no_seq, count=1, words=("screen: the archive stores no sequence",))
    fails(d_ref=no_seq, words=("screen reference: the archive stores no sequence",))
    fails(d_ref=no_seq, count=3, words=("screen reference: the archive stores no sequence",))
    # bounds rows that are none: found on the device, nothing written
    for kind, dt in (("trim", TP.ROW_DTYPE), ("clip", CP.ROW_DTYPE), ("dedup", DP.ROW_DTYPE)):
        good = [(0, A.lens[r], 1) for r in range(5, 69)]
        code = ("trim", "clip", "dedup").index(kind)
        for k, field, value, word in ((9, "record", 15, "its record"), (3, "begin", A.lens[8] + 1, "begin > end"), (60, "end", A.lens[65] + 1, "behind the record's last base")):
            t = np.frombuffer(SP.bounds_rows(good, kind, 5), dtype=dt).copy(); t[field][k] = value
            fails(first=5, count=64, kind=code, d_bounds=gpu.to_device(t.tobytes()), words=("bounds row %d" % k, word))
        t = np.frombuffer(SP.bounds_rows(good, kind, 5), dtype=dt).copy(); t["end"][60] += 1; t["record"][9] = 0
        fails(first=5, count=64, kind=code, d_bounds=gpu.to_device(t.tobytes()), words=("bounds row 9",))      # two of them: the first is named
        buf = torch.zeros(40 * 64, dtype=torch.uint8, device="cuda")                      # and the rows as they stand are fine
        rc, n, tot = raw(gpu, A.d_naf, R.d_naf, 15, 0, code, 1, 5, 64, gpu.to_device(SP.bounds_rows(good, kind, 5)), buf, 64)
        assert rc == 0 and n == 64 and buf.cpu().numpy().tobytes() == SP.model(A.stream, R.stream, 15, first=5, count=64)[0].tobytes()
    # after an error return the same table
    check(gpu, planned, "place15", 15, "own")


def test_archives_without_records(gpu, planned, oracle):
    c, arc, ref = planned["dna_rna"]
    empty = gpu.to_device(oracle.ennaf(b""))
    rows, total = gpu.unnaf_screen(empty, ref["own"].d_naf, k=15)                       # no reads: no rows, and the reference as it is
    want = planned.want("dna_rna", 15)[1]
    assert len(rows) == 0 and total_tuple(total) == (0,) * 8 + want[8:]
    rows, total = gpu.unnaf_screen(arc["own"].d_naf, empty, k=15)                       # no reference: nothing matches
    assert total_tuple(total) == SP.model(arc["own"].stream, SP.Stream([]), 15)[1] and int(total.matched) == 0 and int(total.kept) == arc["own"].N
    d = gpu.to_device(golden_bytes("naf", "acgt_10k.naf"))                              # an archive screened against itself: every read matches
    recs = oracle.unnaf(golden_bytes("naf", "acgt_10k.naf"), oracle.MODE_SEQUENCES, True).decode("latin1").split("\n")[:-1]
    s = SP.Stream(recs)
    for K in (1, 12, 31):
        want, total_w = SP.model(s, s, K)
        rows, total = gpu.unnaf_screen(d, d, k=K)
        differ("rows", rows, want, "acgt_10k k %d" % K)
        assert total_tuple(total) == total_w and total_w[7] == total_w[6] > 0


def test_the_same_table_on_a_fresh_context_and_after_release_scratch(gpu, planned):
    from naf_amd import capi
    c, arc, ref = planned["place17"]
    A, R = arc["own"], ref["own"]
    want, total = planned.want("place17", 17)
    a, ta = gpu.unnaf_screen(A.d_naf, R.d_naf, k=17)
    gpu.unnaf(planned["dna_rna"][2]["oracle"].d_naf, capi.OUT_FASTA)                     # an unrelated call on the same context in between
    with pytest.raises(capi.NafGpuError):
        gpu.unnaf_screen(A.d_naf, R.d_naf, k=99)                                          # and an error return
    b, tb = gpu.unnaf_screen(A.d_naf, R.d_naf, k=17)
    assert a.tobytes() == b.tobytes() == want.tobytes() and total_tuple(ta) == total_tuple(tb) == total
    assert gpu.L.naf_gpu_release_scratch(gpu.h) == 0
    c2, tc = gpu.unnaf_screen(A.d_naf, R.d_naf, k=17)                                    # directly after the scratch was given back
    assert c2.tobytes() == want.tobytes() and total_tuple(tc) == total
    fresh = capi.Context(0)
    try:
        d, td = fresh.unnaf_screen(fresh.to_device(A.naf), fresh.to_device(R.naf), k=17)
        assert d.tobytes() == want.tobytes() and total_tuple(td) == total
    finally:
        fresh.close()


# ---- 7. the kept reads ----------------------------------------------------------------------------------------------------------------
def text_of(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_select_reads_writes_the_kept_reads(gpu, planned, which):
    from naf_amd import capi
    c, arc, ref = planned["chain"]
    A = arc[which]
    text = A.oracle.unnaf(A.naf, A.oracle.MODE_FASTQ)
    for keep in (False, True):
        rows = check(gpu, planned, "chain", 27, which, keep_matched=keep)
        segs = capi.screen_to_segments(rows)
        assert segs == SP.kept_segments(planned.want("chain", 27, keep_matched=keep)[0]) and 20 < len(segs) < A.N
        for fmt, out_type, L in (("fastq", capi.OUT_FASTQ, -1), ("fasta", capi.OUT_FASTA, 0), ("fasta", capi.OUT_FASTA, 1), ("fasta", capi.OUT_FASTA, 60),
                                 ("sequences", capi.OUT_SEQUENCES, -1), ("seq", capi.OUT_SEQ, -1)):
            want = TP.expected_text(text, A.N, segs, fmt, max(L, 0))
            got = text_of(gpu.unnaf_select_reads(A.d_naf, segs, out_type, line_length=L))
            assert got == want, (fmt, L, len(got), len(want))


# ---- 8. the command line --------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_screen_writes_the_reads_and_the_table(gpu, planned, tmp_path):
    c, arc, ref = planned["chain"]
    A, R = arc["own"], ref["own"]
    text = A.oracle.unnaf(A.naf, A.oracle.MODE_FASTQ)
    ref_path = str(tmp_path / "ref.naf")
    open(ref_path, "wb").write(R.naf)
    S = ["--screen", ref_path]
    want = planned.want("chain", 27)[0]
    p = unnaf_cli(S, A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, SP.kept_segments(want), "fastq")
    keep = planned.want("chain", 27, keep_matched=True)[0]
    p = unnaf_cli(S + ["--keep-matched", "--fasta", "--line-length", "60"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, SP.kept_segments(keep), "fasta", 60)
    p = unnaf_cli(S + ["--screen-table"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == SP.table(want, c.ids, A.lens)
    assert {line.split(b"\t")[-1] for line in p.stdout.split(b"\n")[1:-1]} == {b"clean", b"matched"}
    p = unnaf_cli(S + ["--screen-table", "--screen-k", "15", "--min-hits", "100", "--forward-only", "--records", "3-700"], A.naf)
    assert p.returncode == 0 and p.stdout == SP.table(SP.model(A.stream, R.stream, 15, min_hits=100, forward_only=True, first=2, count=698)[0], c.ids, A.lens)
    p = unnaf_cli(S + ["--sequences", "--screen-k", "31"], A.naf)
    assert p.returncode == 0 and p.stdout == TP.expected_text(text, A.N, SP.kept_segments(planned.want("chain", 31)[0]), "sequences")
    # quality trimming and adapter clipping first, duplicate collapsing last, all on the device
    quals = TP.quals_of(text, A.N)
    trows, _ = TP.model(quals, TP.LIMITS["Q20"], 100, TP.ee_units("0.06"))
    tb = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in trows]
    crows = CP.model(A.records, CP.Query([c.adapter]), 100, tb)[0]
    cb = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in crows]
    chain = ["--trim", "20", "--adapter", c.adapter, "--min-length", "100", "--max-ee", "0.06"]
    srows = SP.model(A.stream, R.stream, 27, bounds=cb)[0]
    sb = [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in srows]
    drows = DP.model(A.records, True, sb)[0]
    p = unnaf_cli(S + chain, A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, SP.kept_segments(srows), "fastq")
    p = unnaf_cli(chain + S + ["--dedup", "--either-strand"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, DP.kept_segments(drows), "fastq")
    assert 100 < len(DP.kept_segments(drows)) < len(SP.kept_segments(srows)) < sum(1 for x in crows if int(x["flags"]) & SP.KEPT)
    p = unnaf_cli(["--dedup", "--either-strand"] + S + chain + ["--screen-table"], A.naf)
    assert p.returncode == 0 and p.stdout == SP.table(srows, c.ids, A.lens, drows)
    assert {line.split(b"\t")[-1] for line in p.stdout.split(b"\n")[1:-1]} == {b"clean", b"matched", b"duplicate", b"short", b"errors", b"short,errors"}
    srows_t = SP.model(A.stream, R.stream, 27, bounds=tb)[0]
    p = unnaf_cli(S + ["--trim", "20", "--min-length", "100", "--max-ee", "0.06", "--seq"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == TP.expected_text(text, A.N, SP.kept_segments(srows_t), "seq")
    c2, arc2, ref2 = planned["dna_fastq"]                                               # FASTA reads against a FASTQ reference: FASTA by default
    F = arc2["own"]
    open(ref_path, "wb").write(ref2["oracle"].naf)
    p = unnaf_cli(S + ["--screen-k", "17", "--screen-table"], F.naf)
    assert p.returncode == 0 and p.stdout == SP.table(planned.want("dna_fastq", 17)[0], c2.ids, F.lens)
    segs = SP.kept_segments(planned.want("dna_fastq", 17)[0])
    recs = F.oracle.unnaf(F.naf, F.oracle.MODE_FASTA, True).split(b">")[1:]
    p = unnaf_cli(S + ["--screen-k", "17", "--line-length", "0"], F.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == b"".join(b">" + recs[r].partition(b"\n")[0] + b"\n" + recs[r].partition(b"\n")[2].replace(b"\n", b"") + b"\n" for r, _, _ in segs)
    p = unnaf_cli(S + ["--trim", "20"], F.naf)
    assert p.returncode == 1 and b"no quality" in p.stderr and p.stdout == b""
    for args in (S + ["--region", "nosuch"], S + ["--records", "1-99999"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    open(ref_path, "wb").write(b"not an archive")
    p = unnaf_cli(S, A.naf)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: --screen reference: ")


# ---- 13. who takes part, at the wave and workgroup seams of a launch with a lane per record ------------------------------------------------
def test_considered_and_who_takes_part_at_the_seams_of_a_launch(oracle, gpu):
    """513 reads of 8 to 12 bases, every other one cut out of the reference; the bounds rows carry NAF_GPU_TRIM_KEPT for exactly the first
    n, the last n and every n-th record (dedup_plan.part_sets).  `considered` is the number of set bits, and a read that takes no part has
    no hits and its row as it went in."""
    K = 4
    rng = np.random.default_rng(9950 + SEED)
    ref = SP.Ref("short", ["", SP.capped(rng, 80), SP.capped(rng, 30)])
    B = SP.Builder(9960 + SEED, K, ref)
    for k in range(513):
        n = int(B.rng.integers(8, 13))
        i = B.source(n)
        B.add(B.big[i:i + n] if k % 2 else B.bg(n))
    c = SP.Case("short", B, ref, (K,), lower=False)
    A, R = archives(oracle, gpu, c.text, 0, "fasta", c.records)["oracle"], archives(oracle, gpu, ref.text, 0, "fasta", ref.records)["oracle"]
    assert A.N == 513 and min(A.lens) >= 8 and max(A.lens) <= 12
    for k, (name, takes) in enumerate(DP.part_sets(A.N)):
        bounds = DP.part_bounds(A.lens, takes)
        kw = dict(keep_matched=bool(k % 2), forward_only=bool(k % 4 >= 2))
        want, total_w = SP.model(A.stream, R.stream, K, bounds=bounds, **kw)
        rows, total = gpu.unnaf_screen(A.d_naf, R.d_naf, k=K, bounds=gpu.to_device(SP.bounds_rows(bounds, "trim")), bounds_kind="trim", **kw)
        differ("rows", rows, want, name)
        print(name, "considered", int(total.considered), "of", sum(takes))
        assert total_tuple(total) == total_w, (name, total_tuple(total), total_w)
        assert int(total.considered) == sum(takes), name
        out = [r for r, on in enumerate(takes) if not on]
        assert [(int(x["begin"]), int(x["end"]), int(x["flags"])) for x in rows[out]] == [bounds[r] for r in out] and not rows["hits"][out].any(), name
