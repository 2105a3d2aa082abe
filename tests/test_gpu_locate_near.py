"""GPU tests of the motif search with mismatches (naf_gpu_unnaf_locate_near_count, naf_gpu_unnaf_locate_near, unnaf --locate
--mismatches).  Expected rows never come from the code under test: they are what locate_near_plan.near_hits -- sums of shifted
mismatch arrays per record -- finds in the oracle's --sequences text of the same archive.  Every planned text is searched in two
archives, the oracle's and this library's own ennaf at level 1, at three seeds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import locate_near_plan as NP
import locate_plan as LP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
SEEDS = [3 * SEED + k for k in range(3)]
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
SEQ, SEQUENCES = 2, 3
CASES = [c.name for c in NP.planned(0)]
FIELDS = ("record", "begin", "pattern", "strand", "mismatches", "where")


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
        self.records = LP.records_from_sequences_text(oracle.unnaf(naf, oracle.MODE_SEQUENCES, False), self.h.n_sequences)
        self.d_naf = gpu.to_device(naf)
        self._want = {}

    def want(self, Q):
        """the model's rows, computed once per question and left unchanged"""
        if Q.key() not in self._want:
            self._want[Q.key()] = NP.near_hits(self.records, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count)
        return self._want[Q.key()]


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """(seed, name) -> (case, {"oracle": Archive, "own": Archive}), made when first asked for; the two archives of a text hold the same
    records and share the model's rows"""
    made = {}

    def get(seed, name):
        if (seed, name) not in made:
            c = next(x for x in NP.planned(seed) if x.name == name)
            a = Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type))
            own, _ = gpu.ennaf(gpu.to_device(c.text), seq_type=c.seq_type, level=1)
            b = Archive(oracle, gpu, own.cpu().numpy().tobytes())
            assert a.records == b.records and (c.r7 or a.records == c.records_upper), c.name
            b._want = a._want
            made[seed, name] = (c, {"oracle": a, "own": b})
        return made[seed, name]
    return get


def table(hits):
    return np.stack([hits[f].astype(np.int64) for f in FIELDS], axis=1) if len(hits) else np.zeros((0, 6), dtype=np.int64)


def check_query(gpu, A, Q):
    want = A.want(Q)
    hits, total = gpu.unnaf_locate_near(A.d_naf, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count)
    got = table(hits)
    assert total == len(want) == len(got), (total, len(want))
    if not np.array_equal(got, want):
        k = int(np.nonzero((got != want).any(axis=1))[0][0])
        raise AssertionError("first difference at hit %d: got %s, expected %s (%d hits)" % (k, got[k:k + 3].tolist(), want[k:k + 3].tolist(), len(want)))
    n, per = gpu.unnaf_locate_near_count(A.d_naf, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count)
    assert n == len(want) and per == NP.histogram(want, len(Q.patterns))
    return got


# ---- 1. the tables and the histograms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("seed", SEEDS)
def test_rows_and_histograms_of_the_planned_texts(gpu, planned, seed, name, which):
    c, arc = planned(seed, name)
    got = {}
    for q, Q in enumerate(c.queries):
        got[q] = check_query(gpu, arc[which], Q)
    assert sum(len(v) for v in got.values()) > 0
    NP.check_places(c, lambda q: got[q])                                           # and the cells, read from the device's own table
    if name == "planted_even":
        assert len(got[c.dense_query]) >= 100000


# ---- 2. budget 0 without brackets is the exact search ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_budget_0_without_brackets_gives_the_rows_of_the_exact_search(gpu, planned, name):
    from naf_amd import capi
    c, arc = planned(SEEDS[0], name)
    n_rows = 0
    queries = c.queries[-4:]
    if name.startswith("stored"):                                                  # few windows are free of every laid letter: all queries, and the record that ends in two of them
        queries = c.queries + [NP.Query(["AC", "N", "R"], [0, 0, 0], 3, 2, 1)]
    for Q in queries:
        pats = [capi.motif_letters(p) for p in Q.patterns]
        for which in ("oracle", "own"):
            A = arc[which]
            near, total = gpu.unnaf_locate_near(A.d_naf, pats, 0, Q.strands, Q.first, Q.count)
            exact, total2 = gpu.unnaf_locate(A.d_naf, pats, Q.strands, Q.first, Q.count)
            assert total == total2 == len(near) == len(exact)
            for f in FIELDS[:4]:
                assert np.array_equal(near[f], exact[f]), f
            assert not near["mismatches"].any() and not near["where"].any()
            n_rows += total
    assert n_rows > 0


# ---- 3. restricted searches decode what they need; the trace line ------------------------------------------------------------------------------
def traced(gpu, A, Q, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    n, _ = gpu.unnaf_locate_near_count(A.d_naf, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = re.findall(r"\[locate-near\] patterns (\d+) budget max (\d+) records (\d+)\.\.(\d+) pieces (\d+) sequence bytes decoded (\d+) of (\d+) hits (\d+)\n", err)
    assert len(m) == 1, err
    return n, [int(x) for x in m[0]]


def test_a_restricted_search_decodes_only_the_blocks_behind_its_records(gpu, planned, monkeypatch, capfd):
    c, arc = planned(SEEDS[0], "planted_odd")
    for q in c.mixed_queries:
        Q = c.queries[q]
        for which in ("oracle", "own"):
            A = arc[which]
            n, (P, B, r0, r1, pieces, D, T, H) = traced(gpu, A, Q, monkeypatch, capfd)
            last = A.h.n_sequences if Q.count is None else Q.first + Q.count
            assert n == len(A.want(Q)) == H and (P, B, r0, r1, pieces) == (16, max(Q.budgets), Q.first, last, 1)
            assert T == (A.h.orig[4] + 1) // 2
            if which == "own" and Q.first == 2:
                assert D < T, (D, T)                                               # independent blocks: one record's range of them


# ---- 4. neither the piece size nor the run shows ---------------------------------------------------------------------------------------------
def raw_near(gpu, A, Q, d_hits, cap, budgets=None):
    from naf_amd import capi
    blob = b"".join(p.encode() + b"\0" for p in Q.patterns)
    n = C.c_uint64(12345)
    bud = (C.c_uint32 * len(Q.patterns))(*(Q.budgets if budgets is None else budgets))
    rc = gpu.L.naf_gpu_unnaf_locate_near(gpu.h, C.c_void_p(A.d_naf.data_ptr()), A.d_naf.numel(), blob, len(blob), len(Q.patterns), bud, Q.strands, Q.first,
                                         capi.WHOLE if Q.count is None else Q.count, C.c_void_p(d_hits.data_ptr() if d_hits is not None and d_hits.numel() else 0), cap, C.byref(n))
    return rc, n.value


def table_bytes(gpu, A, Q):
    import torch
    n = len(A.want(Q))
    buf = torch.full((32 * n + 33,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, total = raw_near(gpu, A, Q, buf[1:], n)                                    # the table at an odd address
    torch.cuda.synchronize()
    assert rc == 0 and total == n and int(buf[0]) == 0xA5 and bool((buf[1 + 32 * n:] == 0xA5).all())
    return buf[1:1 + 32 * n].cpu().numpy().tobytes()


@pytest.mark.parametrize("name", ["planted_even", "planted_odd", "stored_odd", "small", "fastq_reads", "surplus"])
def test_the_same_bytes_at_one_record_a_piece_at_the_default_and_on_a_second_run(gpu, planned, name, monkeypatch, capfd):
    from naf_amd import capi
    c, arc = planned(SEEDS[0], name)
    for which in ("oracle", "own"):
        A = arc[which]
        for Q in c.queries[-3:]:
            if name == "fastq_reads" and Q.count is None:
                continue                                                           # (2000 reads: 2000 pieces; the restricted queries cross reads as well)
            want = A.want(Q)
            first = table_bytes(gpu, A, Q)
            assert np.array_equal(table(np.frombuffer(first, dtype=capi.NEAR_HIT_DTYPE)), want)
            assert table_bytes(gpu, A, Q) == first                                 # a second run
            monkeypatch.setenv("NAF_GPU_LOCATE_PIECE", "1")
            assert table_bytes(gpu, A, Q) == first                                 # one record a piece
            n, tr = traced(gpu, A, Q, monkeypatch, capfd)
            last = A.h.n_sequences if Q.count is None else Q.first + Q.count
            assert n == len(want) and (tr[4] > 1 or last - Q.first <= 1)           # it was searched in pieces
            monkeypatch.setenv("NAF_GPU_LOCATE_PIECE", "4097")
            assert table_bytes(gpu, A, Q) == first
            monkeypatch.delenv("NAF_GPU_LOCATE_PIECE")


# ---- 5. capacity, in a fenced arena --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_capacity_in_a_fenced_arena(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x3C, size=4 << 20)
    for name, qi, phase in (("small", 0, 1), ("planted_odd", 0, 0), ("fastq_reads", 1, 65), ("rna", 0, 9)):
        c, arc = planned(SEEDS[0], name)
        A, Q = arc[which], c.queries[qi]
        want = A.want(Q)
        n = len(want)
        assert n >= 2
        # one entry too few: the whole count in *n_hits and in the message, and nothing written
        arena.reset()
        out = arena.out(32 * (n - 1), phase)
        before = out.clone()
        rc, total = raw_near(gpu, A, Q, out, n - 1)
        torch.cuda.synchronize()
        assert rc == E_CAP and total == n
        assert ("%d hits, capacity %d" % (n, n - 1)) in gpu.L.naf_gpu_last_error(gpu.h).decode()
        assert torch.equal(out, before)
        arena.check()
        # exactly enough: n entries and nothing outside the table
        arena.reset()
        out = arena.out(32 * n, phase)
        rc, total = raw_near(gpu, A, Q, out, n)
        torch.cuda.synchronize()
        assert rc == 0 and total == n
        arena.check()
        assert np.array_equal(table(np.frombuffer(out.cpu().numpy().tobytes(), dtype=capi.NEAR_HIT_DTYPE)), want)
    # the binding's own form with a caller's buffer at an odd byte offset
    c, arc = planned(SEEDS[0], "small")
    A, Q = arc[which], c.queries[0]
    want = A.want(Q)
    buf = torch.zeros(32 * len(want) + 33, dtype=torch.uint8, device="cuda")
    view, total = gpu.unnaf_locate_near(A.d_naf, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count, out=buf[1:])
    assert total == len(want) and view.numel() == 32 * total and not bool(buf[1 + 32 * total:].any()) and int(buf[0]) == 0
    assert np.array_equal(table(np.frombuffer(view.cpu().numpy().tobytes(), dtype=capi.NEAR_HIT_DTYPE)), want)
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_locate_near(A.d_naf, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count, out=buf[1:1 + 32 * (len(want) - 1)])
    assert e.value.code == E_CAP and str(len(want)) in e.value.msg


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    from naf_amd import capi
    c, arc = planned(SEEDS[0], "small")
    A = arc["own"]
    N = A.h.n_sequences

    def fails(patterns, budgets=0, strands=3, first=0, count=None, words=()):
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_locate_near_count(A.d_naf, patterns, budgets, strands, first, count)
        assert e.value.code == E_ARG, e.value
        for w in words:
            assert w in e.value.msg, e.value.msg
        with pytest.raises(capi.NafGpuError) as e2:
            gpu.unnaf_locate_near(A.d_naf, patterns, budgets, strands, first, count)
        assert e2.value.code == E_ARG and e2.value.msg == e.value.msg

    fails(["ACGT", "ACXT"], words=("pattern 1", "'X'", "position 3"))
    fails(["AC-T"], words=("pattern 0", "'-'"))
    fails(["NGG", "G[G]", "A[5]"], words=("pattern 2", "'5'", "position 3"))
    fails(["NGG", ""], words=("pattern 1", "0 letters"))
    fails(["A" * 33], words=("pattern 0", "33"))
    fails(["[" + "A" * 33 + "]"], words=("pattern 0", "33"))
    fails(["A", "AC[]G"], words=("pattern 1", "empty brackets", "position 4"))
    fails(["[]"], words=("pattern 0", "empty brackets", "position 2"))
    fails(["A[C[G]]"], words=("pattern 0", "do not nest", "position 4"))
    fails(["AC]G"], words=("pattern 0", "without a '['", "position 3"))
    fails(["A", "A", "AC[GT"], words=("pattern 2", "never closed"))
    fails(["ACGT"], budgets=9, words=("pattern 0", "9 mismatches", "the most is 8"))
    fails(["ACGTACGTACGT", "ACG"], budgets=[3, 3], words=("pattern 1", "3 mismatches", "3 letters outside brackets"))
    fails(["AC[GT]"], budgets=2, words=("pattern 0", "2 letters outside brackets"))
    fails(["[GAATTC]"], budgets=1, words=("pattern 0", "0 letters outside brackets"))
    fails([], words=("patterns",))
    fails(["A"] * 17, words=("17",))
    fails(["A"], strands=0, words=("strand",))
    fails(["A"], strands=4, words=("strand",))
    fails(["A"], first=N + 1, words=("record",))
    fails(["A"], first=1, count=N, words=("records",))
    with pytest.raises(ValueError):
        gpu.unnaf_locate_near_count(A.d_naf, ["A", "C"], [0])                      # a budget per pattern, or one for all
    n, zero = C.c_uint64(), (C.c_uint32 * 3)(0, 0, 0)

    def raw(blob, blob_len, n_patterns, budgets):
        rc = gpu.L.naf_gpu_unnaf_locate_near_count(gpu.h, C.c_void_p(A.d_naf.data_ptr()), A.d_naf.numel(), blob, blob_len, n_patterns, budgets, 3, 0, capi.WHOLE, C.byref(n), None)
        return rc, gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
    rc, msg = raw(b"A\0", 2, 1, None)
    assert rc == E_ARG and "h_max_mismatches is NULL" in msg
    rc, msg = raw(None, 0, 1, zero)
    assert rc == E_ARG and "h_patterns is NULL" in msg
    rc, msg = raw(b"AC\0GT\0", 6, 3, zero)                                        # three announced, two there
    assert rc == E_ARG and "3 patterns announced, 2 zero-terminated strings in 6 bytes" in msg
    rc, msg = raw(b"AC\0GT", 5, 2, zero)                                           # the second one is not terminated inside the bytes given
    assert rc == E_ARG and "2 patterns announced, 1 zero-terminated strings in 5 bytes" in msg
    rc, msg = raw(b"AC\0G\x07T\0", 7, 2, zero)                                     # a letter that cannot be printed is named by its byte
    assert rc == E_ARG and "pattern 1" in msg and "'\\x07' (position 2)" in msg
    rc, msg = raw(b"[A\xE9]\0", 5, 1, zero)
    assert rc == E_ARG and "pattern 0" in msg and "'\\xE9' (position 3)" in msg
    assert gpu.unnaf_locate_near_count(A.d_naf, ["A"], 0, 3, N, 0)[0] == 0 and gpu.unnaf_locate_near_count(A.d_naf, ["A"], 0, 3, N, None)[0] == 0
    assert gpu.unnaf_locate_near_count(A.d_naf, ["[GAATTC]"], 0)[0] == len(NP.near_hits(A.records, ["[GAATTC]"], 0)) > 0      # all letters bracketed: budget 0 is legal
    # protein and text archives are refused; an archive without records has no hits
    for name, word in (("protein_small", "protein"), ("text_small", "text")):
        d = gpu.to_device(golden_bytes("naf", name + ".naf"))
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_locate_near_count(d, ["AC"], 1)
        assert e.value.code == E_ARG and word in e.value.msg
    empty = gpu.to_device(oracle.ennaf(b""))
    assert gpu.unnaf_locate_near_count(empty, ["AC", "N[GG]"], [1, 0]) == (0, [[[0] * 9, [0] * 9]] * 2)
    hits, total = gpu.unnaf_locate_near(empty, ["AC"], 1)
    assert total == 0 and len(hits) == 0


# ---- 7. composition with the selection path -----------------------------------------------------------------------------------------------------
def mismatched(stored, letter):
    return not (stored != "-" and set(LP.SETS[stored]) <= set(LP.SETS[letter]))


@pytest.mark.parametrize("name", ["planted_odd", "stored_even", "small", "rna", "fastq_reads"])
def test_every_hit_selects_a_site_within_the_budget_of_its_pattern(gpu, planned, name):
    from naf_amd import capi
    c, arc = planned(SEEDS[0], name)
    A = arc["own"]
    rng = np.random.default_rng(7990 + SEED)
    seen = set()
    for Q in c.queries[:2] + [q for q in c.queries if q.strands == 2][:1] + c.queries[-2:]:
        hits, total = gpu.unnaf_locate_near(A.d_naf, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count)
        assert total == len(A.want(Q))
        if not total:
            continue                                                               # (a query whose only place is planted not to be a hit)
        pick = hits if total <= 2000 else hits[np.sort(rng.choice(total, 2000, replace=False))]
        segs = capi.hits_to_segments(pick, Q.patterns)
        text = gpu.unnaf_select(A.d_naf, segs, SEQ, use_mask=False).cpu().numpy().tobytes().decode("latin1")
        at = 0
        for h, (r, b, e, rv) in zip(pick, segs):
            letters, fixed = NP.parse(Q.patterns[int(h["pattern"])])
            site = text[at:at + len(letters)].upper().replace("U", "T")              # the strand is applied: the site reads along the pattern
            at += len(letters)
            miss = [mismatched(s, p) for s, p in zip(site, letters)]
            assert e - b == len(letters) == len(site) and rv == int(h["strand"])
            assert sum(miss) == int(h["mismatches"]) <= Q.budgets[int(h["pattern"])], (site, letters, h)
            assert sum(1 << j for j, x in enumerate(miss) if x) == int(h["where"]) and not any(x and f for x, f in zip(miss, fixed)), (site, letters, h)
            seen.add((rv, int(h["mismatches"]) > 0))
        assert at == len(text)
    assert (0, True) in seen and (name == "stored_even" or (0, False) in seen) and (name in ("rna", "stored_even") or (1, True) in seen)      # (the stored texts are searched as stored only)


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf, env=None):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                          env=dict(os.environ, **(env or {})))


def lines(rows, ids, patterns):
    out = []
    for r, b, p, s, e, w in rows.tolist():
        letters = NP.letters_of(patterns[p])
        site = "".join(ch.lower() if w >> j & 1 else ch.upper() for j, ch in enumerate(letters))
        out.append("%s\t%d\t%d\t%s\t%d\t%s\t%s\n" % (ids[r], b, b + len(letters), letters, e, "-" if s else "+", site))
    return "".join(out).encode("latin1")


def test_cli_locate_with_mismatches_and_brackets(gpu, oracle, planned, tmp_path):
    c, arc = planned(SEEDS[0], "small")
    A = arc["own"]
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    assert len(ids) == A.h.n_sequences
    pats = ["GAATTC", "ccAcc", "CC[N]CC"]
    want = NP.near_hits(A.records, pats, 1, 3)
    p = unnaf_cli(["--locate", pats[0], "--locate", pats[1], "--mismatches", "1", "--locate", pats[2]], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == lines(want, ids, pats)
    assert b"\tGAATTC\t1\t-\tgAATTC\n" in p.stdout and b"\tccAcc\t1\t+\tCCaCC\n" in p.stdout and b"\tCCNCC\t0\t+\tCCNCC\n" in p.stdout
    p = unnaf_cli(["--locate", "GAATTC", "--mismatches", "2", "--strand", "-"], A.naf)
    assert p.returncode == 0 and p.stdout == lines(NP.near_hits(A.records, ["GAATTC"], 2, 2), ids, ["GAATTC"]) and p.stdout.count(b"\n") >= 2
    # a bracketed pattern alone takes the near call (budget 0); --mismatches 0 alone does too; neither: the exact call's six columns
    p = unnaf_cli(["--locate", "CC[N]CC"], A.naf)
    assert p.returncode == 0 and p.stdout == lines(NP.near_hits(A.records, ["CC[N]CC"], 0, 3), ids, ["CC[N]CC"]) and p.stdout.count(b"\n") > 2
    p0 = unnaf_cli(["--locate", "GAATTC", "--mismatches", "0"], A.naf)
    assert p0.returncode == 0 and p0.stdout == lines(NP.near_hits(A.records, ["GAATTC"], 0, 3), ids, ["GAATTC"])
    p = unnaf_cli(["--locate", "GAATTC"], A.naf)
    assert p.returncode == 0 and p.stdout == b"".join(b"\t".join(ln.split(b"\t")[:6]) + b"\n" for ln in p0.stdout.splitlines())
    p = unnaf_cli(["--locate", "GAATTC", "--mismatches", "1", "--records", "2-3", "--strand", "+"], A.naf)
    assert p.returncode == 0 and p.stdout == lines(NP.near_hits(A.records, ["GAATTC"], 1, 1, 1, 2), ids, ["GAATTC"])
    p = unnaf_cli(["--locate", "GAATTC", "--mismatches", "1", "--region", ids[1]], A.naf)
    assert p.returncode == 0 and p.stdout == lines(NP.near_hits(A.records, ["GAATTC"], 1, 3, 1, 1), ids, ["GAATTC"]) and p.stdout.count(b"\n") >= 4
    # a FASTQ archive, to a file, in pieces
    c, arc = planned(SEEDS[0], "fastq_reads")
    A = arc["oracle"]
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    pats = ["GATTACAGATTACA", "GATTACA[GATT]ACA"]
    f, out = tmp_path / "reads.naf", tmp_path / "hits.bed"
    f.write_bytes(A.naf)
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--locate", pats[0], "--locate", pats[1], "--mismatches", "2", "-o", str(out), str(f)],
                       env=dict(os.environ, NAF_GPU_LOCATE_PIECE="20001"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout == b"" and out.read_bytes() == lines(NP.near_hits(A.records, pats, 2, 3), ids, pats)
    # what cannot be: nothing on stdout, exit 1
    A = planned(SEEDS[0], "small")[1]["own"]
    for args in (["--locate", "ACGT", "--mismatches", "1", "--region", "nosuch"], ["--locate", "ACGT", "--mismatches", "1", "--records", "1-99"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    p = unnaf_cli(["--locate", "ACGT", "--mismatches", "1"], golden_bytes("naf", "protein_small.naf"))
    assert p.returncode == 1 and p.stdout == b"" and b"protein" in p.stderr
