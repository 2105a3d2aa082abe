"""The selection path (naf_gpu_unnaf_find, naf_gpu_unnaf_select, naf_gpu_unnaf_select_stranded, naf_gpu_unnaf_record_table) on the lists
of tests/select_plan.py: a segment's first and last base, a header's digits, a line end, a mask toggle and a zero-size segment at every
phase of nibble pair, 16-byte chunk, 1 KiB round, 4 KiB tile, 128 KiB stream block and merged range; ids that differ in one byte the
probe does not see (run with -m gpu on an MI355X).

Every text is archived twice -- by the oracle (raw 128 KiB blocks) and by this build's ennaf at its default level -- and what a call must
return is cut in Python out of the ORACLE's text of the archive under test (select_plan.Records), never out of the plan's text or this
library's output.  All inputs are valid archives and valid segments; all comparisons are byte-exact."""
import ctypes as C
import re

import numpy as np
import pytest

import select_plan as SP
from select_plan import FASTA, FASTQ, SEQ, SEQUENCES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def host(t):
    return t.cpu().numpy().tobytes()


_ARCHIVE = {}          # the archive of the current (text, maker, seed) and the oracle's views of it: one at a time


def make_archive(gpu, oracle, text, seq_type, maker, fastq=False):
    if maker == "oracle":
        return oracle.ennaf(text, seq_type, well_formed=fastq)
    d_naf, _ = gpu.ennaf(gpu.to_device(text), seq_type=seq_type)
    return host(d_naf)


def archive(gpu, oracle, name, maker, seed):
    key = (name, maker, seed)
    if _ARCHIVE.get("key") != key:
        _ARCHIVE.clear()
        T = SP.text_of(name, seed, maker)
        naf = make_archive(gpu, oracle, T.data, T.seq_type, maker, T.fastq)
        if maker == "own":
            assert oracle.unnaf(naf, FASTQ if T.fastq else FASTA) == T.data              # the archive under test holds the plan's text
        _ARCHIVE.update(key=key, naf=naf, d_naf=gpu.to_device(naf), T=T, records={})
    return _ARCHIVE


def records(A, oracle, mode, use_mask, ll):
    k = (mode, use_mask, ll)
    if k not in A["records"]:
        A["records"][k] = SP.Records(oracle, A["naf"], mode, use_mask, ll)
    return A["records"][k]


def api(segs, strands=True):
    from naf_amd import capi
    return [(r, b, capi.WHOLE if e is None else e) + ((int(rv),) if strands else ()) for r, b, e, rv in segs]


def check_case(gpu, oracle, A, case, bad, rng):
    """One list: its bytes and its size, through _stranded and (a list without a reverse segment) through naf_gpu_unnaf_select too, and
    eight of its segments alone."""
    d, view = A["d_naf"], (case.mode, case.use_mask, case.ll)
    R = records(A, oracle, *view)
    want = R.expect(case.segs)
    forward = not any(s[3] for s in case.segs)
    got = host(gpu.unnaf_select(d, api(case.segs), *view))                               # 4-tuples: naf_gpu_unnaf_select_stranded
    if forward:                                                                          # all-zero strands there, no strands at all through naf_gpu_unnaf_select
        from naf_amd import capi
        if host(gpu.unnaf_select(d, api(case.segs, False), *view)) != got and len(bad) < 12:
            bad.append("%s: naf_gpu_unnaf_select and _stranded with all-zero strands differ" % case.label)
        n, o = C.c_size_t(), capi.UnnafOpts(*view)
        assert gpu.L.naf_gpu_unnaf_select_stranded_size(gpu.h, C.c_void_p(d.data_ptr()), d.numel(), C.byref(o), gpu._segments(api(case.segs, False)),
                                                        (C.c_uint8 * len(case.segs))(), len(case.segs), C.byref(n)) == 0 and n.value == len(want), case.label
    if got != want and len(bad) < 12:
        bad.append("%s (mode %d mask %d ll %d, %d segments): %s" % (case.label, *view, len(case.segs), first_diff(got, want)))
    assert gpu.unnaf_select_size(d, api(case.segs, not forward), *view) == len(want), case.label
    pick = range(len(case.segs)) if len(case.segs) <= 8 else sorted(set(int(k) for k in rng.integers(0, len(case.segs), 8)))
    for k in pick:
        s = case.segs[k]
        alone = R.segment(*s)
        if host(gpu.unnaf_select(d, api([s]), *view)) != alone and len(bad) < 12:
            bad.append("%s (mode %d mask %d ll %d): segment %d %r alone" % (case.label, *view, k, s))
    return len(want)


def first_diff(got, exp):
    g, e = np.frombuffer(got, dtype=np.uint8), np.frombuffer(exp, dtype=np.uint8)
    m = min(len(g), len(e))
    d = np.flatnonzero(g[:m] != e[:m])
    return "length %d for %d, first differing offset %s" % (len(g), len(e), int(d[0]) if len(d) else "none")


def traced(gpu, call, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    got = call()
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = re.findall(r"\[select\] segments (\d+) ranges (\d+) sequence bytes decoded (\d+) of (\d+) side sections (\d+)\n", err)
    assert len(m) == 1, err
    return got, [int(x) for x in m[0]]


PARAMS = [(name, cls, maker, seed) for name in SP.CLASSES_OF for seed in SP.SEEDS for maker in SP.MAKERS_OF[name] for cls in SP.CLASSES_OF[name]
          if maker in SP.makers_of(name, cls)]                                           # (ordered so that an archive is made once)


# ---- 1. select ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls,maker,seed", PARAMS, ids=["%s-%s-%s-%d" % p for p in PARAMS])
def test_planned_selections(gpu, oracle, name, cls, maker, seed, monkeypatch, capfd):
    seed += SP.SEED
    A = archive(gpu, oracle, name, maker, seed)
    rng = np.random.default_rng(8100 + seed)
    cases = SP.cases_of(name, cls, seed, maker=maker)
    assert cases
    bad, total = [], 0
    for case in cases:
        total += check_case(gpu, oracle, A, case, bad, rng)
    assert not bad, "%d lists, first mismatches:\n%s" % (len(cases), "\n".join(bad))
    assert total > 0
    if cls == "far":                                                                      # ... and what was decoded for them
        T = A["T"]
        for case in cases:
            view = (case.mode, case.use_mask, case.ll)
            got, (K, ranges, D, Tb, side) = traced(gpu, lambda: host(gpu.unnaf_select(A["d_naf"], api(case.segs), *view)), monkeypatch, capfd)
            assert got == records(A, oracle, *view).expect(case.segs)
            assert K == len(case.segs) and side == 1 and Tb == (T.T + 1) // 2
            if K == 32:
                assert ranges == 32, ranges
            else:
                assert 1 < ranges <= 32, ranges
            assert D < Tb, (D, Tb)


# ---- 2. find -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SP.SEEDS)
@pytest.mark.parametrize("maker", ["oracle", "own"])
@pytest.mark.parametrize("n", SP.ID_COUNTS)
def test_planned_id_lookups(gpu, oracle, n, maker, seed):
    seed += SP.SEED
    plan = SP.ids_find(seed)
    naf = make_archive(gpu, oracle, SP.id_text(plan, n), oracle.DNA, maker)
    ids = oracle.zstd_decompress(oracle.parse_naf(naf).frame(naf, 0)).split(b"\0")[:-1]
    assert ids == plan.ids[:n]
    want = SP.first_index(ids)
    d = gpu.to_device(naf)
    lists = SP.id_queries(plan, n, seed)
    assert [len(q) for q in lists[1:]] == list(SP.QUERY_COUNTS)
    for q in lists:
        got = gpu.unnaf_find(d, q)
        exp = [want.get(x) for x in q]
        wrong = [(k, len(q[k]), got[k], exp[k]) for k in range(len(q)) if got[k] != exp[k]]
        assert not wrong, "%d queries; (query, its length, record found, record expected): %s" % (len(q), wrong[:10])
    # the whole path by name: the record numbers of three archived twins, and a sub-range of each
    R = SP.Records(oracle, naf, FASTA)
    there = [t for t in plan.twins if t[0] > 32 and t[2] in want]
    for t in (there[0], there[len(there) // 2], there[-1]):
        r, missing = gpu.unnaf_find(d, [t[2], t[3]])
        assert r == want[t[2]] and missing is None
        seg = (r, 2, 9, 0)
        assert host(gpu.unnaf_select(d, api([seg]), FASTA)) == R.segment(*seg) == b">" + t[2] + b":3-9\n" + R.bases[r][2:9] + b"\n"


# ---- 3. the record table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maker", ["oracle", "own"])
@pytest.mark.parametrize("name", ["dna_seams", "rna_seams", "protein_seams", "text_seams", "fastq_seams"])
def test_record_table_of_the_seam_texts(gpu, oracle, name, maker):
    A = archive(gpu, oracle, name, maker, SP.SEED)
    T, d = A["T"], A["d_naf"]
    views = [(FASTQ, True, -1)] if T.fastq else [(FASTA, True, -1), (FASTA, False, 0), (FASTA, True, 17)]
    at_seams = sorted({0, T.N - 1} | {r for k in ("pad", "big", "tail", "empty_pair") if k in T.marks for r in (T.marks[k] - 1, T.marks[k], T.marks[k] + 1)}
                      | ({T.rec_of(s) + k for s in range(SP.BLOCK, T.T, SP.BLOCK) for k in (-1, 0, 1)} if T.fastq else set()))
    for view in views + [(SEQUENCES, True, -1), (SEQ, True, -1), (SEQ, False, -1)]:
        R = records(A, oracle, *view)
        n_bases, text_off = gpu.unnaf_record_table(d, 0, None, *view)
        assert n_bases == T.lens, view
        assert text_off == [0] + np.cumsum([len(w) for w in R.whole]).tolist(), view
        for r in at_seams:
            a, b = text_off[r], text_off[r + 1]
            whole = host(gpu.unnaf_select(d, [r], *view)) if b > a else b""
            assert whole == R.whole[r], (view, r)
            assert (host(gpu.unnaf_range(d, a, b, *view)) if b > a else b"") == whole, (view, r)
        first, count = max(0, T.N - 5), min(5, T.N)
        nb2, off2 = gpu.unnaf_record_table(d, first, count, *view)                        # a window of the table, the last record in it
        assert nb2 == n_bases[first:] and off2 == text_off[first:]
