"""The motif search with mismatches, the parts that need no GPU: the plan (locate_near_plan.py) held to its claims -- every cell has
its planted hit with exactly the planned mismatches and where, every place planted not to be a hit has none --, its vectorised model
against a triple loop and against the exact search's regexes, the coverage table of seam kind x cell, naf_gpu_compile_motif_near (host
only, through ctypes), the Python helpers, and the command-line checks that run before the device is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import locate_near_plan as NP
import locate_plan as LP
from conftest import GOLDEN, ROOT

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
BIN = os.path.join(ROOT, "naf_amd", "bin")


@pytest.fixture(scope="module")
def cases():
    return NP.planned(SEED)


@pytest.fixture(scope="module")
def rows(cases):
    """(case name, query) -> the model's rows, computed once and left unchanged"""
    cache = {}

    def get(c, q):
        if (c.name, q) not in cache:
            Q = c.queries[q]
            cache[c.name, q] = NP.near_hits(c.records_upper, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count)
        return cache[c.name, q]
    return get


# ---- 1. the plan's claims ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planted_even", "planted_odd", "stored_even", "stored_odd", "small", "rna", "fastq_reads"])
def test_every_cell_has_its_planted_hit_and_no_other(cases, rows, name):
    c = next(x for x in cases if x.name == name)
    assert c.places
    NP.check_places(c, lambda q: rows(c, q))
    for p in c.places:
        assert p.mismatches is None or bin(p.where).count("1") == p.mismatches
    if name.startswith("planted"):
        P = c.planted
        assert P.total % 2 == int(name == "planted_odd")                          # the odd stream ends in a padding nibble
        lens = {len(NP.letters_of(p)) for Q in c.queries for p in Q.patterns}
        assert lens == set(LP.LENGTHS)
        assert {e for Q in c.queries for e in Q.budgets} == set(NP.BUDGETS)
        mixed = c.queries[c.mixed_queries[0]]
        assert len(mixed.patterns) == 16 and len(set(mixed.budgets)) == len(NP.BUDGETS)      # 16 patterns with different budgets in one call
        assert {c.queries[q].first for q in c.mixed_queries} == {0, 3, 8, 2}
    if name == "planted_even":
        assert len(rows(c, c.dense_query)) >= 100000                                # the write pass crosses every tile


def test_the_coverage_table_has_no_empty_cell(cases):
    cov = NP.coverage(cases)
    kinds = list(LP.SEAM_KINDS) + ["none"]
    print("%-40s %s" % ("cell \\ seam kind", " ".join("%7s" % k for k in kinds)))
    for cell in sorted(cov):
        print("%-40s %s" % (cell, " ".join("%7d" % cov[cell].get(k, 0) for k in kinds)))
    planted = [k for k in cov if k.startswith(("budget_", "substituted_", "bracket_", "reverse_"))]
    want = ({"budget_%d_%s" % (e, w) for e in NP.BUDGETS for w in ("exact", "one_more")} |
            {"substituted_%s%s" % (r, b) for r in ("first", "last", "letter_15", "letter_16", "before_the_seam", "behind_the_seam") for b in ("", "_budget_0")} |
            {"bracket_%s_%s" % (w, i) for w in ("start", "end", "across_15_16") for i in ("inside", "outside")} |
            {"reverse_asymmetric", "reverse_bracket_inside", "reverse_bracket_outside"})
    assert set(planted) == want
    for cell in planted:
        assert all(cov[cell].get(k, 0) > 0 for k in LP.SEAM_KINDS), (cell, cov[cell])
    assert all(cov["reaches_over_an_end"].get(k, 0) > 0 for k in ("record", "end", "none"))
    for x in ("N", "R", "gap"):
        for p in "ARN":
            assert cov["stored_%s_under_%s" % (x, p)]["none"] > 0
    for cell in ("palindrome_both_strands", "record_shorter_than_the_pattern", "rna", "fastq"):
        assert cov[cell]["none"] > 0
    # stored N, R and gap under A, R and N, at window bases 0, 15, 16 and m - 1 of 17-, 31- and 32-letter windows: at every seam kind, and
    # wherever a window with that base next to the seam can lie inside one record, once as a hit and once as none
    stored = [c for c in cases if c.name.startswith("stored")]
    assert {len(NP.letters_of(p)) for c in stored for Q in c.queries for p in Q.patterns} == {17, 31, 32}
    for x in ("N", "R", "gap"):
        for p in "ARN":
            for base in ("0", "15", "16", "last"):
                cell = "stored_%s_under_%s_at_base_%s" % (x, p, base)
                assert all(cov[cell].get(k, 0) > 0 for k in LP.SEAM_KINDS), (cell, cov[cell])
                for kind in LP.SEAM_KINDS:
                    got = {q.mismatches is not None for c in stored for q in c.places if q.cell == cell and q.kind == kind}
                    if kind in ("lane", "load32", "tile", "block") or base == "last":
                        assert got == {True, False}, (cell, kind, got)
    for c in stored:                                                              # the laid letters are in the text, on both sides of every seam
        P = c.planted
        for kind, p in P.seams:
            for idx, xx in NP.STORED[c.name == "stored_odd"].items():
                if p - 32 + idx < P.total:
                    r, b = P.to_record(p - 32 + idx)
                    assert c.records_upper[r][b] == xx
    # hits and non-hits both: a cell that only ever says "no hit" would pass on a search that finds nothing
    for c in cases:
        if c.name.startswith("planted"):
            for kind in LP.SEAM_KINDS:
                got = {(p.cell, p.mismatches is not None) for p in c.places if p.kind == kind}
                for cell in planted:
                    expect_hit = not cell.endswith(("one_more", "budget_0", "inside"))
                    if kind == "end" and cell.startswith("substituted_behind"):
                        continue                                                  # behind the stream's end there is nothing to hit
                    assert (cell, expect_hit) in got, (c.name, kind, cell)


# ---- 2. the model -------------------------------------------------------------------------------------------------------------------------
def test_the_match_table_is_the_sets():
    for pi, p in enumerate(LP.LETTERS):
        for ci, s in enumerate(LP.CODES):
            assert bool(NP.OK[pi, ci]) == (s != "-" and set(LP.SETS[s]) <= set(LP.SETS[p]))
    assert not NP.OK[:, 0].any() and NP.OK[LP.LETTERS.index("N"), 1:].all()
    assert sorted(p for p in LP.LETTERS if NP.OK[LP.LETTERS.index(p), LP.CODES.index("R")]) == ["D", "N", "R", "V"]
    assert [p for p in LP.LETTERS if NP.OK[LP.LETTERS.index(p), LP.CODES.index("N")]] == ["N"]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_the_vectorised_model_is_the_triple_loop(cases, k):
    rng = np.random.default_rng(7950 + 10 * SEED + k)
    alphabet = ["ACGT", LP.CODES, "ACGU" + "NRY-"][k]
    recs = ["".join(rng.choice(list(alphabet), int(n))) for n in (0, 300, 1, 77, 0, 150)]
    pats = ["AC", "nnA", "N[N]", "R[Y]A", "acgtac", "G[NN]C", "KMKM", "UUA", "[BD]HV", "TTTTTTTTT", "SW[S]W", "CCWGG", "A" * 17, "AC" * 16, "[GAATTC]", "G"]
    budgets = [1, 2, 0, 1, 3, 1, 2, 1, 1, 8, 2, 3, 8, 8, 0, 0]
    for strands in (1, 2, 3):
        a = NP.near_hits(recs, pats, budgets, strands)
        assert [tuple(x) for x in a.tolist()] == sorted(NP.brute_near(recs, pats, budgets, strands))
        assert len(a) and all(bin(w).count("1") == e for e, w in a[:, 4:6].tolist())
    assert [tuple(x) for x in NP.near_hits(recs, pats, budgets, 3, 1, 3).tolist()] == sorted(NP.brute_near(recs, pats, budgets, 3, 1, 3))
    assert len(NP.near_hits(recs, pats, budgets, 3, 2, 0)) == 0
    small = next(c for c in cases if c.name == "small")
    for Q in small.queries:
        a = NP.near_hits(small.records_upper, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count)
        assert [tuple(x) for x in a.tolist()] == sorted(NP.brute_near(small.records_upper, Q.patterns, Q.budgets, Q.strands, Q.first, Q.count))


def test_budget_0_without_brackets_is_the_exact_search():
    rng = np.random.default_rng(7960 + SEED)
    recs = ["".join(rng.choice(list(LP.CODES), int(n))) for n in (200, 0, 3, 500)] + ["GAATTCGAATTC"]
    pats = ["A", "n", "NN", "RY", "acg", "GNNC", "KM", "U", "BDHV", "GAATTC"]
    a = NP.near_hits(recs, pats, 0, 3)
    assert [tuple(x) for x in a[:, :4].tolist()] == LP.expected_hits(recs, pats, 3) and not a[:, 4:].any()
    assert NP.histogram(a, len(pats))[9][0][0] == 2 and NP.histogram(a, len(pats))[9][1][0] == 2      # the palindrome: two hits a place


# ---- 3. naf_gpu_compile_motif_near --------------------------------------------------------------------------------------------------------
def test_compile_motif_near_brackets_and_fixed():
    from naf_amd import capi
    for text, letters, fixed in (("GAGTCCGAGCAGAAGAAGAA[NGG]", "GAGTCCGAGCAGAAGAAGAANGG", 0b111 << 20), ("[GAATTC]", "GAATTC", 0b111111),
                                 ("[TTTV]NNNNNNNNNNNNNNNNNNNNNNN", "TTTV" + "N" * 23, 0b1111), ("A[c]G[tu]N", "AcGtuN", 0b011010), ("[A]", "A", 1),
                                 ("[" + "ACGT" * 8 + "]", "ACGT" * 8, 2 ** 32 - 1), ("ACGT" * 7 + "ACG[T]", "ACGT" * 8, 1 << 31), ("[A][C]", "AC", 3)):
        fwd, rev, fx = capi.compile_motif_near(text)
        assert (fwd, rev) == capi.compile_motif(letters) and fx == fixed == NP.fixed_mask(text), text
        assert capi.compile_motif_near(text.encode()) == (fwd, rev, fx)
        assert capi.motif_letters(text) == letters == NP.letters_of(text) and capi.motif_letters(text.encode()) == letters.encode()
    rng = np.random.default_rng(7970 + SEED)
    for m in list(range(1, 33)) * 2:                                               # without brackets: naf_gpu_compile_motif's answer and no fixed letter
        text = "".join(rng.choice(list(LP.LETTERS + "Uacgtun"), m))
        assert capi.compile_motif_near(text) == capi.compile_motif(text) + (0,)
        assert capi.motif_letters(text) == text
        a, b = sorted(int(x) for x in rng.choice(m + 1, 2, replace=False))
        fwd, rev, fx = capi.compile_motif_near(text[:a] + "[" + text[a:b] + "]" + text[b:])
        assert (fwd, rev) == capi.compile_motif(text) and fx == sum(1 << j for j in range(a, b))


@pytest.mark.parametrize("text", ["", "A" * 33, "-", "AC-GT", "X", "ACGX", "5", "AC GT", "A\n", "NGG1",
                                  "[]", "A[]C", "[", "]", "[A", "A]", "A[C", "AC]", "[[A]]", "[A[C]]", "[A]]", "]A[", "[A][", "[X]", "[A-]", "[" + "A" * 33 + "]", "A" * 32 + "[C]"])
def test_compile_motif_near_rejects(text):
    from naf_amd import capi
    with pytest.raises(ValueError):
        capi.compile_motif_near(text)
    fwd, rev, fixed, n = (C.c_uint8 * 32)(*([0xEE] * 32)), (C.c_uint8 * 32)(*([0xEE] * 32)), C.c_uint32(77), C.c_size_t(78)
    assert capi.load().naf_gpu_compile_motif_near(text.encode(), fwd, rev, C.byref(fixed), C.byref(n)) == -8
    assert bytes(fwd) == bytes(rev) == b"\xEE" * 32                                # nothing of the caller's is touched


def test_locate_near_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_compile_motif_near", "naf_gpu_unnaf_locate_near_count", "naf_gpu_unnaf_locate_near"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    assert "#define NAF_GPU_LOCATE_MAX_MISMATCHES 8" in header and capi.LOCATE_MAX_MISMATCHES == 8 == NP.MAX_MISMATCHES
    assert "uint32_t mismatches, where; } naf_gpu_near_hit;" in header
    assert C.sizeof(capi.NearHit) == 32 == capi.NEAR_HIT_BYTES and np.dtype(capi.NEAR_HIT_DTYPE).itemsize == 32
    assert [n for n, _ in capi.NearHit._fields_] == [f[0] for f in capi.NEAR_HIT_DTYPE] == ["record", "begin", "pattern", "strand", "mismatches", "where"]
    near = np.array([(3, 10, 1, 0, 1, 4), (4, 2, 0, 1, 0, 0)], dtype=capi.NEAR_HIT_DTYPE)
    assert capi.hits_to_segments(near, ["AC[GT]", "N[G]G"]) == [(3, 10, 13, 0), (4, 2, 6, 1)]
    assert capi.hits_to_segments(near, ["[ACGT]", "NGG"], flank=5, lengths=[0, 0, 0, 15, 9]) == [(3, 5, 15, 0), (4, 0, 9, 1)]
    old = np.array([(3, 10, 1, 0), (4, 2, 0, 1)], dtype=capi.HIT_DTYPE)          # and the exact search's rows as before
    assert capi.hits_to_segments(old, ["ACGT", "NGG"]) == [(3, 10, 13, 0), (4, 2, 6, 1)]


# ---- 4. the command line, before the device is opened ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [(["--mismatches", "1"], b"--mismatches can be used only with --locate"),
                                       (["--locate", "ACGT", "--mismatches", "9"], b"--mismatches parameter"), (["--locate", "ACGT", "--mismatches", "x"], b"--mismatches parameter"),
                                       (["--locate", "ACGT", "--mismatches", "-1"], b"--mismatches parameter"), (["--locate", "ACGT", "--mismatches", ""], b"--mismatches parameter"),
                                       (["--locate", "ACGT", "--mismatches", "10"], b"--mismatches parameter"),
                                       (["--locate", "ACGT", "--mismatches", "1", "--mismatches", "2"], b"only one --mismatches"),
                                       (["--locate", "ACG", "--mismatches", "3"], b"smaller than the pattern's 3 letters"),
                                       (["--locate", "ACGTACGT", "--locate", "[ACG]T", "--mismatches", "1"], b"--locate [ACG]T"),
                                       (["--locate", "[GAATTC]", "--mismatches", "1"], b"smaller than the pattern's 0 letters"),
                                       (["--locate", "[]"], b"--locate parameter"), (["--locate", "A[C"], b"--locate parameter"), (["--locate", "AC]"], b"--locate parameter"),
                                       (["--locate", "[A[C]]"], b"--locate parameter"), (["--locate", "[" + "A" * 33 + "]"], b"--locate parameter"),
                                       (["--locate", "ACGT", "--mismatches", "1", "--fasta"], b"BED"),
                                       (["--locate", "A[C]GT", "--region", "x:1-5"], b"whole sequence")])
def test_near_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr


def test_help_gains_the_mismatches_line():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--mismatches" not in head
    assert b"\n  --mismatches N  - " in tail and b"ID begin end PATTERN mismatches strand SITE" in tail


# ---- 5. the texts decode to what the plan says ------------------------------------------------------------------------------------------------
def test_the_small_and_the_surplus_text_through_the_oracle(oracle, cases):
    for c in cases:
        if c.name not in ("small", "surplus", "stored_even", "stored_odd"):
            continue                                                              # (the others are locate_plan's texts: test_locate_cpu.py decodes them)
        naf = oracle.ennaf(c.text, c.seq_type)
        h = oracle.parse_naf(naf)
        recs = LP.records_from_sequences_text(oracle.unnaf(naf, oracle.MODE_SEQUENCES, False), h.n_sequences)
        if not c.r7:
            assert recs == c.records_upper
            continue
        assert sum(len(r) for r in recs) < h.orig[oracle.SEQ]                     # bases behind the last record: in no hit
        Q = c.queries[0]
        a = NP.near_hits(recs, Q.patterns, Q.budgets, Q.strands)
        last = len(recs) - 1
        assert len(a) and not [x for x in a.tolist() if x[0] == last and x[1] + len(NP.letters_of(Q.patterns[x[2]])) > len(recs[last])]
        assert c.text.decode("latin1").rstrip("\n").endswith("GTTGTTGGTG") and not recs[last].endswith("GTTGTTGGTG")
