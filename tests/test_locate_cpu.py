"""The motif search, the parts that need no GPU: the plan (locate_plan.py) held to its claims, its reference searcher against a
brute-force loop, naf_gpu_compile_motif (host only, through ctypes) against the plan's own tables, the command-line checks that run
before the device is opened, and the planned texts through the oracle's (and, where built, the reference's) unnaf."""
import os
import subprocess

import numpy as np
import pytest

import locate_plan as LP
from conftest import GOLDEN, ROOT

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
BIN = os.path.join(ROOT, "naf_amd", "bin")


def matches(text, pattern):
    """pattern against the stored letters text (same length), by the sets."""
    return len(text) == len(pattern) and all(t != "-" and set(LP.SETS[t]) <= set(LP.SETS[p]) for t, p in zip(text, LP.canon(pattern)))


# ---- 1. the planted texts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
def test_every_cell_is_planted_and_only_the_plants_hit(odd):
    P = LP.Planted(SEED, odd)
    assert P.total % 2 == int(odd) and sum(len(r) for r in P.records) == P.total
    assert [len(r) for r in P.records].count(0) == 4 and not P.records[0] and not P.records[-1]
    starts = [b for b, r in zip(P.rec_base, P.records) if r]
    assert {b & 1 for b in starts} == {0, 1}                                         # records start at both nibble parities
    assert set(P.stream_upper) == set("ACGT") and any(c.islower() for r in P.records for c in r)
    wins = P.windows()
    assert all(b0 - a1 > 32 for (_, a1), (b0, _) in zip(sorted(wins)[:-1], sorted(wins)[1:]))
    outside = bytearray(P.stream_upper.encode())
    for a, b in wins:
        outside[a:b] = b"A" * (b - a)
    assert set(outside.decode()) == set("AC")                                        # the background cannot start a hit
    pats = P.patterns()
    texts = [t for _, _, _, t in pats]
    assert all(t[0] in "GT" for t in texts)
    hits = LP.expected_hits(P.records_upper, texts, 1)
    by_pattern = {}
    for r, b, pi, s in hits:
        assert s == 0
        by_pattern.setdefault(pi, set()).add(P.rec_base[r] + b)
    ends = sorted(set(P.rec_base[1:] + [P.total]))
    table = {}
    for pi, (m, d, n_tail, text) in enumerate(pats):
        got = by_pattern.get(pi, set())
        # what a walk over the planted windows alone finds: a start inside a window, the pattern inside one record
        want = set()
        for a, b in wins:
            for x in range(a, b):
                if x + m <= P.total and matches(P.stream_upper[x:x + m], text) and not any(x < e < x + m for e in ends):
                    want.add(x)
        assert got == want, (m, d, n_tail, sorted(got ^ want)[:5])
        if n_tail:
            continue
        for kind, p in P.seams:
            fits = p + d + m <= P.total
            if fits:
                assert matches(P.stream_upper[p + d:p + d + m], text), (kind, p, m, d)   # the cell is planted
            else:
                assert kind == "end"
                assert d >= 0 or matches(P.stream_upper[p + d:], text[:P.total - p - d])   # what fits of it is (behind the last base nothing does)
            is_hit = P.planted_hit(kind, p, m, d)
            assert (p + d in got) == is_hit, (kind, p, m, d)
            table.setdefault((kind, m), []).append((d, is_hit))
        if m >= 15:
            assert got == {p + d for kind, p in P.seams if P.planted_hit(kind, p, m, d)}, (m, d)   # exactly the plants
    print("\nseam kind x pattern length: offsets planted (-m .. +1 at every seam of the kind) / of them hits; total %d bases (%s)" % (P.total, "odd" if odd else "even"))
    for kind in LP.SEAM_KINDS:
        row = []
        for m in LP.LENGTHS:
            cells = table[(kind, m)]
            assert {d for d, _ in cells} == set(range(-m, 2))                        # every offset, at every seam of the kind
            row.append("m=%d %d/%d" % (m, len(cells), sum(1 for _, h in cells if h)))
        print("%-7s %s" % (kind, "  ".join(row)))
    # a motif that ends on a record's last base is a hit, one base later it is none; the same at the stream's end
    for m in LP.LENGTHS:
        assert P.planted_hit("record", 1501, m, -m) and P.planted_hit("record", 1501, m, 0) and P.planted_hit("end", P.total, m, -m)
        assert not P.planted_hit("end", P.total, m, -m + 1)
        if m > 1:
            assert not P.planted_hit("record", 1501, m, -m + 1)


def test_the_planned_cases_cover_what_the_issue_lists():
    cases = {c.name: c for c in LP.planned(SEED)}
    assert set(cases) == {"planted_even", "planted_odd", "dense", "ambiguity", "rna", "fastq_reads", "surplus"}
    for c in cases.values():
        assert 1 <= len(c.text) <= 700 << 10
        for pats, strands, first, count in c.queries:
            assert 1 <= len(pats) <= 16 and strands in (1, 2, 3)
    assert any(len(p) == 16 and s == 3 for p, s, _, _ in cases["dense"].queries)
    assert any("GAATTC" in p for p, _, _, _ in cases["dense"].queries) and LP.revcomp("GAATTC") == "GAATTC"
    ten = LP.expected_hits(["AAAAAAAAAA"], ["AAA"], 1)
    assert len(ten) == 8                                                             # AAA in a run of ten A
    assert len(LP.expected_hits(["GAATTC"], ["GAATTC"], 3)) == 2                     # a palindromic site: one hit a strand
    fq = cases["fastq_reads"]
    assert len(fq.records_upper) == 2000 and {len(r) for r in fq.records_upper} == {150}
    whole = LP.expected_hits(["".join(fq.records_upper)], ["GATTACAGATTACA"], 1)
    inside = LP.expected_hits(fq.records_upper, ["GATTACAGATTACA"], 1)
    assert len(whole) > len(inside) >= 2                                             # copies that straddle a read's end are no hits
    planted = cases["planted_odd"]
    base = planted.planted.rec_base
    assert any(base[f] % 2 == 1 and base[f] % 4096 and (c is None or base[f + c] % 4096) for _, _, f, c in planted.queries if f)


def test_the_subset_table_of_stored_and_pattern_letters():
    """Every stored code against every pattern letter: the character classes say what the sets say."""
    for p in LP.LETTERS:
        for s in LP.CODES:
            want = s != "-" and set(LP.SETS[s]) <= set(LP.SETS[p])
            assert bool(LP.expected_hits([s], [p], 1)) == want, (s, p)
            assert (s in LP.CLASS[p]) == want
    assert [s for s in LP.CODES if LP.expected_hits([s], ["N"], 1)] == list(LP.CODES[1:])
    assert sorted(p for p in LP.LETTERS if LP.expected_hits(["R"], [p], 1)) == ["D", "N", "R", "V"]
    assert [p for p in LP.LETTERS if LP.expected_hits(["N"], [p], 1)] == ["N"]
    for a, b in zip("ACGTMRWSYKVHDBN", "TGCAKYWSRMBDHVN"):
        assert set(LP.SETS[b]) == {"TGCA"["ACGT".index(x)] for x in LP.SETS[a]}      # the complement table, letter by letter


# ---- 2. the searcher against a triple loop ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_expected_hits_against_brute_force(k):
    rng = np.random.default_rng(7900 + 10 * SEED + k)
    alphabet = ["ACGT", LP.CODES, "ACGU" + "NRY-"][k]
    recs = ["".join(rng.choice(list(alphabet), int(n))) for n in (0, 300, 1, 77, 0, 150)]
    pats = ["A", "n", "NN", "RY", "acg", "GNNC", "KM", "U", "BDHV", "TTT", "SW", "CCWGG"]
    for strands in (1, 2, 3):
        assert LP.expected_hits(recs, pats, strands) == sorted(LP.brute_hits(recs, pats, strands))
    assert LP.expected_hits(recs, pats, 3, 1, 3) == sorted(LP.brute_hits(recs, pats, 3, 1, 3))
    assert LP.expected_hits(recs, pats, 3, 2, 0) == []


# ---- 3. naf_gpu_compile_motif ------------------------------------------------------------------------------------------------------------
def bitrev4(c):
    return ((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | (c >> 3)


def test_compile_motif_against_the_tables():
    from naf_amd import capi
    for p in LP.LETTERS + "U":
        for text in (p, p.lower()):
            fwd, rev = capi.compile_motif(text)
            code = LP.CODES.index(LP.canon(p))
            assert fwd == bytes([code]) and rev == bytes([bitrev4(code)])
            assert {LP.CODES[c] for c in range(1, 16) if c & ~code == 0} == set(LP.CLASS[LP.canon(p)][1:-1])     # the rule and the class agree
            assert LP.CODES[rev[0]] == LP.revcomp(p)
    rng = np.random.default_rng(7950 + SEED)
    for m in list(range(1, 33)) * 2:
        text = "".join(rng.choice(list(LP.LETTERS + "Uacgtun"), m))
        fwd, rev = capi.compile_motif(text)
        assert len(fwd) == len(rev) == m
        assert fwd == bytes(LP.CODES.index(c) for c in LP.canon(text))
        assert rev == bytes(bitrev4(c) for c in fwd[::-1])
        assert rev == bytes(LP.CODES.index(c) for c in LP.revcomp(text))
        assert capi.compile_motif(text.encode()) == (fwd, rev)


@pytest.mark.parametrize("text", ["", "A" * 33, "-", "AC-GT", "X", "ACGX", "5", "AC GT", "A\n", "NGG1"])
def test_compile_motif_rejects(text):
    from naf_amd import capi
    with pytest.raises(ValueError):
        capi.compile_motif(text)


def test_locate_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_compile_motif", "naf_gpu_unnaf_locate_count", "naf_gpu_unnaf_locate"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    import ctypes as C
    assert C.sizeof(capi.Hit) == 24 and np.dtype(capi.HIT_DTYPE).itemsize == 24
    hits = np.array([(3, 10, 1, 0), (4, 2, 0, 1)], dtype=capi.HIT_DTYPE)
    assert capi.hits_to_segments(hits, ["ACGT", "NGG"]) == [(3, 10, 13, 0), (4, 2, 6, 1)]
    assert capi.hits_to_segments(hits, ["ACGT", "NGG"], flank=5, lengths=[0, 0, 0, 15, 9]) == [(3, 5, 15, 0), (4, 0, 9, 1)]


# ---- 4. the command line, before the device is opened -------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [(["--locate", "NGG", "--fasta"], b"BED"), (["--seq", "--locate", "NGG"], b"BED"), (["--locate", "NGG", "--ids"], b"BED"),
                                       (["--locate", "NGG", "--records", "1-2", "--records", "3-4"], b"one --records or one --region"),
                                       (["--locate", "NGG", "--region", "x", "--records", "1"], b"one --records or one --region"),
                                       (["--locate", "NGG", "--region", "x:1-5"], b"whole sequence"), (["--locate", "NGG", "--rc-region", "x"], b"--rc-region can't"),
                                       (["--locate", "NGG", "--region", "x", "--revcomp"], b"--revcomp can't"),
                                       (["--locate", "NGX"], b"--locate parameter"), (["--locate", ""], b"--locate parameter"), (["--locate", "A" * 33], b"--locate parameter"),
                                       (["--locate", "A-C"], b"--locate parameter"), (["--locate", "NGG", "--strand", "x"], b"--strand parameter"),
                                       (["--strand", "+"], b"--strand can be used only with --locate"), (["--locate", "A"] * 17, b"at most 16 --locate")])
def test_locate_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr      # the check of this option, not the one for an option nobody knows


def test_help_gains_the_two_lines():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--locate" not in head and b"--strand" not in head
    assert b"\n  --locate PATTERN " in tail and b"\n  --strand +|-|both " in tail


# ---- 5. the texts decode to what the plan says --------------------------------------------------------------------------------------------
def test_the_planned_texts_through_the_oracle_and_the_reference(oracle, tmp_path):
    for c in LP.planned(SEED):
        naf = oracle.ennaf(c.text, c.seq_type)
        h = oracle.parse_naf(naf)
        recs = LP.records_from_sequences_text(oracle.unnaf(naf, oracle.MODE_SEQUENCES, False), h.n_sequences)
        if c.r7:
            assert sum(len(r) for r in recs) < h.orig[oracle.SEQ]                     # bases behind the last record
            flat = c.text.decode("latin1").upper()
            assert flat.rstrip("\n").endswith("GTTGTTGGTG") and not recs[-1].endswith("GTTGTTGGTG")
            assert not [x for x in LP.expected_hits(recs, ["GTTGTTGGTG"], 1) if x[0] == len(recs) - 1 and x[1] + 10 == len(recs[-1]) + 1]
        else:
            assert recs == c.records_upper, c.name
        if oracle.have_ref():
            args = ["--rna"] if c.seq_type == 1 else []
            ref = oracle.ref_ennaf(c.text, args, str(tmp_path))
            assert LP.records_from_sequences_text(oracle.ref_unnaf(ref, ["--sequences", "--no-mask"]), h.n_sequences) == recs, c.name
