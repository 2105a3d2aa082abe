"""What can be checked of the k-mer counts without a GPU: the plan (kmers_plan.py) against its own claims -- the numpy reference against a
plain loop, the seam coverage of the planted texts, the texts through the oracle --, the host-only parts of the C-ABI (naf_gpu_kmer_index,
naf_gpu_kmer_text, the exports, the row's layout) and the command line's argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmers_plan as KP
from conftest import GOLDEN, ROOT

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
BIN = os.path.join(ROOT, "naf_amd", "bin")


@pytest.fixture(scope="module")
def planned():
    return {c.name: c for c in KP.planned(SEED)}


def _lines(recs):
    return [r.encode("latin1") for r in recs]


# ---- 1. the reference against a plain loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_expected_counts_against_the_brute_loop(k):
    rng = np.random.default_rng(11900 + 10 * SEED + k)
    alphabet = ["ACGTN", KP.CODES, "ACGUacguNn--", "AAACCTTNn"][k]
    lines = _lines(["".join(rng.choice(list(alphabet), int(n))) for n in (0, 400, 1, 77, 0, 0, 150, 2, 12, 13)])
    for K in (1, 2, 3, 4, 5, 12):
        for canonical in (False, True):
            for per in (False, True) if K < 12 else (False,):
                assert KP.as_dicts(KP.expected_counts(lines, K, canonical, per), K) == KP.brute_counts(lines, K, canonical, per), (K, canonical, per)
            assert KP.as_dicts(KP.expected_counts(lines, K, canonical, True, 1, 2), K) == KP.brute_counts(lines, K, canonical, True, 1, 2)
            assert KP.as_dicts(KP.expected_counts(lines, K, canonical, False, 3, 4), K) == KP.brute_counts(lines, K, canonical, False, 3, 4)
        assert KP.expected_counts(lines, K, False, True, 3, 0).shape == (0, 4 ** K) and not KP.expected_counts(lines, K, False, False, 3, 0).any()


def test_the_planned_texts_against_the_brute_loop(planned):
    for name, ks in (("records", (1, 2, 3, 4, 5)), ("rna", (3,)), ("palindromes", (2, 4, 6)), ("lowk", (1, 2, 3)), ("reads", (1, 4)), ("end5", (2, 6)), ("end12", (7,))):
        lines = _lines(planned[name].records)
        for K in ks:
            for canonical in (False, True):
                assert KP.as_dicts(KP.expected_counts(lines, K, canonical), K) == KP.brute_counts(lines, K, canonical), (name, K, canonical)
            if K in planned[name].per_record_ks:
                assert KP.as_dicts(KP.expected_counts(lines, K, True, True), K) == KP.brute_counts(lines, K, True, True), (name, K)
    # K = 12 on sampled records
    rng = np.random.default_rng(11950 + SEED)
    for name in ("records", "palindromes", "two_records", "seams"):
        lines = _lines(planned[name].records)
        pick = sorted(int(x) for x in rng.choice(len(lines), min(4, len(lines)), replace=False))
        for r in pick:
            if len(lines[r]) > 20000:
                continue
            for canonical in (False, True):
                assert KP.as_dicts(KP.expected_counts(lines, 12, canonical, False, r, 1), 12) == KP.brute_counts(lines, 12, canonical, False, r, 1), (name, r)


def test_sparse_and_dense_references_agree(planned):
    lines = _lines(planned["records"].records)
    for K, canonical, per in ((3, False, True), (6, True, True), (8, False, False)):
        t = KP.expected_counts(lines, K, canonical, per, 2, 20).ravel()
        places, values = KP.expected_sparse(lines, K, canonical, per, 2, 20)
        assert np.array_equal(places, np.flatnonzero(t)) and np.array_equal(values, t[places])


def test_the_written_semantics():
    lines = [b"AAAAAAAAAA", b"ACGTNACGT", b"acgu", b"AC", b"", b"ACRGT-AC"]
    assert KP.brute_counts(lines, 3, first=0, count=1) == [{b"AAA": 8}]                # every start position counts
    assert KP.brute_counts(lines, 4, first=1, count=1) == [{b"ACGT": 2}]               # the N invalidates what covers it
    assert KP.brute_counts(lines, 4, first=2, count=1) == [{b"ACGT": 1}]               # case and U
    assert KP.brute_counts(lines, 3, first=3, count=2) == [{}]                         # shorter than K; never across two records
    assert KP.brute_counts(lines, 2, first=5, count=1) == [{b"AC": 2, b"GT": 1}]
    assert KP.brute_counts(lines, 2, canonical=True, first=5, count=1) == [{b"AC": 3}]
    assert KP.brute_counts([b"ACGTACGT"], 4, canonical=True) == [{b"ACGT": 2, b"CGTA": 2, b"GTAC": 1}]      # a palindrome counts once per occurrence, TACG with its reverse complement CGTA
    assert KP.expected_total(lines, 3) == (6, 0, 33, 8 + 7 + 2 + 0 + 0 + 6, 8 + 4 + 2 + 0 + 0 + 0)
    rows = KP.expected_rows(lines, 3, 1, 2)
    assert [tuple(int(v) for v in x) for x in rows] == [(1, 0, 9, 7, 4), (2, 0, 4, 2, 2)]


# ---- 2. the plan's coverage claims -------------------------------------------------------------------------------------------------------
def test_every_seam_kind_has_an_n_and_a_record_boundary_at_every_offset(planned):
    S = planned["seams"].seams
    cov = S.coverage()
    print("\n%-4s %-7s %3s offsets" % ("what", "kind", "K"))
    for what, kinds in (("N", KP.SEAM_KINDS), ("cut", KP.BOUNDARY_KINDS)):
        for kind in kinds:
            for K in KP.SEAM_KS:
                got = sorted(cov.get((what, kind, K), ()))
                print("%-4s %-7s %3d %s" % (what, kind, K, got))
                assert got == list(range(-K, K + 1)), (what, kind, K)
    assert len(S.stream) == S.TOTAL and S.TOTAL % 2 == 1 and S.TOTAL > 2 * KP.BLOCK
    assert sum(1 for r in S.records if not r) == 6 and S.records[0] == "" and S.records[-1] == ""
    assert all(p % 64 == 0 and p % KP.TILE for p in S.seams["lane"]) and all(p % KP.TILE == 0 for p in S.seams["tile"]) and S.seams["block"] == [KP.BLOCK, 2 * KP.BLOCK]


def test_the_streams_end_lies_at_every_distance_behind_a_tile_seam(planned):
    ends = [planned["end%d" % e] for e in range(KP.MAX_K + 2)]
    print("\n%-6s %-6s %-6s %s" % ("text", "behind", "parity", "N at"))
    offsets, parities = set(), set()
    for e, c in enumerate(ends):
        stream = "".join(c.records)
        assert len(stream) == 2 * KP.TILE + e and c.behind_tile == e
        assert stream.count("N") == 1 and stream[len(stream) + c.end_offset] == "N"
        print("%-6s %-6d %-6s %d" % (c.name, e, "odd" if len(stream) % 2 else "even", c.end_offset))
        offsets.add(c.end_offset)
        parities.add((e > 0, len(stream) % 2))
    assert offsets == set(range(-KP.MAX_K, 0))
    assert parities >= {(True, 0), (True, 1), (False, 0)}
    for K in KP.SEAM_KS:
        assert set(range(0, K + 2)) <= {c.behind_tile for c in ends}


def test_the_other_texts(planned):
    recs = planned["records"].records
    lens = [len(r) for r in recs]
    for K in KP.KS:
        assert {0, 1, K - 1, K, K + 1, 63, 64, 65, 4095, 4096, 4097} <= set(lens), K
    assert recs[0] == recs[1] == "" and recs[-1] == "" and any(a == b == "" for a, b in zip(recs[2:], recs[3:]))
    assert any(r and set(r.upper()) == {"N"} for r in recs) and any(set(r) >= set(KP.CODES) for r in recs)
    assert any(r != r.upper() and r != r.lower() for r in recs) and sum(lens) % 2 == 1
    rna = planned["rna"]
    assert rna.seq_type == 1 and b"U" in rna.text and b"T" not in rna.text.split(b"\n", 1)[1].replace(b">r", b"").upper().replace(b"SOME WORDS", b"")
    for K in (3, 6):
        assert np.array_equal(KP.expected_counts(_lines(rna.records), K, True, True), KP.expected_counts(_lines(recs), K, True, True))
    reads = planned["reads"].records
    assert len(reads) >= 4000 and {len(r) for r in reads} == set(KP.READ_LENGTHS)
    at = np.cumsum([0] + [len(r) for r in reads])
    tiles = (at[-1] + KP.TILE - 1) // KP.TILE
    assert all(np.searchsorted(at, (t + 1) * KP.TILE - 1) - np.searchsorted(at, t * KP.TILE, side="right") >= 1 for t in range(tiles - 1))      # a record boundary in every tile
    pal = _lines(planned["palindromes"].records)
    for K in (2, 4, 6, 12):
        plain, canon = KP.brute_counts(pal, K)[0], KP.brute_counts(pal, K, True)[0]
        selfrc = [w for w in plain if w == w.translate(KP._COMP)[::-1]]
        both = [w for w in plain if w != w.translate(KP._COMP)[::-1] and w.translate(KP._COMP)[::-1] in plain]
        assert len(selfrc) >= 2 and len(both) >= 2, K
        assert all(canon[w] == plain[w] for w in selfrc)                            # once per occurrence
        assert sum(canon.values()) == sum(plain.values())
    low = planned["lowk"].records
    assert low[0] == "A" * len(low[0]) and low[1] == "T" * len(low[1])
    assert planned["r7"].r7 and planned["no_records"].text == b"" and len(planned["two_records"].records) == 2
    for c in planned.values():
        assert len(c.text) <= 640 * 1024


# ---- 3. the host-only C-ABI -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,canonical,want", KP.INDEX_TABLE)
def test_kmer_index_against_the_table(text, canonical, want):
    from naf_amd import capi
    if want is None:
        with pytest.raises(ValueError):
            capi.kmer_index(text, canonical)
        return
    assert capi.kmer_index(text, canonical) == want
    assert capi.kmer_index(text.encode(), canonical) == want
    k, idx = want
    u = text.upper().replace("U", "T")
    rc = u.encode().translate(KP._COMP)[::-1].decode()
    assert want == (len(u), min(KP.index_of(u), KP.index_of(rc)) if canonical else KP.index_of(u))      # the table agrees with positional notation
    back = capi.kmer_text(k, idx)
    assert back == (min(u, rc) if canonical else u)
    assert capi.kmer_index(back, False) == (k, idx) and capi.kmer_index(back, True) == capi.kmer_index(text, True)
    if u == rc:
        assert capi.kmer_index(text, True) == capi.kmer_index(text, False)          # canonical of a palindrome is itself


@pytest.mark.parametrize("arg,want", KP.TEXT_TABLE)
def test_kmer_text_against_the_table(arg, want):
    from naf_amd import capi
    if want is None:
        with pytest.raises(ValueError):
            capi.kmer_text(*arg)
    else:
        assert capi.kmer_text(*arg) == want and capi.kmer_index(want) == arg


def test_kmer_round_trips_and_null_pointers():
    from naf_amd import capi
    rng = np.random.default_rng(11990 + SEED)
    for k in range(1, 13):
        for i in [0, 4 ** k - 1] + [int(x) for x in rng.integers(0, 4 ** k, 20)]:
            t = capi.kmer_text(k, i)
            assert len(t) == k and capi.kmer_index(t) == (k, i) and capi.kmer_index(t.lower().replace("t", "u")) == (k, i)
            rc = t.encode().translate(KP._COMP)[::-1].decode()
            assert capi.kmer_index(t, True) == capi.kmer_index(rc, True) == (k, min(i, KP.index_of(rc)))
    assert [capi.kmer_text(2, i) for i in range(16)] == sorted(capi.kmer_text(2, i) for i in range(16))      # ascending index: lexicographic order
    lib = capi.load()
    k, idx, out = C.c_uint(7), C.c_uint64(7), C.create_string_buffer(13)
    assert lib.naf_gpu_kmer_index(None, 0, C.byref(k), C.byref(idx)) != 0 and lib.naf_gpu_kmer_index(b"ACGT", 0, None, C.byref(idx)) != 0
    assert lib.naf_gpu_kmer_index(b"ACGT", 0, C.byref(k), None) != 0 and lib.naf_gpu_kmer_index(b"ACGN", 0, C.byref(k), C.byref(idx)) != 0 and (k.value, idx.value) == (7, 7)
    assert lib.naf_gpu_kmer_text(4, 27, None) != 0 and lib.naf_gpu_kmer_text(4, 256, out) != 0
    with pytest.raises(ValueError):
        capi.kmer_index("AC\0GT")


def test_kmers_are_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_kmer_index", "naf_gpu_kmer_text", "naf_gpu_unnaf_kmers_rows", "naf_gpu_unnaf_kmers"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert C.sizeof(capi.KmerRow) == 40 and np.dtype(capi.KMER_DTYPE).itemsize == 40 and capi.KMER_ROW_BYTES == 40
    assert capi.KMER_DTYPE == KP.KMER_DTYPE
    assert (capi.KMER_CANONICAL, capi.KMER_PER_RECORD) == (1, 2)
    assert [f[0] for f in capi.KmerRow._fields_] == ["record", "begin", "end", "positions", "counted"] and capi.KmerRow.counted.offset == 32
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    for word in ("naf_gpu_kmer_row;", "NAF_GPU_KMER_CANONICAL = 1", "NAF_GPU_KMER_PER_RECORD = 2", "naf_gpu_kmer_index", "naf_gpu_kmer_text", "naf_gpu_unnaf_kmers_rows",
                 "NAF_GPU_KMERS_PIECE", "most significant"):
        assert word in header, word


# ---- 4. the command line, before the device is opened -------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [(["--kmers", "0"], b"--kmers parameter"), (["--kmers", "13"], b"--kmers parameter"), (["--kmers", "x"], b"--kmers parameter"),
                                       (["--kmers", ""], b"--kmers parameter"), (["--kmers", "4.5"], b"--kmers parameter"), (["--kmers", "-3"], b"--kmers parameter"),
                                       (["--kmers", "99999999999999999999"], b"--kmers parameter"), (["--kmers", "4", "--kmers", "5"], b"only one --kmers"),
                                       (["--canonical"], b"--canonical can be used only with --kmers"), (["--per-record"], b"--per-record can be used only with --kmers"),
                                       (["--runs", "N", "--canonical"], b"--canonical can be used only with --kmers"),
                                       (["--kmers", "7", "--per-record"], b"6 at the most"), (["--kmers", "12", "--canonical", "--per-record"], b"6 at the most"),
                                       (["--kmers", "4", "--fasta"], b"no output type"), (["--seq", "--kmers", "4"], b"no output type"), (["--kmers", "4", "--ids"], b"no output type"),
                                       (["--kmers", "4", "--locate", "NGG"], b"--kmers and --locate"), (["--kmers", "4", "--composition"], b"--kmers and --composition"),
                                       (["--kmers", "4", "--quality"], b"--kmers and --quality"), (["--kmers", "4", "--runs", "N"], b"--kmers and --runs"),
                                       (["--masked-runs", "--kmers", "4"], b"--kmers and --masked-runs"),
                                       (["--kmers", "4", "--records", "1-2", "--records", "3-4"], b"one --records or one --region"),
                                       (["--kmers", "4", "--region", "x:1-5"], b"whole sequence"), (["--kmers", "4", "--rc-region", "x"], b"--rc-region can't"),
                                       (["--kmers", "4", "--region", "x", "--revcomp"], b"--revcomp can't")])
def test_kmers_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr      # the check of this option, not the one for an option nobody knows


def test_kmers_without_a_value_is_a_usage_error():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "-c", "--kmers"], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and b"--kmers" in p.stderr


def test_help_gains_the_three_lines():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--kmers" not in head
    for line in (b"\n  --kmers K ", b"\n  --canonical ", b"\n  --per-record "):
        assert line in tail
    assert tail.index(b"\n  --runs CLASS ") < tail.index(b"\n  --kmers K ")


# ---- 5. the texts decode to what the plan says --------------------------------------------------------------------------------------------
def test_the_planned_texts_through_the_oracle(oracle, planned):
    for c in planned.values():
        naf = oracle.ennaf(c.text, c.seq_type, well_formed=c.well_formed)
        h = oracle.parse_naf(naf)
        lines = KP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), h.n_sequences)
        if c.r7:
            assert sum(len(x) for x in lines) < h.orig[oracle.SEQ]                    # bases behind the last record
        else:
            assert [x.decode("latin1") for x in lines] == c.records, c.name
        if c.own_text:                                                              # what this build's ennaf archives instead: the same reads without the empty ones
            naf = oracle.ennaf(c.own_text, c.seq_type)
            lines = KP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), oracle.parse_naf(naf).n_sequences)
            assert [x.decode("latin1") for x in lines] == c.own_records == [r for r in c.records if r] and "" in c.records
