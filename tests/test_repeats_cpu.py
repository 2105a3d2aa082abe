"""CPU tests of the tandem-repeat table: the plan's reference against its brute walk, the planted texts and their coverage table, the host-only
C-ABI (naf_gpu_parse_repeat_spec, naf_gpu_repeat_class), the bindings and what unnaf refuses on the command line before the device is opened.
No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import repeats_plan as RP
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "naf_amd", "bin")


@pytest.fixture(scope="module")
def planned():
    return {c.name: c for c in RP.planned(0)}


# ---- 1. the model against the brute walk ---------------------------------------------------------------------------------------------
def test_the_model_agrees_with_the_brute_walk_on_random_lines():
    rng = np.random.default_rng(424242)
    n = 0
    for alphabet in ("ACGTacgtN", "AC", "ACGU-Rn"):
        for _ in range(40):
            lines = [RP._random(rng, int(rng.integers(0, 150)), alphabet).encode() for _ in range(3)]
            for spec, m, whole in itertools.product((RP.MISA, RP.ALL2, RP.ALL3), (1, 12), (False, True)):
                got = RP.as_tuples(RP.expected_repeats(lines, spec, m, whole))
                assert got == RP.brute_repeats(lines, spec, m, whole), (lines, spec, m, whole)
                n += len(got)
    assert n > 5000
    assert RP.as_tuples(RP.expected_repeats([b"ACACAGAGAG"], RP.ALL2)) == [(0, 0, 5, 0b0100, 2), (0, 4, 10, 0b1000, 2)]     # the contract's example
    assert RP.as_tuples(RP.expected_repeats([b"AAAA", b"ACACACAC", b"acgu" * 3 + b"a"], RP.ALL2)) == [(0, 0, 4, 0, 1), (1, 0, 8, 0b0100, 2), (2, 0, 13, 0b11100100, 4)]
    assert RP.as_tuples(RP.expected_repeats([b"AAAA", b"ACACACAC"], RP.single(2, 2) + ())) == [(1, 0, 8, 0b0100, 2)]     # AAAA is no row of period 2
    assert RP.as_tuples(RP.expected_repeats([b"ACACACA"], RP.single(2, 2), 7, True)) == [] and RP.as_tuples(RP.expected_repeats([b"ACACACA"], RP.single(2, 2), 6, True)) == [(0, 0, 6, 4, 2)]


def test_the_model_agrees_with_the_brute_walk_on_the_planned_texts(planned):
    for c in planned.values():
        big = len(c.text) > 300000
        for spec, m, whole in ((RP.MISA, 1, False), (RP.single(16, 2), 1, True)) if big else ((RP.ALL2, 1, False), (RP.ALL3, 12, True), (RP.MISA, 1, False)):
            assert RP.as_tuples(RP.expected_repeats(c.lines, spec, m, whole)) == RP.brute_repeats(c.lines, spec, m, whole), (c.name, spec)
        for first, count in ((1, 2), (len(c.lines) // 2, None)):
            if c.lines:
                assert RP.as_tuples(RP.expected_repeats(c.lines, RP.ALL3, 1, False, first, count)) == RP.brute_repeats(c.lines, RP.ALL3, 1, False, first, count)


# ---- 2. the texts ----------------------------------------------------------------------------------------------------------------------
def test_every_plant_is_found_with_its_bounds(planned):
    for c in planned.values():
        rows = RP.expected_repeats(c.lines, RP.ALL2)
        have = {t[:3] + (t[4],) for t in RP.as_tuples(rows)}
        assert all(x in have for x in c.plants), (c.name, [x for x in c.plants if x not in have][:5])
        assert not any(x in have for x in c.absent), c.name
        for r, b, e, p in c.absent:                                                 # ... also when the shorter period is not searched
            alone = {t[:3] for t in RP.as_tuples(RP.expected_repeats(c.lines, RP.single(p, 2), 1, False, r, 1))}
            assert (r, b, e) not in alone
    assert len(planned["seams"].plants) > 690 and len(planned["lengths"].plants) > 70 and len(planned["overlap"].plants) > 100 and len(planned["overlap"].absent) >= 20


def test_the_seams_text_covers_every_offset(planned):
    S = planned["seams"].seams
    cov = S.coverage(RP.expected_repeats(planned["seams"].lines, RP.ALL2))
    print("\nseam kind x which end x period: the offsets at which the planted repeat's first / last base lies")
    for kind in RP.SEAM_KINDS:
        for side in ("first", "last"):
            for p in RP.PERIODS:
                print("%-7s %-5s p=%-2d %s" % (kind, side, p, sorted(cov.get((kind, side, p), ()))))
    for kind in ("lane", "load32", "tile", "record"):
        for side in ("first", "last"):
            for p in RP.PERIODS:
                assert cov.get((kind, side, p)) == set(range(-(p + 1), 3)), (kind, side, p)      # no cell is empty
    # a text of this size has two block seams and one end (the plan's docstring): the cells they can have
    assert sum(len(v) for k, v in cov.items() if k[0] == "block") == 2 and cov[("end", "last", 16)] == {-1}
    assert len(S.stream) == S.TOTAL and S.TOTAL % 2 == 1 and sum(1 for r in S.records if not r) == 6
    assert all(x % 4096 == 0 for x in S.seams["tile"]) and set(S.seams["block"]) <= set(S.seams["tile"])
    assert {x % 2 for x in S.seams["record"]} == {0, 1}
    # a plant across a record's end is two parts; at period 1 both can be rows
    assert any(len(S.rows_of(a, b, p)) == 2 for kind, _, p, _, _, a, b in S.plants if kind == "record")


def test_the_other_texts(planned):
    L = planned["lengths"]
    lens = {(p, e - b) for _, b, e, p in L.plants}
    for p in (1, 2, 3, 4, 7, 16):
        assert {(p, n) for n in (2 * p, 2 * p + 1, 63, 64, 65, 4095, 4096, 4097, 13001) if n >= 2 * p} <= lens
        assert any(q == p and e - b == 2 * p - 1 for _, b, e, q in L.absent) or p == 1
        assert any(len(r) == n for r in L.records for n in (p, 2 * p - 1, 2 * p, 2 * p + 1))
    recs = L.records
    assert recs[0] == "" and recs[-1] == recs[-2] == "" and sum(len(r) for r in recs) % 2 == 1
    rows = RP.as_tuples(RP.expected_repeats(L.lines, RP.ALL2))
    pairs = 0                                                                       # a repeat up to a record's last base, one with the same motif from base 0 of the next non-empty record
    for r, b, e, m, p in rows:
        if e == len(recs[r]) and e - b > 3 * p:
            n = next((k for k in range(r + 1, len(recs)) if recs[k]), None)
            pairs += n is not None and n > r + 1 and any(x[0] == n and x[1] == 0 and x[4] == p and RP.class_of(RP.motif_text(x[3], p)) == RP.class_of(RP.motif_text(m, p)) for x in rows)
    assert pairs >= 6
    O = planned["overlap"]
    rows = RP.as_tuples(RP.expected_repeats(O.lines, RP.ALL2))
    shared = {(p, e - b2) for (r, b, e, _, p), (r2, b2, e2, _, p2) in itertools.combinations(rows, 2) if r == r2 and p == p2 and b < b2 < e < e2}
    for p in (2, 3, 4, 5, 7, 8, 15, 16):
        assert {(p, k) for k in range(1, p)} <= shared, p                            # same-period repeats that share 1 .. p - 1 bases
    assert any(sum(1 for y in rows if y[:2] == x[:2]) >= 2 for x in rows)            # several periods begin on one base
    assert {p for _, _, _, p in O.absent} == {2, 4, 6, 8, 9, 12, 15, 16}
    U, R = planned["unknown"], planned["rna"]
    assert sum(len(r) for r in U.records) % 2 == 1 and R.seq_type == 1 and b"U" in R.text and b"T" not in R.text.split(b"\n", 1)[1].replace(b"some words", b"")
    assert RP.expected_repeats(U.lines, RP.ALL2).tobytes() == RP.expected_repeats(R.lines, RP.ALL2).tobytes()
    for ch in "NR-":
        assert any(ch in r for r in U.records)
    assert any(r != r.upper() and r != r.lower() for r in U.records)
    F = planned["fastq"]
    assert sorted({len(r) for r in F.records}) == list(range(41)) + [150] and F.well_formed and F.own_text != F.text
    D = planned["dense"]
    d = RP.expected_repeats(D.lines, RP.ALL2)
    assert len(d) > 50000 and set("".join(D.records[:4])) == {"A", "C"}
    for r in (4, 5, 7):
        assert [t[1:] for t in RP.as_tuples(d) if t[0] == r] == [(0, len(D.records[r]), "ACGT".index(D.records[r][0].upper()), 1)]      # one letter: one row, of period 1
    assert planned["no_records"].text == b""
    for c in planned.values():
        assert len(c.text) <= 720 * 1024 and (not c.text or len(c.text) >= 6 * 1024)


# ---- 3. the host-only C-ABI -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,want", RP.PARSE_TABLE)
def test_parse_repeat_spec_against_the_table(text, want):
    from naf_amd import capi
    if want is None:
        with pytest.raises(ValueError):
            capi.parse_repeat_spec(text)
    else:
        assert capi.parse_repeat_spec(text) == want
        assert capi.parse_repeat_spec(text.encode()) == want
        assert text == "misa" or sorted(text.split(",")) == sorted(RP.spec_text(want).split(","))


def test_parse_repeat_spec_rejects_null_and_leaves_the_spec():
    from naf_amd import capi
    lib = capi.load()
    sp = capi.RepeatSpec((C.c_uint32 * 16)(*[7] * 16))
    assert lib.naf_gpu_parse_repeat_spec(None, C.byref(sp)) != 0 and lib.naf_gpu_parse_repeat_spec(b"misa", None) != 0
    for bad in (b"", b"1-1", b"1-10,", b"1-10,1-10"):
        assert lib.naf_gpu_parse_repeat_spec(bad, C.byref(sp)) == -8 and list(sp.min_copies) == [7] * 16
    with pytest.raises(ValueError):
        capi.parse_repeat_spec("1-10\0,2-6")
    assert RP.MISA == tuple(capi.parse_repeat_spec("misa"))


def test_repeat_class_of_every_motif_of_periods_1_to_6():
    from naf_amd import capi
    n = 0
    for p in range(1, 7):
        for letters in itertools.product("ACGT", repeat=p):
            word = "".join(letters)
            motif = sum("ACGT".index(ch) << (2 * i) for i, ch in enumerate(word))
            rc = word[::-1].translate(str.maketrans("ACGT", "TGCA"))
            want = min([word[k:] + word[:k] for k in range(p)] + [rc[k:] + rc[:k] for k in range(p)])       # a plain minimum over the 2p strings
            cls = capi.repeat_class(motif, p)
            assert capi.repeat_motif_text(cls, p) == want, word
            assert capi.repeat_motif_text(motif, p) == word and capi.repeat_motif_text(motif, p, rna=True) == word.replace("T", "U")
            n += 1
    assert n == 4 + 16 + 64 + 256 + 1024 + 4096
    assert {capi.repeat_motif_text(capi.repeat_class(sum("ACGT".index(ch) << (2 * i) for i, ch in enumerate(w)), 2), 2) for w in ("CA", "AC", "TG", "GT")} == {"AC"}
    assert capi.repeat_motif_text(capi.repeat_class(0xFFFFFFFF, 16), 16) == "A" * 16
    for motif, p in ((0, 0), (0, 17), (4, 1), (1 << 12, 6)):
        with pytest.raises(ValueError):
            capi.repeat_class(motif, p)
    assert capi.load().naf_gpu_repeat_class(0, 1, None) != 0
    with pytest.raises(ValueError):
        capi.repeat_motif_text(16, 2)


def test_repeats_are_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_parse_repeat_spec", "naf_gpu_repeat_class", "naf_gpu_unnaf_repeats_count", "naf_gpu_unnaf_repeats"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert C.sizeof(capi.Repeat) == 32 and np.dtype(capi.REPEAT_DTYPE).itemsize == 32 and capi.REPEAT_BYTES == 32 and C.sizeof(capi.RepeatSpec) == 64
    assert capi.REPEAT_DTYPE == RP.REPEAT_DTYPE and capi.REPEATS_WHOLE_UNITS == 1
    assert [f[0] for f in capi.Repeat._fields_] == ["record", "begin", "end", "motif", "period", "reserved"] and capi.Repeat.motif.offset == 24 and capi.Repeat.period.offset == 28
    assert np.dtype(capi.REPEAT_DTYPE).fields["period"][1] == 28
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    for word in ("naf_gpu_repeat;", "naf_gpu_repeat_spec;", "NAF_GPU_REPEATS_WHOLE_UNITS = 1", "naf_gpu_parse_repeat_spec", "naf_gpu_repeat_class", "naf_gpu_unnaf_repeats_count",
                 "NAF_GPU_REPEATS_PIECE", "ACACAGAGAG", "[repeats] rows R candidates K periods P pieces N sequence bytes decoded X of Y"):
        assert word in header, word


def test_repeats_to_segments():
    from naf_amd import capi
    rows = np.zeros(3, dtype=capi.REPEAT_DTYPE)
    rows["record"], rows["begin"], rows["end"], rows["period"] = [3, 4, 4], [10, 2, 8], [13, 6, 10], [1, 2, 1]
    assert capi.repeats_to_segments(rows) == [(3, 10, 13), (4, 2, 6), (4, 8, 10)]
    assert capi.repeats_to_segments(rows, flank=5, lengths=[0, 0, 0, 15, 9]) == [(3, 5, 15), (4, 0, 9), (4, 3, 9)]
    assert capi.repeats_to_segments(rows, flank=2) == [(3, 8, 15), (4, 0, 8), (4, 6, 12)]
    assert capi.repeats_to_segments(rows[:0]) == []


# ---- 4. the command line, before the device is opened -----------------------------------------------------------------------------------
REFUSED = [(["--repeats", "misa", "--locate", "NGG"], b"--repeats and --locate can't be used together"),
           (["--repeats", "misa", "--composition"], b"--repeats and --composition can't be used together"),
           (["--repeats", "misa", "--quality"], b"--repeats and --quality can't be used together"),
           (["--repeats", "misa", "--runs", "N"], b"--repeats and --runs can't be used together"),
           (["--masked-runs", "--repeats", "misa"], b"--repeats and --masked-runs can't be used together"),
           (["--repeats", "misa", "--kmers", "3"], b"--repeats and --kmers can't be used together"),
           (["--repeats", "misa", "--orfs"], b"--repeats and --orfs can't be used together"),
           (["--translate", "--repeats", "misa"], b"--repeats and --translate can't be used together"),
           (["--repeats", "misa", "--fasta"], b"no output type"), (["--seq", "--repeats", "misa"], b"no output type"), (["--repeats", "1-10", "--ids"], b"no output type"),
           (["--repeats", "misa", "--region", "x", "--revcomp"], b"--revcomp can't"), (["--repeats", "misa", "--rc-region", "x"], b"--rc-region can't"),
           (["--repeats", "misa", "--records", "1-2", "--records", "3-4"], b"one --records or one --region"),
           (["--repeats", "misa", "--region", "x", "--records", "1"], b"one --records or one --region"),
           (["--repeats", "misa", "--region", "x:1-5"], b"whole sequence"),
           (["--min-repeat", "12"], b"--min-repeat can be used only with --repeats"), (["--whole-units"], b"--whole-units can be used only with --repeats"),
           (["--runs", "N", "--whole-units"], b"--whole-units can be used only with --repeats"),
           (["--repeats", "misa", "--repeats", "1-10"], b"only one --repeats"),
           (["--repeats", ""], b"--repeats parameter"), (["--repeats", "1-1"], b"--repeats parameter"), (["--repeats", "17-2"], b"--repeats parameter"),
           (["--repeats", "1-10,"], b"--repeats parameter"), (["--repeats", "1-10, 2-6"], b"--repeats parameter"), (["--repeats", "1-10,1-12"], b"--repeats parameter"),
           (["--repeats", "misa", "--min-repeat", "0"], b"--min-repeat parameter"), (["--repeats", "misa", "--min-repeat", "x"], b"--min-repeat parameter")]


@pytest.mark.parametrize("args,word", REFUSED)
def test_repeats_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr      # the check of this option, not the one for an option nobody knows


@pytest.mark.parametrize("args", [["--repeats"], ["--repeats", "misa", "--min-repeat"]])
def test_an_option_without_its_value_is_a_usage_error(args):
    p = subprocess.run([os.path.join(BIN, "unnaf"), os.path.join(GOLDEN, "naf", "acgt_10k.naf"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"unknown or incomplete argument \"%s\"" % args[-1].encode() in p.stderr


def test_help_gains_the_three_lines_behind_code_table():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--repeats" not in head and b"--min-repeat" not in head and b"--whole-units" not in head
    at = [tail.index(line) for line in (b"\n  --code-table ", b"\n  --repeats SPEC ", b"\n  --min-repeat N ", b"\n  --whole-units ")]
    assert at == sorted(at)


# ---- 5. the texts decode to what the plan says ------------------------------------------------------------------------------------------
def test_the_planned_texts_through_the_oracle(oracle, planned):
    for c in planned.values():
        naf = oracle.ennaf(c.text, c.seq_type, well_formed=c.well_formed)
        h = oracle.parse_naf(naf)
        lines = RP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), h.n_sequences)
        assert [x.decode("latin1") for x in lines] == c.records, c.name
