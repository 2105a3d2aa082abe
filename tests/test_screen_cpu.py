"""CPU tests of k-mer screening: the plan's model against its brute force, the plants against their claims and their places, the
coverage table, the references, the bindings and what unnaf refuses on the command line before the device is opened.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import screen_plan as SP
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "naf_amd", "bin")
SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
SMALL_TEXT = 20000                                                                       # bases a text may have for the triple loop over all of it


@pytest.fixture(scope="module")
def cases():
    return SP.planned(SEED)


def against(loop, records, ref_records, K, forward_only, bounds, where, only=None):
    """the model's rows and totals against a loop over str; only: the reads whose hits are compared (None: all)"""
    rows, total = SP.model(SP.Stream(records), SP.Stream(ref_records), K, forward_only=forward_only, bounds=bounds)
    if only is not None:
        hits, _, ref_pos, ref_kmers = loop([records[r] for r in only], ref_records, K, forward_only, [bounds[r] for r in only] if bounds else None)
        assert [int(rows[r]["hits"]) for r in only] == [h or 0 for h in hits], where
        assert total[10:] == (ref_pos, ref_kmers), where
        return rows, total
    hits, kmers, ref_pos, ref_kmers = loop(records, ref_records, K, forward_only, bounds)
    assert len(rows) == len(records) == len(hits)
    considered = matched = bases = kept_bases = 0
    for r, x in enumerate(rows):
        b, e, f = bounds[r] if bounds is not None else (0, len(records[r]), SP.KEPT)
        assert (int(x["record"]), int(x["begin"]), int(x["end"]), int(x["reserved"])) == (r, b, e, 0), (where, r)
        if hits[r] is None:
            assert (int(x["hits"]), int(x["flags"])) == (0, f), (where, r)
            continue
        assert int(x["hits"]) == hits[r], (where, r, hits[r], x)
        assert int(x["flags"]) == (SP.MATCHED if hits[r] else SP.KEPT) | (f & SP.CLIPPED), (where, r)
        considered += 1; matched += hits[r] > 0; bases += e - b; kept_bases += 0 if hits[r] else e - b
    assert total == (len(records), considered, matched, considered - matched, bases, kept_bases, kmers, sum(h or 0 for h in hits), len(ref_records), sum(len(r) for r in ref_records),
                     ref_pos, ref_kmers), where
    return rows, total


# ---- 1. the model against the loops over str ------------------------------------------------------------------------------------------
def test_the_model_agrees_with_the_triple_loop_on_the_small_planted_texts(cases):
    n = 0
    for c in cases:
        if sum(len(r) for r in c.records) > SMALL_TEXT:
            continue
        for K in c.ks:
            for fwd in (False, True):
                against(SP.brute, c.records, c.ref.records, K, fwd, None, (c.name, K, fwd))
                n += 1
    assert n > 200


def test_the_model_agrees_with_the_loops_on_the_long_planted_texts(cases):
    """every start of every read by slices; the reads that hold a plant -- but the longest -- letter by letter as well"""
    n = 0
    for c in cases:
        if sum(len(r) for r in c.records) <= SMALL_TEXT:
            continue
        for K in c.ks:
            for fwd in (False, True):
                against(SP.brute_slices, c.records, c.ref.records, K, fwd, None, (c.name, K, fwd))
            for bs in c.bsets:
                against(SP.brute_slices, c.records, c.ref.records, K, bool(K % 2), c.bounds(bs), (c.name, K, bs))
            held = [p.rec for p in c.plants if len(c.records[p.rec]) < 5000][::3]
            against(SP.brute, c.records, c.ref.records, K, bool(K % 2), None, (c.name, K, "plants"), only=held)
            n += 1
    assert n >= len(SP.KS) + 1


def test_the_model_agrees_with_the_triple_loop_on_random_reads():
    recs, ref = SP.random_reads(SEED)
    rng = np.random.default_rng(5 + SEED)
    wins = [tuple(sorted(int(v) for v in rng.integers(0, len(r) + 1, 2))) + (int(rng.choice([1, 1, 1, 9, 2, 4, 6, 12, 0])),) for r in recs]
    seen = 0
    for K in (1, 2, 3, 5, 11, 16, 31):
        for fwd in (False, True):
            for bounds in (None, wins):
                rows, total = against(SP.brute, recs, ref, K, fwd, bounds, (K, fwd, bounds is not None))
                seen += total[7]
    assert seen > 1000 and set("".join(recs).upper()) >= set(SP.LP.CODES)
    assert SP.canon("acgu") == "ACGT" and SP.rc("AACG") == "CGTT"


def test_the_key_is_the_k_mer_index_with_the_first_base_most_significant():
    s = SP.Stream(["ACGTT", "GGA"])
    f, r, valid = s.keys(3)
    assert [int(x) for x in f[:3]] == [0b000110, 0b011011, 0b101111] and [int(x) for x in r[:3]] == [0b011011, 0b000110, 0b000001]      # ACG CGT GTT; their reverse complements CGT ACG AAC
    assert list(s.starts(3)) == [True, True, True, False, False, True]                   # no k-mer over the record's end
    assert SP._key_of("ACG", True) == 6 and SP._key_of("CGT", False) == 6 and SP._key_of("ANG", True) is None
    S, pos = SP.ref_set(SP.Stream(["ACGT", "ACG", "acgu", "NNNN", "AC"]), 3)
    assert [int(x) for x in S] == [6] and pos == 5                                       # ACG and CGT are one canonical key
    assert len(SP.ref_set(SP.Stream(["ACGT"]), 3, True)[0]) == 2
    assert int(SP.Stream(["T" * 31]).keys(31)[0][0]) == 2 ** 62 - 1                      # the largest key: all ones stays free


# ---- 2. the plants ---------------------------------------------------------------------------------------------------------------------
def test_every_plant_is_what_it_claims(cases):
    n = 0
    for c in cases:
        for K in c.ks:
            for fwd in (False, True):
                rows = SP.model(c.stream, c.ref.stream, K, forward_only=fwd)[0]
                assert SP.claims_hold(c, K, rows, fwd), (c.name, K, fwd)
            for bs in c.bsets:
                for fwd in (False, True):
                    rows = SP.model(c.stream, c.ref.stream, K, forward_only=fwd, bounds=c.bounds(bs))[0]
                    assert SP.claims_hold(c, K, rows, fwd, bs), (c.name, K, bs)
        n += len(c.plants)
    assert n > 2800
    # and the claims are no empty ones: a text's expected hits are there, strand plants hit on the other strand only
    for c in cases:
        if c.name.startswith("place") and c.ks[0] >= SP.EXACT_K:
            K = c.ks[0]
            want, want_fwd = c.expected(K), c.expected(K, True)
            assert sum(want) > sum(want_fwd) > 500 and sum(1 for p in c.plants if p.cell == "strand" and want[p.rec] == p.j + 1 and want_fwd[p.rec] == 0) == 2 * 3 * (K + 4)


def test_the_plants_lie_where_they_say(cases):
    n = 0
    for c in cases:
        total = int(c.starts[-1])
        for p in c.plants:
            if p.mark is None:
                continue
            seam = p.mark - p.off
            if p.kind == "lane":
                assert seam % SP.LANE == 0
            elif p.kind == "load":
                assert seam % SP.LANE == SP.LOAD
            elif p.kind == "tile":
                assert seam % SP.TILE == 0 and seam > 0
            elif p.kind == "block":
                assert seam % SP.BLOCK == 0 and seam > 0
            elif p.kind == "record":
                assert seam in set(c.starts[p.rec:p.rec + 3].tolist()), (c.name, p.off, p.j)
            else:
                assert seam == total and c.name.startswith("end")
            first, last = int(c.starts[p.rec]), int(c.starts[p.rec + 1])
            assert first <= p.mark < last or (p.kind == "record" and p.mark >= first), (c.name, p.kind, p.off)
            if p.cell in ("forward", "strand") and p.kind != "record" and p.kind != "stream":      # the plant's bases are there, at the mark
                s = SP.canon(c.records[p.rec])[p.mark - first:p.mark - first + p.K + p.j]
                big = SP.canon(c.ref.records[SP.BIG])
                assert len(s) == p.K + p.j and ((SP.rc(s) if p.cell == "strand" else s) in big), (c.name, p.kind, p.off)
            n += 1
    assert n > 2400


def test_every_cell_has_a_plant_and_every_offset_its_seams(cases):
    cov = SP.coverage(cases)
    print("%-14s" % "" + "".join("%8s" % k for k in SP.SEAM_KINDS))
    for cell in SP.CELLS:
        print("%-14s" % cell + "".join("%8d" % cov.get((cell, k), 0) for k in SP.SEAM_KINDS))
    for cell in SP.CELLS:
        assert sum(cov.get((cell, k), 0) for k in SP.SEAM_KINDS) > 0, cell
    for k in SP.SEAM_KINDS:
        assert cov.get(("forward", k), 0) > 0, k
    seen = {(p.K, p.j, p.kind, p.off, p.cell) for c in cases for p in c.plants if p.mark is not None}
    for K in SP.KS:
        for off in SP.offsets(K):
            for j in SP.JS:
                for kind in ("lane", "load", "tile", "record"):
                    assert (K, j, kind, off, "forward") in seen, (K, j, kind, off)
                for kind in ("lane", "load"):
                    assert (K, j, kind, off, "strand") in seen, (K, j, kind, off)
            if off < 0:
                for j in SP.JS:
                    assert (K, j, "stream", off, "forward") in seen, (K, j, off)
        assert sum(1 for s in seen if s[0] == K and s[2] == "block") >= 3
    assert {s[3] for s in seen if s[0] in (1, 2) and s[2] == "block" and s[4] == "forward"} >= set(SP.offsets(1))
    assert {s[1] for s in seen if s[2] == "block"} == set(SP.JS) == {s[1] for s in seen if s[2] == "stream"}
    # the lengths, the one-base reads and the size of the texts
    for c in cases:
        if c.name.startswith("place"):
            K = c.ks[0]
            assert {len(r) for r in c.records} >= {0, 1, 2, 3, K - 1, K, K + 1, 63, 64, 65, 150, 4095, 4096, 4097, 13001, 300000}, c.name
            subs = [p for p in c.plants if p.cell == "substitution"]
            assert {p.off for p in subs} == {0, K + 4} | ({K - 17, K - 16} if K >= 17 else set()) and len(subs) == 4 * len({p.off for p in subs})
            assert {p.off for p in c.plants if p.cell == "window"} == {-1, 0, 1} and sum(1 for p in c.plants if p.cell == "dropped") == 3
            assert c.verdict_read is not None and c.expected(K)[c.verdict_read] == 6
            assert sum(1 for p in c.plants if p.cell == "spanning") == (K >= 2) and sum(1 for p in c.plants if p.cell == "near") == (4 if K > 1 else 0)
    ones = next(c for c in cases if c.name == "ones")
    assert len(ones.records) == 5000 and all(len(r) == 1 for r in ones.records)
    assert any(p.cell == "palindrome" for c in cases for p in c.plants if c.ks == (16,))
    sizes = [sum(len(r) for r in c.records) for c in cases]
    assert max(sizes) <= 1320000 and max(sizes) > 4 * SP.BLOCK


def test_the_references_are_what_the_plan_says(cases):
    ref = cases[0].ref
    for K in SP.KS:
        if K > SP.RUN_CAP:
            SP.check_reference(ref.records, K)
    with pytest.raises(AssertionError):
        SP.check_reference(["ACGT" + "ACCA" * 4 + "G"], 15)
    with pytest.raises(AssertionError):
        SP.check_reference(["TTGTGTGGGTTTGTGTc"], 15)
    lens = [len(r) for r in ref.records]
    assert set(lens) >= {n for K in SP.KS for n in (K - 1, K, K + 1)} and max(lens) > 3 * SP.TILE and lens[0] == 0
    assert any("N" in r for r in ref.records) and any(r != r.upper() for r in ref.records) and ref.records[SP.NEXT] == ref.records[SP.NEXT + 1]
    for K in (15, 27, 31):
        S, pos = SP.ref_set(ref.stream, K)
        assert 0 < len(S) < pos                                                          # every k-mer of one record is there twice
    assert ref.palindrome == SP.rc(ref.palindrome) and len(ref.palindrome) == 16
    by = {c.name: c for c in cases}
    assert by["dna_rna"].ref.seq_type == 1 and "U" in by["dna_rna"].ref.records[SP.BIG] and by["rna_dna"].seq_type == 1 and "U" in "".join(by["rna_dna"].records)
    assert by["dna_fastq"].ref.fmt == "fastq" and by["dna_fastq"].ref.text.startswith(b"@ref0 ")
    for K in by["dna_none"].ks:
        assert SP.ref_set(by["dna_none"].ref.stream, K) [1] == 0 and len(by["dna_none"].ref.records) == 4
    assert by["dna_empty"].ref.records == [] and by["dna_empty"].ref.text == b""
    for name in ("dna_rna", "rna_dna", "dna_fastq"):
        c = by[name]
        for K in c.ks:
            assert sum(c.expected(K)) > sum(c.expected(K, True)) > 0, name
    assert SP.model(by["chain"].stream, by["chain"].ref.stream, 27)[1][2] > 20            # the chain's reads: copies of the reference's reads match


def test_the_verdict_cells(cases):
    c = next(c for c in cases if c.name == "place27")
    r = c.verdict_read
    for min_hits, matched in ((5, True), (6, True), (7, False)):
        for keep in (False, True):
            rows, total = SP.model(c.stream, c.ref.stream, 27, min_hits=min_hits, keep_matched=keep)
            assert int(rows[r]["hits"]) == 6 and bool(int(rows[r]["flags"]) & SP.MATCHED) == matched and bool(int(rows[r]["flags"]) & SP.KEPT) == (matched == keep)
            assert total[3] == (total[2] if keep else total[1] - total[2]) and 0 < total[2] < total[1]


def test_the_table_lines():
    rows = np.zeros(5, dtype=SP.ROW_DTYPE)
    rows[0] = (0, 0, 5, 0, SP.KEPT, 0); rows[1] = (1, 1, 6, 3, SP.MATCHED | SP.CLIPPED, 0); rows[2] = (2, 0, 0, 0, SP.SHORT | SP.ERRORS, 0); rows[3] = (3, 0, 3, 0, SP.KEPT | SP.CLIPPED, 0)
    rows[4] = (4, 0, 4, 2, SP.MATCHED | SP.KEPT, 0)
    assert SP.table(rows, list("abcde"), [5, 7, 9, 3, 4]) == (b"#seq\tlength\tbegin\tend\thits\tstatus\na\t5\t0\t5\t0\tclean\nb\t7\t1\t6\t3\tmatched\nc\t9\t0\t0\t0\tshort,errors\n"
                                                              b"d\t3\t0\t3\t0\tclean\ne\t4\t0\t4\t2\tmatched\n")
    d = np.zeros(5, dtype=[("flags", "<u4")]); d["flags"] = [1, 32 | 8, 6, 16 | 8, 16]
    assert SP.table(rows, list("abcde"), [5, 7, 9, 3, 4], d).split(b"\n")[4:6] == [b"d\t3\t0\t3\t0\tduplicate", b"e\t4\t0\t4\t2\tduplicate"]
    assert SP.kept_segments(rows) == [(0, 0, 5), (3, 0, 3), (4, 0, 4)]
    for kind, size, at in (("trim", 40, 32), ("clip", 40, 36), ("dedup", 48, 40)):
        b = SP.bounds_rows([(1, 2, 9), (0, 7, 4)], kind, 5)
        assert len(b) == 2 * size and b[at:at + 4] == bytes([9, 0, 0, 0]) and b[size + at] == 4 and b[size:size + 8] == bytes([6] + [0] * 7)


# ---- 3. the C-ABI and the bindings ----------------------------------------------------------------------------------------------------
def test_screen_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    assert "naf_gpu_unnaf_screen" in capi.EXPORTS and hasattr(lib, "naf_gpu_unnaf_screen")
    assert np.dtype(capi.SCREEN_DTYPE).itemsize == 40 == capi.SCREEN_BYTES and capi.SCREEN_DTYPE == SP.ROW_DTYPE
    assert [np.dtype(capi.SCREEN_DTYPE).fields[f][1] for f in ("record", "begin", "end", "hits", "flags", "reserved")] == [0, 8, 16, 24, 32, 36]
    assert [np.dtype(capi.TRIM_DTYPE).fields[f][1] for f in ("record", "begin", "end", "ee", "flags", "reserved")] == [0, 8, 16, 24, 32, 36]      # a trim row with hits where ee stands
    assert C.sizeof(capi.ScreenOpts) == 24 and capi.ScreenOpts.min_hits.offset == 16 and capi.ScreenOpts.bounds_kind.offset == 8 and C.sizeof(capi.ScreenTotal) == 96
    assert [f[0] for f in capi.ScreenTotal._fields_] == ["reads", "considered", "matched", "kept", "bases", "kept_bases", "kmers", "hit_kmers", "ref_records", "ref_bases", "ref_positions", "ref_kmers"]
    assert (capi.SCREEN_MATCHED, capi.SCREEN_KEEP_MATCHED, capi.SCREEN_FORWARD_ONLY, capi.SCREEN_BOUNDS_TRIM, capi.SCREEN_BOUNDS_CLIP, capi.SCREEN_BOUNDS_DEDUP, capi.SCREEN_MAX_K) == (32, 1, 2, 0, 1, 2, 31)
    assert SP.MATCHED == 32 and capi.TRIM_KEPT == SP.KEPT and capi.CLIP_CLIPPED == SP.CLIPPED and capi.DEDUP_DUPLICATE == SP.DUPLICATE
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    for word in ("naf_gpu_screen_row;", "naf_gpu_screen_opts;", "naf_gpu_screen_total;", "NAF_GPU_SCREEN_MATCHED = 32", "NAF_GPU_SCREEN_KEEP_MATCHED = 1, NAF_GPU_SCREEN_FORWARD_ONLY = 2",
                 "NAF_GPU_SCREEN_BOUNDS_TRIM = 0, NAF_GPU_SCREEN_BOUNDS_CLIP = 1, NAF_GPU_SCREEN_BOUNDS_DEDUP = 2", "NAF_GPU_SCREEN_HASH_BITS", "NAF_GPU_SCREEN_FILTER_BITS", "NAF_GPU_SCREEN_PIECE",
                 "reads cannot be screened in %s sequences", "[screen] k K ref records R ref kmers U of V slots S filter bits F reads N considered C matched M filtered Q probed P sequence"):
        assert word in header, word


def test_screen_to_segments():
    from naf_amd import capi
    rows = np.zeros(5, dtype=capi.SCREEN_DTYPE)
    rows["record"], rows["begin"], rows["end"], rows["flags"] = [3, 4, 5, 6, 7], [1, 0, 2, 0, 4], [9, 0, 7, 5, 8], [1, 32, 1 | 8, 32 | 1, 6]
    assert capi.screen_to_segments(rows) == [(3, 1, 9), (5, 2, 7), (6, 0, 5)] == SP.kept_segments(rows) and capi.screen_to_segments(rows[:0]) == []


# ---- 4. the command line, before the device is opened ---------------------------------------------------------------------------------
A13 = "AGATCGGAAGAGC"
REF = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
REFUSED = [(["--screen-k", "21"], b"--screen-k can be used only with --screen"), (["--min-hits", "2"], b"--min-hits can be used only with --screen"),
           (["--keep-matched"], b"--keep-matched can be used only with --screen"), (["--forward-only", "--dedup"], b"--forward-only can be used only with --screen"),
           (["--screen-table", "--trim", "20"], b"--screen-table can be used only with --screen"),
           (["--screen", REF, "--screen-k", "0"], b"can't parse the value of --screen-k parameter (a k-mer length of 1 to 31)"),
           (["--screen", REF, "--screen-k", "32"], b"can't parse the value of --screen-k parameter (a k-mer length of 1 to 31)"),
           (["--screen", REF, "--screen-k", "x"], b"can't parse the value of --screen-k parameter"),
           (["--screen", REF, "--min-hits", "0"], b"can't parse the value of --min-hits parameter (a positive number of k-mers)"),
           (["--screen", REF, "--screen", REF], b"only one --screen reference can be given"), (["--screen", ""], b"empty --screen parameter"),
           (["--screen", REF, "--locate", "NGG"], b"--screen and --locate can't be used together"), (["--composition", "--screen", REF], b"--screen and --composition can't be used together"),
           (["--screen", REF, "--quality"], b"--screen and --quality can't be used together"), (["--screen", REF, "--kmers", "3"], b"--screen and --kmers can't be used together"),
           (["--screen", REF, "--orfs"], b"--screen and --orfs can't be used together"), (["--translate", "--screen", REF], b"--screen and --translate can't be used together"),
           (["--screen", REF, "--repeats", "misa"], b"--screen and --repeats can't be used together"), (["--screen", REF, "--runs", "N"], b"--screen and --runs can't be used together"),
           (["--screen", REF, "--trim", "20", "--trim-table"], b"--trim-table can't be used with --screen"), (["--screen", REF, "--adapter", A13, "--clip-table"], b"--clip-table can't be used with --screen"),
           (["--screen", REF, "--dedup", "--dedup-table"], b"--dedup-table can't be used with --screen"),
           (["--screen", REF, "--region", "x", "--revcomp"], b"--revcomp can't"), (["--screen", REF, "--rc-region", "x"], b"--rc-region can't"),
           (["--screen", REF, "--region", "x:1-5"], b"whole sequence"), (["--screen", REF, "--records", "1-2", "--records", "3-4"], b"one --records or one --region"),
           (["--screen", REF, "--screen-table", "--fastq"], b"--screen writes a table: no output type"), (["--seq", "--screen", REF, "--screen-table"], b"--screen writes a table: no output type"),
           (["--screen", REF, "--4bit"], b"no other output type"), (["--ids", "--screen", REF], b"no other output type"),
           (["--screen", REF, "--max-ee", "1"], b"--max-ee can be used only with --trim"), (["--screen", REF, "--min-length", "12"], b"--min-length can be used only with --trim or --adapter"),
           (["--screen", REF, "--either-strand"], b"--either-strand can be used only with --dedup"),
           (["--screen", REF, "--trim", "20"], b"the archive has no quality section"), (["--screen", REF, "--fastq"], b"input has no qualities"),
           (["--screen", os.path.join(GOLDEN, "naf", "no_such_file.naf")], b"can't open the --screen reference file"),
           (["--screen", os.path.join(GOLDEN, "naf", "protein_small.naf")], b"reads cannot be screened in protein sequences")]


@pytest.mark.parametrize("args,word", REFUSED)
def test_screen_arguments_are_checked_on_the_command_line(args, word):
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c", REF], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr


def test_protein_archives_are_refused():
    for args in (["--screen", REF], ["--screen", REF, "--screen-table", "--keep-matched"]):
        p = subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c", os.path.join(GOLDEN, "naf", "protein_small.naf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"unnaf error: reads cannot be screened in protein sequences\n"


ACCEPTED = [["--screen", REF], ["--screen", REF, "--screen-k", "31", "--min-hits", "3", "--keep-matched", "--forward-only", "--fasta", "--line-length", "60"], ["--screen", REF, "--screen-table"],
            ["--screen", REF, "--screen-table", "--dedup", "--either-strand", "--region", "x"], ["--screen", REF, "--sequences", "--records", "2-3"], ["--screen", REF, "--seq", "--dedup"],
            ["--screen", REF, "--trim", "20", "--max-ee", "0.5", "--min-length", "30", "--fastq"], ["--adapter", A13, "--screen", REF, "--min-overlap", "5", "--adapter-errors", "0.2"],
            ["--trim", "none", "--adapter", A13, "--adapter", "ACGT", "--dedup", "--screen", REF, "--screen-table", "--either-strand", "--screen-k", "1"]]


@pytest.mark.parametrize("args", ACCEPTED)
def test_accepted_command_lines_reach_the_input(args):
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, os.path.join(GOLDEN, "naf", "no_such_file.naf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"unnaf error: can't open input file\n"


def test_help_gains_the_block_in_front_of_the_dedup_options():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    text = p.stderr
    at = [text.index(line) for line in (b"\n  --whole-units ", b"\nOptions for screening reads against a reference", b"\n  --screen REF.naf ", b"\n  --screen-k K ", b"\n  --min-hits N ", b"\n  --keep-matched ",
                                        b"\n  --forward-only ", b"\n  --screen-table ", b"\nOptions for collapsing duplicate reads", b"\n  --dedup  ", b"\nOptions for clipping adapters")]
    assert at == sorted(at) and text.endswith(b"short,errors)\n")
    assert text.count(b"\n  --screen ") == 1 and text.count(b"\n  --screen-table ") == 1 and text.count(b"\n  --screen-k ") == 1
