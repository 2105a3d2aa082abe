"""CPU tests of the translation: the plan's own claims (translate_plan.py), the host-only parts of the C-ABI (genetic codes, the codon table,
frames to segments) and the checks unnaf makes before it opens the device.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import translate_plan as TP
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "naf_amd", "bin")
E_ARG = -8


@pytest.fixture(scope="module")
def planned():
    return TP.planned(TP.SEED)


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------------
def test_the_plants_cover_every_seam_offset_and_strand(planned, capsys):
    cov = TP.coverage(planned)
    cells = TP.coverage_cells()
    with capsys.disabled():
        print("\n  translate plan, seed %d: kind / d / strand -> texts" % TP.SEED)
        for cell in cells:
            print("    %-7s %+d %d  %s" % (cell + (" ".join(sorted(set(cov.get(cell, [])))) or "-",)))
    assert len(cells) == 3 * 5 * 2 + 2 * 6 * 2 + 3 * 2
    for cell in cells:
        assert cov.get(cell), cell
    assert set(cov) == set(cells)


@pytest.mark.parametrize("seed", TP.SEEDS)
def test_every_seed_covers_the_table(seed):
    cov = TP.coverage(TP.planned(seed))
    assert all(cov.get(cell) for cell in TP.coverage_cells())


def test_the_background_translates_to_no_m(planned):
    """every M of a planted call is a plant: the background holds no T"""
    for c in planned:
        if c.name in ("output", "blocks", "far", "records") or c.name.startswith("end"):
            plants = sum(len(call.plants) for call in c.calls) + len(getattr(c, "src_plants", ()))       # one T each, or none where only "A" or "C" fits
            assert plants > 0 and sum(r.count("T") for r in c.records) <= plants, c.name


def test_the_planned_calls_ask_what_the_issue_lists(planned):
    by = {c.name: c for c in planned}
    assert {c.line_length for c in by["small"].calls} >= set(TP.LINE_LENGTHS) and {c.line_length for c in by["records"].calls} >= set(TP.LINE_LENGTHS)
    segs = by["small"].calls[0].segs
    assert {(b % 6, e - b, rc) for _, b, e, rc in segs if e != TP.WHOLE} == {(m, n, rc) for m in range(6) for n in TP.SMALL_SPANS for rc in (0, 1)}
    assert (0, 0, TP.WHOLE, 0) in segs and by["small"].records[0] == ""                 # the whole empty record
    every = by["small"].records[2]
    assert len(every) == 3 * 4096 and {every[i:i + 3] for i in range(0, len(every), 3)} == set(TP.triples(1))
    assert by["rna"].seq_type == 1 and "U" in by["rna"].records[2] and "T" not in by["rna"].records[2].upper()
    assert by["reads"].fastq and by["reads"].text.startswith(b"@")
    ones = next(c for c in by["records"].calls if c.tag == "ones")
    assert len(ones.segs) == 5000 and all(e - b == 3 for _, b, e, _ in ones.segs) and {rc for *_, rc in ones.segs} == {0, 1}
    mix = next(c for c in by["records"].calls if c.tag == "mix").segs
    assert len(mix) > len(set(mix))                                                 # repeats
    lo, hi = by["far"].far_bases[1], by["far"].far_bases[2]
    assert hi - lo > 2 * TP.BLOCK
    assert 300000 <= len(by["far"].stream) <= 1400000 and 300000 <= len(by["blocks"].stream) <= 1400000
    assert len(by["blocks"].stream) > 4 * TP.BLOCK


@pytest.mark.parametrize("code", [1, 2, 6, 22, TP.CUSTOM_ACGT])
def test_the_model_against_the_codon_walk(code):
    rng = np.random.default_rng(77 + TP.SEED)
    for n in (0, 1, 2, 3, 4, 5, 6, 47, 48, 49, 3000):
        s = "".join(np.asarray(list("ACGT" * 8 + TP.CODES))[rng.integers(0, 48, n)]) if n else ""
        assert TP.translate(s, code) == TP.translate_walk(s, code) and len(TP.translate(s, code)) == n // 3
    every = "".join(a + b + c for a in TP.CODES for b in TP.CODES for c in TP.CODES)
    assert TP.translate(every, code) == TP.translate_walk(every, code)


def test_a_few_translations_by_hand():
    assert TP.translate("ATGGCCTAA") == "MA*" and TP.translate("ATGGCCTAAT") == "MA*" and TP.translate("AT") == ""
    assert TP.translate("GCNTARTGANNN---A-CRAY") == "A**X-XX"                          # GCN A, TAR *, TGA *, NNN X, --- -, A-C X, RAY X (AAC N, AAT N, GAC D, GAT D)
    assert TP.translate("AAYTGA", 4) == "NW" and TP.translate("TAATAG", 6) == "QQ" and TP.translate("AGAAGG", 2) == "**" and TP.translate("YTG") == "L"
    assert TP.reading(b"aacgTu", 0, 6, 1) == "AACGTT" and TP.reading(b"AACGTN-R", 1, 8, 1) == "Y-NACGT"
    lines, ids, names = [b"ATGGCCTAAGG", b""], ["a", "b"], ["first one", ""]
    assert TP.protein_text(lines, ids, names, [0, (0, 0, TP.WHOLE, 1), (0, 1, 10, 0), (0, 2, 99, 1), 1, (1, 0, TP.WHOLE, 1), (0, 3, 5, 0)], 1, 2) == (
        b">a first one\nMA\n*\n" b">a/rc first one\nP*\nA\n" b">a:2-10\nWP\nK\n" b">a:3-11/rc\nP*\nA\n" b">b\n" b">b/rc\n" b">a:4-5\n")
    assert TP.protein_text(lines, ids, names, [0], 1, 0) == b">a first one\nMA*\n" and TP.protein_text(lines, ids, names, [0], 1, 3) == b">a first one\nMA*\n"


def test_frame_segments_of_the_plan_equal_the_table():
    for lengths, frames, records, want in TP.FRAMES_TABLE:
        assert TP.frame_segments(lengths, frames, records) == want


# ---- 2. genetic codes and the codon table ----------------------------------------------------------------------------------------------------
def test_the_two_spellings_of_the_standard_code_agree():
    assert len(TP.STANDARD_TCAG) == len(TP.STANDARD_ACGT) == 64
    perm = "".join(TP.STANDARD_TCAG[16 * "TCAG".index(a) + 4 * "TCAG".index(b) + "TCAG".index(c)] for a in "ACGT" for b in "ACGT" for c in "ACGT")
    assert perm == TP.STANDARD_ACGT == TP.letters_acgt(1)
    assert TP.STANDARD_ACGT[14] == "M" and [i for i, x in enumerate(TP.STANDARD_ACGT) if x == "*"] == [48, 50, 56]


@pytest.mark.parametrize("ncbi", sorted(TP.DIFFS))
def test_every_built_in_code_equals_its_difference_list(ncbi):
    from naf_amd import capi
    g = capi.genetic_code(ncbi)
    assert g.letters == TP.letters_acgt(ncbi)
    assert capi.genetic_code_stops(ncbi) == TP.stops_of(ncbi)
    assert capi.genetic_code(g) is g


def test_what_is_no_code_is_refused_and_nothing_is_written():
    from naf_amd import capi
    lib = capi.load()
    g = capi.GeneticCode()
    C.memset(C.byref(g), 0x5A, 64)
    for bad in TP.NOT_CODES:
        assert lib.naf_gpu_genetic_code_by_id(bad, C.byref(g)) == E_ARG and bytes(g.aa) == b"Z" * 64, bad
        with pytest.raises(ValueError):
            capi.genetic_code(bad)
    assert lib.naf_gpu_genetic_code_by_id(1, None) == E_ARG
    good = TP.STANDARD_ACGT.encode()
    for bad in (b"", good[:63], good + b"K", good[:10] + b"-" + good[11:], good[:10] + b"1" + good[11:], good[:63] + b" ", good[:5] + b"\xc4" + good[6:], good[:30] + b"." + good[31:]):
        assert lib.naf_gpu_genetic_code_parse(bad, C.byref(g)) == E_ARG and bytes(g.aa) == b"Z" * 64, bad
        with pytest.raises(ValueError):
            capi.genetic_code(bad)
    assert lib.naf_gpu_genetic_code_parse(None, C.byref(g)) == E_ARG and lib.naf_gpu_genetic_code_parse(good, None) == E_ARG
    for bad in (None, 1.5, True, good + b"\0"):
        with pytest.raises(ValueError):
            capi.genetic_code(bad)
    # stops and the table of what is no code (a struct nobody filled in), and of NULLs
    s, lut = C.c_uint64(5), (C.c_uint8 * 4096)(*([7] * 4096))
    z = capi.GeneticCode()
    assert lib.naf_gpu_genetic_code_stops(C.byref(z), C.byref(s)) == E_ARG and s.value == 5
    assert lib.naf_gpu_genetic_code_stops(None, C.byref(s)) == E_ARG and lib.naf_gpu_genetic_code_stops(C.byref(capi.genetic_code(1)), None) == E_ARG and s.value == 5
    assert lib.naf_gpu_codon_lut(C.byref(z), lut) == E_ARG and lib.naf_gpu_codon_lut(None, lut) == E_ARG and bytes(lut) == b"\x07" * 4096
    assert lib.naf_gpu_codon_lut(C.byref(capi.genetic_code(1)), None) == E_ARG


def test_a_parsed_code_takes_either_case():
    from naf_amd import capi
    assert capi.genetic_code(TP.STANDARD_ACGT.lower()).letters == TP.STANDARD_ACGT == capi.genetic_code(TP.STANDARD_ACGT.encode()).letters
    assert capi.genetic_code(TP.CUSTOM_ACGT).letters == TP.CUSTOM_ACGT and capi.genetic_code_stops(TP.CUSTOM_ACGT) == 1


@pytest.mark.parametrize("code", [1, 2, 6, TP.CUSTOM_ACGT], ids=["1", "2", "6", "parsed"])
def test_all_4096_entries_of_the_codon_table(code):
    from naf_amd import capi
    got, want = capi.codon_lut(code), TP.expected_lut(code)
    assert len(got) == 4096
    bad = [(i, TP.CODES[i >> 8] + TP.CODES[(i >> 4) & 15] + TP.CODES[i & 15], chr(got[i]), chr(want[i])) for i in range(4096) if got[i] != want[i]]
    assert not bad, bad[:8]
    assert chr(got[TP.lut_index("ATG")]) == "M" and got[0] == ord("-") and chr(got[TP.lut_index("GCN")]) == "A" and chr(got[TP.lut_index("A-C")]) == "X"
    assert set(got) <= set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ*-")


def test_the_stops_of_the_standard_code_are_the_orf_defaults():
    from naf_amd import capi
    assert capi.genetic_code_stops(1) == capi.parse_codon_set("TAA,TAG,TGA") == (1 << 48) | (1 << 50) | (1 << 56)
    assert capi.genetic_code_stops(4) == capi.parse_codon_set("TAA,TAG") and capi.genetic_code_stops(6) == capi.parse_codon_set("TGA")


def test_frames_to_segments_against_the_table():
    from naf_amd import capi
    assert capi.WHOLE == TP.WHOLE
    for lengths, frames, records, want in TP.FRAMES_TABLE:
        assert capi.frames_to_segments(lengths, frames, records) == want, (lengths, frames, records)
    for bad in (0, 4, -4, 6):
        with pytest.raises(ValueError):
            capi.frames_to_segments([10], [bad])


def test_translation_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_genetic_code_by_id", "naf_gpu_genetic_code_parse", "naf_gpu_genetic_code_stops", "naf_gpu_codon_lut", "naf_gpu_unnaf_translate_size", "naf_gpu_unnaf_translate"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert C.sizeof(capi.GeneticCode) == 64
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    for word in ("typedef struct { char aa[64]; } naf_gpu_genetic_code;", "naf_gpu_genetic_code_by_id", "naf_gpu_genetic_code_parse", "naf_gpu_genetic_code_stops",
                 "uint8_t lut[4096]", "naf_gpu_unnaf_translate_size", "[translate] segments S codons C ranges R sequence bytes decoded X of Y", "feed naf_gpu_unnaf_translate",
                 "(c0 << 8) | (c1 << 4) | c2", "ORFfinder"):
        assert word in header, word
    assert "Nothing is translated" not in header


# ---- 3. the command line, before the device is opened ---------------------------------------------------------------------------------------
TABLE = TP.STANDARD_ACGT


@pytest.mark.parametrize("args,word", [
    (["--translate", "--fasta"], b"--translate writes protein FASTA: no output type"), (["--seq", "--translate"], b"no output type"), (["--translate", "--ids"], b"no output type"),
    (["--translate", "--fastq"], b"no output type"), (["--translate", "--4bit"], b"no output type"),
    (["--translate", "--locate", "NGG"], b"--translate and --locate"), (["--composition", "--translate"], b"--translate and --composition"),
    (["--translate", "--quality"], b"--translate and --quality"), (["--translate", "--runs", "N"], b"--translate and --runs"),
    (["--masked-runs", "--translate"], b"--translate and --masked-runs"), (["--translate", "--kmers", "3"], b"--translate and --kmers"),
    (["--frame", "1"], b"--frame can be used only with --translate"), (["--code", "4"], b"--code can be used only with --translate"),
    (["--code-table", TABLE], b"--code-table can be used only with --translate"), (["--orfs", "--code", "4"], b"--code can be used only with --translate"),
    (["--orfs", "--frame", "2"], b"--frame can be used only with --translate"), (["--orfs", "--translate", "--frame", "1"], b"--frame can't be used with --orfs"),
    (["--translate", "--code", "1", "--code-table", TABLE], b"--code and --code-table"), (["--translate", "--code-table", TABLE, "--code", "2"], b"--code and --code-table"),
    (["--orfs", "--translate", "--code", "1", "--code-table", TABLE], b"--code and --code-table"),
    (["--translate", "--frame", ""], b"--frame parameter"), (["--translate", "--frame", "0"], b"--frame parameter"), (["--translate", "--frame", "4"], b"--frame parameter"),
    (["--translate", "--frame", "1,"], b"--frame parameter"), (["--translate", "--frame", ",1"], b"--frame parameter"), (["--translate", "--frame", "1,1"], b"--frame parameter"),
    (["--translate", "--frame", "1,6"], b"--frame parameter"), (["--translate", "--frame", "-4"], b"--frame parameter"), (["--translate", "--frame", "+1"], b"--frame parameter"),
    (["--translate", "--frame", "1 2"], b"--frame parameter"), (["--translate", "--frame", "12"], b"--frame parameter"), (["--translate", "--frame", "--1"], b"--frame parameter"),
    (["--translate", "--code", "0"], b"--code parameter"), (["--translate", "--code", "7"], b"--code parameter"), (["--translate", "--code", "x"], b"--code parameter"),
    (["--translate", "--code", ""], b"--code parameter"), (["--translate", "--code", "27"], b"--code parameter"), (["--translate", "--code", "-1"], b"--code parameter"),
    (["--translate", "--code", "99999999999"], b"--code parameter"),
    (["--translate", "--code-table", TABLE[:63]], b"--code-table parameter"), (["--translate", "--code-table", TABLE + "K"], b"--code-table parameter"),
    (["--translate", "--code-table", "-" + TABLE[1:]], b"--code-table parameter"), (["--translate", "--code-table", ""], b"--code-table parameter"),
    (["--translate", "--frame", "1", "--frame", "2"], b"only one --frame"), (["--translate", "--code", "1", "--code", "2"], b"only one --code"),
    (["--translate", "--code-table", TABLE, "--code-table", TABLE], b"only one --code-table"),
    (["--orfs", "--translate", "--fasta"], b"no output type"), (["--orfs", "--translate", "--code", "6", "--starts", "TGA"], b"share a codon"),
    (["--translate", "--revcomp"], b"--revcomp can be used only with"), (["--translate", "--strand", "+"], b"--strand can be used only with"),
    (["--translate", "--region", ":1-2"], b"--region parameter"), (["--translate", "--line-length", "x"], b"--line-length parameter")])
def test_translate_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1, p.stderr
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr


@pytest.mark.parametrize("opt", ["--frame", "--code", "--code-table"])
def test_a_translate_option_without_its_value_is_a_usage_error(opt):
    p = subprocess.run([os.path.join(BIN, "unnaf"), "-c", "--translate", opt], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and opt.encode() in p.stderr


def test_help_gains_the_translate_lines_behind_the_orf_lines():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--translate" not in head and b"--frame" not in head and b"--code" not in head
    for line in (b"\n  --translate ", b"\n  --frame LIST ", b"\n  --code N ", b"\n  --code-table LETTERS "):
        assert line in tail, line
    assert tail.index(b"\n  --split-unknown ") < tail.index(b"\n  --translate ") and tail.index(b"\n  --orfs ") < tail.index(b"\n  --translate ")
    assert b"1,2,3,-1,-2,-3" in tail and b"default 1" in tail


# ---- 4. the texts decode to what the plan says -----------------------------------------------------------------------------------------------
def test_the_planned_texts_through_the_oracle(oracle, planned):
    for c in planned:
        naf = oracle.ennaf(c.text, c.seq_type)
        h = oracle.parse_naf(naf)
        lines = TP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), h.n_sequences)
        assert [x.decode("latin1") for x in lines] == c.records, c.name
        ids = oracle.zstd_decompress(h.frame(naf, 0)).decode("latin1").split("\0")[:-1]
        names = oracle.zstd_decompress(h.frame(naf, 1)).decode("latin1").split("\0")[:-1]
        assert (ids, names) == (c.ids, c.names), c.name
        assert bool(h.flags & 1) == c.fastq
        if c.name == "blocks":
            assert (h.orig[oracle.SEQ] + 1) // 2 > 4 * 131072                         # four whole raw blocks of 128 KiB and a fifth
