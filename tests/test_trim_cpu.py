"""CPU tests of the trim table: the plan's model against its brute force and against its own associative combine, the planted reads and
their coverage table, the host-only C-ABI (naf_gpu_trim_limit), the bindings and what unnaf refuses on the command line before the device
is opened.  No GPU."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import trim_plan as TP
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "naf_amd", "bin")


@pytest.fixture(scope="module")
def planned():
    return {c.name: c for c in TP.planned(0)}


# ---- 1. the model against the brute force and against the combine ------------------------------------------------------------------------
def test_the_model_agrees_with_the_brute_force_on_the_planned_reads(planned):
    n = 0
    for c in planned.values():
        for q in c.quals:
            if len(q) <= 300 and n < 1500:                                            # (every plant but the long ones is among the first reads of `seams`; the filler is random)
                for name in ("Q2", "Q13", "Q20", "0.05", "none"):
                    assert TP.stretch(q, TP.LIMITS[name]) == TP.brute(q, TP.LIMITS[name]), (c.name, name, q)
                n += 1
    for c in planned.values():                                                          # every plant of up to 300 bytes, at every limit
        for (cls, cell), v in c.cells.items():
            for r, claim in v:
                if len(c.quals[r]) <= 300:
                    for name, limit in TP.LIMITS.items():
                        assert TP.stretch(c.quals[r], limit) == TP.brute(c.quals[r], limit), (cls, cell, name)


def test_the_model_agrees_with_the_brute_force_on_random_reads():
    rng = np.random.default_rng(20240)
    letters = np.frombuffer(b"#.58I", dtype=np.uint8)                                   # at DESIGN: far below, zero, +1, +1 (8 and 5 differ), far above... and `$`-free
    for k in range(2000):
        q = letters[rng.integers(0, 5, int(rng.integers(1, 40)))].tobytes()
        limit = TP.LIMITS[("Q13", "Q20", "Q2", "0.05")[k % 4]]
        assert TP.stretch(q, limit) == TP.brute(q, limit), (q, limit)


def test_the_combine_is_associative_and_gives_the_model():
    rng = np.random.default_rng(20241)
    letters = np.frombuffer(b"$.8I#", dtype=np.uint8)

    def tree(q, lo):
        if len(q) == 1 or (len(q) < 6 and rng.integers(0, 3) == 0):
            return TP.Summary.of(q, TP.DESIGN, lo)
        k = int(rng.integers(1, len(q)))
        return TP.combine(tree(q[:k], lo), tree(q[k:], lo + k))
    for _ in range(1500):
        q = letters[rng.integers(0, 5, int(rng.integers(1, 30)))].tobytes()
        assert tree(q, 0).answer() == TP.stretch(q, TP.DESIGN)[:2] == TP.brute(q, TP.DESIGN)[:2], q
    q = b"8" * 10 + b"$" + b"8" * 10                                                    # the equal dip: joined, whichever way it is cut
    for k in range(1, len(q)):
        assert TP.combine(TP.Summary.of(q[:k], TP.DESIGN), TP.Summary.of(q[k:], TP.DESIGN, k)).answer() == (0, 21)


# ---- 2. the plants and the coverage table -------------------------------------------------------------------------------------------------
def test_every_plant_has_the_stretch_it_claims(planned):
    n = 0
    for c in planned.values():
        for (cls, cell), v in c.cells.items():
            for r, claim in v:
                if claim is not None:
                    assert TP.stretch(c.quals[r], TP.DESIGN)[:2] == claim, (c.name, cls, cell)
                    n += 1
    assert n > 150


def test_every_cell_of_every_class_is_covered(planned):
    cov, want = TP.coverage(planned.values()), TP.expected_cells()
    for cls in TP.CLASSES:
        print("%-8s %3d cells: %s" % (cls, len(cov[cls]), " ".join("%s=%d" % (k.replace(" ", "_"), n) for k, n in sorted(cov[cls].items()))))
        assert cov[cls], cls
        for cell in want[cls]:
            assert cov[cls].get(cell, 0) > 0, (cls, cell)


def test_the_seam_plants_lie_where_they_say(planned):
    step = {"lane": (TP.LANE, 0), "load": (TP.LANE, TP.LOAD), "tile": (TP.TILE, 0), "block": (TP.BLOCK, 0)}
    for c, cls, cell, v in [(c, cls, cell, v) for c in planned.values() for (cls, cell), v in c.cells.items() if cls == "seam"]:
        kind, role, d = cell.split()
        for r, claim in v:
            at = int(c.starts[r]) + (claim[0] if role == "first" else claim[1] - 1)        # the stretch's first or last base, as a stream byte
            if kind in step:
                assert (at - int(d) - step[kind][1]) % step[kind][0] == 0 and at - int(d) > 0, cell
            elif kind == "record":
                assert at - int(d) in (int(c.starts[r]), int(c.starts[r + 1])), cell
            else:
                assert at - int(d) == int(c.starts[-1]), cell
    c = planned["seams"]
    assert len(c.ends) == 10 and all(0 < e < len(c.quals) for e in c.ends)
    for cell, shift in (("tile", (0, 9)),):
        got = sorted((int(c.starts[r]) + 40) % TP.TILE for r, _ in c.cells[("cross", cell)])
        assert got == list(shift)
    assert (int(c.starts[c.cells[("cross", "block")][0][0]]) + 21) % TP.BLOCK == 0
    L = planned["long"]
    for (cls, cell), v in L.cells.items():
        for r, (b, e) in v if cls == "long" else []:
            t_first, t_last = int(L.starts[r]) // TP.TILE, (int(L.starts[r + 1]) - 1) // TP.TILE
            tb, te = (int(L.starts[r]) + b) // TP.TILE, (int(L.starts[r]) + e - 1) // TP.TILE
            assert (tb, te) == (t_first, t_last) if cell.startswith("first") else (t_first < tb == te < t_last), cell
    assert set(len(q) for q in L.quals) >= {4095, 4096, 4097, 8193, 13001, 300000}
    assert all(sum(len(q) for q in c.quals) < 700000 for c in planned.values())


def test_the_filters_around_the_planted_stretch(planned):
    c = planned["seams"]
    q = c.quals[c.filters]
    b, e, ee = TP.stretch(q, TP.DESIGN)
    assert (b, e) == (5, 55) and ee == 50 * TP.ERR[ord("I")]
    for min_len, max_ee, want in ((49, ee + 1, TP.KEPT), (50, ee, TP.KEPT), (51, ee, TP.SHORT), (50, ee - 1, TP.ERRORS), (51, ee - 1, TP.SHORT | TP.ERRORS)):
        rows, total = TP.model([q], TP.DESIGN, min_len, max_ee)
        assert int(rows[0]["flags"]) == want and total == (1, int(want == TP.KEPT), 60, 50 * (want == TP.KEPT), ee * (want == TP.KEPT), int(bool(want & 2)), int(bool(want & 4)))
    rows, total = TP.model([b"", b"#"], TP.DESIGN)
    assert [int(x) for x in rows["flags"]] == [TP.SHORT, TP.SHORT] and total == (2, 0, 1, 0, 0, 2, 0)
    rows, total = TP.model([b"", b"#"], TP.NONE, 1, 0)
    assert [tuple(int(v) for v in x) for x in rows] == [(0, 0, 0, 0, TP.SHORT, 0), (1, 0, 1, TP.ERR[35], TP.ERRORS, 0)]


# ---- 3. the texts decode to what the plan says ------------------------------------------------------------------------------------------
def test_the_planned_texts_through_the_oracle(oracle, planned):
    for c in planned.values():
        naf = oracle.ennaf(c.text, well_formed=True)
        h = oracle.parse_naf(naf)
        text = oracle.unnaf(naf, oracle.MODE_FASTQ)
        assert h.n_sequences == len(c.quals) and TP.quals_of(text, h.n_sequences) == c.quals, c.name
        assert text == c.text
        segs = TP.kept_segments(TP.model(c.quals, TP.NONE)[0])
        assert TP.expected_text(text, h.n_sequences, segs, "fastq") == b"".join(b"@%s w\n%s\n+\n%s\n" % (c.ids[r].encode(), c.seqs[r], c.quals[r]) for r, _, _ in segs)
    assert TP.expected_text(b"@a x y\nACGTN\n+\n12345\n", 1, [(0, 1, 4)], "fastq", strands=[1]) == b"@a/rc x y\nACG\n+\n432\n"
    assert TP.expected_text(b"@a\nACGTN\n+\n12345\n", 1, [(0, 0, 5), (0, 2, 3)], "fasta", 2, strands=[1, 0]) == b">a/rc\nNA\nCG\nT\n>a\nG\n"
    assert TP.expected_text(b"@a\nACGTN\n+\n12345\n", 1, [(0, 0, 5)], "sequences") + TP.expected_text(b"@a\nACGTN\n+\n12345\n", 1, [(0, 1, 2)], "seq") == b"ACGTN\nC"


# ---- 4. the C-ABI and the bindings ------------------------------------------------------------------------------------------------------
def test_trim_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_trim_limit", "naf_gpu_unnaf_trim", "naf_gpu_unnaf_select_reads_size", "naf_gpu_unnaf_select_reads"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert C.sizeof(capi.TrimRow) == 40 == np.dtype(capi.TRIM_DTYPE).itemsize == capi.TRIM_BYTES and C.sizeof(capi.TrimOpts) == 24 and C.sizeof(capi.TrimTotal) == 56
    assert capi.TRIM_DTYPE == TP.ROW_DTYPE and (capi.TRIM_KEPT, capi.TRIM_SHORT, capi.TRIM_ERRORS, capi.TRIM_NONE) == (1, 2, 4, 2 ** 64 - 1)
    assert [f[0] for f in capi.TrimRow._fields_] == ["record", "begin", "end", "ee", "flags", "reserved"] and capi.TrimRow.ee.offset == 24 and capi.TrimRow.flags.offset == 32
    assert [f[0] for f in capi.TrimTotal._fields_] == ["reads", "kept", "bases", "kept_bases", "kept_ee", "n_short", "n_errors"]
    assert [f[0] for f in capi.TrimOpts._fields_] == ["limit", "min_len", "max_ee"] and np.dtype(capi.TRIM_DTYPE).fields["flags"][1] == 32
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    for word in ("naf_gpu_trim_row;", "naf_gpu_trim_opts;", "naf_gpu_trim_total;", "NAF_GPU_TRIM_NONE UINT64_MAX", "NAF_GPU_TRIM_KEPT = 1, NAF_GPU_TRIM_SHORT = 2, NAF_GPU_TRIM_ERRORS = 4",
                 "NAF_GPU_TRIM_PIECE", "smallest begin, then the largest end", "(end - begin) * limit",
                 "[trim] records R kept K pieces P quality bytes decoded X of Y open tiles T", "naf_gpu_unnaf_select_reads_size"):
        assert word in header, word


def test_trim_limit():
    from naf_amd import capi
    assert capi.quality_error_table() == TP.ERR
    for q in range(94):
        assert capi.trim_limit(q) == TP.ERR[33 + q]
    assert capi.trim_limit(0) == 2 ** 32 and capi.trim_limit(93) == 2 == round(2 ** 32 * 10 ** -9.3)
    for name, limit in TP.LIMITS.items():
        if name.startswith("Q"):
            assert capi.trim_limit(int(name[1:])) == limit
    for bad in (94, 255, 2 ** 32 - 1, -1):
        with pytest.raises(ValueError):
            capi.trim_limit(bad)
    lib = capi.load()
    v = C.c_uint64(77)
    assert lib.naf_gpu_trim_limit(94, C.byref(v)) == -8 and v.value == 77 and lib.naf_gpu_trim_limit(20, None) == -8


def test_ee_units():
    from naf_amd import capi
    assert capi.ee_units("0") == 0 and capi.ee_units("1") == 2 ** 32 and capi.ee_units("0.5") == 2 ** 31
    assert capi.ee_units("0.000000001") == 4 and capi.ee_units("1.999999999") == 2 ** 33 - 5
    assert capi.ee_units(2) == 2 ** 33 and capi.ee_units(Fraction(1, 3)) == 2 ** 32 // 3 and capi.ee_units(b"10.25") == 41 * 2 ** 30
    for text in ("0", "1", "0.5", "0.000000001", "1.999999999", "4294967295.999999999"):
        assert capi.ee_units(text) == TP.ee_units(text) == int(Fraction(text) * 2 ** 32)
    for bad in ("1e3", "1.", ".5", "", "1,000", "-1", "+1", " 1", "1.0000000001", "0x10", 0.5, True, -1, 2 ** 32, "4294967296"):
        with pytest.raises(ValueError):
            capi.ee_units(bad)


def test_trim_to_segments():
    from naf_amd import capi
    rows = np.zeros(4, dtype=capi.TRIM_DTYPE)
    rows["record"], rows["begin"], rows["end"], rows["flags"] = [3, 4, 5, 6], [1, 0, 2, 0], [9, 0, 7, 5], [1, 2, 1, 6]
    assert capi.trim_to_segments(rows) == [(3, 1, 9), (5, 2, 7)] and capi.trim_to_segments(rows[:0]) == []


# ---- 5. the command line, before the device is opened -----------------------------------------------------------------------------------
REFUSED = [(["--trim", "20", "--locate", "NGG"], b"--trim and --locate can't be used together"),
           (["--trim", "20", "--composition"], b"--trim and --composition can't be used together"),
           (["--quality", "--trim", "20"], b"--trim and --quality can't be used together"),
           (["--trim", "20", "--runs", "N"], b"--trim and --runs can't be used together"),
           (["--masked-runs", "--trim", "20"], b"--trim and --masked-runs can't be used together"),
           (["--trim", "20", "--kmers", "3"], b"--trim and --kmers can't be used together"),
           (["--trim", "20", "--orfs"], b"--trim and --orfs can't be used together"),
           (["--translate", "--trim", "20"], b"--trim and --translate can't be used together"),
           (["--trim", "20", "--repeats", "misa"], b"--trim and --repeats can't be used together"),
           (["--trim", "20", "--4bit"], b"no other output type"), (["--ids", "--trim", "20"], b"no other output type"), (["--trim", "none", "--lengths"], b"no other output type"),
           (["--trim", "20", "--masked-fasta"], b"no other output type"), (["--trim", "20", "--charcount"], b"no other output type"),
           (["--trim", "20", "--trim-table", "--fastq"], b"--trim writes a table: no output type"), (["--seq", "--trim", "20", "--trim-table"], b"--trim writes a table: no output type"),
           (["--trim", "20", "--region", "x", "--revcomp"], b"--revcomp can't"), (["--trim", "20", "--rc-region", "x"], b"--rc-region can't"),
           (["--trim", "20", "--records", "1-2", "--records", "3-4"], b"one --records or one --region"),
           (["--trim", "20", "--region", "x:1-5"], b"whole sequence"),
           (["--min-length", "12"], b"--min-length can be used only with --trim"), (["--max-ee", "1"], b"--max-ee can be used only with --trim"),
           (["--trim-table"], b"--trim-table can be used only with --trim"), (["--quality", "--trim-table"], b"--trim-table can be used only with --trim"),
           (["--trim", "20", "--trim", "30"], b"only one --trim"), (["--trim", "20", "--max-ee", "1", "--max-ee", "2"], b"only one --max-ee"),
           (["--trim", ""], b"--trim parameter"), (["--trim", "94"], b"--trim parameter"), (["--trim", "Q20"], b"--trim parameter"), (["--trim", "-1"], b"--trim parameter"),
           (["--trim", "2,0"], b"--trim parameter"), (["--trim", "None"], b"--trim parameter"),
           (["--trim", "20", "--min-length", "0"], b"--min-length parameter"), (["--trim", "20", "--min-length", "x"], b"--min-length parameter"),
           (["--trim", "20", "--max-ee", "1e3"], b"--max-ee parameter"), (["--trim", "20", "--max-ee", "1."], b"--max-ee parameter"), (["--trim", "20", "--max-ee", ".5"], b"--max-ee parameter"),
           (["--trim", "20", "--max-ee", "0.0000000001"], b"--max-ee parameter"), (["--trim", "20", "--max-ee", "4294967296"], b"--max-ee parameter"),
           (["--trim", "20", "--max-ee", "-1"], b"--max-ee parameter"), (["--trim", "20", "--max-ee", ""], b"--max-ee parameter"),
           (["--trim", "20"], b"the archive has no quality section"), (["--trim", "none", "--trim-table"], b"the archive has no quality section")]


@pytest.mark.parametrize("args,word", REFUSED)
def test_trim_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c", naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr      # the check of this option, not the one for an option nobody knows


ACCEPTED = [["--trim", "20"], ["--trim", "0", "--fasta", "--line-length", "60"], ["--trim", "93", "--sequences"], ["--trim", "none", "--seq", "--max-ee", "0.5"],
            ["--trim", "30", "--min-length", "1,000", "--max-ee", "4294967295.999999999", "--fastq", "--records", "2-3"], ["--trim", "13", "--trim-table", "--region", "x"]]


@pytest.mark.parametrize("args", ACCEPTED)
def test_accepted_command_lines_reach_the_input(args):
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, os.path.join(GOLDEN, "naf", "no_such_file.naf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"unnaf error: can't open input file\n"


@pytest.mark.parametrize("args", [["--trim"], ["--trim", "20", "--min-length"], ["--trim", "20", "--max-ee"]])
def test_an_option_without_its_value_is_a_usage_error(args):
    p = subprocess.run([os.path.join(BIN, "unnaf"), os.path.join(GOLDEN, "naf", "acgt_10k.naf"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"unknown or incomplete argument \"%s\"" % args[-1].encode() in p.stderr


def test_help_gains_the_four_lines_behind_whole_units():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--trim" not in head and b"--min-length" not in head and b"--max-ee" not in head
    at = [tail.index(line) for line in (b"\n  --whole-units ", b"\n  --trim Q ", b"\n  --min-length N ", b"\n  --max-ee X ", b"\n  --trim-table ")]
    assert at == sorted(at) and tail.endswith(b"short,errors)\n")
