"""CPU tests of duplicate collapsing: the plan's model against its brute force, the plants against their claims and their places, the
coverage table, the host-only C-ABI (naf_gpu_dedup_level), the bindings and what unnaf refuses on the command line before the device is
opened.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dedup_plan as DP
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "naf_amd", "bin")
SEED = int(os.environ.get("NAF_TEST_SEED", "0"))


@pytest.fixture(scope="module")
def cases():
    return DP.planned(SEED)


def against_brute(records, both, bounds, where):
    rows, total, levels = DP.model(records, both, bounds)
    want = DP.brute(records, both, bounds)
    assert len(rows) == len(records) == len(want)
    firsts = 0
    for r, x in enumerate(rows):
        b, e, f = bounds[r] if bounds is not None else (0, len(records[r]), DP.KEPT)
        assert (int(x["record"]), int(x["begin"]), int(x["end"])) == (r, b, e), (where, r)
        if want[r] is None:
            assert (int(x["first"]), int(x["copies"]), int(x["flags"]), int(x["strand"])) == (r, 0, f, 0), (where, r)
            continue
        first, copies, strand = want[r]
        assert (int(x["first"]), int(x["copies"]), int(x["strand"])) == (first, copies, strand), (where, r, want[r], x)
        assert int(x["flags"]) == (DP.KEPT if first == r else DP.DUPLICATE) | (f & DP.CLIPPED), (where, r)
        firsts += first == r
    considered = sum(w is not None for w in want)
    assert total[:4] == (len(records), considered, firsts, considered - firsts) and sum(levels) == firsts, where
    assert total[4] == sum(1 for r, w in enumerate(want) if w and w[0] == r and w[1] == 1) and total[5] == max([w[1] for w in want if w] or [0]), where
    return rows


# ---- 1. the model against the brute force ---------------------------------------------------------------------------------------------
def test_the_model_agrees_with_all_pairs_on_the_planted_texts(cases):
    n = 0
    for c in cases:
        for both in (False, True):
            against_brute(c.records, both, None, (c.name, both))
            for bs in c.bsets:
                against_brute(c.records, both, c.bounds(bs), (c.name, both, bs))
            n += 1
    assert n == 2 * len(cases)


def test_the_model_agrees_with_all_pairs_on_random_reads():
    recs = DP.random_reads(SEED)
    rng = np.random.default_rng(5 + SEED)
    wins = [tuple(sorted(int(v) for v in rng.integers(0, len(r) + 1, 2))) + (int(rng.choice([1, 1, 1, 9, 2, 4, 6, 12])),) for r in recs]
    dups = 0
    for both in (False, True):
        for bounds in (None, wins):
            rows = against_brute(recs, both, bounds, (both, bounds is not None))
            dups += int((rows["flags"] & DP.DUPLICATE != 0).sum())
            assert both is False or (rows["strand"] == 1).any()
    assert dups > 100 and set("".join(recs).upper()) >= set(DP.CODES)


def test_the_complement_is_the_bit_reversal_of_the_code():
    for k, ch in enumerate(DP.CODES):
        rev = int("{:04b}".format(k)[::-1], 2)
        assert DP.rc(ch) == DP.CODES[rev], ch
    assert DP.rc("ACGTN-R") == "Y-NACGT" and DP.canon("acgu") == "ACGT"


def test_the_levels_are_fastqcs_bins():
    edges = {1: 0, 2: 1, 9: 8, 10: 9, 49: 9, 50: 10, 99: 10, 100: 11, 499: 11, 500: 12, 999: 12, 1000: 13, 4999: 13, 5000: 14, 9999: 14, 10000: 15, 2 ** 63: 15}
    for n, level in edges.items():
        assert DP.level_of(n) == level, n


# ---- 2. the plants ---------------------------------------------------------------------------------------------------------------------
def test_every_plant_is_what_it_claims(cases):
    n = 0
    for c in cases:
        rows = {}
        for p in c.plants:
            for both in (False, True):
                key = (both, p.bset)
                if key not in rows:
                    rows[key] = DP.model(c.records, both, c.bounds(p.bset) if p.bset else None)[0]
                assert DP.holds(p, rows[key], both), (c.name, p.cell, p.kind, p.off, p.name, p.rel, both)
            a, b = DP.canon(c.records[p.a]), DP.canon(c.records[p.b])
            if p.bset:
                (ab, ae, _), (bb, be, _) = c.bounds(p.bset)[p.a], c.bounds(p.bset)[p.b]
                a, b = a[ab:ae], b[bb:be]
            if p.rel == "same":
                assert a == b
            elif p.rel == "rc":
                assert a == DP.rc(b) and a != b
            elif p.rel == "near":
                assert a != b and a != DP.rc(b) and (abs(len(a) - len(b)) == 1 or (len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 1)), (c.name, p.name)
            elif p.rel == "differ":
                assert a != b and a != DP.rc(b)
            n += 1
    assert n > 700


def test_the_plants_lie_where_they_say(cases):
    n = 0
    for c in cases:
        for p in c.plants:
            if p.mark is None:
                continue
            first, last = int(c.starts[p.b]), int(c.starts[p.b + 1]) - 1
            unit = {"lane": DP.LANE, "load": DP.LANE, "tile": DP.TILE, "block": DP.BLOCK}[p.kind]
            seam = p.mark - p.off - (DP.LOAD if p.kind == "load" else 0)
            assert seam % unit == 0 and seam > 0, (c.name, p.kind, p.off, p.name)
            assert p.mark in (first, last) and ("first" in p.name) == (p.mark == first) or first == last or p.cell == "near", (c.name, p.kind, p.off, p.name)
            n += 1
    assert n > 400


def test_every_cell_has_a_plant_at_every_seam_kind(cases):
    cov = DP.coverage(cases)
    print("%-12s" % "" + "".join("%8s" % k for k in DP.SEAM_KINDS))
    for cell in DP.CELLS:
        print("%-12s" % cell + "".join("%8d" % cov[cell][k] for k in DP.SEAM_KINDS))
    for cell in DP.CELLS:
        for k in DP.SEAM_KINDS:
            assert cov[cell][k] > 0, (cell, k)
    # every offset of every seam that is placed by a position, for the first and for the last base
    seen = {(p.kind, p.off, "first" in p.name) for c in cases for p in c.plants if p.mark is not None}
    for kind in ("lane", "load", "tile", "block"):
        for off in DP.OFFSETS:
            for first in (True, False):
                assert (kind, off, first) in seen, (kind, off, first)
    # the four ways round of even and odd first bases of a second read and its class's first
    ways = set()
    for c in cases:
        rows = DP.model(c.records, True)[0]
        for p in c.plants:
            if p.rel in ("same", "rc") and p.bset is None:
                ways.add((p.rel, int(c.starts[int(rows[p.b]["first"])]) % 2, int(c.starts[p.b]) % 2))
    assert ways == {(rel, x, y) for rel in ("same", "rc") for x in (0, 1) for y in (0, 1)}
    sizes = {len(r) for c in cases for r in c.records}
    assert sizes >= set(DP.SMALL) | set(DP.LONG) | {0, 300000}
    assert all(sum(len(r) for r in c.records) <= 1300000 for c in cases)
    assert max(sum(len(r) for r in c.records) for c in cases) > 2 * DP.BLOCK             # two block seams


def test_the_classes_case_has_a_class_at_every_level_edge(cases):
    c = next(c for c in cases if c.name == "classes")
    rows, total, levels = DP.model(c.records)
    empties = sum(1 for r in c.records if not r)
    assert empties == 5 and c.records[0] == "" == c.records[-1] and any(not a and not b for a, b in zip(c.records, c.records[1:]))
    assert sorted(int(x["copies"]) for x in rows if int(x["flags"]) & DP.KEPT) == sorted(c.sizes + (empties,))
    assert levels == [1, 1, 0, 0, 1, 0, 0, 0, 1, 2, 1, 1, 1, 1, 0, 0] and total[5] == 1000
    assert any(a != b and a.upper() == b.upper() for a, b in zip(c.records[1:], c.records[2:])) or len({r for r in c.records}) > len({r.upper() for r in c.records})


def test_the_planned_texts_through_the_oracle(oracle, cases):
    for c in cases:
        if sum(len(r) for r in c.records) > 200000:
            continue                                                                    # (the GPU tests hold the larger ones to their records)
        naf = oracle.ennaf(c.text, c.seq_type, well_formed=c.fmt == "fastq")
        h = oracle.parse_naf(naf)
        assert h.n_sequences == len(c.records)
        text = oracle.unnaf(naf, oracle.MODE_SEQUENCES, True)
        assert [DP.canon(r) for r in text.decode("latin1").split("\n")[:-1]] == [DP.canon(r) for r in c.records], c.name


def test_the_table_lines():
    rows = np.zeros(4, dtype=DP.ROW_DTYPE)
    rows[0] = (0, 0, 5, 0, 2, DP.KEPT, 0); rows[1] = (1, 1, 6, 0, 2, DP.DUPLICATE | DP.CLIPPED, 1); rows[2] = (2, 0, 0, 2, 0, DP.SHORT | DP.ERRORS, 0); rows[3] = (3, 0, 3, 3, 1, DP.KEPT | DP.CLIPPED, 0)
    assert DP.table(rows, ["a", "b", "c", "d"], [5, 7, 9, 3]) == (b"#seq\tlength\tbegin\tend\tfirst\tcopies\tstrand\tstatus\n"
                                                                 b"a\t5\t0\t5\ta\t2\t+\tfirst\nb\t7\t1\t6\ta\t2\t-\tduplicate\nc\t9\t0\t0\tc\t0\t+\tshort,errors\nd\t3\t0\t3\td\t1\t+\tfirst\n")
    assert DP.kept_segments(rows) == [(0, 0, 5), (3, 0, 3)]


# ---- 3. the C-ABI and the bindings ----------------------------------------------------------------------------------------------------
def test_dedup_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_dedup_level", "naf_gpu_unnaf_dedup"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert np.dtype(capi.DEDUP_DTYPE).itemsize == 48 == capi.DEDUP_BYTES and capi.DEDUP_DTYPE == DP.ROW_DTYPE
    assert [np.dtype(capi.DEDUP_DTYPE).fields[f][1] for f in ("record", "begin", "end", "first", "copies", "flags", "strand")] == [0, 8, 16, 24, 32, 40, 44]
    assert C.sizeof(capi.DedupOpts) == 8 and capi.DedupOpts.bounds_kind.offset == 4 and C.sizeof(capi.DedupTotal) == 64
    assert [f[0] for f in capi.DedupTotal._fields_] == ["reads", "considered", "classes", "duplicates", "singletons", "largest", "bases", "kept_bases"]
    assert (capi.DEDUP_DUPLICATE, capi.DEDUP_BOTH_STRANDS, capi.DEDUP_BOUNDS_TRIM, capi.DEDUP_BOUNDS_CLIP, capi.DEDUP_LEVELS) == (16, 1, 0, 1, 16) == (DP.DUPLICATE, 1, 0, 1, len(DP.LEVEL_EDGES))
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    for word in ("naf_gpu_dedup_row;", "naf_gpu_dedup_opts;", "naf_gpu_dedup_total;", "NAF_GPU_DEDUP_DUPLICATE = 16", "NAF_GPU_DEDUP_BOTH_STRANDS = 1", "NAF_GPU_DEDUP_BOUNDS_TRIM = 0, NAF_GPU_DEDUP_BOUNDS_CLIP = 1",
                 "#define NAF_GPU_DEDUP_LEVELS 16", "/* 48 bytes */", "NAF_GPU_DEDUP_HASH_BITS", "duplicates cannot be collapsed in %s sequences", "NAF_GPU_ENOMEM: there is no piece size to set",
                 "[dedup] records R considered C classes U rounds J verified V sequence bytes decoded X of Y"):
        assert word in header, word
    assert "NAF_GPU_DEDUP_PIECE" not in header


def test_dedup_level():
    from naf_amd import capi
    lib = capi.load()
    edges = [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (7, 6), (8, 7), (9, 8), (10, 9), (49, 9), (50, 10), (99, 10), (100, 11), (499, 11), (500, 12), (999, 12), (1000, 13),
             (4999, 13), (5000, 14), (9999, 14), (10000, 15), (10001, 15), (2 ** 64 - 1, 15)]
    for n, level in edges:
        assert capi.dedup_level(n) == level == DP.level_of(n), n
        v = C.c_uint(77)
        assert lib.naf_gpu_dedup_level(n, C.byref(v)) == 0 and v.value == level
    v = C.c_uint(77)
    assert lib.naf_gpu_dedup_level(0, C.byref(v)) == -8 and v.value == 77 and lib.naf_gpu_dedup_level(5, None) == -8
    for bad in (0, -1, 2 ** 64):
        with pytest.raises(ValueError):
            capi.dedup_level(bad)


def test_dedup_to_segments():
    from naf_amd import capi
    rows = np.zeros(5, dtype=capi.DEDUP_DTYPE)
    rows["record"], rows["begin"], rows["end"], rows["flags"] = [3, 4, 5, 6, 7], [1, 0, 2, 0, 4], [9, 0, 7, 5, 8], [1, 16, 1 | 8, 16 | 8, 6]
    assert capi.dedup_to_segments(rows) == [(3, 1, 9), (5, 2, 7)] == DP.kept_segments(rows) and capi.dedup_to_segments(rows[:0]) == []


# ---- 4. the command line, before the device is opened ---------------------------------------------------------------------------------
A13 = "AGATCGGAAGAGC"
REFUSED = [(["--either-strand"], b"--either-strand can be used only with --dedup"), (["--dedup-table"], b"--dedup-table can be used only with --dedup"),
           (["--trim", "20", "--dedup-table"], b"--dedup-table can be used only with --dedup"), (["--adapter", A13, "--either-strand"], b"--either-strand can be used only with --dedup"),
           (["--dedup", "--locate", "NGG"], b"--dedup and --locate can't be used together"), (["--composition", "--dedup"], b"--dedup and --composition can't be used together"),
           (["--dedup", "--quality"], b"--dedup and --quality can't be used together"), (["--dedup", "--runs", "N"], b"--dedup and --runs can't be used together"),
           (["--dedup", "--masked-runs"], b"--dedup and --masked-runs can't be used together"), (["--dedup", "--kmers", "3"], b"--dedup and --kmers can't be used together"),
           (["--dedup", "--orfs"], b"--dedup and --orfs can't be used together"), (["--translate", "--dedup"], b"--dedup and --translate can't be used together"),
           (["--dedup", "--repeats", "misa"], b"--dedup and --repeats can't be used together"),
           (["--dedup", "--trim", "20", "--trim-table"], b"--trim-table can't be used with --dedup"), (["--dedup", "--adapter", A13, "--clip-table"], b"--clip-table can't be used with --dedup"),
           (["--dedup", "--dedup-table", "--adapter", A13, "--clip-table"], b"--clip-table can't be used with --dedup"),
           (["--dedup", "--region", "x", "--revcomp"], b"--revcomp can't"), (["--dedup", "--rc-region", "x"], b"--rc-region can't"),
           (["--dedup", "--region", "x:1-5"], b"whole sequence"), (["--dedup", "--records", "1-2", "--records", "3-4"], b"one --records or one --region"),
           (["--dedup", "--dedup-table", "--fastq"], b"--dedup writes a table: no output type"), (["--seq", "--dedup", "--dedup-table"], b"--dedup writes a table: no output type"),
           (["--dedup", "--4bit"], b"no other output type"), (["--ids", "--dedup"], b"no other output type"),
           (["--dedup", "--max-ee", "1"], b"--max-ee can be used only with --trim"), (["--dedup", "--min-length", "12"], b"--min-length can be used only with --trim or --adapter"),
           (["--dedup", "--min-overlap", "3"], b"--min-overlap can be used only with --adapter"),
           (["--dedup", "--trim", "20"], b"the archive has no quality section"), (["--dedup", "--fastq"], b"input has no qualities")]


@pytest.mark.parametrize("args,word", REFUSED)
def test_dedup_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c", naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr


def test_protein_archives_are_refused():
    for args in (["--dedup"], ["--dedup", "--dedup-table", "--either-strand"]):
        p = subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c", os.path.join(GOLDEN, "naf", "protein_small.naf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"unnaf error: duplicates cannot be collapsed in protein sequences\n"


ACCEPTED = [["--dedup"], ["--dedup", "--either-strand", "--fasta", "--line-length", "60"], ["--dedup", "--dedup-table"], ["--dedup", "--dedup-table", "--either-strand", "--region", "x"],
            ["--dedup", "--sequences", "--records", "2-3"], ["--dedup", "--seq"], ["--dedup", "--trim", "20", "--max-ee", "0.5", "--min-length", "30", "--fastq"],
            ["--adapter", A13, "--dedup", "--min-overlap", "5", "--adapter-errors", "0.2"], ["--trim", "none", "--adapter", A13, "--adapter", "ACGT", "--dedup", "--dedup-table", "--either-strand"]]


@pytest.mark.parametrize("args", ACCEPTED)
def test_accepted_command_lines_reach_the_input(args):
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, os.path.join(GOLDEN, "naf", "no_such_file.naf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"unnaf error: can't open input file\n"


def test_help_gains_the_block_in_front_of_the_clipping_options():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    text = p.stderr
    at = [text.index(line) for line in (b"\n  --whole-units ", b"\nOptions for collapsing duplicate reads", b"\n  --dedup  ", b"\n  --either-strand ", b"\n  --dedup-table ",
                                        b"\nOptions for clipping adapters", b"\n  --adapter SEQ ", b"\nOptions for trimming reads by quality", b"\n  --trim-table ")]
    assert at == sorted(at) and text.endswith(b"short,errors)\n")
    assert text.count(b"\n  --dedup ") == 1 and text.count(b"\n  --dedup-table ") == 1 and text.count(b"\n  --either-strand ") == 1
