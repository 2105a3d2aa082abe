"""CPU tests of adapter clipping: the plan's model against its brute force, the plants against their claims and their places, the coverage
table, the host-only C-ABI (naf_gpu_clip_budgets), the bindings and what unnaf refuses on the command line before the device is opened.
No GPU."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import clip_plan as CP
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "naf_amd", "bin")
SEED = int(os.environ.get("NAF_TEST_SEED", "0"))


@pytest.fixture(scope="module")
def plan():
    return CP.planned(SEED)


def row_tuple(x):
    return tuple(int(x[f]) for f in ("begin", "end", "adapter", "mismatches", "overlap", "flags"))


# ---- 1. the model against the brute force ---------------------------------------------------------------------------------------------
def test_the_model_agrees_with_the_brute_force_on_the_plants(plan):
    P, cases = plan
    n = 0
    for c in cases:
        want, seen = {}, set()
        for p in c.plants:
            rec = c.records[p.record]
            if len(rec) > 5000 or (p.cell, p.name, p.off if p.kind != "load" else None) in seen:   # (the load seams' plants are the lane seams' with other letters around them)
                continue
            seen.add((p.cell, p.name, p.off))
            for qn, bs, min_len, _ in p.claims:
                key = (qn, bs)
                if key not in want:
                    want[key] = CP.clip_points(c.records, P.q[qn], [(b[0], b[1]) for b in c.bounds(bs)] if bs else None)
                b, e = c.bounds(bs)[p.record][:2] if bs else (0, len(rec))
                assert CP.brute(rec, P.q[qn], b, e) == want[key][p.record], (c.name, p.cell, p.name, p.kind, p.off, qn, bs)
                n += 1
    assert n > 1000


def test_the_model_agrees_with_the_brute_force_on_random_reads(plan):
    P, _ = plan
    recs = CP.random_reads(SEED)
    rng = np.random.default_rng(5 + SEED)
    wins = [tuple(sorted(int(v) for v in rng.integers(0, len(r) + 1, 2))) for r in recs]
    loose = CP.Query(["GT", "NNG", "RYKM", "TGTGTGTGTGTGTGTGTGTGTGTGTGTGTGTGTG"[:32]], 1, budgets=[[0] + [min(L - 1, 1 + L // 3) for L in range(1, 33)]] * 4)
    clipped = 0
    for q in (P.q["four1"], P.q["iupac"], P.q["tbl"], P.q["o1"], P.q["m13"], P.q["o13"], loose):
        for windows in (None, wins):
            got = CP.clip_points(recs, q, windows)
            for k, r in enumerate(recs):
                b, e = windows[k] if windows else (0, len(r))
                assert CP.brute(r, q, b, e) == got[k], (k, r, q.adapters, b, e)
                clipped += got[k] is not None
    assert clipped > 300


# ---- 2. the plants --------------------------------------------------------------------------------------------------------------------
def test_every_plant_is_what_it_claims(plan):
    P, cases = plan
    for c in cases:
        rows = {}
        for p in c.plants:
            assert p.claims, (c.name, p.name)
            for qn, bs, min_len, claim in p.claims:
                key = (qn, bs, min_len)
                if key not in rows:
                    rows[key] = CP.model(c.records, P.q[qn], min_len, c.bounds(bs) if bs else None)[0]
                assert row_tuple(rows[key][p.record]) == claim, (c.name, p.cell, p.name, p.kind, p.off, qn, bs, min_len)


def test_every_clipped_row_is_a_plant(plan):
    """the background has no candidate of its own, under any query of the plan"""
    P, cases = plan
    for c in cases:
        if c.name in ("ones", "fastq"):
            continue
        planted = {p.record for p in c.plants}
        for qn, q in P.q.items():
            rows = CP.model(c.records, q)[0]
            assert set(rows["record"][rows["flags"] & CP.CLIPPED != 0].tolist()) <= planted, (c.name, qn)


def test_the_plants_lie_where_they_say(plan):
    _, cases = plan
    parity = set()
    for c in cases:
        for p in c.plants:
            a, b = int(c.starts[p.record]), int(c.starts[p.record + 1])
            parity.add(a % 2)
            if p.kind == "stream":
                assert p.record == len(c.records) - 1 and b == c.starts[-1]
            if p.mark is None or p.kind in ("record", "stream"):
                continue
            seam = p.mark - p.off
            if p.kind == "lane":
                assert seam % CP.LANE == 0, (c.name, p.name)
            elif p.kind == "load":
                assert seam % CP.LANE == CP.LOAD, (c.name, p.name)
            elif p.kind == "block":
                assert seam == CP.BLOCK and a - 40 <= seam <= b + 40, (c.name, p.name, a, b)
            elif b - a >= 4000:
                assert a // CP.TILE != (b - 1) // CP.TILE                               # a read of 4095 bases and more crosses a tile seam wherever it lies
            else:
                assert seam % CP.TILE == 0 and seam != CP.BLOCK, (c.name, p.name)
    assert parity == {0, 1}                                                             # records start on odd and on even bases


def test_every_cell_has_a_plant_at_every_seam_kind(plan):
    _, cases = plan
    cov = CP.coverage(cases)
    print("\n%-9s" % "cell" + "".join("%8s" % k for k in CP.SEAM_KINDS))
    for cell in CP.CELLS:
        print("%-9s" % cell + "".join("%8d" % cov[cell][k] for k in CP.SEAM_KINDS))
    for cell in CP.CELLS:
        for kind in CP.SEAM_KINDS:
            assert cov[cell][kind] > 0, (cell, kind)
    # the sub-values the lane, load and tile seams carry in full
    first = [p for c in cases for p in c.plants if p.cell == "first"]
    for kind in ("lane", "load", "tile"):
        assert sorted(p.off for p in first if p.kind == kind) == list(CP.OFFSETS)
    assert sorted(p.off for p in first if p.kind == "record" and p.name.endswith("record's end")) == list(CP.OFFSETS)
    ends = [p for c in cases for p in c.plants if p.cell == "end"]
    for kind in ("lane", "load"):
        assert sorted({(p.name, p.off) for p in ends if p.kind == kind}) == sorted(("L %d" % L, off) for L in (2, 3, 4, 9, 10, 11, 15, 16, 17, 31, 32) for off in range(-2, 3))
    assert {p.name for p in ends if p.kind == "tile"} == {"L %d" % L for L in (2, 3, 4, 9, 10, 11, 15, 16, 17, 31, 32)}
    budget = {p.name for c in cases for p in c.plants if p.cell == "budget" and p.kind == "tile"}
    for L in (9, 10, 19, 20, 29, 30):
        assert any(n.startswith("L %d at" % L) for n in budget) and any(n.startswith("L %d over" % L) for n in budget)
    lens = {len(c.records[p.record]) for c in cases for p in c.plants if p.cell == "lengths"}
    assert lens >= {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 150, 4095, 4096, 4097}
    assert sum(len(c.text) for c in cases) < 2 << 20 and all(len(c.text) <= 400 << 10 for c in cases)


def test_the_planned_texts_through_the_oracle(oracle, plan):
    _, cases = plan
    for c in cases:
        naf = oracle.ennaf(c.text, c.seq_type, well_formed=c.fmt == "fastq")
        h = oracle.parse_naf(naf)
        assert h.n_sequences == len(c.records)
        text = oracle.unnaf(naf, oracle.MODE_SEQUENCES, True)
        assert text.decode("latin1").split("\n")[:-1] == c.records, c.name


# ---- 3. the C-ABI and the bindings ----------------------------------------------------------------------------------------------------
def test_clip_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_clip_budgets", "naf_gpu_unnaf_clip"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert np.dtype(capi.CLIP_DTYPE).itemsize == 40 == capi.CLIP_BYTES and capi.CLIP_DTYPE == CP.ROW_DTYPE
    assert C.sizeof(capi.ClipOpts) == 16 and capi.ClipOpts.min_len.offset == 8 and C.sizeof(capi.ClipTotal) == 64
    assert [f[0] for f in capi.ClipTotal._fields_] == ["reads", "clipped", "kept", "bases", "kept_bases", "removed_bases", "n_short", "n_errors"]
    assert (capi.CLIP_CLIPPED, capi.CLIP_NO_ADAPTER, capi.CLIP_MAX_ADAPTERS) == (8, 2 ** 32 - 1, 16) == (CP.CLIPPED, CP.NO_ADAPTER, 16)
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    for word in ("naf_gpu_clip_row;", "naf_gpu_clip_opts;", "naf_gpu_clip_total;", "NAF_GPU_CLIP_NO_ADAPTER UINT32_MAX", "NAF_GPU_CLIP_CLIPPED = 8", "NAF_GPU_CLIP_MAX_ADAPTERS 16",
                 "NAF_GPU_CLIP_PIECE", "L = min(m_k, end_r - x)", "Expected errors only fall when a stretch gets shorter",
                 "[clip] adapters A records R clipped C pieces P sequence bytes decoded X of Y"):
        assert word in header, word


def test_clip_budgets():
    from naf_amd import capi
    lib = capi.load()
    for rate in ("0.1", "0", "0.2", "0.34", "0.999999999", Fraction(1, 3), Fraction(1, 7), 0, "0.05"):
        r = Fraction(rate) if not isinstance(rate, str) else Fraction(rate)
        for m in (1, 2, 3, 9, 10, 11, 13, 20, 31, 32):
            want = [0] + [min(L - 1, (L * r.numerator) // r.denominator) if L <= m else 0 for L in range(1, 33)]
            assert capi.clip_budgets(rate, m) == want == CP.budgets_of(r, m), (rate, m)
            out = (C.c_uint8 * 33)(*([77] * 33))
            assert lib.naf_gpu_clip_budgets(r.numerator, r.denominator, m, out) == 0 and list(out) == want
    assert capi.clip_budgets("0.1", 32)[10] == 1 and capi.clip_budgets("0.1", 32)[9] == 0 and capi.clip_budgets("0.1", 32)[32] == 3
    assert capi.clip_budgets(5, 8) == [0] + list(range(8)) + [0] * 24                  # a rate of one and more: capped at L - 1
    big = (C.c_uint8 * 33)()
    assert lib.naf_gpu_clip_budgets(2 ** 64 - 1, 1, 32, big) == 0 and list(big) == [0] + list(range(32))
    out = (C.c_uint8 * 33)(*([77] * 33))
    for num, den, m, o in ((1, 0, 13, out), (1, 10, 0, out), (1, 10, 33, out), (1, 10, 13, None)):
        assert lib.naf_gpu_clip_budgets(num, den, m, o) == -8
    assert list(out) == [77] * 33
    for bad in (0.1, True, "1e-1", ".1", "0.", "-0.1", "0.0000000001", ""):
        with pytest.raises(ValueError):
            capi.clip_budgets(bad, 13)
    for m in (0, 33, -1):
        with pytest.raises(ValueError):
            capi.clip_budgets("0.1", m)


def test_clip_to_segments():
    from naf_amd import capi
    rows = np.zeros(5, dtype=capi.CLIP_DTYPE)
    rows["record"], rows["begin"], rows["end"], rows["flags"] = [3, 4, 5, 6, 7], [1, 0, 2, 0, 4], [9, 0, 7, 5, 8], [1, 2 | 8, 1 | 8, 6, 4 | 8]
    assert capi.clip_to_segments(rows) == [(3, 1, 9), (5, 2, 7)] == CP.kept_segments(rows) and capi.clip_to_segments(rows[:0]) == []


# ---- 4. the command line, before the device is opened ---------------------------------------------------------------------------------
A13 = "AGATCGGAAGAGC"
REFUSED = [(["--adapter-errors", "0.1"], b"--adapter-errors can be used only with --adapter"), (["--min-overlap", "3"], b"--min-overlap can be used only with --adapter"),
           (["--clip-table"], b"--clip-table can be used only with --adapter"), (["--trim", "20", "--clip-table"], b"--clip-table can be used only with --adapter"),
           (["--adapter", A13, "--locate", "NGG"], b"--adapter and --locate can't be used together"), (["--composition", "--adapter", A13], b"--adapter and --composition can't be used together"),
           (["--adapter", A13, "--quality"], b"--adapter and --quality can't be used together"), (["--adapter", A13, "--runs", "N"], b"--adapter and --runs can't be used together"),
           (["--adapter", A13, "--masked-runs"], b"--adapter and --masked-runs can't be used together"), (["--adapter", A13, "--kmers", "3"], b"--adapter and --kmers can't be used together"),
           (["--adapter", A13, "--orfs"], b"--adapter and --orfs can't be used together"), (["--translate", "--adapter", A13], b"--adapter and --translate can't be used together"),
           (["--adapter", A13, "--repeats", "misa"], b"--adapter and --repeats can't be used together"),
           (["--adapter", A13, "--trim", "20", "--trim-table"], b"--trim-table can't be used with --adapter"),
           (["--adapter", A13, "--region", "x", "--revcomp"], b"--revcomp can't"), (["--adapter", A13, "--rc-region", "x"], b"--rc-region can't"),
           (["--adapter", A13, "--region", "x:1-5"], b"whole sequence"), (["--adapter", A13, "--records", "1-2", "--records", "3-4"], b"one --records or one --region"),
           (["--adapter", A13, "--records", "1-2", "--region", "x"], b"one --records or one --region"),
           (["--adapter", A13, "--clip-table", "--fastq"], b"--adapter writes a table: no output type"), (["--seq", "--adapter", A13, "--clip-table"], b"--adapter writes a table: no output type"),
           (["--adapter", A13, "--4bit"], b"no other output type"), (["--ids", "--adapter", A13], b"no other output type"),
           (["--adapter", A13, "--max-ee", "1"], b"--max-ee can be used only with --trim"), (["--min-length", "12"], b"--min-length can be used only with --trim or --adapter"),
           (["--adapter", "AC[GT]"], b"--adapter parameter"), (["--adapter", "ACGX"], b"--adapter parameter"), (["--adapter", ""], b"--adapter parameter"), (["--adapter", "AC-T"], b"--adapter parameter"),
           (["--adapter", "ACGT" * 8 + "A"], b"the first 32 decide the same clip points"),
           (["--adapter", A13] * 17, b"at most 16 --adapter"),
           (["--adapter", A13, "--adapter-errors", "1"], b"--adapter-errors parameter"), (["--adapter", A13, "--adapter-errors", "1.5"], b"--adapter-errors parameter"),
           (["--adapter", A13, "--adapter-errors", "0.1", "--adapter-errors", "0.2"], b"only one --adapter-errors"),
           (["--adapter", A13, "--adapter-errors", ".1"], b"--adapter-errors parameter"), (["--adapter", A13, "--adapter-errors", "1e-1"], b"--adapter-errors parameter"),
           (["--adapter", A13, "--adapter-errors", "0.0000000001"], b"--adapter-errors parameter"), (["--adapter", A13, "--adapter-errors", "-0.1"], b"--adapter-errors parameter"),
           (["--adapter", A13, "--min-overlap", "0"], b"--min-overlap parameter"), (["--adapter", A13, "--min-overlap", "33"], b"--min-overlap parameter"),
           (["--adapter", A13, "--min-overlap", "x"], b"--min-overlap parameter"), (["--adapter", A13, "--min-length", "0"], b"--min-length parameter"),
           (["--adapter", A13, "--trim", "20"], b"the archive has no quality section"), (["--adapter", A13, "--fastq"], b"input has no qualities")]


@pytest.mark.parametrize("args,word", REFUSED)
def test_clip_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c", naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr


def test_protein_archives_are_refused():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--adapter", A13, "-c", os.path.join(GOLDEN, "naf", "protein_small.naf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"unnaf error: adapters cannot be clipped in protein sequences\n"


ACCEPTED = [["--adapter", A13], ["--adapter", A13.lower(), "--adapter", "NNNNACGU", "--fasta", "--line-length", "60"], ["--adapter", A13, "--adapter-errors", "0", "--sequences"],
            ["--adapter", A13, "--adapter-errors", "0.125", "--min-overlap", "1", "--min-length", "1,000", "--seq"], ["--adapter", A13, "--clip-table", "--region", "x"],
            ["--adapter", A13, "--trim", "20", "--min-length", "30", "--max-ee", "0.5", "--fastq", "--records", "2-3"], ["--trim", "none", "--adapter", "ACGT" * 8, "--clip-table", "--min-overlap", "32"]]


@pytest.mark.parametrize("args", ACCEPTED)
def test_accepted_command_lines_reach_the_input(args):
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, os.path.join(GOLDEN, "naf", "no_such_file.naf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"unnaf error: can't open input file\n"


@pytest.mark.parametrize("args", [["--adapter"], ["--adapter", A13, "--adapter-errors"], ["--adapter", A13, "--min-overlap"]])
def test_an_option_without_its_value_is_a_usage_error(args):
    p = subprocess.run([os.path.join(BIN, "unnaf"), os.path.join(GOLDEN, "naf", "acgt_10k.naf"), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"unknown or incomplete argument \"%s\"" % args[-1].encode() in p.stderr


def test_help_gains_the_block_in_front_of_the_trimming_options():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    text = p.stderr
    at = [text.index(line) for line in (b"\n  --whole-units ", b"\nOptions for clipping adapters", b"\n  --adapter SEQ ", b"\n  --adapter-errors R ", b"\n  --min-overlap N ", b"\n  --clip-table ",
                                        b"\nOptions for trimming reads by quality", b"\n  --trim Q ", b"\n  --min-length N ", b"\n  --max-ee X ", b"\n  --trim-table ")]
    assert at == sorted(at) and text.endswith(b"short,errors)\n")
    assert text.count(b"\n  --min-length N ") == 1 and text.count(b"\n  --trim Q ") == 1
