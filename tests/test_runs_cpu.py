"""What can be checked of the run table without a GPU: the plan (runs_plan.py) against its own claims -- the regex reference against a
plain loop, the seam coverage of the planted texts, the texts through the oracle --, the host-only parts of the C-ABI
(naf_gpu_parse_base_class, the exports, the row's layout), the binding's helpers and the command line's argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import runs_plan as RP
from conftest import GOLDEN, ROOT

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
BIN = os.path.join(ROOT, "naf_amd", "bin")


@pytest.fixture(scope="module")
def planned():
    return {c.name: c for c in RP.planned(SEED)}


def _lines(recs):
    return [r.encode("latin1") for r in recs]


def _expected(lines, q, m, first=0, count=None):
    _, s, each, masked, _ = q
    return RP.expected_masked(lines, m, first, count) if masked else RP.expected_runs(lines, s, each, m, first, count)


# ---- 1. the reference against a plain loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_expected_runs_against_the_brute_loop(k):
    rng = np.random.default_rng(9900 + 10 * SEED + k)
    alphabet = ["ACGTNN", RP.CODES, "ACGUacguNn--", "AAACCNnn"][k]
    recs = ["".join(rng.choice(list(alphabet), int(n))) for n in (0, 400, 1, 77, 0, 0, 150, 2)]
    lines = _lines(recs)
    for s, each in ((0x8000, False), (0x7FFF, False), (0x0001, False), (0x0116, True), (0x0116, False), (RP.ALL, True), (RP.ALL, False), (0x8001, True)):
        for m in (1, 2, 3, 10):
            assert RP.as_tuples(RP.expected_runs(lines, s, each, m)) == RP.brute_runs(lines, s, each, False, m)
        assert RP.as_tuples(RP.expected_runs(lines, s, each, 2, 1, 6)) == RP.brute_runs(lines, s, each, False, 2, 1, 6)
        assert len(RP.expected_runs(lines, s, each, 1, 3, 0)) == 0
    for m in (1, 2, 5):
        assert RP.as_tuples(RP.expected_masked(lines, m)) == RP.brute_runs(lines, masked=True, min_len=m)
    assert RP.as_tuples(RP.expected_masked(lines, 1, 2, 5)) == RP.brute_runs(lines, masked=True, first=2, count=5)


def test_the_small_planned_texts_against_the_brute_loop(planned):
    for name in ("record_ends", "record_ends_masked", "all16"):
        c = planned[name]
        lines = _lines(c.records)
        for q in c.queries:
            for m in q[4]:
                assert RP.as_tuples(_expected(lines, q, m)) == RP.brute_runs(lines, q[1], q[2], q[3], m), (name, q[:4], m)


def test_the_class_is_literal():
    lines = [b"ANRNNYN-nACGT"]
    assert RP.as_tuples(RP.expected_runs(lines, 0x8000)) == [(0, 1, 2, 15), (0, 3, 5, 15), (0, 6, 7, 15), (0, 8, 9, 15)]      # R and Y are no N
    assert RP.as_tuples(RP.expected_runs(lines, 0x7FFF)) == [(0, 0, 1, 8), (0, 2, 3, 10), (0, 5, 6, 5), (0, 7, 8, 0), (0, 9, 13, 8)]
    assert RP.as_tuples(RP.expected_runs(lines, 0x8000, min_len=2)) == [(0, 3, 5, 15)]


# ---- 2. the plan's coverage claims -------------------------------------------------------------------------------------------------------
def test_every_seam_kind_has_a_first_and_a_last_base_at_every_offset(planned):
    S = planned["seams"].seams
    cov = S.coverage()
    print("\n%-5s %-7s %-6s offsets" % ("what", "kind", "side"))
    for what in ("N", "mask"):
        for kind in RP.SEAM_KINDS:
            for side in ("first", "last"):
                got = sorted(cov.get((what, kind, side), ()))
                print("%-5s %-7s %-6s %s" % (what, kind, side, got))
                if kind != "end":
                    assert got == list(RP.OFFSETS), (what, kind, side)
    # the lengths of the plants, the masked ones of exactly 255 and 510 among them
    assert {b - a for what, _, _, _, _, a, b in S.plants if what == "N"} >= set(RunSeamsLengths)
    assert {b - a for what, _, _, _, _, a, b in S.plants if what == "mask"} >= {255, 510}
    assert S.stream[0] == "n" and S.stream[-1] == "n" and len(S.stream) % 2 == 1
    # runs at record seams that cross the record's end, and ones that do not
    ends = set(S.seams["record"])
    crossing = [1 for what, kind, _, _, _, a, b in S.plants if kind == "record" and any(a < e < b for e in ends)]
    inside = [1 for what, kind, _, _, _, a, b in S.plants if kind == "record" and not any(a < e < b for e in ends)]
    assert len(crossing) >= 4 and len(inside) >= 4
    assert sum(1 for r in S.records if not r) == 6


RunSeamsLengths = RP.RunSeams.PLANT_LENGTHS


def test_the_streams_end_is_covered_by_the_texts_together(planned):
    """The stream has one end: a run's first base at -2 and at -1 of it, and a run's last base at -2 and at -1, come from three texts."""
    first, last = set(), set()
    for name, rx in (("seams", "[Nn]+"), ("lengths", "[Nn]+"), ("record_ends", "-+"), ("record_ends_masked", "[a-z]+")):
        stream = "".join(planned[name].records)
        T = len(stream)
        for m in re.finditer(rx, stream):
            if m.start() >= T - 2:
                first.add(m.start() - T)
            if m.end() - 1 >= T - 2:
                last.add(m.end() - 1 - T)
    print("\nend: first", sorted(first), "last", sorted(last))
    assert first == {-2, -1} and last == {-2, -1}


def test_the_lengths_text(planned):
    c = planned["lengths"]
    lines = _lines(c.records)
    runs = RP.expected_runs(lines, 0x8000)
    lens = sorted(int(x["end"] - x["begin"]) for x in runs)
    assert lens == sorted(RP.LENGTHS + (65,)), lens
    masked = sorted(int(x["end"] - x["begin"]) for x in RP.expected_masked(lines))
    assert masked == sorted(RP.LENGTHS + RP.MASK_LENGTHS)
    assert any(a < RP.BLOCK < b for a, b in c.laid)                                 # one run lies across a block seam
    a, b = max(c.laid, key=lambda x: x[1] - x[0])
    assert (b // 4096) - (-(-a // 4096)) >= 2                                       # whole tiles inside a run: no event in them
    for L in RP.LENGTHS:
        for q in c.queries[:2]:
            assert {L - 1, L, L + 1} - {0} <= set(q[4])


def test_the_record_ends_text(planned):
    c = planned["record_ends"]
    recs = c.records
    lines = _lines(recs)
    runs = RP.as_tuples(RP.expected_runs(lines, 0x8000))
    by_rec = {}
    for r, b, e, _ in runs:
        by_rec.setdefault(r, []).append((b, e))

    def ends_with_run(r):
        return by_rec.get(r, [(0, 0)])[-1][1] == len(recs[r]) and len(recs[r]) > 0

    def starts_with_run(r):
        return by_rec.get(r, [(1, 1)])[0][0] == 0
    gaps = set()
    for r in range(len(recs)):
        if ends_with_run(r):
            n = next((k for k in range(r + 1, len(recs)) if recs[k]), None)
            if n is not None and starts_with_run(n):
                gaps.add(n - r - 1)
    assert gaps >= {0, 1, 3}, gaps                                                  # directly, one empty record between, three
    assert any(by_rec.get(r) == [(0, len(recs[r]))] and ends_with_run(r - 1) and starts_with_run(r + 1) for r in range(1, len(recs) - 1) if recs[r])
    stream = "".join(recs)
    assert len(stream) % 2 == 1 and stream[-1] == "-" and stream[0] == "n" and stream[1] == "N"
    dash = RP.as_tuples(RP.expected_runs(lines, 0x0001))
    assert dash[-1] == (len(recs) - 1, 0, 1, 0)                                     # the last base alone; behind it the padding nibble
    low = RP.as_tuples(RP.expected_masked(lines))
    assert any(recs[r] and recs[r] == recs[r].lower() and (r, 0, len(recs[r]), 0) in low for r in range(len(recs)))      # a record wholly inside a masked stretch
    m = planned["record_ends_masked"]
    s2 = "".join(m.records)
    assert s2[0].islower() and s2[-1].islower() and len(s2) % 2 == 1


def test_the_other_cases(planned):
    assert set(planned) >= {"all16", "rna", "fastq", "r7", "no_records", "nomask"}
    a = planned["all16"]
    assert any(q[1] == RP.ALL and q[2] for q in a.queries)
    assert {int(x["code"]) for x in RP.expected_runs(_lines(a.records), RP.ALL, True)} == set(range(16))
    f = planned["fastq"]
    assert all(len(r) == 150 for r in f.records)
    runs = RP.as_tuples(RP.expected_runs(_lines(f.records), 0x8000))
    assert any((r, 147, 150, 15) in runs and (r + 1, 0, 2, 15) in runs for r in range(len(f.records) - 1))
    assert planned["rna"].seq_type == 1 and b"U" in planned["rna"].text and planned["nomask"].no_mask and planned["no_records"].text == b""
    for c in planned.values():
        assert len(c.text) <= 640 * 1024


# ---- 3. the host-only C-ABI -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,want", RP.PARSE_TABLE)
def test_parse_base_class_against_the_table(text, want):
    from naf_amd import capi
    if want is None:
        with pytest.raises(ValueError):
            capi.parse_base_class(text)
    else:
        assert capi.parse_base_class(text) == want
        assert capi.parse_base_class(text.encode()) == want
        letters = text.lstrip("^").upper()
        assert want == (RP.set_of(letters) ^ 0xFFFF if text.startswith("^") else RP.set_of(letters))      # the table agrees with CODES


def test_parse_base_class_rejects_null_and_zero_bytes():
    from naf_amd import capi
    lib = capi.load()
    s = C.c_uint16(7)
    assert lib.naf_gpu_parse_base_class(None, C.byref(s)) != 0 and lib.naf_gpu_parse_base_class(b"N", None) != 0
    assert lib.naf_gpu_parse_base_class(b"", C.byref(s)) != 0 and lib.naf_gpu_parse_base_class(b"^", C.byref(s)) != 0 and s.value == 7
    with pytest.raises(ValueError):
        capi.parse_base_class("N\0N")


def test_runs_are_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_parse_base_class", "naf_gpu_unnaf_runs_count", "naf_gpu_unnaf_runs"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert C.sizeof(capi.Run) == 32 and np.dtype(capi.RUN_DTYPE).itemsize == 32 and capi.RUN_BYTES == 32
    assert capi.RUN_DTYPE == RP.RUN_DTYPE
    assert (capi.RUNS_EACH, capi.RUNS_MASKED) == (1, 2)
    assert [f[0] for f in capi.Run._fields_] == ["record", "begin", "end", "code", "reserved"] and capi.Run.code.offset == 24
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    for word in ("naf_gpu_run;", "NAF_GPU_RUNS_EACH = 1", "NAF_GPU_RUNS_MASKED = 2", "naf_gpu_parse_base_class", "naf_gpu_unnaf_runs_count", "LITERAL", "NAF_GPU_RUNS_PIECE"):
        assert word in header, word


def test_runs_to_segments():
    from naf_amd import capi
    runs = np.array([(3, 10, 13, 15, 0), (4, 2, 6, 0, 0), (4, 8, 9, 8, 0)], dtype=capi.RUN_DTYPE)
    assert capi.runs_to_segments(runs) == [(3, 10, 13), (4, 2, 6), (4, 8, 9)]
    assert capi.runs_to_segments(runs, flank=5, lengths=[0, 0, 0, 15, 9]) == [(3, 5, 15), (4, 0, 9), (4, 3, 9)]
    assert capi.runs_to_segments(runs, flank=2) == [(3, 8, 15), (4, 0, 8), (4, 6, 11)]
    assert capi.runs_to_segments(runs[:0]) == []


# ---- 4. the command line, before the device is opened -------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [(["--runs", "N", "--fasta"], b"BED"), (["--seq", "--runs", "N"], b"BED"), (["--masked-runs", "--ids"], b"BED"),
                                       (["--runs", "N", "--records", "1-2", "--records", "3-4"], b"one --records or one --region"),
                                       (["--masked-runs", "--region", "x", "--records", "1"], b"one --records or one --region"),
                                       (["--runs", "N", "--region", "x:1-5"], b"whole sequence"), (["--runs", "N", "--rc-region", "x"], b"--rc-region can't"),
                                       (["--masked-runs", "--region", "x", "--revcomp"], b"--revcomp can't"),
                                       (["--runs", "NX"], b"--runs parameter"), (["--runs", ""], b"--runs parameter"), (["--runs", "^"], b"--runs parameter"),
                                       (["--runs", "^-TGKCYSBAWRDMHVN"], b"--runs parameter"), (["--runs", "N", "--runs", "A"], b"only one --runs"),
                                       (["--runs", "N", "--min-run", "0"], b"--min-run parameter"), (["--runs", "N", "--min-run", "x"], b"--min-run parameter"),
                                       (["--min-run", "5"], b"--min-run can be used only with"), (["--each"], b"--each can be used only with --runs"),
                                       (["--masked-runs", "--each"], b"--each can be used only with --runs"), (["--runs", "N", "--masked-runs"], b"can't be used together"),
                                       (["--runs", "N", "--locate", "NGG"], b"--runs and --locate"), (["--masked-runs", "--composition"], b"--masked-runs and --composition"),
                                       (["--runs", "N", "--quality"], b"--runs and --quality")])
def test_runs_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr      # the check of this option, not the one for an option nobody knows


def test_help_gains_the_four_lines():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--runs" not in head
    for line in (b"\n  --runs CLASS ", b"\n  --masked-runs ", b"\n  --min-run N ", b"\n  --each "):
        assert line in tail


# ---- 5. the texts decode to what the plan says --------------------------------------------------------------------------------------------
def test_the_planned_texts_through_the_oracle(oracle, planned):
    for c in planned.values():
        naf = oracle.ennaf(c.text, c.seq_type, no_mask=c.no_mask)
        h = oracle.parse_naf(naf)
        lines = RP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), h.n_sequences)
        if c.r7:
            assert sum(len(x) for x in lines) < h.orig[oracle.SEQ]                    # bases behind the last record
        else:
            assert [x.decode("latin1") for x in lines] == c.records, c.name
        assert bool((h.flags >> 2) & 1) == (c.name != "nomask"), c.name
