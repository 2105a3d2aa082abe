"""The base composition, the parts that need no GPU: the plan (composition_plan.py) held to its claims, its expected_rows against a
per-base loop, naf_gpu_composition_rows_of (host only, through ctypes), the row's layout, the command-line checks that run before the
device is opened, and the planned texts through the oracle's (and, where built, the reference's) unnaf."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import composition_plan as CP
from conftest import GOLDEN, ROOT

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
BIN = os.path.join(ROOT, "naf_amd", "bin")
CASES = [c.name for c in CP.planned(0)]


@pytest.fixture(scope="module")
def planned(oracle):
    """name -> (case, the lines of the oracle's --sequences text of its archive, mask on)"""
    out = {}
    for c in CP.planned(SEED):
        naf = oracle.ennaf(c.text, c.seq_type, no_mask=c.no_mask)
        h = oracle.parse_naf(naf)
        out[c.name] = (c, CP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), h.n_sequences), naf)
    return out


# ---- 1. the plan ------------------------------------------------------------------------------------------------------------------------
def test_the_seams_text_plants_what_it_claims(planned):
    c, lines, _ = planned["seams"]
    S = c.seams
    T = S.TOTAL
    assert [x.decode() for x in lines] == S.records and sum(len(r) for r in S.records) == T and T % 2 == 1
    assert (T + 1) // 2 > 2 * 131072                                               # the packed stream crosses two block seams
    up = S.stream.upper()
    ends = set(S.bounds[1:-1])
    starts = [a for a, b in zip(S.bounds[:-1], S.bounds[1:]) if b > a]
    lens = [len(r) for r in S.records]
    assert {a & 1 for a in starts} == {0, 1} and lens.count(0) == 4 and lens[0] == 0 and lens[-1] == 0 and lens.count(1) == 2
    table = {k: {} for k in CP.SEAM_KINDS}
    for kind in ("lane", "load32", "tile"):
        p = S.seams[kind]
        unit, off = {"lane": (64, 0), "load32": (64, 32), "tile": (4096, 0)}[kind]
        assert all(q % unit == off for q in p) and (kind == "tile" or all(q % 4096 for q in p))
        assert {p[0] - 1, p[1], p[2] + 1} <= ends
        table[kind]["record ends at"] = "-1 0 +1"
    b1, b2 = S.seams["block"]
    assert (b1, b2) == (262144, 524288) and {b1 - 1, b1, b1 + 1} <= ends
    table["block"]["record ends at"] = "-1 0 +1"
    # CG: across a seam, starting on it, ending on it; each is inside one record and is counted by the per-base loop
    for kind, q, d in S.cg:
        assert up[q + d:q + d + 2] == "CG" and not (q + d + 1) in ends, (kind, q, d)
        table[kind].setdefault("CG with C at", []).append("%+d" % d)
    assert {(k, d) for k, _, d in S.cg} >= {(k, d) for k in ("lane", "load32", "tile") for d in (-1, 0, -2)} | {("block", -1)}
    assert {(q + d) & 1 for _, q, d in S.cg} == {0, 1}                              # the C in a low and in a high nibble
    # the sixteen codes before and behind
    for kind in ("lane", "load32", "tile"):
        pairs = [(q, a, b) for k, q, a, b in S.code_pairs if k == kind]
        assert sorted(a for _, a, _ in pairs) == list(range(16)) and sorted(b for _, _, b in pairs) == list(range(16))
        table[kind]["codes before / behind"] = "16 / 16"
    for kind, q, a, b in S.code_pairs:
        assert up[q - 1] == CP.CODES[a] and up[q] == CP.CODES[b], (kind, q, a, b)
    table["block"]["codes before / behind"] = "%d / %d" % (len({a for k, _, a, _ in S.code_pairs if k == "block"}), len({b for k, _, _, b in S.code_pairs if k == "block"}))
    assert "-" in up
    # toggles within one base of the seams and of window ends
    tog = {i for i in range(1, T) if S.stream[i].islower() != S.stream[i - 1].islower()}
    for kind, q, d in S.toggles_near:
        assert q + d in tog or (S.stream[q + d] == "-" or S.stream[q + d - 1] == "-"), (kind, q, d)
        table[kind].setdefault("toggle at", []).append("%+d" % d)
    assert all({-1, 0, 1} <= {d for k, _, d in S.toggles_near if k == kind} for kind in ("lane", "load32", "tile"))
    rb = S.bounds[S.longest]
    near = 0
    for w, k, d, at in S.window_toggles:
        assert at == rb + k * w + d and rb + k * w < S.bounds[S.longest + 1]
        near += at in tog or at + 5 in tog
    assert near >= len(S.window_toggles) - 4                                        # (random runs may swallow a few)
    # C ends a record and G opens the next: no CpG there; the stream ends in C
    assert len(S.c_then_g) >= 2 and all(e in ends and up[e - 1:e + 1] == "CG" for e in S.c_then_g) and up[-1] == "C"
    whole = CP.brute_rows([S.stream.encode()], (0,))[0][0][5]
    split = sum(x[5] for x in CP.brute_rows(lines, (0,))[0])
    straddle = sum(1 for e in ends if 0 < e < T and up[e - 1:e + 1] == "CG")
    assert whole - split == straddle >= len(S.c_then_g)
    print("\nseam kind x what is planted (stream of %d bases, %d records)" % (T, len(S.records)))
    for kind in CP.SEAM_KINDS:
        print("%-7s %s" % (kind, "; ".join("%s %s" % (k, v if isinstance(v, str) else " ".join(v)) for k, v in table[kind].items())))
        assert set(table[kind]) == {"record ends at", "CG with C at", "codes before / behind", "toggle at"}


def test_the_planned_cases_are_what_the_issue_lists(planned):
    assert set(planned) == {"seams", "plain", "sparse_iupac", "all16", "rna", "fastq", "r7", "nomask", "no_records"}
    for name, (c, lines, naf) in planned.items():
        bases = sum(len(x) for x in lines)
        assert bases <= 700 << 10
        if c.records is not None and not c.no_mask:
            assert [x.decode() for x in lines] == c.records, name
        assert set(c.windows) >= ({0, 100} if name == "no_records" else set(CP.WINDOWS_BIG))
        assert max(c.windows) > max([len(x) for x in lines] + [0])
    text = b"".join(planned["plain"][1])
    assert set(text) == set(b"ACGT")                                                 # only tiles of single upper-case nucleotides
    sp = b"".join(planned["sparse_iupac"][1])
    amb = [i for i, ch in enumerate(sp) if ch not in b"ACGT"]
    assert len(amb) >= 10 and all(b - a > 2 * 4096 for a, b in zip(amb[:-1], amb[1:])) and len(sp) == len(text)   # tiles of both paths adjoin
    a16 = b"".join(planned["all16"][1]).upper()
    assert set(a16) == set(CP.CODES.encode()) and len(a16) < 21000 and set(planned["all16"][0].windows) >= set(CP.WINDOWS_SMALL)
    assert all(a16[i:i + 4096].translate(None, b"ACGT") for i in range(0, len(a16), 4096))     # no tile of it is nucleotides only
    assert any(ch.islower() for ch in b"".join(planned["all16"][1]).decode())
    c, lines, naf = planned["rna"]
    assert b"U" in b"".join(lines).upper() and b"T" not in b"".join(lines).upper()
    c, lines, naf = planned["fastq"]
    assert 2000 <= len(lines) and {len(x) for x in lines} >= {1, 2, 63, 64, 65, 300} and max(len(x) for x in lines) == 300
    assert set(c.windows) >= set(CP.WINDOWS_SMALL)


def test_the_malformed_and_the_maskless_archives(planned, oracle):
    c, lines, naf = planned["r7"]
    h = oracle.parse_naf(naf)
    assert sum(len(x) for x in lines) < h.orig[oracle.SEQ]                             # bases behind the last record
    c, lines, naf = planned["nomask"]
    h = oracle.parse_naf(naf)
    assert not (h.flags >> 2) & 1 and any(ch.islower() for ch in c.text.decode()) and not any(x != x.upper() for x in lines)
    c, lines, naf = planned["no_records"]
    assert oracle.parse_naf(naf).n_sequences == 0 and lines == []
    assert len(CP.expected_rows([], 0)) == 0 and len(CP.expected_rows([b"", b""], 5)) == 0 and len(CP.expected_rows([b"", b""], 0)) == 2


@pytest.mark.parametrize("name", CASES)
def test_expected_rows_against_the_per_base_loop(planned, name):
    c, lines, _ = planned[name]
    windows = (0, 100, 4097) if name != "all16" else (0, 3, 64)
    brute = CP.brute_rows(lines, windows)
    for w in windows:
        rows = CP.expected_rows(lines, w)
        assert CP.as_tuples(rows) == brute[w], (name, w)
        assert all(sum(x[3]) == x[2] - x[1] for x in brute[w])
        assert len(rows) == sum(CP.rows_of(len(x), w) for x in lines)
    if len(lines) > 3:
        assert CP.as_tuples(CP.expected_rows(lines, 100, 1, 2)) == CP.brute_rows(lines, (100,), 1, 2)[100]
        tot = CP.expected_total(lines, CP.expected_rows(lines, 100, 1, 2), 1, 2)
        assert tot[0] == 2 and tot[2] == len(lines[1]) + len(lines[2]) == sum(tot[3])


def test_the_planned_texts_through_the_reference(planned, oracle, tmp_path):
    if not oracle.have_ref():
        return
    for name, (c, lines, naf) in planned.items():
        if not c.text:
            continue
        args = (["--rna"] if c.seq_type == 1 else []) + (["--no-mask"] if c.no_mask else [])
        ref = oracle.ref_ennaf(c.text, args, str(tmp_path))
        assert oracle.ref_unnaf(ref, ["--sequences"]) == oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), name


# ---- 2. the C-ABI's host side --------------------------------------------------------------------------------------------------------------
def test_composition_rows_of_against_ceil():
    from naf_amd import capi
    for n in (0, 1, 2, 63, 64, 65, 99, 100, 101, 4096, 10 ** 12, 2 ** 64 - 1):
        assert capi.composition_rows_of(n, 0) == 1
        for w in (1, 2, 3, 64, 100, 4097, 2 ** 40, 2 ** 64 - 1):
            assert capi.composition_rows_of(n, w) == -(-n // w) == CP.rows_of(n, w), (n, w)


def test_composition_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_composition_rows_of", "naf_gpu_unnaf_composition_rows", "naf_gpu_unnaf_composition"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert C.sizeof(capi.CompRow) == 168 == np.dtype(capi.COMP_DTYPE).itemsize == np.dtype(CP.ROW_DTYPE).itemsize
    assert capi.COMP_DTYPE == CP.ROW_DTYPE and capi.COMP_MASK == 1
    row = capi.CompRow(1, 2, 3, (C.c_uint64 * 16)(*range(10, 26)), 4, 5)
    a = np.frombuffer(bytes(row), dtype=capi.COMP_DTYPE)[0]
    assert (int(a["record"]), int(a["begin"]), int(a["end"]), list(a["n"]), int(a["masked"]), int(a["cpg"])) == (1, 2, 3, list(range(10, 26)), 4, 5)
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    assert "naf_gpu_comp_row" in header and "NAF_GPU_COMP_MASK = 1" in header


def test_the_table_the_command_line_prints():
    rows = np.zeros(2, dtype=CP.ROW_DTYPE)
    rows[0] = (0, 0, 10, [1, 2, 3, 0, 1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 1], 4, 1)
    rows[1] = (1, 5, 7, [0] * 15 + [2], 0, 0)
    assert CP.table(rows, ["a", "b"]) == (b"#seq\tstart\tend\tA\tC\tG\tT\tN\tother\tgap\tmasked\tCpG\tGC\n"
                                          b"a\t0\t10\t2\t1\t3\t2\t1\t0\t1\t4\t1\t0.500000\nb\t5\t7\t0\t0\t0\t0\t2\t0\t0\t0\t0\tNA\n")
    assert CP.table(rows[:0], [], rna=True).split(b"\t")[6] == b"U"


# ---- 3. the command line, before the device is opened ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [(["--composition", "--fasta"], b"--composition writes a table"), (["--seq", "--composition"], b"--composition writes a table"),
                                       (["--composition", "--ids"], b"--composition writes a table"), (["--composition", "--charcount"], b"--composition writes a table"),
                                       (["--composition", "--records", "1", "--revcomp"], b"--revcomp can't"), (["--composition", "--rc-region", "x"], b"--rc-region can't"),
                                       (["--composition", "--records", "1-2", "--records", "3-4"], b"--composition can be restricted by one --records or one --region"),
                                       (["--composition", "--region", "x", "--records", "1"], b"--composition can be restricted by one --records or one --region"),
                                       (["--composition", "--region", "x", "--region", "y"], b"--composition can be restricted by one --records or one --region"),
                                       (["--composition", "--region", "x:1-5"], b"--composition can be restricted to a whole sequence"),
                                       (["--window", "100"], b"--window can be used only with --composition"), (["--fasta", "--window", "100"], b"--window can be used only with --composition"),
                                       (["--composition", "--window", "0"], b"--window parameter"), (["--composition", "--window", "-5"], b"--window parameter"),
                                       (["--composition", "--window", "1e3"], b"--window parameter"), (["--composition", "--window", ""], b"--window parameter"),
                                       (["--composition", "--window", ","], b"--window parameter"), (["--composition", "--window", "99999999999999999999999"], b"--window parameter"),
                                       (["--composition", "--locate", "NGG"], b"--composition and --locate")])
def test_composition_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr


def test_help_gains_the_two_lines():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--composition" not in head and b"--window" not in head
    assert b"\n  --composition   - " in tail and b"\n  --window N      - " in tail
    assert tail.index(b"--locate PATTERN") < tail.index(b"\n  --composition")
