"""The quality statistics, the parts that need no GPU: the error table (host only, through ctypes) against `decimal`, the row's layout,
the plan (quality_plan.py) held to its claims, its numpy rows against a per-byte loop, the command-line checks that run before the device
is opened, and the planned texts through the oracle's (and, where built, the reference's) unnaf."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import quality_plan as QP
from conftest import GOLDEN, ROOT

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
BIN = os.path.join(ROOT, "naf_amd", "bin")
CASES = [c.name for c in QP.planned(0)]


@pytest.fixture(scope="module")
def planned(oracle):
    """name -> (case, the quality lines of the oracle's --fastq text of its archive, the archive)"""
    out = {}
    for c in QP.planned(SEED):
        naf = oracle.ennaf(c.text, c.seq_type, well_formed=c.well_formed)
        h = oracle.parse_naf(naf)
        quals = QP.quals_of(oracle.unnaf(naf, oracle.MODE_FASTQ), h.n_sequences) if h.n_sequences else []
        out[c.name] = (c, quals, naf)
    return out


# ---- 1. the error table and the row ------------------------------------------------------------------------------------------------------
def test_the_error_table_is_the_decimal_one():
    from naf_amd import capi
    tab = capi.quality_error_table()
    assert len(tab) == 256 and tab == QP.ERR
    assert all(v == 2 ** 32 for v in tab[:34]) and tab[43] == 429496730 and tab[53] == 42949673 and tab[73] == 429497 and tab[126] == 2
    assert sum(tab[33:127]) == 20882629606 and tab[132] == 1 and not any(tab[133:])
    assert all(a >= b for a, b in zip(tab[33:], tab[34:]))
    assert capi.load().naf_gpu_quality_error_table(None) != 0


def test_quality_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_quality_error_table", "naf_gpu_unnaf_quality_rows", "naf_gpu_unnaf_quality"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert C.sizeof(capi.QualRow) == 56 == capi.QUAL_ROW_BYTES == np.dtype(capi.QUAL_DTYPE).itemsize == np.dtype(QP.ROW_DTYPE).itemsize
    assert capi.QUAL_DTYPE == QP.ROW_DTYPE
    row = capi.QualRow(1, 2, 3, 4, 5, 6, 7, 8)
    a = np.frombuffer(bytes(row), dtype=capi.QUAL_DTYPE)[0]
    assert QP.as_tuples([a]) == [(1, 2, 3, 4, 5, 6, 7, 8)]
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    assert "} naf_gpu_qual_row;" in header and "uint64_t n_q20, n_q30;" in header and "uint32_t min, max;" in header
    for s in ("naf_gpu_quality_error_table(uint64_t tab[256])", "naf_gpu_unnaf_quality_rows(", "naf_gpu_unnaf_quality(", "NAF_GPU_QUALITY_PIECE"):
        assert s in header


# ---- 2. the plan ---------------------------------------------------------------------------------------------------------------------------
def test_the_seams_text_plants_what_it_claims(planned):
    c, quals, _ = planned["seams"]
    S = c.seams
    T = S.TOTAL
    assert quals == S.quals and b"".join(quals) == S.stream and len(S.stream) == T == 600001
    s = S.stream
    ends = set(S.bounds[1:-1])
    lens = [len(q) for q in quals]
    assert lens[0] == 0 and lens[-1] == 0 and lens.count(0) == 4 and 0 in lens[2:-2] and max(lens) <= 70001
    unit = {"lane": (64, 0), "load": (64, 16), "tile": (4096, 0), "block": (131072, 0)}
    assert S.seams["block"][:2] == [131072, 262144] and T > S.seams["block"][-1]
    for kind in QP.SEAM_KINDS:
        p = S.seams[kind]
        assert all(q % unit[kind][0] == unit[kind][1] for q in p)
        assert kind in ("tile", "block") or all(q % 4096 for q in p)
        assert {p[0] - 1, p[1 if kind != "block" else 0], p[2 if kind != "block" else 0] + 1} <= ends                   # record ends at seam - 1, seam, seam + 1
    b0 = S.seams["block"][0]
    assert {b0 - 1, b0, b0 + 1} <= ends and quals.count(s[b0 - 1:b0]) >= 1 and [b0 - 1, b0, b0 + 1] == [e for e in sorted(ends) if abs(e - b0) <= 1]   # two reads of length 1 on it
    for kind, q, u, v in S.pairs:
        assert (s[q - 1], s[q]) == (u, v), (kind, q)
    for kind in ("lane", "load", "tile"):
        assert sorted(u for k, _, u, _ in S.pairs if k == kind) == sorted(v for k, _, _, v in S.pairs if k == kind) == sorted(QP.PLANTS)
    blk = [(u, v) for k, _, u, v in S.pairs if k == "block"]
    assert sorted(u for u, _ in blk) + sorted(v for _, v in blk) and {x for uv in blk for x in uv} == set(QP.PLANTS) and len(blk) == 4
    # a read whose only lowest / highest code lies right before, and one where it lies right behind, a tile seam
    starts = sorted(set(S.bounds))
    seen = set()
    for kind, q, u, v in S.pairs:
        if kind != "tile":
            continue
        a = max(x for x in starts if x <= q - 1)
        e = min(x for x in starts if x > q)
        read = s[a:e]
        assert a < q - 1 and e > q + 1                                              # the pair lies inside one read, across the seam
        for side, val in (("before", u), ("behind", v)):
            if val == 33:
                assert min(read) == 33 and read.count(33) == 1
                seen.add(("min", side))
            if val == 126:
                assert max(read) == 126 and read.count(126) == 1
                seen.add(("max", side))
    assert seen == {("min", "before"), ("min", "behind"), ("max", "before"), ("max", "behind")}
    assert set(s) <= set(range(33, 127)) and c.own_quals == [q for q in quals if q] and b"".join(c.own_quals) == s


def test_the_planned_cases_are_what_the_issue_lists(planned):
    assert list(planned) == ["seams", "short", "long", "allbytes", "protein", "no_records"]
    for name, (c, quals, naf) in planned.items():
        assert quals == c.quals, name                                              # the text comes back from the oracle
        assert sum(len(q) for q in quals) <= 700 << 10
        far = max([len(q) for q in quals] + [0])
        assert set(c.widths) == {W for W in QP.WIDTHS if -(-far // W) <= QP.MAX_ROWS} or name == "no_records"
        assert (c.own_text is not None) == (bool(quals) and all(quals) and set(b"".join(quals)) <= set(range(33, 127)) or name == "seams")
    c, quals, _ = planned["seams"]
    assert 1 in c.widths and 1 << 40 in c.widths
    c, quals, _ = planned["short"]
    lens = [len(q) for q in quals]
    assert len(quals) == 3000 and lens[:6] == [1, 2, 63, 64, 65, 300] and min(lens) == 1 and max(lens) == 300 and set(b"".join(quals)) == set(range(33, 74))
    c, quals, _ = planned["long"]
    lens = [len(q) for q in quals]
    K = QP.LDS_BINS
    assert max(lens) == 70000 > K + 4096 and {K - 1, K, K + 1} <= set(lens) and 1 in c.widths
    assert sum(n > K - 1 for n in lens) >= 3 and sum(n > K for n in lens) >= 2      # bins K - 1 and K hold codes of several reads
    c, quals, naf = planned["allbytes"]
    h = np.bincount(np.frombuffer(b"".join(quals), dtype=np.uint8), minlength=256)
    assert h[10] == 0 and all(h[v] >= 2 for v in range(256) if v != 10) and b"" in quals
    c, quals, naf = planned["protein"]
    assert c.seq_type == 2
    c, quals, naf = planned["no_records"]
    assert quals == [] and len(QP.record_rows([])) == 0 and len(QP.cycle_rows([], 5)) == 0 and QP.total_of([]) == (0, 0, 0, 0, 0, 0, 255, 0)


def test_the_archives_of_the_plan(planned, oracle):
    for name, (c, quals, naf) in planned.items():
        h = oracle.parse_naf(naf)
        assert h.n_sequences == len(quals)
        if quals:
            assert h.flags & 1 and h.orig[oracle.QUAL] == sum(len(q) for q in quals) and h.seq_type == c.seq_type


@pytest.mark.parametrize("name", ["short", "long", "allbytes", "protein", "no_records"])
def test_numpy_rows_against_the_per_byte_loop(planned, name):
    c, quals, _ = planned[name]
    widths = (1, 64, 100) if name != "long" else (1, 1000)
    if name == "short":
        quals = quals[:400]
    rec, cyc, hist = QP.brute(quals, widths)
    assert QP.as_tuples(QP.record_rows(quals)) == rec and QP.hist_of(quals) == hist
    for W in widths:
        assert QP.as_tuples(QP.cycle_rows(quals, W)) == cyc[W], (name, W)
        assert len(cyc[W]) == QP.n_cycle_rows(quals, W)
        assert sum(t[1] for t in cyc[W]) == sum(t[1] for t in rec)
    tot = QP.total_of(quals)
    assert tot[:6] == (len(quals),) + tuple(sum(t[f] for t in rec) for f in range(1, 6))
    if len(quals) > 5:
        rec2, cyc2, hist2 = QP.brute(quals, (64,), 2, 3)
        assert QP.as_tuples(QP.record_rows(quals, 2, 3)) == rec2 and QP.as_tuples(QP.cycle_rows(quals, 64, 2, 3)) == cyc2[64] and QP.hist_of(quals, 2, 3) == hist2
        assert QP.total_of(quals, 2, 3)[0] == 3 and len(cyc2[64]) == -(-max(len(q) for q in quals[2:5]) // 64)


def test_the_planned_texts_through_the_reference(planned, oracle, tmp_path):
    if not oracle.have_ref():
        return
    for name, (c, quals, naf) in planned.items():
        if c.own_text is None:
            continue                                                                # (the reference's parser takes codes 33..126 and no empty reads)
        ref = oracle.ref_ennaf(c.own_text, ["--protein"] if c.seq_type == 2 else [], str(tmp_path))
        text = oracle.ref_unnaf(ref, ["--fastq"])
        assert QP.quals_of(text, len(c.own_quals)) == c.own_quals, name


# ---- 3. the tables the command line prints -------------------------------------------------------------------------------------------------
def test_the_tables_the_command_line_prints():
    rows = np.zeros(3, dtype=QP.ROW_DTYPE)
    rows[0] = (0, 4, 4 * 33 + 10, 3 * 2 ** 31, 1, 0, 33, 53)
    rows[1] = (1, 0, 0, 0, 0, 0, 255, 0)
    rows[2] = (2, 3, 3 * 73, 3 * 429497, 3, 3, 73, 73)
    assert QP.table(rows, ["a", "b", "c"]) == (b"#seq\tlength\tmean\tmin\tmax\tq20\tq30\tee\n" b"a\t4\t2.5000\t0\t20\t1\t0\t1.500000\n"
                                               b"b\t0\tNA\tNA\tNA\t0\t0\t0.000000\n" b"c\t3\t40.0000\t40\t40\t3\t3\t0.000300\n")
    cyc = np.zeros(2, dtype=QP.ROW_DTYPE)
    cyc[0] = (0, 5, 5 * 43, 5 * 429496730, 0, 0, 43, 43)
    cyc[1] = (1, 2, 2 * 63, 2 * 4294967, 2, 2, 63, 63)
    assert QP.cycle_table(cyc, 100, 150) == (b"#cycle_begin\tcycle_end\tn\tmean\tmin\tmax\tq20\tq30\tee\n" b"1\t100\t5\t10.0000\t10\t10\t0\t0\t0.500000\n"
                                             b"101\t150\t2\t30.0000\t30\t30\t2\t2\t0.002000\n")
    assert QP.table(rows[:0], []).count(b"\n") == 1 and QP.cycle_table(cyc[:0], 1, 0).count(b"\n") == 1


# ---- 4. the command line, before the device is opened ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [(["--quality", "--fastq"], b"--quality writes a table"), (["--seq", "--quality"], b"--quality writes a table"),
                                       (["--quality", "--ids"], b"--quality writes a table"), (["--quality", "--locate", "NGG"], b"--quality and --locate"),
                                       (["--quality", "--composition"], b"--quality and --composition"), (["--composition", "--quality", "--cycles", "5"], b"--quality and --composition"),
                                       (["--quality", "--records", "1", "--revcomp"], b"--revcomp can't"), (["--quality", "--rc-region", "x"], b"--rc-region can't"),
                                       (["--quality", "--records", "1-2", "--records", "3-4"], b"--quality can be restricted by one --records or one --region"),
                                       (["--quality", "--region", "x", "--records", "1"], b"--quality can be restricted by one --records or one --region"),
                                       (["--quality", "--region", "x:1-5"], b"--quality can be restricted to a whole sequence"),
                                       (["--cycles", "100"], b"--cycles can be used only with --quality"), (["--fastq", "--cycles", "100"], b"--cycles can be used only with --quality"),
                                       (["--quality", "--cycles", "0"], b"--cycles parameter"), (["--quality", "--cycles", "-5"], b"--cycles parameter"),
                                       (["--quality", "--cycles", "1e3"], b"--cycles parameter"), (["--quality", "--cycles", ""], b"--cycles parameter"),
                                       (["--quality", "--cycles", ","], b"--cycles parameter"), (["--quality", "--cycles", "99999999999999999999999"], b"--cycles parameter")])
def test_quality_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "fastq_4k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr


def test_help_gains_the_two_lines_behind_the_window_line():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    head, sep, tail = p.stderr.partition(b"\n  --window N      - ")
    assert sep and b"--quality" not in head and b"--cycles" not in head
    assert b"\n  --quality       - " in tail and b"\n  --cycles N      - " in tail and tail.index(b"--quality  ") < tail.index(b"--cycles N")
