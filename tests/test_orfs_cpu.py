"""What can be checked of the open reading frames without a GPU: the plan (orfs_plan.py) against its own claims -- the numpy model against
a plain walk, one codon at a time, and against a look-ahead regex; the seam coverage of the planted texts; the texts through the oracle --,
the host-only parts of the C-ABI (naf_gpu_parse_codon_set, the exports, the row's layout) and the command line's argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orfs_plan as OP
from conftest import GOLDEN, ROOT

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
BIN = os.path.join(ROOT, "naf_amd", "bin")
STOPS3, START1 = {"TAA", "TAG", "TGA"}, {"ATG"}


@pytest.fixture(scope="module")
def planned():
    return {c.name: c for c in OP.planned(0)}


def _lines(recs):
    return [r.encode("latin1") for r in recs]


# ---- 1. the model against a plain walk -------------------------------------------------------------------------------------------------
def _codons_of(text):
    return set(text.upper().replace("U", "T").split(",")) if text else set()


def slow_rows(lines, q, first=0, count=None):
    """The same table by a walk over the codons of every frame, one at a time; the reverse strand is walked on the reverse-complemented
    text and its coordinates are turned back.  Codon sets are sets of strings (no IUPAC letters in them)."""
    stops, starts = _codons_of(q.stops), _codons_of(q.starts)
    split, closed = q.flags & OP.SPLIT_UNKNOWN, q.flags & OP.CLOSED
    rows = []
    for r in range(first, len(lines) if count is None else first + count):
        fwd = lines[r].decode("latin1").upper().replace("U", "T")
        L = len(fwd)
        for s in (0, 1):
            if not (q.strands >> s) & 1:
                continue
            t = OP.revcomp(fwd) if s else fwd                                       # letters that have no complement stay: they are unknown either way
            for f in range(3):
                open_at, left_stop, first_start = f, False, None
                o = f
                while True:
                    at_end = o + 3 > L
                    w = None if at_end else t[o:o + 3]
                    known = w is not None and not w.strip("ACGT")
                    is_stop = known and w in stops
                    if at_end or is_stop or (split and not known):
                        b, e = (open_at if first_start is None else first_start), o
                        if starts and first_start is None:
                            b = e
                        if e > b and e - b >= q.min_len and (is_stop or not closed):
                            fl = (OP.STOP3 if is_stop else 0) | (OP.STOP5 if left_stop else 0)
                            rows.append((r, b, e, s, f, fl) if s == 0 else (r, L - e, L - b, 1, f, fl))
                        if at_end:
                            break
                        open_at, left_stop, first_start = o + 3, is_stop, None
                    elif known and w in starts and first_start is None:
                        first_start = o
                    o += 3
    out = np.array(rows, dtype=OP.ORF_DTYPE) if rows else np.zeros(0, dtype=OP.ORF_DTYPE)
    return out[np.lexsort((out["strand"], out["end"], out["begin"], out["record"]))]


def model(lines, q, first=0, count=None):
    st, sa = q.sets()
    return OP.expected_rows(lines, st, sa, q.min_len, q.strands, q.flags, first, count)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_the_model_against_the_plain_walk_on_random_lines(k):
    rng = np.random.default_rng(12900 + 10 * SEED + k)
    alphabet = ["ACGT", "ACGTN", "ACGUacguNnR-", "AATTG"][k]
    lines = _lines(["".join(rng.choice(list(alphabet), int(n))) for n in (0, 400, 1, 77, 0, 0, 150, 2, 3, 4, 5, 12, 13, 1000)])
    for q in OP.QS_ALL + [OP.Q("TAA", "ATG,TTG", 1, 3, 3), OP.Q("TGA,TTT", None, 6, 2, 1)]:
        assert model(lines, q).tobytes() == slow_rows(lines, q).tobytes(), q
        assert model(lines, q, 1, 3).tobytes() == slow_rows(lines, q, 1, 3).tobytes(), q
        assert len(model(lines, q, 3, 0)) == 0


def test_the_planned_texts_against_the_plain_walk(planned):
    seen = 0
    for c in planned.values():
        if c.records is None:
            continue
        lines = _lines(c.records)
        for q in (c.qs if len(c.text) < 200000 else c.qs[:2]):
            want = slow_rows(lines, q)
            assert model(lines, q).tobytes() == want.tobytes(), (c.name, q)
            seen += len(want)
    assert seen > 10000


def test_the_model_against_a_regex_on_the_dense_text(planned):
    """stop to stop: a frame's stretches are what lies between its stops; with a start: ATG and every codon up to the next stop in frame,
    found with a look-ahead so that every offset is tried, and only the first ATG of a stretch counts"""
    lines = _lines(planned["dense"].records)
    q = OP.Q(OP.STD_STOPS, OP.STD_STARTS, 30, 1)
    got = model(lines, q)
    pat = re.compile(r"(?=(ATG(?:(?!TAA|TAG|TGA)[ACGT]{3})*)(TAA|TAG|TGA))")
    for r in (1, 2, 4, 5):                                                          # records without N (every third one has some)
        t = lines[r].decode().upper()
        assert "N" not in t
        best = {}
        for m in pat.finditer(t):
            e = m.start() + len(m.group(1))
            best.setdefault((e, m.start() % 3), m.start())                          # the first ATG that reaches this stop in its frame
        want = sorted((b, e) for (e, f), b in best.items() if e - b >= 30)
        have = sorted((int(x["begin"]), int(x["end"])) for x in got if x["record"] == r and x["flags"] & OP.STOP3)
        assert have == want and len(want) > 5, r
    q2 = OP.Q(OP.STD_STOPS, None, 3, 1, OP.CLOSED)
    got2 = model(lines, q2)
    for r in (1, 2):
        t = lines[r].decode().upper()
        want = []
        for f in range(3):
            codons = [t[o:o + 3] for o in range(f, len(t) - 2, 3)]
            at = [-1] + [i for i, w in enumerate(codons) if w in STOPS3]
            want += [(f + 3 * (a + 1), f + 3 * b) for a, b in zip(at[:-1], at[1:]) if b > a + 1]
        have = sorted((int(x["begin"]), int(x["end"])) for x in got2 if x["record"] == r)
        assert have == sorted(want), r


def test_a_few_rows_by_hand():
    #            0         1         2
    #            0123456789012345678901234567
    lines = [b"CCATGAAACCCTAAGGCATCCCTTACC"]
    std = OP.codon_set("TAA,TAG,TGA")
    rows = OP.expected_rows(lines, std, OP.codon_set("ATG"), 3, 3, 0)
    # forward: ATG at 2 (frame 2), codons ATG AAA CCC, then TAA at 11: [2, 11), closed; the stretch began at the record's edge.
    # reverse, forward offsets 1, 4, 7, ... (L = 27, frame (27 - 4) mod 3 = 2): CAT CAA ACC CTA AGG CAT CCC TTA.  CTA at 10 and TTA at 22 are
    # reverse stops.  The stretch [13, 22) lies between them and its start codon of greatest offset is CAT at 16: [13, 19), STOP3 and STOP5.
    # The stretch [1, 10) runs from the record's edge (its 3' end) to CTA (in front of its 5' end); its start is CAT at 1: [1, 4), STOP5.
    assert [tuple(int(v) for v in x) for x in rows] == [(0, 1, 4, 1, 2, OP.STOP5), (0, 2, 11, 0, 2, OP.STOP3), (0, 13, 19, 1, 2, OP.STOP3 | OP.STOP5)]
    # stop to stop, forward, min 6.  Frame 0: CCA, then TGA at 3 (its [0, 3) is too short), then [6, 27) to the edge.  Frame 1: no stop,
    # [1, 25).  Frame 2: [2, 11) up to TAA and [14, 26) behind it.
    rows = OP.expected_rows(lines, std, 0, 6, 1, 0)
    assert [tuple(int(v) for v in x) for x in rows] == [(0, 1, 25, 0, 1, 0), (0, 2, 11, 0, 2, OP.STOP3), (0, 6, 27, 0, 0, OP.STOP5), (0, 14, 26, 0, 2, OP.STOP5)]
    assert OP.totals(rows) == (4, 24 + 9 + 21 + 12, [1, 1, 2, 0, 0, 0])
    assert OP.cli_lines(rows[1:2], ["x"]) == b"x\t2\t11\t+3\t3\t+\tstop\n"


# ---- 2. the coverage of the planted texts --------------------------------------------------------------------------------------------------
def test_the_plants_cover_every_seam_offset_strand_and_kind(planned, capsys):
    cov = OP.coverage(planned.values())
    with capsys.disabled():
        print()
        for kind in OP.SEAM_KINDS:
            for strand, what, letters in OP.PLANTS:
                print("  %-7s %s %-5s %s  " % (kind, "+-"[strand], what, letters) + " ".join("%+d:%s" % (d, ",".join(cov.get((kind, d, strand, what), ["--"]))[:14]) for d in OP.OFFSETS))
    for cell in OP.coverage_cells():
        assert cov.get(cell), cell
    assert len(OP.coverage_cells()) == 6 * 6 * 4 + 3 * 4


def test_the_background_has_no_event(planned):
    """letters of A, C and G alone give no stop and no start on either strand"""
    rng = np.random.default_rng(12990 + SEED)
    lines = _lines(["".join(rng.choice(list("ACG"), 20000))])
    assert len(model(lines, OP.Q(OP.STD_STOPS, OP.STD_STARTS, 3))) == 0
    rows = model(lines, OP.DENSEST)
    assert sorted((int(x["begin"]), int(x["end"]), int(x["flags"])) for x in rows) == sorted([(0, 19998, 0), (1, 19999, 0), (2, 20000, 0)] * 2)
    big = next(r for r in planned["records"].records if len(r) == 3 * OP.TILE)
    assert not set(big) - set("ACG")                                                # a stretch of more than two tiles without an event
    s = planned["seams0"]
    assert len(s.stream) == 600001 and len(s.stream) // OP.BLOCK == 2               # three raw blocks of the packed stream


# ---- 3. naf_gpu_parse_codon_set ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,want", OP.CODON_TABLE)
def test_parse_codon_set_against_the_table(text, want):
    from naf_amd import capi
    lib = capi.load()
    s = C.c_uint64(0x1234567)
    rc = lib.naf_gpu_parse_codon_set(text.encode(), C.byref(s))
    if want is None:
        assert rc == -8 and s.value == 0x1234567                                    # nothing written on failure
        with pytest.raises(ValueError):
            capi.parse_codon_set(text)
        return
    assert rc == 0 and s.value == want
    assert capi.parse_codon_set(text) == want == capi.parse_codon_set(text.encode())
    assert OP.codon_set(text) == want                                               # the table agrees with positional notation


def test_parse_codon_set_follows_kmer_index_and_null_pointers():
    from naf_amd import capi
    for i in range(64):
        w = capi.kmer_text(3, i)
        assert capi.parse_codon_set(w) == 1 << i == capi.parse_codon_set(w.lower().replace("t", "u"))
    lib = capi.load()
    s = C.c_uint64(5)
    assert lib.naf_gpu_parse_codon_set(None, C.byref(s)) == -8 and lib.naf_gpu_parse_codon_set(b"TAA", None) == -8 and s.value == 5
    with pytest.raises(ValueError):
        capi.parse_codon_set("TA\0A")


def test_orfs_are_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_parse_codon_set", "naf_gpu_unnaf_orfs_count", "naf_gpu_unnaf_orfs"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert C.sizeof(capi.Orf) == 32 and np.dtype(capi.ORF_DTYPE).itemsize == 32 and capi.ORF_BYTES == 32
    assert capi.ORF_DTYPE == OP.ORF_DTYPE
    assert (capi.ORF_STOP3, capi.ORF_STOP5, capi.ORF_SPLIT_UNKNOWN, capi.ORF_CLOSED) == (1, 2, 1, 2)
    assert [f[0] for f in capi.Orf._fields_] == ["record", "begin", "end", "strand", "frame", "flags"]
    assert (capi.Orf.strand.offset, capi.Orf.frame.offset, capi.Orf.flags.offset) == (24, 28, 30)
    header = open(os.path.join(ROOT, "include", "naf_gpu.h")).read()
    for word in ("naf_gpu_orf;", "NAF_GPU_ORF_STOP3 = 1", "NAF_GPU_ORF_STOP5 = 2", "NAF_GPU_ORF_SPLIT_UNKNOWN = 1", "NAF_GPU_ORF_CLOSED = 2", "naf_gpu_parse_codon_set",
                 "naf_gpu_unnaf_orfs_count", "NAF_GPU_ORFS_PIECE", "ORFfinder", "EMBOSS", "uint16_t frame, flags"):
        assert word in header, word


def test_orfs_to_segments():
    from naf_amd import capi
    rows = np.array([(3, 10, 40, 0, 1, 1), (3, 10, 40, 1, 0, 1), (4, 0, 9, 0, 0, 2), (5, 6, 12, 1, 2, 0)], dtype=OP.ORF_DTYPE)
    assert capi.orfs_to_segments(rows) == [(3, 10, 40, 0), (3, 10, 40, 1), (4, 0, 9, 0), (5, 6, 12, 1)]
    assert capi.orfs_to_segments(rows, include_stop=True) == [(3, 10, 43, 0), (3, 7, 40, 1), (4, 0, 9, 0), (5, 6, 12, 1)]


# ---- 4. the command line, before the device is opened -------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [(["--orfs", "--min-orf", "0"], b"--min-orf parameter"), (["--orfs", "--min-orf", "x"], b"--min-orf parameter"),
                                       (["--orfs", "--min-orf", ""], b"--min-orf parameter"), (["--orfs", "--min-orf", "-3"], b"--min-orf parameter"),
                                       (["--orfs", "--min-orf", "99999999999999999999"], b"--min-orf parameter"),
                                       (["--orfs", "--stops", "TA"], b"--stops parameter"), (["--orfs", "--stops", ""], b"--stops parameter"), (["--orfs", "--stops", "TAA,"], b"--stops parameter"),
                                       (["--orfs", "--stops", "TA-"], b"--stops parameter"), (["--orfs", "--starts", "ATGG"], b"--starts parameter"), (["--orfs", "--starts", "AXG"], b"--starts parameter"),
                                       (["--orfs", "--stops", "TAA", "--stops", "TAG"], b"only one --stops"), (["--orfs", "--starts", "ATG", "--starts", "GTG"], b"only one --starts"),
                                       (["--orfs", "--starts", "TAA"], b"share a codon"), (["--orfs", "--stops", "ATG"], b"share a codon"), (["--orfs", "--stops", "NNN"], b"share a codon"),
                                       (["--orfs", "--stop-to-stop", "--starts", "ATG"], b"--stop-to-stop and --starts"),
                                       (["--orfs", "--strand", "x"], b"--strand parameter"),
                                       (["--min-orf", "30"], b"--min-orf can be used only with --orfs"), (["--stops", "TAA"], b"--stops can be used only with --orfs"),
                                       (["--starts", "ATG"], b"--starts can be used only with --orfs"), (["--stop-to-stop"], b"--stop-to-stop can be used only with --orfs"),
                                       (["--closed"], b"--closed can be used only with --orfs"), (["--split-unknown"], b"--split-unknown can be used only with --orfs"),
                                       (["--runs", "N", "--closed"], b"--closed can be used only with --orfs"), (["--strand", "+"], b"--strand can be used only with"),
                                       (["--orfs", "--fasta"], b"no output type"), (["--seq", "--orfs"], b"no output type"), (["--orfs", "--ids"], b"no output type"),
                                       (["--orfs", "--locate", "NGG"], b"--orfs and --locate"), (["--orfs", "--composition"], b"--orfs and --composition"),
                                       (["--orfs", "--quality"], b"--orfs and --quality"), (["--orfs", "--runs", "N"], b"--orfs and --runs"),
                                       (["--masked-runs", "--orfs"], b"--orfs and --masked-runs"), (["--kmers", "4", "--orfs"], b"--orfs and --kmers"),
                                       (["--orfs", "--records", "1-2", "--records", "3-4"], b"one --records or one --region"),
                                       (["--orfs", "--region", "x:1-5"], b"whole sequence"), (["--orfs", "--rc-region", "x"], b"--rc-region can't"),
                                       (["--orfs", "--region", "x", "--revcomp"], b"--revcomp can't")])
def test_orfs_arguments_are_checked_on_the_command_line(args, word):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and p.stderr.count(b"\n") == 1
    assert word in p.stderr and b"unknown or incomplete" not in p.stderr, p.stderr      # the check of this option, not the one for an option nobody knows


@pytest.mark.parametrize("opt", ["--min-orf", "--stops", "--starts"])
def test_an_orfs_option_without_its_value_is_a_usage_error(opt):
    p = subprocess.run([os.path.join(BIN, "unnaf"), "-c", "--orfs", opt], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: ") and opt.encode() in p.stderr


def test_help_gains_the_orf_lines():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--orfs" not in head
    for line in (b"\n  --orfs ", b"\n  --min-orf N ", b"\n  --stops LIST ", b"\n  --starts LIST ", b"\n  --stop-to-stop ", b"\n  --closed ", b"\n  --split-unknown "):
        assert line in tail, line
    assert tail.index(b"\n  --kmers K ") < tail.index(b"\n  --orfs ")
    assert b"default 75" in tail and b"TAA,TAG,TGA" in tail and b"default ATG" in tail


# ---- 5. the texts decode to what the plan says --------------------------------------------------------------------------------------------
def test_the_planned_texts_through_the_oracle(oracle, planned):
    for c in planned.values():
        naf = oracle.ennaf(c.text, c.seq_type, well_formed=c.well_formed)
        h = oracle.parse_naf(naf)
        lines = OP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), h.n_sequences)
        if c.r7:
            assert sum(len(x) for x in lines) < h.orig[oracle.SEQ]                    # bases behind the last record
        else:
            assert [x.decode("latin1") for x in lines] == c.records, c.name
        if c.name.startswith("seams"):
            assert (h.orig[oracle.SEQ] + 1) // 2 == 300001 > 2 * 131072               # packed bytes: two whole raw blocks of 128 KiB and a third
        if c.own_text:                                                              # what this build's ennaf archives instead: the same reads without the empty ones
            naf = oracle.ennaf(c.own_text, c.seq_type)
            lines = OP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), oracle.parse_naf(naf).n_sequences)
            assert [x.decode("latin1") for x in lines] == c.own_records == [r for r in c.records if r] and "" in c.records
