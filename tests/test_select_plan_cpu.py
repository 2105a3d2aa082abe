"""tests/select_plan.py held to what it claims, with the oracle alone: every cell of its coverage table filled, the structure of its
texts as the oracle's decoder shows it, the twin property of its ids, the arithmetic of its far-apart intervals, and its expectation
builder against a second, plain walk of the oracle's text."""
from collections import defaultdict
from functools import lru_cache

import numpy as np
import pytest

import select_plan as SP
from select_plan import FASTA, FASTQ, SEQ, SEQUENCES

SEAM_TEXTS = ("dna_seams", "rna_seams", "protein_seams", "text_seams", "fastq_seams")


@lru_cache(maxsize=None)
def archive(name, seed=0):
    from oracle import oracle as O
    T = SP.TEXTS[name](seed)
    return O.ennaf(T.data, T.seq_type, well_formed=T.fastq)               # (a read of no bases: select_plan.fastq_seams)


@lru_cache(maxsize=64)
def records(name, mode, use_mask=True, ll=-1, seed=0):
    from oracle import oracle as O
    return SP.Records(O, archive(name, seed), mode, use_mask, ll)


# ---- 1. the coverage table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SP.SEEDS)
def test_every_cell_of_the_coverage_table_is_filled(seed, capsys):
    cov, want = SP.coverage(seed), SP.expected_cells()
    assert len(set(want)) == len(want) and set(cov) <= set(want), sorted(set(cov) - set(want))[:10]
    if seed == 0:
        rows = defaultdict(lambda: [0, 0, 0])                  # (class, text) -> cells, filled, placements
        for c in want:
            row = rows[(c[0], c[1][0])]
            row[0] += 1; row[1] += cov[c] > 0; row[2] += cov[c]
        with capsys.disabled():
            print("\n%-8s %-14s %6s %6s %10s" % ("class", "text", "cells", "filled", "placements"))
            for (cls, text), (n, f, p) in sorted(rows.items()):
                print("%-8s %-14s %6d %6d %10d" % (cls, text, n, f, p))
            print("cells %d, filled %d" % (len(want), sum(cov[c] > 0 for c in want)))
    assert [c for c in want if not cov[c]] == []


def test_the_classes_run_on_the_texts_the_plan_names():
    assert set(SP.CLASSES_OF) == set(SP.TEXTS) == set(SP.MAKERS_OF)
    assert set(c for v in SP.CLASSES_OF.values() for c in v) == set(SP.GENERATORS)
    assert all(SP.MAKERS_OF[n] == ("oracle", "own") for n in SEAM_TEXTS)


# ---- 2. the structure of the texts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SEAM_TEXTS)
def test_the_oracle_gives_the_text_back_and_the_record_table_is_the_plans(oracle, name):
    T = SP.TEXTS[name](0)
    naf = archive(name)
    h = oracle.parse_naf(naf)
    assert h.seq_type == T.seq_type and h.n_sequences == T.N
    mode = FASTQ if T.fastq else FASTA
    assert oracle.unnaf(naf, mode) == T.data                                            # (every text is in the form the decoder writes)
    if not T.fastq:
        assert h.line_length == T.width == 60
    R = records(name, SEQUENCES)
    assert [len(b) for b in R.bases] == T.lens and R.ids == [r[0] for r in T.recs]
    if oracle.have_ref():
        assert oracle.ref_unnaf(naf, ["--fastq"] if T.fastq else ["--fasta"]) == T.data
        assert oracle.ref_unnaf(naf, ["--sequences"]) == oracle.unnaf(naf, SEQUENCES)


def test_letters_move_with_the_seed_and_structure_does_not():
    for name in SEAM_TEXTS:
        a, b = SP.TEXTS[name](0), SP.TEXTS[name](1)
        assert a.lens == b.lens and [r[:2] for r in a.recs] == [r[:2] for r in b.recs] and a.data != b.data and len(a.data) == len(b.data)
        if a.fourbit and not a.fastq:
            case = lambda T: [((r[2] & 0x20) != 0).tobytes() for r in T.recs if r[0] != b"codes"]
            assert case(a) == case(b)
    assert SP.toggles_of(SP.dna_seams(0)) == SP.toggles_of(SP.dna_seams(2))


@pytest.mark.parametrize("name", ["dna_seams", "rna_seams"])
def test_nucleotide_seam_texts(oracle, name):
    T = SP.TEXTS[name](0)
    R = records(name, SEQUENCES)
    # records start at even and at odd base indices, among them records a 33-base segment fits into
    long_starts = {T.cum[r] % 2 for r in range(T.N) if T.lens[r] > 73}
    long_ends = {T.cum[r + 1] % 2 for r in range(T.N) if T.lens[r] > 73}
    assert long_starts == long_ends == {0, 1}
    assert {T.cum[r] % 2 for r in range(T.N) if T.lens[r] in SP.SMALL_LENGTHS} == {0, 1}
    assert set(SP.SMALL_LENGTHS) <= set(T.lens)
    # empty records first, last and two adjacent in the middle
    e = T.marks["empty_pair"]
    assert T.lens[0] == T.lens[-1] == T.lens[e] == T.lens[e + 1] == 0 and 0 < e < T.N - 2 and T.lens[e - 1] and T.lens[e + 2]
    # the case runs, as the oracle's masked text shows them: 64 single bases, then runs of 2, 3, 15, 16, 17
    s = np.frombuffer(R.bases[T.marks["toggle"]], dtype=np.uint8)
    low = (s >= 97) & (s <= 122)
    edges = np.flatnonzero(low[1:] != low[:-1]) + 1
    runs = np.diff(edges).tolist()
    assert edges[0] == T.marks["alt_at"] == 20 and runs[:63] == [1] * 63
    assert runs[63:] == [1] + [n for n in SP.TOGGLE_RUNS[1:] for _ in range(8)][:-1]      # (the last run of 17 runs on into the record's end)
    assert [(T.cum[T.marks["toggle"]] + int(x)) for x in edges] == [t for t, _ in SP.toggles_of(T)]
    for run in SP.TOGGLE_RUNS:
        assert sum(1 for _, n in SP.toggles_of(T) if n == run) >= 7
    assert R.bases[T.marks["lower"]].islower() and len(R.bases[T.marks["lower"]]) == 100
    codes = R.bases[T.marks["codes"]]
    assert len(set(codes.upper())) == 16 and b"-" in codes and codes[:32].isupper() and codes[32:].replace(b"-", b"").islower()
    assert len(set(codes[:16].translate(R.comp))) == 16


def test_dna_seams_blocks(oracle):
    T = SP.dna_seams(0)
    step = 2 * SP.BLOCK
    seams = list(range(step, T.T, step))
    assert 1_150_000 <= T.T <= 1_300_000 and len(seams) + 1 >= 4
    inside = [s for s in seams if s not in T.cum]
    on = [s for s in seams if s in T.cum]
    assert len(inside) >= 3 and len(on) == 1 and T.lens[T.rec_of(on[0])] > 0 and T.lens[T.rec_of(on[0] - 1)] > 0
    big = T.marks["big"]
    assert T.lens[big] >= 1_000_001 and all(T.rec_of(s) == big for s in inside)
    assert T.cum[T.marks["tail"]] > seams[-1] and T.cum[T.marks["tail"] + 1] == T.T and T.lens[T.marks["tail"]] % 2 == 1
    assert [k for s, k in SP._block_seams(T)].count("own") == 3
    # the archive stores the stream in blocks of that size
    fi = oracle.zstd_frame_info(oracle.parse_naf(archive("dna_seams")).frame(archive("dna_seams"), oracle.SEQ))
    assert fi.n_blocks == fi.n_raw == len(seams) + 1


@pytest.mark.parametrize("name", ["protein_seams", "text_seams"])
def test_byte_seam_texts(oracle, name):
    T = SP.TEXTS[name](0)
    seams = list(range(SP.BLOCK, T.T, SP.BLOCK))
    assert T.T >= 300 * 1024 and len(seams) >= 2 and not T.fourbit
    assert [s for s in seams if s in T.cum] == [SP.BLOCK] and all(T.rec_of(s) == T.marks["big"] for s in seams[1:]) and len(seams) >= 3
    assert T.lens[0] == T.lens[-1] == 0 and set(SP.SMALL_LENGTHS) <= set(T.lens)
    text = records(name, SEQUENCES).text
    if name == "protein_seams":
        assert any(c in text for c in b"acdx") and any(c in text for c in b"ACDX")
    else:
        assert set(text) - {10} == set(range(33, 127)) - {ord(">")}


def test_fastq_seams(oracle):
    T = SP.fastq_seams(0)
    assert tuple(T.lens[:len(SP.READ_LENGTHS)]) == SP.READ_LENGTHS and set(T.lens) == set(SP.READ_LENGTHS) | {150}
    assert sum(1 for k in T.marks["small"] if k > len(SP.READ_LENGTHS)) >= 15 and max(T.marks["small"]) > T.N // 2
    assert T.T > 2 * SP.BLOCK                                                           # two blocks of packed bases, three of qualities
    R = records("fastq_seams", FASTQ)
    assert set(b"".join(R.qual)) == set(range(33, 127)) and b"N" in b"".join(R.bases[:200])
    assert {len(r[0]) % 2 for k, r in enumerate(T.recs) if k in T.marks["small"]} == {0, 1}   # header lengths of both parities: texts of any size


def test_far_intervals_and_the_ranges_they_leave():
    iv = SP.far_intervals()
    gap = SP.SEL_GAP_BLOCKS * SP.BLOCK * 2
    assert gap == 524_288 and len(iv) == SP.FAR_INTERVALS == 36 and all(50 <= n <= 5000 for _, n in iv)
    dist = [b[0] - (a[0] + a[1]) for a, b in zip(iv, iv[1:])]
    assert all(d > gap for d in dist)                                                   # neighbours, so every pair
    assert all(gap < d <= gap + 300 for d in dist[0::2]) and all(2 * gap < d <= 2 * gap + 300 for d in dist[1::2])
    for count, ranges, doublings in ((32, 32, 0), (33, 17, 1), (36, 18, 1)):
        rg, dbl = SP.ranges_after_merging(iv[:count])
        assert (len(rg), dbl) == (ranges, doublings) and 1 < len(rg) <= SP.SEL_MAX_RANGES
        assert rg[0][0] == iv[0][0] and rg[-1][1] == iv[count - 1][0] + iv[count - 1][1]     # the first and the last segment abut a range's g_lo and g_hi
        assert all(any(a == lo for lo, _ in rg) or any(a + n == hi for _, hi in rg) for a, n in iv[:count])
    T = SP.dna_far(0)
    assert T.N == 5 and 27_000_000 <= T.T <= 29_000_000
    for seed in SP.SEEDS:
        for count in (32, 33, 36):
            segs = SP.far_segments(T, count, seed)
            assert sorted(T.g0(s) for s in segs) == [a for a, _ in iv[:count]] and [T.g0(s) for s in segs] != [a for a, _ in iv[:count]]
            assert all(s[2] <= T.lens[s[0]] for s in segs) and {s[3] for s in segs} == {0, 1} and len({s[0] for s in segs}) >= 4


# ---- 3. the ids ------------------------------------------------------------------------------------------------------------------------
def test_ids_and_their_twins(oracle):
    plan = SP.ids_find(0)
    ids = plan.ids
    assert len(ids) == 200 and {len(i) for i in ids} >= set((0,) + SP.ID_SHORT + SP.ID_LONG)
    have = set(ids)
    seen = defaultdict(set)
    for n, p, a, b in plan.twins:
        assert len(a) == len(b) == n and a in have and b not in have and a != b
        assert [k for k in range(n) if a[k] != b[k]] == [p]
        seen[n].add(p)
        base = a[:p] + b"?" + a[p + 1:]
        family = [i for i in ids if len(i) == n and i[:p] + b"?" + i[p + 1:] == base]
        assert len(family) >= 1 + (n > 1)                                                # an archived sibling that differs there too
        if n > 32:
            assert 16 <= p <= n - 17 and all(i[:16] == a[:16] and i[-16:] == a[-16:] for i in family + [b])
    for n in SP.ID_LONG:
        assert {16, n - 17} <= seen[n]
        assert seen[n] >= {p for p in (1023, 1024, 2047, 2048) if 16 <= p <= n - 17}
    assert seen[5000] == {16, 1023, 1024, 2047, 2048, 4983}
    for n in SP.ID_SHORT:
        assert seen[n] == {p for p in (0, 7, 8, 15, 16, n - 1) if p < n}
    first = SP.first_index(ids)
    dup = sorted((k - first[i], len(i)) for k, i in enumerate(ids) if first[i] != k)
    assert len(dup) == 3 and dup[0][0] < 64 and first[ids[63]] // 64 == 63 // 64                    # one wavefront of records
    assert dup[1][0] > 64 and dup[2][0] > 64 and sorted(d[1] > 32 for d in dup[1:]) == [False, True]     # two wavefronts: a short id, and one the wavefront compares
    assert ids.index(b"") > 65
    for n in SP.ID_COUNTS:
        text = SP.id_text(plan, n)
        naf = oracle.ennaf(text)
        assert oracle.zstd_decompress(oracle.parse_naf(naf).frame(naf, 0)).split(b"\0")[:-1] == ids[:n]
        assert len(ids[n - 1]) < 16
        lists = SP.id_queries(plan, n, 0)
        assert [len(q) for q in lists[1:]] == list(SP.QUERY_COUNTS)
        want = SP.first_index(ids[:n])
        everything = lists[0]
        assert set(ids) | set(plan.absent) | {b""} <= set(everything) and len(everything) > len(set(everything))
        assert sum(1 for q in everything if q in want) >= n and sum(1 for q in everything if q not in want) >= len(plan.absent)
        assert (b"" in want) == (n == 200)
        assert all(any(len(x) > 32 and x not in want for x in q) for q in lists[1:])


# ---- 4. the expectation builder against a second walk -------------------------------------------------------------------------------
def plain_segment(bases, ident, begin, end, L, mark=b""):
    """A sub-range's FASTA text, a byte at a time."""
    out = bytearray(b">" + ident + b":" + str(begin + 1).encode() + b"-" + str(min(end, len(bases))).encode() + mark + b"\n")
    col = 0
    for k in range(begin, min(end, len(bases))):
        out.append(bases[k]); col += 1
        if L and col == L:
            out.append(10); col = 0
    if col or not L:
        out.append(10)
    return bytes(out)


@pytest.mark.parametrize("name", SEAM_TEXTS)
def test_whole_forward_segments_laid_end_to_end_are_the_oracles_text(oracle, name):
    T = SP.TEXTS[name](0)
    naf = archive(name)
    views = [(FASTQ, True, -1)] if T.fastq else [(FASTA, True, -1), (FASTA, False, 0), (FASTA, True, 17), (FASTA, True, 2 ** 32)]
    for mode, um, ll in views + [(SEQUENCES, True, -1), (SEQUENCES, False, -1), (SEQ, True, -1)]:
        R = records(name, mode, um, ll)
        assert R.expect([(r, 0, None, 0) for r in range(R.n)]) == oracle.unnaf(naf, mode, um, ll), (mode, um, ll)
        L = T.width if ll < 0 else ll
        assert [len(w) for w in R.whole] == [T.size((r, 0, None, 0), mode, L) for r in range(T.N)]
    for ll in SP.HUGE_L:
        assert oracle.unnaf(naf, FASTA, True, ll) == oracle.unnaf(naf, FASTA, True, 0) or T.fastq


@pytest.mark.parametrize("name", ["dna_seams", "rna_seams", "fastq_seams"])
def test_a_reverse_segment_reversed_again_is_the_forward_one(name):
    T = SP.TEXTS[name](0)
    if T.fastq:
        R = records(name, FASTQ)
        for r in T.marks["small"][:30] + [T.N - 1]:
            f, v = R.segment(r, 0, None, 0).split(b"\n"), R.segment(r, 0, None, 1).split(b"\n")
            assert v[1].translate(R.comp)[::-1] == f[1] and v[3][::-1] == f[3] and v[2] == f[2] == b"+" and len(v) == 5
            assert v[0] == b"@" + R.ids[r] + b"/rc" + f[0][1 + len(R.ids[r]):]
        return
    R, F = records(name, SEQ), records(name, FASTA)
    segs = [s for c in SP.cases_of(name, "parity", 0) + SP.cases_of(name, "toggle", 0)[:2] for s in c.segs if s[3]]
    assert len(segs) > 500
    for r, b, e, _ in segs:
        fwd = R.segment(r, b, e, 0)
        assert R.segment(r, b, e, 1).translate(R.comp)[::-1] == fwd
        if e is not None:                                                                # the header and the wrapping of the reversed bases, a byte at a time
            n = len(fwd)
            plain = plain_segment(R.segment(r, b, e, 1), b"", 0, n, 60)
            assert plain.startswith(b">:1-%d\n" % n)
            assert F.segment(r, b, e, 1) == b">%s:%d-%d/rc\n" % (R.ids[r], b + 1, b + n) + plain[len(b">:1-%d\n" % n):]


@pytest.mark.parametrize("name", ["dna_seams", "protein_seams"])
def test_sub_range_wrapping_against_a_byte_at_a_time_loop(name):
    T = SP.TEXTS[name](0)
    big = T.marks["big"]
    for ll in (-1, 0, 1, 2, 15, 16, 17, 2 ** 32 - 1, 2 ** 62):
        R = records(name, FASTA, True, ll)
        L = T.width if ll < 0 else ll
        for b, n in ((0, 1), (7, 59), (7, 60), (7, 61), (1001, 121), (99_999, 34), (T.lens[big] - 5, 9), (3, 17), (3, 32)):
            assert R.segment(big, b, b + n, 0) == plain_segment(R.bases[big], R.ids[big], b, b + n, L), (ll, b, n)


@pytest.mark.parametrize("name", list(SP.CLASSES_OF))
def test_the_plans_sizes_and_features_are_the_expectations(name):
    """The arithmetic the generators place things with (Text.size, Text.layout) against the bytes of the expectation."""
    if name == "dna_far":
        T = SP.dna_far(0)
        for c in SP.cases_of(name, "far", 0):
            assert all(0 <= s[1] < s[2] <= T.lens[s[0]] for s in c.segs)
        return
    T = SP.TEXTS[name](0)
    mark = {"hdr_first": b">@", "hdr_last": b"\n", "line_end": b"\n"}
    n_cases = n_feats = 0
    for cls in SP.CLASSES_OF[name]:
        for k, c in enumerate(SP.cases_of(name, cls, 0)):
            if cls == "phase" and k % 3 and "total" not in c.label:
                continue                                                                 # (a third of them: the arithmetic is the same)
            R = records(name, c.mode, c.use_mask, c.ll)
            L = T.line_length(c)
            assert all(0 <= s[1] and (s[2] is None or s[1] < min(s[2], T.lens[s[0]])) for s in c.segs), c.label
            want = R.expect(c.segs)
            feats, total = T.layout(c)
            assert total == len(want) == sum(T.size(s, c.mode, L) for s in c.segs), c.label
            for kind, x in feats:
                if kind in mark:
                    assert want[x] in mark[kind], (c.label, kind, x)
                elif kind == "last_base":
                    assert want[x] != 10 and (x + 1 == total or want[x + 1] == 10 or c.mode == SEQ), (c.label, x)
            n_cases += 1; n_feats += len(feats)
    assert n_cases >= 10 and n_feats >= 100


def test_the_crowd_holds_the_runs_of_zero_size_segments_it_names():
    T = SP.dna_seams(0)
    cases = SP.cases_of("dna_seams", "crowd", 0)
    many = next(c for c in cases if "tile seam" in c.label)
    z = [T.nb(s) == 0 for s in many.segs]
    runs, k = [], 0
    while k < len(z):
        j = k
        while j < len(z) and z[j] == z[k]:
            j += 1
        if z[k]:
            runs.append((k, j - k))
        k = j
    assert runs[0][0] == 0 and runs[-1][0] + runs[-1][1] == len(z) and sorted(n for _, n in runs[1:-1]) == [1, 2, 70]
    assert all(T.nb(s) <= 1 for s in many.segs) and T.layout(many)[1] > SP.TILE + 64
    by_S = {len(c.segs) for c in cases if c.label.endswith("segments")}
    assert by_S == set(SP.CROWD_S)
    only = next(c for c in cases if c.label.startswith("nothing"))
    assert T.layout(only)[1] == 0 and len(only.segs) > 32
