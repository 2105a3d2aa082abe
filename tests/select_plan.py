"""What to select for the tests of the selection path (tests/test_gpu_select_plan.py, tests/test_select_plan_cpu.py): texts whose
structure is fixed (record lengths, case runs, empty records, ids) and whose letters move with the seed, lists of segments that put a
segment's first and last base, a header's digits, a line end, a mask toggle and a zero-size segment at every phase of every seam
naf_amd/csrc/emit_select.h has -- nibble pair, 16-byte chunk, 1 KiB round, 4 KiB tile, 128 KiB stream block, merged range, wavefront of
64 ids -- and the expectation: the text of a segment, cut in Python out of the oracle's whole text of the archive under test.
Nothing here touches the GPU or the code under test; it imports the oracle, numpy and the standard library.

A list is a Case: the segments (record, begin, end or None for the whole record, strand) of ONE select call with its mode, mask flag and
line length.  Every generator also records the cells (class, phase) it fills, worked out from the geometry of what it emitted (the
output offsets are sums of segment sizes, restated here as arithmetic over the record table), not from what it meant to emit;
expected_cells() lists what must be filled and tests/test_select_plan_cpu.py holds the one to the other."""
import os
from collections import Counter, namedtuple
from functools import lru_cache

import numpy as np

from oracle import oracle as O

FASTA, FASTQ, SEQ, SEQUENCES = O.MODE_FASTA, O.MODE_FASTQ, O.MODE_SEQ, O.MODE_SEQUENCES
MODE_NAME = {FASTA: "fasta", FASTQ: "fastq", SEQ: "seq", SEQUENCES: "sequences"}
SEED = int(os.environ.get("NAF_TEST_SEED", "0"))          # other letters in the same structure: NAF_TEST_SEED=n python -m pytest ...
SEEDS = (0, 1, 2)
CHUNK, ROUND, TILE, BLOCK = 16, 1024, 4096, 131072        # bytes of output (chunk, round, tile) and of a stored stream (block)
OWN_BLOCK = 32768                                         # block of this build's own frames
SEL_MAX_RANGES, SEL_GAP_BLOCKS = 32, 2                    # the rule of emit_select.h's header comment, restated for the arithmetic of `far`
HUGE_L = (2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 62)
LINE_LENGTHS = (-1, 0, 1, 2, 15, 16, 17, 4095, 4096) + HUGE_L          # -1: the stored one
SMALL_LENGTHS = (1, 15, 16, 17, 31, 32, 33)
TOGGLE_RUNS = (1, 2, 3, 15, 16, 17)
READ_LENGTHS = tuple(range(19)) + (31, 32, 33)
CROWD_S = (1, 31, 32, 33, 255, 256, 257)                  # block sizes of k_select_hdr (32 segments) and k_select_layout (256)

COMP_DNA = bytes.maketrans(b"ACGTMRWSYKVHDBN-acgtmrwsykvhdbn-", b"TGCAKYWSRMBDHVN-tgcakywsrmbdhvn-")
COMP_RNA = bytes.maketrans(b"ACGUMRWSYKVHDBN-acgumrwsykvhdbn-", b"UGCAKYWSRMBDHVN-ugcakywsrmbdhvn-")

Case = namedtuple("Case", "label mode use_mask ll segs")


# ---- the expectation, from the oracle's whole text -------------------------------------------------------------------------------
class Records:
    """The records of an archive as the oracle prints them under (mode, use_mask, line_length), and from them the text of a segment:
    forward for every sequence type, on either strand for DNA and RNA."""

    def __init__(self, oracle, naf, mode, use_mask=True, line_length=-1):
        h = oracle.parse_naf(naf)
        self.mode, self.has_ids = mode, bool(h.flags & 0x20)
        self.comp = COMP_RNA if h.seq_type == 1 else COMP_DNA if h.seq_type == 0 else None
        self.L = line_length if line_length >= 0 else h.line_length
        self.ids = oracle.zstd_decompress(h.frame(naf, 0)).split(b"\0")[:-1] if self.has_ids else [b""] * h.n_sequences
        self.text = oracle.unnaf(naf, FASTQ if mode == FASTQ else FASTA if mode == FASTA else SEQUENCES, use_mask, line_length)
        self.whole, self.bases, self.head, self.plus, self.qual = [], [], [], [], []
        t = self.text
        if mode == FASTQ:
            lines = t.split(b"\n")[:-1]
            assert len(lines) == 4 * h.n_sequences
            for k in range(0, len(lines), 4):
                self.whole.append(b"\n".join(lines[k:k + 4]) + b"\n")
                self.head.append(lines[k]); self.bases.append(lines[k + 1]); self.plus.append(lines[k + 2]); self.qual.append(lines[k + 3])
        elif mode == FASTA:
            lens = [len(x) for x in oracle.unnaf(naf, SEQUENCES, use_mask, line_length).split(b"\n")[:-1]]
            assert len(lens) == h.n_sequences
            a = 0
            for ln in lens:
                assert t[a:a + 1] == b">"
                body = t.index(b"\n", a) + 1
                b = body + (0 if ln == 0 else ln + ((ln + self.L - 1) // self.L if self.L else 1))
                self.whole.append(t[a:b]); self.head.append(t[a:body - 1]); self.bases.append(t[body:b].replace(b"\n", b"")); a = b
                assert len(self.bases[-1]) == ln
            assert a == len(t)
        else:
            lines = t.split(b"\n")[:-1]
            assert len(lines) == h.n_sequences
            for ln in lines:
                self.bases.append(ln); self.whole.append(ln + (b"\n" if mode == SEQUENCES else b""))
        self.n = len(self.whole)

    def wrap(self, s):
        if not s:
            return b""
        if self.L == 0 or self.L >= len(s):
            return s + b"\n"
        return b"".join(s[i:i + self.L] + b"\n" for i in range(0, len(s), self.L))

    def segment(self, rec, begin=0, end=None, reverse=0):
        whole = begin == 0 and end is None
        if whole and not reverse:
            return self.whole[rec]
        s = self.bases[rec] if whole else self.bases[rec][begin:min(end, len(self.bases[rec]))]
        assert whole or s, "the test asks for an empty sub-range"
        if reverse:
            assert self.comp is not None, "protein and text have no reverse complement"
            s = s.translate(self.comp)[::-1]
        if self.mode == SEQ:
            return s
        if self.mode == SEQUENCES:
            return s + b"\n"
        mark = b"/rc" if reverse else b""
        if whole:                                            # (reverse) '>' id "/rc", then what the stored line has behind the id; without ids the stored line, then "/rc"
            hd = self.head[rec]
            if self.has_ids:
                assert hd[1:1 + len(self.ids[rec])] == self.ids[rec]
                hd = hd[:1 + len(self.ids[rec])] + mark + hd[1 + len(self.ids[rec]):]
            else:
                hd = hd + mark
            if self.mode == FASTQ:
                return hd + b"\n" + s + b"\n" + self.plus[rec] + b"\n" + self.qual[rec][::-1] + b"\n"
            return hd + b"\n" + self.wrap(s)
        assert self.mode == FASTA
        return b">" + self.ids[rec] + b":%d-%d" % (begin + 1, begin + len(s)) + mark + b"\n" + self.wrap(s)

    def expect(self, segs):
        return b"".join(self.segment(*s) for s in segs)


# ---- the texts ---------------------------------------------------------------------------------------------------------------------
def _letters(rng, n, alphabet):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)]


def _wrap(b, width):
    """The letters b in lines of `width` (0: one line); nothing for no letters."""
    n = len(b)
    if n == 0:
        return b""
    if not width:
        return b.tobytes() + b"\n"
    out = np.full(n + -(-n // width), 10, dtype=np.uint8)
    idx = np.arange(n)
    out[idx + idx // width] = b
    return out.tobytes()


def _case_runs(b, fixed, every, longest):
    """Lower-case runs of 1 .. longest letters about every `every`, at places that do not move with the seed."""
    b = b.copy()
    at = int(fixed.integers(1, every))
    while at < len(b) - longest - 1:
        n = int(fixed.integers(1, longest + 1))
        b[at:at + n] |= 0x20
        at += n + int(fixed.integers(1, 2 * every))
    return b


class Text:
    """A text as its records (id, name, letters) and the arithmetic the generators need: first base of a record in the stream, the
    sizes of a segment's header and text under a mode and a line length."""

    def __init__(self, name, seq_type, recs, width=60, quals=None, marks=None):
        self.name, self.seq_type, self.recs, self.width, self.quals = name, seq_type, recs, width, quals
        self.fastq = quals is not None
        self.fourbit = seq_type <= O.RNA
        self.per_byte = 2 if self.fourbit else 1
        self.lens = [len(r[2]) for r in recs]
        self.cum = [0]
        for n in self.lens:
            self.cum.append(self.cum[-1] + n)
        self.T = self.cum[-1]
        self.N = len(recs)
        self.marks = marks or {}                             # named records and positions: "big", "toggle", ...
        self._data = None

    @property
    def data(self):
        if self._data is None:
            out = []
            for k, (i, nm, b) in enumerate(self.recs):
                hd = i + (b" " + nm if nm or not i else b"")
                if self.fastq:
                    out.append(b"@" + hd + b"\n" + b.tobytes() + b"\n+\n" + self.quals[k].tobytes() + b"\n")
                else:
                    out.append(b">" + hd + b"\n" + _wrap(b, self.width))
            self._data = b"".join(out)
        return self._data

    def modes(self):
        return (FASTQ,) if self.fastq else (FASTA, SEQUENCES, SEQ)

    def rec_of(self, g):
        """The record that holds base g of the stream (the last one that starts at or before it and is not empty)."""
        r = int(np.searchsorted(self.cum, g, side="right")) - 1
        assert 0 <= r < self.N and self.cum[r] <= g < self.cum[r + 1], (g, r)
        return r

    def g0(self, seg):
        return self.cum[seg[0]] + seg[1]

    def nb(self, seg):
        r, b, e, _ = seg
        return self.lens[r] if e is None else min(e, self.lens[r]) - b

    def hl(self, seg, mode):
        if mode not in (FASTA, FASTQ):
            return 0
        r, b, e, rv = seg
        i, nm, _ = self.recs[r]
        if e is None:
            h = 1 + len(i) + (1 + len(nm) if nm else 0) + 1
        else:
            h = 1 + len(i) + 1 + len(str(b + 1)) + 1 + len(str(min(e, self.lens[r]))) + 1
        return h + (3 if rv else 0)

    def size(self, seg, mode, L):
        n, h = self.nb(seg), self.hl(seg, mode)
        if mode == FASTQ:
            return h + 2 * n + 4
        if mode == SEQUENCES:
            return n + 1
        if mode == SEQ:
            return n
        return h + (n + (-(-n // L) if L else 1) if n else 0)

    def line_length(self, case):
        return self.width if case.ll < 0 else case.ll

    def layout(self, case):
        """Where the features of a list's text stand: (kind, offset) for a header's first and last byte, every line end, a segment's
        last base and the first byte of every segment but the first; and the size of the text."""
        mode, L, off, feats = case.mode, self.line_length(case), 0, []
        for seg in case.segs:
            h, n, sz = self.hl(seg, mode), self.nb(seg), self.size(seg, mode, L)
            if off and sz:
                feats.append(("boundary", off))
            if h:
                feats += [("hdr_first", off), ("hdr_last", off + h - 1)]
            if mode == FASTA and n:
                if L:
                    feats += [("line_end", off + h + k * (L + 1) - 1) for k in range(1, min(n // L, 200) + 1) if k * L < n]
                feats += [("line_end", off + sz - 1), ("last_base", off + sz - 2)]
            elif mode == SEQUENCES:
                feats += [("line_end", off + n)] + ([("last_base", off + n - 1)] if n else [])
            elif mode == SEQ and n:
                feats.append(("last_base", off + n - 1))
            elif mode == FASTQ:
                feats += [("line_end", off + h + n), ("line_end", off + h + n + 2), ("line_end", off + sz - 1)] + ([("last_base", off + h + n - 1)] if n else [])
            off += sz
        return feats, off


def _small_records(rng, alphabet, codes):
    """The records every nucleotide text begins with: an empty one, records of 1 .. 33 letters, the toggle record, an all-lower-case one,
    one of all sixteen codes, two adjacent empty ones.  -> records, marks."""
    recs = [(b"e0", b"empty first", _letters(rng, 0, alphabet))]
    for n in SMALL_LENGTHS:
        recs.append((b"s%d" % n, b"len %d" % n, _letters(rng, n, alphabet)))
    # 20 upper, 64 that alternate from base to base (the first lower), eight runs each of 2, 3, 15, 16 and 17, 20 upper
    lower = [False] * 20 + [k % 2 == 0 for k in range(64)]
    state = True
    for run in TOGGLE_RUNS[1:]:
        for _ in range(8):
            lower += [state] * run
            state = not state
    lower += [False] * 20
    b = _letters(rng, len(lower), alphabet) | (np.asarray(lower, dtype=np.uint8) << 5)
    marks = {"toggle": len(recs), "alt_at": 20}
    recs.append((b"tog", b"case runs", b.astype(np.uint8)))
    marks["lower"] = len(recs)
    recs.append((b"low", b"", _letters(rng, 100, alphabet) | 0x20))
    marks["codes"] = len(recs)
    c = np.frombuffer(codes * 2 + codes.lower() * 2, dtype=np.uint8)
    recs.append((b"codes", b"all sixteen", c.copy()))
    marks["empty_pair"] = len(recs)
    recs += [(b"e1", b"", _letters(rng, 0, alphabet)), (b"e2", b"second of two", _letters(rng, 0, alphabet))]
    return recs, marks


@lru_cache(maxsize=None)
def dna_seams(seed):
    rng, fixed = np.random.default_rng(7000 + seed), np.random.default_rng(7000)
    recs, marks = _small_records(rng, b"ACGT", b"ACGTMRWSYKVHDBN-")
    at = sum(len(r[2]) for r in recs)
    marks["pad"] = len(recs)
    recs.append((b"pad", b"up to the first seam", _case_runs(_letters(rng, 2 * BLOCK - at, b"ACGTN"), fixed, 3000, 90)))
    marks["big"] = len(recs)
    recs.append((b"big", b"a million and ten", _case_runs(_letters(rng, 1_000_010, b"ACGT"), fixed, 5000, 200)))
    marks["tail"] = len(recs)
    recs.append((b"tail", b"", _case_runs(_letters(rng, 4097, b"ACGTRYN"), fixed, 300, 40)))
    recs.append((b"e3", b"empty last", _letters(rng, 0, b"ACGT")))
    return Text("dna_seams", O.DNA, recs, 60, marks=marks)


@lru_cache(maxsize=None)
def rna_seams(seed):
    rng, fixed = np.random.default_rng(7100 + seed), np.random.default_rng(7100)
    recs, marks = _small_records(rng, b"ACGU", b"ACGUMRWSYKVHDBN-")
    marks["big"] = marks["pad"] = len(recs)
    recs.append((b"pad", b"forty thousand and one", _case_runs(_letters(rng, 40001, b"ACGUN"), fixed, 500, 60)))
    marks["tail"] = len(recs)
    recs.append((b"tail", b"", _case_runs(_letters(rng, 97, b"ACGU"), fixed, 20, 5)))
    recs.append((b"e3", b"empty last", _letters(rng, 0, b"ACGU")))
    return Text("rna_seams", O.RNA, recs, 60, marks=marks)


def _bytes_seams(name, seq_type, alphabet, seed, salt):
    rng = np.random.default_rng(salt + seed)
    recs = [(b"e0", b"empty first", _letters(rng, 0, alphabet))]
    for n in SMALL_LENGTHS:
        recs.append((b"s%d" % n, b"len %d" % n, _letters(rng, n, alphabet)))
    marks = {"empty_pair": len(recs)}
    recs += [(b"e1", b"", _letters(rng, 0, alphabet)), (b"e2", b"second of two", _letters(rng, 0, alphabet))]
    at = sum(len(r[2]) for r in recs)
    marks["pad"] = len(recs)
    recs.append((b"pad", b"up to the first seam", _letters(rng, BLOCK - at, alphabet)))
    marks["big"] = len(recs)
    recs.append((b"big", b"holds the second and the third seam", _letters(rng, 280_000, alphabet)))
    marks["tail"] = len(recs)
    recs.append((b"tail", b"", _letters(rng, 701, alphabet)))
    recs.append((b"e3", b"empty last", _letters(rng, 0, alphabet)))
    return Text(name, seq_type, recs, 60, marks=marks)


@lru_cache(maxsize=None)
def protein_seams(seed):
    return _bytes_seams("protein_seams", O.PROTEIN, b"ACDEFGHIKLMNPQRSTVWYacdefghiklmnxX*", seed, 7200)


@lru_cache(maxsize=None)
def text_seams(seed):
    return _bytes_seams("text_seams", O.TEXT, bytes(c for c in range(33, 127) if c != ord(">")), seed, 7300)


@lru_cache(maxsize=None)
def fastq_seams(seed, zero=True):
    """zero=False: the same reads without the empty ones.  A read of no bases has a form only the oracle's well-formed parser takes
    (the tolerant one, which this build's ennaf follows, skips the blank quality line), so this build archives the text without."""
    rng = np.random.default_rng(7400 + seed)
    lens, small = list(READ_LENGTHS), []
    for k in range(1900):
        if k % 100 == 50:
            lens.append(READ_LENGTHS[(k // 100) % len(READ_LENGTHS)])
        lens.append(150)
    if not zero:
        lens = [n for n in lens if n]
    front = len(READ_LENGTHS) - (not zero)
    recs, quals, k150 = [], [], 0
    for k, n in enumerate(lens):
        if n == 150:
            i, nm = b"r%04d" % k150, (b"x" if k150 % 7 == 3 else b"")
            k150 += 1
        else:
            i, nm = b"q%d" % n if k < front else b"m%d.%d" % (n, k), (b"short read" if n % 5 == 0 else b"")
            small.append(k)
        recs.append((i, nm, _letters(rng, n, b"ACGTACGTACGTN")))
        q = _letters(rng, n, bytes(range(33, 127)))
        if n == 150:
            q[:94] = (np.arange(94) + k) % 94 + 33                      # every printable code in every long read
        quals.append(q)
    return Text("fastq_seams", O.DNA, recs, 0, quals=quals, marks={"small": small, "front": small[:front]})


FAR_INTERVALS = 36


def far_intervals():
    """(g0, n) of the far-apart intervals in the stream of dna_far: 50 .. 5000 bases, each further behind its predecessor's end than
    SEL_GAP_BLOCKS blocks of stream -- alternately just above one such gap and just above two."""
    gap = SEL_GAP_BLOCKS * BLOCK * 2
    fixed = np.random.default_rng(7500)
    out, at = [], 70_001
    for k in range(FAR_INTERVALS):
        n = (50, 5000)[k] if k < 2 else int(fixed.integers(50, 5001))
        out.append((at, n))
        at += n + (gap + 1 + int(fixed.integers(0, 300)) if k % 2 == 0 else 2 * gap + 1 + int(fixed.integers(0, 300)))
    return out


def ranges_after_merging(intervals, per_byte=2):
    """The rule of emit_select.h's header comment as plain arithmetic: sorted intervals at most `gap` apart become one range, and the
    gap doubles until at most SEL_MAX_RANGES remain.  -> ranges, doublings."""
    ivs = sorted((a, a + n) for a, n in intervals)
    gap, doublings = SEL_GAP_BLOCKS * BLOCK * per_byte, 0
    while True:
        rgs = []
        for a, b in ivs:
            if rgs and a <= rgs[-1][1] + gap:
                rgs[-1][1] = max(rgs[-1][1], b)
            else:
                rgs.append([a, b])
        if len(rgs) <= SEL_MAX_RANGES:
            return rgs, doublings
        gap *= 2
        doublings += 1


@lru_cache(maxsize=1)
def dna_far(seed):
    """About 28 M bases in five records whose boundaries lie in the middle of four of the gaps."""
    rng = np.random.default_rng(7500 + seed)
    iv = far_intervals()
    total = iv[-1][0] + iv[-1][1] + 90_003
    cuts = [0] + [(iv[k][0] + iv[k][1] + iv[k + 1][0]) // 2 | 1 for k in (6, 14, 21, 29)] + [total]
    recs = [(b"far%d" % k, b"record %d" % k, _letters(rng, cuts[k + 1] - cuts[k], b"ACGT")) for k in range(5)]
    return Text("dna_far", O.DNA, recs, 80, marks={"intervals": iv})


# ---- the id look-up plan -----------------------------------------------------------------------------------------------------------
ID_SHORT = (1, 7, 8, 9, 15, 16, 17, 31, 32)
ID_LONG = (33, 47, 48, 49, 1023, 1024, 1025, 1039, 1040, 2047, 2048, 2049, 5000)
ID_COUNTS = (63, 64, 65, 200)
QUERY_COUNTS = (1, 8, 9, 16, 17)
_ID_ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_.|"


def twin_positions(n):
    """Where twins of length n differ: a byte that is neither among the first 16 nor among the last 16."""
    if n <= 32:
        return sorted({p for p in (0, 7, 8, 15, 16, n - 1) if p < n})
    return sorted({p for p in (16, n - 17, 1023, 1024, 1024 + 16 * 63 + 15, 2048) if 16 <= p <= n - 17})


def _with(b, p, c):
    return b[:p] + c + b[p + 1:]


IdPlan = namedtuple("IdPlan", "text ids absent twins")


@lru_cache(maxsize=None)
def ids_find(seed):
    """The text of 200 records, its ids in order, the twins that are queried and not archived, and (length, position, archived twin,
    absent twin) of every family."""
    rng = np.random.default_rng(7600 + seed)
    word = lambda n: _letters(rng, n, _ID_ALPHABET).tobytes()
    special, absent, twins = [], [], []
    for n in ID_SHORT + ID_LONG:
        base = word(n)
        if n > 1:
            special.append(base)
        for p in twin_positions(n):
            special.append(_with(base, p, b"#")); absent.append(_with(base, p, b"%"))
            twins.append((n, p, special[-1], absent[-1]))
    plain = lambda: word(int(rng.integers(2, 15)))
    ids = special[:62] + [plain() for _ in range(5)] + special[62:] + [b""]
    ids += [plain() for _ in range(ID_COUNTS[-1] - len(ids))]
    ids[63] = ids[10]                                        # the same id twice within one wavefront of records ...
    ids[150] = ids[5]                                        # ... in two wavefronts, a short one ...
    long_at = next(k for k in range(67, 95) if len(ids[k]) >= 1024)
    ids[170] = ids[long_at]                                  # ... and one the wavefront compares
    recs = [(i, b"n%d" % k, _letters(rng, int(rng.integers(10, 51)), b"ACGT")) for k, i in enumerate(ids)]
    return IdPlan(Text("ids_find", O.DNA, recs, 60), ids, absent, twins)


def id_text(plan, n):
    """The first n records of the id text."""
    return Text("ids_find_%d" % n, O.DNA, plan.text.recs[:n], 60).data


def first_index(ids):
    d = {}
    for k, i in enumerate(ids):
        d.setdefault(i, k)
    return d


def id_queries(plan, n, seed):
    """The query lists against the first n records: everything at once (every id of the whole text, every absent twin, prefixes,
    one-byte extensions, the empty id, repeats), then lists of 1, 8, 9, 16 and 17 queries that hold a long twin each."""
    rng = np.random.default_rng(7700 + seed + n)
    ids = plan.ids
    q = list(ids) + list(plan.absent) + [b""]
    q += [i[:-1] for i in ids[::3] if i] + [i + b"Z" for i in ids[1::3]] + [i + i[-1:] for i in ids[2::9] if i]
    q += [ids[k] for k in (0, 0, 61, 199)] + [plan.absent[0], plan.absent[0], b""]
    order = rng.permutation(len(q))
    lists = [[q[k] for k in order]]
    long_twins = [t for t in plan.twins if t[0] > 32]
    for j, c in enumerate(QUERY_COUNTS):
        t = long_twins[(j * 7 + seed) % len(long_twins)]
        lists.append(([t[3], t[2]] + [q[int(k)] for k in rng.integers(0, len(q), c)])[:c] if c > 1 else [t[3]])
    return lists


# ---- segment classes -------------------------------------------------------------------------------------------------------------
def both(seg):
    return [seg[:3] + (0,), seg[:3] + (1,)]


def at_begin(T, g, n):
    """The segment of n bases (clamped to its record) whose first base is base g of the stream."""
    r = T.rec_of(g)
    b = g - T.cum[r]
    return (r, b, min(T.lens[r], b + n), 0)


def at_end(T, g, n):
    """The segment of n bases (clamped) whose last base is base g - 1 of the stream."""
    r = T.rec_of(g - 1)
    e = g - T.cum[r]
    return (r, max(0, e - n), e, 0)


def gen_parity(T, seed, fill):
    rng = np.random.default_rng(7800 + seed)
    segs = []
    for n in range(1, 34):
        for par in (0, 1):
            for place in ("first", "middle", "last"):
                cand = [r for r in range(T.N) if T.lens[r] > n + 40]
                if place == "first":
                    r = next(r for r in cand if T.cum[r] % 2 == par); s = (r, 0, n, 0)
                elif place == "last":
                    r = next(r for r in cand if (T.cum[r + 1] - n) % 2 == par); s = (r, T.lens[r] - n, T.lens[r], 0)
                else:
                    r = cand[int(rng.integers(0, len(cand)))]
                    b = int(rng.integers(20, T.lens[r] - n - 20))
                    b += (T.cum[r] + b + par) % 2
                    s = (r, b, b + n, 0)
                assert T.nb(s) == n and T.g0(s) % 2 == par
                fill("parity", (T.name, n, par, place))
                segs += both(s)
    r = T.marks["toggle"]
    for kind, e in (("len", T.lens[r]), ("len+1", T.lens[r] + 1), ("clamped", T.lens[r] + 1000), ("clamped", 2 ** 63)):
        for n in (1, 9, 16, 17):
            segs += both((r, T.lens[r] - n, e, 0))
        fill("parity", (T.name, "end", kind))
    return [Case("fasta", FASTA, True, -1, segs), Case("seq unmasked", SEQ, False, -1, segs), Case("sequences", SEQUENCES, True, -1, segs[::3])]


def _block_seams(T):
    step = BLOCK * T.per_byte
    out = [(s, "boundary" if s in T.cum else "inside") for s in range(step, T.T, step)]
    own = OWN_BLOCK * T.per_byte
    return out + [(s, "own") for s in (own, 5 * own, (T.T - 1) // own * own) if s % step]


def gen_block(T, seed, fill):
    """One list per placement: a list's intervals are merged into one range before anything is decoded, so a base beside a seam is the
    range's first or last only when its segment stands alone (forward and reverse of the same bases)."""
    cases, lengths, c = [], (1, 2, 17, 300, 5000), seed
    strands = both if T.fourbit else (lambda s: [s])
    if T.fastq:
        for what, step in (("seq", BLOCK * 2), ("qual", BLOCK)):         # (a read has as many quality bytes as bases)
            for s in range(step, T.T, step):
                r = T.rec_of(s)
                for d, rr in (("before", r - 1), ("across", r), ("after", r + 1)):
                    cases.append(Case("%s seam %d read %s" % (what, s, d), FASTQ, True, -1, both((rr, 0, None, 0))))
                    fill("block", (T.name, what, d))
                cases.append(Case("%s seam %d reads around" % (what, s), FASTQ, True, -1, [(rr, 0, None, (rr + seed) & 1) for rr in range(r - 3, r + 4)]))
        return cases
    seams = _block_seams(T)
    for s, kind in seams:
        for d in (-2, -1, 0, 1, 2):
            for side in ("begin", "end"):
                n = lengths[c % len(lengths)]; c += 1
                seg = at_begin(T, s + d, n) if side == "begin" else at_end(T, s + d, n)
                assert T.g0(seg) == s + d if side == "begin" else T.g0(seg) + T.nb(seg) == s + d
                mode = (FASTA, SEQ, SEQUENCES)[c % 3]
                cases.append(Case("%s seam %d %s %+d" % (kind, s, side, d), mode, c % 2 == 0, -1, strands(seg)))
                fill("block", (T.name, kind, side, d))
                fill("block", (T.name, "g_lo odd" if T.g0(seg) & 1 else "g_lo even"))
                fill("block", (T.name, "g_hi odd" if (T.g0(seg) + T.nb(seg)) & 1 else "g_hi even"))
    inside = [s for s, k in seams if k == "inside"]
    a, b = inside[0], inside[1]
    r = T.rec_of(a)
    if T.rec_of(b) == r:
        cases.append(Case("across two seams", FASTA, True, -1, strands((r, a - T.cum[r] - 5, b - T.cum[r] + 5, 0))))
        fill("block", (T.name, "two_seams"))
    r = T.marks["tail"]
    if T.cum[r] > max(s for s, k in seams if k != "own"):
        cases.append(Case("the last block to the last base", FASTA, True, -1, strands((r, 0, T.lens[r], 0)) + strands((r, 0, None, 0))))
        fill("block", (T.name, "last_block"))
    everything = [s for c_ in cases for s in c_.segs if T.nb(s) <= 300]
    cases.append(Case("all placements in one list", FASTA, True, -1, everything))
    return cases


def toggles_of(T):
    """Base indices (in the stream) at which the case changes inside the toggle record, with the length of the run that begins there."""
    r = T.marks["toggle"]
    b = T.recs[r][2]
    low = (b & 0x20) != 0
    t = (np.flatnonzero(low[1:] != low[:-1]) + 1).tolist()
    return [(T.cum[r] + x, (t[k + 1] if k + 1 < len(t) else len(b)) - x) for k, x in enumerate(t)]


def gen_toggle(T, seed, fill):
    tg = toggles_of(T)
    r = T.marks["toggle"]
    segs = []
    for run in TOGGLE_RUNS:
        mine = [t for t, n in tg if n == run]
        for t in (mine[0], mine[(len(mine) // 2 + seed) % len(mine)], mine[-1]):
            for d in (-2, -1, 0, 1, 2):
                segs += both(at_begin(T, t + d, 40)) + both(at_end(T, t + d, 40)) + both(at_begin(T, t + d, 3))
                fill("toggle", (T.name, run, "begin", d)); fill("toggle", (T.name, run, "end", d))
    lo = T.marks["lower"]
    segs += both((lo, 3, 50, 0)) + both((lo, 0, None, 0)) + both((lo, 99, 100, 0)) + both((lo, 40, 41, 0))
    fill("toggle", (T.name, "all_lower"))
    cases = [Case("fasta masked", FASTA, True, -1, segs), Case("seq masked", SEQ, True, -1, segs)]
    cases += [Case("fasta unmasked", FASTA, False, -1, segs[::2] + segs[1::2]), Case("seq unmasked", SEQ, False, -1, segs[1::4])]
    fill("toggle", (T.name, "mask_on")); fill("toggle", (T.name, "mask_off"))
    # how many toggles a chunk of 16 bases meets: one segment alone from offset 0, so that chunk j holds bases g0 + 16 j ...
    a = T.cum[r] + T.marks["alt_at"]
    ts = np.asarray([t for t, _ in tg])
    for k in range(0, 17):
        for n in (16, 48):
            seg = (r, a - T.cum[r] - k, a - T.cum[r] - k + n, 0)
            g = T.g0(seg)
            for j in range(n // 16):
                inside = int(((ts > g) & (ts >= g + 16 * j) & (ts < g + 16 * j + 16)).sum())
                if inside:
                    fill("toggle", (T.name, "in_chunk", inside))
            for rv in (0, 1):
                cases.append(Case("chunk of toggles %d %d %s" % (k, n, "rc" if rv else "fwd"), SEQ, True, -1, [seg[:3] + (rv,)]))
    return cases


def gen_digits(T, seed, fill):
    r = T.marks["big"]
    segs = []
    for k in range(1, 7):
        for d in (-1, 0, 1):
            v = 10 ** k + d
            n = (5, 61, 1)[(k + d + seed) % 3]
            for what, s in (("begin", (r, v - 1, v - 1 + n, 0)), ("end", (r, max(0, v - n), v, 0))):
                assert s[1] + 1 == v if what == "begin" else s[2] == v
                segs += both(s)
                fill("digits", (T.name, what, k, d))
    return [Case("fasta", FASTA, True, -1, segs), Case("fasta one line", FASTA, False, 0, segs[::-1])]


def gen_lines(T, seed, fill):
    r = T.marks["big"]
    cases = []
    for ll in LINE_LENGTHS:
        L = T.width if ll < 0 else ll
        if L == 0 or L in HUGE_L:
            lengths = [(n, str(n)) for n in (1, 16, 17, 5000)]
        else:
            lengths = [(k * L + d, "%dL%+d" % (k, d)) for k in (1, 2, 3) for d in (-1, 0, 1) if k * L + d > 0]
        segs = []
        for j, (n, what) in enumerate(lengths):
            b = 1001 + 2 * seed + 7919 * j + (j & 1)
            segs += both((r, b, b + n, 0))
            fill("lines", (T.name, ll, what))
        segs += [(T.marks["toggle"], 0, None, 0), (T.marks["toggle"], 0, None, 1), (T.marks["empty_pair"], 0, None, 0)]
        cases.append(Case("line length %d" % ll, FASTA, ll % 2 == 0, ll, segs))
    return cases


def _fill_to(T, mode, L, target):
    """Forward filler segments of the big record whose texts have `target` bytes in all."""
    r, b0, out = T.marks["big"], 1001, []
    one = lambda n: T.size((r, b0, b0 + n, 0), mode, L)
    for _ in range(6):
        lo, hi = 1, target
        while lo < hi:                                       # the size grows with n: the smallest n that reaches the target
            mid = (lo + hi) // 2
            if one(mid) >= target: hi = mid
            else: lo = mid + 1
        if one(lo) == target:
            return out + [(r, b0, b0 + lo, 0)]
        out.append((r, 7, 8 + len(out), 0))                  # the target falls into a jump of the size (a new line, a new digit): a small one in front
        target -= T.size(out[-1], mode, L)
    raise AssertionError("no filler of that size")


def _fill_reads(T, target):
    """Whole forward reads whose texts have `target` bytes in all: 150-base reads of one size, then up to a few short ones."""
    long_r = next(k for k in range(T.N) if T.lens[k] == 150 and not T.recs[k][1])
    big = T.size((long_r, 0, None, 0), FASTQ, 0)
    assert target >= 2 * big
    sizes = {}
    for k in T.marks["small"]:
        sizes.setdefault(T.size((k, 0, None, 0), FASTQ, 0), k)
    a = target // big - 1
    rem = target - a * big
    best = {0: []}
    for s in range(1, rem + 1):
        for sz, k in sizes.items():
            if s - sz in best and (s not in best or len(best[s - sz]) + 1 < len(best[s])):
                best[s] = best[s - sz] + [k]
    assert rem in best, (target, rem)
    longs = [k for k in range(T.N) if T.lens[k] == 150 and not T.recs[k][1]]
    return [(longs[(j * 37) % len(longs)], 0, None, 0) for j in range(a)] + [(k, 0, None, 0) for k in best[rem]]


PHASE_KINDS = {FASTA: ("hdr_first", "hdr_last", "line_end", "last_base", "boundary"), SEQUENCES: ("line_end", "last_base", "boundary"),
               SEQ: ("last_base", "boundary"), FASTQ: ("hdr_first", "hdr_last", "line_end", "last_base", "boundary")}
PHASE_TOTALS = (0, 1, 15, 16, 17, 4095)


def _phase_cells(T, case, fill, group_from):
    feats, total = T.layout(case)
    m = MODE_NAME[case.mode]
    starts, off = [], 0
    for seg in case.segs:
        starts.append(off); off += T.size(seg, case.mode, T.line_length(case))
    for kind, x in feats:
        if x < starts[group_from]:
            continue                                         # (the filler's own features are not what is placed)
        fill("phase", (T.name, m, kind, "chunk", x % CHUNK))
        for d in (-2, -1, 0, 1, 2):
            s = x - d
            if s > 0 and s % TILE == 0:
                fill("phase", (T.name, m, kind, "tile", d))
            elif s > 0 and s % ROUND == 0:
                fill("phase", (T.name, m, kind, "round", d))
    return total


def gen_phase(T, seed, fill):
    cases = []
    big = T.marks.get("big")
    for mode in T.modes():
        m = MODE_NAME[mode]
        L = T.width
        if T.fastq:
            by_len = {T.lens[k]: k for k in T.marks["front"]}
            group = [(by_len[n], 0, None, (n + seed) & 1) for n in (1, 17, 0, 33, 5) if n in by_len] + [(by_len[2], 0, None, 0)]
            filler = lambda target: _fill_reads(T, target)
            base = 1600
        else:
            rc = 1 if T.fourbit else 0
            tg = T.marks.get("toggle", T.marks["tail"])
            group = [(big, 998, 998 + 2 * L + 7, 0), (1, 0, None, 0), (big, 99_999, 100_000 + 33, rc), (T.marks["empty_pair"], 0, None, 0), (tg, 0, None, rc), (big, 8, 9, 0)]
            if mode != FASTA:
                group = [s for s in group if T.nb(s)] + [(T.marks["empty_pair"], 0, None, 0)] * (mode == SEQUENCES)
            filler = lambda target: _fill_to(T, mode, L, target)
            base = 700
        def place(label, kind, seam, forward_only):
            """The group with feature `kind` (its first one) at output offset `seam`, behind a filler of the size that takes."""
            grp = [s[:3] + (0,) for s in group] if forward_only else group
            f0 = next(x for kd, x in [("boundary", 0)] + T.layout(Case("", mode, True, -1, grp))[0] if kd == kind)
            f = filler(seam - f0)
            c = Case("%s %s" % (m, label), mode, True, -1, f + grp)
            _phase_cells(T, c, fill, len(f))
            cases.append(c)

        for kind in PHASE_KINDS[mode]:
            for k in range(CHUNK):
                place("%s at %d" % (kind, base + k), kind, base + k, (k + len(kind)) % 2 == 0)
            for seam, what in ((3 * ROUND, "round"), (2 * TILE, "tile")):
                for d in (-2, -1, 0, 1, 2):
                    place("%s %+d behind a %s seam" % (kind, d, what), kind, seam + d, (d + seed) % 2 == 0)
        # the end of the whole text: a last chunk of every length, the last tile full, nearly full and nearly empty
        for total in [2 * TILE + v for v in PHASE_TOTALS] + [TILE + 32 + v for v in range(2, 15)]:
            f = filler(total)
            c = Case("%s total %d" % (m, total), mode, True, -1, f)
            assert T.layout(c)[1] == total
            fill("phase", (T.name, m, "final_chunk", (total - 1) % CHUNK + 1))
            if total % TILE in PHASE_TOTALS:
                fill("phase", (T.name, m, "total%4096", total % TILE))
            cases.append(c)
    if T.fastq:
        sm = T.marks["front"]
        for rv in (0, 1):
            cases.append(Case("short reads %d" % rv, FASTQ, True, -1, [(k, 0, None, rv) for k in sm]))
            for k in sm:
                fill("phase", (T.name, "fastq", "read_len", T.lens[k], rv))
    return cases


def gen_crowd(T, seed, fill):
    cases = []
    e = T.marks["empty_pair"] if not T.fastq else T.marks["small"][0]
    zero = (e, 0, None, 0)
    if T.fastq:
        for rv in (0, 1):
            zs = [k for k in T.marks["small"] if T.lens[k] == 0]
            assert zs, "the text without empty reads has no crowd of them"
            cases.append(Case("empty reads %d" % rv, FASTQ, True, -1, [(k, 0, None, rv) for k in zs] + [(zs[0], 0, None, rv)] * 300))
            fill("crowd", (T.name, "empty", "fastq", rv))
        return cases
    big = T.marks["big"]
    assert T.lens[e] == 0 and T.lens[e + 1] == 0 and T.lens[0] == 0 and T.lens[-1] == 0
    one = lambda k: (big, 2000 + 3 * k + seed, 2001 + 3 * k + seed, (k % 3 == 0) * T.fourbit)
    for S in CROWD_S:
        segs = [one(k) if k % 5 else (e + (k // 5) % 2, 0, None, 0) for k in range(S)]
        cases.append(Case("%d segments" % S, SEQ, True, -1, segs))
        cases.append(Case("%d segments with headers" % S, FASTA, True, -1, segs))
        fill("crowd", (T.name, "S", S))
    many = [zero] + [one(k) for k in range(1000)] + [zero] + [one(k) for k in range(1000, 2100)] + [zero, (e + 1, 0, None, 0)]
    many += [one(k) for k in range(2100, 4090)] + [(0, 0, None, 0), zero, (T.N - 1, 0, None, 0)] * 23 + [zero] + [one(k) for k in range(4090, 5003)] + [(T.N - 1, 0, None, 0)]
    cases.append(Case("one-base segments across a tile seam, zero-size ones among them", SEQ, True, -1, many))
    assert T.layout(cases[-1])[1] > TILE + 2 * CHUNK
    for w in ("first", "last", "run1", "run2", "run70", "tile_seam"):
        fill("crowd", (T.name, "zeros", w))
    cases.append(Case("nothing but zero-size segments", SEQ, True, -1, [zero, (e + 1, 0, None, 0), (0, 0, None, 0)] * 11))
    assert T.layout(cases[-1])[1] == 0
    fill("crowd", (T.name, "zeros", "only"))
    for mode in (FASTA, SEQUENCES):
        for rv in ((0, 1) if T.fourbit else (0,)):
            cases.append(Case("empty records %s %d" % (MODE_NAME[mode], rv), mode, True, -1, [(0, 0, None, rv), (e, 0, None, rv), (e + 1, 0, None, rv), (T.N - 1, 0, None, rv)] * 5))
            fill("crowd", (T.name, "empty", MODE_NAME[mode], rv))
    return cases


def gen_order(T, seed, fill):
    big, tg = T.marks["big"], T.marks["toggle"]
    rng = np.random.default_rng(7900 + seed)
    asc = sorted((int(rng.integers(0, T.N)), int(rng.integers(0, 5)), int(rng.integers(5, 400)), 0) for _ in range(40))
    asc = [s for s in asc if T.lens[s[0]] > s[1]]
    desc = asc[::-1] + [(big, 900_000, 900_100, 0), (big, 500_000, 500_100, 1), (big, 100, 200, 0)]
    fill("order", (T.name, "descending"))
    rep = [(big, 777, 1234, 0)] * 3 + [(tg, 0, None, 1)] * 2 + [(big, 777, 1234, 0)]
    fill("order", (T.name, "repeat"))
    nested = [(big, 1000, 3000, 0), (big, 1500, 1600, 0), (big, 1000, 3000, 1), (big, 1599, 1600, 1), (big, 1000, 1001, 0), (big, 2999, 3000, 0)]
    fill("order", (T.name, "nested"))
    over = [(big, 5000, 5200, 0), (big, 5100, 5300, 1), (big, 5199, 5201, 0), (big, 5299, 5400, 0)]
    fill("order", (T.name, "overlap"))
    pairs = [x for s in asc[:10] + nested for x in both(s)]
    fill("order", (T.name, "both_strands"))
    segs = desc + rep + nested + over + pairs
    return [Case("fasta", FASTA, True, -1, segs), Case("seq", SEQ, True, -1, segs), Case("sequences unmasked", SEQUENCES, False, -1, segs[::-1])]


def far_segments(T, count, seed):
    """The first `count` far-apart intervals as segments, in shuffled order, strands mixed."""
    segs = []
    for k, (g, n) in enumerate(T.marks["intervals"][:count]):
        r = T.rec_of(g)
        assert T.rec_of(g + n - 1) == r
        segs.append((r, g - T.cum[r], g - T.cum[r] + n, (k + seed) % 3 == 0))
    order = np.random.default_rng(8000 + seed + count).permutation(count)
    return [segs[int(k)][:3] + (int(segs[int(k)][3]),) for k in order]


def gen_far(T, seed, fill):
    cases = []
    for count in (32, 33, FAR_INTERVALS):
        cases.append(Case("%d intervals" % count, (FASTA, SEQ, SEQUENCES)[(count + seed) % 3], True, -1, far_segments(T, count, seed)))
        fill("far", (T.name, count))
    return cases


TEXTS = {"dna_seams": dna_seams, "rna_seams": rna_seams, "protein_seams": protein_seams, "text_seams": text_seams, "fastq_seams": fastq_seams, "dna_far": dna_far}
GENERATORS = {"parity": gen_parity, "block": gen_block, "toggle": gen_toggle, "digits": gen_digits, "lines": gen_lines, "phase": gen_phase, "crowd": gen_crowd,
              "order": gen_order, "far": gen_far}
CLASSES_OF = {"dna_seams": ("parity", "block", "toggle", "digits", "lines", "phase", "crowd", "order"), "rna_seams": ("parity", "toggle"),
              "protein_seams": ("block", "phase", "crowd"), "text_seams": ("block", "phase", "crowd"), "fastq_seams": ("block", "phase", "crowd"), "dna_far": ("far",)}
MAKERS_OF = {name: (("oracle",) if name == "dna_far" else ("oracle", "own")) for name in TEXTS}


def makers_of(name, cls):
    """The archive makers a class runs under: the oracle's raw 128 KiB blocks and this build's own frames."""
    return ("oracle",) if (name, cls) == ("fastq_seams", "crowd") else MAKERS_OF[name]


def text_of(name, seed, maker="oracle"):
    return fastq_seams(seed, False) if (name, maker) == ("fastq_seams", "own") else TEXTS[name](seed)


def cases_of(name, cls, seed, table=None, maker="oracle"):
    """The lists of class cls on text `name`; table (a Counter) receives the cells they fill."""
    table = Counter() if table is None else table

    def fill(c, phase):
        table[(c, phase)] += 1
    return GENERATORS[cls](text_of(name, seed, maker), seed, fill)


def coverage(seed=0):
    """(class, phase) -> how many placements fill it, over every text and class."""
    table = Counter()
    for name, classes in CLASSES_OF.items():
        for cls in classes:
            cases_of(name, cls, seed, table)
    return table


def expected_cells():
    """Every cell the plan claims, listed without looking at what the generators emit."""
    cells = []
    for name in ("dna_seams", "rna_seams"):
        cells += [("parity", (name, n, par, place)) for n in range(1, 34) for par in (0, 1) for place in ("first", "middle", "last")]
        cells += [("parity", (name, "end", k)) for k in ("len", "len+1", "clamped")]
        cells += [("toggle", (name, run, side, d)) for run in TOGGLE_RUNS for side in ("begin", "end") for d in range(-2, 3)]
        cells += [("toggle", (name, k)) for k in ("all_lower", "mask_on", "mask_off")] + [("toggle", (name, "in_chunk", c)) for c in range(1, 17)]
    for name in ("dna_seams", "protein_seams", "text_seams"):
        kinds = ("inside", "boundary", "own")
        cells += [("block", (name, kind, side, d)) for kind in kinds for side in ("begin", "end") for d in range(-2, 3)]
        cells += [("block", (name, k)) for k in ("g_lo odd", "g_lo even", "g_hi odd", "g_hi even", "two_seams", "last_block")]
        modes = ("fasta", "sequences", "seq")
        cells += [("phase", (name, MODE_NAME[m], kind, "chunk", p)) for m in PHASE_KINDS if m != FASTQ for kind in PHASE_KINDS[m] for p in range(CHUNK)]
        cells += [("phase", (name, MODE_NAME[m], kind, seam, d)) for m in PHASE_KINDS if m != FASTQ for kind in PHASE_KINDS[m] for seam in ("round", "tile") for d in range(-2, 3)]
        cells += [("phase", (name, m, "final_chunk", n)) for m in modes for n in range(1, 17)] + [("phase", (name, m, "total%4096", v)) for m in modes for v in PHASE_TOTALS]
        cells += [("crowd", (name, "S", S)) for S in CROWD_S] + [("crowd", (name, "zeros", w)) for w in ("first", "last", "run1", "run2", "run70", "tile_seam", "only")]
        cells += [("crowd", (name, "empty", m, rv)) for m in ("fasta", "sequences") for rv in ((0, 1) if name == "dna_seams" else (0,))]
    cells += [("block", ("fastq_seams", what, d)) for what in ("seq", "qual") for d in ("before", "across", "after")]
    cells += [("phase", ("fastq_seams", "fastq", kind, "chunk", p)) for kind in PHASE_KINDS[FASTQ] for p in range(CHUNK)]
    cells += [("phase", ("fastq_seams", "fastq", kind, seam, d)) for kind in PHASE_KINDS[FASTQ] for seam in ("round", "tile") for d in range(-2, 3)]
    cells += [("phase", ("fastq_seams", "fastq", "final_chunk", n)) for n in range(1, 17)] + [("phase", ("fastq_seams", "fastq", "total%4096", v)) for v in PHASE_TOTALS]
    cells += [("phase", ("fastq_seams", "fastq", "read_len", n, rv)) for n in READ_LENGTHS for rv in (0, 1)]
    cells += [("crowd", ("fastq_seams", "empty", "fastq", rv)) for rv in (0, 1)]
    cells += [("digits", ("dna_seams", what, k, d)) for what in ("begin", "end") for k in range(1, 7) for d in (-1, 0, 1)]
    for ll in LINE_LENGTHS:
        L = 60 if ll < 0 else ll
        if L == 0 or L in HUGE_L:
            cells += [("lines", ("dna_seams", ll, str(n))) for n in (1, 16, 17, 5000)]
        else:
            cells += [("lines", ("dna_seams", ll, "%dL%+d" % (k, d))) for k in (1, 2, 3) for d in (-1, 0, 1) if k * L + d > 0]
    cells += [("order", ("dna_seams", k)) for k in ("descending", "repeat", "nested", "overlap", "both_strands")]
    cells += [("far", ("dna_far", n)) for n in (32, 33, FAR_INTERVALS)]
    return cells
