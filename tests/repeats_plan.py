"""The plan of the tandem-repeat tests (test_repeats_cpu.py holds it to its claims, test_gpu_repeats.py runs it): the reference, the texts and
the queries.  Pure Python and numpy; nothing here comes from the code under test.

The reference works on the oracle's --sequences text of an archive (one line per record).  expected_repeats upper-cases a line, maps U to T
and takes, per period p, the mask ok[p:] & ok[:-p] & (a[p:] == a[:-p]) -- base i and base i + p are both A/C/G/T and equal --, finds its
runs with np.diff, and lengthens each by p: a run [s, e) of the mask is the repeat [s, e + p).  Then the motif, the primitivity test, the
thresholds, and a sort by (begin, period) per record.  brute_repeats walks base by base in plain Python and shares no code with it.

The `seams` text lays repeats of 3p + 1 bases, p in PERIODS, each bounded by a mismatching base on either side, so that the repeat's first
base and, in a separate plant, its last base lie at every offset -(p + 1) .. +2 of a seam of the sweep: a lane's 64 bases, a 16-byte load
(32 bases), a tile (4096 bases) and a record's end -- 174 plants a kind.  The seam so falls at each place between the repeat's first base
and the first base that "continues" (p behind it), and on either side of them.  A plant across a record's end is cut there: its parts of
at least 2p bases are the rows.  Two kinds cannot have every cell in a text of this size: a zstd block of the packed stream (262144 bases)
has two seams in 717 K bases -- they are tile seams 63 and 127, whose plants count for both kinds; to the sweep a block seam is a tile seam,
and the pieces test decodes across them --, and the stream has one end: the plant whose last base is the stream's last.  What the sweep
does at the stream's end it does at the end of every piece, so test_gpu_repeats.py asks every record of this text alone: each record seam
is then the end of one sweep and the start of the next, at every offset."""
import numpy as np

from locate_plan import _random, fasta
from composition_plan import lines_of                                               # noqa: F401  (the records of a --sequences text)

REPEAT_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("motif", "<u4"), ("period", "u1"), ("reserved", "u1", (3,))]
SEAM_KINDS = ("lane", "load32", "tile", "block", "record", "end")
PERIODS = (1, 2, 3, 5, 6, 7, 15, 16)                                                # of the planted seams
BLOCK = 262144
MISA = (10, 6, 5, 5, 5, 5) + (0,) * 10
ALL2, ALL3 = (2,) * 16, (3,) * 16
MIN_LENS = (1, 12, 100)

# naf_gpu_parse_repeat_spec: text -> the sixteen min_copies, None = rejected.  Written out, not computed.
PARSE_TABLE = [
    ("misa", [10, 6, 5, 5, 5, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("1-10,2-6,3-5,4-5,5-5,6-5", [10, 6, 5, 5, 5, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("1-10", [10, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("2-6,1-10", [10, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("16-2", [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2]),
    ("3-4294967295", [0, 0, 4294967295, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("1-2,2-2,3-2,4-2,5-2,6-2,7-2,8-2,9-2,10-2,11-2,12-2,13-2,14-2,15-2,16-2", [2] * 16),
    ("7-3,16-9,12-100", [0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 100, 0, 0, 0, 9]),
    ("", None), ("misa,1-10", None), ("MISA", None), ("misa ", None), ("1-10,", None), (",1-10", None), ("1-10,,2-6", None), ("1-10,1-5", None), ("2-6,3-5,2-6", None),
    ("0-5", None), ("17-2", None), ("1-0", None), ("1-1", None), ("5-1", None), ("1-4294967296", None), ("1-99999999999999999999", None), (" 1-10", None), ("1-10 ", None),
    ("1 -10", None), ("1- 10", None), ("1-10, 2-6", None), ("1", None), ("1-", None), ("-10", None), ("1--10", None), ("1-10-2", None), ("a-10", None), ("1-x", None),
    ("1:10", None), ("+1-10", None), ("1-+10", None), ("1-10\n", None), ("1-10;2-6", None),
]


def spec_text(min_copies):
    return ",".join("%d-%d" % (p + 1, c) for p, c in enumerate(min_copies) if c)


def single(p, copies):
    return tuple(copies if q == p - 1 else 0 for q in range(16))


def _range(lines, first, count):
    return range(first, len(lines) if count is None else first + count)


_LUT = np.full(256, 255, dtype=np.uint8)
for _k, _ch in enumerate("ACGT"):
    _LUT[ord(_ch)] = _LUT[ord(_ch.lower())] = _k
_LUT[ord("U")] = _LUT[ord("u")] = 3


def _divisors(p):
    return [d for d in range(1, p) if p % d == 0]


def base_rows(lines, min_copies, first=0, count=None):
    """(record, begin, end, motif, period) of every primitive maximal repeat that has its period's copies, as five int64 arrays in the order
    of the contract -- what expected_repeats filters."""
    cols = [[], [], [], [], []]
    for r in _range(lines, first, count):
        a = _LUT[np.frombuffer(lines[r], dtype=np.uint8)]
        ok = a < 4
        n = len(a)
        rec = [[], [], [], []]
        for p in range(1, 17):
            mc = min_copies[p - 1]
            if not mc or n < 2 * p:
                continue
            m = ok[p:] & ok[:-p] & (a[p:] == a[:-p])
            d = np.diff(np.concatenate(([0], m.astype(np.int8), [0])))
            begin, end = np.flatnonzero(d == 1), np.flatnonzero(d == -1) + p
            keep = (end - begin) // p >= mc
            begin, end = begin[keep], end[keep]
            if not len(begin):
                continue
            W = a[begin[:, None] + np.arange(p)[None, :]].astype(np.int64)              # the motifs, one a row
            prim = np.ones(len(begin), dtype=bool)
            for dv in _divisors(p):
                prim &= ~(W[:, dv:] == W[:, :-dv]).all(axis=1)
            motif = (W << (2 * np.arange(p))[None, :]).sum(axis=1)
            rec[0].append(begin[prim]); rec[1].append(end[prim]); rec[2].append(motif[prim]); rec[3].append(np.full(int(prim.sum()), p, dtype=np.int64))
        if rec[0]:
            b, e, mo, pe = (np.concatenate(x) for x in rec)
            order = np.lexsort((pe, b))
            cols[0].append(np.full(len(b), r, dtype=np.int64))
            for k, x in enumerate((b, e, mo, pe)):
                cols[k + 1].append(x[order])
    return tuple(np.concatenate(c) if c else np.zeros(0, dtype=np.int64) for c in cols)


def filter_rows(base, min_len=1, whole=False):
    """The REPEAT_DTYPE table of base_rows' repeats that have min_len bases, cut to whole units first when asked."""
    rec, b, e, mo, pe = base
    if whole:
        e = b + (e - b) // pe * pe
    keep = e - b >= min_len
    out = np.zeros(int(keep.sum()), dtype=REPEAT_DTYPE)
    out["record"], out["begin"], out["end"], out["motif"], out["period"] = rec[keep], b[keep], e[keep], mo[keep], pe[keep]
    return out


def expected_repeats(lines, min_copies, min_len=1, whole=False, first=0, count=None):
    """The rows of records [first, first + count) as a REPEAT_DTYPE array, in the order of the contract."""
    return filter_rows(base_rows(lines, min_copies, first, count), min_len, whole)


def brute_repeats(lines, min_copies, min_len=1, whole=False, first=0, count=None):
    """[(record, begin, end, motif, period)] by a walk over the bases (no numpy): a repeat starts at b where x[b] == x[b + p] and
    x[b - 1] != x[b - 1 + p]."""
    out = []
    val = {"A": 0, "C": 1, "G": 2, "T": 3}
    for r in _range(lines, first, count):
        t = lines[r].decode("latin1").upper().replace("U", "T")
        n = len(t)
        rows = []
        for p in range(1, 17):
            mc = min_copies[p - 1]
            if not mc:
                continue
            b = 0
            while b + p < n:
                if t[b] in val and t[b] == t[b + p]:
                    e = b
                    while e + p < n and t[e] in val and t[e] == t[e + p]:
                        e += 1
                    begin, end = b, e + p
                    w = t[begin:begin + p]
                    copies = (end - begin) // p
                    if whole:
                        end = begin + copies * p
                    if copies >= mc and end - begin >= min_len and not any(w == w[:d] * (p // d) for d in range(1, p) if p % d == 0):
                        rows.append((begin, p, end, sum(val[ch] << (2 * i) for i, ch in enumerate(w))))
                    b = e + 1
                else:
                    b += 1
        out += [(r, b, e, m, p) for b, p, e, m in sorted(rows)]
    return out


def as_tuples(rows):
    return [(int(x["record"]), int(x["begin"]), int(x["end"]), int(x["motif"]), int(x["period"])) for x in rows]


def motif_text(motif, p, rna=False):
    return "".join(("ACGU" if rna else "ACGT")[(motif >> (2 * i)) & 3] for i in range(p))


def class_of(word):
    """The motif class of a word over ACGT by its definition: the smallest of the rotations of the word and of its reverse complement."""
    rc = word[::-1].translate(str.maketrans("ACGT", "TGCA"))
    return min(w[k:] + w[:k] for w in (word, rc) for k in range(len(word)))


def table_lines(rows, names, rna=False):
    """The lines unnaf --repeats prints for the rows."""
    out = []
    for x in rows:
        p, b, e = int(x["period"]), int(x["begin"]), int(x["end"])
        cls = class_of(motif_text(int(x["motif"]), p))
        out.append("%s\t%d\t%d\t%d\t%s\t%d\t%s\n" % (names[int(x["record"])], b, e, p, motif_text(int(x["motif"]), p, rna), (e - b) // p, cls.replace("T", "U") if rna else cls))
    return "".join(out).encode("latin1")


# ---- texts -------------------------------------------------------------------------------------------------------------------------
def _unit(rng, p, alphabet="ACGT"):
    """a primitive word of p letters"""
    while True:
        w = _random(rng, p, alphabet)
        if not any(w == w[:d] * (p // d) for d in _divisors(p)):
            return w


def _rep(w, n, phase=0):
    return "".join(w[(phase + i) % len(w)] for i in range(n))


def _other(rng, *not_these):
    return str(rng.choice([ch for ch in "ACGT" if ch not in not_these]))


def _bounded(rng, w, n):
    """a base that does not extend the repeat, n bases of it, and another such base"""
    s = _rep(w, n)
    p = len(w)
    return _other(rng, s[p - 1] if n >= p else "") + s + _other(rng, s[n - p] if n >= p else "")


def _put(s, at, text):
    assert 0 <= at and at + len(text) <= len(s)
    s[at:at + len(text)] = np.frombuffer(text.encode(), dtype=np.uint8)


def _cut(stream, bounds):
    return [stream[a:b] for a, b in zip(bounds[:-1], bounds[1:])]


class Case:
    """name, the input text and how it is archived, the records, and the specs (sixteen min_copies each) every one of which is asked at
    MIN_LENS with and without whole units."""

    def __init__(self, name, text, records, specs, seq_type=0, well_formed=False, own_text=None):
        self.name, self.text, self.records, self.specs, self.seq_type, self.well_formed = name, text, records, specs, seq_type, well_formed
        self.own_text = text if own_text is None else own_text                       # what this library's own ennaf is given
        self.lines = [r.encode() for r in records]
        self.plants = []                                                             # (record, begin, end, period): rows of ALL2 at min_len 1
        self.absent = []                                                             # (record, begin, end, period): no row of any spec


class RepeatSeams:
    """A stream of 716837 bases (odd), background upper-case ACGT, with the plants of the module's docstring.  Combination i of (period, side,
    offset) lies at tile seam 4096 (i + 1), at the lane seam 1088 behind it, at the load seam 2080 behind it and at the record seam
    3072 + i % 3 behind it.  Empty records: one at record seam 3, three at record seam 7, one in front and one at the end."""
    COMBOS = [(p, side, d) for p in PERIODS for side in ("first", "last") for d in range(-(p + 1), 3)]
    TOTAL = 4096 * (len(COMBOS) + 1) + 37

    def __init__(self, seed):
        rng = np.random.default_rng(11000 + seed)
        T = self.TOTAL
        s = np.frombuffer(_random(rng, T, "ACGT").encode(), dtype=np.uint8).copy()
        self.seams = {"tile": [], "lane": [], "load32": [], "record": [], "block": [BLOCK, 2 * BLOCK], "end": [T]}
        self.plants = []                                                             # (kind, seam, period, side, offset, a, b)
        for i, (p, side, d) in enumerate(self.COMBOS):
            t = 4096 * (i + 1)
            for kind, seam in (("tile", t), ("lane", t + 1088), ("load32", t + 2080), ("record", t + 3072 + i % 3)):
                self.seams[kind].append(seam)
                n = 3 * p + 1
                a = seam + d if side == "first" else seam + d - n + 1
                _put(s, a - 1, _bounded(rng, _unit(rng, p), n))
                self.plants.append((kind, seam, p, side, d, a, a + n))
                if kind == "tile" and seam in self.seams["block"]:
                    self.plants.append(("block", seam, p, side, d, a, a + n))
        assert all(x % 64 == 0 and x % 4096 for x in self.seams["lane"]) and all(x % 64 == 32 for x in self.seams["load32"])
        assert sum(1 for x in self.plants if x[0] == "block") == 2
        _put(s, T - 50, _bounded(rng, _unit(rng, 16), 49)[:-1])                      # the stream's last base is the repeat's last
        self.plants.append(("end", T, 16, "last", -1, T - 49, T))
        self.stream = s.tobytes().decode()
        cuts = list(self.seams["record"])
        cuts = sorted(cuts + [cuts[3]] + [cuts[7]] * 3)
        self.bounds = [0, 0] + cuts + [T, T]
        self.records = _cut(self.stream, self.bounds)
        self.text = fasta(self.records, 61)

    def rows_of(self, a, b, p):
        """the rows a plant [a, b) of the stream has to give: its parts in the records, those of at least 2p bases"""
        out = []
        for r in range(len(self.records)):
            lo, hi = self.bounds[r], self.bounds[r + 1]
            x, y = max(a, lo), min(b, hi)
            if y - x >= 2 * p:
                out.append((r, x - lo, y - lo, p))
        return out

    def coverage(self, rows):
        """{(kind, side, period): offsets} of the plants whose parts are all rows of `rows` (ALL2 at min_len 1) with exactly their bounds"""
        have = {(int(x["record"]), int(x["begin"]), int(x["end"]), int(x["period"])) for x in rows}
        cov = {}
        for kind, seam, p, side, d, a, b in self.plants:
            parts = self.rows_of(a, b, p)
            if parts and all(x in have for x in parts) and (a if side == "first" else b - 1) == seam + d:
                cov.setdefault((kind, side, p), set()).add(d)
        return cov


def seams_case(seed):
    S = RepeatSeams(seed)
    c = Case("seams", S.text, S.records, [MISA, ALL2, ALL3, single(1, 4), single(16, 2), single(7, 3)])
    c.seams = S
    c.plants = [x for _, _, p, _, _, a, b in S.plants for x in S.rows_of(a, b, p)]
    return c


def lengths_case(seed):
    """Per period of LP: repeats of 2p - 1 (no row), 2p, 2p + 1, 63 .. 65, 4095 .. 4097 and 13001 bases (the last spans tiles without an
    event), each bounded; records of p, 2p - 1, 2p and 2p + 1 bases that are one repeat, and for p = 1, 3, 16 of 63 .. 65, 127, 128 and 4096 bases
    (swept alone, such a record ends its piece on or next to a lane's last base); empty records first, last and side by side; a repeat
    up to a record's last base and one with the same motif from base 0 of the next non-empty record: two rows.  The stream ends in a repeat."""
    rng = np.random.default_rng(11100 + seed)
    recs, plants, absent = [""], [], []
    for p in (1, 2, 3, 4, 7, 16):
        parts, at = [], 0
        for n in (2 * p - 1, 2 * p, 2 * p + 1, 63, 64, 65, 4095, 4096, 4097, 13001):
            if n < 2 * p - 1:
                continue
            gap = _random(rng, int(rng.integers(40, 90)), "ACGT")
            parts += [gap, _bounded(rng, _unit(rng, p), n)]
            at += len(gap) + n + 2
            (plants if n >= 2 * p else absent).append((len(recs), at - n - 1, at - 1, p))
        recs.append("".join(parts) + _random(rng, 33, "ACGT"))
        w = _unit(rng, p)
        for n in (p, 2 * p - 1, 2 * p, 2 * p + 1) + ((63, 64, 65, 127, 128, 4096) if p in (1, 3, 16) else ()):     # (a record that ends on a lane's last base, as a piece of its own)
            (plants if n >= 2 * p else absent).append((len(recs), 0, n, p))
            recs.append(_rep(w, n))
        recs += [""] * (p % 3)
        w = _unit(rng, p)
        plants += [(len(recs), 200, 200 + 5 * p + 1, p), (len(recs) + 2, 0, 4 * p, p)]
        recs += [_random(rng, 199, "ACGT") + _bounded(rng, w, 5 * p + 1)[:-1], "", _bounded(rng, w, 4 * p)[1:] + _random(rng, 50, "ACGT")]
    recs += ["", ""]
    if sum(len(r) for r in recs) % 2 == 0:
        recs[1] = "G" + recs[1]
        plants = [(r, b + 1, e + 1, p) if r == 1 else (r, b, e, p) for r, b, e, p in plants]
        absent = [(r, b + 1, e + 1, p) if r == 1 else (r, b, e, p) for r, b, e, p in absent]
    c = Case("lengths", fasta(recs, 80), recs, [MISA, ALL2, ALL3, single(2, 2), single(16, 2), single(4, 1024)])
    c.plants, c.absent = plants, absent
    return c


def overlap_case(seed):
    """Same-period repeats that share 1 .. p - 1 bases; repeats of several periods that begin on one base; motifs that are whole powers of
    a word of every proper divisor of p = 2, 4, 6, 8, 9, 12, 15, 16: no row of period p, also when the shorter period is not searched."""
    rng = np.random.default_rng(11200 + seed)
    recs, plants, absent = ["ACACAGAGAG"], [(0, 0, 5, 2), (0, 4, 10, 2)], []
    for p in (2, 3, 4, 5, 7, 8, 15, 16):
        for k in range(1, p):
            while True:                                                              # until the two repeats are what the reference finds
                w1, w2 = _unit(rng, p), _unit(rng, p)
                s1 = _rep(w1, 3 * p)
                s2 = _rep(s1[-k:] + w2[k:], 3 * p)
                text = _other(rng, s1[p - 1]) + s1 + s2[k:] + _other(rng, s2[-p])
                want = {(0, 1, 1 + 3 * p, p), (0, 1 + 3 * p - k, 1 + 6 * p - k, p)}
                got = {t[:3] + (t[4],) for t in as_tuples(expected_repeats([text.encode()], single(p, 2)))}
                if want <= got:
                    break
            plants += [(len(recs), b, e, p) for _, b, e, p in sorted(want)]
            recs.append(text)
    for w, more in (("AAC", (1, 3)), ("AATAATG", (1, 7)), ("CCGCCGCCA", (1, 3, 9)), ("TTAGTTAGTTAC", (1, 4, 12))):   # (AA) and (AAC..) begin on base 0
        text = _rep(w, 4 * len(w)) + "N"
        plants += [(len(recs), 0, 2, 1), (len(recs), 0, 4 * len(w), len(w))]
        recs.append(text)
    for p in (2, 4, 6, 8, 9, 12, 15, 16):
        for d in _divisors(p):
            recs.append(_random(rng, 20, "ACGT") + _bounded(rng, _unit(rng, d), 3 * p + 1) + _random(rng, 20, "ACGT"))
            absent.append((len(recs) - 1, 21, 21 + 3 * p + 1, p))
    c = Case("overlap", fasta(recs, 70), recs, [MISA, ALL2, ALL3] + [single(p, 2) for p in (2, 4, 6, 8, 9, 12, 15, 16)])
    c.plants, c.absent = plants, absent
    return c


def _unknown_records(rng, t="T"):
    recs = []
    for p in (1, 2, 3, 5, 16):
        w = _unit(rng, p)
        for pos in range(p):
            for ch in "NR-":
                s = list(_rep(w, 6 * p + 2))
                s[3 * p + pos] = ch                                                  # at each place of a unit
                recs.append("G" + "".join(s))
        recs.append(_rep(w.lower(), 4 * p + 1) + "n" + _rep(w, 3 * p))               # lower case, then upper case behind an n
        recs.append("".join(ch.lower() if (i * 7 // 3) % 2 else ch for i, ch in enumerate(_rep(w, 5 * p + 3))))   # mixed case
    recs.append(_random(rng, 3000, "ACGTacgtNRY-"))
    if sum(len(r) for r in recs) % 2 == 0:
        recs.append("CAC")
    return [r.replace("T", t).replace("t", t.lower()) for r in recs]


def unknown_case(seed):
    """An N, an R and a '-' at each place of a unit; lower-case and mixed-case units; the stream is odd."""
    recs = _unknown_records(np.random.default_rng(11300 + seed))
    assert sum(len(r) for r in recs) % 2 == 1
    return Case("unknown", fasta(recs, 60), recs, [MISA, ALL2, ALL3, single(1, 2), single(5, 2)])


def rna_case(seed):
    """The RNA twin of `unknown`: the same records with U for T."""
    recs = _unknown_records(np.random.default_rng(11300 + seed), "U")
    return Case("rna", fasta(recs, 60), recs, [MISA, ALL2, ALL3, single(3, 2)], seq_type=1)


def fastq_case(seed):
    """Reads of 0 to 40 and of 150 bases, with short repeats at their ends and starts.  The reference's format takes a read of no bases
    only from a well-formed text, and the tolerant parser of this library's ennaf not at all: its archive holds the other reads."""
    rng = np.random.default_rng(11400 + seed)
    recs = [_random(rng, n, "ACGT" * 6 + "N") for n in range(41)]
    for k in range(400):
        p = 1 + k % 6
        w = _unit(rng, p)
        r = _random(rng, 150, "ACGT" * 8 + "N")
        n = 2 * p + k % 11
        recs.append((_rep(w, n) + r[n:-n] + _rep(w, n, 150 - n)) if k % 3 else r)   # (the read behind it starts with the same motif in phase every other time)
    def fq(reads):
        return "".join("@read%d x\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(reads)).encode()
    return Case("fastq", fq(recs), recs, [MISA, ALL2, ALL3, single(6, 2)], well_formed=True, own_text=fq(recs[1:]))


def dense_case(seed):
    """200 K bases over A and C only: at 2 copies for all sixteen periods the candidate tables are at their worst.  And one letter repeated:
    a single row of period 1 per record and nothing at any other period."""
    rng = np.random.default_rng(11500 + seed)
    stream = _random(rng, 200001, "AC")
    recs = _cut(stream, [0, 70001, 70001, 130000, 200001]) + ["A" * 5000, "c" * 77, "", "G" * 2, "T"]
    c = Case("dense", fasta(recs, 100), recs, [MISA, ALL2, ALL3, single(1, 2), single(16, 2)])
    c.plants = [(4, 0, 5000, 1), (5, 0, 77, 1), (7, 0, 2, 1)]
    return c


def no_records_case(seed):
    return Case("no_records", b"", [], [MISA, ALL2])


def planned(seed=0):
    return [seams_case(seed), lengths_case(seed), overlap_case(seed), unknown_case(seed), rna_case(seed), fastq_case(seed), dense_case(seed), no_records_case(seed)]
