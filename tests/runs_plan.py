"""The plan of the run-table tests (test_runs_cpu.py holds it to its claims, test_gpu_runs.py runs it): the reference, the texts and the
queries.  Pure Python and numpy; nothing here comes from the code under test.

The reference works on the oracle's --sequences text of an archive, mask on (one line per record).  expected_runs upper-cases a line, maps
U to T and lets `re.finditer` find the maximal stretches of a character class made of the LETTERS of the set -- `[..]+`, or `([..])\\1*` when
every letter is a class of its own; expected_masked finds `[a-z]+` in the line as it is.  brute_runs is a plain loop over the bases and
shares no code with either.  Membership is literal: the class N is the letter N and nothing else.

The `seams` text lays its runs around six kinds of seams of the sweep -- a lane's 64 bases, a 16-byte load (32 bases), a tile (4096
bases), a zstd block of the packed stream (128 KiB = 262144 bases), a record's end and the stream's end -- so that a run's first base and,
separately, a run's last base lie at every offset -2 .. +2 of a seam of the kind; see RunSeams."""
import re

import numpy as np

from locate_plan import CODES, _random, fasta, r7_case as _locate_r7
from composition_plan import lines_of                                               # noqa: F401  (the records of a --sequences text)

RUN_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("code", "<u4"), ("reserved", "<u4")]
SEAM_KINDS = ("lane", "load32", "tile", "block", "record", "end")
OFFSETS = (-2, -1, 0, 1, 2)
BLOCK = 262144
LENGTHS = (1, 2, 63, 64, 65, 4095, 4096, 4097, 13001)                               # the last: more than three tiles, so tiles without an event
MASK_LENGTHS = (255, 510)                                                           # the unit encoding's continuation: 255 is "go on"
ALL = 0xFFFF

# naf_gpu_parse_base_class: text -> set (bit c = code c of CODES), None = rejected.  Written out, not computed.
PARSE_TABLE = [
    ("N", 0x8000), ("n", 0x8000), ("-", 0x0001), ("A", 0x0100), ("C", 0x0010), ("G", 0x0004), ("T", 0x0002), ("U", 0x0002), ("u", 0x0002),
    ("K", 0x0008), ("Y", 0x0020), ("S", 0x0040), ("B", 0x0080), ("W", 0x0200), ("R", 0x0400), ("D", 0x0800), ("M", 0x1000), ("H", 0x2000), ("V", 0x4000),
    ("ACGT", 0x0116), ("acgu", 0x0116), ("TGCA", 0x0116), ("AACC", 0x0110), ("ACGTU", 0x0116), ("N-", 0x8001), ("RYSWKM", 0x1668), ("BDHV", 0x6880),
    ("^N", 0x7FFF), ("^n", 0x7FFF), ("^-", 0xFFFE), ("^ACGT", 0xFEE9), ("^N-", 0x7FFE), ("-TGKCYSBAWRDMHVN", 0xFFFF), ("^ACGTRYSWKMBDHVN", 0x0001),
    ("", None), ("^", None), ("X", None), ("ACGX", None), ("N^", None), ("^^N", None), ("A C", None), ("N\n", None), ("5", None), ("AC,GT", None), ("*", None),
]


def set_of(letters):
    """The set of a string of upper-case letters of CODES (U is T)."""
    s = 0
    for ch in letters:
        s |= 1 << CODES.index("T" if ch == "U" else ch)
    return s


def letters_of(s):
    return "".join(CODES[c] for c in range(16) if (s >> c) & 1)


def _class(s):
    return b"[" + re.escape(letters_of(s)).encode() + b"]"


def _range(lines, first, count):
    return range(first, len(lines) if count is None else first + count)


def _table(rows):
    out = np.zeros(len(rows), dtype=RUN_DTYPE)
    if rows:
        a = np.array(rows, dtype=np.uint64)
        out["record"], out["begin"], out["end"], out["code"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return out


def expected_runs(lines, s, each=False, min_len=1, first=0, count=None):
    """The runs of class s (a set) in records [first, first + count) as a RUN_DTYPE array, in the order of the contract."""
    rx = re.compile(b"(" + _class(s) + b")\\1*" if each else _class(s) + b"+")
    rows = []
    for r in _range(lines, first, count):
        t = lines[r].upper().replace(b"U", b"T")
        rows += [(r, m.start(), m.end(), CODES.index(chr(t[m.start()]))) for m in rx.finditer(t) if m.end() - m.start() >= min_len]
    return _table(rows)


def expected_masked(lines, min_len=1, first=0, count=None):
    """The soft-masked intervals: the lower-case stretches of every line; code 0."""
    rx = re.compile(b"[a-z]+")
    rows = []
    for r in _range(lines, first, count):
        rows += [(r, m.start(), m.end(), 0) for m in rx.finditer(lines[r]) if m.end() - m.start() >= min_len]
    return _table(rows)


def brute_runs(lines, s=0, each=False, masked=False, min_len=1, first=0, count=None):
    """[(record, begin, end, code)] by one walk over the bases (no numpy, no regex)."""
    out = []
    code_of = {ch: k for k, ch in enumerate(CODES)}
    code_of["U"] = 1
    for r in _range(lines, first, count):
        t = lines[r].decode("latin1")
        begin, key = None, None                                                     # the open run and what its bases share
        for i in range(len(t) + 1):
            if i < len(t):
                code = code_of[t[i].upper()]
                if masked:
                    k = True if t[i] != t[i].upper() else None
                else:
                    k = (code if each else True) if (s >> code) & 1 else None
            else:
                k = None
            if begin is not None and k != key:
                if i - begin >= min_len:
                    out.append((r, begin, i, 0 if masked else code_of[t[begin].upper()]))
                begin = None
            if begin is None and k is not None:
                begin, key = i, k
    return out


def as_tuples(rows):
    return [(int(x["record"]), int(x["begin"]), int(x["end"]), int(x["code"])) for x in rows]


def bed(rows, names, name=None, rna=False):
    """The lines unnaf --runs / --masked-runs prints for the rows; name: the fourth column (None: the run's letter, as with --each)."""
    letters = CODES.replace("T", "U") if rna else CODES
    return "".join("%s\t%d\t%d\t%s\n" % (names[int(x["record"])], x["begin"], x["end"], name if name is not None else letters[int(x["code"])]) for x in rows).encode("latin1")


# ---- texts -------------------------------------------------------------------------------------------------------------------------
def _lay(s, low, a, b, what):
    """bases [a, b) of the stream: the letter N (what = "N"), or lower case (what = "mask")"""
    assert 0 <= a < b <= len(s)
    if what == "mask":
        low[a:b] = True
    else:
        s[a:b] = ord(what)


def _finish(s, low):
    letters = (s >= 65) & (s <= 90)
    s = s.copy()
    s[low & letters] += 32
    return s.tobytes().decode()


def _cut(stream, bounds):
    return [stream[a:b] for a, b in zip(bounds[:-1], bounds[1:])]


class RunSeams:
    """A stream of 600001 bases (it ends on an odd base), background upper-case ACGT, with N runs and lower-case stretches laid around
    seams, cut into records.

    seams[kind]: twenty positions per kind (lane: multiples of 64 that are none of 4096; load32: 32 + multiples of 64; tile: multiples of
    4096; record: stream positions where a record ends and the next one starts).  At seam j of a kind, j = 0 .. 4, an N run has its FIRST
    base at seam + (j - 2); j = 5 .. 9, an N run has its LAST base at seam + (j - 7); seams 10 .. 19 carry lower-case stretches the same
    way.  The run lengths go through PLANT_LENGTHS, the masked ones start with exactly 255 and 510 bases, so runs at record seams do and do
    not cross the record's end.
    block: a text of this size has two such seams, and five runs cannot start within two bases of one: runs of ONE base lie at -2, 0, +2
    of the first and at -1, +1 of the second (lower case: the other way round) -- every offset for first and last bases alike; the longer
    runs lie at the tile seams, which is what a block seam is to the sweep, and the `lengths` text has a run ACROSS a block seam.
    end: the stream has one end.  This text ends with an N run [T - 2, T) (first base at -2, last at -1) and a lower-case last letter; the
    `lengths` text has a run whose last base is at -2 and the `record_ends` text a run that is the last base alone (first at -1).
    Empty records: one at record seam 3, three at record seam 7, one in front and one at the end.  The stream starts with NN, lower case."""
    TOTAL = 600001
    PLANT_LENGTHS = (1, 2, 3, 5, 64, 70, 130, 255, 510, 600)
    MASK_PLANT_LENGTHS = (255, 510, 1, 2, 70, 510, 255, 3, 130, 600)

    def __init__(self, seed):
        rng = np.random.default_rng(9000 + seed)
        T = self.TOTAL
        s = np.frombuffer(_random(rng, T, "ACGT").encode(), dtype=np.uint8).copy()
        low = np.zeros(T, dtype=bool)
        self.seams = {"tile": [4096 * (3 + 3 * j) for j in range(20)],
                      "lane": [64 * (4200 + 37 * j) for j in range(20)],
                      "load32": [32 + 64 * (5200 + 37 * j) for j in range(20)],
                      "record": [400001 + 5003 * j for j in range(20)],
                      "block": [BLOCK, 2 * BLOCK], "end": [T]}
        assert all(p % 4096 for p in self.seams["lane"]) and all(p % 64 == 32 for p in self.seams["load32"])
        self.plants = []                                                             # (what, kind, seam, "first" | "last", offset, a, b)
        for kind in ("lane", "load32", "tile", "record"):
            for j, p in enumerate(self.seams[kind]):
                what = "N" if j < 10 else "mask"
                L = (self.PLANT_LENGTHS if j < 10 else self.MASK_PLANT_LENGTHS)[(j + SEAM_KINDS.index(kind)) % 10]
                k = j % 10
                if k < 5:
                    a, b, side, d = p + k - 2, p + k - 2 + L, "first", k - 2
                else:
                    a, b, side, d = p + k - 7 - L + 1, p + k - 7 + 1, "last", k - 7
                _lay(s, low, a, b, what)
                self.plants.append((what, kind, p, side, d, a, b))
        b1, b2 = self.seams["block"]
        for what, p, ds in (("N", b1, (-2, 0, 2)), ("N", b2, (-1, 1)), ("mask", b1, (-1, 1)), ("mask", b2, (-2, 0, 2))):
            for d in ds:
                _lay(s, low, p + d, p + d + 1, what)
                self.plants += [(what, "block", p, "first", d, p + d, p + d + 1), (what, "block", p, "last", d, p + d, p + d + 1)]
        _lay(s, low, T - 2, T, "N")
        self.plants += [("N", "end", T, "first", -2, T - 2, T), ("N", "end", T, "last", -1, T - 2, T)]
        _lay(s, low, T - 1, T, "mask")
        self.plants += [("mask", "end", T, "first", -1, T - 1, T), ("mask", "end", T, "last", -1, T - 1, T)]
        _lay(s, low, 0, 2, "N")
        _lay(s, low, 0, 1, "mask")
        self.stream = _finish(s, low)
        cuts = list(self.seams["record"])
        cuts = sorted(cuts + [cuts[3]] + [cuts[7]] * 3)
        self.bounds = [0, 0] + cuts + [T, T]
        self.records = _cut(self.stream, self.bounds)
        self.text = fasta(self.records, 61)

    def coverage(self):
        """{(what, kind, side): offsets} of the plants that ARE maximal stretches of the stream with that first / last base."""
        runs = {"N": {(m.start(), m.end()) for m in re.finditer("[Nn]+", self.stream)}, "mask": {(m.start(), m.end()) for m in re.finditer("[a-z]+", self.stream)}}
        cov = {}
        for what, kind, p, side, d, a, b in self.plants:
            if (a, b) in runs[what] and (a if side == "first" else b - 1) == p + d:
                cov.setdefault((what, kind, side), set()).add(d)
        return cov


class Case:
    """name, the input text and how it is archived, and the queries: (class text or None, set, each, masked, min_lens)."""

    def __init__(self, name, text, queries, seq_type=0, no_mask=False, records=None, r7=False):
        self.name, self.text, self.queries, self.seq_type, self.no_mask, self.records, self.r7 = name, text, queries, seq_type, no_mask, records, r7


def _around(lengths):
    return tuple(sorted({m for L in lengths for m in (L - 1, L, L + 1) if m >= 1}))


def queries(min_lens=(1, 2, 10, 100), mask_lens=None, more=()):
    """The five questions every text is asked -- N, ^N, -, ACGT with each, the mask -- at the given min_lens (homopolymers: those up to 3,
    and 10; a random background has hardly a longer one)."""
    q = [("N", 0x8000, False, False, min_lens), ("^N", 0x7FFF, False, False, min_lens), ("-", 0x0001, False, False, min_lens[:2]),
         ("ACGT", 0x0116, True, False, tuple(m for m in min_lens if m <= 3) + (10,)), (None, 0, False, True, mask_lens or min_lens)]
    return q + list(more)


def seams_case(seed):
    S = RunSeams(seed)
    c = Case("seams", S.text, queries(_around(RunSeams.PLANT_LENGTHS), _around(RunSeams.MASK_PLANT_LENGTHS)), records=S.records)
    c.seams = S
    return c


def lengths_case(seed):
    """N runs of every length of LENGTHS, each at a phase of its own; the one of 4097 lies across the first block seam, the last one ends at
    the stream's last base but one (its last base at offset -2 of the stream's end).  Lower-case stretches of the same lengths elsewhere."""
    rng = np.random.default_rng(9100 + seed)
    T = 330003
    s = np.frombuffer(_random(rng, T, "ACGT").encode(), dtype=np.uint8).copy()
    low = np.zeros(T, dtype=bool)
    at, laid = 1000, []
    for k, L in enumerate(LENGTHS):
        a = BLOCK - 2000 if L == 4097 else at + 7 * k + 1
        _lay(s, low, a, a + L, "N")
        laid.append((a, a + L))
        if L != 4097:
            at = a + L + 3000
    _lay(s, low, T - 66, T - 1, "N")
    laid.append((T - 66, T - 1))
    at = 60000
    for k, L in enumerate(LENGTHS + MASK_LENGTHS):
        _lay(s, low, at + 5 * k, at + 5 * k + L, "mask")
        at += L + 2500
    assert at < BLOCK - 2100 and all(b <= T for _, b in laid)
    stream = _finish(s, low)
    bounds = [0, 500, 500, 200001, T]
    recs = _cut(stream, bounds)
    c = Case("lengths", fasta(recs, 80), queries(_around(LENGTHS), _around(LENGTHS + MASK_LENGTHS)), records=recs)
    c.laid, c.stream = laid, stream
    return c


def record_ends_case(seed):
    """Runs up to a record's last base and from the next record's base 0 -- directly, with one and with three empty records between --, a
    record that lies wholly inside one class run, runs on the first and on the last base of the stream; the same for N, for '-' and for
    lower case.  The stream is odd and ends in a '-': behind it lies the padding nibble, whose code is that of '-'."""
    rng = np.random.default_rng(9200 + seed)

    def bg(n):
        return _random(rng, n, "ACGT")
    recs = ["", "NN" + bg(1000) + "NNNN", "NNN" + bg(501) + "NN", "", "NNNNN" + bg(300) + "n", "", "", "", "N" + bg(4100) + "nnn", "NNNNNNN",
            "NN" + bg(777) + "--", "-" + bg(64) + "acgt", "ac" + bg(63) + "tt", "tttt", "ttA" + bg(4095) + "--", "", "---" + bg(130) + "N", "", "", "-"]
    recs[1] = "n" + recs[1][1:]                                                       # the text's first letter is lower case ...
    if sum(len(r) for r in recs) % 2 == 0:
        recs[4] = recs[4][:7] + "A" + recs[4][7:]
    assert sum(len(r) for r in recs) % 2 == 1
    c = Case("record_ends", fasta(recs, 70), queries((1, 2, 3, 4, 7, 8), (1, 2, 4, 5), more=[("N-", 0x8001, False, False, (1, 3)), ("^-", 0xFFFE, False, False, (1, 100)),
                                                                                          ("T", 0x0002, False, False, (1, 4))]), records=recs)
    return c


def record_ends_masked_case(seed):
    """The same records with the stream's last letter in lower case (a '-' has no lower case, so this text ends in a letter)."""
    c = record_ends_case(seed)
    recs = list(c.records)
    recs[-1] = "c"
    assert sum(len(r) for r in recs) % 2 == 1
    return Case("record_ends_masked", fasta(recs, 70), queries((1, 2, 3), (1, 2, 4, 5)), records=recs)


def all16_case(seed):
    """All sixteen codes, in runs of 1 to 5 of one code; every code is a class of its own over the whole set."""
    rng = np.random.default_rng(9300 + seed)
    parts = []
    while sum(len(p) for p in parts) < 30011:
        parts.append(CODES[int(rng.integers(0, 16))] * int(rng.integers(1, 6)))
    stream = "".join(parts)[:30011]
    b = bytearray(stream.encode())
    for _ in range(60):
        a = int(rng.integers(0, len(b))); e = min(len(b), a + int(rng.integers(1, 300)))
        b[a:e] = bytes(b[a:e]).lower()
    stream = b.decode()
    cuts = sorted(int(x) for x in rng.integers(1, len(stream), 8))
    recs = _cut(stream, [0, 0] + cuts[:4] + [cuts[4]] * 2 + cuts[5:] + [len(stream)])
    more = [(None, ALL, True, False, (1, 2, 3, 5, 6)), (None, ALL, False, False, (1, 1000)), ("RYSWKM", 0x1668, False, False, (1, 2)), ("BDHV", 0x6880, True, False, (1, 4)),
            ("^ACGT", 0xFEE9, False, False, (1, 9))]
    return Case("all16", fasta(recs, 50), queries((1, 2, 5, 6), more=more), records=recs)


def rna_case(seed):
    rng = np.random.default_rng(9400 + seed)
    b = bytearray(_random(rng, 60003, "ACGU" * 4 + "NNUU").encode())
    for _ in range(30):
        a = int(rng.integers(0, len(b))); e = min(len(b), a + int(rng.integers(1, 900)))
        b[a:e] = bytes(b[a:e]).lower()
    stream = b.decode()
    cuts = sorted(int(x) for x in rng.integers(1, len(stream), 4))
    recs = _cut(stream, [0] + cuts + [len(stream)])
    return Case("rna", fasta(recs, 70), queries((1, 2, 3), more=[("U", 0x0002, False, False, (1, 2, 3)), ("acgu", 0x0116, True, False, (2,))]), seq_type=1, records=recs)


def fastq_case(seed):
    """2000 reads of 150 with N runs at read ends: read k ends in k % 4 N's and read k + 1 starts with (k + 1) % 3."""
    rng = np.random.default_rng(9500 + seed)
    recs = []
    for k in range(2000):
        r = list(_random(rng, 150, "ACGT" * 8 + "N"))
        if k % 4:
            r[-(k % 4):] = "N" * (k % 4)
        if k % 3:
            r[:k % 3] = "N" * (k % 3)
        recs.append("".join(r))
    text = "".join("@read%d x\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(recs)).encode()
    return Case("fastq", text, queries((1, 2, 3, 4, 10)), records=recs)


def r7_case(seed):
    c = _locate_r7(seed)                                                            # bases behind the last record: in no run
    return Case("r7", c.text, queries((1, 2, 5)), records=None, r7=True)


def nomask_case(seed):
    rng = np.random.default_rng(9600 + seed)
    b = bytearray(_random(rng, 50001, "ACGTN").encode())
    for _ in range(20):
        a = int(rng.integers(0, len(b))); e = min(len(b), a + int(rng.integers(1, 2000)))
        b[a:e] = bytes(b[a:e]).lower()                                              # lower case in the text, no mask section in the archive
    stream = b.decode()
    cuts = sorted(int(x) for x in rng.integers(1, len(stream), 3))
    recs = _cut(stream, [0] + cuts + [len(stream)])
    return Case("nomask", fasta(recs, 60), queries((1, 2, 3)), no_mask=True, records=[r.upper() for r in recs])


def no_records_case(seed):
    return Case("no_records", b"", queries((1, 5)), records=[])


def planned(seed=0):
    return [seams_case(seed), lengths_case(seed), record_ends_case(seed), record_ends_masked_case(seed), all16_case(seed), rna_case(seed), fastq_case(seed),
            r7_case(seed), nomask_case(seed), no_records_case(seed)]
