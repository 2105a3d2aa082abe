"""The plan of the trim tests (test_trim_cpu.py holds it to its claims, test_gpu_trim.py runs it): the texts, the limits, the expected rows
and the expected trimmed texts.  Pure Python and numpy; nothing here comes from the code under test.

The rule (include/naf_gpu.h): a quality byte b scores limit - ERR[b]; the stretch of a read is its non-empty interval of the largest
positive score sum, the smallest begin among equal sums, then the largest end; none: begin = end = 0.  `model` answers it in O(n) a read
from the prefix sums P: for every end e the best begin is the FIRST position of the smallest P in front of e (a running minimum: Kadane's
recurrence, kept as indices), and of the ends that reach the largest sum the one with the smallest such begin, then the largest, wins.
`brute` tries every interval in a double Python loop and shares no code with it.  Summary / combine is the associative form of the rule,
(total, best prefix, best suffix, best), which the CPU test holds against `model` on random splits.

The planned texts: `#` (Q2) is the background, far below every cutoff between Q13 and Q30, `I` (Q40) the stretch code, far above; the
claims of the plants hold at DESIGN = Q13, where `.` (Q13) scores 0 and one `$` (Q3) costs exactly what ten `8` (Q23) gain.  Three texts:
`seams` (every seam class, cross, dip, tie, short, filters; about 660 kB of quality, five zstd blocks), `long`, and `bytes` (a read of all
255 storable byte values).  Every plant is a read
of its own, registered in cells[(class, cell)] with the stretch it claims at DESIGN; the filler between the plants is random reads."""
from fractions import Fraction

import numpy as np

from quality_plan import ERR, fastq, quals_of  # noqa: F401  (the error table is quality_plan's: `decimal` at 60 digits)

ROW_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("ee", "<u8"), ("flags", "<u4"), ("reserved", "<u4")]
KEPT, SHORT, ERRORS = 1, 2, 4
NONE = 2 ** 64 - 1
NO_MAX = 2 ** 64 - 1
LIMITS = {"Q0": ERR[33], "Q2": ERR[35], "Q13": ERR[46], "Q20": ERR[53], "Q30": ERR[63], "Q41": ERR[74], "Q93": ERR[126], "0.05": 214748365, "none": NONE}
assert LIMITS["0.05"] == -(-2 ** 32 // 20) and LIMITS["Q0"] == 2 ** 32                  # ceil(0.05 * 2^32): no table entry
DESIGN = LIMITS["Q13"]
TILE, LANE, LOAD, BLOCK = 4096, 64, 16, 131072
_ERR = np.array(ERR, dtype=np.int64)
assert ERR[ord("$")] - DESIGN == 10 * (DESIGN - ERR[ord("8")]) > 0 and ERR[ord(".")] == DESIGN > ERR[ord("I")] and ERR[ord("#")] > DESIGN


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def stretch(q, limit):
    """(begin, end, ee) of one read's quality bytes"""
    n = len(q)
    a = np.frombuffer(q, dtype=np.uint8)
    e = _ERR[a]
    if limit == NONE:
        return 0, n, int(e.sum())
    if n == 0:
        return 0, 0, 0
    P = np.concatenate([[0], np.cumsum(limit - e)])                                    # |P| < 2^32 * n: exact in int64
    low = np.minimum.accumulate(P[:-1])                                                # the smallest prefix sum in front of end e = i + 1
    idx = np.arange(n)
    first = np.maximum.accumulate(np.where(np.concatenate([[True], P[1:-1] < low[:-1]]), idx, 0))   # where it stands first
    val = P[1:] - low
    best = int(val.max())
    if best <= 0:
        return 0, 0, 0
    ends = np.nonzero(val == best)[0]
    b = int(first[ends].min())
    end = int(ends[first[ends] == b].max()) + 1
    return b, end, (end - b) * limit - best


def flags_of(begin, end, ee, min_len, max_ee):
    f = (SHORT if end - begin < min_len else 0) | (ERRORS if ee > max_ee else 0)
    return f or KEPT


def model(quals, limit, min_len=1, max_ee=NO_MAX, first=0, count=None):
    """(rows, total): total = (reads, kept, bases, kept_bases, kept_ee, n_short, n_errors)"""
    last = len(quals) if count is None else first + count
    rows = np.zeros(last - first, dtype=ROW_DTYPE)
    t = [0] * 7
    for j, r in enumerate(range(first, last)):
        b, e, ee = stretch(quals[r], limit)
        f = flags_of(b, e, ee, min_len, max_ee)
        rows[j] = (r, b, e, ee, f, 0)
        t[0] += 1; t[2] += len(quals[r]); t[5] += bool(f & SHORT); t[6] += bool(f & ERRORS)
        if f == KEPT:
            t[1] += 1; t[3] += e - b; t[4] += ee
    return rows, tuple(t)


def brute(q, limit):
    """(begin, end, ee) by every interval"""
    if limit == NONE:
        return 0, len(q), sum(ERR[v] for v in q)
    best = None
    for b in range(len(q)):
        s = 0
        for e in range(b + 1, len(q) + 1):
            s += limit - ERR[q[e - 1]]
            if s > 0 and (best is None or (s, -b, e) > best):
                best = (s, -b, e)
    if best is None:
        return 0, 0, 0
    s, nb, e = best
    return -nb, e, sum(ERR[v] for v in q[-nb:e])


class Summary:
    """What the kernels keep of a piece of a read: bytes [lo, hi) of it."""

    def __init__(self, lo, hi, tot, pre, suf, best):
        self.lo, self.hi, self.tot, self.pre, self.suf, self.best = lo, hi, tot, pre, suf, best   # pre: (sum, end); suf: (sum, begin); best: (sum, begin, end) or None

    @staticmethod
    def of(q, limit, lo=0):
        S = Summary(lo, lo, 0, (0, lo), (0, lo), None)
        for i, v in enumerate(q):
            s = limit - ERR[v]
            p = lo + i
            S = combine(S, Summary(p, p + 1, s, (s, p + 1) if s >= 0 else (0, p), (s, p) if s >= 0 else (0, p + 1), (s, p, p + 1) if s > 0 else None))
        return S

    def answer(self):
        return (0, 0) if self.best is None else (self.best[1], self.best[2])


def combine(L, R):
    assert L.hi == R.lo
    pre = max(L.pre, (L.tot + R.pre[0], R.pre[1]))                                     # ties: the larger end
    suf = max((R.suf[0], -R.suf[1]), (R.tot + L.suf[0], -L.suf[1]))                    # ties: the smaller begin
    cands = [(b[0], -b[1], b[2]) for b in (L.best, R.best) if b is not None]
    if L.suf[0] + R.pre[0] > 0:
        cands.append((L.suf[0] + R.pre[0], -L.suf[1], R.pre[1]))
    best = max(cands) if cands else None
    return Summary(L.lo, R.hi, L.tot + R.tot, pre, (suf[0], -suf[1]), None if best is None else (best[0], -best[1], best[2]))


def ee_units(x):
    """floor(x * 2^32) of a decimal text, an int or a Fraction"""
    return int(Fraction(x) * 2 ** 32)


# ---- texts -------------------------------------------------------------------------------------------------------------------------
class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.quals, self.pos, self.cells, self.ends = [], 0, {}, []

    def add(self, q, cls=None, cell=None, claim=None):
        """a read; claim: the (begin, end) it is planted to have at DESIGN"""
        k = len(self.quals)
        self.quals.append(bytes(q)); self.pos += len(q)
        if cls:
            self.cells.setdefault((cls, cell), []).append((k, claim))
        return k

    def fill_to(self, p):
        assert p >= self.pos, (p, self.pos)
        while self.pos < p:
            n = min(p - self.pos, int(self.rng.integers(1, 301)))
            self.add(np.frombuffer(b"#+5?I", dtype=np.uint8)[self.rng.integers(0, 5, n)].tobytes())


def _seams_text(seed):
    B = Builder(9500 + seed)
    B.add(b"", "short", "empty first", (0, 0))
    # short reads, all byte values, ties and single bases: in front of the first seam
    for n in (1, 2, 3, 63, 64, 65, 150):
        B.add(b"#" * (n // 3) + b"I" * (n - n // 3), "short", "len %d" % n, (n // 3, n))
    B.add(b"", "short", "empty pair", (0, 0)); B.add(b"", "short", "empty pair", (0, 0))
    for v, cell, claim in ((b"I", "one positive", (0, 1)), (b".", "one zero", (0, 0)), (b"#", "one negative", (0, 0)),
                           (b"." * 40, "only zero", (0, 0)), (b"#" * 40, "only negative", (0, 0)), (b"I8" * 20, "only positive", (0, 40))):
        B.add(v, "tie", cell, claim)
    for fl in (1, 2, 3):
        for fr in (1, 2, 3):
            B.add(b"#" * 4 + b"." * fl + b"I" * 9 + b"." * fr + b"#" * 3, "tie", "flanks %d %d" % (fl, fr), (4, 4 + fl + 9 + fr))
    # dips: one `$` costs what ten `8` gain at DESIGN
    for c, cell in ((11, "less"), (10, "equal"), (9, "more")):
        B.add(b"#" * 3 + b"8" * 30 + b"$" + b"8" * c + b"#" * 2, "dip", cell, (3, 34 + c) if c >= 10 else (3, 33))
        B.add(b"#" * 3 + b"8" * c + b"$" + b"8" * 30 + b"#" * 2, "dip", "mirrored " + cell, (3, 34 + c) if c >= 10 else (4 + c, 34 + c))
    B.add(b"#" + b"8" * 10 + b"$" + b"8" * 10 + b"$" + b"8" * 10 + b"#", "dip", "two equal dips", (1, 33))
    # filters: a stretch of 50 `I`; test_gpu_trim and test_trim_cpu put min_len and max_ee around it
    B.filters = B.add(b"#" * 5 + b"I" * 50 + b"#" * 5, "filters", "stretch", (5, 55))
    # everything that has a place in the stream: (first byte, reads as (bytes, cells, claim)), laid out in stream order below
    jobs = []

    def plant(at, role, cell, L=37, a=5, b=7):
        """a stretch of L `I` whose first (role 0) or last (role 1) base is stream byte `at`"""
        jobs.append((at - a if role == 0 else at - L + 1 - a, [(b"#" * a + b"I" * L + b"#" * b, [("seam", cell)], (a, a + L))]))
    CROSS = b"#" * 2 + b"I" * 15 + b"#" * 13 + b"I" * 20 + b"#" * 13 + b"I" * 15 + b"#" * 2      # the best is [30, 50): ten bases either side of the seam at byte 40
    TIE = b"#" * 15 + b"I" * 10 + b"#" * 10 + b"I" * 10 + b"#" * 15                             # two stretches of equal sum either side of the seam at byte 30: the left one
    # lane and load seams: stretch ends at -2 .. +2
    k = 30
    for kind, off in (("lane", 0), ("load", LOAD)):
        for role in (0, 1):
            for d in range(-2, 3):
                plant(LANE * k + off + d, role, "%s %s %+d" % (kind, ("first", "last")[role], d)); k += 3
    jobs.append((LANE * k - 40, [(CROSS, [("cross", "lane")], (30, 50))])); k += 3
    jobs.append((LANE * k - 30, [(TIE, [("tie", "lane seam")], (15, 25))])); k += 3
    assert LANE * k < 3 * TILE - 100
    # tile seams: stretch ends at -18 .. +18 (the tile origin moves by up to 15 with the stream's address); every 32nd is a block seam and has plants of its own
    seams = [t for t in range(3, 92) if t % 32]
    for role in (0, 1):
        for d in range(-18, 19):
            plant(TILE * seams.pop(0) + d, role, "tile %s %+d" % (("first", "last")[role], d))
    for shift in (0, 9):                                                              # (the seam at the stream's own multiple of 4096, and nine bytes on)
        jobs.append((TILE * seams.pop(0) - 40 + shift, [(CROSS, [("cross", "tile")], (30, 50))]))
        jobs.append((TILE * seams.pop(0) - 30 + shift, [(TIE, [("tie", "tile seam")], (15, 25))]))
    # block seams: last d and first d + 1 in two neighbouring reads; at the fifth a stretch of five bases from -2 to +2, which is the cross case too
    for j, d in enumerate(range(-2, 2)):
        s = BLOCK * (j + 1)
        jobs.append((s + d - 36 - 5, [(b"#" * 5 + b"I" * 37, [("seam", "block last %+d" % d)], (5, 42)), (b"I" * 21 + b"#" * 4, [("seam", "block first %+d" % (d + 1))], (0, 21))]))
    jobs.append((5 * BLOCK - 2 - 19, [(b"#" * 2 + b"I" * 4 + b"#" * 13 + b"I" * 5 + b"#" * 13 + b"I" * 4 + b"#" * 2, [("seam", "block first -2"), ("seam", "block last +2"), ("cross", "block")], (19, 24))]))
    assert B.pos < min(j[0] for j in jobs), B.pos
    for start, reads in sorted(jobs):
        B.fill_to(start)
        for q, cells, claim in reads:
            r = B.add(q)
            for cell in cells:
                B.cells.setdefault(cell, []).append((r, claim))
    # record ends: a stretch's first and last base at -2 .. +2 of a record's end; ends[] are the records behind such an end (first / count cut there)
    B.fill_to(B.pos + 50)
    for d in range(-2, 3):
        if d < 0:
            B.add(b"#" * 5 + b"I" * -d, "seam", "record first %+d" % d, (5, 5 - d)); B.ends.append(len(B.quals))
            B.add(b"#" * 5 + b"I" * 20 + b"#" * (-d - 1), "seam", "record last %+d" % d, (5, 25)); B.ends.append(len(B.quals))
        else:
            B.ends.append(len(B.quals)); B.add(b"#" * d + b"I" * 20 + b"#" * 6, "seam", "record first %+d" % d, (d, d + 20))
            B.ends.append(len(B.quals)); B.add(b"I" * (d + 1) + b"#" * 6, "seam", "record last %+d" % d, (0, d + 1))
    B.fill_to(B.pos + 500)
    # the stream's end (the other two texts end in a stretch's last base at -2 and in one of a single base)
    k = B.add(b"#" * 5 + b"I" * 2, "seam", "stream first -2", (5, 7))
    B.cells[("seam", "stream last -1")] = [(k, (5, 7))]
    B.add(b"", "short", "empty last", (0, 0))
    return B


def _long_text(seed):
    B = Builder(9600 + seed)
    B.add(b"#" * 150)
    for n in (4095, 4096, 4097, 8193, 13001, 300000):
        B.fill_to(-(-B.pos // TILE) * TILE + 7)                                       # seven bytes behind a tile seam
        q = bytearray(b"#" * n)
        q[3:n - 3] = b"I" * (n - 6)
        claim = (3, n - 3)
        if n > 2 * TILE:                                                              # dips of one `#` (62 `I` and more are needed to bridge it) on the tile seams the read crosses
            for s in range(-(-B.pos // TILE) * TILE, B.pos + n - 100, TILE):
                q[s - B.pos] = ord("#")
        B.add(q, "long", "first to last tile %d" % n, claim)
        if n >= 8193:
            q = bytearray(b"#" * n)
            a = 2 * TILE - 7 + 100 if n > 3 * TILE else TILE - 7 + 50                 # inside the read's second or third tile
            q[a:a + 1000] = b"I" * 1000
            B.fill_to(-(-B.pos // TILE) * TILE + 7)
            B.add(q, "long", "middle tile %d" % n, (a, a + 1000))
    B.fill_to(B.pos + 300)
    B.add(b"#" * 5 + b"I" * 20 + b"#", "seam", "stream last -2", (5, 25))
    return B


class Case:
    def __init__(self, name, B):
        self.name, self.quals, self.cells, self.ends = name, B.quals, B.cells, B.ends
        self.filters = getattr(B, "filters", None)
        rng = np.random.default_rng(len(B.quals))
        self.seqs = [np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, len(q))].tobytes() for q in B.quals]
        self.ids = ["r%d" % k for k in range(len(B.quals))]
        self.text = fastq(self.seqs, self.quals, self.ids)
        keep = [k for k, q in enumerate(self.quals) if q and min(q) >= 33 and max(q) <= 126]   # what the tolerant parser of this build's ennaf takes
        self.own_keep = keep
        self.own_quals = [self.quals[k] for k in keep]
        self.own_text = fastq([self.seqs[k] for k in keep], self.own_quals, [self.ids[k] for k in keep])
        self.starts = np.concatenate([[0], np.cumsum([len(q) for q in self.quals])])


def bytes_case(seed):
    """every storable byte value (all but the newline) in one read, among short ones; the oracle's archive only"""
    B = Builder(9700 + seed)
    B.add(b"I" * 10)
    vals = np.array([v for v in range(256) if v != 10], dtype=np.uint8)
    B.rng.shuffle(vals)
    B.add(vals.tobytes(), "short", "all 255 byte values", None)
    B.add(b"#" * 3 + b"I", "seam", "stream first -1", (3, 4))
    return Case("bytes", B)


_cache = {}


def planned(seed=0):
    if seed not in _cache:
        _cache[seed] = [Case("seams", _seams_text(seed)), Case("long", _long_text(seed)), bytes_case(seed)]
    return _cache[seed]


CLASSES = ("seam", "cross", "dip", "tie", "long", "short", "filters")


def coverage(cases):
    """{class: {cell: number of reads}} over all cases"""
    out = {c: {} for c in CLASSES}
    for c in cases:
        for (cls, cell), v in c.cells.items():
            out[cls][cell] = out[cls].get(cell, 0) + len(v)
    return out


def expected_cells():
    """the cells every class must have"""
    want = {c: [] for c in CLASSES}
    for kind, ds in (("lane", range(-2, 3)), ("load", range(-2, 3)), ("tile", range(-18, 19)), ("block", range(-2, 3)), ("record", range(-2, 3))):
        want["seam"] += ["%s %s %+d" % (kind, role, d) for role in ("first", "last") for d in ds]
    want["seam"] += ["stream first -2", "stream first -1", "stream last -2", "stream last -1"]
    want["cross"] = ["lane", "tile", "block"]
    want["dip"] = [m + c for m in ("", "mirrored ") for c in ("less", "equal", "more")] + ["two equal dips"]
    want["tie"] = ["lane seam", "tile seam", "one positive", "one zero", "one negative", "only zero", "only negative", "only positive"] + ["flanks %d %d" % (a, b) for a in (1, 2, 3) for b in (1, 2, 3)]
    want["long"] = ["first to last tile %d" % n for n in (4095, 4096, 4097, 8193, 13001, 300000)] + ["middle tile %d" % n for n in (8193, 13001, 300000)]
    want["short"] = ["len %d" % n for n in (1, 2, 3, 63, 64, 65, 150)] + ["empty first", "empty pair", "empty last", "all 255 byte values"]
    want["filters"] = ["stretch"]
    return want


# ---- the trimmed texts ----------------------------------------------------------------------------------------------------------------
_COMP = bytes.maketrans(b"ACGTUMRWSYKVHDBNacgtumrwsykvhdbn", b"TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn")


def expected_text(fastq_text, n_records, segments, fmt, line_length=0, strands=None):
    """The text of a selection of reads -- segments: (record, begin, end) -- cut out of the oracle's --fastq text of the archive.
    fmt: "fastq", "fasta" (lines of line_length, 0 = one line), "sequences" or "seq"."""
    lines = fastq_text.split(b"\n")
    assert len(lines) == 4 * n_records + 1
    out = []
    for k, (r, b, e) in enumerate(segments):
        head, seq, qual = lines[4 * r][1:], lines[4 * r + 1][b:e], lines[4 * r + 3][b:e]
        if strands and strands[k]:
            name = head.split(b" ", 1)
            head = name[0] + b"/rc" + (b" " + name[1] if len(name) > 1 else b"")
            seq, qual = seq.translate(_COMP)[::-1], qual[::-1]
        if fmt == "fastq":
            out += [b"@", head, b"\n", seq, b"\n+\n", qual, b"\n"]
        elif fmt == "fasta":
            out += [b">", head, b"\n"]
            W = line_length or len(seq)
            out += [seq[i:i + W] + b"\n" for i in range(0, len(seq), W)]
        elif fmt == "sequences":
            out += [seq, b"\n"]
        else:
            out.append(seq)
    return b"".join(out)


def kept_segments(rows):
    return [(int(x["record"]), int(x["begin"]), int(x["end"])) for x in rows if int(x["flags"]) == KEPT]


def status_of(flags):
    return {KEPT: "kept", SHORT: "short", ERRORS: "errors", SHORT | ERRORS: "short,errors"}[int(flags)]


def table(rows, names, lengths):
    """The lines unnaf --trim Q --trim-table prints."""
    out = ["#seq\tlength\tbegin\tend\tee\tstatus\n"]
    for x in rows:
        r = int(x["record"])
        out.append("%s\t%d\t%d\t%d\t%.6f\t%s\n" % (names[r], lengths[r], x["begin"], x["end"], int(x["ee"]) / 2 ** 32, status_of(x["flags"])))
    return "".join(out).encode("latin1")
