"""The plan of the quality-statistics tests (test_quality_cpu.py holds it to its claims, test_gpu_quality.py runs it): the texts, the
bin widths and the expected rows.  Pure Python and numpy; nothing here comes from the code under test.

Expected rows work on the quality lines of the oracle's --fastq text of an archive (quals_of: line 4 r + 3 of the text; a quality byte is
never a newline).  record_rows / cycle_rows / hist_of / total_of are numpy; brute does the same with a per-byte Python loop and shares
no code with them.  ERR is the error table, from `decimal` at 60 digits: 2^32 below 33, round_half_up(2^32 * 10^(-(b - 33) / 10)) from 33.

LDS_BINS is the number of cycle bins the count kernel keeps per workgroup (its trace states it; the `long` text is laid around it)."""
from decimal import ROUND_HALF_UP, Decimal, getcontext

import numpy as np

ROW_DTYPE = [("key", "<u8"), ("n", "<u8"), ("sum", "<u8"), ("ee", "<u8"), ("n_q20", "<u8"), ("n_q30", "<u8"), ("min", "<u4"), ("max", "<u4")]
WIDTHS = (1, 2, 63, 64, 65, 100, 4096, 4097, 1 << 40)
MAX_ROWS = 100000                                                                # a width that gives a case more cycle rows than this is dropped from its list
PLANTS = (33, 52, 53, 62, 63, 126)                                               # both thresholds from both sides, the lowest and the highest code
SEAM_KINDS = ("lane", "load", "tile", "block")
BLOCK = 131072
LDS_BINS = 1024


def _err_table():
    getcontext().prec = 60
    out = []
    for b in range(256):
        v = Decimal(2 ** 32) if b < 33 else Decimal(2 ** 32) * Decimal(10) ** (Decimal(33 - b) / Decimal(10))
        out.append(int(v.quantize(Decimal(1), rounding=ROUND_HALF_UP)))
    return out


ERR = _err_table()
_ERR64 = np.array(ERR, dtype=np.uint64)


def quals_of(fastq_text, n_records):
    """The quality lines of a --fastq text: four lines a record, the fourth."""
    lines = fastq_text.split(b"\n")
    assert len(lines) == 4 * n_records + 1 and lines[-1] == b""
    return [lines[4 * r + 3] for r in range(n_records)]


def _select(quals, first, count):
    last = len(quals) if count is None else first + count
    return first, last


def record_rows(quals, first=0, count=None):
    first, last = _select(quals, first, count)
    rows = np.zeros(last - first, dtype=ROW_DTYPE)
    rows["min"] = 255
    for j, r in enumerate(range(first, last)):
        a = np.frombuffer(quals[r], dtype=np.uint8)
        rows[j]["key"] = r
        rows[j]["n"] = len(a)
        if len(a):
            rows[j]["sum"] = int(a.sum(dtype=np.uint64)); rows[j]["ee"] = int(_ERR64[a].sum(dtype=np.uint64))
            rows[j]["n_q20"] = int((a >= 53).sum()); rows[j]["n_q30"] = int((a >= 63).sum())
            rows[j]["min"] = int(a.min()); rows[j]["max"] = int(a.max())
    return rows


def longest(quals, first=0, count=None):
    first, last = _select(quals, first, count)
    return max([len(q) for q in quals[first:last]] + [0])


def n_cycle_rows(quals, W, first=0, count=None):
    return -(-longest(quals, first, count) // W) if W else 0


def cycle_rows(quals, W, first=0, count=None):
    first, last = _select(quals, first, count)
    nb = n_cycle_rows(quals, W, first, count)
    rows = np.zeros(nb, dtype=ROW_DTYPE)
    rows["key"] = np.arange(nb, dtype=np.uint64)
    rows["min"] = 255
    if nb == 0:
        return rows
    a = np.frombuffer(b"".join(quals[first:last]), dtype=np.uint8)
    pos = np.concatenate([np.arange(len(q), dtype=np.int64) for q in quals[first:last]])
    k = pos // W
    ee = _ERR64[a]
    assert float(ee.sum(dtype=np.float64)) < 2.0 ** 53                             # (bincount adds in doubles: exact below 2^53)
    rows["n"] = np.bincount(k, minlength=nb)
    rows["sum"] = np.bincount(k, weights=a, minlength=nb).astype(np.uint64)
    rows["ee"] = np.bincount(k, weights=ee.astype(np.float64), minlength=nb).astype(np.uint64)
    rows["n_q20"] = np.bincount(k, weights=a >= 53, minlength=nb).astype(np.uint64)
    rows["n_q30"] = np.bincount(k, weights=a >= 63, minlength=nb).astype(np.uint64)
    mn = np.full(nb, 255, dtype=np.uint32); mx = np.zeros(nb, dtype=np.uint32)
    np.minimum.at(mn, k, a); np.maximum.at(mx, k, a)
    rows["min"] = mn; rows["max"] = mx
    return rows


def hist_of(quals, first=0, count=None):
    first, last = _select(quals, first, count)
    return [int(v) for v in np.bincount(np.frombuffer(b"".join(quals[first:last]), dtype=np.uint8), minlength=256)]


def total_of(quals, first=0, count=None):
    """(key, n, sum, ee, n_q20, n_q30, min, max) of h_total"""
    first, last = _select(quals, first, count)
    rec = record_rows(quals, first, last - first)
    return (last - first, int(rec["n"].sum()), int(rec["sum"].sum()), int(rec["ee"].sum(dtype=np.uint64)), int(rec["n_q20"].sum()), int(rec["n_q30"].sum()),
            int(rec["min"].min()) if len(rec) else 255, int(rec["max"].max()) if len(rec) else 0)


def as_tuples(rows):
    return [tuple(int(x[f]) for f, *_ in ROW_DTYPE) for x in rows]


def brute(quals, widths, first=0, count=None):
    """(record rows, {W: cycle rows}, hist) as lists of tuples in ROW_DTYPE's order, by one walk over the bytes (no numpy)."""
    first, last = _select(quals, first, count)
    far = max([len(q) for q in quals[first:last]] + [0])
    rec, hist = [], [0] * 256
    cyc = {W: [[k, 0, 0, 0, 0, 0, 255, 0] for k in range(-(-far // W))] for W in widths}
    for r in range(first, last):
        row = [r, 0, 0, 0, 0, 0, 255, 0]
        for i, v in enumerate(quals[r]):
            hist[v] += 1
            for t in [row] + [cyc[W][i // W] for W in widths]:
                t[1] += 1; t[2] += v; t[3] = (t[3] + ERR[v]) % 2 ** 64; t[4] += v >= 53; t[5] += v >= 63; t[6] = min(t[6], v); t[7] = max(t[7], v)
        rec.append(tuple(row))
    return rec, {W: [tuple(t) for t in cyc[W]] for W in widths}, hist


# ---- texts -------------------------------------------------------------------------------------------------------------------------
def fastq(seqs, quals, ids=None):
    out = []
    for k, (s, q) in enumerate(zip(seqs, quals)):
        out += [b"@", (ids[k] if ids else "q%d" % k).encode(), b" w\n", s, b"\n+\n", q, b"\n"]
    return b"".join(out)


def _bases(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


class Case:
    def __init__(self, name, text, widths, quals, seq_type=0, well_formed=False, own_text=None, own_quals=None):
        self.name, self.text, self.quals, self.seq_type, self.well_formed = name, text, quals, seq_type, well_formed
        self.own_text, self.own_quals = own_text, own_quals                          # what this library's own ennaf is given (None: no own archive)
        far = max([len(q) for q in quals] + [0])
        self.widths = tuple(W for W in widths if -(-far // W) <= MAX_ROWS)


class Seams:
    """A quality stream of 600001 bytes, background 34..73 (so a planted 33 is a read's only lowest and a planted 126 its only highest
    code wherever the read holds one of them), cut into reads.  The seams of the count kernel and of the decoder: a lane's 64 bytes, a
    16-byte load (positions 16 mod 64), a tile of 4096 bytes, a zstd block of 128 KiB.

    seams[kind]: the seam positions of the kind that carry plants; for lane, load and tile, in this order:
      [0:3]   record ends at seam - 1, seam, seam + 1
      [3:9]   PLANTS[j] as the last byte before the seam and PLANTS[(j + 3) % 6] as the first byte behind it, j = 0 .. 5; for `tile` a
              record ends 2000 bytes behind every one of these seams, so each pair has a read of its own: the 33 and the 126 before and
              behind a tile seam are their read's only minimum / maximum
    block: 131072 carries the three record ends -- two reads of length 1, holding 52 and 53 -- and 262144, 393216, 524288 the pairs
    (62, 63), (126, 33), (53, 52): the six plants once each side of some block seam.  (A block seam is a tile seam to the count kernel: the
    tile seams carry every plant on both sides.)  Empty reads: in front, two in the middle, one at the end; every other cut keeps the
    reads below 70002 bytes.  `own`: the same reads without the empty ones, for the tolerant parser."""
    TOTAL = 600001

    def __init__(self, seed):
        rng = np.random.default_rng(9000 + seed)
        T = self.TOTAL
        s = rng.integers(34, 74, T).astype(np.uint8)
        step = {"lane": 64, "load": 64, "tile": 4096}
        off = {"lane": 0, "load": 16, "tile": 0}
        first = {"lane": 1001, "load": 3001, "tile": 3}
        self.seams, self.pairs, cuts = {}, [], []
        for kind in ("lane", "load", "tile"):
            ks = [first[kind] + (3 if kind == "tile" else 38) * j for j in range(9)]
            p = self.seams[kind] = [off[kind] + step[kind] * k for k in ks]
            cuts += [p[0] - 1, p[1], p[2] + 1]
            for j in range(6):
                q = p[3 + j]
                s[q - 1], s[q] = PLANTS[j], PLANTS[(j + 3) % 6]
                self.pairs.append((kind, q, PLANTS[j], PLANTS[(j + 3) % 6]))
                if kind == "tile":
                    cuts += [q - 2000, q + 2000]
        b = self.seams["block"] = [BLOCK, 2 * BLOCK, 3 * BLOCK, 4 * BLOCK]
        cuts += [b[0] - 1, b[0], b[0] + 1]
        for q, (u, v) in zip(b, ((52, 53), (62, 63), (126, 33), (53, 52))):
            s[q - 1], s[q] = u, v
            self.pairs.append(("block", q, u, v))
        cuts += [7, 150003, 150003, 150003] + list(range(70001, T, 70001))
        bounds = [0, 0] + sorted(cuts) + [T, T]
        self.bounds = bounds
        self.stream = s.tobytes()
        self.quals = [self.stream[a:e] for a, e in zip(bounds[:-1], bounds[1:])]
        self.seqs = [_bases(rng, len(q)) for q in self.quals]
        self.text = fastq(self.seqs, self.quals)
        keep = [k for k, q in enumerate(self.quals) if q]
        self.own_quals = [self.quals[k] for k in keep]
        self.own_text = fastq([self.seqs[k] for k in keep], self.own_quals, ids=["q%d" % k for k in keep])


def seams_case(seed):
    S = Seams(seed)
    c = Case("seams", S.text, WIDTHS, S.quals, well_formed=True, own_text=S.own_text, own_quals=S.own_quals)
    c.seams = S
    return c


def short_case(seed):
    rng = np.random.default_rng(9100 + seed)
    lens = [int(x) for x in rng.integers(1, 301, 3000)]
    lens[:6] = [1, 2, 63, 64, 65, 300]
    quals = [rng.integers(33, 74, n).astype(np.uint8).tobytes() for n in lens]
    text = fastq([_bases(rng, n) for n in lens], quals)
    return Case("short", text, WIDTHS, quals, own_text=text, own_quals=quals)


def long_case(seed):
    rng = np.random.default_rng(9200 + seed)
    K = LDS_BINS
    lens = [150, K - 1, 70000, 1, K + 1, 300, K, 64]
    quals = [rng.integers(33, 75, n).astype(np.uint8).tobytes() for n in lens]
    text = fastq([_bases(rng, n) for n in lens], quals)
    return Case("long", text, WIDTHS, quals, own_text=text, own_quals=quals)


def allbytes_case(seed):
    rng = np.random.default_rng(9300 + seed)
    vals = [v for v in range(256) if v != 10]
    stream = np.array(vals * 3, dtype=np.uint8)
    rng.shuffle(stream)
    stream = stream.tobytes()
    cuts = sorted(int(x) for x in rng.integers(1, len(stream), 11))
    bounds = [0] + cuts + [len(stream)]
    quals = [stream[a:e] for a, e in zip(bounds[:-1], bounds[1:])]
    quals.insert(4, b"")
    text = fastq([_bases(rng, len(q)) for q in quals], quals)
    return Case("allbytes", text, WIDTHS, quals, well_formed=True)


def protein_case(seed):
    rng = np.random.default_rng(9400 + seed)
    lens = [int(x) for x in rng.integers(1, 500, 40)]
    quals = [rng.integers(33, 127, n).astype(np.uint8).tobytes() for n in lens]
    text = fastq([_bases(rng, n, b"ACDEFGHIKLMNPQRSTVWY") for n in lens], quals)
    return Case("protein", text, WIDTHS, quals, seq_type=2, own_text=text, own_quals=quals)


def no_records_case(seed):
    return Case("no_records", b"", (1, 100), [])


def planned(seed=0):
    return [seams_case(seed), short_case(seed), long_case(seed), allbytes_case(seed), protein_case(seed), no_records_case(seed)]


# ---- the command line's tables -------------------------------------------------------------------------------------------------------
def _stats(x):
    n = int(x["n"])
    if n == 0:
        return "NA\tNA\tNA"
    return "%.4f\t%d\t%d" % (int(x["sum"]) / n - 33, int(x["min"]) - 33, int(x["max"]) - 33)


def table(rows, names):
    """The lines unnaf --quality prints for record rows."""
    out = ["#seq\tlength\tmean\tmin\tmax\tq20\tq30\tee\n"]
    for x in rows:
        out.append("%s\t%d\t%s\t%d\t%d\t%.6f\n" % (names[int(x["key"])], x["n"], _stats(x), x["n_q20"], x["n_q30"], int(x["ee"]) / 2 ** 32))
    return "".join(out).encode("latin1")


def cycle_table(rows, W, far):
    """The lines unnaf --quality --cycles W prints for cycle rows; far: the longest selected read."""
    out = ["#cycle_begin\tcycle_end\tn\tmean\tmin\tmax\tq20\tq30\tee\n"]
    for x in rows:
        k = int(x["key"])
        out.append("%d\t%d\t%d\t%s\t%d\t%d\t%.6f\n" % (k * W + 1, min((k + 1) * W, far), x["n"], _stats(x), x["n_q20"], x["n_q30"], int(x["ee"]) / 2 ** 32))
    return "".join(out).encode("latin1")
