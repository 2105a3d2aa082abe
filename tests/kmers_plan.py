"""The plan of the k-mer tests (test_kmers_cpu.py holds it to its claims, test_gpu_kmers.py runs it): the reference, the texts and the
K to test.  Pure Python and numpy; nothing here comes from the code under test.

The reference works on the oracle's --sequences text of an archive (one line per record).  expected_counts upper-cases a line, maps U to T,
turns the letters into 2-bit values (A 0, C 1, G 2, T 3; anything else: invalid), builds the index of every window by numpy shifts -- the
first base the most significant --, keeps the windows without an invalid letter and counts them with np.bincount(minlength=4**k).  With
`canonical` the index of the reverse complement is built the same way from 3 - value, the last base the most significant, and the smaller
one counts.  brute_counts is a plain loop over string slices into a dict; its reverse complement comes from bytes.translate and [::-1].  It
shares no code with expected_counts.

The `seams` text lays single N's and record boundaries around the seams of the sweep -- a lane's 64 bases, a 16-byte load (32 bases), a tile
(4096 bases), a zstd block of the packed stream (128 KiB = 262144 bases), a record's end -- at every offset -12 .. +12, which is every
offset -K .. +K of every tested K; see KmerSeams.  The stream's end has a text of its own per distance from a tile seam: ends_cases."""
import numpy as np

from locate_plan import CODES, _random, fasta, r7_case as _locate_r7
from composition_plan import lines_of                                               # noqa: F401  (the records of a --sequences text)

KMER_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("positions", "<u8"), ("counted", "<u8")]
KS = (1, 2, 3, 4, 5, 6, 7, 8, 11, 12)                                               # both sides of either LDS limit, and the largest table
SEAM_KS = (2, 6, 7, 12)
MAX_K = 12
OFFSETS = tuple(range(-MAX_K, MAX_K + 1))
SEAM_KINDS = ("lane", "load32", "tile", "block", "record")
BOUNDARY_KINDS = ("lane", "tile")
BLOCK = 262144
TILE = 4096
RECORD_LENGTHS = tuple(sorted({0, 1, 63, 64, 65, 4095, 4096, 4097} | {k + d for k in KS for d in (-1, 0, 1)}))

# naf_gpu_kmer_index: (text, canonical) -> (k, index), None = rejected.  Written out, not computed.
INDEX_TABLE = [
    ("A", False, (1, 0)), ("C", False, (1, 1)), ("G", False, (1, 2)), ("T", False, (1, 3)), ("U", False, (1, 3)), ("a", False, (1, 0)), ("u", False, (1, 3)),
    ("A", True, (1, 0)), ("C", True, (1, 1)), ("G", True, (1, 1)), ("T", True, (1, 0)),
    ("AA", False, (2, 0)), ("AC", False, (2, 1)), ("CA", False, (2, 4)), ("TT", False, (2, 15)), ("GT", False, (2, 11)), ("gu", False, (2, 11)),
    ("TT", True, (2, 0)), ("GT", True, (2, 1)), ("AC", True, (2, 1)), ("CG", True, (2, 6)), ("AT", True, (2, 3)), ("TA", True, (2, 12)), ("GC", True, (2, 9)),
    ("ACG", False, (3, 6)), ("CGT", False, (3, 27)), ("CGT", True, (3, 6)), ("TTT", True, (3, 0)),
    ("ACGT", False, (4, 27)), ("ACGT", True, (4, 27)), ("AATT", True, (4, 15)), ("TTAA", True, (4, 240)), ("GGGG", True, (4, 85)), ("CCCC", False, (4, 85)),
    ("GAATTC", False, (6, 2109)), ("GAATTC", True, (6, 2109)), ("GATTACA", False, (7, 9156)), ("TGTAATC", True, (7, 9156)), ("TGTAATC", False, (7, 15117)),
    ("TTTTTTTTTTTT", False, (12, 16777215)), ("TTTTTTTTTTTT", True, (12, 0)), ("AAAAAAAAAAAA", False, (12, 0)), ("ACGTACGTACGT", True, (12, 1776411)),
    ("acgtACGUacgu", False, (12, 1776411)),
    ("", False, None), ("N", False, None), ("ACGN", False, None), ("AC GT", False, None), ("ACGTACGTACGTA", False, None), ("R", True, None), ("A-", False, None),
    ("AC\n", False, None), ("5", False, None), ("ACGTX", True, None),
]
# naf_gpu_kmer_text: (k, index) -> text, None = rejected
TEXT_TABLE = [((1, 0), "A"), ((1, 3), "T"), ((2, 4), "CA"), ((2, 11), "GT"), ((3, 27), "CGT"), ((4, 27), "ACGT"), ((6, 2109), "GAATTC"), ((7, 9156), "GATTACA"),
              ((12, 16777215), "TTTTTTTTTTTT"), ((12, 0), "AAAAAAAAAAAA"), ((12, 1776411), "ACGTACGTACGT"),
              ((0, 0), None), ((13, 0), None), ((1, 4), None), ((2, 16), None), ((12, 16777216), None), ((6, 4096), None)]

_VAL = np.full(256, 255, dtype=np.uint8)
for _k, _ch in enumerate("ACGT"):
    _VAL[ord(_ch)] = _k
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _range(lines, first, count):
    return range(first, len(lines) if count is None else first + count)


def record_kmers(line, k, canonical=False):
    """The indices of the counted k-mers of one record, in position order, as an int64 array."""
    v = _VAL[np.frombuffer(line.upper().replace(b"U", b"T"), dtype=np.uint8)]
    n = len(v) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    bad = np.zeros(n, dtype=bool)
    fwd = np.zeros(n, dtype=np.int64)
    rev = np.zeros(n, dtype=np.int64)
    for i in range(k):
        w = v[i:i + n]
        bad |= w == 255
        w = w.astype(np.int64) & 3
        fwd |= w << (2 * (k - 1 - i))
        rev |= (3 - w) << (2 * i)
    idx = np.minimum(fwd, rev) if canonical else fwd
    return idx[~bad]


def expected_counts(lines, k, canonical=False, per_record=False, first=0, count=None):
    """The tables of records [first, first + count) as a uint64 array of shape (n_rows, 4**k): one row per record, or one for them all."""
    kmers = [record_kmers(lines[r], k, canonical) for r in _range(lines, first, count)]
    if per_record:
        return np.stack([np.bincount(x, minlength=4 ** k).astype(np.uint64) for x in kmers]) if kmers else np.zeros((0, 4 ** k), dtype=np.uint64)
    return np.bincount(np.concatenate(kmers + [np.zeros(0, dtype=np.int64)]), minlength=4 ** k).astype(np.uint64).reshape(1, 4 ** k)


def expected_sparse(lines, k, canonical=False, per_record=False, first=0, count=None):
    """The same tables as (places, values) of their non-zero counters in ascending place, place = row * 4**k + index; no table is made."""
    rng = _range(lines, first, count)
    if not per_record:
        t = expected_counts(lines, k, canonical, False, first, count).ravel()
        nz = np.flatnonzero(t)
        return nz.astype(np.int64), t[nz]
    places, values = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.uint64)]
    for i, r in enumerate(rng):
        u, c = np.unique(record_kmers(lines[r], k, canonical), return_counts=True)
        places.append(u + i * 4 ** k)
        values.append(c.astype(np.uint64))
    return np.concatenate(places), np.concatenate(values)


def expected_rows(lines, k, first=0, count=None):
    """The rows of naf_gpu_unnaf_kmers with PER_RECORD as a KMER_DTYPE array; counted is that of the plain count (canonical: the same)."""
    rng = _range(lines, first, count)
    out = np.zeros(len(rng), dtype=KMER_DTYPE)
    for i, r in enumerate(rng):
        out[i] = (r, 0, len(lines[r]), max(len(lines[r]) - k + 1, 0), len(record_kmers(lines[r], k)))
    return out


def expected_total(lines, k, first=0, count=None):
    """(record, begin, end, positions, counted) of h_total"""
    rows = expected_rows(lines, k, first, count)
    return (len(rows), 0, int(rows["end"].sum()), int(rows["positions"].sum()), int(rows["counted"].sum()))


def brute_counts(lines, k, canonical=False, per_record=False, first=0, count=None):
    """[{k-mer text: count}] per row, by a loop over string slices; letters outside ACGT (after U -> T, upper case) invalidate."""
    out = []
    for r in _range(lines, first, count):
        if per_record or not out:
            out.append({})
        d = out[-1]
        t = bytes(lines[r]).upper().replace(b"U", b"T")
        for s in range(len(t) - k + 1):
            w = t[s:s + k]
            if w.strip(b"ACGT"):
                continue
            if canonical:
                w = min(w, w.translate(_COMP)[::-1])
            d[w] = d.get(w, 0) + 1
    if not per_record and not out:
        out.append({})
    return out


def index_of(text):
    """The index of an upper-case k-mer of ACGT, by positional notation in base 4"""
    return int("".join(str("ACGT".index(ch)) for ch in text), 4)


def as_dicts(table, k):
    """A (n_rows, 4**k) table as brute_counts gives it"""
    out = []
    for row in np.asarray(table):
        d = {}
        for i in np.flatnonzero(row):
            n, t = int(i), []
            for _ in range(k):
                t.append("ACGT"[n & 3]); n >>= 2
            d["".join(reversed(t)).encode()] = int(row[i])
        out.append(d)
    return out


def kmer_names(k, canonical=False, rna=False):
    """The columns of unnaf --kmers K --per-record: every k-mer in index order; with canonical those that are the smaller of the two."""
    out = []
    for i in range(4 ** k):
        n, t = i, []
        for _ in range(k):
            t.append("ACGT"[n & 3]); n >>= 2
        w = "".join(reversed(t))
        if canonical and w.encode().translate(_COMP)[::-1].decode() < w:
            continue
        out.append((i, w.replace("T", "U") if rna else w))
    return out


def cli_total(table, k, rna=False):
    """The lines unnaf --kmers K prints for the one table of a selection"""
    names = dict(kmer_names(k, False, rna))
    row = np.asarray(table).ravel()
    return "".join("%s\t%d\n" % (names[int(i)], row[i]) for i in np.flatnonzero(row)).encode()


def cli_per_record(table, rows, names_of_records, k, canonical=False, rna=False):
    cols = kmer_names(k, canonical, rna)
    out = ["#seq\tlength\tcounted" + "".join("\t" + w for _, w in cols) + "\n"]
    for i, x in enumerate(rows):
        out.append("%s\t%d\t%d" % (names_of_records[int(x["record"])], x["end"], x["counted"]) + "".join("\t%d" % table[i][j] for j, _ in cols) + "\n")
    return "".join(out).encode("latin1")


# ---- texts -------------------------------------------------------------------------------------------------------------------------
class KmerSeams:
    """A stream of 600001 bases (it ends on an odd base), background upper-case ACGT, cut into records.

    n_at[kind]: for every offset d of OFFSETS one seam of the kind with ONE N at seam + d and no other N within MAX_K bases of it, so the
    invalidation reaches across the seam from either side, alone.  lane: multiples of 64 that are none of 4096; load32: 32 + multiples of 64;
    tile: multiples of 4096 that are none of 262144; record: stream positions where a record ends and the next one starts.
    block: a text of this size has two such seams; the N's at even offsets lie around the first and those at odd offsets around the second,
    two bases apart: alone for K = 2, in company for the larger K -- the seams of the other kinds have them alone, and to the sweep a block
    seam is a tile seam.
    cut_at[kind], kind in BOUNDARY_KINDS: for every offset d one seam of the kind with a record boundary at seam + d.
    Empty records: one in front, one at the end, one at record seam 3 and three at record seam 7."""
    TOTAL = 600001

    def __init__(self, seed):
        rng = np.random.default_rng(11000 + seed)
        T = self.TOTAL
        s = np.frombuffer(_random(rng, T, "ACGT").encode(), dtype=np.uint8).copy()
        n = len(OFFSETS)
        self.seams = {"tile": [TILE * (2 + j) for j in range(n)],
                      "lane": [64 * (2001 + 8 * j) for j in range(n)],
                      "load32": [32 + 64 * (2300 + 7 * j) for j in range(n)],
                      "record": [190001 + 1013 * j for j in range(n)],
                      "block": [BLOCK, 2 * BLOCK]}
        self.cut_seams = {"lane": [64 * (2701 + 8 * j) for j in range(n)], "tile": [TILE * (70 + j) for j in range(n)]}
        assert all(p % TILE for p in self.seams["lane"] + self.cut_seams["lane"]) and all(p % 64 == 32 for p in self.seams["load32"])
        assert all(p % BLOCK for p in self.seams["tile"] + self.cut_seams["tile"])
        self.n_at = {}                                                               # kind -> {offset: position of the N}
        for kind in ("tile", "lane", "load32", "record"):
            self.n_at[kind] = {d: p + d for d, p in zip(OFFSETS, self.seams[kind])}
        self.n_at["block"] = {d: self.seams["block"][d & 1] + d for d in OFFSETS}
        for at in self.n_at.values():
            for p in at.values():
                s[p] = ord("N")
        s[T - 3] = ord("N")
        self.cut_at = {kind: {d: p + d for d, p in zip(OFFSETS, self.cut_seams[kind])} for kind in BOUNDARY_KINDS}
        cuts = list(self.seams["record"]) + [p for at in self.cut_at.values() for p in at.values()]
        cuts = sorted(cuts + [self.seams["record"][3]] + [self.seams["record"][7]] * 3)
        self.bounds = [0, 0] + cuts + [T, T]
        self.stream = s.tobytes().decode()
        self.records = [self.stream[a:b] for a, b in zip(self.bounds[:-1], self.bounds[1:])]
        self.text = fasta(self.records, 61)

    def coverage(self):
        """{("N", kind, K): offsets} and {("cut", kind, K): offsets} that the stream and the bounds really have"""
        cov = {}
        ns = np.flatnonzero(np.frombuffer(self.stream.encode(), dtype=np.uint8) == ord("N"))
        bounds = set(self.bounds)
        for K in SEAM_KS:
            for kind in SEAM_KINDS:
                for d, p in self.n_at[kind].items():
                    alone = kind == "block" or int(np.sum(np.abs(ns - p) < MAX_K)) == 1
                    if abs(d) <= K and self.stream[p] == "N" and alone:
                        cov.setdefault(("N", kind, K), set()).add(d)
            for kind in BOUNDARY_KINDS:
                for d, p in self.cut_at[kind].items():
                    if abs(d) <= K and p in bounds:
                        cov.setdefault(("cut", kind, K), set()).add(d)
        return cov


class Case:
    """name, the input text and how it is archived, and the K it is asked at"""

    def __init__(self, name, text, ks=KS, seq_type=0, records=None, r7=False, per_record_ks=(), well_formed=False, own_text=None, own_records=None):
        self.name, self.text, self.ks, self.seq_type, self.records, self.r7, self.per_record_ks = name, text, ks, seq_type, records, r7, per_record_ks
        # well_formed: the text needs the oracle's well-formed parser; own_text / own_records: what this build's ennaf archives instead
        self.well_formed, self.own_text, self.own_records = well_formed, own_text, own_records


def seams_case(seed):
    S = KmerSeams(seed)
    c = Case("seams", S.text, records=S.records)
    c.seams = S
    return c


def ends_cases(seed):
    """The stream ends e = 0 .. MAX_K + 1 bases behind a tile seam -- an even and an odd number of bases, the padding nibble behind the odd
    ones --, with an N at offset -((e mod MAX_K) + 1) of the end: every offset -1 .. -MAX_K once at the least.  Two records; the first
    ends 5 bases in front of the tile seam."""
    out = []
    for e in range(MAX_K + 2):
        rng = np.random.default_rng(11100 + 20 * seed + e)
        T = 2 * TILE + e
        s = list(_random(rng, T, "ACGT"))
        d = -((e % MAX_K) + 1)
        s[T + d] = "N"
        s = "".join(s)
        recs = [s[:2 * TILE - 5], s[2 * TILE - 5:]]
        c = Case("end%d" % e, fasta(recs, 70), ks=SEAM_KS, records=recs)
        c.end_offset, c.behind_tile = d, e
        out.append(c)
    return out


def _records(seed, letters="ACGT"):
    rng = np.random.default_rng(11200 + seed)

    def bg(n):
        return _random(rng, n, letters)
    recs = ["", ""] + [bg(n) for n in RECORD_LENGTHS] + ["", "", ""]
    recs += ["N" * 5, "N" * 64, "n" * 100, CODES * 3, "".join(rng.permutation(list(CODES * 40))), bg(300) + "R" + bg(11) + "Y" + bg(12) + "-" + bg(13) + "N" + bg(200)]
    low = bg(5000)
    recs += [low[:1000] + low[1000:2500].lower() + low[2500:4000] + low[4000:].lower(), bg(2000).lower(), _random(rng, 3000, letters + "N"), ""]
    if sum(len(r) for r in recs) % 2 == 0:
        recs[-2] += "A"
    assert sum(len(r) for r in recs) % 2 == 1
    return recs


def records_case(seed):
    recs = _records(seed)
    return Case("records", fasta(recs, 70), records=recs, per_record_ks=(1, 2, 3, 4, 5, 6, 7, 8))


def rna_case(seed):
    """The records text with U for T, archived as RNA: the same tables"""
    recs = [r.replace("T", "U").replace("t", "u") for r in _records(seed)]
    return Case("rna", fasta(recs, 70), seq_type=1, records=recs, per_record_ks=(3, 6))


READ_LENGTHS = tuple(range(19)) + (31, 32, 33, 150)


def _fastq(recs):
    return "".join("@read%d x\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in recs).encode()


def reads_case(seed):
    """A FASTQ text of 4002 reads of 0 to 18, 31, 32, 33 and 150 bases, an N here and there: every tile holds many records.  A read of no
    bases has a form only the oracle's well-formed parser takes (the tolerant one, which this build's ennaf follows, skips the blank
    quality line), so this build archives the same reads without the empty ones (own_text)."""
    rng = np.random.default_rng(11300 + seed)
    recs = [_random(rng, READ_LENGTHS[k % len(READ_LENGTHS)], "ACGT" * 12 + "N") for k in range(174 * len(READ_LENGTHS))]
    full = [r for r in recs if r]
    return Case("reads", _fastq(enumerate(recs)), records=recs, per_record_ks=(1, 2, 3, 4, 5, 6, 7, 8), well_formed=True,
                own_text=_fastq((k, r) for k, r in enumerate(recs) if r), own_records=full)


def palindromes_case(seed):
    """Dense in k-mers that are their own reverse complement (K = 2, 4, 6, 12) and in pairs of a k-mer and its reverse complement"""
    rng = np.random.default_rng(11400 + seed)
    pairs = []
    for _ in range(200):
        w = _random(rng, 12, "ACGT")
        pairs.append(w + w.encode().translate(_COMP)[::-1].decode())
    recs = ["ACGT" * 500, "AATT" * 300 + "AT" * 200 + "TA" * 100 + "CG" * 100 + "GC" * 100, "GAATTC" * 300 + "TTTAAA" * 50, "GAATTCGAATTC" * 100 + "ACGTACGTACGT" * 30 + "AAAAAATTTTTT" * 30,
            "".join(pairs), "".join(pairs).lower()]
    return Case("palindromes", fasta(recs, 80), ks=(2, 4, 6, 12, 3, 7), records=recs, per_record_ks=(2, 4, 6))


def lowk_case(seed):
    """One repeated letter -- every lane on the same bin -- and random text, for K = 1, 2, 3"""
    rng = np.random.default_rng(11500 + seed)
    recs = ["A" * 10000, "T" * 5001, _random(rng, 20000, "ACGT"), "c" * 4096]
    return Case("lowk", fasta(recs, 100), ks=(1, 2, 3, 4), records=recs, per_record_ks=(1, 2, 3))


def two_records_case(seed):
    rng = np.random.default_rng(11600 + seed)
    recs = [_random(rng, 3001, "ACGT" * 10 + "N"), _random(rng, 2500, "ACGT")]
    return Case("two_records", fasta(recs, 60), ks=(12,), records=recs, per_record_ks=(12,))


def r7_case(seed):
    c = _locate_r7(seed)                                                            # bases behind the last record: in no k-mer
    return Case("r7", c.text, ks=(1, 4, 7, 12), records=None, r7=True, per_record_ks=(4,))


def no_records_case(seed):
    return Case("no_records", b"", ks=(1, 6, 12), records=[])


def planned(seed=0):
    return [seams_case(seed), records_case(seed), rna_case(seed), reads_case(seed), palindromes_case(seed), lowk_case(seed), two_records_case(seed), r7_case(seed),
            no_records_case(seed)] + ends_cases(seed)
