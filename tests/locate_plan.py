"""The plan of the motif-search tests (test_locate_cpu.py holds it to its claims, test_gpu_locate.py runs it): the reference searcher
and the texts and patterns it is asked about.  Pure Python; nothing here comes from the code under test.

The searcher: a pattern letter is the regex character class of the STORED letters it contains (a stored base is a set of nucleotides and
matches a pattern letter that contains all of it; a gap matches nothing), a pattern is a look-ahead `(?=[..][..]..)` so that every start
position is found, overlapping ones too, and the reverse strand is the pattern's reverse complement by the table written out below.

The planted texts: ONE run RUN of 66 letters from {G, T} is laid over every seam of a background from {A, C} so that RUN[32] is the
first base behind the seam; the patterns are the substrings RUN[32 + d : 32 + d + m] for every length m of LENGTHS and every offset
d = -m .. +1, some letters made degenerate (K, N, B -- all contain the letter they replace).  A pattern starts with G or T, so it can
only hit where a run was laid; pattern (m, d) hits at seam + d of every seam -- unless the seam is a record's end and the hit would
straddle it, or the stream ends there."""
import re

import numpy as np

CODES = "-TGKCYSBAWRDMHVN"                                  # the 4-bit code of a stored letter is its index
LETTERS = "ACGTRYSWKMBDHVN"                                 # the pattern letters (U is T)
SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
        "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
# pattern letter -> the stored letters it contains, as a character class
CLASS = {"A": "[A]", "C": "[C]", "G": "[G]", "T": "[T]", "R": "[AGR]", "Y": "[CTY]", "S": "[CGS]", "W": "[ATW]", "K": "[GTK]", "M": "[ACM]",
         "B": "[CGTYSKB]", "D": "[AGTRWKD]", "H": "[ACTYWMH]", "V": "[ACGRSMV]", "N": "[ACGTRYSWKMBDHVN]"}
COMP = str.maketrans("ACGTMRWSYKVHDBN", "TGCAKYWSRMBDHVN")  # as test_gpu_select_strand.COMP_DNA
LENGTHS = (1, 2, 15, 16, 17, 31, 32)
SEAM_KINDS = ("lane", "load32", "tile", "block", "record", "end")


def canon(pattern):
    return pattern.upper().replace("U", "T")


def revcomp(pattern):
    return canon(pattern).translate(COMP)[::-1]


def expected_hits(records_upper, patterns, strands=3, first=0, count=None):
    """[(record, begin, pattern, strand)] in the order of the contract.  records_upper: the records' bases as upper-case str (U or T)."""
    last = len(records_upper) if count is None else first + count
    cols = []
    for pi, pat in enumerate(patterns):
        for s in (0, 1):
            if not strands & (1 << s):
                continue
            p = revcomp(pat) if s else canon(pat)
            rx = re.compile("(?=" + "".join(CLASS[ch] for ch in p) + ")")
            for r in range(first, last):
                pos = np.fromiter((m.start() for m in rx.finditer(records_upper[r].replace("U", "T"))), dtype=np.int64)
                if len(pos):
                    cols.append(np.stack([np.full(len(pos), r, dtype=np.int64), pos, np.full(len(pos), pi, dtype=np.int64), np.full(len(pos), s, dtype=np.int64)], axis=1))
    if not cols:
        return []
    a = np.concatenate(cols)
    a = a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]
    return [tuple(int(v) for v in row) for row in a]


def brute_hits(records_upper, patterns, strands=3, first=0, count=None):
    """The same by a triple loop over the sets (small texts only)."""
    last = len(records_upper) if count is None else first + count
    out = []
    for r in range(first, last):
        t = records_upper[r].replace("U", "T")
        for b in range(len(t)):
            for pi, pat in enumerate(patterns):
                for s in (0, 1):
                    if not strands & (1 << s):
                        continue
                    p = revcomp(pat) if s else canon(pat)
                    if b + len(p) <= len(t) and all(t[b + j] != "-" and set(SETS[t[b + j]]) <= set(SETS[p[j]]) for j in range(len(p))):
                        out.append((r, b, pi, s))
    return out


# ---- texts -------------------------------------------------------------------------------------------------------------------------
def _wrap(s, w=60):
    return "".join(s[i:i + w] + "\n" for i in range(0, len(s), w))


def fasta(records, width=60, ids=None):
    return "".join(">%s some words\n%s" % (ids[k] if ids else "r%d" % k, _wrap(r, width)) for k, r in enumerate(records)).encode()


def _random(rng, n, alphabet):
    return "".join(np.asarray(list(alphabet))[rng.integers(0, len(alphabet), n)]) if n else ""


def _lower_runs(rng, s, n_runs, longest):
    b = bytearray(s.encode())
    for _ in range(n_runs):
        a = int(rng.integers(0, max(len(b), 1))); e = min(len(b), a + int(rng.integers(1, longest)))
        b[a:e] = bytes(b[a:e]).lower()
    return b.decode()


class Planted:
    """A stream of `total` bases from {A, C} with RUN over every seam, cut into records (empty ones in front, in the middle and at the
    end).  seams: [(kind, position)]; a record seam is the stream position where a record ends and the next one starts."""

    def __init__(self, seed, odd):
        rng = np.random.default_rng(7000 + 2 * seed + int(odd))
        self.run = _random(rng, 66, "GT")
        self.total = 300033 if odd else 300032
        rec_seams = [1501, 20000, 100001, 270010]                     # records that start on an odd and on an even base of the stream
        self.seams = ([("lane", 64 * k) for k in (5, 131, 1001)] + [("load32", 32 + 64 * k) for k in (9, 200, 3000)] +
                      [("tile", 4096 * k) for k in (1, 7, 33)] + [("block", 262144)] + [("record", p) for p in rec_seams] + [("end", self.total)])
        s = bytearray(_random(rng, self.total, "AC").encode())
        for kind, p in self.seams:
            w = self.run.encode()[:32] if kind == "end" else self.run.encode()
            s[p - 32:p - 32 + len(w)] = w
        self.stream_upper = s.decode()
        stream = _lower_runs(rng, self.stream_upper, 40, 3000)         # the soft mask plays no part
        cuts = sorted(rec_seams + [777, 150003, 280001])
        bounds = [0, 0] + cuts[:3] + [cuts[3]] * 3 + cuts[4:] + [self.total, self.total]     # empty: record 0, two in the middle, the last
        self.records = [stream[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
        self.records_upper = [r.upper() for r in self.records]
        self.rec_base = bounds[:-1]
        self.text = fasta(self.records)
        self.odd = odd

    def pattern(self, m, d, n_tail=False):
        """RUN[32 + d : 32 + d + m], every third inner letter K, N or B; n_tail: the last letter N."""
        p = list(self.run[32 + d:32 + d + m])
        for j in range(1, m - 1):
            if (j + d + m) % 3 == 0:
                p[j] = "KNB"[(j + m) % 3]
        if n_tail and m > 1:
            p[-1] = "N"
        return "".join(p)

    def patterns(self):
        """[(m, d, n_tail, text)]: every length at every offset -m .. +1, and per length one pattern that ends in N one base on."""
        out = [(m, d, False, self.pattern(m, d)) for m in LENGTHS for d in range(-m, 2)]
        return out + [(m, -m + 1, True, self.pattern(m, -m + 1, True)) for m in LENGTHS if m > 1]

    def windows(self):
        """The stream intervals a run was laid over."""
        return [(p - 32, p if kind == "end" else p + 34) for kind, p in self.seams]

    def to_record(self, g):
        """stream position -> (record, begin): the last record that starts at or before g (empty ones share a base)."""
        r = max(k for k, b in enumerate(self.rec_base) if b <= g and len(self.records[k]))
        return r, g - self.rec_base[r]

    def planted_hit(self, kind, p, m, d):
        """Is the copy of pattern (m, d) at seam p a hit?  It starts at p + d; it must lie inside one record and inside the stream."""
        a, b = p + d, p + d + m
        if b > self.total or (kind == "end" and d > -m):
            return False
        ends = sorted(set(self.rec_base[1:] + [self.total]))
        return not any(a < e < b for e in ends)


def batches(items, n=16):
    return [items[k:k + n] for k in range(0, len(items), n)]


class Case:
    """name, the input text and its sequence type, and the queries: (patterns, strands, first, count)."""

    def __init__(self, name, text, queries, seq_type=0, records_upper=None, r7=False):
        self.name, self.text, self.queries, self.seq_type, self.records_upper, self.r7 = name, text, queries, seq_type, records_upper, r7


def planted_case(seed, odd):
    P = Planted(seed, odd)
    pats = [t for _, _, _, t in P.patterns()]
    q = [(b, 1, 0, None) for b in batches(pats)]
    q.append(([pats[0], pats[3]] + pats[7:21], 3, 0, None))                              # the reverse strand of short patterns: dense in {A, C}
    n = len(P.records)
    # restricted: ranges that start and end in the middle of a tile, on an odd base (record 3 starts at base 1501, record 8 at 150003) and an even one
    q += [(pats[40:56], 1, 3, 5), (pats[100:116], 3, 8, n - 8), (pats[:8], 3, 2, 1), (pats[60:70], 1, 0, 3), (pats[120:], 1, n - 2, 2)]
    c = Case("planted_odd" if odd else "planted_even", P.text, q, records_upper=P.records_upper)
    c.planted = P
    return c


def dense_case(seed):
    rng = np.random.default_rng(7100 + seed)
    recs = ["", "A" * 5000, "a" * 777, "AAAAAAAAAA", "", "N" * 3001, "ACGT" * 1000, _random(rng, 40000, "ACGT"), "T" * 4097, ""]
    body = list(recs[7]); body[1000:1006] = "GAATTC"; body[4090:4096] = "GAATTC"; body[39994:40000] = "GAATTC"; recs[7] = "".join(body)
    sixteen = ["A", "C", "G", "T", "N", "R", "Y", "AC", "GT", "NN", "ACG", "GAATTC", "NGG", "CCN", "W", "S"]
    q = [(["A", "AAA", "N"], 3, 0, None), (["A", "AAA", "N"], 1, 1, 3), (sixteen, 3, 0, None), (["GAATTC"], 3, 7, 1), (["AAA"], 2, 8, 2)]
    return Case("dense", fasta(recs, 80), q, records_upper=[r.upper() for r in recs])


def ambiguity_case(seed):
    rng = np.random.default_rng(7200 + seed)
    recs = [CODES * 3, "".join(rng.permutation(list(CODES * 40))), CODES[::-1] * 5 + "-"]
    q = [(list(LETTERS), 3, 0, None), (list(LETTERS.lower()), 1, 1, 1), (["RY", "NN", "BDHV", "KM", "SW-"[:2]], 3, 0, None)]
    return Case("ambiguity", fasta(recs, 50), q, records_upper=recs)


def rna_case(seed):
    rng = np.random.default_rng(7300 + seed)
    recs = [_random(rng, 30000, "ACGU"), _random(rng, 4099, "ACGUN"), "UUUUGUUUU"]
    q = [(["U", "T", "GU", "gt", "ACGU", "uuuu"], 3, 0, None), (["U"], 2, 2, 1)]
    return Case("rna", fasta(recs, 70), q, seq_type=1, records_upper=recs)


def fastq_case(seed):
    rng = np.random.default_rng(7400 + seed)
    stream = list(_random(rng, 2000 * 150, "ACGT"))
    motif = "GATTACAGATTACA"
    for k in (1, 2, 3, 27, 28, 1000, 1999):                                              # across the end of read k - 1, d = -14 .. +1
        d = -14 + (k * 5) % 16
        a = 150 * k + d
        if a + len(motif) <= len(stream):
            stream[a:a + len(motif)] = motif
    stream[len(stream) - 14:] = motif
    stream = "".join(stream)
    recs = [stream[150 * k:150 * k + 150] for k in range(2000)]
    text = "".join("@read%d x\n%s\n+\n%s\n" % (k, r, "I" * 150) for k, r in enumerate(recs)).encode()
    q = [([motif, "NGG", "TGTAATC"], 3, 0, None), ([motif, "CCN"], 3, 27, 2), (["GATTACA"], 1, 1990, 10)]
    return Case("fastq_reads", text, q, records_upper=recs)


def r7_case(seed):
    """A control byte inside an id puts a base into the stream that no length accounts for: the records are what the lengths
    cut out of the stream and the bases behind the last one are not searched.  The text ends in the motif, so its last letters lie there."""
    rng = np.random.default_rng(7500 + seed)
    a, b = _random(rng, 60000, "ACGTacgtNn"), _random(rng, 50001, "ACGTacgtNn") + "GTTGTTGGTG"
    text = (">big\x01\x02 c\n" + _wrap(a) + ">big2\x05\n" + _wrap(b)).encode()
    q = [(["GTTGTTGGTG", "GTG", "N", "TGGTG"], 3, 0, None), (["GTG"], 1, 1, 1)]
    return Case("surplus", text, q, records_upper=None, r7=True)


def planned(seed=0):
    return [planted_case(seed, False), planted_case(seed, True), dense_case(seed), ambiguity_case(seed), rna_case(seed), fastq_case(seed), r7_case(seed)]


def records_from_sequences_text(text, n_records):
    """The records of the oracle's --sequences text (use_mask=False), upper case: one line each; what follows the last line of a
    malformed archive is not a record."""
    lines = text.decode("latin1").split("\n")
    assert len(lines) >= n_records + 1 or n_records == 0
    return [ln.upper() for ln in lines[:n_records]]
