"""The plan of the open-reading-frame tests (test_orfs_cpu.py holds it to its claims, test_gpu_orfs.py runs it): the model, the texts and
the questions.  Pure Python and numpy; nothing here comes from the code under test.

The model works on the oracle's --sequences text of an archive (one line per record).  expected_rows upper-cases a line, maps U to T, turns
the letters into 2-bit values (A 0, C 1, G 2, T 3; anything else: unknown) and builds, for every offset at once, the index of the codon that
begins there and of its reverse complement.  For each strand and each forward offset mod 3 the codons of that frame are one array; the
bounds of the stretches are the places of its stops (with SPLIT_UNKNOWN: and of its unknown codons), found with np.flatnonzero, and the
start codon of a stretch comes from np.searchsorted over the places of the starts.  There is no Python loop over codons.

The planted texts have a background of seeded letters of {A, C, G} only.  Every standard stop on either strand (TAA TAG TGA; seen forward
as TTA CTA TCA) and ATG / CAT holds a T, so such a background has no stop and no start in any of the six frames: every event is a planted
one, and stretches run across many tiles.  A plant is one codon -- TAA (forward stop), TTA (reverse stop), ATG (forward start) or CAT
(reverse start) -- with its first base at seam + d, d = -3 .. +2, of a seam of one kind:
  lane    a multiple of 64 that is none of 4096              load32  32 + a multiple of 64
  tile    a multiple of 4096 that is none of 262144          block   a multiple of 262144 (a raw block of the oracle's packed stream)
  record  a stream position where a record ends and the next one begins
  piece   the same in a text whose every record is a piece of its own at NAF_GPU_ORFS_PIECE = PIECE (the `bounds` text serves both)
  end     the end of the stream; only d = -3, -2, -1: a well-formed stream has no base behind its end (the r7 text has some, and ends in stops)
A block seam takes two plants that do not overlap (d and d + 3), and a text of 600001 bases has two such seams: the seams text comes in six
variants that differ in the plants at their block seams."""
import numpy as np

from locate_plan import _random, _wrap, fasta
from composition_plan import lines_of                                               # noqa: F401  (the records of a --sequences text)

ORF_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("strand", "<u4"), ("frame", "<u2"), ("flags", "<u2")]
STOP3, STOP5 = 1, 2
SPLIT_UNKNOWN, CLOSED = 1, 2
TILE, BLOCK, PIECE = 4096, 262144, 5000
OFFSETS = (-3, -2, -1, 0, 1, 2)
PLANTS = ((0, "stop", "TAA"), (1, "stop", "TTA"), (0, "start", "ATG"), (1, "start", "CAT"))   # strand, what, the letters as stored
SEAM_KINDS = ("lane", "load32", "tile", "block", "record", "piece", "end")
STD_STOPS, STD_STARTS = "TAA,TAG,TGA", "ATG"
N_SEAM_VARIANTS = 6

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}

# naf_gpu_parse_codon_set: text -> set, None = rejected.  Written out, not computed.
CODON_TABLE = [
    ("TAA", 1 << 48), ("TAG", 1 << 50), ("TGA", 1 << 56), ("ATG", 1 << 14), ("AAA", 1), ("TTT", 1 << 63), ("AAC", 2), ("ACA", 16), ("CAA", 1 << 16),
    ("TAA,TAG,TGA", (1 << 48) | (1 << 50) | (1 << 56)), ("TAR,TGA", (1 << 48) | (1 << 50) | (1 << 56)), ("taa,uag,UGA", (1 << 48) | (1 << 50) | (1 << 56)),
    ("ATG,GTG,TTG", (1 << 14) | (1 << 46) | (1 << 62)), ("NTG", (1 << 14) | (1 << 30) | (1 << 46) | (1 << 62)), ("aug", 1 << 14), ("AUG,ATG", 1 << 14),
    ("NNN", (1 << 64) - 1), ("nnn", (1 << 64) - 1), ("TRA", (1 << 48) | (1 << 56)), ("YAA", (1 << 16) | (1 << 48)), ("AAB", 2 | 4 | 8), ("AAD", 1 | 4 | 8), ("AAH", 1 | 2 | 8),
    ("AAV", 1 | 2 | 4), ("AAS", 2 | 4), ("AAW", 1 | 8), ("AAK", 4 | 8), ("AAM", 1 | 2), ("TGA,TGA", 1 << 56),
    ("", None), (",", None), ("TAA,", None), (",TAA", None), ("TAA,,TAG", None), ("TA", None), ("TAAA", None), ("TAA,TA", None), ("TAA,TAGG", None), ("TA-", None), ("---", None),
    ("TAA TAG", None), ("TAA;TAG", None), ("TAX", None), ("T A", None), ("TAA\n", None), ("123", None), ("TAA, TAG", None), ("T", None),
]

_VAL = np.full(256, 255, dtype=np.uint8)
for _k, _ch in enumerate("ACGT"):
    _VAL[ord(_ch)] = _k
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def codon_set(text):
    """The 64-bit set of a comma-separated list of codons, IUPAC letters expanded; positional notation in base 4"""
    if not text:
        return 0
    s = 0
    for item in text.upper().split(","):
        assert len(item) == 3
        for a in IUPAC[item[0]]:
            for b in IUPAC[item[1]]:
                for c in IUPAC[item[2]]:
                    s |= 1 << int("".join(str("ACGT".index(x)) for x in (a, b, c)), 4)
    return s


def revcomp(s):
    return s.encode("latin1").translate(_COMP)[::-1].decode("latin1")


def _range(lines, first, count):
    return range(first, len(lines) if count is None else first + count)


def _member(idx, known, s):
    """known codons whose index is in the set"""
    tab = np.array([(s >> i) & 1 for i in range(64)], dtype=bool)
    return known & tab[idx]


def record_rows(r, line, stops, starts, min_len, strands, flags):
    """The rows of one record, unsorted, as a list of tuples (record, begin, end, strand, frame, flags)"""
    v = _VAL[np.frombuffer(bytes(line).upper().replace(b"U", b"T"), dtype=np.uint8)]
    L = len(v)
    n = L - 2
    if n <= 0:
        return []
    a, b, c = v[0:n].astype(np.int64), v[1:n + 1].astype(np.int64), v[2:n + 2].astype(np.int64)
    known = (a != 255) & (b != 255) & (c != 255)
    idx = [(16 * a + 4 * b + c) & 63, (16 * (3 - c) + 4 * (3 - b) + (3 - a)) & 63]           # as read on strand 0 and on strand 1
    out = []
    for s in (0, 1):
        if not (strands >> s) & 1:
            continue
        stop = _member(idx[s], known, stops)
        start = _member(idx[s], known, starts) if starts else None
        bound = stop | ~known if flags & SPLIT_UNKNOWN else stop
        for f in range(3):
            m = len(bound[f::3])                                                    # the codons of this frame: offsets f, f + 3, ...
            if m == 0:
                continue
            at = np.flatnonzero(bound[f::3])
            lo = np.concatenate(([0], at + 1))                                      # a stretch is codons [lo, hi)
            hi = np.concatenate((at, [m]))
            left = np.concatenate(([False], stop[f::3][at]))                        # a STOP codon bounds it on that side
            right = np.concatenate((stop[f::3][at], [False]))
            keep = hi > lo
            lo, hi, left, right = lo[keep], hi[keep], left[keep], right[keep]
            fl = (np.where(right, STOP3, 0) | np.where(left, STOP5, 0)) if s == 0 else (np.where(left, STOP3, 0) | np.where(right, STOP5, 0))
            if starts:
                st = np.flatnonzero(start[f::3])
                if s == 0:                                                          # the first start at or behind lo
                    j = np.searchsorted(st, lo, side="left")
                    ok = j < len(st)
                    first = np.where(ok, st[np.minimum(j, len(st) - 1)] if len(st) else 0, 0)
                    ok &= first < hi
                    lo = np.where(ok, first, lo)
                else:                                                               # the last start in front of hi
                    j = np.searchsorted(st, hi, side="left") - 1
                    ok = j >= 0
                    last = np.where(ok, st[np.maximum(j, 0)] if len(st) else 0, 0)
                    ok &= last >= lo
                    hi = np.where(ok, last + 1, hi)
                lo, hi, fl = lo[ok], hi[ok], fl[ok]
            begin, end = f + 3 * lo, f + 3 * hi
            keep = end - begin >= min_len
            if flags & CLOSED:
                keep &= (fl & STOP3) != 0
            for x, y, z in zip(begin[keep].tolist(), end[keep].tolist(), fl[keep].tolist()):
                out.append((r, x, y, s, f if s == 0 else (L - y) % 3, z))
    return out


def expected_rows(lines, stops, starts, min_len, strands=3, flags=0, first=0, count=None):
    """The table of records [first, first + count) as an ORF_DTYPE array in the contract's order.  stops, starts: 64-bit sets (starts 0:
    stop to stop)."""
    rows = []
    for r in _range(lines, first, count):
        rows += record_rows(r, lines[r], stops, starts, min_len, strands, flags)
    out = np.array(rows, dtype=ORF_DTYPE) if rows else np.zeros(0, dtype=ORF_DTYPE)
    return out[np.lexsort((out["strand"], out["end"], out["begin"], out["record"]))]


def totals(rows):
    """(n_orfs, n_bases, per_frame) as naf_gpu_unnaf_orfs_count gives them"""
    pf = [int(np.sum((rows["strand"] == s) & (rows["frame"] == f))) for s in (0, 1) for f in range(3)]
    return len(rows), int((rows["end"] - rows["begin"]).sum()), pf


def cli_lines(rows, names):
    """The lines unnaf --orfs prints"""
    return "".join("%s\t%d\t%d\t%s%d\t%d\t%s\t%s\n" % (names[int(x["record"])], x["begin"], x["end"], "-" if x["strand"] else "+", x["frame"] + 1, (x["end"] - x["begin"]) // 3,
                                                    "-" if x["strand"] else "+", "stop" if x["flags"] & STOP3 else "open") for x in rows).encode("latin1")


# ---- the questions ----------------------------------------------------------------------------------------------------------------------
class Q:
    """One question: the sets as text (None: stop to stop), min_len, strands, flags"""

    def __init__(self, stops, starts, min_len, strands=3, flags=0):
        self.stops, self.starts, self.min_len, self.strands, self.flags = stops, starts, min_len, strands, flags
        self.key = (stops, starts, min_len, strands, flags)

    def sets(self):
        return codon_set(self.stops), codon_set(self.starts)

    def __repr__(self):
        return "Q%r" % (self.key,)


DEFAULTS = Q(STD_STOPS, STD_STARTS, 75)                                            # the command line's
DENSEST = Q(STD_STOPS, None, 3)
QS_ALL = [DEFAULTS, DENSEST, Q(STD_STOPS, STD_STARTS, 3), Q(STD_STOPS, STD_STARTS, 3, 3, SPLIT_UNKNOWN), Q(STD_STOPS, None, 3, 3, SPLIT_UNKNOWN),
          Q(STD_STOPS, STD_STARTS, 3, 3, CLOSED), Q(STD_STOPS, None, 3, 1, CLOSED | SPLIT_UNKNOWN), Q(STD_STOPS, STD_STARTS, 3, 2), Q(STD_STOPS, None, 75, 2, CLOSED),
          Q(STD_STOPS, STD_STARTS, 300), Q(STD_STOPS, None, 300, 1), Q("TAA,TAG", "ATG,GTG,TTG", 30), Q("TAA,TAG", "ATG,GTG,TTG", 3, 3, SPLIT_UNKNOWN)]
QS_SEAMS = [DENSEST, Q(STD_STOPS, STD_STARTS, 3), Q(STD_STOPS, STD_STARTS, 75, 3, CLOSED), Q(STD_STOPS, None, 3, 3, SPLIT_UNKNOWN)]


class Case:
    """name, the input text and how it is archived, and the questions it is asked"""

    def __init__(self, name, text, qs, seq_type=0, records=None, r7=False, well_formed=False, own_text=None, own_records=None, plants=()):
        self.name, self.text, self.qs, self.seq_type, self.records, self.r7 = name, text, qs, seq_type, records, r7
        self.well_formed, self.own_text, self.own_records = well_formed, own_text, own_records
        self.plants = list(plants)                                                  # (kind, d, strand, what, stream position of the codon's first base, letters present)


def _plant(s, plants, kind, q, seam):
    """plant number q = 0 .. 23 -- PLANTS[q // 6] at offset OFFSETS[q % 6] -- at `seam` of stream s (a bytearray)"""
    strand, what, letters = PLANTS[q // 6]
    d = OFFSETS[q % 6]
    p = seam + d
    n = min(3, len(s) - p)                                                          # (at the stream's end: the letters that fit)
    s[p:p + n] = letters[:n].encode()
    plants.append((kind, d, strand, what, p, n))


def seams_case(seed, variant=0):
    """600001 bases (the stream ends on an odd base) in five records with bases and three without; see the module's text"""
    rng = np.random.default_rng(12000 + 10 * seed + variant)
    T = 600001
    s = bytearray(_random(rng, T, "ACG").encode())
    plants = []
    for q in range(24):
        _plant(s, plants, "lane", q, 64 * (2001 + 8 * q))
        _plant(s, plants, "load32", q, 32 + 64 * (2300 + 7 * q))
        _plant(s, plants, "tile", q, TILE * (70 + q))
    for b in (0, 1):                                                                # pair number 2 variant + b: plant (kind k, d) and (kind k, d + 3)
        pair = 2 * variant + b
        k, j = pair // 3, pair % 3
        _plant(s, plants, "block", 6 * k + j, BLOCK * (b + 1))
        _plant(s, plants, "block", 6 * k + j + 3, BLOCK * (b + 1))
    codons = ("TAA", "TAG", "TGA", "TTA", "CTA", "TCA", "ATG", "CAT")
    free = np.arange(420000, 580000, 40)
    for p in rng.choice(free[np.abs(free - 2 * BLOCK) > 100], 300, replace=False):  # and some more, away from the seams above
        p = int(p) + int(rng.integers(0, 30))
        s[p:p + 3] = codons[int(rng.integers(0, 8))].encode()
    bounds = [0, 0, 100000, 250001, 400000, 400000, 590000, T, T]
    stream = s.decode()
    recs = [stream[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    c = Case("seams%d" % variant, fasta(recs, 61), QS_SEAMS if variant == 0 else QS_SEAMS[:2], records=recs, plants=plants)
    c.stream = stream
    return c


def bounds_case(seed):
    """25 records of about 4000 bases, each a piece of its own at PIECE; plant q lies around the boundary behind record q"""
    rng = np.random.default_rng(12100 + seed)
    lens = [4001 + int(x) for x in rng.integers(0, 30, 25)]
    bounds = np.concatenate(([0], np.cumsum(lens))).tolist()
    s = bytearray(_random(rng, bounds[-1], "ACG").encode())
    plants = []
    for q in range(24):
        _plant(s, plants, "record", q, bounds[q + 1])
    plants += [("piece",) + p[1:] for p in plants]
    stream = s.decode()
    recs = [stream[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    assert all(PIECE // 2 < len(r) <= PIECE for r in recs)
    c = Case("bounds", fasta(recs, 80), QS_SEAMS, records=recs, plants=plants)
    c.stream = stream
    return c


def ends_cases(seed):
    """The stream ends q bases behind a tile seam with plant (kind, d), d = -3, -2, -1, at its end: a whole codon, two letters, one"""
    out = []
    for k in range(4):
        for j in range(3):
            q = 6 * k + j
            rng = np.random.default_rng(12200 + 40 * seed + q)
            T = 2 * TILE + q
            s = bytearray(_random(rng, T, "ACG").encode())
            plants = []
            _plant(s, plants, "end", q, T)
            stream = s.decode()
            recs = [stream[:TILE + 7], stream[TILE + 7:]]
            c = Case("end%d" % q, fasta(recs, 70), QS_SEAMS[:2], records=recs, plants=plants)
            c.stream = stream
            out.append(c)
    return out


def _records(seed):
    rng = np.random.default_rng(12300 + seed)

    def bg(n):
        return _random(rng, n, "ACG")
    recs = ["", ""]
    for _ in range(8):                                                              # records of 0 .. 8 bases: they begin at every stream position mod 6
        recs += [_random(rng, n, "ACGT") for n in (0, 1, 2, 3, 4, 5, 6, 7, 8, 5, 1, 0, 0, 7)]
    recs += ["TAA", "TTA", "ATG", "CAT", "TA", "A", "ATGTAA", "TTACAT"]
    recs += [bg(30) + "TA", "A" + bg(29), bg(30) + "T", "AA" + bg(31), bg(30) + "AT", "G" + bg(60) + "TAA"]          # TA|A, T|AA, AT|G: no codons
    recs += [bg(30) + "TAATAG" + bg(30), bg(31) + "TTACTA" + bg(32)]                # two stops back to back: an empty stretch
    recs += [bg(3 * TILE)]                                                          # more than two tiles without an event
    for u in "NR-":                                                                 # an unknown letter at each place of a would-be stop and of a codon inside a stretch
        for place in range(3):
            for codon in ("TAA", "TTA", "ATG", "ACG"):
                w = codon[:place] + u + codon[place + 1:]
                recs.append(bg(30) + "ATG" + bg(30) + w + bg(33) + "TGA" + bg(10) + "TCA" + bg(31) + w + bg(30) + "CAT" + bg(8))
    recs += [bg(30) + "TAN" + bg(30) + "TAA" + bg(3), bg(40) + "NTA" + bg(41)]
    recs += [(bg(40) + "atg" + bg(60).lower() + "taa" + bg(10)), (bg(12) + "ttA" + bg(61) + "cAt" + bg(9)).lower()]
    starts = [bg(90) + "TAA" + bg(4),                                               # a stretch with no start
              bg(9) + "ATG" + bg(90) + "TAA" + bg(5),                               # with one
              bg(9) + "ATG" + bg(30) + "ATG" + bg(60) + "TAG" + bg(6),              # a second one downstream
              bg(7) + "TAA" + bg(30) + "ATG" + "TGA" + bg(5),                       # a start as the stretch's last codon
              bg(10) + "TAA" + "ATG" + bg(90) + "TAA" + bg(7)]                      # a start directly behind a stop
    recs += starts + [revcomp(x) for x in starts]
    for L in (0, 3, 6, 72, 75, 78, 297, 300, 303):                                  # ORFs of min_len - 3, min_len, min_len + 3
        for lead in (7, 8, 9):
            x = bg(lead) + "TAG" + ("ATG" + bg(L - 3) if L else "") + "TAA" + bg(5)
            recs += [x, revcomp(x)]
        recs += ["ATG" + bg(L) , revcomp("ATG" + bg(L)), bg(L), bg(L + 1)]          # ended by the record's edge on both sides
    recs += ["", "", ""]
    if sum(len(r) for r in recs) % 2 == 0:
        recs[-4] += "A"
    return recs


def records_case(seed):
    recs = _records(seed)
    assert sum(len(r) for r in recs) % 2 == 1
    return Case("records", fasta(recs, 70), QS_ALL, records=recs)


def rna_case(seed):
    recs = [r.replace("T", "U").replace("t", "u") for r in _records(seed)]
    return Case("rna", fasta(recs, 70), [DEFAULTS, DENSEST, Q("UAA,UAG,UGA", "AUG", 3, 3, SPLIT_UNKNOWN)], seq_type=1, records=recs)


def dense_case(seed):
    """Seeded ACGT, about 300 K bases in 36 records, an N here and there in some of them"""
    rng = np.random.default_rng(12400 + seed)
    recs = [_random(rng, int(n), "ACGT" * 50 + "N" if k % 3 == 0 else "ACGT") for k, n in enumerate(rng.integers(100, 17000, 36))]
    return Case("dense", fasta(recs, 60), QS_ALL, records=recs)


READ_LENGTHS = tuple(range(19)) + (31, 32, 33, 150)


def _fastq(recs):
    return "".join("@read%d x\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in recs).encode()


def reads_case(seed):
    """A FASTQ text of reads of 0 to 18, 31, 32, 33 and 150 bases: every tile holds many records.  A read of no bases has a form only the
    oracle's well-formed parser takes, so this build archives the same reads without the empty ones (own_text)."""
    rng = np.random.default_rng(12500 + seed)
    recs = [_random(rng, READ_LENGTHS[k % len(READ_LENGTHS)], "ACGT" * 12 + "N") for k in range(60 * len(READ_LENGTHS))]
    full = [r for r in recs if r]
    return Case("reads", _fastq(enumerate(recs)), [DENSEST, Q(STD_STOPS, STD_STARTS, 3), Q(STD_STOPS, STD_STARTS, 30, 3, SPLIT_UNKNOWN), Q(STD_STOPS, None, 12, 2, CLOSED)],
                records=recs, well_formed=True, own_text=_fastq((k, r) for k, r in enumerate(recs) if r), own_records=full)


def r7_case(seed):
    """A control byte inside an id puts a base into the stream that no length accounts for: the records are what the lengths
    cut out of the stream and the bases behind the last one are in no codon.  The text ends in stops and starts."""
    rng = np.random.default_rng(12600 + seed)
    a, b = _random(rng, 9000, "ACGTacgtNn"), _random(rng, 7001, "ACGTacgtNn") + "ATGCATTAATTATAGCTA"
    text = (">big\x01\x02 c\n" + _wrap(a) + ">big2\x05\n" + _wrap(b)).encode()
    return Case("r7", text, [DENSEST, Q(STD_STOPS, STD_STARTS, 3), Q(STD_STOPS, None, 3, 3, SPLIT_UNKNOWN)], records=None, r7=True)


def no_records_case(seed):
    return Case("no_records", b"", [DEFAULTS, DENSEST], records=[])


def planned(seed=0):
    return ([seams_case(seed, v) for v in range(N_SEAM_VARIANTS)] + [bounds_case(seed), records_case(seed), rna_case(seed), dense_case(seed), reads_case(seed), r7_case(seed),
            no_records_case(seed)] + ends_cases(seed))


def coverage(cases):
    """{(seam kind, d, strand, what): [case names]} of the plants whose letters the texts really hold at the seams they claim"""
    cov = {}
    for c in cases:
        for kind, d, strand, what, p, n in c.plants:
            letters = next(x[2] for x in PLANTS if x[:2] == (strand, what))
            seam = p - d
            ok = c.stream[p:p + 3] == letters[:n] and n == min(3, len(c.stream) - p)
            if kind == "lane":
                ok &= seam % 64 == 0 and seam % TILE != 0
            elif kind == "load32":
                ok &= seam % 64 == 32
            elif kind == "tile":
                ok &= seam % TILE == 0 and seam % BLOCK != 0
            elif kind == "block":
                ok &= seam % BLOCK == 0 and seam > 0
            elif kind in ("record", "piece"):
                b = np.cumsum([len(r) for r in c.records]).tolist()
                ok &= seam in b[:-1]
            elif kind == "end":
                ok &= seam == len(c.stream) and d < 0
            if ok:
                cov.setdefault((kind, d, strand, what), []).append(c.name)
    return cov


def coverage_cells():
    """every cell the table must have"""
    return [(kind, d, strand, what) for kind in SEAM_KINDS for d in OFFSETS if not (kind == "end" and d >= 0) for strand, what, _ in PLANTS]
