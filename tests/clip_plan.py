"""The plan of the adapter-clipping tests (test_clip_cpu.py holds it to its claims, test_gpu_clip.py runs it): the model, the brute force,
the texts, the queries and the plants.  Pure Python and numpy; nothing here comes from the code under test.

The rule (include/naf_gpu.h): start x of a record's window [begin, end) overlaps adapter k in L = min(m_k, end - x) letters; it is a
candidate when L >= min_overlap and at most budget[k][L] of the adapter's first L letters mismatch; the clip point is the smallest
candidate, the lowest adapter number at equal x.  `model` answers it for a whole text at once: the mismatch arrays of
locate_near_plan (OK[letter][stored code]) over the concatenated stream, letter j's array shifted by j and counted only where x + j
lies in front of the window's end -- so the sum is over the first L letters --, the first start within budget per record, ties to
the lower adapter number.  `brute` is a triple loop over str and set and shares no code with it.

The planted texts: the background is letters of {A, C}, the adapters are letters of {G, T}: at rate 1/10 and min_overlap 3 an overlap
of L < 10 letters needs L exact G/T and a longer one at least L - floor(L / 10) matches, so the background has no candidate of its
own (test_clip_cpu asserts it) and every clipped row is a plant.  A plant is a read (with the reads around it that it needs) whose
marked base lies at seam + off of a seam of the stream: lane (64 bases), load (16 bytes: 32 bases), tile (4096), block (a zstd block
of 128 KiB of packed bytes: 262144 bases), or is placed by the record's or the stream's end.  It carries the rows it claims under
the queries it was made for."""
from fractions import Fraction

import numpy as np

import locate_near_plan as NP
import locate_plan as LP

ROW_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("adapter", "<u4"), ("mismatches", "<u4"), ("overlap", "<u4"), ("flags", "<u4")]
KEPT, SHORT, ERRORS, CLIPPED = 1, 2, 4, 8
NO_ADAPTER = 2 ** 32 - 1
LANE, LOAD, TILE, BLOCK = 64, 32, 4096, 262144
SEAM_KINDS = ("lane", "load", "tile", "block", "record", "stream")
CELLS = ("first", "end", "budget", "leftmost", "bounds", "stored", "lengths")
OFFSETS = tuple(range(-33, 3))
LENGTHS = (3, 13, 16, 17, 31, 32)


def budgets_of(rate, m):
    """floor(L * rate) for L <= m, at most L - 1, 0 above m and at 0: what naf_gpu_clip_budgets fills"""
    r = Fraction(rate)
    return [0] + [min(L - 1, (L * r.numerator) // r.denominator) if L <= m else 0 for L in range(1, 33)]


class Query:
    """adapters, one table of 33 budgets each, min_overlap"""

    def __init__(self, adapters, min_overlap=3, rate="1/10", budgets=None):
        self.adapters, self.min_overlap = list(adapters), min_overlap
        self.budgets = [list(b) for b in budgets] if budgets else [budgets_of(rate, len(a)) for a in self.adapters]


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def _codes(text):
    return NP._CODE_OF[np.frombuffer(text.upper().encode("latin1"), dtype=np.uint8)]


def clip_points(records, q, windows=None):
    """per record None or (x, adapter, mismatches, overlap); windows: per record (begin, end), None: the whole records"""
    lens = np.array([len(r) for r in records], dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(lens)])
    n = int(base[-1])
    out = [None] * len(records)
    if n == 0:
        return out
    wb = np.array([w[0] for w in windows], dtype=np.int64) if windows is not None else np.zeros(len(records), dtype=np.int64)
    we = np.array([w[1] for w in windows], dtype=np.int64) if windows is not None else lens
    codes = _codes("".join(records))
    bad = np.ascontiguousarray(~NP.OK[:, codes])                                       # bad[letter][g]: stored base g mismatches the letter
    rec_of = np.repeat(np.arange(len(records)), lens)
    x = np.arange(n, dtype=np.int64)
    E = (base[:-1] + we)[rec_of]                                                       # the end of the window that holds position x, as a stream position
    inside = (x >= (base[:-1] + wb)[rec_of]) & (x < E)
    best = {}
    for k, adapter in enumerate(q.adapters):
        letters = LP.canon(adapter)
        m = len(letters)
        d = np.zeros(n, dtype=np.int64)
        for j, ch in enumerate(letters):
            b = np.zeros(n, dtype=bool)
            b[:n - j] = bad[NP.LETTERS.index(ch), j:]
            d += b & (x + j < E)
        L = np.minimum(m, E - x)
        cand = inside & (L >= q.min_overlap) & (d <= np.array(q.budgets[k], dtype=np.int64)[np.clip(L, 0, 32)])
        idx = np.nonzero(cand)[0]
        if not len(idx):
            continue
        recs, firsts = np.unique(rec_of[idx], return_index=True)                      # idx ascends: the first of a record is its smallest
        for r, f in zip(recs.tolist(), firsts.tolist()):
            g = int(idx[f])
            key = (g - int(base[r]), k, int(d[g]), int(L[g]))
            if r not in best or key[:2] < best[r][:2]:
                best[r] = key
    for r, v in best.items():
        out[r] = v
    return out


def flags_of(begin, end, clipped, min_len, errors=False):
    f = (SHORT if end - begin < min_len else 0) | (ERRORS if errors else 0)
    return (f or KEPT) | (CLIPPED if clipped else 0)


def model(records, q, min_len=1, bounds=None, first=0, count=None):
    """(rows, total, per_adapter) -- bounds: per record of the text (begin, end, flags) or None; total = (reads, clipped, kept, bases,
    kept_bases, removed_bases, n_short, n_errors); per_adapter[k][L]"""
    last = len(records) if count is None else first + count
    sel = records[first:last]
    win = [(b[0], b[1]) for b in bounds[first:last]] if bounds is not None else None
    pts = clip_points(sel, q, win)
    rows = np.zeros(len(sel), dtype=ROW_DTYPE)
    t = [0] * 8
    per = [[0] * 33 for _ in q.adapters]
    for j, rec in enumerate(sel):
        b, e = win[j] if win else (0, len(rec))
        errors = bool(bounds is not None and bounds[first + j][2] & ERRORS)
        p = pts[j]
        end, ad, d, L = (p[0], p[1], p[2], p[3]) if p else (e, NO_ADAPTER, 0, 0)
        f = flags_of(b, end, p is not None, min_len, errors)
        rows[j] = (first + j, b, end, ad, d, L, f)
        t[0] += 1; t[1] += p is not None; t[3] += e - b; t[5] += e - end; t[6] += bool(f & SHORT); t[7] += bool(f & ERRORS)
        if f & KEPT:
            t[2] += 1; t[4] += end - b
        if p:
            per[ad][L] += 1
    return rows, tuple(t), per


def _matches(stored, letter):
    s = stored.upper().replace("U", "T")
    return s != "-" and set(LP.SETS[s]) <= set(LP.SETS[letter.upper().replace("U", "T")])


def brute(rec, q, begin=0, end=None):
    """None or (x, adapter, mismatches, overlap) of one record, a base at a time"""
    end = len(rec) if end is None else end
    for x in range(begin, end):
        for k, adapter in enumerate(q.adapters):
            L = min(len(adapter), end - x)
            if L < q.min_overlap:
                continue
            d = 0
            for j in range(L):
                if not _matches(rec[x + j], adapter[j]):
                    d += 1
            if d <= q.budgets[k][L]:
                return x, k, d, L
    return None


def kept_segments(rows):
    return [(int(x["record"]), int(x["begin"]), int(x["end"])) for x in rows if int(x["flags"]) & KEPT]


def status_of(flags):
    return {KEPT: "kept", SHORT: "short", ERRORS: "errors", SHORT | ERRORS: "short,errors"}[int(flags) & 7]


def table(rows, names, lengths):
    """The lines unnaf --adapter ... --clip-table prints."""
    out = ["#seq\tlength\tbegin\tend\tadapter\tmismatches\toverlap\tstatus\n"]
    for x in rows:
        r = int(x["record"])
        out.append("%s\t%d\t%d\t%d\t%s\t%d\t%d\t%s\n" % (names[r], lengths[r], x["begin"], x["end"], "." if int(x["adapter"]) == NO_ADAPTER else str(int(x["adapter"]) + 1),
                                                        x["mismatches"], x["overlap"], status_of(x["flags"])))
    return "".join(out).encode("latin1")


def bud(L):
    return L // 10


# ---- the adapters and the queries -------------------------------------------------------------------------------------------------
def _gt(seed, n):
    return LP._random(np.random.default_rng(seed), n, "GT")


def _flip(s, idx):
    b = list(s)
    for i in idx:
        b[i] = "T" if b[i] == "G" else "G"
    return "".join(b)


def budget_variants():
    """(L, substitutions, how, their places): exactly floor(L / 10) and one more, at the overlap's ends and letters 15 / 16, or either side of its middle"""
    for L in (9, 10, 19, 20, 29, 30):
        for extra in (0, 1):
            nsub = bud(L) + extra
            for how, order in (("ends", [0, L - 1, 15, 16]), ("seam", [L // 2 - 1, L // 2, 0, L - 1])):
                idx = [i for i in order if i < L][:nsub]
                if len(set(idx)) == nsub:
                    yield L, nsub, how, idx


def _tail_free(A):
    """no tail of three or more letters of a copy that is planted NOT to be a candidate is one itself: the read then has no candidate at all"""
    for L, nsub, how, idx in budget_variants():
        if nsub > bud(L):
            s = _flip(A[:L], idx)
            for i in range(1, L - 2):
                if sum(a != b for a, b in zip(s[i:], A)) <= bud(L - i):
                    return False
    return True


class Plan:
    """The adapters (A: 32 letters, its prefixes the shorter ones; B, C: two others) and the queries by name."""

    def __init__(self, seed):
        self.A = next(a for a in (_gt(9800 + seed + 1000 * t, 32) for t in range(4000)) if _tail_free(a))
        self.B, self.C = _gt(9810 + seed, 20), _gt(9820 + seed, 13)
        A = self.A
        self.tbl = [0] + [min(L - 1, L // 10 + 1) for L in range(1, 33)]                 # a caller's own table: one more than floor(L / 10)
        gs = [i for i in range(5, 16) if A[i] == "G"]
        assert len(gs) >= 2, A
        self.iupac_at = (4, gs[0], gs[1])                                                # letters N, R and G of the adapter `iupac`
        I = list(A[:16]); I[4] = "N"; I[gs[0]] = "R"
        self.I = "".join(I)
        self.q = {"m%d" % m: Query([A[:m]]) for m in LENGTHS}
        self.q.update({"o1": Query([A], 1), "o13": Query([A], 13), "tbl": Query([A], 3, budgets=[self.tbl]), "four": Query([A, self.B, self.C, A[:16]]),
                       "iupac": Query([self.I]), "lower": Query([A.lower()]), "rna": Query([A.replace("T", "U")]), "four1": Query([A, self.B, self.C, A[:16]], 1)})


# ---- plants ------------------------------------------------------------------------------------------------------------------------
class Spec:
    """reads: the texts of a job, laid out one behind the other; target: the index of the read that carries the claims; feat: the offset,
    from the job's first base, of the base that is to lie at seam + off (free: no place is asked for).
    claims: [(query, bounds set or None, min_len, (begin, end, adapter, mismatches, overlap, flags))]; bsets: {name: (begin, end, flags)} of the target."""

    def __init__(self, cell, name, reads, target, feat, claims, bsets=None, offs=(0,), free=False):
        self.cell, self.name, self.reads, self.target, self.feat, self.claims, self.bsets, self.offs, self.free = cell, name, reads, target, feat, claims, bsets or {}, offs, free


class Plant:
    """mark: the stream position of the base that was to lie at seam + off (None: the plant was not placed by a position)"""

    def __init__(self, spec, kind, off, record, mark=None):
        self.cell, self.name, self.kind, self.off, self.record, self.claims, self.mark = spec.cell, spec.name, kind, off, record, spec.claims, mark


def _row(begin, wend, p, min_len=1, errors=False):
    """the claimed row: p = None or (x, adapter, mismatches, overlap)"""
    if p is None:
        return (begin, wend, NO_ADAPTER, 0, 0, flags_of(begin, wend, False, min_len, errors))
    return (begin, p[0], p[1], p[2], p[3], flags_of(begin, p[0], True, min_len, errors))


def specs_first(P, rng, pre=40):
    """the first base of the adapter at every offset of the seam: one copy of A serves all six lengths"""
    bg = lambda n: LP._random(rng, n, "AC")
    rd = bg(pre) + P.A + bg(45)
    n = len(rd)
    claims = [("m%d" % m, None, 1, _row(0, n, (pre, 0, 0, m))) for m in LENGTHS]
    claims += [(qn, None, 1, _row(0, n, (pre, 0, 0, 32))) for qn in ("o1", "o13", "tbl", "four", "lower")]
    bsets = {}
    for L in (2, 3, 4, 9, 10, 11, 15, 16, 17, 31, 32):                                   # the same read cut by a bounds row's end
        bsets["end%d" % L] = (0, pre + L, 0)
        claims.append(("m32", "end%d" % L, 1, _row(0, pre + L, (pre, 0, 0, L) if L >= 3 else None)))
    return [Spec("first", "A at the seam", [rd], 0, pre, claims, bsets, OFFSETS)]


def specs_first_record(P, rng):
    """the first base of the adapter at every offset of a record's end: in front of it the end cuts the adapter, behind it the next read holds it"""
    bg = lambda n: LP._random(rng, n, "AC")
    out = []
    for off in OFFSETS:
        if off < 0:
            rd, L = bg(60) + P.A[:-off], -off
            claims = [("m%d" % m, None, 1, _row(0, len(rd), (60, 0, 0, min(m, L)) if min(m, L) >= 3 else None)) for m in LENGTHS]
            out.append(Spec("first", "A at the record's end", [rd], 0, 60, claims, offs=(off,), free=True))
        else:
            rd = bg(off) + P.A + bg(45)
            claims = [("m%d" % m, None, 1, _row(0, len(rd), (off, 0, 0, m))) for m in LENGTHS]
            out.append(Spec("first", "A at the record's end", [bg(60), rd], 1, 60 + off, claims, offs=(off,), free=True))
    return out


def specs_end(P, rng):
    """the read's end cutting the adapter: L letters of it are left"""
    bg = lambda n: LP._random(rng, n, "AC")
    out = []
    for L in (2, 3, 4, 9, 10, 11, 15, 16, 17, 31, 32):
        k = 150 - L if L == 17 else 50
        rd = bg(k) + P.A[:L]
        claims = [("m%d" % m, None, 1, _row(0, len(rd), (k, 0, 0, min(m, L)) if min(m, L) >= 3 else None)) for m in LENGTHS]
        claims += [("o1", None, 1, _row(0, len(rd), (k, 0, 0, L))), ("o13", None, 1, _row(0, len(rd), (k, 0, 0, L) if L >= 13 else None))]
        out.append(Spec("end", "L %d" % L, [rd], 0, len(rd), claims, offs=(-2, -1, 0, 1, 2)))
    return out


def specs_budget(P, rng):
    """exactly budget[L] and budget[L] + 1 substitutions in an overlap of L letters at the read's end; the seam lies inside the overlap"""
    bg = lambda n: LP._random(rng, n, "AC")
    out = []
    for L, nsub, how, idx in budget_variants():
        k = 50
        rd = bg(k) + _flip(P.A[:L], idx)
        hit = nsub <= bud(L)
        assert nsub <= P.tbl[L]                                                          # (the caller's own table takes every one of them)
        claims = [("m32", None, 1, _row(0, len(rd), (k, 0, nsub, L) if hit else None)), ("tbl", None, 1, _row(0, len(rd), (k, 0, nsub, L)))]
        out.append(Spec("budget", "L %d %s %d subs %s" % (L, "at" if hit else "over", nsub, how), [rd], 0, k + L // 2, claims, offs=(0,)))
    return out


def specs_leftmost(P, rng):
    """two candidates in one read: the first with three substitutions, the second exact and a full overlap: the first wins"""
    bg = lambda n: LP._random(rng, n, "AC")
    A3 = _flip(P.A, (0, 15, 31))
    out = []
    for name, gap, feat_second in (("one lane", 2, False), ("neighbouring lanes", 8, True)):
        rd = bg(30) + A3 + bg(gap) + P.A + bg(40)
        x1, x2 = 30, 30 + 32 + gap
        claims = [("m32", None, 1, _row(0, len(rd), (x1, 0, 3, 32))), ("four", None, 1, _row(0, len(rd), (x1, 0, 3, 32)))]
        # one lane: the first starts at seam + 0 and the second 34 on; neighbouring: the second starts at seam + 0, the first 40 in front
        out.append(Spec("leftmost", name, [rd], 0, x2 if feat_second else x1, claims, offs=(0,)))
    rd = bg(20) + P.C + bg(9) + P.A + bg(40)                                            # two adapters at two positions: the position wins over the number
    out.append(Spec("leftmost", "position over number", [rd], 0, 20 + 13 + 9, [("four", None, 1, _row(0, len(rd), (20, 2, 0, 13))), ("m32", None, 1, _row(0, len(rd), (42, 0, 0, 32)))], offs=(0,)))
    rd = bg(25) + P.A + bg(40)                                                          # two adapters at one position: A and its first 16 letters
    out.append(Spec("leftmost", "number at one position", [rd], 0, 25, [("four", None, 1, _row(0, len(rd), (25, 0, 0, 32)))], offs=(0,)))
    return out


def specs_bounds(P, rng, x0=44):
    bg = lambda n: LP._random(rng, n, "AC")
    rd = bg(x0) + P.A + bg(40)
    n = len(rd)
    hit = (x0, 0, 0, 32)
    bsets = {"begin-1": (x0 + 1, n, 0), "begin": (x0, n, 0), "empty": (x0 + 5, x0 + 5, SHORT), "errors": (3, n - 2, ERRORS), "errors short": (n, n, SHORT | ERRORS), "inner": (x0 // 2, x0 + 20, 0)}
    claims = [("m32", "begin-1", 1, _row(x0 + 1, n, None)), ("m32", "begin", 1, _row(x0, n, hit)), ("m32", "empty", 1, _row(x0 + 5, x0 + 5, None)),
              ("m32", "errors", 1, _row(3, n - 2, hit, 1, True)), ("m32", "errors short", 1, _row(n, n, None, 1, True)), ("m32", "inner", 1, _row(x0 // 2, x0 + 20, (x0, 0, 0, 20))),
              ("m32", None, x0 - 1, _row(0, n, hit, x0 - 1)), ("m32", None, x0, _row(0, n, hit, x0)), ("m32", None, x0 + 1, _row(0, n, hit, x0 + 1))]
    assert claims[1][3][5] == SHORT | CLIPPED and claims[6][3][5] == KEPT | CLIPPED and claims[8][3][5] == SHORT | CLIPPED
    return [Spec("bounds", "begin, end, flags and min_len", [rd], 0, x0, claims, bsets, offs=(-1, 0, 1))]


def specs_stored(P, rng, pre=35):
    """stored N, R and '-' inside the overlap against the adapter's N, R and G"""
    bg = lambda n: LP._random(rng, n, "AC")
    out = []
    iN, iR, iG = P.iupac_at
    for st in "NR-":
        for at, letter in ((iN, "N"), (iR, "R"), (iG, "G")):
            copy = list(P.A[:16]); copy[at] = st
            rd = bg(pre) + "".join(copy) + bg(40)
            d = 0 if _matches(st, letter) else 1
            dA = 0 if _matches(st, P.A[at]) else 1                                       # against A itself (a G or a T there)
            claims = [("iupac", None, 1, _row(0, len(rd), (pre, 0, d, 16))), ("m16", None, 1, _row(0, len(rd), (pre, 0, dA, 16))), ("m13", None, 1, _row(0, len(rd), (pre, 0, dA if at < 13 else 0, 13)))]
            out.append(Spec("stored", "stored %s against %s" % (st, letter), [rd], 0, pre + at, claims, offs=(0,)))
    rd = (bg(35) + P.A + bg(40)).lower()
    out.append(Spec("stored", "lower case", [rd], 0, 35, [("m32", None, 1, _row(0, len(rd), (35, 0, 0, 32))), ("lower", None, 1, _row(0, len(rd), (35, 0, 0, 32)))], offs=(0,)))
    return out


def specs_lengths(P, rng):
    """reads of 0 to 3, 31 to 33, 63 to 65, 150 and 4095 to 4097 bases: background only, and with the adapter (or what fits of it) at the end"""
    bg = lambda n: LP._random(rng, n, "AC")
    out = []
    for n in (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 150, 4095, 4096, 4097):
        rd = bg(n)
        out.append(Spec("lengths", "%d plain" % n, [rd], 0, n, [("m32", None, 1, _row(0, n, None)), ("o1", None, 1, _row(0, n, None))], offs=(0,)))
        L = min(n, 32)
        if L:
            rd = bg(n - L) + P.A[:L]
            claims = [("o1", None, 1, _row(0, n, (n - L, 0, 0, L))), ("m32", None, 1, _row(0, n, (n - L, 0, 0, L) if L >= 3 else None))]
            out.append(Spec("lengths", "%d with the adapter" % n, [rd], 0, n, claims, offs=(0,)))
    out.append(Spec("lengths", "all adapter", [P.A], 0, 0, [("m32", None, 1, _row(0, 32, (0, 0, 0, 32))), ("m13", None, 1, _row(0, 32, (0, 0, 0, 13)))], offs=(0,)))
    return out


# ---- texts -------------------------------------------------------------------------------------------------------------------------
class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.pos, self.plants, self.bsets = [], 0, [], {}

    def add(self, rd):
        self.reads.append(rd); self.pos += len(rd)
        return len(self.reads) - 1

    def fill_to(self, p):
        assert p >= self.pos, (p, self.pos)
        while self.pos < p:
            self.add(LP._random(self.rng, min(p - self.pos, int(self.rng.integers(20, 151))), "AC"))

    def job(self, spec, kind, off, at=None):
        """the job's reads, its marked base at stream position `at` (None: where the stream stands)"""
        if at is not None:
            self.fill_to(at - spec.feat)
        first, start = len(self.reads), self.pos
        for rd in spec.reads:
            self.add(rd)
        r = first + spec.target
        self.plants.append(Plant(spec, kind, off, r, start + spec.feat))
        for name, b in spec.bsets.items():
            self.bsets.setdefault(name, {})[r] = b


def _place(B, groups, tile_groups, block, stream):
    """groups: specs laid at every off of theirs over lane and load seams and, free of a place, by their own record's end; tile_groups: specs
    over tile seams, the offs taken in turn; block: [(spec, off)] in front of and behind the one block seam; stream: the spec that ends the text."""
    small = []
    for s in groups:
        for kind in ("lane", "load"):
            small += [(s, kind, off) for off in s.offs if not s.free]
        small.append((s, "record", s.offs[0] if s.free else 0))
    tiles = []
    for k, s in enumerate(tile_groups):
        offs = s.offs if s.cell == "first" else (s.offs[k % len(s.offs)],)
        tiles += [(s, off) for off in offs]
    T = 1
    B.add("")                                                                           # an empty record first
    B.add(LP._random(B.rng, 151, "AC"))                                                 # (the records behind it start on an odd base until a plant sets the place)
    while small or tiles or T <= BLOCK // TILE:
        seam = T * TILE
        if seam == BLOCK:
            (sx, e), sy = block                                                         # a read that ends at seam + e, and one that starts there: its mark lies where it falls
            B.job(sx, "block", e, seam + e)
            B.job(sy, "block", B.pos + sy.feat - seam)
        elif tiles and max(len(r) for r in tiles[0][0].reads) < 4000:
            s, off = tiles.pop(0)
            B.job(s, "tile", off, seam + off)
        # the inside of the tile: lane and load seams four lanes apart, and the free plants
        p = seam + 512
        while small and p + 640 < seam + TILE:
            s, kind, off = small.pop(0)
            if max(len(r) for r in s.reads) >= 4000:
                B.job(s, "tile", 0)                                                      # a read of 4095 to 4097 bases crosses a tile seam wherever it lies
                break
            if kind == "record":
                B.job(s, kind, off)
            else:
                lane = -(-(B.pos + s.feat - off + 8) // LANE) * LANE
                B.job(s, kind, off, lane + (LOAD if kind == "load" else 0) + off)
            p = B.pos
        T = max(T + 1, -(-(B.pos + 400) // TILE))
    B.fill_to(B.pos + 300)
    B.add(""); B.add("")                                                                # an empty pair
    B.fill_to(B.pos + 100)
    B.job(stream, "stream", 0)
    return B


class Case:
    def __init__(self, name, B, fmt="fasta", seq_type=0, lower=True):
        self.name, self.plants, self.bsets, self.seq_type, self.fmt = name, B.plants, B.bsets, seq_type, fmt
        recs = B.reads
        if lower:                                                                       # the soft mask plays no part
            rng = np.random.default_rng(len(recs))
            for k in rng.integers(0, len(recs), 40):
                recs[k] = recs[k].lower() if int(k) % 2 else recs[k][:len(recs[k]) // 2] + recs[k][len(recs[k]) // 2:].lower()
        self.records = recs
        self.records_upper = [r.upper() for r in recs]
        self.ids = ["r%d" % k for k in range(len(recs))]
        self.text = LP.fasta(recs, 80, self.ids)
        self.starts = np.concatenate([[0], np.cumsum([len(r) for r in recs])])

    def bounds(self, bset):
        """the bounds rows of a set: the plants' own, the whole record for every other read"""
        own = self.bsets.get(bset, {})
        return [own.get(r, (0, len(rec), 0)) for r, rec in enumerate(self.records)]


def _seam_case(name, seed, P, makers, tile_makers, block, stream):
    B = Builder(seed)
    groups = [s for mk in makers for s in mk(P, B.rng)]
    tile_groups = [s for mk in tile_makers for s in mk(P, B.rng)]
    pick = lambda mk, word: next(s for s in mk(P, B.rng) if word in s.name)
    (mx, wx, e), (my, wy, kw) = block
    _place(B, groups, tile_groups, [(pick(mx, wx), e), next(s for s in my(P, B.rng, **kw) if wy in s.name)], pick(*stream))
    return Case(name, B)


def long_case(seed, P):
    """reads of 13001 and 300000 bases with one candidate in the first tile and one in the last; the longer one crosses the block seam with a
    candidate on either side of it"""
    B = Builder(9900 + seed)
    bg = lambda n: LP._random(B.rng, n, "AC")
    A3 = _flip(P.A, (0, 15, 31))
    B.add(bg(150))
    rd = list(bg(13001)); rd[100:132] = A3; rd[12950:12982] = P.A
    B.reads.append("".join(rd)); B.pos += 13001
    B.plants.append(Plant(Spec("leftmost", "13001 first and last tile", [], 0, 0, [("m32", None, 1, _row(0, 13001, (100, 0, 3, 32)))]), "tile", 0, 1))
    rd = list(bg(13001)); rd[12950:12982] = P.A                                         # only the last tile has one
    B.reads.append("".join(rd)); B.pos += 13001
    B.plants.append(Plant(Spec("leftmost", "13001 last tile", [], 0, 0, [("m32", None, 1, _row(0, 13001, (12950, 0, 0, 32)))]), "tile", 0, 2))
    B.fill_to(B.pos + 777)
    start = B.pos
    assert start + 300000 > BLOCK + 100 and start < BLOCK - 5000
    rd = list(bg(300000)); a = BLOCK - start
    rd[a - 40:a - 8] = A3; rd[a:a + 32] = P.A; rd[300000 - 32:] = P.A
    B.reads.append("".join(rd)); B.pos += 300000
    r = len(B.reads) - 1
    B.bsets["late"] = {r: (a + 1, 300000, 0)}                                           # behind the begin only the copy in the last tile, at the stream's end, is left
    B.plants.append(Plant(Spec("leftmost", "300000 either side of the block seam", [], 0, 0, [("m32", None, 1, _row(0, 300000, (a - 40, 0, 3, 32)))]), "block", 0, r))
    B.plants.append(Plant(Spec("leftmost", "300000 last tile", [], 0, 0, [("m32", "late", 1, _row(a + 1, 300000, (300000 - 32, 0, 0, 32)))]), "stream", 0, r))
    return Case("long", B, lower=False)


def rna_case(seed, P):
    B = Builder(9950 + seed)
    rng = B.rng
    A = P.A.replace("T", "U")
    for k in range(60):
        B.add(LP._random(rng, int(rng.integers(1, 200)), "AC"))
        if k % 3 == 0:
            x0 = int(rng.integers(0, 50))
            rd = LP._random(rng, x0, "AC") + A[:int(rng.integers(3, 33))]
            B.add(rd)
            B.plants.append(Plant(Spec("stored", "RNA", [], 0, 0, [("m32", None, 1, _row(0, len(rd), (x0, 0, 0, len(rd) - x0)))]), "record", 0, len(B.reads) - 1))
    rd = LP._random(rng, 17, "AC") + A                                                  # the stream ends in the adapter
    B.add(rd)
    B.plants.append(Plant(Spec("stored", "RNA", [], 0, 0, [("m32", None, 1, _row(0, 49, (17, 0, 0, 32))), ("rna", None, 1, _row(0, 49, (17, 0, 0, 32)))]), "stream", 0, len(B.reads) - 1))
    return Case("rna", B, seq_type=1, lower=False)


def tail_case(name, seed, spec):
    """a short text that ends in one plant"""
    B = Builder(seed)
    B.fill_to(700)
    B.job(spec, "stream", 0)
    return Case(name, B, lower=False)


def ones_case(seed):
    """5000 reads of one base"""
    B = Builder(9960 + seed)
    for ch in B.rng.integers(0, 4, 5000):
        B.add("ACGT"[int(ch)])
    return Case("ones", B, lower=False)


def fastq_case(seed, P):
    """reads with qualities, the adapter behind an insert of 20 to 150 bases in every third one, the quality falling towards the end: what
    unnaf_trim gives of it are the bounds of the clip call"""
    B = Builder(9970 + seed)
    rng = B.rng
    quals = []
    for k in range(900):
        n = 150
        ins = int(rng.integers(20, 151)) if k % 3 == 0 else n
        rd = LP._random(rng, ins, "ACGT")
        if ins < n:
            a = _flip(P.A, [int(v) for v in rng.choice(32, int(rng.integers(0, 4)), replace=False)])
            rd = (rd + a + LP._random(rng, n, "ACGT"))[:n]
        B.add(rd)
        drop = int(rng.integers(60, 151))
        q = np.where(np.arange(n) < drop, rng.integers(30, 41, n), rng.integers(2, 25, n)) + 33
        quals.append(bytes(q.astype(np.uint8)))
    c = Case("fastq", B, fmt="fastq", lower=False)
    c.quals = quals
    c.text = b"".join(b"@%s w\n%s\n+\n%s\n" % (i.encode(), r.encode(), q) for i, r, q in zip(c.ids, c.records, quals))
    return c


_cache = {}


def planned(seed=0):
    """(plan, cases)"""
    if seed not in _cache:
        P = Plan(seed)
        cases = [_seam_case("seams0", 9830 + seed, P, (specs_first, specs_first_record, specs_end), (specs_first, specs_end),
                            [(specs_end, "L 17", -1), (specs_first, "A at", {"pre": 2})], (specs_end, "L 17")),
                 _seam_case("seams1", 9840 + seed, P, (specs_budget, specs_leftmost, specs_bounds), (specs_budget, specs_leftmost, specs_bounds),
                            [(specs_budget, "L 20 at 2 subs seam", 0), (specs_bounds, "begin", {"x0": 4})], (specs_budget, "L 20 at 2 subs seam")),
                 _seam_case("seams2", 9850 + seed, P, (specs_stored, specs_lengths), (specs_stored,),
                            [(specs_lengths, "150 with", 0), (specs_stored, "stored N against N", {"pre": 0})], (specs_lengths, "all adapter")),
                 long_case(seed, P), rna_case(seed, P), ones_case(seed), fastq_case(seed, P),
                 tail_case("tail_first", 9860 + seed, specs_first(P, np.random.default_rng(9861 + seed))[0]),
                 tail_case("tail_bounds", 9870 + seed, specs_bounds(P, np.random.default_rng(9871 + seed))[0])]
        _cache[seed] = (P, cases)
    return _cache[seed]


def coverage(cases):
    """{cell: {seam kind: plants}}"""
    out = {c: {k: 0 for k in SEAM_KINDS} for c in CELLS}
    for c in cases:
        for p in c.plants:
            out[p.cell][p.kind] += 1
    return out


def random_reads(seed, n=300):
    """reads over all sixteen codes, short enough for the brute force"""
    rng = np.random.default_rng(9990 + seed)
    return [LP._random(rng, int(rng.integers(0, 90)), LP.CODES if k % 2 else "ACGTGTGTN") for k in range(n)]
