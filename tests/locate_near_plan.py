"""The plan of the tests of the motif search with mismatches (test_locate_near_cpu.py holds it to its claims, test_gpu_locate_near.py runs
it): the model searcher, the texts, the queries and the cells -- the places where a hit is planted, or planted not to be one.  Pure
Python and numpy; nothing here comes from the code under test.

The model: a boolean table OK[pattern letter][stored code] made from the sets of locate_plan.SETS (a stored base is a set of
nucleotides and matches a letter that contains all of it; a gap matches nothing).  Per record the stored codes give, per pattern
letter, the array "this base mismatches that letter"; the mismatches of a pattern at every start are the sum over its letters j of
those arrays shifted by j, a start is a hit when no bracketed letter mismatches, the others' mismatches are within the budget and
b + m <= len; `where` is read from the same arrays at the hits.  brute_near is the same by a triple loop over str and set.

The planted texts are locate_plan.Planted's: ONE run RUN of 66 letters from {G, T} laid over every seam (lane 64, load 32 bytes, tile
4096, zstd block, record end, stream end) of a background from {A, C}, RUN[32] the first base behind the seam, records starting on
odd and on even bases.  The laid copy is the same at every seam, so the substitutions of a copy are made on the side of the pattern:
pattern (m, d, S) is RUN[32 + d : 32 + d + m] with the letters of S changed to the other of G and T.  At seam + d of EVERY seam the
stored bases then differ from it in exactly the letters S -- one cell is tried at all seam kinds at once.  A copy is a hit there when
|S| is within the budget, S avoids the brackets and the window lies inside one record; d runs over -m (the window ends at the seam),
offsets that straddle it and 0, +1 (it starts at or behind the seam), so S = "the letter on either side of the seam" exists."""
import numpy as np

import locate_plan as LP

CODES, LETTERS, SETS, LENGTHS, SEAM_KINDS = LP.CODES, LP.LETTERS, LP.SETS, LP.LENGTHS, LP.SEAM_KINDS
MAX_MISMATCHES = 8
BUDGETS = (0, 1, 2, 3, 8)

# OK[letter][code]: the stored code is not a gap and all of it lies in the letter's set
OK = np.array([[c != 0 and set(SETS[CODES[c]]) <= set(SETS[p]) for c in range(16)] for p in LETTERS], dtype=bool)
_CODE_OF = np.zeros(256, dtype=np.uint8)
for _c, _ch in enumerate(CODES):
    _CODE_OF[ord(_ch)] = _c
_CODE_OF[ord("U")] = CODES.index("T")


def parse(pattern):
    """(letters, fixed): the pattern's letters upper case, U as T, brackets taken out; fixed[j] -- letter j stood in brackets."""
    letters, fixed, inside = [], [], False
    for ch in pattern:
        if ch == "[":
            assert not inside
            inside = True
        elif ch == "]":
            assert inside
            inside = False
        else:
            letters.append(ch)
            fixed.append(inside)
    assert not inside and letters
    return LP.canon("".join(letters)), fixed


def letters_of(pattern):
    return pattern.replace("[", "").replace("]", "")


def fixed_mask(pattern):
    return sum(1 << j for j, f in enumerate(parse(pattern)[1]) if f)


def _oriented(pattern, s):
    """what the stored bases of a window are held against on strand s: (letters, fixed, bit) -- window base i faces pattern letter bit[i]"""
    letters, fixed = parse(pattern)
    m = len(letters)
    if s:
        return LP.revcomp(letters), fixed[::-1], [m - 1 - i for i in range(m)]
    return letters, fixed, list(range(m))


def near_hits(records_upper, patterns, budgets, strands=3, first=0, count=None):
    """int64 rows (record, begin, pattern, strand, mismatches, where) in the order of the contract."""
    last = len(records_upper) if count is None else first + count
    budgets = [budgets] * len(patterns) if isinstance(budgets, int) else list(budgets)
    out = []
    for r in range(first, last):
        rec = records_upper[r]
        if not rec:
            continue
        codes = _CODE_OF[np.frombuffer(rec.encode("latin1"), dtype=np.uint8)]
        bad = np.ascontiguousarray(~OK[:, codes]).astype(np.uint8)         # bad[letter][g]: stored base g mismatches the letter
        for pi, pat in enumerate(patterns):
            for s in (0, 1):
                if not strands & (1 << s):
                    continue
                letters, fixed, bit = _oriented(pat, s)
                m, n = len(letters), len(rec) - len(letters) + 1
                if n <= 0:
                    continue
                li = [LETTERS.index(ch) for ch in letters]
                mism, fix = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
                for j in range(m):
                    if fixed[j]:
                        fix |= bad[li[j], j:j + n]
                    else:
                        mism += bad[li[j], j:j + n]
                idx = np.nonzero((fix == 0) & (mism <= budgets[pi]))[0]
                if not len(idx):
                    continue
                where = np.zeros(len(idx), dtype=np.int64)
                for j in range(m):
                    where |= bad[li[j], idx + j].astype(np.int64) << bit[j]
                out.append(np.stack([np.full(len(idx), r, dtype=np.int64), idx.astype(np.int64), np.full(len(idx), pi, dtype=np.int64),
                                     np.full(len(idx), s, dtype=np.int64), mism[idx].astype(np.int64), where], axis=1))
    if not out:
        return np.zeros((0, 6), dtype=np.int64)
    a = np.concatenate(out)
    return a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]


def brute_near(records_upper, patterns, budgets, strands=3, first=0, count=None):
    """The same, a base at a time (small texts only): a list of tuples."""
    last = len(records_upper) if count is None else first + count
    budgets = [budgets] * len(patterns) if isinstance(budgets, int) else list(budgets)
    out = []
    for r in range(first, last):
        t = records_upper[r].replace("U", "T")
        for b in range(len(t)):
            for pi, pat in enumerate(patterns):
                for s in (0, 1):
                    if not strands & (1 << s):
                        continue
                    letters, fixed, bit = _oriented(pat, s)
                    if b + len(letters) > len(t):
                        continue
                    miss = [not (t[b + j] != "-" and set(SETS[t[b + j]]) <= set(SETS[letters[j]])) for j in range(len(letters))]
                    if any(x and f for x, f in zip(miss, fixed)) or sum(miss) > budgets[pi]:
                        continue
                    out.append((r, b, pi, s, sum(miss), sum(1 << bit[j] for j, x in enumerate(miss) if x)))
    return out


def histogram(rows, n_patterns):
    """[[[hits with d mismatches for d in 0..8] for strand in (0, 1)] for pattern]"""
    h = np.zeros((n_patterns, 2, MAX_MISMATCHES + 1), dtype=np.int64)
    if len(rows):
        np.add.at(h, (rows[:, 2], rows[:, 3], rows[:, 4]), 1)
    return h.tolist()


# ---- queries and cells ---------------------------------------------------------------------------------------------------------------
class Query:
    def __init__(self, patterns, budgets, strands=1, first=0, count=None):
        self.patterns, self.budgets, self.strands, self.first, self.count = list(patterns), list(budgets), strands, first, count
        assert len(self.patterns) == len(self.budgets) and 1 <= len(self.patterns) <= 16

    def key(self):
        return tuple(self.patterns), tuple(self.budgets), self.strands, self.first, self.count


class Place:
    """Cell `cell` at seam kind `kind`: pattern `pat` of query `q` on strand `strand` at (record, begin) -- a hit with `mismatches` and
    `where`, or (mismatches None) no hit."""

    def __init__(self, cell, kind, q, pat, strand, record, begin, mismatches, where):
        self.cell, self.kind, self.q, self.pat, self.strand, self.record, self.begin, self.mismatches, self.where = cell, kind, q, pat, strand, record, begin, mismatches, where


class Case:
    def __init__(self, name, text, seq_type=0, records_upper=None, r7=False):
        self.name, self.text, self.seq_type, self.records_upper, self.r7 = name, text, seq_type, records_upper, r7
        self.queries, self.places = [], []


def _flip(s, idx):
    s = list(s)
    for i in idx:
        s[i] = "T" if s[i] == "G" else "G"
    return "".join(s)


def _offsets(m, few=False):
    """the window ends at the seam, straddles it by one base, lies half over it, straddles it but for one base, starts at it, one behind;
    few: ends at it, half over it, all but one base in front of it, starts at it"""
    return sorted({d for d in ((-m, -(m // 2), -1, 0) if few else (-m, -m + 1, -(m // 2), -1, 0, 1)) if -32 <= d and d + m <= 34})


def _bracket(p, a, b):
    return p[:a] + "[" + p[a:b] + "]" + p[b:]


class _Builder:
    """collects (cell, pattern, budget, strand, m, d, S-as-pattern-bits or None) and packs them into queries of 16 patterns a strand"""

    def __init__(self, P, case):
        self.P, self.case, self.pending = P, case, {1: [], 2: []}

    def add(self, cell, pattern, budget, m, d, where, hit, strand=0):
        self.pending[1 << strand].append((cell, pattern, budget, m, d, where if hit else None, strand))
        if len(self.pending[1 << strand]) == 16:
            self.flush(1 << strand)

    def flush(self, mask=None):
        for sm in ((1, 2) if mask is None else (mask,)):
            items, self.pending[sm] = self.pending[sm], []
            if not items:
                continue
            q = len(self.case.queries)
            self.case.queries.append(Query([it[1] for it in items], [it[2] for it in items], sm))
            for k, (cell, pattern, budget, m, d, where, strand) in enumerate(items):
                self.places(cell, q, k, strand, m, d, where)

    def places(self, cell, q, k, strand, m, d, where):
        P = self.P
        for kind, p in P.seams:
            a = p + d
            if a < 0 or a >= P.total:
                continue                                                         # no start position there (behind the stream's end)
            r, b = P.to_record(a)
            inside = P.planted_hit(kind, p, m, d)
            if not inside:                                                       # within budget only by reaching over a record's end, the stream's end or into the padding nibble
                self.case.places.append(Place("reaches_over_an_end", kind, q, k, strand, r, b, None, 0))
            hit = inside and where is not None
            self.case.places.append(Place(cell, kind, q, k, strand, r, b, bin(where).count("1") if hit else None, where if hit else 0))


def _subs(m, d, k):
    """k letters of a pattern (m, d): first, last, 15 and 16 (the two halves of the window), those on either side of the seam, then the rest"""
    order = [j for j in (0, m - 1, 15, 16, -d - 1, -d) if 0 <= j < m]
    order = list(dict.fromkeys(order + list(range(m))))
    return sorted(order[:k])


def planted_case(seed, odd):
    P = LP.Planted(seed, odd)
    c = Case("planted_odd" if odd else "planted_even", P.text, records_upper=P.records_upper)
    c.planted = P
    B = _Builder(P, c)
    win = lambda m, d: P.run[32 + d:32 + d + m]
    bits = lambda S: sum(1 << j for j in S)
    # a copy with exactly e and with e + 1 substitutions under budget e
    for e in BUDGETS:
        for m in LENGTHS:
            if (e and e >= m) or e + 1 > m:
                continue
            for d in _offsets(m, few=e > 1):
                S, S1 = _subs(m, d, e), _subs(m, d, e + 1)
                B.add("budget_%d_exact" % e, _flip(win(m, d), S), e, m, d, bits(S), True)
                B.add("budget_%d_one_more" % e, _flip(win(m, d), S1), e, m, d, bits(S1), False)
    # which letter is substituted: one substitution under budget 1 (a hit that names it) and under budget 0 (none)
    for m in (2, 16, 17, 32):
        for d in _offsets(m, few=True):
            roles = {"first": 0, "last": m - 1, "letter_15": 15, "letter_16": 16, "before_the_seam": -d - 1, "behind_the_seam": -d}
            for role, j in roles.items():
                if not 0 <= j < m or (role in ("letter_15", "letter_16") and m < 17):
                    continue
                B.add("substituted_" + role, _flip(win(m, d), [j]), 1, m, d, 1 << j, True)
                B.add("substituted_" + role + "_budget_0", _flip(win(m, d), [j]), 0, m, d, 1 << j, False)
    # a bracketed run at the start, at the end, across letters 15 / 16: a substitution just inside it (no hit), just outside it (a hit)
    for m in (15, 17, 32):
        for d in _offsets(m, few=True):
            spans = [("start", 0, 3, (2,), (3,)), ("end", m - 3, m, (m - 3,), (m - 4,))]
            if m >= 20:
                spans.append(("across_15_16", 14, 18, (15, 16), (13, 18)))      # the brackets lie in both halves of the window
            for name, a, b, inside, outside in spans:
                for j in inside:
                    B.add("bracket_%s_inside" % name, _bracket(_flip(win(m, d), [j]), a, b), 1, m, d, 1 << j, False)
                for j in outside:
                    B.add("bracket_%s_outside" % name, _bracket(_flip(win(m, d), [j]), a, b), 1, m, d, 1 << j, True)
    # the reverse strand: an asymmetric substitution fixes the orientation of `where` (window base i is pattern letter m - 1 - i)
    for m in (16, 17, 32):
        for d in _offsets(m, few=True):
            i = 1
            B.add("reverse_asymmetric", LP.revcomp(_flip(win(m, d), [i])), 1, m, d, 1 << (m - 1 - i), True, strand=1)
            # brackets on the reverse strand: the pattern's letters 0..2 face window bases m - 1 .. m - 3
            B.add("reverse_bracket_inside", _bracket(LP.revcomp(_flip(win(m, d), [m - 2])), 0, 3), 1, m, d, 1 << 1, False, strand=1)
            B.add("reverse_bracket_outside", _bracket(LP.revcomp(_flip(win(m, d), [m - 4])), 0, 3), 1, m, d, 1 << 3, True, strand=1)
    B.flush()
    n = len(P.records)
    # 16 patterns with different budgets in one call, on both strands; and the same restricted to records that start and end in the
    # middle of a tile, on an odd base (record 3 starts at base 1501, record 8 at 150003) and on an even one
    mixed = [(_flip(win(m, d), _subs(m, d, e)), e) for (m, d, e) in
             ((32, -32, 8), (32, -16, 3), (31, -1, 2), (31, 0, 1), (17, -17, 0), (17, -8, 3), (16, -16, 3), (16, 1, 2),
              (15, -15, 1), (15, -7, 3), (2, -2, 1), (2, 0, 0), (1, -1, 0), (32, 1, 1), (17, 0, 2), (31, -31, 3))]
    mixed[13] = (_bracket(mixed[13][0], 29, 32), 1)
    # (on the reverse strand the short ones are dense in the background, their reverse complements being made of A and C)
    for strands, first, count in ((1, 0, None), (3, 3, 5), (1, 8, n - 8), (3, 2, 1)):
        c.queries.append(Query([p for p, _ in mixed], [e for _, e in mixed], strands, first, count))
    c.mixed_queries = list(range(len(c.queries) - 4, len(c.queries)))
    if not odd:                                                                   # dense: the write pass crosses every tile (10^5 hits or more)
        c.queries.append(Query(["AC"], [1], 1))
        c.dense_query = len(c.queries) - 1
    return c


# the stored letters laid into the run of a stored_case, by index in RUN (31 is the last base in front of the seam, 32 the first behind it):
# N, R and a gap each within two bases on either side of the seam, over the two texts
STORED = {False: {30: "R", 31: "N", 32: "-", 33: "R"}, True: {30: "-", 31: "R", 32: "N", 33: "-"}}


def stored_case(seed, odd):
    """The planted text with substitutions on the STORED side of every laid copy: N, R and '-' at the four bases round the seam.  A
    cell (m, i, s, p) is the window of m = 17, 31 or 32 letters whose base i = 0, 15, 16 or m - 1 (the ends and the last base of the low
    and the first of the high half of the window) lies on the stored letter at run index s, under pattern letter p = A, R or N there
    and the run's own letters elsewhere.  What mismatches is told by the sets, base by base, from the laid run alone: the stored letter
    under p, and the other stored letters the window covers under the run's G and T.  Budget = that number is a hit, one less is none."""
    P = LP.Planted(seed, odd)
    laid = list(P.run)
    for idx, x in STORED[odd].items():
        laid[idx] = x
    recs = [list(r) for r in P.records]
    for kind, p in P.seams:
        for idx, x in STORED[odd].items():
            g = p - 32 + idx
            if g < P.total:                                                       # (the stream's end carries RUN[:32] only)
                r, b = P.to_record(g)
                recs[r][b] = x
    P.records = ["".join(r) for r in recs]
    P.records_upper = [r.upper() for r in P.records]
    P.text = LP.fasta(P.records)
    c = Case("stored_odd" if odd else "stored_even", P.text, records_upper=P.records_upper)
    c.planted = P
    B = _Builder(P, c)
    for m in (17, 31, 32):
        for base, i in (("0", 0), ("15", 15), ("16", 16), ("last", m - 1)):
            for s_idx, x in STORED[odd].items():
                d = s_idx - 32 - i
                if d < -32 or d + m > 34:
                    continue
                for letter in "ARN":
                    pat = list(P.run[32 + d:32 + d + m])
                    pat[i] = letter
                    miss = [not (laid[32 + d + j] != "-" and set(SETS[laid[32 + d + j]]) <= set(SETS[pat[j]])) for j in range(m)]
                    e, where = sum(miss), sum(1 << j for j, v in enumerate(miss) if v)
                    assert e <= MAX_MISMATCHES and miss[i] == (x == "-" or not set(SETS[x]) <= set(SETS[letter]))
                    cell = "stored_%s_under_%s_at_base_%s" % ("gap" if x == "-" else x, letter, base)
                    B.add(cell, "".join(pat), e, m, d, where, True)
                    if e:
                        B.add(cell, "".join(pat), e - 1, m, d, where, False)
    B.flush()
    return c


def small_case(seed):
    """A palindrome on both strands, stored N, R and - under A, R and N, records shorter than the pattern, empty records."""
    rng = np.random.default_rng(7600 + seed)
    bg = lambda n: LP._random(rng, n, "AC")
    stored = "NR-AGY"
    recs = ["", "CC" + bg(9) + "GAATTC" + bg(11) + "GAATTG" + bg(8) + "CC", "ACG", "", "TTTT".join("CC" + x + "CC" for x in stored), "A", "GAATT", "C" + bg(30), ""]
    c = Case("small", LP.fasta(recs, 50), records_upper=recs)
    at = recs[1].index("GAATTC"), recs[1].index("GAATTG")
    c.queries.append(Query(["GAATTC"], [1], 3))
    c.places += [Place("palindrome_both_strands", "none", 0, 0, s, 1, at[0], 0, 0) for s in (0, 1)]
    c.places += [Place("palindrome_both_strands", "none", 0, 0, 0, 1, at[1], 1, 1 << 5), Place("palindrome_both_strands", "none", 0, 0, 1, 1, at[1], 1, 1 << 0)]
    # record 6 "GAATT" and the C that starts record 7: within budget 0 only across the record's end
    c.places.append(Place("reaches_over_an_end", "none", 0, 0, 0, 6, 0, None, 0))
    pats = ["CCACC", "CCRCC", "CCNCC"]
    for q, budget in ((1, 1), (2, 0)):
        c.queries.append(Query(pats, [budget] * 3, 1))
        for k, x in enumerate(stored):
            for pi, p in enumerate(pats):
                miss = not (x != "-" and set(SETS[x]) <= set(SETS[p[2]]))
                ok = int(miss) <= budget
                c.places.append(Place("stored_%s_under_%s" % ("gap" if x == "-" else x, p[2]), "none", q, pi, 0, 4, 9 * k, int(miss) if ok else None, 4 if miss and ok else 0))
    # records shorter than the pattern: ACG under ACGA, budget 1, would be a hit with the first base of the next record that has one
    c.queries.append(Query(["ACGA", "AC", "[A]C"], [1, 1, 0], 3))
    c.places += [Place("record_shorter_than_the_pattern", "none", 3, 0, 0, 2, 0, None, 0), Place("record_shorter_than_the_pattern", "none", 3, 1, 0, 5, 0, None, 0),
                 Place("record_shorter_than_the_pattern", "none", 3, 1, 0, 2, 0, 0, 0)]
    return c


def rna_case(seed):
    base = LP.rna_case(seed)
    c = Case("rna", base.text, seq_type=1, records_upper=base.records_upper)
    c.queries += [Query(["ACGUACGU", "GU[GU]GU", "uuuuguuuu", "ACGTNNACGT"], [2, 1, 3, 1], 3), Query(["UUUUGAUUU"], [1], 2, 2, 1)]
    c.places.append(Place("rna", "none", 1, 0, 1, 2, 0, None, 0))                 # (the reverse complement of the stored bases is AAAACAAAA)
    c.places.append(Place("rna", "none", 0, 2, 0, 2, 0, 0, 0))
    return c


def fastq_case(seed):
    base = LP.fastq_case(seed)
    c = Case("fastq_reads", base.text, records_upper=base.records_upper)
    motif = "GATTACAGATTACA"
    c.queries += [Query([motif, "GATTACA[GATT]ACA", "TGTAATC", "[NGG]ACGT"], [2, 1, 1, 2], 3), Query([motif, "CCN"], [3, 0], 3, 27, 2), Query(["GATTACA"], [1], 1, 1990, 10)]
    last = len(base.records_upper) - 1
    c.places.append(Place("fastq", "none", 0, 0, 0, last, 150 - 14, 0, 0))         # the text ends in the motif
    return c


def r7_case(seed):
    base = LP.r7_case(seed)
    c = Case("surplus", base.text, records_upper=None, r7=True)
    c.queries += [Query(["GTTGTTGGTG", "TGGTG", "G[TG]", "N"], [2, 1, 0, 0], 3), Query(["GTTGTTGGTC"], [1], 1, 1, 1)]
    return c


def planned(seed=0):
    return [planted_case(seed, False), planted_case(seed, True), stored_case(seed, False), stored_case(seed, True), small_case(seed), rna_case(seed), fastq_case(seed), r7_case(seed)]


def coverage(cases):
    """{cell: {seam kind: places}} over the cases"""
    t = {}
    for c in cases:
        for p in c.places:
            t.setdefault(p.cell, {}).setdefault(p.kind, 0)
            t[p.cell][p.kind] += 1
    return t


def check_places(case, rows_of_query):
    """Holds a case's places against the rows of its queries (rows_of_query(q) -> int64 rows): every planted hit is there with exactly
    its mismatches and where, every place planted not to be a hit has no row."""
    for q in sorted({p.q for p in case.places}):
        rows = rows_of_query(q)
        have = {(int(r), int(b), int(k), int(s)): (int(e), int(w)) for r, b, k, s, e, w in rows}
        for p in case.places:
            if p.q != q:
                continue
            got = have.get((p.record, p.begin, p.pat, p.strand))
            want = None if p.mismatches is None else (p.mismatches, p.where)
            assert got == want, (case.name, p.cell, p.kind, case.queries[q].patterns[p.pat], case.queries[q].budgets[p.pat], p.record, p.begin, p.strand, got, want)
