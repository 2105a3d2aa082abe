"""The plan of the duplicate-collapsing tests (test_dedup_cpu.py holds it to its claims, test_gpu_dedup.py runs it): the model, the brute
force, the texts and the plants.  Pure Python and numpy; nothing here comes from the code under test.

The rule (include/naf_gpu.h): two records that take part are in one class iff their windows hold the same stored codes -- with both
strands also when one is the reverse complement of the other; first is the smallest record of the class, copies its size, strand 1 when
the window equals only the reverse complement of the first's.  `model` is a dict over the upper-cased window strings (U read as T), the
key min(s, rc(s)) with both strands; `brute` compares all pairs of equal length over str and shares no code with it.

The planted texts: the background is random reads over A, C, G, T of 40 to 150 bases, long enough that chance duplicates are negligible
(the model is a dict and is right whatever happens).  A plant is a pair of reads, an original in a calm place and a second read whose
first or last base lies at seam + off of a seam of the stream -- lane (64 bases), load (16 bytes: 32 bases), tile (4096), block (a zstd
block of 128 KiB of packed bytes: 262144 bases) -- or, through a bounds row, at off bases from its record's or the stream's end.  Its
relation says what the rows must show: `same` (one class, strand 0), `near` (one base changed, longer or shorter: never one class), `differ`
(never one class, whatever the difference) or `rc` (one class with both strands only, strand 1)."""
import bisect

import numpy as np

import locate_plan as LP

ROW_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("first", "<u8"), ("copies", "<u8"), ("flags", "<u4"), ("strand", "<u4")]
KEPT, SHORT, ERRORS, CLIPPED, DUPLICATE = 1, 2, 4, 8, 16
LANE, LOAD, TILE, BLOCK = 64, 32, 4096, 262144
SEAM_KINDS = ("lane", "load", "tile", "block", "record", "stream")
CELLS = ("same first", "same last", "near", "strand")
OFFSETS = (-2, -1, 0, 1, 2)
SMALL = (1, 2, 3, 31, 32, 33, 63, 64, 65, 150)
LONG = (511, 512, 513, 4095, 4096, 4097, 8193, 13001)         # 512: the longest window one lane compares
CODES = LP.CODES
# the complement of every stored letter, as IUPAC defines it (test_dedup_cpu holds it to the bit reversal of the 4-bit code)
COMP = str.maketrans("ACGTRYKMBVDHSWN-", "TGCAYRMKVBHDSWN-")
LEVEL_EDGES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000]     # FastQC's duplication levels: the smallest count of each


def rc(s):
    return s.translate(COMP)[::-1]


def canon(s):
    return s.upper().replace("U", "T")


def level_of(copies):
    assert copies >= 1
    return bisect.bisect_right(LEVEL_EDGES, copies) - 1


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def model(records, both=False, bounds=None, first=0, count=None):
    """(rows, total, levels) -- bounds: per record of the text (begin, end, flags) or None; total = (reads, considered, classes,
    duplicates, singletons, largest, bases, kept_bases); classes form among records [first, first + count) only"""
    last = len(records) if count is None else first + count
    rows = np.zeros(last - first, dtype=ROW_DTYPE)
    classes, members = {}, []
    for r in range(first, last):
        b, e, f = bounds[r] if bounds is not None else (0, len(records[r]), KEPT)
        if not f & KEPT:
            rows[r - first] = (r, b, e, r, 0, f, 0)
            continue
        w = canon(records[r][b:e])
        key = min(w, rc(w)) if both else w
        c = classes.setdefault(key, [r, 0, w])
        c[1] += 1
        members.append((r, b, e, f, c, 0 if w == c[2] else 1))
    t = [last - first, len(members), len(classes), len(members) - len(classes), 0, 0, 0, 0]
    levels = [0] * 16
    for r, b, e, f, c, strand in members:
        rows[r - first] = (r, b, e, c[0], c[1], (KEPT if c[0] == r else DUPLICATE) | (f & CLIPPED), strand)
        t[6] += e - b
        if c[0] == r:
            t[4] += c[1] == 1; t[5] = max(t[5], c[1]); t[7] += e - b
            levels[level_of(c[1])] += 1
    return rows, tuple(t), levels


def brute(records, both=False, bounds=None):
    """per record None (takes no part) or (first, copies, strand): every pair of windows of one length compared as str"""
    n = len(records)
    win = [None] * n
    for r in range(n):
        b, e, f = bounds[r] if bounds is not None else (0, len(records[r]), KEPT)
        if f & KEPT:
            win[r] = records[r][b:e].upper().replace("U", "T")
    by_len, first_of, strand = {}, [None] * n, [0] * n
    for r in range(n):
        if win[r] is None:
            continue
        firsts = by_len.setdefault(len(win[r]), [])
        for f in firsts:                                                                 # the firsts so far, ascending: the smallest equal one
            if win[f] == win[r]:
                first_of[r] = f
                break
            if both and win[f][::-1].translate(COMP) == win[r]:
                first_of[r], strand[r] = f, 1
                break
        else:
            first_of[r] = r
            firsts.append(r)
    copies = {}
    for f in first_of:
        if f is not None:
            copies[f] = copies.get(f, 0) + 1
    return [None if first_of[r] is None else (first_of[r], copies[first_of[r]], strand[r]) for r in range(n)]


def kept_segments(rows):
    return [(int(x["record"]), int(x["begin"]), int(x["end"])) for x in rows if int(x["flags"]) & KEPT]


def status_of(flags):
    f = int(flags)
    return "duplicate" if f & DUPLICATE else {KEPT: "first", SHORT: "short", ERRORS: "errors", SHORT | ERRORS: "short,errors"}[f & 7]


def table(rows, names, lengths):
    """The lines unnaf --dedup --dedup-table prints."""
    out = ["#seq\tlength\tbegin\tend\tfirst\tcopies\tstrand\tstatus\n"]
    for x in rows:
        r = int(x["record"])
        out.append("%s\t%d\t%d\t%d\t%s\t%d\t%s\t%s\n" % (names[r], lengths[r], x["begin"], x["end"], names[int(x["first"])], x["copies"], "-" if int(x["strand"]) else "+", status_of(x["flags"])))
    return "".join(out).encode("latin1")


def bounds_rows(bounds, kind, first=0):
    """the bounds as the rows naf_gpu_unnaf_trim (kind "trim") or naf_gpu_unnaf_clip ("clip") would have written them, as bytes"""
    if kind == "trim":
        t = np.zeros(len(bounds), dtype=[("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("ee", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])
        t["ee"] = 12345
    else:
        t = np.zeros(len(bounds), dtype=[("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("adapter", "<u4"), ("mismatches", "<u4"), ("overlap", "<u4"), ("flags", "<u4")])
        t["adapter"] = 2 ** 32 - 1; t["overlap"] = 7                                     # (an overlap where a trim row has its flags)
    t["record"] = np.arange(first, first + len(bounds)); t["begin"] = [b[0] for b in bounds]; t["end"] = [b[1] for b in bounds]; t["flags"] = [b[2] for b in bounds]
    return t.tobytes()


# ---- plants ------------------------------------------------------------------------------------------------------------------------
class Plant:
    """a: the original's record, b: the second read's; rel: same, near or rc; bset: the bounds set under which the claim holds (None:
    the whole records); mark: the stream position that was to lie at seam + off (None: not placed by a position)"""

    def __init__(self, cell, kind, off, a, b, rel, name, bset=None, mark=None):
        self.cell, self.kind, self.off, self.a, self.b, self.rel, self.name, self.bset, self.mark = cell, kind, off, a, b, rel, name, bset, mark


def holds(p, rows, both):
    """the plant's claim in the rows of its text (of the model or of the device)"""
    one = int(rows[p.a]["first"]) == int(rows[p.b]["first"])
    if p.rel == "alone":
        return int(rows[p.b]["copies"]) >= 1
    if p.rel == "same":
        return one and int(rows[p.b]["strand"]) == int(rows[p.a]["strand"]) and int(rows[p.b]["copies"]) >= 2
    if p.rel in ("near", "differ"):
        return not one
    return one == both and (not both or int(rows[p.b]["strand"]) != int(rows[p.a]["strand"]))


class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.pos, self.plants, self.bsets = [], 0, [], {}

    def bg(self, n, alphabet="ACGT"):
        return LP._random(self.rng, n, alphabet)

    def add(self, rd):
        self.reads.append(rd); self.pos += len(rd)
        return len(self.reads) - 1

    def fill_to(self, p):
        assert p >= self.pos, (p, self.pos)
        while self.pos < p:
            left = p - self.pos
            n = int(self.rng.integers(40, 151))
            self.add(self.bg(left if left < n + 40 else n))                              # (no short rest: the last read takes it)

    def at_parity(self, odd):
        if self.pos % 2 != odd:
            self.add(self.bg(41 if (self.pos + 41) % 2 == odd else 42))

    def put(self, rd, where, seam_pos):
        """rd with its first (where "first") or last base at stream position seam_pos"""
        self.fill_to(seam_pos if where == "first" else seam_pos - len(rd) + 1)
        return self.add(rd)

    def window(self, bset, r, b, e, f=KEPT):
        self.bsets.setdefault(bset, {})[r] = (b, e, f)


def change(s, i, to=None):
    """s with base i changed: an A to `to`, any other letter to the next of ACGT"""
    ch = to if to is not None else "ACGT"[("ACGT".index(s[i]) + 1) % 4]
    assert ch != s[i]
    return s[:i] + ch + s[i + 1:]


def second_of(orig, rel, rng):
    """the second read of a plant"""
    if rel == "same":
        return orig
    if rel == "rc":
        return rc(orig)
    return change(orig, int(rng.integers(0, len(orig))))


class Originals:
    """per length two originals, one on an even and one on an odd first base, so that a second read on either parity meets a first on either"""

    def __init__(self, B, lengths):
        self.B, self.rec = B, {}
        for n in lengths:
            for odd in (0, 1):
                s = B.bg(n)
                while n > 3 and s == rc(s):
                    s = B.bg(n)
                B.at_parity(odd)
                self.rec[(n, odd)] = B.add(s)
                B.fill_to(B.pos + 100)

    def get(self, n, k):
        r = self.rec[(n, k % 2)]
        return r, self.B.reads[r]


def seams_case(name, seed, small_kinds, tile_lengths, block_offs, near_at_seams):
    """small_kinds: lane / load seams that get the whole matrix of SMALL x first, last x OFFSETS; tile_lengths: the lengths laid over tile
    seams; block_offs: per block seam (last_off or None, first_off or None, the relation of the read that starts there)"""
    B = Builder(seed)
    B.add("")                                                                           # an empty record first
    O = Originals(B, sorted(set(SMALL) | set(tile_lengths)))
    k = 0
    rels = ("same", "same", "rc", "near")
    jobs = [(kind, n, where, off) for kind in small_kinds for n in SMALL for where in ("first", "last") for off in OFFSETS]
    tiles = [(n, where, off) for n in tile_lengths for where in ("first", "last") for off in OFFSETS]
    blocks = list(block_offs)
    T = -(-(B.pos + 200) // TILE)
    while jobs or tiles or blocks:
        seam = T * TILE
        if seam % BLOCK == 0 and blocks:
            last_off, first_off, first_rel = blocks.pop(0)
            for where, off in (("last", last_off), ("first", first_off)):
                if off is None:
                    continue
                for rel in (("same",) if where == "last" else (first_rel,)):
                    a, s = O.get(150, k)
                    b = B.put(second_of(s, rel, B.rng), where, seam + off)
                    B.plants.append(Plant("same " + where if rel == "same" else "strand" if rel == "rc" else "near", "block", off, a, b, rel, "150 %s" % where, None, seam + off))
                    k += 1
        elif tiles:
            n, where, off = tiles.pop(0)
            rel = rels[k % 4] if n > 3 else "same"
            a, s = O.get(n, k)
            b = B.put(second_of(s, rel, B.rng), where, seam + off)
            B.plants.append(Plant("same " + where if rel == "same" else "strand" if rel == "rc" else "near", "tile", off, a, b, rel, "%d %s" % (n, where), None, seam + off))
            k += 1
        while jobs and B.pos + 700 < (T + 1) * TILE:                                    # the inside of the tile: lane and load seams
            kind, n, where, off = jobs.pop(0)
            rel = (rels[k % 4] if near_at_seams else ("same", "rc")[k % 2]) if n > 3 else "same"
            a, s = O.get(n, k)
            lane = -(-(B.pos + 260) // LANE) * LANE + (LOAD if kind == "load" else 0)
            b = B.put(second_of(s, rel, B.rng), where, lane + off)
            B.plants.append(Plant("same " + where if rel == "same" else "strand" if rel == "rc" else "near", kind, off, a, b, rel, "%d %s" % (n, where), None, lane + off))
            k += 1
        T = max(T + 1, -(-(B.pos + 200) // TILE))
        if not jobs and not tiles and blocks:                                            # nothing left but block seams: on to the next one
            T = max(T, -(-(B.pos + 400) // BLOCK) * (BLOCK // TILE))
    # windows at 0 to 2 bases from their record's ends: the bounds set "win"
    for n in (31, 150):
        for x in (0, 1, 2):
            for y in (0, 1, 2):
                for rel in ("same", "rc", "near"):
                    a, s = O.get(n, k)
                    b = B.add(B.bg(x) + second_of(s, rel, B.rng) + B.bg(y))
                    B.window("win", b, x, x + n)
                    cell = ("same first" if x else "same last") if rel == "same" else "strand" if rel == "rc" else "near"
                    B.plants.append(Plant(cell, "record", x if x else -y, a, b, rel, "%d in a window" % n, "win"))
                    k += 1
    B.fill_to(B.pos + 300)
    B.add(""); B.add("")                                                                # an empty pair
    B.fill_to(B.pos + 100)
    return Case(name, B)


def near_case(seed):
    """one original of 150 bases with an A at every place that is changed; second reads with ONE base changed -- the first, the last,
    either side of every dword and lane boundary of the window -- to another base, N, R or '-', one base longer and one base shorter,
    each with its first base at -2 .. +2 of a lane seam"""
    B = Builder(seed)
    n = 150
    places = sorted({0, n - 1} | {p for q in range(8, n, 8) for p in (q - 1, q)})
    s = list(B.bg(n))
    for p in places:
        s[p] = "A"
    s = "".join(s)
    B.add(B.bg(77))
    a = B.add(s)
    k = 0
    for p in places:
        for to in ("C", "N", "R", "-"):
            lane = -(-(B.pos + 200) // LANE) * LANE
            off = OFFSETS[k % 5]
            b = B.put(change(s, p, to), "first", lane + off)
            B.plants.append(Plant("near", "lane", off, a, b, "near", "base %d to %s" % (p, to), None, lane + off))
            k += 1
    for name, t in (("one longer", s + "A"), ("one longer in front", "A" + s), ("one shorter", s[:-1]), ("one shorter in front", s[1:])):
        for off in OFFSETS:
            lane = -(-(B.pos + 200) // LANE) * LANE + LOAD
            b = B.put(t, "first", lane + off)
            B.plants.append(Plant("near", "load", off, a, b, "near", name, None, lane + off))
    b = B.add(s)
    B.plants.append(Plant("same first", "lane", 0, a, b, "same", "the original again"))
    return Case("near", B)


def long_case(seed):
    """windows of 511 to 13001 bases (a wavefront compares those above 512) and of 300000, which crosses block seams"""
    B = Builder(seed)
    B.add(B.bg(151))
    k = 0
    for n in LONG:
        s = B.bg(n)
        B.at_parity(k % 2)
        a = B.add(s)
        for rel, odd in (("same", 1 - k % 2), ("rc", k % 2), ("near", 1 - k % 2)):
            B.fill_to(B.pos + 77)
            B.at_parity(odd)
            t = second_of(s, rel, B.rng) if rel != "near" else change(s, (n - 1, 0, n // 2, n // 16 * 8, n // 16 * 8 - 1, n - 2, 1, 64)[k % 8])
            b = B.add(t)
            B.plants.append(Plant("same first" if rel == "same" else "strand" if rel == "rc" else "near", "tile", 0, a, b, rel, "%d" % n))
        k += 1
    s = B.bg(300000)
    B.at_parity(0)
    a = B.add(s)
    B.add(B.bg(41))
    b = B.add(s)
    B.plants.append(Plant("same first", "block", 0, a, b, "same", "300000"))
    b = B.add(rc(s))
    B.plants.append(Plant("strand", "block", 0, a, b, "rc", "300000"))
    return Case("long", B, lower=False)


def strand_case(seed):
    """palindromes, a window equal both ways, all sixteen codes"""
    B = Builder(seed)
    B.add(B.bg(99))
    half = B.bg(40)
    pal = half + rc(half)                                                               # its own reverse complement
    assert pal == rc(pal)
    a = B.add(pal); B.add(B.bg(50)); b = B.add(pal)
    B.plants.append(Plant("same first", "lane", 0, a, b, "same", "a palindrome twice: strand 0 both ways"))
    for small in ("AT", "ACGT", "N", "SWN-NWS", "-"):
        assert small == rc(small)
        a = B.add(small); B.add(B.bg(60)); b = B.add(small)
        B.plants.append(Plant("same first", "lane", 0, a, b, "same", "palindrome " + small))
    for k in range(12):
        s = LP._random(B.rng, int(B.rng.integers(5, 200)), CODES)
        if k == 0:
            s = CODES + s
        B.at_parity(k % 2)
        a = B.add(s)
        B.add(B.bg(43 + k % 2))
        b = B.add(rc(s))
        B.plants.append(Plant("strand", "lane", 0, a, b, "rc", "all sixteen codes"))
        c = B.add(s.lower())
        B.plants.append(Plant("same first", "lane", 0, a, c, "same", "all sixteen codes, lower case"))
        i = int(B.rng.integers(0, len(s)))
        d = B.add(s[:i] + CODES[(CODES.index(s[i]) + 1 + k) % 16] + s[i + 1:])
        B.plants.append(Plant("near", "lane", 0, a, d, "near", "all sixteen codes, one other"))
    # N equals only N, a gap only a gap
    s = B.bg(60)
    a = B.add(s[:30] + "N" + s[31:])
    for ch in "ACGT-R":
        b = B.add(s[:30] + ch + s[31:])
        B.plants.append(Plant("near", "lane", 0, a, b, "near", "N against " + ch))
    return Case("strand", B, lower=False)


def classes_case(seed):
    """classes of 1, 2, 9, 10, 49, 50, 100, 500 and 1000 reads, their members dealt out over the text; empty records first, last and side
    by side; reads that differ in case only"""
    B = Builder(seed)
    sizes = (1, 2, 9, 10, 49, 50, 100, 500, 1000)
    seqs = [B.bg(int(B.rng.integers(40, 90))) for _ in sizes]
    deck = [k for k, n in enumerate(sizes) for _ in range(n)]
    B.rng.shuffle(deck)
    B.add("")
    seen = {}
    for j, k in enumerate(deck):
        if j in (300, 900):
            B.add("")
        if j == 300:
            B.add("")                                                                   # a pair side by side
        s = seqs[k]
        r = B.add(s.lower() if j % 7 == 3 else s[:11] + s[11:].lower() if j % 7 == 5 else s)
        if k in seen and j % 50 == 0:
            B.plants.append(Plant("same first", "lane", 0, seen[k], r, "same", "class of %d" % sizes[k]))
        seen.setdefault(k, r)
    B.add("")
    c = Case("classes", B, lower=False)
    c.sizes = sizes
    return c


def ones_case(seed):
    """5000 reads of one base"""
    B = Builder(seed)
    for ch in B.rng.integers(0, 4, 5000):
        B.add("ACGT"[int(ch)])
    return Case("ones", B, lower=False)


def rna_case(seed):
    B = Builder(seed)
    for k in range(40):
        s = B.bg(int(B.rng.integers(1, 200)), "ACGU")
        a = B.add(s)
        B.add(B.bg(int(B.rng.integers(1, 90)), "ACGU"))
        if k % 2:
            b = B.add(s)
            B.plants.append(Plant("same first", "lane", 0, a, b, "same", "RNA"))
        else:
            b = B.add(rc(s.replace("U", "T")).replace("T", "U"))
            B.plants.append(Plant("strand", "lane", 0, a, b, "rc", "RNA"))
    return Case("rna", B, seq_type=1, lower=False)


def fastq_case(seed):
    """900 reads of 150 bases with qualities falling towards the end; every third read copies an earlier one -- with qualities of its own
    --, every ninth as its reverse complement; a G/T adapter behind a short insert in every fifth: what unnaf_trim and unnaf_clip give of it
    are the bounds of the dedup call"""
    B = Builder(seed)
    rng = B.rng
    quals = []
    adapter = LP._random(rng, 32, "GT")
    for k in range(900):
        n = 150
        if k % 3 == 2 and k > 10:
            src = B.reads[int(rng.integers(0, k))]
            rd = rc(src) if k % 9 == 8 else src
        else:
            rd = B.bg(n)
            if k % 5 == 0:
                rd = (rd[:int(rng.integers(20, 140))] + adapter + B.bg(n))[:n]
        B.add(rd)
        drop = int(rng.integers(60, 151))
        if k % 2 == 0 or (k % 3 == 2 and k > 10):                                       # these keep their quality to the end: trimmed, a copy still equals such a source
            drop = n
        q = np.where(np.arange(n) < drop, rng.integers(30, 41, n), rng.integers(2, 25, n)) + 33
        quals.append(bytes(q.astype(np.uint8)))
    c = Case("fastq", B, fmt="fastq", lower=False)
    c.quals, c.adapter = quals, adapter
    c.text = b"".join(b"@%s w\n%s\n+\n%s\n" % (i.encode(), r.encode(), q) for i, r, q in zip(c.ids, c.records, quals))
    return c


def bounds_case(seed):
    """windows that make two different reads equal and two equal reads different; rows without KEPT in the middle of a class, its would-be
    first among them; begin == end"""
    B = Builder(seed)
    B.add(B.bg(120))
    core = B.bg(70)
    a = B.add(B.bg(13) + core + B.bg(20)); B.window("cut", a, 13, 83)
    b = B.add(B.bg(6) + core + B.bg(3)); B.window("cut", b, 6, 76, KEPT | CLIPPED)
    B.plants.append(Plant("same first", "record", 13, a, b, "same", "two different reads, equal windows", "cut"))
    c = B.add(B.bg(2) + rc(core)); B.window("cut", c, 2, 72)
    B.plants.append(Plant("strand", "record", 2, a, c, "rc", "a window's reverse complement", "cut"))
    s = B.bg(100)
    a = B.add(s); b = B.add(s); B.window("cut", a, 0, 99); B.window("cut", b, 1, 100)
    B.plants.append(Plant("near", "record", 1, a, b, "differ", "two equal reads, different windows", "cut"))
    s = B.bg(88)
    m = [B.add(s) for _ in range(5)]                                                    # a class of five: its would-be first and its third take no part
    B.window("cut", m[0], 0, 88, SHORT); B.window("cut", m[2], 3, 80, ERRORS | CLIPPED)
    B.plants.append(Plant("same first", "record", 0, m[1], m[4], "same", "a class whose would-be first has no KEPT", "cut"))
    B.dropped = (m[0], m[2])
    e1 = B.add(B.bg(50)); e2 = B.add(B.bg(60)); e3 = B.add("")                          # begin == end: empty windows are equal to each other, and to an empty record
    B.window("cut", e1, 7, 7); B.window("cut", e2, 60, 60)
    B.plants.append(Plant("same last", "record", 0, e1, e2, "same", "begin == end", "cut"))
    B.plants.append(Plant("same last", "record", 0, e1, e3, "same", "begin == end and an empty record", "cut"))
    B.add(B.bg(90))
    c = Case("bounds", B, lower=False)
    c.dropped = B.dropped
    return c


def tail_case(name, seed, rel, y):
    """a short text whose last read is a plant's second read, its window's last base y bases in front of the stream's end"""
    B = Builder(seed)
    s = B.bg(150)
    a = B.add(s)
    B.fill_to(700 + y)
    b = B.add(second_of(s, rel, B.rng) + B.bg(y))
    B.window("win", b, 0, 150)
    cell = "same last" if rel == "same" else "strand" if rel == "rc" else "near"
    B.plants.append(Plant(cell, "stream", -y, a, b, rel, "the stream's last read", "win" if y else None))
    if rel == "same" and y == 0:                                                        # and one whose FIRST base is the stream's last
        c = B.add("G")
        B.window("win", c, 0, 1)
        B.plants.append(Plant("same first", "stream", 0, c, c, "alone", "one base at the stream's end"))
    return Case(name, B, lower=False)


# ---- texts -------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, B, fmt="fasta", seq_type=0, lower=True):
        self.name, self.plants, self.bsets, self.seq_type, self.fmt = name, B.plants, B.bsets, seq_type, fmt
        recs = B.reads
        if lower:                                                                       # the soft mask plays no part
            rng = np.random.default_rng(len(recs))
            for k in rng.integers(0, len(recs), 40):
                recs[k] = recs[k].lower() if int(k) % 2 else recs[k][:len(recs[k]) // 2] + recs[k][len(recs[k]) // 2:].lower()
        self.records = recs
        self.ids = ["r%d" % k for k in range(len(recs))]
        self.text = LP.fasta(recs, 80, self.ids)
        self.starts = np.concatenate([[0], np.cumsum([len(r) for r in recs])])

    def bounds(self, bset):
        """the bounds rows of a set: the plants' own, the whole record (kept) for every other read"""
        own = self.bsets.get(bset, {})
        return [own.get(r, (0, len(rec), KEPT)) for r, rec in enumerate(self.records)]


_cache = {}


def planned(seed=0):
    """the cases"""
    if seed not in _cache:
        _cache[seed] = [
            seams_case("seams0", 7100 + seed, ("lane", "load"), (150,), [(-2, -1, "same"), (-1, 0, "rc"), (0, 1, "near")], False),
            seams_case("seams1", 7110 + seed, (), (31, 32, 33, 63, 64, 65, 150), [(1, 2, "near"), (2, None, None), (None, -2, "same")], True),
            near_case(7120 + seed), long_case(7130 + seed), strand_case(7140 + seed), classes_case(7150 + seed), ones_case(7160 + seed),
            rna_case(7170 + seed), fastq_case(7180 + seed), bounds_case(7190 + seed),
            tail_case("tail0", 7200 + seed, "same", 0), tail_case("tail1", 7210 + seed, "near", 1), tail_case("tail2", 7220 + seed, "rc", 2)]
    return _cache[seed]


SMALL_CASES = ("near", "strand", "rna", "bounds", "tail0", "tail1", "tail2")            # few enough classes for every value of the lever


def coverage(cases):
    """{cell: {seam kind: plants}}"""
    out = {c: {k: 0 for k in SEAM_KINDS} for c in CELLS}
    for c in cases:
        for p in c.plants:
            out[p.cell][p.kind] += 1
    return out


def random_reads(seed, n=400):
    """reads over all sixteen codes, short, with copies, reverse complements and near copies among them"""
    rng = np.random.default_rng(7290 + seed)
    out = []
    for k in range(n):
        if k > 20 and k % 3 == 0:
            s = out[int(rng.integers(0, k))]
            s = rc(s.upper().replace("U", "T")) if k % 2 else s.lower()
            if k % 5 == 0 and s:
                i = int(rng.integers(0, len(s))); s = s[:i] + CODES[int(rng.integers(0, 16))] + s[i + 1:]
            out.append(s)
        else:
            out.append(LP._random(rng, int(rng.integers(0, 12 if k % 4 == 0 else 90)), CODES if k % 2 else "ACGTN"))
    return out


# ---- who takes part ------------------------------------------------------------------------------------------------------------------
PART_N = (1, 63, 64, 65, 255, 256, 257, 513)                                            # the wave and workgroup seams of a launch of 256 lanes, a lane per record


def part_sets(N):
    """(name, per record: it takes part) -- exactly the first n records, exactly the last n, every n-th, for every n of PART_N"""
    for n in PART_N:
        yield "the first %d" % n, [k < n for k in range(N)]
        yield "the last %d" % n, [k >= N - n for k in range(N)]
        yield "every %d-th" % n, [k % n == 0 for k in range(N)]


def part_bounds(lens, takes):
    """trim-kind bounds of reads of at least 3 bases: windows that differ from read to read; NAF_GPU_TRIM_KEPT where the read takes part,
    one of the three other states of a trim row where it does not"""
    return [(k % 3, n - k % 2, KEPT if on else (SHORT, ERRORS, SHORT | ERRORS)[k % 3]) for k, (n, on) in enumerate(zip(lens, takes))]
