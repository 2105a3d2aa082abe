"""The plan of the k-mer screening tests (test_screen_cpu.py holds it to its claims, test_gpu_screen.py runs it): the model, the brute
force, the references, the texts and the plants.  Pure Python and numpy; nothing here comes from the code under test.

The rule (include/naf_gpu.h): the set holds the keys of all valid k-mers of all records of the reference -- K bases of ONE record, each
stored as exactly A, C, G or T/U; the key two bits a base, the first base the most significant; the smaller of a k-mer's key and its
reverse complement's unless forward_only --, hits_r counts the starts of read r's window whose k-mer is valid and whose key is in the set,
a read is matched iff hits_r >= min_hits, and a matched read is dropped unless keep_matched, which drops the others.  `model` computes
the keys of a whole stream at once in numpy; `brute` is a triple loop over str (reads, starts, letters) and shares no code with it.

The planted texts.  A reference text is seeded ACGT with at most RUN_CAP letters in a row from {A, C} and at most RUN_CAP from {G, T}
(`check_reference` asserts it), the background of the reads is seeded over {A, C} alone: for K > RUN_CAP no k-mer of the background is
in the set on either strand.  (At K = 1 and 2 no such reference exists -- every base is a 1-mer of one of the two classes -- so there
the claims are lower bounds and the model alone decides.)  A plant is a copy of K + j bases of the reference's long record; the
background letter on either side of it differs from the reference's letter there, so that from K = EXACT_K on the hits of every read are
known by construction: `expect` holds them, and every read that holds no plant expects none.

Placement: per K one text in which a plant's first base lies at seam + off for every off in -(K + 1) .. +2, every j in JS and the seams
lane (64 bases), load (16 bytes: 32 bases), tile (4096) and record (the plant is laid over the boundary of two reads: each read counts
the k-mers that lie wholly in it).  A block seam (a zstd block of 128 KiB of packed bytes: 262144 bases) takes one plant, so a text of
1.3 M bases has five: the K = 1 text has every offset there, the other texts two seams whose offsets rotate with K and the seed.  The
stream's end takes one text per offset and j (tiny ones, `ends`)."""
import numpy as np

import locate_plan as LP

ROW_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("hits", "<u8"), ("flags", "<u4"), ("reserved", "<u4")]
KEPT, SHORT, ERRORS, CLIPPED, DUPLICATE, MATCHED = 1, 2, 4, 8, 16, 32
LANE, LOAD, TILE, BLOCK = 64, 32, 4096, 262144
KS = (1, 2, 15, 16, 17, 27, 31)
JS = (0, 1, 5)
RUN_CAP = 6
EXACT_K = 15
SEAM_KINDS = ("lane", "load", "tile", "record", "block", "stream")
CELLS = ("forward", "strand", "substitution", "near", "spanning", "palindrome", "length", "window", "dropped")
COMP = str.maketrans("ACGT", "TGCA")
VAL = {"A": 0, "C": 1, "G": 2, "T": 3}


def canon(s):
    return s.upper().replace("U", "T")


def rc(s):
    return s.translate(COMP)[::-1]


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
_LUT = np.full(256, 4, dtype=np.uint8)
for _ch, _v in zip("ACGTU", (0, 1, 2, 3, 3)):
    _LUT[ord(_ch)] = _LUT[ord(_ch.lower())] = _v


class Stream:
    """records laid end to end, as the archive stores them"""

    def __init__(self, records):
        self.records = records
        self.n = len(records)
        self.lens = np.array([len(r) for r in records], dtype=np.int64)
        self.base = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.codes = _LUT[np.frombuffer("".join(records).encode("latin1"), dtype=np.uint8)]
        self.rec_of = np.repeat(np.arange(self.n, dtype=np.int64), self.lens)
        self._keys = {}

    def keys(self, K):
        """(forward key, reverse complement's key, K single nucleotides) of every start of the stream that has K bases behind it"""
        if K not in self._keys:
            c = self.codes
            m = max(len(c) - K + 1, 0)
            bad = np.concatenate([[0], np.cumsum(c == 4)])
            valid = (bad[K:K + m] - bad[:m]) == 0
            c3 = (c & 3).astype(np.uint64)
            f, r = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
            for j in range(K):
                f = (f << np.uint64(2)) | c3[j:j + m]
                r |= (np.uint64(3) - c3[j:j + m]) << np.uint64(2 * j)
            self._keys[K] = (f, r, valid)
        return self._keys[K]

    def starts(self, K, begin=None, end=None, part=None):
        """the starts whose k-mer is valid and lies in the window of its record, of a record that takes part"""
        valid = self.keys(K)[2]
        m = len(valid)
        rec = self.rec_of[:m]
        b = self.base[:-1] + (0 if begin is None else begin)
        e = self.base[:-1] + (self.lens if end is None else end)
        p = np.arange(m, dtype=np.int64)
        ok = valid & (p >= b[rec]) & (p + K <= e[rec])
        if part is not None:
            ok &= part[rec]
        return ok

    def chosen(self, K, forward_only):
        f, r, _ = self.keys(K)
        return f if forward_only else np.minimum(f, r)


def ref_set(ref, K, forward_only=False):
    """(the distinct keys ascending, the reference's valid positions)"""
    ok = ref.starts(K)
    return np.unique(ref.chosen(K, forward_only)[ok]), int(ok.sum())


def model(reads, ref, K, min_hits=1, keep_matched=False, forward_only=False, bounds=None, first=0, count=None):
    """(rows, total) -- reads, ref: Streams; bounds: per read of the text (begin, end, flags) or None; total = (reads, considered, matched,
    kept, bases, kept_bases, kmers, hit_kmers, ref_records, ref_bases, ref_positions, ref_kmers)"""
    N = reads.n
    last = N if count is None else first + count
    if bounds is not None:
        begin, end, flags = (np.array([b[k] for b in bounds], dtype=np.int64) for k in range(3))
    else:
        begin, end, flags = np.zeros(N, dtype=np.int64), reads.lens.copy(), np.full(N, KEPT, dtype=np.int64)
    sel = np.zeros(N, dtype=bool)
    sel[first:last] = True
    part = ((flags & KEPT) != 0) & sel
    S, ref_pos = ref_set(ref, K, forward_only)
    ok = reads.starts(K, begin, end, part)
    hit = ok & np.isin(reads.chosen(K, forward_only), S)
    hits = np.bincount(reads.rec_of[:len(ok)][hit], minlength=N)[:N] if N else np.zeros(0, dtype=np.int64)
    matched = part & (hits >= min_hits)
    kept = part & (matched == bool(keep_matched))
    rows = np.zeros(last - first, dtype=ROW_DTYPE)
    s = slice(first, last)
    rows["record"], rows["begin"], rows["end"], rows["hits"] = np.arange(first, last), begin[s], end[s], hits[s]
    rows["flags"] = np.where(part, matched * MATCHED | kept * KEPT | (flags & CLIPPED), flags)[s]
    total = (last - first, int(part.sum()), int(matched.sum()), int(kept.sum()), int((end - begin)[part].sum()), int((end - begin)[kept].sum()), int(ok.sum()), int(hit.sum()),
             ref.n, int(ref.lens.sum()), ref_pos, len(S))
    return rows, total


def _key_of(s, forward_only):
    f = 0
    for ch in s:
        if ch not in VAL:
            return None
        f = f * 4 + VAL[ch]
    if forward_only:
        return f
    r = 0
    for ch in reversed(s):
        r = r * 4 + 3 - VAL[ch]
    return min(f, r)


_brute_sets = {}


def _brute_set(ref_records, K, forward_only):
    """(the set, the valid positions) of a reference, letter by letter; kept per list of records (many texts share one reference)"""
    key = (id(ref_records), K, forward_only)
    if key not in _brute_sets or _brute_sets[key][0] is not ref_records:
        S, ref_pos = set(), 0
        for r in ref_records:
            r = canon(r)
            for i in range(len(r) - K + 1):
                k = _key_of(r[i:i + K], forward_only)
                if k is not None:
                    S.add(k); ref_pos += 1
        _brute_sets[key] = (ref_records, S, ref_pos)
    return _brute_sets[key][1:]


def brute(records, ref_records, K, forward_only=False, bounds=None):
    """(hits per read or None where it takes no part, kmers, ref_positions, ref_kmers): a loop over the reads, their starts and the letters"""
    S, ref_pos = _brute_set(ref_records, K, forward_only)
    hits, kmers = [], 0
    for n, r in enumerate(records):
        b, e, f = bounds[n] if bounds is not None else (0, len(r), KEPT)
        if not f & KEPT:
            hits.append(None)
            continue
        w = canon(r)[b:e]
        h = 0
        for i in range(len(w) - K + 1):
            k = _key_of(w[i:i + K], forward_only)
            if k is not None:
                kmers += 1
                h += k in S
        hits.append(h)
    return hits, kmers, ref_pos, len(S)


def brute_slices(records, ref_records, K, forward_only=False, bounds=None):
    """what `brute` gives, for the long texts: the letters of a k-mer are compared as one slice, the keys are the slices themselves (the
    order of the keys is the order of the strings) and the set holds both strands"""
    S, distinct, ref_pos = set(), set(), 0
    for r in ref_records:
        r = canon(r)
        for i in range(len(r) - K + 1):
            s = r[i:i + K]
            if s.strip("ACGT"):
                continue
            ref_pos += 1
            S.add(s)
            if not forward_only:
                S.add(rc(s))
            distinct.add(s if forward_only else min(s, rc(s)))
    hits, kmers = [], 0
    for n, r in enumerate(records):
        b, e, f = bounds[n] if bounds is not None else (0, len(r), KEPT)
        if not f & KEPT:
            hits.append(None)
            continue
        w = canon(r)[b:e]
        h = 0
        for i in range(len(w) - K + 1):
            s = w[i:i + K]
            if not s.strip("ACGT"):
                kmers += 1
                h += s in S
        hits.append(h)
    return hits, kmers, ref_pos, len(distinct)


def kept_segments(rows):
    return [(int(x["record"]), int(x["begin"]), int(x["end"])) for x in rows if int(x["flags"]) & KEPT]


def status_of(flags, duplicate=False):
    """what was carried first (the read never took part), then what the last step found"""
    f = int(flags)
    if f & (SHORT | ERRORS):
        return {SHORT: "short", ERRORS: "errors", SHORT | ERRORS: "short,errors"}[f & (SHORT | ERRORS)]
    return "duplicate" if duplicate else "matched" if f & MATCHED else "clean"


def table(rows, names, lengths, dedup_rows=None):
    """The lines unnaf --screen --screen-table prints; dedup_rows: what --dedup made of the screen rows as its bounds."""
    out = ["#seq\tlength\tbegin\tend\thits\tstatus\n"]
    for k, x in enumerate(rows):
        r = int(x["record"])
        dup = dedup_rows is not None and bool(int(dedup_rows[k]["flags"]) & DUPLICATE)
        out.append("%s\t%d\t%d\t%d\t%d\t%s\n" % (names[r], lengths[r], x["begin"], x["end"], x["hits"], status_of(x["flags"], dup)))
    return "".join(out).encode("latin1")


def bounds_rows(bounds, kind, first=0):
    """the bounds as the rows naf_gpu_unnaf_trim ("trim"), naf_gpu_unnaf_clip ("clip") or naf_gpu_unnaf_dedup ("dedup") would have written them, as bytes"""
    if kind == "trim":
        t = np.zeros(len(bounds), dtype=[("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("ee", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])
        t["ee"] = 12345
    elif kind == "clip":
        t = np.zeros(len(bounds), dtype=[("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("adapter", "<u4"), ("mismatches", "<u4"), ("overlap", "<u4"), ("flags", "<u4")])
        t["adapter"] = 2 ** 32 - 1; t["overlap"] = 7                                     # (an overlap where a trim row has its flags)
    else:
        t = np.zeros(len(bounds), dtype=[("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("first", "<u8"), ("copies", "<u8"), ("flags", "<u4"), ("strand", "<u4")])
        t["first"] = 7; t["copies"] = 3; t["strand"] = 1                                 # (a 7 where a trim row has its flags, a 3 where a clip row has them)
    t["record"] = np.arange(first, first + len(bounds)); t["begin"] = [b[0] for b in bounds]; t["end"] = [b[1] for b in bounds]; t["flags"] = [b[2] for b in bounds]
    return t.tobytes()


# ---- references ----------------------------------------------------------------------------------------------------------------------
def capped(rng, n, cap=RUN_CAP):
    """n seeded letters of ACGT with at most `cap` in a row from {A, C} and from {G, T}"""
    s = list(LP._random(rng, n, "ACGT"))
    cls, run = None, 0
    for i, ch in enumerate(s):
        k = ch in "AC"
        run = run + 1 if k == cls else 1
        cls = k
        if run > cap:
            s[i] = ("GT" if k else "AC")[int(rng.integers(0, 2))]
            cls, run = not k, 1
    return "".join(s)


def longest_class_run(records):
    best = 0
    for r in records:
        cls, run = None, 0
        for ch in canon(r):
            k = True if ch in "AC" else False if ch in "GT" else None
            run = run + 1 if (k is not None and k == cls) else (1 if k is not None else 0)
            cls = k
            best = max(best, run)
    return best


def check_reference(records, K):
    """no K consecutive letters from {A, C} and none from {G, T}"""
    assert longest_class_run(records) < K, (longest_class_run(records), K)


def fastq_text(ids, records, quals=None):
    return b"".join(b"@%s w\n%s\n+\n%s\n" % (i.encode(), r.encode(), (quals[k] if quals else b"I" * len(r))) for k, (i, r) in enumerate(zip(ids, records)))


class Ref:
    def __init__(self, name, records, fmt="fasta", seq_type=0):
        self.name, self.records, self.fmt, self.seq_type = name, records, fmt, seq_type
        self.ids = ["ref%d" % k for k in range(len(records))]
        self.text = fastq_text(self.ids, records) if fmt == "fastq" else LP.fasta(records, 70, self.ids) if records else b""
        self.stream = Stream(records)


BIG, NEXT = 1, 2                                                                         # the long record of a main reference and the record behind it


def main_ref(seed, name="main", fmt="fasta", seq_type=0, big=13001):
    """an empty record; the long record the plants are copies of (longer than three tiles); a record twice, so that every k-mer of it is
    there twice; records of K - 1, K and K + 1 bases for every K; N inside; lower case; a 16-base and a 2-base palindrome"""
    rng = np.random.default_rng(9100 + seed)
    recs = ["", capped(rng, big)]
    twice = capped(rng, 200)
    recs += [twice, twice]
    recs += [capped(rng, n) for n in sorted({n for K in KS for n in (K - 1, K, K + 1)})]
    s = capped(rng, 300)
    recs.append(s[:150] + "N" + s[151:220] + "nn" + s[222:])
    s = capped(rng, 200)
    recs.append(s[:90] + s[90:].lower())
    half = capped(rng, 8)
    recs += [half + rc(half), "AT"]
    if seq_type == 1:
        recs = [r.replace("T", "U").replace("t", "u") for r in recs]
    if fmt == "fastq":
        recs = [r or "ACGTA" for r in recs]
    R = Ref(name, recs, fmt, seq_type)
    R.palindrome = canon(half + rc(half))
    return R


def none_ref(seed):
    """no valid k-mer for K >= 15: N every ten bases, and records shorter than that"""
    rng = np.random.default_rng(9200 + seed)
    s = capped(rng, 400)
    return Ref("none", ["".join("N" if i % 10 == 9 else ch for i, ch in enumerate(s)), capped(rng, 14), "", "NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"])


# ---- plants ------------------------------------------------------------------------------------------------------------------------
class Plant:
    """rec: the read that holds the plant's first base; mark: the stream position that was to lie at seam + off (None: not placed by a position)"""

    def __init__(self, cell, kind, off, K, j, rec, mark=None, name=""):
        self.cell, self.kind, self.off, self.K, self.j, self.rec, self.mark, self.name = cell, kind, off, K, j, rec, mark, name


def flank(rng, avoid):
    """a background letter that is not `avoid`"""
    return "C" if avoid == "A" else "A" if avoid == "C" else "AC"[int(rng.integers(0, 2))]


class Builder:
    def __init__(self, seed, K, ref):
        self.rng = np.random.default_rng(seed)
        self.K, self.ref, self.big = K, ref, canon(ref.records[BIG])
        self.reads, self.pos, self.plants = [], 0, []
        self.expect, self.expect_fwd = {}, {}                                            # read -> hits known by construction (canonical, forward only)
        self.bsets, self.expect_win = {}, {}

    def bg(self, n):
        return LP._random(self.rng, n, "AC")

    def add(self, rd, hits=0, hits_fwd=None):
        self.reads.append(rd); self.pos += len(rd)
        r = len(self.reads) - 1
        if hits or hits_fwd:
            self.expect[r] = hits
            self.expect_fwd[r] = hits if hits_fwd is None else hits_fwd
        return r

    def fill_to(self, p):
        assert p >= self.pos, (p, self.pos)
        while self.pos < p:
            left = p - self.pos
            n = int(self.rng.integers(40, 151))
            self.add(self.bg(left if left < n + 40 else n))

    def source(self, L):
        """a place in the long record with a base on either side"""
        return int(self.rng.integers(1, len(self.big) - L - 1))

    def piece(self, L, strand=False):
        """(the plant, what the letter in front of it must not be, what the letter behind it must not be)"""
        p = self.source(L)
        s, before, after = self.big[p:p + L], self.big[p - 1], self.big[p + L]
        if strand:
            return rc(s), rc(after), rc(before)
        return s, before, after

    def wrapped(self, s, before, after, pre, post):
        """the plant in background, `pre` letters in front and `post` behind"""
        left = (self.bg(pre - 1) + flank(self.rng, before)) if pre else ""
        right = (flank(self.rng, after) + self.bg(post - 1)) if post else ""
        return left + s + right

    def put(self, cell, kind, off, j, seam, strand=False):
        """a plant of K + j bases in a read of its own, its first base at seam + off"""
        K, L = self.K, self.K + j
        s, before, after = self.piece(L, strand)
        pre = int(self.rng.integers(1, 20))
        self.fill_to(seam + off - pre)
        r = self.add(self.wrapped(s, before, after, pre, int(self.rng.integers(1, 20))), j + 1, 0 if strand else j + 1)
        self.plants.append(Plant(cell, kind, off, K, j, r, seam + off))
        return r

    def put_over_records(self, off, j, seam):
        """a plant of K + j bases laid over the boundary `seam` of two reads, its first base at seam + off"""
        K, L = self.K, self.K + j
        s, before, after = self.piece(L)
        pre = int(self.rng.integers(1, 20))
        n_a = min(max(-off, 0), L)                                                       # the plant's bases in the read in front
        if off < 0:
            self.fill_to(seam + off - pre)
            a = self.bg(pre - 1) + flank(self.rng, before) + s[:n_a]
            if -off > L:
                a += flank(self.rng, after) + self.bg(-off - L - 1)
            rec = self.add(a, max(0, n_a - K + 1))
            assert self.pos == seam, (off, j)
            self.add(s[n_a:] + flank(self.rng, after) + self.bg(int(self.rng.integers(1, 20))), max(0, L - n_a - K + 1))
        else:
            self.fill_to(seam)
            b = ((self.bg(off - 1) + flank(self.rng, before)) if off else "") + s + flank(self.rng, after) + self.bg(int(self.rng.integers(1, 20)))
            rec = self.add(b, j + 1)
        self.plants.append(Plant("forward", "record", off, K, j, rec, seam + off))

    def window(self, bset, r, b, e, f, hits, hits_fwd=None):
        self.bsets.setdefault(bset, {})[r] = (b, e, f)
        self.expect_win.setdefault(bset, {})[r] = (hits, hits if hits_fwd is None else hits_fwd)


def offsets(K):
    return range(-(K + 1), 3)


def place_case(seed, K, ref, block_offs):
    """the placement, strand, substitution, length and bounds cells of one K"""
    B = Builder(9300 + 37 * K + seed, K, ref)
    rng = B.rng
    B.add("")                                                                            # an empty record first
    B.add(B.bg(70))
    # length cells: reads that are reference bases from end to end
    for n in sorted({0, 1, 2, 3, K - 1, K, K + 1, 63, 64, 65, 150, 4095, 4096, 4097, 13001}):
        p = 0 if n >= len(B.big) else int(rng.integers(0, len(B.big) - n))
        r = B.add(B.big[p:p + n], max(0, n - K + 1))
        B.plants.append(Plant("length", "record", 0, K, n - K, r, None, "%d reference bases" % n))
        B.add(B.bg(int(rng.integers(1, 90))))
    # lane and load seams: forward with every j, the reverse complement with every j
    for kind, add in (("lane", 0), ("load", LOAD)):
        for strand in (False, True):
            for j in JS:
                for off in offsets(K):
                    seam = -(-(B.pos + 60) // LANE) * LANE + add
                    B.put("strand" if strand else "forward", kind, off, j, seam, strand)
    # record seams
    for j in JS:
        for off in offsets(K):
            B.put_over_records(off, j, B.pos + 80)
    # substitutions in a plant of K + 5 bases: the hits lost are the windows that cover the changed base
    L = K + 5
    for i in sorted({0, L - 1} | ({K - 17, K - 16} if K >= 17 else set())):
        for to in ("other", "N", "R", "-"):
            s, before, after = B.piece(L)
            ch = to if to != "other" else "ACGT"[("ACGT".index(s[i]) + 1 + int(rng.integers(0, 3))) % 4]
            assert ch != s[i]
            lost = min(i, 5) - max(0, i - K + 1) + 1
            seam = -(-(B.pos + 60) // LANE) * LANE
            pre = int(rng.integers(1, 20))
            B.fill_to(seam - pre - (K - 1 if i else 0))                                  # the changed base's k-mers on either side of a lane seam
            r = B.add(B.wrapped(s[:i] + ch + s[i + 1:], before, after, pre, int(rng.integers(1, 20))), 6 - lost)
            B.plants.append(Plant("substitution", "lane", i, K, 5, r, None, "base %d to %s" % (i, ch)))
    # K - 1 bases of a k-mer of the set and one other base
    for _ in range(4 if K > 1 else 0):
        s, before, after = B.piece(K)
        last = "ACGT"[("ACGT".index(s[-1]) + 1 + int(rng.integers(0, 3))) % 4]
        r = B.add(B.wrapped(s[:-1] + last, before, None, 7, 9))
        B.plants.append(Plant("near", "lane", 0, K, 0, r, None, "K - 1 bases of the set"))
    # a k-mer that spans two reference records
    if K >= 2:
        x, y = canon(ref.records[BIG]), canon(ref.records[NEXT])
        a = K // 2
        r = B.add(B.bg(33) + x[-a:] + y[:K - a] + B.bg(21))
        B.plants.append(Plant("spanning", "lane", 0, K, 0, r, None, "a k-mer over two reference records"))
    # the even-K palindrome: once, whichever strand
    if K == len(ref.palindrome):
        r = B.add(B.bg(40) + ref.palindrome + B.bg(31), 1)
        B.plants.append(Plant("palindrome", "lane", 0, K, 0, r, None, "its own reverse complement"))
    # windows that cut a plant to K - 1, K and K + 1 bases, from either end; rows without KEPT on a plant
    for m in (K - 1, K, K + 1):
        for front in (False, True):
            s, before, after = B.piece(K + 5)
            pre = int(rng.integers(1, 20))
            r = B.add(B.wrapped(s, before, after, pre, 12), 6)
            b, e = (pre + K + 5 - m, pre + K + 5) if front else (pre, pre + m)
            B.window("win", r, b, e, KEPT | (CLIPPED if front else 0), max(0, m - K + 1))
            B.plants.append(Plant("window", "record", m - K, K, 5, r, None, "a window of %d plant bases" % m))
    for f in (SHORT, ERRORS | CLIPPED, 0):
        s, before, after = B.piece(K + 5)
        r = B.add(B.wrapped(s, before, after, 9, 12), 6)
        B.window("win", r, 3, K + 9, f, None)
        B.plants.append(Plant("dropped", "record", 0, K, 5, r, None, "flags %d" % f))
    B.verdict_read = B.plants[-1].rec                                                    # six hits without bounds: the verdict cells
    # tile seams
    for j in JS:
        for off in offsets(K):
            B.put("forward", "tile", off, j, -(-(B.pos + 60) // TILE) * TILE)
    # a read of 300000 bases that begins here, a plant in it over the next block seam
    s, before, after = B.piece(K + 5)
    seam = -(-(B.pos + K + 40) // BLOCK) * BLOCK
    pre = seam - (K + 2) - B.pos
    r = B.add(B.wrapped(s, before, after, pre, 300000 - pre - K - 5), 6)
    assert len(B.reads[r]) == 300000
    B.plants.append(Plant("length", "block", -(K + 2), K, 5, r, seam - K - 2, "300000 bases"))
    # block seams: one plant each
    seam = -(-(B.pos + 60) // BLOCK) * BLOCK
    for n, off in enumerate(block_offs):
        B.put("forward", "block", off, JS[(n + K + seed) % 3], seam + n * BLOCK)
    B.fill_to(B.pos + 100)
    B.add("")
    return Case("place%d" % K, B, ref, (K,))


def end_case(seed, K, off, j, ref):
    """a tiny text whose stream ends -off bases behind a plant's first base: the plant is cut there"""
    B = Builder(9500 + 41 * K - off + 1000 * j + seed, K, ref)
    L = K + j
    s, before, after = B.piece(L)
    B.add(B.bg(int(B.rng.integers(1, 9))))
    B.fill_to(int(B.rng.integers(150, 400)))
    n = min(-off, L)
    rd = B.wrapped(s[:n], before, None, int(B.rng.integers(1, 20)), 0)
    if -off > L:
        rd += flank(B.rng, after) + B.bg(-off - L - 1)
    r = B.add(rd, max(0, n - K + 1))
    B.plants.append(Plant("forward", "stream", off, K, j, r, B.pos + off))
    return Case("end%d%dj%d" % (K, off, j), B, ref, (K,), lower=False)


def ones_case(seed, ref):
    """5000 reads of one base"""
    B = Builder(9600 + seed, 1, ref)
    for ch in B.rng.integers(0, 5, 5000):
        B.add("ACGTN"[int(ch)])
    return Case("ones", B, ref, (1, 15), lower=False)


def small_case(name, seed, ref, ks, alphabet="ACGT", seq_type=0, source=None):
    """a few plants of K + 5 bases per K, forward and reverse complement, against a reference of another kind"""
    B = None
    reads, expect, expect_fwd = [], {}, {}
    for K in ks:
        B = Builder(9700 + seed + K, K, source or ref)
        for strand in (False, True):
            for _ in range(3):
                B.put("strand" if strand else "forward", "lane", int(B.rng.integers(-K, 3)), 5, -(-(B.pos + 60) // LANE) * LANE, strand)
        B.add(B.bg(50))
        for p in B.plants:                                                               # K + 5 bases of the reference: hits at every K of the case
            for K2 in ks:
                expect[(K2, len(reads) + p.rec)] = max(0, K + 5 - K2 + 1); expect_fwd[(K2, len(reads) + p.rec)] = 0 if p.cell == "strand" else max(0, K + 5 - K2 + 1)
        reads += B.reads
    B.reads = [r.replace("T", "U") for r in reads] if seq_type == 1 else reads
    B.plants = []
    c = Case(name, B, ref, ks, seq_type=seq_type, lower=False)
    c.expect_k, c.expect_fwd_k = expect, expect_fwd
    return c


def big_ref_case(seed, source):
    """a reference of 150 000 bases -- more keys than half the bits of the default prefilter -- and a few plants of it among clean reads"""
    rng = np.random.default_rng(9900 + seed)
    ref = Ref("big", ["", capped(rng, 150000), capped(rng, 300)])
    return small_case("big_ref", seed + 5, ref, (15, 27))


def chain_case(seed):
    """dedup_plan's FASTQ reads -- qualities that fall, adapters, copies and reverse complements -- against a reference made of eleven of them"""
    import dedup_plan as DP
    d = DP.fastq_case(7180 + seed)
    ref = Ref("reads", [d.records[k] for k in (3, 14, 40, 77, 100, 250, 251, 400, 555, 700, 899)] + [DP.rc(d.records[9])])
    B = Builder(0, 27, main_ref(seed))
    B.reads = d.records
    c = Case("chain", B, ref, (27,), fmt="fastq", lower=False)
    c.quals, c.adapter, c.text, c.ids = d.quals, d.adapter, d.text, d.ids
    return c


# ---- texts -------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, B, ref, ks, fmt="fasta", seq_type=0, lower=True):
        self.name, self.ref, self.ks, self.fmt, self.seq_type = name, ref, ks, fmt, seq_type
        self.plants, self.bsets, self.expect, self.expect_fwd, self.expect_win = B.plants, B.bsets, B.expect, B.expect_fwd, B.expect_win
        self.verdict_read = getattr(B, "verdict_read", None)
        recs = B.reads
        if lower and recs:                                                               # the soft mask plays no part
            rng = np.random.default_rng(len(recs))
            for k in rng.integers(0, len(recs), 40):
                recs[k] = recs[k].lower() if int(k) % 2 else recs[k][:len(recs[k]) // 2] + recs[k][len(recs[k]) // 2:].lower()
        self.records = recs
        self.ids = ["r%d" % k for k in range(len(recs))]
        self.text = LP.fasta(recs, 80, self.ids)
        self.stream = Stream(recs)
        self.starts = self.stream.base
        self.expect_k = self.expect_fwd_k = None

    def bounds(self, bset):
        """the bounds rows of a set: the plants' own, the whole record (kept) for every other read"""
        own = self.bsets.get(bset, {})
        return [own.get(r, (0, len(rec), KEPT)) for r, rec in enumerate(self.records)]

    def expected(self, K, forward_only=False, bset=None):
        """the hits of every read as the construction has them, None where the read takes no part"""
        if self.expect_k is not None:
            src = self.expect_fwd_k if forward_only else self.expect_k
            return [src.get((K, r), 0) for r in range(len(self.records))]
        src = self.expect_fwd if forward_only else self.expect
        out = [src.get(r, 0) for r in range(len(self.records))]
        for r, (h, hf) in (self.expect_win.get(bset, {}) if bset else {}).items():
            out[r] = hf if forward_only else h
        return out


def claims_hold(case, K, rows, forward_only=False, bset=None):
    """the rows of a whole text against what its construction says: equal from K = EXACT_K on, at least that below"""
    if not case.expect and not case.expect_k:
        return True
    want = case.expected(K, forward_only, bset)
    bounds = case.bounds(bset) if bset else None
    for r, w in enumerate(want):
        got = int(rows[r]["hits"])
        if w is None or (bounds and not bounds[r][2] & KEPT):
            if got != 0 or (bounds and int(rows[r]["flags"]) != bounds[r][2]):
                return False
        elif got != w if K >= EXACT_K else got < w:
            return False
    return True


_cache = {}


def planned(seed=0):
    """the cases"""
    if seed not in _cache:
        ref = main_ref(seed)
        for K in KS:
            if K > RUN_CAP:
                check_reference(ref.records, K)
        cases = []
        for n, K in enumerate(KS):
            offs = list(offsets(K))
            if K == 1:
                cases.append(place_case(seed, K, ref, offs[:4]))                         # (the fifth offset is K = 2's: with the long read's that makes five seams, 1.3 M bases)
            else:
                cases.append(place_case(seed, K, ref, [offs[(3 * n + 2 * seed + q * (len(offs) // 2 + 1)) % len(offs)] for q in range(2)] + ([2] if K == 2 else [])))
        for K in KS:
            for off in range(-(K + 1), 0):
                for j in JS:
                    cases.append(end_case(seed, K, off, j, ref))
        cases.append(ones_case(seed, ref))
        rna, fq = main_ref(seed, "rna", seq_type=1, big=3000), main_ref(seed, "fastq", fmt="fastq", big=3000)
        cases += [small_case("dna_rna", seed, rna, (15, 27)), small_case("rna_dna", seed + 1, main_ref(seed, big=3000), (16, 31), seq_type=1),
                  small_case("dna_fastq", seed + 2, fq, (17, 31)),
                  small_case("dna_none", seed + 3, none_ref(seed), (15, 31), source=ref), small_case("dna_empty", seed + 4, Ref("empty", []), (15, 27), source=ref),
                  chain_case(seed)]
        for c in cases[-3:-1]:                                                           # no read matches a reference without k-mers
            c.expect_k = {k: 0 for k in c.expect_k}; c.expect_fwd_k = dict(c.expect_k)
        cases.append(big_ref_case(seed, ref))
        _cache[seed] = cases
    return _cache[seed]


def small_names(cases):
    """the cases small enough for every value of the levers (insertion is quadratic when every key shares one chain)"""
    return [c.name for c in cases if c.name.startswith("end") or c.name in ("dna_none", "dna_empty")]


def coverage(cases):
    """{(cell, seam kind): plants}"""
    out = {}
    for c in cases:
        for p in c.plants:
            out[(p.cell, p.kind)] = out.get((p.cell, p.kind), 0) + 1
    return out


def random_reads(seed, n=300):
    """reads over all sixteen codes, short, with pieces of a random reference among them; (reads, reference records)"""
    rng = np.random.default_rng(9800 + seed)
    ref = [LP._random(rng, int(rng.integers(0, 120)), "ACGTN" if k % 3 else LP.CODES + "acgtu") for k in range(12)]
    out = []
    for k in range(n):
        s = LP._random(rng, int(rng.integers(0, 12 if k % 4 == 0 else 90)), LP.CODES if k % 2 else "ACGTN")
        if k % 3 == 0:
            src = canon(ref[int(rng.integers(0, len(ref)))])
            a = int(rng.integers(0, len(src) + 1)); piece = src[a:a + int(rng.integers(0, 40))]
            s = s[:len(s) // 2] + (rc(piece) if k % 2 and set(piece) <= set("ACGT") else piece.lower() if k % 5 == 0 else piece) + s[len(s) // 2:]
        out.append(s)
    return out, ref
