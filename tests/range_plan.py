"""Where to cut a text for byte-range tests (tests/test_gpu_ranges.py, tests/test_ranges_cpu.py): the text offsets at which something
changes -- a record's header, a line end, the nibble pair and the group of 16 of the packed stream, the stream and block seams of a
frame, a mask toggle, the bases behind the last record -- listed by class from the oracle's text and the archive's header alone.
Nothing here touches the GPU or the code under test.

A Plan restates the text's layout (oracle/naf_oracle.c nafo_unnaf) as arithmetic over the record lengths, so that the offset of any base
is a formula and a text of tens of MB needs no array of its size; brute_base_map() is the plain walk of the text beside the bases that
tests/test_ranges_cpu.py holds the formula to."""
import numpy as np

from oracle import oracle as O

FASTA, FASTQ, SEQ, SEQUENCES, FOURBIT = O.MODE_FASTA, O.MODE_FASTQ, O.MODE_SEQ, O.MODE_SEQUENCES, O.MODE_4BIT
CLASSES = ("record", "line", "pair", "group", "stream", "block", "mask", "tail", "fastq")
LENGTHS = (1, 16, 4095, 4096, 4097, 3 * 4096 + 5)          # of a planned cut: below, at and above a tile, and a few tiles
PATHS = ("", "long", "span", "short", "slow")              # NAF_GPU_EMIT, and NAF_GPU_FORCE_SLOW=1


def record_lengths(naf, h=None):
    h = h or O.parse_naf(naf)
    if h.payload_off[O.LENGTHS] is None or h.orig[O.LENGTHS] == 0:
        return np.zeros(0, dtype=np.int64)
    u = np.frombuffer(O.zstd_decompress(h.frame(naf, O.LENGTHS)), dtype="<u4").astype(np.int64)
    assert not (u == 0xFFFFFFFF).any(), "a record of 4 Gi bases: not in these tests"
    return u[: h.n_sequences]


class Plan:
    """The layout of `want` = oracle.unnaf(naf, mode, use_mask, ll).  own: the archive is this build's (frames of 32 KiB blocks in four
    streams); otherwise the reference's (128 KiB blocks)."""

    def __init__(self, naf, want, mode, use_mask=True, ll=-1, own=False):
        h = O.parse_naf(naf)
        self.want, self.mode, self.own = want, mode, own
        self.fourbit = h.seq_type <= O.RNA
        self.n = len(want)
        self.lens = record_lengths(naf, h)
        self.N = len(self.lens)
        self.cum = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)          # first base of record r
        self.T = int(self.cum[-1])                                                       # bases the records hold
        self.T_all = int(h.orig[O.SEQ])                                                  # bases of the stream
        self.surplus = self.T_all - self.T
        assert self.surplus >= 0
        self.L = int(h.line_length if ll < 0 else ll) if mode == FASTA else 0
        w = np.frombuffer(want, dtype=np.uint8)
        L, lens = self.L, self.lens
        if mode in (FASTA, FASTQ):
            if mode == FASTA:
                body = np.where(lens > 0, lens + (-(-lens // L) if L else 1), 0)
            else:
                body = 2 * lens + 4                                                      # bases \n + \n quality \n
            nl = np.flatnonzero(w == 10)
            self.hdr = np.zeros(self.N, dtype=np.int64)                                  # first byte of the header line
            self.body = np.zeros(self.N, dtype=np.int64)                                 # first byte behind it
            p = 0
            for r in range(self.N):
                self.hdr[r] = p
                e = int(nl[np.searchsorted(nl, p)]) + 1                                  # (a name holds no line end)
                self.body[r] = e
                p = e + int(body[r])
            self.main_total = p
        elif mode == SEQUENCES:
            self.body = self.cum[:-1] + np.arange(self.N)
            self.hdr = self.body
            self.main_total = self.T + self.N
        elif mode == SEQ:
            self.body = self.hdr = self.cum[:-1]
            self.main_total = self.T
        else:
            self.body = self.hdr = self.cum[:-1] // 2
            self.main_total = self.n
        assert self.main_total <= self.n and (self.surplus or self.main_total == self.n or mode == FOURBIT), (self.main_total, self.n)
        # case of every base, in stream order (the mask, as the text shows it)
        self.toggles = np.zeros(0, dtype=np.int64)
        if mode != FOURBIT and use_mask:
            s = np.frombuffer(O.unnaf(naf, SEQ, use_mask=True), dtype=np.uint8)[: self.T]
            low = (s >= 97) & (s <= 122)
            self.toggles = np.flatnonzero(low[1:] != low[:-1]) + 1
            if mode == FASTQ:                                                            # (FASTQ output never masks: unnaf.c:442)
                self.toggles = self.toggles[:0]
        bpb = 2 if self.fourbit else 1
        self.stream_bases = 8192 * bpb if own else 0
        self.block_bases = (32768 if own else 131072) * bpb

    # ---- base index -> text offset -----------------------------------------------------------------------------------------------
    def base_pos(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        if self.mode == SEQ:
            return idx.copy()
        if self.mode == FOURBIT:
            return idx // 2
        r = np.searchsorted(self.cum, idx, side="right") - 1
        k = idx - self.cum[r]
        return self.body[r] + k + (k // self.L if self.L else 0)

    def anchors(self, cls, among):
        """The positions of `among` a trimmed sample must keep: the header's first and last byte and the first byte behind it of the
        first and the last record; the first and last three line ends of the first and the last record that have lines."""
        among = np.asarray(among, dtype=np.int64)
        if cls == "record" and self.N:
            r = np.asarray([0, self.N - 1])
            want = np.concatenate([self.hdr[r], self.body[r] - 1, self.body[r]]) if self.mode in (FASTA, FASTQ) else self.body[r]
            return np.intersect1d(among, want)
        if cls == "line" and self.mode == FASTA and self.N:
            full = np.flatnonzero(self.lens > 0)
            out = []
            for r in ([full[0], full[-1]] if len(full) else []):
                end = self.hdr[r + 1] if r + 1 < self.N else self.main_total
                inside = among[(among >= self.body[r]) & (among < end)]
                out += inside[:3].tolist() + inside[-3:].tolist()
            return np.unique(np.asarray(out, dtype=np.int64))
        return among[:0]

    def count(self, cls):
        return len(self.positions(cls, None, None))

    def possible(self):
        """The classes this text can have, from the archive's properties alone."""
        c = {"record", "tail"}
        if self.mode in (FASTA, SEQUENCES) and self.T:
            c.add("line")
        if self.fourbit and self.T > 1:
            c.add("pair")
        if self.fourbit and self.T > 16:
            c.add("group")
        if self.stream_bases and self.T > self.stream_bases:
            c.add("stream")
        if self.T > self.block_bases:
            c.add("block")
        if len(self.toggles):
            c.add("mask")
        if self.mode == FASTQ:
            c.add("fastq")
        return c

    # ---- positions by class ------------------------------------------------------------------------------------------------------
    def _pick(self, count, k, rng, always=()):
        """k of range(count), the `always` among them; all when k is None or count <= k."""
        if k is None or count <= k:
            return np.arange(count, dtype=np.int64)
        a = np.unique(np.asarray([x for x in always if 0 <= x < count], dtype=np.int64))[:k]
        rest = rng.choice(count, size=min(count, 2 * k), replace=False) if count <= 100_000 else rng.integers(0, count, 2 * k + 8)
        rest = np.setdiff1d(np.unique(rest), a)
        rng.shuffle(rest)
        return np.sort(np.concatenate([a, rest[: k - len(a)]])).astype(np.int64)

    def positions(self, cls, k, rng):
        """Text offsets of class cls: all of them (k None) or a seeded sample that holds k where the text has k (empty records share
        their offsets, so the sample is widened until it does); sorted, unique, inside [0, n]."""
        kk = k
        for _ in range(12):
            p = self._positions(cls, kk, rng)
            if k is None or len(p) >= k:
                break
            kk *= 4
        return p

    def _positions(self, cls, k, rng):
        T, lens = self.T, self.lens
        if cls == "record":
            r = self._pick(self.N, k, rng, always=(0, 1, self.N - 2, self.N - 1))
            if self.mode in (FASTA, FASTQ):
                p = np.concatenate([self.hdr[r], self.body[r] - 1, self.body[r]])
            elif self.mode == SEQUENCES:
                p = np.concatenate([self.body[r], self.body[r] + lens[r]])
            else:
                p = self.body[r]
        elif cls == "line":
            if self.mode == SEQUENCES:
                r = self._pick(self.N, k, rng, always=(0, 1, 2, self.N - 3, self.N - 2, self.N - 1))
                p = self.body[r] + lens[r]
            elif self.mode == FASTA:
                L = self.L
                nlines = np.where(lens > 0, -(-lens // L) if L else 1, 0)
                lc = np.concatenate([[0], np.cumsum(nlines)])
                tot = int(lc[-1])
                always = []
                full = np.flatnonzero(lens > 0)
                for r in self._pick(self.N, None if k is None else max(2, k // 6), rng, always=(int(full[0]), int(full[-1])) if len(full) else ()):
                    a, b = int(lc[r]), int(lc[r + 1])
                    always += [x for x in (a, a + 1, a + 2, b - 3, b - 2, b - 1) if a <= x < b]        # the first and last three of a record
                j = self._pick(tot, k, rng, always=always)
                r = np.searchsorted(lc, j, side="right") - 1
                q = j - lc[r]
                last = q == nlines[r] - 1
                p = np.where(last, self.body[r] + lens[r] + nlines[r] - 1, self.body[r] + (q + 1) * (L + 1) - 1)
            else:
                p = np.zeros(0, dtype=np.int64)
        elif cls == "pair":
            p = self.base_pos(2 * self._pick(T // 2, k, rng, always=(0, T // 2 - 1)) + 1) if self.fourbit else np.zeros(0, dtype=np.int64)
        elif cls == "group":
            if self.fourbit and T > 16:
                g = self._pick((T - 1) // 16, k, rng, always=(0, (T - 1) // 16 - 1))               # group g + 1 starts at base 16 (g + 1)
                p = self.base_pos(np.concatenate([16 * (g + 1) - 1, 16 * (g + 1)]))
            else:
                p = np.zeros(0, dtype=np.int64)
        elif cls in ("stream", "block"):
            step = self.stream_bases if cls == "stream" else self.block_bases
            cnt = (T - 1) // step if step and T else 0
            s = self._pick(cnt, k, rng, always=(0, cnt - 1))
            p = self.base_pos(step * (s + 1))
        elif cls == "mask":
            t = self.toggles
            p = self.base_pos(t[self._pick(len(t), k, rng, always=(0, len(t) - 1))]) if len(t) else np.zeros(0, dtype=np.int64)
        elif cls == "tail":
            p = np.asarray(([self.main_total] if self.surplus and self.mode != FOURBIT else []) + [self.n], dtype=np.int64)
        elif cls == "fastq":
            if self.mode == FASTQ:
                r = self._pick(self.N, k, rng, always=(0, self.N - 1))
                b, n = self.body[r], lens[r]
                p = np.concatenate([self.hdr[r], b - 1, b, b + n, b + n + 1, b + n + 2, b + n + 3, b + 2 * n + 3])
            else:
                p = np.zeros(0, dtype=np.int64)
        else:
            raise KeyError(cls)
        p = np.unique(p)
        return p[(p >= 0) & (p <= self.n)]


def brute_base_map(want, bases, lens, mode):
    """Text offset of every base of the records, by walking the text: skip a record's header line, then take bytes that are no
    line end until the record's bases are used up, each compared with the base it should be (case apart)."""
    out, p, i = [], 0, 0
    for n in lens:
        if mode in (FASTA, FASTQ):
            p = want.index(b"\n", p) + 1
        for _ in range(int(n)):
            while want[p] == 10:
                p += 1
            assert (want[p] ^ bases[i]) & 0xDF == 0, (p, i)
            out.append(p); p += 1; i += 1
        if mode == FASTQ:
            assert want[p:p + 3] == b"\n+\n"
            p += 3 + int(n) + 1
        elif mode == SEQUENCES or (mode == FASTA and n):
            assert want[p] == 10
            p += 1
    return out, p


def first_diff(got, exp):
    if len(got) != len(exp):
        m = min(len(got), len(exp))
        g, e = np.frombuffer(got[:m], dtype=np.uint8), np.frombuffer(exp[:m], dtype=np.uint8)
        d = np.flatnonzero(g != e)
        return "length %d for %d, first differing offset %d" % (len(got), len(exp), int(d[0]) if len(d) else m)
    d = np.flatnonzero(np.frombuffer(got, dtype=np.uint8) != np.frombuffer(exp, dtype=np.uint8))
    return "first differing offset %d" % int(d[0])


# ---- the texts of the sweeps (built from the seed alone, so that the CPU module plans the very texts the GPU module cuts) ------------
def _dna(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)]


def _wrap(b, width):
    from naf_amd import synth
    return synth.wrap_lines(np.asarray(b, dtype=np.uint8), width)


def _short_runs(rng, per):
    """`per` bases whose case changes every 1..40 bases (tests/test_gpu_encode.py test_mask_of_short_runs_written_without_the_scan)."""
    b = _dna(rng, per)
    edges = np.cumsum(rng.integers(1, 41, per // 10)); edges = edges[edges < per]
    lower = (np.searchsorted(edges, np.arange(per), side="right") & 1).astype(bool)
    return np.where(lower, b | 0x20, b).astype(np.uint8)


def _with_run(b, at, n, lower):
    b[at:at + n] = (b[at:at + n] | 0x20) if lower else (b[at:at + n] & 0xDF)


def planned_texts(seed):
    """(name, text, seq_type) of sweep (b): 1 .. 3 MB each."""
    from naf_amd import synth
    rng = np.random.default_rng(1000 + seed)
    out = [("mixed_long", synth.fasta_mixed(60, 40000, 60, seed=101 + seed, empty_every=5), O.DNA),
           ("mixed_short", synth.fasta_mixed(4000, 300, 60, seed=102 + seed, empty_every=7), O.DNA)]
    for w in (60, 61, 80, 4095, 4096, 4097, 0):
        out.append(("acgt_w%d" % w, synth.fasta_acgt(1_000_003, 3, w, seed=110 + w + seed), O.DNA))
    recs = []
    for r in range(4):
        b = _short_runs(rng, 300_000)
        if r == 0: _with_run(b, 0, 254, False); _with_run(b, 100_000, 254, True); _with_run(b, 200_000, 255, True)
        if r == 1: _with_run(b, 50_000, 256, False); _with_run(b, 120_000, 70_000, True)
        if r == 3: _with_run(b, 300_000 - 300, 300, True)
        recs.append(b">s%d\n" % (r + 1) + _wrap(b, 60))
    out.append(("short_runs", b"".join(recs), O.DNA))
    # a control byte inside an id puts an N into the stream that no length accounts for: bases behind the last record
    out.append(("surplus", b">big\x01\x02 c\n" + _wrap(_dna(rng, 600_000, b"ACGTacgtNn"), 60) + b">big2\x05\n" + _wrap(_dna(rng, 500_001, b"ACGTacgtNn"), 60)
                + b">third" + b"\x01" * 130 + b" x\n" + _wrap(_dna(rng, 7), 60), O.DNA))
    aa = b"ACDEFGHIKLMNPQRSTVWYacdxX*"
    out.append(("protein", b"".join(b">p%d some protein\n" % k + _wrap(_dna(rng, int(rng.integers(0, 600)), aa), 60) for k in range(4000)), O.PROTEIN))
    chars = bytes(c for c in range(33, 127) if c != ord(">"))
    out.append(("text", b"".join(b">t%d\n" % k + _wrap(_dna(rng, int(rng.integers(1, 100_000)), chars), 70) for k in range(24)), O.TEXT))
    out.append(("fastq_fixed", synth.fastq_reads(4000, 150, seed=120 + seed), O.DNA))
    out.append(("fastq_var", synth.fastq_reads(8000, 150, seed=121 + seed, var_len=True), O.DNA))
    return out


def views_of(text, seq_type, k=0):
    """(mode, use_mask, ll) text k of sweep (b) is cut under; the first is the one sampled at full depth.  The line lengths 0, 1, 15, 16,
    17, 33 take the mask on and off alternately, odd texts the other way round than even ones: every pairing occurs across the texts."""
    if text[:1] == b"@":
        return [(FASTQ, True, -1), (FASTA, True, -1), (FASTA, k & 1 == 1, 16), (SEQ, True, -1), (SEQ, False, -1), (SEQUENCES, True, -1), (FOURBIT, True, -1)]
    v = [(FASTA, True, -1), (FASTA, False, -1)] + [(FASTA, (i + k) & 1 == 0, ll) for i, ll in enumerate((0, 1, 15, 16, 17, 33))]
    v += [(SEQ, True, -1), (SEQ, False, -1), (SEQUENCES, True, -1), (SEQUENCES, False, -1)]
    return v + ([(FOURBIT, True, -1)] if seq_type <= O.RNA else [])


# bases, records, width, read in place under a range: an odd count whose odd base is alone in the last block (a Raw block of one byte), an
# even one, one that ends on a block -- and an odd count whose last block holds the odd nibble beside others: a second Huffman tree, a
# frame the whole-text call reads mostly in place and most range calls decode
FLAT_TEXTS = ((65536 * 457 + 1, 3, 80, True), (30_000_000, 5, 71, True), (65536 * 420, 1, 60, True), (30_000_001, 3, 80, False))
FLAT_VIEWS = [(FASTA, True, -1), (FASTA, False, -1), (FASTA, True, 50), (FASTA, True, 0), (SEQ, True, -1), (SEQ, False, -1), (SEQUENCES, True, -1)]
FLAT_CLASSES = ("pair", "group", "stream", "block", "line", "record", "tail")
FLAT_LENGTHS = LENGTHS + (98_304 + 77,)                                            # and about a block and a half of this build's frames


def flat_text(k, seed):
    """Text k of sweep (c): uniform A C G T, large enough for the frame to be read in place with NAF_GPU_SPEC_MIN=8."""
    from naf_amd import synth
    n, rec, w, _ = FLAT_TEXTS[k]
    return synth.fasta_acgt(n, rec, w, seed=130 + k + seed)


MATCH_GOLDEN = ("repeat_l1", "repeat_l19", "repeat_long27", "fastq_4k", "mixed_60")
MATCH_CLASSES = ("block", "record", "line", "pair")


def sparse_text(seed):
    """Mostly unique sequence with a few far-apart copies (level 5 finds them): sweep (d)'s own archive."""
    rng = np.random.default_rng(2000 + seed)
    body = _dna(rng, 2_000_000).copy()
    for k in range(8):
        a, b = int(rng.integers(0, 1_700_000)), int(rng.integers(0, 1_950_000))
        body[b:b + 40_000] = body[a:a + 40_000].copy()
    return b">chrS sparse repeats\n" + _wrap(body, 70)


def match_views(name):
    return [(FASTQ, True, -1), (SEQUENCES, True, -1)] if name.startswith("fastq") else [(FASTA, True, -1), (SEQUENCES, True, -1)]


K_MAIN, K_OTHER = 20, 3        # positions per class in a text's first view / in each other view


def planned_jobs(plan, classes, k, rng, lengths=LENGTHS, paths=PATHS, counter=0):
    """The range calls of one view: per class up to k positions, per position the ten anchors (a begin, an end, at p-2 .. p+2), every
    anchor with one length and one path, both rotating from anchor to anchor -- (class, p, a, b, path)."""
    jobs, c = [], counter
    for cls in classes:
        p_all = plan.positions(cls, k, rng)
        if k is not None and len(p_all) > k:                   # trim to k, the anchors first (at most three fifths of k, one at least)
            keep = plan.anchors(cls, p_all)[: max(1, 3 * k // 5)]
            rest = np.setdiff1d(p_all, keep)
            p_all = np.sort(np.concatenate([keep, rng.choice(rest, size=k - len(keep), replace=False)])).astype(np.int64)
        for p in p_all:
            p = int(p)
            for d in (-2, -1, 0, 1, 2):
                x = p + d
                if not 0 <= x <= plan.n:
                    continue
                for side in (0, 1):
                    ln = lengths[c % len(lengths)]; path = paths[(c // 2) % len(paths)]; c += 1
                    a, b = (x, min(plan.n, x + ln)) if side == 0 else (max(0, x - ln), x)
                    if b > a:
                        jobs.append((cls, p, a, b, path))
    return jobs, c


PLANNED_NAMES = ("mixed_long", "mixed_short", "acgt_w60", "acgt_w61", "acgt_w80", "acgt_w4095", "acgt_w4096", "acgt_w4097", "acgt_w0", "short_runs", "surplus",
                 "protein", "text", "fastq_fixed", "fastq_var")            # planned_texts(), in order
