"""Texts for the encoder's seam tests (tests/test_gpu_seams.py, tests/test_seams_cpu.py): a regular FASTA or FASTQ background with each
structural feature of such a text -- a header's '>', the blank behind an ID, a case toggle, a damaged byte, a '+' line ... -- planted so
that the byte that defines it sits at a chosen offset against the seams the split kernels cut a text by: the tile of 4096 bytes, the
lane's 64 and the piece of 16.  Nothing here touches the GPU or the code under test, and nothing is imported from it.

A plant is (feature, unit, delta): the feature's defining byte lies at k * unit + delta for a seam k inside the text.  A plant is moved to
its place by the record in front of it: that record's free-form comment is lengthened (FASTA: and its last line left ragged, as the last
line of a record is), so the line lattice behind a plant has whatever phase that leaves -- each Text lists its plants with their offsets.
Plants follow each other SPACING tiles apart (never closer than three), the first one of every text at the seam of tiles 0 / 1 behind
blank lines (the first marker is not the text's first byte), and every text's last byte is a plant of its own (END_FEATURES: with and
without a final line end; the end of the text is where it is, so it alone may lie closer to the plant in front of it).  "The last whole
seam before the end" is read as that end plant: no other feature is planted in a text's last tiles.  The segment-count, alignment and
dying texts carry their own plants only, neither a first-seam plant nor an end plant.

Every FASTA text also holds one long record of plain, regular tiles (STRETCH), the only place a direct block of 65536 bases can lie:
plants a few tiles apart leave no room for one.  What a direct block can hold of the features -- a lower-case run -- is planted inside
that record as well, its first and its last base at every delta of the tile seam (stretch_lower_first / stretch_lower_last), so that
the gather of a direct block's codes and case bits across tile seams meets planted seams too.

Text.decoded() is the text an archive of it gives back, worked out from the format's rules alone (the records re-wrapped at the longest
line, blanks dropped, letters and bytes the format does not keep replaced): what the oracle's and the reference's decoders are held to.

Structure never depends on the random numbers: the letters, names and qualities of a text come from np.random.default_rng(base + seed),
its plants stay where they are under every seed."""
import os
import re

import numpy as np

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
TILE, LANE, PIECE = 4096, 64, 16
ANCHORS = tuple([(TILE, d) for d in (-2, -1, 0, 1, 2)] + [(LANE, d) for d in (-1, 0, 1)] + [(PIECE, d) for d in (-1, 0)])
SPACING = 4                       # tiles from a plant's seam to the next one's
PER_TEXT = 11                     # plants of a text (and its end)
WIDTHS = (32, 33, 61, 80, 2047)   # 32: the smallest width of a regular tile; 2047: two lines a tile
STRETCH = 170_000                 # bases of every FASTA text's one long record: a whole block of 65536 bases of plain, regular tiles
# combinations of feature x anchor that cannot be planted, each with its structural reason (tests/test_seams_cpu.py caps the list)
IMPOSSIBLE = []

FASTA_FAMILIES = {
    "headers": ("gt", "hdr_nl", "id_space", "id_tab", "acgt_hdr", "hdr_1byte"),
    "letters": ("lower1", "lower_first", "lower_last", "N", "R", "bang", "dash"),
    "lines": ("blank", "crlf", "cr", "space", "tab", "short_nl", "long_nl", "long5000", "odd_last"),
}
FASTQ_FAMILIES = {
    # what the tolerant parser has nothing to tolerate in: tiles stay on the fast path
    "regular": ("l0_first", "l1_first", "l2_first", "l3_first", "l0_nl", "l1_nl", "l2_nl", "l3_nl", "id_space", "id_tab", "no_comment",
                "long_hdr_first", "long_hdr_blank", "qual_at", "qual_plus", "plus_name"),
    "irregular": ("blank", "crlf", "space_seq", "bad_z", "q01", "q7f", "q80", "h01", "tab2"),
    "iupac": ("iupac",),          # the tile is regular, but handed back for its letter
}
END_FEATURES = ("end_nl", "end_no_nl")
SEGMENT_COUNTS = (63, 64, 65, 255, 256, 257)
DYING = {   # cause -> the reference's message (%d: the record's number, or that of the record in front)
    "q_short": "quality length of sequence %d (149) doesn't match sequence length (150)",
    "q_long": "quality length of sequence %d (151) doesn't match sequence length (150)",
    "no_plus": "can't find '+' line of sequence %d",
    "no_at": "Can't find '@' after sequence %d",
    "cut_hdr": "truncated FASTQ input: last sequence has no sequence data",
    "cut_seq": "truncated FASTQ input: last sequence has no quality",
    "cut_plus": "truncated FASTQ input: last sequence has no quality",
}
DYING_DELTAS = (-1, 0, 1)


class Plant:
    def __init__(self, feature, unit, delta, offset, note=""):
        self.feature, self.unit, self.delta, self.offset, self.note = feature, unit, delta, offset, note
        self.residues = (offset % TILE, offset % LANE, offset % PIECE)                             # as planted, for the record

    def __repr__(self):
        return "%s@%d (%d%+d%s)" % (self.feature, self.offset, self.unit, self.delta, ", " + self.note if self.note else "")


class Text:
    """name: kind_family_..., kind: 'fasta' / 'fastq', width: the FASTA line width (0: FASTQ), dies: the reference's message or None."""

    def __init__(self, name, kind, family, width, data, plants, dies=None, info=None):
        self.name, self.kind, self.family, self.width, self.data, self.plants, self.dies, self.info = name, kind, family, width, bytes(data), plants, dies, info or {}

    def nearest(self, offset, k=3):
        return sorted(self.plants, key=lambda p: abs(p.offset - offset))[:k]

    def decoded(self):
        return decoded_fasta(self.data) if self.kind == "fasta" else decoded_fastq(self.data)


# ---- what an archive gives back, from the format's rules ---------------------------------------------------------------------------
def _lines(data):
    """The lines of a text: any of LF, VT, FF, CR ends one, and a line with nothing in it is none."""
    return [l for l in re.split(b"[\n\x0b\x0c\r]", data) if l]


def _name(line):
    """ID and comment of a header line (its marker taken off) as they come back: the ID ends at the first blank, whatever blank it is comes
    back as one space, no comment no blank, and a control byte in the comment is a '?'."""
    m = re.search(b"[\t ]", line)
    assert not re.search(b"[\x00-\x08\x0e-\x1f\x7f\xff]", line[:m.start()] if m else line)          # (no plan damages an ID)
    if not m:
        return line
    cmt = re.sub(b"[\x00-\x1f\x7f\xff]", b"?", line[m.end():])
    return line[:m.start()] + (b" " + cmt if cmt else b"")


def _bases(line):
    """A line's letters as the 4-bit codes keep them: blanks dropped, what is no IUPAC code or '-' an N, case kept."""
    return re.sub(b"[^ABCDGHKMNRSTVWYabcdghkmnrstvwy-]", b"N", re.sub(b"[\t ]", b"", line))


def decoded_fasta(data):
    recs, L = [], 0
    for l in _lines(data):
        if l[:1] == b">":
            recs.append((_name(l[1:]), []))
        else:
            b = _bases(l)
            L = max(L, len(b))
            recs[-1][1].append(b)
    out = []
    for name, parts in recs:
        s = b"".join(parts)
        out.append(b">" + name + b"\n" + b"".join(s[i:i + L] + b"\n" for i in range(0, len(s), L)))
    return b"".join(out)


def decoded_fastq(data):
    ls = _lines(data)
    assert len(ls) % 4 == 0
    out = []
    for i in range(0, len(ls), 4):
        h, s, p, q = ls[i:i + 4]
        assert h[:1] == b"@" and p[:1] == b"+"
        q = re.sub(b"[^\x21-\x7e]", b"!", re.sub(b"[\t ]", b"", q))
        out.append(b"@" + _name(h[1:]) + b"\n" + _bases(s).upper() + b"\n+\n" + q + b"\n")
    return b"".join(out)


def target(k, unit, delta, i, t=0):
    """The offset of plant i of text t at tile seam k: on the seam (unit 4096), or on a lane / piece seam of the tile behind it that is
    no seam of the next larger unit -- any of the tile's lanes 1 .. 63 (pieces 1 .. 3 of lanes 0 .. 63), moving with i and t."""
    if unit == TILE:
        return k * TILE + delta
    if unit == LANE:
        return k * TILE + LANE * (1 + (7 * i + 11 * t) % 63) + delta
    return k * TILE + LANE * ((5 * i + 13 * t) % 64) + PIECE * (1 + (i + t) % 3) + delta


def _chunks(seq, n):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


def _deal(features):
    """The cross product features x ANCHORS in texts of PER_TEXT plants, dealt so that a text mixes features and anchors."""
    combos = [(f, u, d) for f in features for (u, d) in ANCHORS]
    combos = [combos[(37 * i) % len(combos)] for i in range(len(combos))]                       # (37 divides no count of combinations here)
    assert len(set(combos)) == len(combos)
    return _chunks(combos, PER_TEXT)


# ---- FASTA -------------------------------------------------------------------------------------------------------------------------
class _Fa:
    def __init__(self, rng, W):
        self.W, self.out, self.nrec, self.rng = W, bytearray(), 0, rng
        self.pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 700_000)]
        self.at = 0
        self.tags = np.frombuffer(b"ABCDEFGHJKLMNPQRSTUVWXYZ", dtype=np.uint8)[rng.integers(0, 24, 40_000)].tobytes()

    def bases(self, n):
        if self.at + n > len(self.pool):
            self.at = 0
        self.at += n
        return self.pool[self.at - n:self.at]

    def ident(self):
        self.nrec += 1
        return b"s%04d" % self.nrec + self.tags[4 * self.nrec:4 * self.nrec + 4]                       # 9 bytes, whatever the seed

    def wrap(self, b):
        """The bases b in lines of W, every line with its line end."""
        W, n = self.W, len(b)
        full = n // W
        a = np.full((full, W + 1), 10, dtype=np.uint8)
        a[:, :W] = np.asarray(b[:full * W]).reshape(full, W)
        return a.tobytes() + (bytes(b[full * W:]) + b"\n" if n % W else b"")

    def lines(self, n):
        return self.wrap(self.bases(n))

    def fill_to(self, start):
        """Background records up to `start`, the last one with the comment and the ragged last line that end it there."""
        W = self.W
        std = max(2, -(-1200 // W)) * W
        while start - len(self.out) > std + std // W + 60:
            self.out += b">" + self.ident() + b" len=%d\n" % std + self.lines(std)
        r = start - len(self.out) - 11                                                          # '>', the ID, the header's line end
        assert r >= 0, (start, len(self.out))
        c = r % 53
        n, rem = divmod(r - c, W + 1)
        if rem == 1:
            c, rem = c + 1, 0
        self.out += b">" + self.ident() + (b" " + b"c" * (c - 1) if c else b"") + b"\n" + self.lines(n * W + (rem - 1 if rem else 0))
        assert len(self.out) == start

    def hdr(self, tag):
        return b">" + self.ident() + b" " + tag + b"\n"

    def pre(self, depth, least=0):
        return self.lines(max(least, -(-depth // (self.W + 1))) * self.W)

    def post(self):
        return self.lines(2 * self.W + self.W // 3)


def _fa_fragment(b, f, col, depth):
    """(bytes, index of the defining byte) of feature f: a record of its own, the feature `depth` bytes of wrapped lines into it where it
    is a feature of the lines (the header that moves it is then not in its tile)."""
    W = b.W
    tag = f.encode()
    if f in ("gt", "hdr_nl", "id_space", "id_tab"):
        h = b">" + b.ident() + (b"\t" if f == "id_tab" else b" ") + tag + b"\n"
        return h + b.post(), {"gt": 0, "hdr_nl": len(h) - 1, "id_space": 10, "id_tab": 10}[f]
    if f == "acgt_hdr":
        return b">" + bytes(b.bases(2 * TILE + 300)) + b"\n" + b.post(), 0
    if f == "hdr_1byte":
        return b">\n" + b.post(), 0
    h = b.hdr(tag)
    if f in ("lower1", "N", "R", "bang", "dash"):
        p = b.pre(depth)
        line = bytearray(bytes(b.bases(W)))
        line[col] = {"lower1": line[col] | 0x20, "N": ord("N"), "R": ord("R"), "bang": ord("!"), "dash": ord("-")}[f]
        return h + p + bytes(line) + b"\n" + b.post(), len(h) + len(p) + col
    if f in ("lower_first", "lower_last"):
        b0 = max(-(-depth // (W + 1)) * W + col, 299)
        run = 300
        s = b.bases(b0 + 2 * W + 400).copy()
        if f == "lower_first":
            s[b0:b0 + run] |= 0x20
        else:
            s[b0 - run + 1:b0 + 1] |= 0x20
        return h + b.wrap(s), len(h) + b0 + b0 // W
    p = b.pre(depth, least=1 if f == "long5000" else 0)
    at = len(h) + len(p)
    if f == "blank":
        return h + p + b"\n" + b.post(), at
    if f in ("crlf", "cr"):
        return h + p + bytes(b.bases(W)) + (b"\r\n" if f == "crlf" else b"\r") + b.post(), at + W
    if f in ("space", "tab"):
        line = bytes(b.bases(W))
        return h + p + line[:col] + (b" " if f == "space" else b"\t") + line[col:] + b"\n" + b.post(), at + col
    if f in ("short_nl", "long_nl"):
        n = W - 1 if f == "short_nl" else W + 1
        return h + p + bytes(b.bases(n)) + b"\n" + b.post(), at + n
    if f == "long5000":
        return h + p + bytes(b.bases(5000)) + b"\n" + b.post(), at
    if f == "odd_last":
        n = col + 1
        if (len(p) // (W + 1) * W + n) % 2 == 0:
            n = n + 1 if n < W else n - 1
        return h + p + bytes(b.bases(n)) + b"\n", at + n - 1
    raise KeyError(f)


def _fa_end(b, f, X):
    frag = b.hdr(f.encode()) + b.post()
    if f == "end_no_nl":
        frag = frag[:-1]
    b.fill_to(X - len(frag) + 1)
    b.out += frag
    assert len(b.out) == X + 1


def fasta_text(name, family, W, combos, end, rng, t=0):
    b = _Fa(rng, W)
    b.out += b"\n\n"
    plants, k = [], 1
    cols = (0, W - 1, W // 2, 1, W - 2)
    for i, (f, unit, delta) in enumerate(combos):
        X = target(k, unit, delta, i, t)
        depth = TILE + 100 if i else (1000 if W < 1000 else 0)
        frag, idx = _fa_fragment(b, f, cols[i % 5], depth)
        b.fill_to(X - idx)
        b.out += frag
        plants.append(Plant(f, unit, delta, X, "width %d" % W))
        k = max(k + SPACING, -(-(len(b.out) + TILE + 2 * W + 400) // TILE))           # (room for the next plant's own lines)
    # the one long record: plain, regular tiles enough for a direct block
    b.out += b">" + b.ident() + b" one long record\n"
    B, s = len(b.out), b.bases(STRETCH).copy()
    k = B // TILE + 4
    for j, delta in enumerate((-2, -1, 0, 1, 2) * 2):
        f = "stretch_lower_first" if j < 5 else "stretch_lower_last"
        if (k * TILE + delta - B) % (W + 1) == W:                         # a line end lies there: the next seam
            k += 1
        X = k * TILE + delta
        i0 = (X - B) - (X - B) // (W + 1)                                  # the base at text offset X
        if j < 5:
            s[i0:i0 + 300] |= 0x20
        else:
            s[i0 - 299:i0 + 1] |= 0x20
        plants.append(Plant(f, TILE, delta, X, "width %d, in the long record" % W))
        k += 4 if j == 4 else 3                                           # (three tiles and more apart, whatever the deltas)
    assert i0 + 2 * TILE < STRETCH
    b.out += b.wrap(s)
    k = max(len(b.out) // TILE + 3, 288 * 1024 // TILE + 1)
    f, unit, delta = end
    X = target(k, unit, delta, len(combos), t)
    _fa_end(b, f, X)
    plants.append(Plant(f, unit, delta, X, "width %d" % W))
    return Text(name, "fasta", family, W, b.out, plants)


# ---- FASTQ -------------------------------------------------------------------------------------------------------------------------
class _Fq:
    def __init__(self, rng):
        self.out, self.rng, self.r, self.n_rec = bytearray(), rng, 100_000, 0
        self.run = int(rng.integers(1, 9))
        self.pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 300_000)]
        self.qpool = rng.integers(0x21, 0x7F, 300_000, dtype=np.uint8)
        self.at = self.qat = 0
        self.nseq = self.nids = self.ncmt = 0                                                    # what the streams hold so far

    def bases(self, n):
        if self.at + n > len(self.pool):
            self.at = 0
        self.at += n
        return self.pool[self.at - n:self.at].tobytes()

    def quals(self, n):
        if self.qat + n > len(self.qpool):
            self.qat = 0
        self.qat += n
        return self.qpool[self.qat - n:self.qat].tobytes()

    def parts(self, n=150, id_extra=b"", blank=b" ", cmt=None, plus=None, e=(b"\n", b"\n", b"\n", b"\n"), at=b"@"):
        """['@', ID, blank, comment, eol, bases, eol, '+' line, eol, qualities, eol] of the next record; every eleventh repeats its name."""
        self.r += 1
        ident = b"SRR%d.%d" % (self.run, self.r) + id_extra
        if cmt is None:
            cmt = b"%d:N:0:ACGT length=%d" % (1 + (self.r & 1), n)
        if plus is None:
            plus = b"+" + (ident + blank + cmt if self.r % 11 == 0 else b"")
        return [at, ident, blank, cmt, e[0], self.bases(n), e[1], plus, e[2], self.quals(n), e[3]]

    def emit(self, p):
        self.out += b"".join(p)
        self.n_rec += 1
        self.nseq += len(p[5]); self.nids += len(p[1]) + 1; self.ncmt += len(p[3]) + 1

    def fill_to(self, start):
        while start - len(self.out) > 760:
            self.emit(self.parts())
        p = self.parts(plus=b"+")
        c = start - len(self.out) - sum(len(x) for x in p)
        assert c >= 0, (start, len(self.out))
        if c:
            p[3] += b" " + b"x" * (c - 1)
        self.emit(p)
        assert len(self.out) == start

    def state(self):
        return (len(self.out), self.r, self.n_rec, self.at, self.qat, self.nseq, self.nids, self.ncmt)

    def restore(self, s):
        n, self.r, self.n_rec, self.at, self.qat, self.nseq, self.nids, self.ncmt = s
        del self.out[n:]


def _off(p, i):
    return sum(len(x) for x in p[:i])


def _set(s, i, c):
    return s[:i] + bytes([c]) + s[i + 1:]


def _fq_fragment(b, f, col, first):
    """(parts of the record, index of the defining byte).  first: the plant of tiles 0 / 1, where a long header has less room."""
    LF4 = [b"\n"] * 4
    piece = {"l0_first": 0, "l1_first": 5, "l2_first": 7, "l3_first": 9, "l0_nl": 4, "l1_nl": 6, "l2_nl": 8, "l3_nl": 10, "id_space": 2}
    if f in piece:
        p = b.parts()
        return p, _off(p, piece[f])
    if f == "id_tab":
        p = b.parts(blank=b"\t")
        return p, _off(p, 2)
    if f == "no_comment":
        p = b.parts(blank=b"", cmt=b"")
        return p, _off(p, 4)
    if f == "long_hdr_first":
        p = b.parts(cmt=b"1:N:0:ACGT " + b.quals(2 * TILE + 200).replace(b"\t", b"_"))
        return p, 0
    if f == "long_hdr_blank":
        n = 3000 if first else 2 * TILE + 200
        p = b.parts(id_extra=b"_" + b.bases(n), cmt=b"2:N:0:ACGT " + b.quals(TILE + 200 if first else 40))
        return p, _off(p, 2)
    if f in ("qual_at", "qual_plus"):
        p = b.parts(plus=b"+")
        p[9] = _set(p[9], 0, ord("@") if f == "qual_at" else ord("+"))
        return p, _off(p, 9)
    if f == "plus_name":
        p = b.parts()
        p[7] = b"+" + p[1] + p[2] + p[3]
        return p, _off(p, 7) + len(p[7]) // 2
    if f == "blank":
        p = b.parts(e=(b"\n", b"\n", b"\n", b"\n\n"))
        return p, _off(p, 10) + 1
    if f == "crlf":
        p = b.parts(e=(b"\n", b"\r\n", b"\r\n", b"\r\n"))
        return p, _off(p, 6)
    if f == "space_seq":
        p = b.parts()
        p[5] = p[5][:col] + b" " + p[5][col:]
        return p, _off(p, 5) + col
    if f in ("bad_z", "iupac"):
        p = b.parts()
        p[5] = _set(p[5], col, ord("z") if f == "bad_z" else ord("R"))
        return p, _off(p, 5) + col
    if f in ("q01", "q7f", "q80"):
        p = b.parts()
        p[9] = _set(p[9], col, {"q01": 0x01, "q7f": 0x7F, "q80": 0x80}[f])
        return p, _off(p, 9) + col
    if f == "h01":
        p = b.parts()
        p[3] += b"\x01"
        return p, _off(p, 4) - 1
    if f == "tab2":
        p = b.parts(blank=b"\t", cmt=b"1:N:0:ACGT\tlength=150")
        return p, _off(p, 3) + 10
    raise KeyError(f)


def _fq_end(b, f, X):
    p = b.parts(plus=b"+")
    if f == "end_no_nl":
        p[10] = b""
    b.fill_to(X - sum(len(x) for x in p) + 1)
    b.emit(p)
    assert len(b.out) == X + 1


def fastq_text(name, family, combos, end, rng, t=0):
    b = _Fq(rng)
    b.out += b"\n\n"
    plants, k = [], 1
    cols = (1, 149, 75, 2, 148)
    for i, (f, unit, delta) in enumerate(combos):
        X = target(k, unit, delta, i, t)
        p, idx = _fq_fragment(b, f, cols[i % 5], i == 0)
        b.fill_to(X - idx)
        b.emit(p)
        plants.append(Plant(f, unit, delta, X))
        k += SPACING + (3 if f.startswith("long_hdr") else 0)
    k = max(k, 96 * 1024 // TILE + 1)
    f, unit, delta = end
    X = target(k, unit, delta, len(combos), t)
    _fq_end(b, f, X)
    plants.append(Plant(f, unit, delta, X))
    return Text(name, "fastq", family, 0, b.out, plants)


def _short_tile(b, c):
    """4096 bytes of short reads that begin a record and hold exactly c line ends, the last byte one of them; and the lines that
    complete the last record behind them."""
    nrec, part = divmod(c, 4)
    s = (4 * TILE // c - 9) // 2                                    # bases of a read: a record of '@ab', s, '+', s is 2 s + 8 bytes
    n_hdr = nrec + (1 if part else 0)
    fixed = nrec * (2 * s + 5) + ((1 if part >= 1 else 0) + (s + 1 if part >= 2 else 0) + (2 if part >= 3 else 0))
    room = TILE - fixed                                            # the bytes of the headers behind their '@'... and with it
    assert room >= 3 * n_hdr, (c, s, room)
    lens = [room // n_hdr + (1 if j < room % n_hdr else 0) for j in range(n_hdr)]
    tile, tail = bytearray(), b""
    for j in range(n_hdr):
        name = (b"@r%d" % (j + 1)).ljust(lens[j], b"x")[:lens[j]]
        seq, qual = b.bases(s), b.quals(s)
        lines = [name + b"\n", seq + b"\n", b"+\n", qual + b"\n"]
        take = 4 if j < nrec else part
        tile += b"".join(lines[:take]); tail = b"".join(lines[take:])
        b.n_rec += 1
    assert len(tile) == TILE and tile.count(b"\n") == c and tile[-1] == 10, (c, len(tile), tile.count(b"\n"))
    return bytes(tile), tail


def segment_text(c, rng):
    b = _Fq(rng)
    b.out += b"\n\n"
    k = 8
    b.fill_to(k * TILE)
    tile, tail = _short_tile(b, c)
    b.out += tile + tail
    b.fill_to(24 * TILE + 77)
    b.emit(b.parts())
    return Text("fq_segments_%d" % c, "fastq", "segments", 0, b.out, [Plant("nl%d" % c, TILE, 0, k * TILE, "%d line ends in the tile" % c)], info={"tile": k, "count": c})


def alignment_texts(rng_of):
    """The read in front of a tile seam lengthened by 0 .. 15 bases ('seq': the tile's offset in the sequence and quality streams takes
    residue j mod 16) or its name by 0 .. 15 bytes ('ids', and 'cmt': the comment stream's offset, which the name's length moves
    against the text).  The record behind the seam begins on it, so the offsets are the streams' lengths of the text in front."""
    jobs = [(kind, j) for kind in ("seq", "ids", "cmt") for j in range(16)]
    out = []
    for t, chunk in enumerate(_chunks(jobs, 12)):
        b = _Fq(rng_of(t))
        b.out += b"\n\n"
        plants, k = [], 2
        for kind, j in chunk:
            X = k * TILE
            s0 = b.state()
            for e in range(17):
                assert e < 16, (kind, j)
                b.restore(s0)
                p = b.parts(n=150 + e, plus=b"+") if kind == "seq" else b.parts(id_extra=b"x" * e, plus=b"+")
                b.fill_to(X - sum(len(x) for x in p))
                b.emit(p)
                if {"seq": b.nseq, "ids": b.nids, "cmt": b.ncmt}[kind] % 16 == j:
                    break
            plants.append(Plant("align_" + kind, TILE, 0, X, "residue %d, lengthened by %d" % (j, e)))
            k += SPACING
        b.fill_to(max(k, 25) * TILE + 33)
        b.emit(b.parts())
        out.append(Text("fq_alignment_%d" % t, "fastq", "alignment", 0, b.out, plants, info={"jobs": chunk}))
    return out


def dying_text(cause, delta, rng):
    b = _Fq(rng)
    b.out += b"\n\n"
    cut = cause.startswith("cut")
    X = (24 if cut else 12) * TILE + delta
    if cause in ("q_short", "q_long"):
        p = b.parts(plus=b"+")
        p[9] = p[9][:-1] if cause == "q_short" else p[9] + b"I"
        idx = _off(p, 10)
    elif cause == "no_plus":
        p = b.parts(plus=b"", e=(b"\n", b"\n", b"", b"\n"))
        p[9] = _set(p[9], 0, ord("I"))
        idx = _off(p, 9)
    elif cause == "no_at":
        p = b.parts(at=b"")
        idx = 0
    elif cause == "cut_hdr":
        p = b.parts()[:2]
        idx = _off(p, 2) - 1
    elif cause == "cut_seq":
        p = b.parts()[:7]
        idx = _off(p, 7) - 1
    else:
        p = b.parts(plus=b"+")[:9]
        idx = _off(p, 9) - 1
    b.fill_to(X - idx)
    n = b.n_rec + 1                                                 # the damaged record's number
    b.out += b"".join(p)
    if not cut:
        b.fill_to(25 * TILE + 5)
        b.emit(b.parts())
    msg = DYING[cause]
    if "%d" in msg:
        msg = msg % (n - 1 if cause == "no_at" else n)
    return Text("fq_die_%s_%+d" % (cause, delta), "fastq", "dying", 0, b.out, [Plant(cause, TILE, delta, X)], dies=msg)


# ---- all of them -------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def texts(seed=0):
    """Every planned text under `seed` (NAF_TEST_SEED is added to it)."""
    if seed in _CACHE:
        return _CACHE[seed]
    base = [7000]

    def rng():
        base[0] += 1
        return np.random.default_rng(base[0] * 1000 + seed + SEED)

    out = []
    ends = [(f, u, d) for f in END_FEATURES for (u, d) in ANCHORS]
    t = 0
    for fam, feats in FASTA_FAMILIES.items():
        for i, combos in enumerate(_deal(feats)):
            W = WIDTHS[t % len(WIDTHS)]
            out.append(fasta_text("fa_%s_w%d_%d" % (fam, W, i), fam, W, combos, ends[t % len(ends)], rng(), t))
            t += 1
    assert t >= len(ends)
    t = 0
    for fam, feats in FASTQ_FAMILIES.items():
        for i, combos in enumerate(_deal(feats)):
            out.append(fastq_text("fq_%s_%d" % (fam, i), fam, combos, ends[t % len(ends)], rng(), t))
            t += 1
    assert t >= len(ends)
    for c in SEGMENT_COUNTS:
        out.append(segment_text(c, rng()))
    out += alignment_texts(lambda t: rng())
    for cause in DYING:
        for d in DYING_DELTAS:
            out.append(dying_text(cause, d, rng()))
    _CACHE[seed] = out
    return out


def names():
    return [t.name for t in texts(0)]


def cross_product():
    """{(kind, feature, unit, delta): times planted} over texts(0), every cell of the cross product present (zero where it is not)."""
    want = {}
    for kind, fams in (("fasta", FASTA_FAMILIES), ("fastq", FASTQ_FAMILIES)):
        for f in [f for fs in fams.values() for f in fs] + list(END_FEATURES):
            for (u, d) in ANCHORS:
                want[(kind, f, u, d)] = 0
    for t in texts(0):
        for p in t.plants:
            key = (t.kind, p.feature, p.unit, p.delta)
            if key in want:
                want[key] += 1
    return want
