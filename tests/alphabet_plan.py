"""Texts and models for the encoder's alphabet, damaged-ID and --strict tests (tests/test_gpu_alphabets.py, tests/test_alphabets_cpu.py):
the plan of tests/seam_plan.py carried over to what it left out.  Part A plants the features of the 8-bit alphabets (protein, text) and a
damaged byte in an ID (every alphabet) at the seam phases of seam_plan.ANCHORS; part B builds texts for --strict: one FIRST offender F at
an anchor with weaker decoys behind it, many headers in front of F, and a FASTQ's strict byte beside each structural death.  Nothing
here touches the GPU or the code under test, and nothing is imported from it.

The models are a plain walk in input order (walk): what the split keeps of a text, the four histograms of unexpected bytes, and where
the reference would stop -- at the first unexpected byte under --strict, or at the structural error in front of it.  decoded(),
unexpected() and strict_verdict() are read off that walk.  The rules, from the reference's reader:
  * a line ends at LF, VT, FF or CR; blanks are those and TAB and space.  Leading blanks in front of the first marker are skipped.
  * an ID ends at the first blank.  A byte below 0x21, 0x7F or 0xFF in it (and '>' in a text FASTA) is counted, DROPPED from the ID,
    and a '?' goes into the sequence stream in front of the record's own letters, where no length accounts for it: the records come
    back cut out of that stream by their lengths (shifted by the strays in front), a FASTA prints what is left behind the last record
    wrapped on from the last record's line, a FASTQ drops it.
  * a comment runs to the line end; a byte below 0x20 (TAB too), 0x7F or 0xFF in it is counted and comes back as '?'.
  * sequence lines: blanks are dropped, a byte the alphabet does not hold is counted and replaced (N / X / ?).  A '>' first on a line
    starts a record; elsewhere it is data in a text and unexpected otherwise.
  * FASTQ: four lines, blank lines between them skipped; the first byte of a quality line is kept whatever it is, the others must be
    0x21 .. 0x7E or are counted and replaced by '!'.
Structure never depends on the random numbers: letters, names and qualities come from np.random.default_rng(base + seed)."""
import re

import numpy as np

import seam_plan as P
from seam_plan import ANCHORS, LANE, PIECE, SPACING, TILE, Plant, Text, _deal, _Fa, _fa_end, _fa_fragment, _Fq, _fq_end, _fq_fragment, _off, _set, target

DNA, RNA, PROTEIN, TEXT = 0, 1, 2, 3
TYPE_NAME = ("DNA", "RNA", "protein", "text")
TYPE_TAG = ("dna", "rna", "protein", "text")
AMINO = b"ACDEFGHIKLMNPQRSTVWY"
PRINTABLE = bytes(c for c in range(0x21, 0x7F) if c != 0x3E)
LETTERS = (b"ACGT", b"ACGU", AMINO, PRINTABLE)
REPLACEMENT = (b"N", b"N", b"X", b"?")
WIDTHS = P.WIDTHS
IMPOSSIBLE = []                    # (alphabet, kind, family, feature, unit, delta, reason): tests/test_alphabets_cpu.py caps the list

_COMMON_FA = ("gt", "hdr_nl", "id_space", "id_tab", "hdr_1byte", "blank", "crlf", "cr", "space", "tab", "short_nl", "long_nl", "odd_last")
FEATURES = {
    ("fasta", PROTEIN): _COMMON_FA + ("star", "dash", "lower1", "digit", "bang", "hi80", "ctl01"),
    ("fasta", TEXT): _COMMON_FA + ("gt_mid", "gt_line", "gt_in_id", "bang", "hi80", "hiFE", "del7F", "hiFF", "ctl01"),
    ("fastq", PROTEIN): ("l0_first", "l1_first", "l2_first", "l3_first", "l0_nl", "l1_nl", "l2_nl", "l3_nl", "qual_at", "qual_plus", "plus_name",
                         "bad_seq", "q01", "q7f", "q80", "blank", "crlf", "space_seq"),
}
FEATURES[("fastq", TEXT)] = FEATURES[("fastq", PROTEIN)]
ID_FEATURES = tuple("id_%s_%s" % (b, w) for b in ("ctl", "7f", "ff") for w in ("first", "mid", "last"))
ID_BYTE = {"ctl": 0x01, "7f": 0x7F, "ff": 0xFF}
END_FEATURES = P.END_FEATURES
# the byte a letter feature puts into a sequence line
LETTER = {"star": 0x2A, "digit": 0x37, "hi80": 0x80, "hiFE": 0xFE, "del7F": 0x7F, "hiFF": 0xFF, "ctl01": 0x01, "gt_mid": 0x3E}
BAD_SEQ = {PROTEIN: 0x37, TEXT: 0x7F}


class AText(Text):
    """A seam_plan.Text of one alphabet (seq_type).  info['first']: the offset of a strict text's FIRST offender, info['what']: its kind."""

    def __init__(self, name, kind, family, width, data, plants, seq_type, info=None):
        Text.__init__(self, name, kind, family, width, data, plants, None, info)
        self.seq_type = seq_type

    def decoded(self):
        return decoded(self.data, self.seq_type)


# ---- the model: one walk in input order ----------------------------------------------------------------------------------------------
_EOL = re.compile(b"[\n\x0b\x0c\r]")
_EOLS = b"\n\x0b\x0c\r"
_BLANK = re.compile(b"[\t ]")
_BAD_ID = re.compile(b"[\x00-\x08\x0e-\x1f\x7f\xff]")
_BAD_ID_GT = re.compile(b"[\x00-\x08\x0e-\x1f\x7f\xff>]")
_BAD_CMT = re.compile(b"[\x00-\x1f\x7f\xff]")
_BAD_QUAL = re.compile(b"[^\x21-\x7e\t ]")
_EXPECTED = (b"ABCDGHKMNRSTVWYabcdghkmnrstvwy-", b"ABCDGHKMNRSUVWYabcdghkmnrsuvwy-",
             bytes(range(0x41, 0x5B)) + bytes(range(0x61, 0x7B)) + b"*-", bytes(c for c in range(0x21, 0xFF) if c != 0x7F))


def _seq_rules(seq_type):
    """(regex of the bytes counted in a sequence line, translation of a line to what is kept of it)."""
    ok = set(_EXPECTED[seq_type])
    bad = bytes(c for c in range(256) if c not in ok and c not in b"\t \n\x0b\x0c\r")
    table = bytes(c if c in ok else REPLACEMENT[seq_type][0] for c in range(256))
    return re.compile(b"[" + re.escape(bad) + b"]"), table


class Stop(Exception):
    """Where the reference stops reading: its message (without 'ennaf error: ' and the line end)."""


class Walk:
    """ids, comments (as stored), lengths, stream (every kept sequence byte, the strays of damaged IDs included), quals, longest line,
    hist: {'id', 'comment', 'seq', 'qual'} -> 257 counts, fmt, stop: the message the walk ended with (None: it read the whole text)."""

    def __init__(self, data, seq_type, strict=False):
        self.data, self.seq_type, self.strict = bytes(data), seq_type, strict
        self.ids, self.cmts, self.lengths, self.quals, self.stream = [], [], [], [], bytearray()
        self.hist = {k: [0] * 257 for k in ("id", "comment", "seq", "qual")}
        self.longest, self.n, self.fmt, self.stop = 0, 0, None, None
        try:
            self._run()
        except Stop as e:
            self.stop = str(e)

    def _bad(self, kind, c):
        if self.strict:
            what = {"id": "character '%c' in ID of", "comment": "character '%c' in comment of", "seq": TYPE_NAME[self.seq_type] + " code '%c' in",
                    "qual": "quality code '%c' in"}[kind]
            raise Stop("unexpected " + what % c + " sequence %d" % (self.n + 1))
        self.hist[kind][c] += 1

    def _line(self, pos):
        m = _EOL.search(self.data, pos)
        return (self.data[pos:m.start()], m.start() + 1, True) if m else (self.data[pos:], len(self.data), False)

    def _skip(self, pos):
        d, n = self.data, len(self.data)
        while pos < n and d[pos] in _EOLS:
            pos += 1
        return pos

    def _header(self, line):
        m = _BLANK.search(line)
        ident, cmt = (line[:m.start()], line[m.end():]) if m else (line, b"")
        bad_id = _BAD_ID_GT if (self.seq_type == TEXT and self.fmt == "fasta") else _BAD_ID
        for x in bad_id.finditer(ident):
            self._bad("id", x.group()[0])
            self.stream += b"?"
        for x in _BAD_CMT.finditer(cmt):
            self._bad("comment", x.group()[0])
        self.ids.append(bad_id.sub(b"", ident)); self.cmts.append(_BAD_CMT.sub(b"?", cmt))

    def _seq_line(self, line):
        for x in self.bad_seq.finditer(line):
            self._bad("seq", x.group()[0])
        kept = line.translate(self.table, b"\t ")
        self.stream += kept
        self.longest = max(self.longest, len(kept))
        return len(kept)

    def _run(self):
        d, n = self.data, len(self.data)
        pos, last = 0, 10
        while pos < n and d[pos] in b"\t \n\x0b\x0c\r":
            last = d[pos]; pos += 1
        if pos == n:
            return
        if d[pos] not in b">@" or last not in _EOLS:
            raise Stop("input is neither FASTA nor FASTQ")                                       # (no text of the plan)
        self.fmt = "fasta" if d[pos] == 0x3E else "fastq"
        self.bad_seq, self.table = _seq_rules(self.seq_type)
        pos += 1
        if self.fmt == "fasta":
            while True:
                line, pos, more = self._line(pos)
                self._header(line)
                start = len(self.stream)
                if more and d[pos:pos + 1] == b">":
                    pos += 1                                                                     # an empty record
                elif more:
                    while True:
                        line, pos, more = self._line(pos)
                        self._seq_line(line)
                        pos = self._skip(pos)
                        more = more and pos < n
                        if not more or d[pos] == 0x3E:
                            pos += 1
                            break
                self.lengths.append(len(self.stream) - start); self.n += 1
                if not more:
                    return
        while True:
            line, pos, more = self._line(pos)
            self._header(line)
            if not more: raise Stop("truncated FASTQ input: last sequence has no sequence data")
            line, pos, more = self._line(pos)
            read = self._seq_line(line)
            pos = self._skip(pos)
            if not more or pos >= n: raise Stop("truncated FASTQ input: last sequence has no quality")
            if d[pos] != 0x2B: raise Stop("invalid FASTQ input: can't find '+' line of sequence %d" % (self.n + 1))
            line, pos, more = self._line(pos)
            pos = self._skip(pos)
            if not more or pos >= n: raise Stop("truncated FASTQ input: last sequence has no quality")
            line, pos, more = self._line(pos)
            for x in _BAD_QUAL.finditer(line, 1):                                                # the first byte is kept whatever it is
                self._bad("qual", x.group()[0])
            q = line[:1] + _BAD_QUAL.sub(b"!", line[1:]).translate(None, b"\t ")
            if len(q) != read: raise Stop("quality length of sequence %d (%d) doesn't match sequence length (%d)" % (self.n + 1, len(q), read))
            self.quals.append(q); self.lengths.append(read); self.n += 1
            pos = self._skip(pos)
            if pos >= n:
                return
            if d[pos] != 0x40: raise Stop("invalid FASTQ input: Can't find '@' after sequence %d" % self.n)
            pos += 1


_WALKS = {}


def walk(data, seq_type=DNA, strict=False):
    key = (bytes(data), seq_type, strict)
    if key not in _WALKS:
        if len(_WALKS) > 32:
            _WALKS.clear()
        _WALKS[key] = Walk(data, seq_type, strict)
    return _WALKS[key]


def _name(ident, cmt):
    return ident + (b" " + cmt if cmt else b"")


def decoded(data, seq_type=DNA, no_mask=False):
    """The text an archive of `data` gives back (the default view of unnaf).  no_mask: an 8-bit stream is stored in upper case."""
    w = walk(data, seq_type)
    assert w.stop is None, w.stop
    s = bytes(w.stream)
    if no_mask and seq_type >= PROTEIN:
        s = s.upper()
    if seq_type <= RNA:                                                  # 4-bit codes: what is no code is an N, the case bit is the letter's
        s = re.sub(b"[^A-Za-z-]", b"N", s)
    out, at, L = [], 0, w.longest
    if w.fmt == "fastq":
        for ident, cmt, n, q in zip(w.ids, w.cmts, w.lengths, w.quals):
            out.append(b"@" + _name(ident, cmt) + b"\n" + (s[at:at + n].upper() if seq_type <= RNA else s[at:at + n]) + b"\n+\n" + q + b"\n")
            at += n
        return b"".join(out)
    room = L                                                             # what the current line still takes
    for ident, cmt, n in zip(w.ids, w.cmts, w.lengths):
        out.append(b">" + _name(ident, cmt) + b"\n")
        if n:
            r = s[at:at + n]
            out.append(b"".join(r[i:i + L] + b"\n" for i in range(0, n, L)))
            room = L - (n % L or L)
            at += n
    rest = s[at:]
    if rest and any(w.lengths):                                          # the strays of damaged IDs: wrapped on from the last record's line
        lines = [rest[:room]] + [rest[i:i + L] for i in range(room, len(rest), L)]
        out.append(b"\n".join(lines))
    return b"".join(out)


def unexpected(data, seq_type=DNA):
    """{'id', 'comment', 'seq', 'qual'} -> the 257 counts of the report."""
    w = walk(data, seq_type)
    assert w.stop is None, w.stop
    return w.hist


def strict_verdict(data, seq_type=DNA, fmt=None):
    """None, or the message the reference stops with under --strict: the first unexpected byte or the structural error in front of it."""
    w = walk(data, seq_type, True)
    assert fmt is None or w.fmt == fmt
    return w.stop


def said(text):
    """The message of a refusal as the binding words it ('naf_gpu error N: message', a line end behind it), without both."""
    return text.split(": ", 1)[1].rstrip("\n")


def same_verdict(t, got, verdict, what=""):
    if got != verdict:
        raise AssertionError("%s%s: refused with %r, the model says %r; plants: %s" % (t.name, what and " under " + what, got, verdict, t.plants))


def same_histograms(t, got, want):
    """The report's four histograms are the plan's: which count differs, and the plants."""
    for key in ("id", "comment", "seq", "qual"):
        if list(got[key]) != list(want[key]):
            d = [(i, a, b) for i, (a, b) in enumerate(zip(got[key], want[key])) if a != b]
            raise AssertionError("%s: unexpected %s bytes (byte, reported, planned) %s; plants: %s" % (t.name, key, d[:8], t.plants))


def report(hist, seq_type):
    """The reference's report of unexpected characters on stderr (without --strict)."""
    out = []
    for key, name in (("id", "id"), ("comment", "comment"), ("seq", TYPE_NAME[seq_type]), ("qual", "quality")):
        n = hist[key]
        if sum(n):
            out.append("input has %d unexpected %s characters:\n" % (sum(n), name))
            out += ["    '\\x%02X': %d\n" % (i, n[i]) if (i < 32 or i >= 127) else "    '%c': %d\n" % (i, n[i]) for i in list(range(32)) + list(range(32, 127)) + list(range(127, 256)) if n[i]]
    return "".join(out)


# ---- builders of one alphabet --------------------------------------------------------------------------------------------------------
class _Fa8(_Fa):
    def __init__(self, rng, W, seq_type):
        _Fa.__init__(self, rng, W)
        a = np.frombuffer(LETTERS[seq_type], dtype=np.uint8)
        self.pool = a[rng.integers(0, len(a), 300_000)]


class _Fq8(_Fq):
    def __init__(self, rng, seq_type):
        _Fq.__init__(self, rng)
        a = np.frombuffer(LETTERS[seq_type], dtype=np.uint8)
        self.pool = a[rng.integers(0, len(a), 300_000)]


def _fa8_fragment(b, f, col, depth):
    """seam_plan._fa_fragment and the features of the 8-bit alphabets."""
    if f in LETTER:
        h, p, line = b.hdr(f.encode()), b.pre(depth), bytearray(bytes(b.bases(b.W)))
        col = max(col, 1) if f == "gt_mid" else col
        line[col] = LETTER[f]
        return h + p + bytes(line) + b"\n" + b.post(), len(h) + len(p) + col
    if f == "gt_line":                                                   # behind whole lines, not behind a header as `gt` is
        h, p = b.hdr(b"gt_line"), b.pre(depth)
        return h + p + b.hdr(b"begins here") + b.post(), len(h) + len(p)
    if f == "gt_in_id":
        i = b.ident()
        return b">" + i[:4] + b">" + i[4:] + b" gt_in_id\n" + b.post(), 5
    if f in ID_FEATURES:
        _, byte, where = f.split("_")
        i = b.ident()
        at = {"first": 0, "mid": 4, "last": 8}[where]
        return b">" + _set(i, at, ID_BYTE[byte]) + b" cmt\x01ctl " + f.encode() + b"\n" + b.post(), 1 + at
    return _fa_fragment(b, f, col, depth)


def _fq8_fragment(b, f, col, first, seq_type):
    if f == "bad_seq":
        p = b.parts()
        p[5] = _set(p[5], col, BAD_SEQ[seq_type])
        return p, _off(p, 5) + col
    if f in ID_FEATURES:
        _, byte, where = f.split("_")
        p = b.parts()
        at = {"first": 0, "mid": len(p[1]) // 2, "last": len(p[1]) - 1}[where]
        p[1] = _set(p[1], at, ID_BYTE[byte]); p[3] = b"cmt\x01ctl " + p[3]
        return p, 1 + at
    return _fq_fragment(b, f, col, first)


def fasta_text(name, family, W, combos, end, rng, seq_type, t=0, lead=b"\n\n"):
    """seam_plan.fasta_text without the long record: an 8-bit stream has no direct block."""
    b = _Fa8(rng, W, seq_type)
    b.out += lead
    plants, k = [], 1
    cols = (0, W - 1, W // 2, 1, W - 2)
    for i, (f, unit, delta) in enumerate(combos):
        X = target(k, unit, delta, i, t)
        depth = TILE + 100 if i else (1000 if W < 1000 else 0)
        frag, idx = _fa8_fragment(b, f, cols[i % 5], depth)
        b.fill_to(X - idx)
        b.out += frag
        plants.append(Plant(f, unit, delta, X, "width %d" % W))
        k = max(k + SPACING, -(-(len(b.out) + TILE + 2 * W + 400) // TILE))
    f, unit, delta = end
    if seq_type <= RNA:
        # 4-bit: one long record of plain, regular tiles (room for a direct block) and 288 KiB in all, the floor of the one pass
        # (k_enc_fused) under NAF_GPU_DIRECT=2
        b.out += b">" + b.ident() + b" one long record\n" + b.lines(P.STRETCH)
        k = max(len(b.out) // TILE + 3, ONE_PASS_TILES)
    X = target(k, unit, delta, len(combos), t)
    _fa_end(b, f, X)
    plants.append(Plant(f, unit, delta, X, "width %d" % W))
    return AText(name, "fasta", family, W, b.out, plants, seq_type)


def fastq_text(name, family, combos, end, rng, seq_type, t=0):
    b = _Fq8(rng, seq_type)
    b.out += b"\n\n"
    plants, k = [], 1
    cols = (1, 149, 75, 2, 148)
    for i, (f, unit, delta) in enumerate(combos):
        X = target(k, unit, delta, i, t)
        p, idx = _fq8_fragment(b, f, cols[i % 5], i == 0, seq_type)
        b.fill_to(X - idx)
        b.emit(p)
        plants.append(Plant(f, unit, delta, X))
        k += SPACING
    f, unit, delta = end
    X = target(max(k, 17), unit, delta, len(combos), t)
    _fq_end(b, f, X)
    plants.append(Plant(f, unit, delta, X))
    return AText(name, "fastq", family, 0, b.out, plants, seq_type)


# ---- B: --strict -----------------------------------------------------------------------------------------------------------------------
STRICT_KINDS = {"fasta": ("id", "comment", "seq"), "fastq": ("id", "comment", "seq", "qual")}
# (the FIRST offender, its decoys in the same line): a decoy is the smaller byte
F_SEQ = {DNA: (0x7E, 0x21), RNA: (0x7E, 0x21), PROTEIN: (0x7E, 0x21), TEXT: (0xFF, 0x7F)}
NEAR = (1, PIECE, LANE)                                                  # decoys at F + 1, in the next piece, in the next lane
ONE_PASS_TILES = 288 * 1024 // TILE + 1                                   # a 4-bit FASTA of this size is read once under NAF_GPU_DIRECT=2
F_AT = 5                                                                 # the tile seam of F: tiles in front of it are plain


def _hurt(s, at, first, decoy):
    s = _set(s, at, first)
    for d in NEAR:
        s = _set(s, at + d, decoy)
    return s


def _decoy_header(b, kind, seam):
    """A header whose ID holds 0x01 at -1, 0 and +1 of `seam`: kind 0 and the smallest byte there is."""
    if kind == "fasta":
        i = b.ident()
        b.fill_to(seam - 1 - 4)
        b.out += b">" + i[:3] + b"\x01\x01\x01" + i[6:] + b" decoy\n" + b.post()
    else:
        p = b.parts()
        p[1] = p[1][:3] + b"\x01\x01\x01" + p[1][6:]
        b.fill_to(seam - 1 - 4)
        b.emit(p)


def strict_text(kind, seq_type, what, unit, delta, rng, t=0):
    """One FIRST offender F (`what`: id / comment / seq / qual / gt_in_id / seq_iupac) at the anchor of tile seam F_AT, and decoys behind
    it, each of a smaller byte value: at F + 1, in the next piece and the next lane (F's own line, so F's own kind, whatever F is), and
    at -1, 0 and +1 of the next tile seam that leaves room and 20 tiles on (bytes of an ID: kind 0, smaller than F's unless F is an ID
    byte).  A 4-bit FASTA is 288 KiB long: the one pass reads it under NAF_GPU_DIRECT=2."""
    X = target(F_AT, unit, delta, 3, t)
    if kind == "fasta":
        b = _Fa8(rng, 80, seq_type)
        b.out += b"\n\n"
        i, c = b.ident() + b"x" * 100, b"c" * 120
        if what == "id": i = _hurt(i, 3, 0xFF, 0x01)
        if what == "gt_in_id": i = _hurt(i, 3, 0x3E, 0x01)
        if what == "comment": c = _hurt(c, 3, 0xFF, 0x01)
        h = b">" + i + b" " + c + b"\n"
        if what == "seq":
            p, line = b.pre(TILE + 100), bytes(b.bases(80))
            frag, idx = h + p + _hurt(line, 3, *F_SEQ[seq_type]) + b"\n" + b.post(), len(h) + len(p) + 3
        else:
            frag, idx = h + b.post(), (1 if what != "comment" else 2 + len(i)) + 3
        b.fill_to(X - idx)
        b.out += frag
    else:
        b = _Fq8(rng, seq_type)
        b.out += b"\n\n"
        p = b.parts(id_extra=b"x" * 100, cmt=b"c" * 120)
        part = {"id": 1, "comment": 3, "seq": 5, "seq_iupac": 5, "qual": 9}[what]
        first, decoy = F_SEQ[seq_type] if what == "seq" else (0x21, 0x01) if what == "seq_iupac" else (0xFF, 0x01)
        p[part] = _hurt(p[part], 3, first, decoy)
        idx = _off(p, part) + 3
        if what == "seq_iupac":                                           # an R two reads in front: the tile is regular and handed back
            q, r = b.parts(), b.parts()
            q[5] = _set(q[5], 70, ord("R"))
            b.fill_to(X - idx - sum(len(x) for x in q + r))
            b.emit(q); b.emit(r)
        else:
            b.fill_to(X - idx)
        b.emit(p)
    k2 = (len(b.out) + 1300) // TILE + 1
    _decoy_header(b, kind, k2 * TILE)
    _decoy_header(b, kind, (F_AT + 20) * TILE)
    end = (ONE_PASS_TILES if kind == "fasta" and seq_type <= RNA else F_AT + 22) * TILE + 77
    if kind == "fasta":
        _fa_end(b, "end_nl", end)
    else:
        _fq_end(b, "end_nl", end)
    name = "%s_%s_strict_%s_%d%+d" % ("fa" if kind == "fasta" else "fq", TYPE_TAG[seq_type], what, unit, delta)
    plants = [Plant("F_" + what, unit, delta, X)] + [Plant("decoy", unit, delta, X + d, "beside F") for d in NEAR] + \
             [Plant("decoy", TILE, d, k2 * TILE + d) for d in (-1, 0, 1)] + [Plant("decoy", TILE, d, (F_AT + 20) * TILE + d) for d in (-1, 0, 1)]
    return AText(name, kind, "strict", 80 if kind == "fasta" else 0, b.out, plants, seq_type, info={"what": what, "first": X})


BLOCK = 65536                                                            # text bytes per block of the header count


def numbered_text(kind, seq_type, blocks, delta, lead, rng):
    """Short records -- 300 headers and more in every 64 KiB -- in front of one offender F with F - p0 = blocks * 65536 + delta (p0: the
    first marker, behind `lead`).  FASTA: records of 91 bytes (coprime to 256: a header's '>' takes every residue of the count's
    256-byte stride).  FASTQ: every 7th record has a blank line behind it, every 5th ends its lines in CR LF (but the header's: the reference
    reads the LF behind a header's CR as an empty read).  F is a sequence letter."""
    a = np.frombuffer(LETTERS[seq_type], dtype=np.uint8)
    pool = a[rng.integers(0, len(a), 1 << 16)].tobytes()
    qpool = rng.integers(0x21, 0x7F, 1 << 16, dtype=np.uint8).tobytes()
    out, r, X = bytearray(lead), 0, len(lead) + blocks * BLOCK + delta
    first, _ = F_SEQ[seq_type]

    def rec(pad=0, hurt=None):
        nonlocal r
        r += 1
        s = pool[(41 * r) % 60000:][:40]
        if hurt is not None:
            s = _set(s, hurt, first)
        name = b"r%06d" % r + (b" " + b"p" * (pad - 1) if pad else b"")
        if kind == "fasta":
            return b">" + name + b"\n" + s + b"\n" + pool[(43 * r) % 60000:][:40] + b"\n"
        e = b"\r\n" if r % 5 == 0 and hurt is None else b"\n"
        return b"@" + name + b"\n" + s + e + b"+" + e + qpool[(47 * r) % 60000:][:40] + e + (b"\n" if r % 7 == 0 and hurt is None else b"")

    S = X - 12                                                            # where the offender's record begins: marker, name, line end, 3 letters
    while S - len(out) >= 200:
        out += rec()
    one = rec()
    r -= 1
    pad = S - len(out) - len(one)
    assert pad >= 0, (kind, blocks, delta, pad)
    out += rec(pad)
    assert len(out) == S
    out += rec(hurt=3)
    assert out[X] == first, (kind, blocks, delta, out[X - 12:X + 4])
    for _ in range(4):
        out += rec()
    name = "%s_%s_numbered_%d%+d_lead%d" % ("fa" if kind == "fasta" else "fq", TYPE_TAG[seq_type], blocks, delta, len(lead))
    return AText(name, kind, "numbered", 40, out, [Plant("F_seq", BLOCK, delta, X)], seq_type, info={"what": "seq", "first": X, "p0": len(lead)})


BIG = (64 << 20) + 70 * 1024


def big_text(seed=0):
    """64 MiB + 70 KiB of short records by tiling and one offender behind them: the header count's clamp at 1024 blocks.  Returns the
    text and the message, the record's number from a numpy count of the headers."""
    rng = np.random.default_rng(7777 + seed + P.SEED)
    unit = np.frombuffer(b"".join(b">u%05d\n" % i + np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 84)].tobytes() + b"\n" for i in range(4096)), dtype=np.uint8)
    a = np.concatenate([np.frombuffer(b"\n\n", dtype=np.uint8), np.tile(unit, -(-BIG // len(unit))), np.frombuffer(b">last one\nACGTAC!TAC\nAC\x01GT\n>z\x01 \x01\nAC\n", dtype=np.uint8)])
    n = int(np.count_nonzero((a[1:] == 0x3E) & (a[:-1] == 0x0A))) - 1                             # headers in front of the '!': all but '>z'
    return a.tobytes(), "unexpected DNA code '!' in sequence %d" % n


ORDER_PLACES = ("id", "comment", "seq", "qual")
ORDER_DEATHS = ("q_short", "q_long", "no_plus", "no_at")
ORDER_CUTS = ("cut_hdr", "cut_seq", "cut_plus")


def _order_parts(b, death=None, place=None):
    p = b.parts(plus=b"+")
    if death == "q_short": p[9] = p[9][:-1]
    if death == "q_long": p[9] = p[9] + b"I"
    if death == "no_plus": p[7], p[8], p[9] = b"", b"", _set(p[9], 0, ord("I"))
    if death == "no_at": p[0] = b""
    if place:
        i = {"id": 1, "comment": 3, "seq": 5, "qual": 9}[place]
        p[i] = _set(p[i], 3, 0xFF if place != "seq" else 0x7E)
    if death == "cut_hdr": p = p[:2]
    if death == "cut_seq": p = p[:7]
    if death == "cut_plus": p = p[:9]
    return p


def order_text(place, death, rel, delta, rng):
    """A strict byte in `place` of record r, whose last byte lies at tile seam 3 + delta, beside a structural death in record r + rel (a
    truncation: of the last record, which is r + 1, or r itself with rel = 0: the strict byte inside the truncated record)."""
    b = _Fq(rng)
    b.out += b"\n\n"
    cut = death.startswith("cut")
    recs = [_order_parts(b, death if rel == j else None, place if j == 0 else None) for j in (-1, 0, 1)]
    if cut and rel == 0:
        recs = recs[:2]
    size = sum(len(x) for p in recs[:2] for x in p)
    b.fill_to(3 * TILE + delta + 1 - size)
    for p in recs:
        b.out += b"".join(p)
    if not cut:
        b.out += b"".join(b.parts()) + b"".join(b.parts())
    name = "fq_order_%s_%s_%+d_%+d" % (place, death, rel, delta)
    return AText(name, "fastq", "order", 0, b.out, [Plant("record_end", TILE, delta, 3 * TILE + delta)], DNA, info={"what": place})


def clean_text(kind, seq_type, rng):
    if kind == "fasta":
        b = _Fa8(rng, 61, seq_type)
        b.out += b"\n\n"
        _fa_end(b, "end_nl", 24 * TILE + 33)
    else:
        b = _Fq8(rng, seq_type)
        b.out += b"\n\n"
        _fq_end(b, "end_nl", 24 * TILE + 33)
    return AText("%s_%s_clean" % ("fa" if kind == "fasta" else "fq", TYPE_TAG[seq_type]), kind, "clean", 61, b.out, [], seq_type)


# ---- all of them -----------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def texts(seed=0):
    """Every planned text under `seed` (NAF_TEST_SEED is added to it), the 64 MiB one apart (big_text)."""
    if seed in _CACHE:
        return _CACHE[seed]
    base = [9000]

    def rng():
        base[0] += 1
        return np.random.default_rng(base[0] * 1000 + seed + P.SEED)

    out = []
    ends = [(f, u, d) for f in END_FEATURES for (u, d) in ANCHORS]
    t = 0
    for (kind, st), feats in FEATURES.items():                             # A: the 8-bit alphabets
        for i, combos in enumerate(_deal(feats)):
            name = "%s_%s_features_%d" % ("fa" if kind == "fasta" else "fq", TYPE_TAG[st], i)
            if kind == "fasta":
                out.append(fasta_text(name, "features", WIDTHS[t % len(WIDTHS)], combos, ends[t % len(ends)], rng(), st, t))
            else:
                out.append(fastq_text(name, "features", combos, ends[t % len(ends)], rng(), st, t))
            t += 1
    for st in (DNA, RNA, PROTEIN, TEXT):                                   # A: damaged IDs
        for kind in ("fasta", "fastq"):
            for i, combos in enumerate(_deal(ID_FEATURES)):
                name = "%s_%s_ids_%d" % ("fa" if kind == "fasta" else "fq", TYPE_TAG[st], i)
                if kind == "fasta":
                    out.append(fasta_text(name, "ids", WIDTHS[t % len(WIDTHS)], combos, ends[t % len(ends)], rng(), st, t))
                else:
                    out.append(fastq_text(name, "ids", combos, ends[t % len(ends)], rng(), st, t))
                t += 1
    for st in (DNA, RNA, PROTEIN, TEXT):                                   # B: the FIRST offender at every anchor
        for kind in ("fasta", "fastq"):
            kinds = STRICT_KINDS[kind] + (("gt_in_id",) if (kind, st) == ("fasta", TEXT) else ()) + (("seq_iupac",) if (kind, st) == ("fastq", DNA) else ())
            for what in kinds:
                for j, (u, d) in enumerate(ANCHORS):
                    out.append(strict_text(kind, st, what, u, d, rng(), j))
    for kind in ("fasta", "fastq"):                                        # B: record numbers
        for j, (blocks, delta) in enumerate([(k, d) for k in (1, 2, 3) for d in (-1, 0, 1)]):
            out.append(numbered_text(kind, (DNA, PROTEIN, TEXT)[j % 3], blocks, delta, (b"\n\n", b"\n \n\t\n", b"")[(j // 3 + j) % 3], rng()))
    for place in ORDER_PLACES:                                             # B: FASTQ order across a tile seam
        for death in ORDER_DEATHS:
            for rel in (-1, 0, 1):
                for delta in (-1, 0, 1):
                    out.append(order_text(place, death, rel, delta, rng()))
        for death in ORDER_CUTS:
            for rel in (1, 0):
                if rel == 0 and (place == "qual" or (place, death) in (("comment", "cut_hdr"), ("seq", "cut_hdr"))):
                    continue                                               # (the truncated record does not reach that place)
                for delta in (-1, 0, 1):
                    out.append(order_text(place, death, rel, delta, rng()))
    for st in (DNA, RNA, PROTEIN, TEXT):                                   # B: nothing to stop at
        for kind in ("fasta", "fastq"):
            out.append(clean_text(kind, st, rng()))
    out.append(AText("fa_dna_U", "fasta", "strict_small", 4, b">a\nACGT\n>b c\nACGU\nA!\n", [], DNA, info={"what": "seq"}))
    out.append(AText("fa_rna_T", "fasta", "strict_small", 4, b">a\nACGU\n>b c\nACGT\nA!\n", [], RNA, info={"what": "seq"}))
    assert len({x.name for x in out}) == len(out)
    _CACHE[seed] = out
    return out


def names(family=None):
    return [t.name for t in texts(0) if family is None or t.family == family]


def seam_strict_texts(seed=0):
    """The texts of seam_plan that hold an unexpected byte (bang, bad_z, q01, q7f, q80, h01): the verdict is the model's."""
    return [t for t in P.texts(seed) if not t.dies and {p.feature for p in t.plants} & {"bang", "bad_z", "q01", "q7f", "q80", "h01"}]


def cross_product():
    """{(alphabet, kind, family, feature, unit, delta): times planted} over texts(0), every cell present (zero where it is not)."""
    want = {}
    for (kind, st), feats in FEATURES.items():
        for f in feats:
            for (u, d) in ANCHORS:
                want[(st, kind, "features", f, u, d)] = 0
    for st in (DNA, RNA, PROTEIN, TEXT):
        for kind in ("fasta", "fastq"):
            for f in ID_FEATURES:
                for (u, d) in ANCHORS:
                    want[(st, kind, "ids", f, u, d)] = 0
            kinds = STRICT_KINDS[kind] + (("gt_in_id",) if (kind, st) == ("fasta", TEXT) else ()) + (("seq_iupac",) if (kind, st) == ("fastq", DNA) else ())
            for f in kinds:
                for (u, d) in ANCHORS:
                    want[(st, kind, "strict", "F_" + f, u, d)] = 0
    for t in texts(0):
        for p in t.plants:
            key = (t.seq_type, t.kind, t.family, p.feature, p.unit, p.delta)
            if key in want:
                want[key] += 1
    return want
