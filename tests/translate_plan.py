"""The plan of the translation tests (test_translate_cpu.py holds it to its claims, test_gpu_translate.py runs it): the model, the texts and
the calls.  Pure Python and numpy; nothing here comes from the code under test.

The model works on the oracle's --sequences text of an archive (one line per record) and on its ids and names.  A genetic code is a dict
from the 64 three-letter strings over ACGT to a letter, made from NCBI's own TCAG-order string of code 1 and the difference lists below by
string expansion; the letter of a codon that holds other codes is found by expanding each of its letters to its bases (codon_letter), and a
text is translated through a dict of all 16^3 triples of the stored letters made that way (never from the library's table).  The header
rule and the wrap are written out in protein_text.

The planted texts have a background of seeded letters of {A, C, G}: neither strand of it reads ATG in any frame (ATG and its reverse
complement CAT both hold a T), so no letter of its translation is M.  A plant is the codon ATG (strand 0) or CAT (strand 1: read as ATG), and
a planted call is a list of segments in which every plant is in frame, so each gives one M:
  chunk / round / tile   the plant's LETTER falls at d = -2 .. +2 of a multiple of 16 (not of 1024), of 1024 (not of 4096), of 4096 of the
                         call's output: one whole record on one line, so that letter j is output byte (header length + j)
  block                  the plant's first BASE lies at d = -3 .. +2 of base 262144 k of the stream: a raw block of the oracle's packed stream
  record                 the same around the stream position where a record ends and the next one begins; d = -2, -1: no codon fits, the
                         record ends in the plant's first two or one letters and a segment that is in frame with them drops them
  end                    the same at the stream's end, d = -3, -2, -1"""
import os

import numpy as np

from locate_plan import _random, _wrap, fasta
from composition_plan import lines_of                                               # noqa: F401  (the records of a --sequences text)

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
SEEDS = (0, 1, 2)
WHOLE = 2 ** 64 - 1
BLOCK = 262144                                                                      # bases of a 128 KiB block of the packed stream
LINE_LENGTHS = (0, 1, 2, 15, 16, 17, 60, 4096)
SMALL_SPANS = (1, 2, 3, 4, 5, 6, 7, 8, 47, 48, 49)
OUT_OFFSETS = (-2, -1, 0, 1, 2)
SRC_OFFSETS = (-3, -2, -1, 0, 1, 2)
OUT_KINDS = ("chunk", "round", "tile")
SRC_KINDS = ("block", "record", "end")
CODES = "-TGKCYSBAWRDMHVN"                                                          # the stored 4-bit codes, by value

# NCBI's table 1 in NCBI's own order: the bases T, C, A, G, first base slowest
STANDARD_TCAG = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
# the same in the library's order (A, C, G, T): written out a second time, the CPU test permutes one into the other
STANDARD_ACGT = "KNKNTTTTRSRSIIMI" "QHQHPPPPRRRRLLLL" "EDEDAAAAGGGGVVVV" "*Y*YSSSS*CWCLFLF"
# the other built-in codes as differences from 1: codon, letter
DIFFS = {
    1: "", 2: "AGA * AGG * ATA M TGA W", 3: "ATA M CTT T CTC T CTA T CTG T TGA W", 4: "TGA W", 5: "AGA S AGG S ATA M TGA W", 6: "TAA Q TAG Q",
    9: "AAA N AGA S AGG S TGA W", 10: "TGA C", 11: "", 12: "CTG S", 13: "AGA G AGG G ATA M TGA W", 14: "AAA N AGA S AGG S TAA Y TGA W", 15: "TAG Q",
    16: "TAG L", 21: "AAA N AGA S AGG S ATA M TGA W", 22: "TCA * TAG L", 23: "TTA *", 24: "AGA S AGG K TGA W", 25: "TGA G", 26: "CTG A",
}
NOT_CODES = (0, 7, 8, 17, 18, 19, 20, 27, 28, 33, -1, 100, 2 ** 31 - 1)
# a code of its own for --code-table / naf_gpu_genetic_code_parse: code 1 with every stop read through and AAA as the only stop
CUSTOM_ACGT = "*" + STANDARD_ACGT[1:].replace("*", "Q")
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
_COMP = bytes.maketrans(b"ACGTMRWSYKVHDBN-", b"TGCAKYWSRMBDHVN-")


def code_dict(code=1):
    """{"AAA": "K", ...} of a built-in id, or of 64 letters in ACGT order"""
    if isinstance(code, str):
        assert len(code) == 64
        return {a + b + c: code[16 * i + 4 * j + k].upper() for i, a in enumerate("ACGT") for j, b in enumerate("ACGT") for k, c in enumerate("ACGT")}
    d = {a + b + c: STANDARD_TCAG[16 * i + 4 * j + k] for i, a in enumerate("TCAG") for j, b in enumerate("TCAG") for k, c in enumerate("TCAG")}
    words = DIFFS[code].split()
    for codon, letter in zip(words[0::2], words[1::2]):
        assert codon in d and d[codon] != letter
        d[codon] = letter
    return d


def letters_acgt(code):
    d = code_dict(code)
    return "".join(d[a + b + c] for a in "ACGT" for b in "ACGT" for c in "ACGT")


def stops_of(code):
    """the codon set of a code's stops: positional notation in base 4"""
    return sum(1 << int("".join(str("ACGT".index(x)) for x in codon), 4) for codon, letter in code_dict(code).items() if letter == "*")


def codon_letter(codon, d):
    """the letter of three stored letters (upper case, T for U) under the code dict d"""
    if codon == "---":
        return "-"
    if "-" in codon:
        return "X"
    seen = {d[a + b + c] for a in IUPAC[codon[0]] for b in IUPAC[codon[1]] for c in IUPAC[codon[2]]}
    return seen.pop() if len(seen) == 1 else "X"


_TRIPLES = {}


def triples(code):
    """every triple of the sixteen stored letters -> its letter"""
    key = code if isinstance(code, int) else code.upper()
    if key not in _TRIPLES:
        d = code_dict(code)
        _TRIPLES[key] = {a + b + c: codon_letter(a + b + c, d) for a in CODES for b in CODES for c in CODES}
    return _TRIPLES[key]


def lut_index(codon):
    return (CODES.index(codon[0]) << 8) | (CODES.index(codon[1]) << 4) | CODES.index(codon[2])


def expected_lut(code):
    t = triples(code)
    out = bytearray(4096)
    for codon, letter in t.items():
        out[lut_index(codon)] = ord(letter)
    return bytes(out)


def reading(line, b, e, rc):
    """bases [b, e) of a record's line (bytes) in reading direction, upper case, T for U"""
    s = line[b:e].upper().replace(b"U", b"T")
    return (s.translate(_COMP)[::-1] if rc else s).decode("latin1")


def translate(s, code=1):
    t = triples(code)
    return "".join([t[s[i:i + 3]] for i in range(0, len(s) - 2, 3)])


def translate_walk(s, code=1):
    """the same, a codon at a time and without the dict of triples"""
    d = code_dict(code)
    out = []
    i = 0
    while i + 3 <= len(s):
        out.append(codon_letter(s[i:i + 3], d))
        i += 3
    return "".join(out)


def seg4(seg):
    if isinstance(seg, int):
        return seg, 0, WHOLE, 0
    return (seg[0], seg[1], seg[2], seg[3] if len(seg) == 4 else 0)


def header_of(ident, name, b, e, whole, rc):
    if whole:
        return ">" + ident + ("/rc" if rc else "") + (" " + name if name else "") + "\n"
    return ">%s:%d-%d%s\n" % (ident, b + 1, e, "/rc" if rc else "")


def pieces(lines, ids, names, segs, code=1, line_length=60):
    """[(header, letters)] of the segments"""
    out = []
    for seg in segs:
        r, b, e, rc = seg4(seg)
        whole = b == 0 and e == WHOLE
        e = min(e, len(lines[r]))
        assert whole or b < e
        out.append((header_of(ids[r], names[r], b, e, whole, rc), translate(reading(lines[r], b, e, rc), code)))
    return out


def protein_text(lines, ids, names, segs, code=1, line_length=60):
    """the bytes naf_gpu_unnaf_translate writes: header line, then the letters in lines of line_length (0: one line), each with its newline"""
    out = []
    for head, prot in pieces(lines, ids, names, segs, code, line_length):
        out.append(head)
        if prot:
            w = line_length if line_length else len(prot)
            out.extend(prot[i:i + w] + "\n" for i in range(0, len(prot), w))
    return "".join(out).encode("latin1")


def frame_segments(lengths, frames, records=None):
    """the segments of reading frames of whole records: frame f > 0 from base f - 1 on, frame -f the reverse complement from base f - 1 on;
    1 and -1 are the whole record, a frame without a base is left out"""
    out = []
    for r in (range(len(lengths)) if records is None else records):
        for f in frames:
            if f == 1:
                out.append((r, 0, WHOLE, 0))
            elif f == -1:
                out.append((r, 0, WHOLE, 1))
            elif f > 0 and f - 1 < lengths[r]:
                out.append((r, f - 1, lengths[r], 0))
            elif f < 0 and -f - 1 < lengths[r]:
                out.append((r, 0, lengths[r] + f + 1, 1))
    return out


# capi.frames_to_segments, by hand: (lengths, frames, records) -> segments
FRAMES_TABLE = [
    ([10], [1], None, [(0, 0, WHOLE, 0)]),
    ([10], [2], None, [(0, 1, 10, 0)]),
    ([10], [3], None, [(0, 2, 10, 0)]),
    ([10], [-1], None, [(0, 0, WHOLE, 1)]),
    ([10], [-2], None, [(0, 0, 9, 1)]),
    ([10], [-3], None, [(0, 0, 8, 1)]),
    ([7, 0, 1, 2, 3], [1, 2, 3, -1, -2, -3], None,
     [(0, 0, WHOLE, 0), (0, 1, 7, 0), (0, 2, 7, 0), (0, 0, WHOLE, 1), (0, 0, 6, 1), (0, 0, 5, 1),
      (1, 0, WHOLE, 0), (1, 0, WHOLE, 1),
      (2, 0, WHOLE, 0), (2, 0, WHOLE, 1),
      (3, 0, WHOLE, 0), (3, 1, 2, 0), (3, 0, WHOLE, 1), (3, 0, 1, 1),
      (4, 0, WHOLE, 0), (4, 1, 3, 0), (4, 2, 3, 0), (4, 0, WHOLE, 1), (4, 0, 2, 1), (4, 0, 1, 1)]),
    ([5, 6, 7], [-3, 2], [2, 0], [(2, 0, 5, 1), (2, 1, 7, 0), (0, 0, 3, 1), (0, 1, 5, 0)]),
    ([], [1, -1], None, []),
    ([4], [], None, []),
]


class Call:
    """segments, code and line length of one naf_gpu_unnaf_translate; plants: (kind, d, strand, output byte of the planted M) under this call"""

    def __init__(self, tag, segs, code=1, line_length=60, plants=()):
        self.tag, self.segs, self.code, self.line_length, self.plants = tag, list(segs), code, line_length, list(plants)


class Case:
    def __init__(self, name, text, records, ids, names, calls, seq_type=0, fastq=False):
        self.name, self.text, self.records, self.ids, self.names, self.calls, self.seq_type, self.fastq = name, text, records, ids, names, calls, seq_type, fastq

    def lines(self):
        return [r.encode() for r in self.records]

    def expected(self, call, lines=None, ids=None, names=None):
        return protein_text(lines if lines is not None else self.lines(), ids or self.ids, names or self.names, call.segs, call.code, call.line_length)


def _ids(n):
    return ["r%d" % k for k in range(n)], ["some words"] * n


def _cut(stream, bounds):
    return [stream[a:b] for a, b in zip(bounds[:-1], bounds[1:])]


def _in_frame(o, n, rc, before=5, after=6):
    """a segment of a record of n bases in which the codon at offset o is in frame: about `before` codons in front of it in reading direction"""
    if not rc:
        b = o - 3 * min(before, o // 3)
        return b, min(n, o + 3 + 3 * after + 1)
    e = o + 3 + 3 * min(before, (n - o - 3) // 3)
    return max(0, o - 3 * after - 1), e


def output_case(seed):
    """two records of 60000 bases, one for each strand; as one whole record on one line, letter j is output byte (header length + j)"""
    rng = np.random.default_rng(13000 + seed)
    n = 66000
    ids, names = _ids(2)
    recs = [bytearray(_random(rng, n, "ACG").encode()) for _ in range(2)]
    calls = []
    for rc in (0, 1):
        hl = len(header_of(ids[rc], names[rc], 0, n, True, rc))
        plants = []
        for kind, seams in (("chunk", [16 * (7 + 5 * q) for q in range(5)]), ("round", [1024 * (1 + 2 * q) for q in range(5)]),
                            ("tile", [4096, 8192, 12288, 16384, 4096])):                # (22 KB of text: four tile seams; d = -2 and d = +2 share one)
            for seam, d in zip(seams, OUT_OFFSETS):
                j = seam + d - hl
                o = 3 * j if not rc else n - 3 * (j + 1)
                recs[rc][o:o + 3] = b"CAT" if rc else b"ATG"
                plants.append((kind, d, rc, seam + d))
        calls.append(Call("whole%d" % rc, [(rc, 0, WHOLE, rc)], 1, 0, plants))
    records = [r.decode() for r in recs]
    calls.append(Call("both", [(0, 0, WHOLE, 0), (1, 0, WHOLE, 1), (0, 0, WHOLE, 1)], 11, 4096))
    calls.append(Call("six", frame_segments([n, n], [1, 2, 3, -1, -2, -3]), 1, 60))
    return Case("output", fasta(records, 70), records, ids, names, calls)


def blocks_case(seed, name="blocks", total=1310000, groups=(((-3, 0), (0, 1)), ((-2, 0), (1, 1)), ((-1, 0), (2, 1)), ((-3, 1), (0, 0)))):
    """a stream of `total` bases in records of uneven lengths; block seam k + 1 takes the two plants (d, strand) of groups[k], which do not overlap"""
    rng = np.random.default_rng(13100 + seed + len(name))
    s = bytearray(_random(rng, total, "ACG").encode())
    bounds = [0, 0, 100001, 300000, 300000, 655360, 900003, total, total]
    bounds = [b for b in bounds if b <= total]
    if bounds[-1] != total:
        bounds += [total, total]
    lens = [b - a for a, b in zip(bounds[:-1], bounds[1:])]
    ids, names = _ids(len(lens))
    segs, plants = [], []
    for k, group in enumerate(groups):
        seam = BLOCK * (k + 1)
        for d, rc in group:
            p = seam + d
            r = max(i for i in range(len(lens)) if bounds[i] <= p and lens[i])
            o = p - bounds[r]
            s[p:p + 3] = b"CAT" if rc else b"ATG"
            b, e = _in_frame(o, lens[r], rc)
            segs.append((r, b, e, rc))
            plants.append(("block", d, rc, (r, b, e, rc), p))
    stream = s.decode()
    records = _cut(stream, bounds)
    c = Case(name, fasta(records, 80), records, ids, names, [])
    c.stream, c.src_plants = stream, plants
    c.calls.append(Call("seams", segs, 1, 60))
    return c, bounds, lens


def far_case(seed):
    """800000 bases; the remaining block plants, and segments more than two blocks of packed stream (524288 bases) apart: several ranges"""
    c, bounds, lens = blocks_case(seed, "far", 800000, (((-2, 1), (1, 0)), ((-1, 1), (2, 0))))
    assert lens[1] and lens[5] and bounds[5] == 655360
    far = [(1, 10, 400, 0), (5, 100000, 100300, 1), (1, 500, 900, 1), (5, 100100, 100200, 0)]      # stream bases 10 .. 900 and 755360 .. 755660
    c.calls.append(Call("far", far, 1, 60))
    c.far_bases = (bounds[1] + 10, bounds[1] + 900, bounds[5] + 100000, bounds[5] + 100300)
    assert c.far_bases[2] - c.far_bases[1] > 2 * BLOCK                              # the selection merges neighbours up to two blocks apart
    return c


def records_case(seed):
    """40 records of 0 to 4000 bases, a plant around the end of every other one: (d, strand) by q = 0 .. 11"""
    rng = np.random.default_rng(13200 + seed)
    lens = [int(x) for x in rng.integers(300, 4000, 40)]
    lens[0] = 0
    lens[20] = 0
    lens[21] = 0
    lens[39] = 3001
    bounds = np.concatenate(([0], np.cumsum(lens))).tolist()
    s = bytearray(_random(rng, bounds[-1], "ACG").encode())
    ids, names = _ids(40)
    segs, plants = [], []

    def plant(kind, seam_record, d, rc):
        """the plant whose first base is d from the end of record seam_record"""
        r = seam_record if d < 0 else seam_record + 1
        o = lens[r] + d if d < 0 else d
        fit = min(3, lens[r] - o)
        letters = b"CAT" if rc else b"ATG"
        s[bounds[r] + o:bounds[r] + o + fit] = letters[:fit]
        if fit == 3:
            b, e = _in_frame(o, lens[r], rc)
        else:                                                                     # no codon fits: a segment to the record's end, `fit` bases more than whole codons --
            b, e = lens[r] - 12 - fit, lens[r]                                     # forward they are dropped, reverse they are the head of the first codon read
        segs.append((r, b, e, rc))
        plants.append((kind, d, rc, (r, b, e, rc), bounds[r] + o, fit))

    for q in range(12):
        plant("record", 2 * q + 1 if q <= 8 else 2 * q + 5, SRC_OFFSETS[q % 6], q // 6)      # (records 0, 20 and 21 are empty)
    stream = s.decode()
    records = _cut(stream, bounds)
    c = Case("records", fasta(records, 61), records, ids, names, [])
    c.stream, c.src_plants, c.bounds = stream, plants, bounds
    for L in LINE_LENGTHS:
        c.calls.append(Call("seams_L%d" % L, segs, 1, L))
    # repeats and overlaps, whole records among them, in no order
    mix = [(5, 0, 300, 0), (5, 0, 300, 0), (5, 100, 250, 1), (5, 0, WHOLE, 0), 7, (7, 0, WHOLE, 1), (5, 1, 300, 0), (5, 2, 300, 1), (0, 0, WHOLE, 0), (20, 0, WHOLE, 1), (5, 0, 300, 0),
           (3, 10, 10 ** 12, 0), (3, 10, WHOLE, 1)]
    c.calls.append(Call("mix", mix, 2, 17))
    c.calls.append(Call("mix6", mix, 6, 0))
    # 5 000 segments of one codon each
    pick = rng.integers(1, 40, 5000)
    ones = []
    for k, r in enumerate(pick):
        r = int(r) if lens[int(r)] else 5
        b = int(rng.integers(0, lens[r] - 3))
        ones.append((r, b, b + 3, k & 1))
    c.calls.append(Call("ones", ones, 1, 60))
    c.calls.append(Call("six", frame_segments(lens, [1, 2, 3, -1, -2, -3]), CUSTOM_ACGT, 60))
    return c


def end_cases(seed):
    """short texts whose stream ends d = -3, -2, -1 behind a plant's first base, both strands; odd and even lengths"""
    out = []
    rng = np.random.default_rng(13300 + seed)
    for q, (d, rc) in enumerate((d, rc) for rc in (0, 1) for d in (-3, -2, -1)):
        n = 5000 + q
        s = bytearray(_random(rng, n, "ACG").encode())
        fit = -d
        s[n + d:n] = (b"CAT" if rc else b"ATG")[:fit]
        b, e = _in_frame(n - 3, n, rc) if fit == 3 else (n - 12 - fit, n)
        records = [_random(rng, 100 + q, "ACG"), s.decode()]
        ids, names = _ids(2)
        c = Case("end%d" % q, fasta(records, 60), records, ids, names, [Call("end", [(1, b, e, rc), (1, 0, WHOLE, rc)], 1, 60)])
        c.stream = "".join(records)
        c.src_plants = [("end", d, rc, (1, b, e, rc), 100 + q + n + d, fit)]
        out.append(c)
    return out


def small_segments(n_record):
    """begin on every residue mod 6, spans of 1 .. 8 and 47, 48, 49 bases, both strands"""
    return [(1, 12 + b, 12 + b + n, rc) for rc in (0, 1) for b in range(6) for n in SMALL_SPANS]


def small_case(seed, rna=False):
    """record 0 is empty, record 1 has 240 letters of every code, record 2 is all 4096 triples of the sixteen codes"""
    rng = np.random.default_rng(13400 + seed)
    every = "".join(a + b + c for a in CODES for b in CODES for c in CODES)
    lower = "".join(ch.lower() if rng.integers(0, 3) == 0 else ch for ch in _random(rng, 240, "ACGT" * 6 + CODES))
    records = ["", lower, every, _random(rng, 50, "ACGT")]
    if rna:
        records = [r.replace("T", "U").replace("t", "u") for r in records]
    ids, names = _ids(4)
    calls = []
    for L in LINE_LENGTHS:
        calls.append(Call("small_L%d" % L, [(0, 0, WHOLE, 0)] + small_segments(240) + [(0, 0, WHOLE, 1)], 1, L))
    for code in (1, 2, 6, 11, 22, CUSTOM_ACGT):
        calls.append(Call("every_%s" % (code if isinstance(code, int) else "custom"), [2, (2, 0, WHOLE, 1), (2, 1, 12288, 0), (2, 0, 12286, 1), (2, 5, 12288, 1)], code, 64))
    return Case("rna" if rna else "small", fasta(records, 60), records, ids, names, calls, seq_type=1 if rna else 0)


def reads_case(seed):
    """a FASTQ text: the translation is FASTA-shaped, '>' headers, whole reads and parts of them"""
    rng = np.random.default_rng(13500 + seed)
    lens = [1 + k % 33 for k in range(200)] + [150] * 50
    records = [_random(rng, n, "ACGT" * 12 + "N") for n in lens]
    text = "".join("@read%d x\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(records)).encode()
    ids, names = ["read%d" % k for k in range(len(records))], ["x"] * len(records)
    calls = [Call("reads6", frame_segments(lens, [1, 2, 3, -1, -2, -3]), 1, 20), Call("parts", [(k, 1, 40, k & 1) for k in range(len(records)) if lens[k] > 1], 1, 0)]
    return Case("reads", text, records, ids, names, calls, fastq=True)


def planned(seed=SEED):
    return [output_case(seed), blocks_case(seed)[0], far_case(seed), records_case(seed), small_case(seed), small_case(seed, rna=True), reads_case(seed)] + end_cases(seed)


def coverage(cases):
    """{(kind, d, strand): [case names]} of the plants that are where they claim and give the M they claim in the model's text"""
    cov = {}
    for c in cases:
        lines = c.lines()
        for call in c.calls:
            if not call.plants:
                continue
            want = c.expected(call)
            for kind, d, rc, at in call.plants:
                seam = at - d
                ok = want[at:at + 1] == b"M" and want.count(b"M") == len(call.plants)
                ok &= seam % 16 == 0 and {"chunk": seam % 1024 != 0, "round": seam % 1024 == 0 and seam % 4096 != 0, "tile": seam % 4096 == 0}[kind]
                if ok:
                    cov.setdefault((kind, d, rc), []).append(c.name)
        for plant in getattr(c, "src_plants", ()):
            kind, d, rc, seg, p = plant[:5]
            fit = plant[5] if len(plant) > 5 else 3
            letters = ("CAT" if rc else "ATG")[:fit]
            ok = c.stream[p:p + fit] == letters
            seam = p - d
            if kind == "block":
                ok &= seam % BLOCK == 0 and seam > 0
            elif kind == "record":
                ends = np.cumsum([len(r) for r in c.records]).tolist()
                ok &= seam in ends[:-1] and seam != ends[-1]
            else:
                ok &= seam == len(c.stream) and d < 0
            prot = pieces(lines, c.ids, c.names, [seg])[0][1]
            r, b, e, _ = seg
            if fit == 3:
                ok &= prot.count("M") == 1 and (e - b) // 3 == len(prot)
            else:                                                                 # no codon: the segment is in frame with the letters that fit and drops them
                ok &= "M" not in prot and (e - b) % 3 == fit and e == len(c.records[r])
            if ok:
                cov.setdefault((kind, d, rc), []).append(c.name)
    return cov


def coverage_cells():
    return ([(kind, d, rc) for kind in OUT_KINDS for d in OUT_OFFSETS for rc in (0, 1)] +
            [(kind, d, rc) for kind in SRC_KINDS for d in SRC_OFFSETS if not (kind == "end" and d >= 0) for rc in (0, 1)])
