"""The plan of the base-composition tests (test_composition_cpu.py holds it to its claims, test_gpu_composition.py runs it): the texts,
the windows and the expected rows.  Pure Python and numpy; nothing here comes from the code under test.

expected_rows works on the oracle's --sequences text of an archive, mask on (one line per record): letters map to 4-bit codes through
CODES after upper-casing (U is T's code), a lower-case letter counts as masked, and CpG is a C whose next letter IN THE SAME LINE is a G.
brute_rows does the same with a per-base Python loop and shares no code with it.

The `seams` text lays its plants around four kinds of seams of the count kernel -- a lane's 64 bases, a 16-byte load (32 bases), a tile
(4096 bases) and a zstd block of the packed stream (128 KiB = 262144 bases) -- see Seams.  All seams are even stream positions, so a CG
ACROSS a seam always has its C in a byte's high nibble; the other phase is a CG that starts ON the seam and one that ends on it."""
import re

import numpy as np

from locate_plan import CODES, _random, _wrap, fasta, r7_case as _locate_r7

ROW_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("n", "<u8", (16,)), ("masked", "<u8"), ("cpg", "<u8")]
WINDOWS_BIG = (0, 63, 64, 65, 100, 4095, 4096, 4097, 262144, 1 << 40)           # the last: larger than every record
WINDOWS_SMALL = (1, 2, 3, 7, 16)
SEAM_KINDS = ("lane", "load32", "tile", "block")
BLOCK = 262144
_CODE_OF = np.full(256, 255, dtype=np.uint8)
for _k, _ch in enumerate(CODES):
    _CODE_OF[ord(_ch)] = _k
    _CODE_OF[ord(_ch.lower())] = _k
_CODE_OF[ord("U")] = _CODE_OF[ord("u")] = 1


def rows_of(n, window):
    return 1 if window == 0 else -(-n // window)


def lines_of(sequences_text, n_records):
    """The records of a --sequences text: one line each; what follows the last line of a malformed archive is not a record."""
    lines = sequences_text.split(b"\n")
    assert len(lines) >= n_records + 1 or n_records == 0
    return lines[:n_records]


def expected_rows(lines, window, first=0, count=None):
    """The rows of records [first, first + count) as a ROW_DTYPE array, in the order of the contract."""
    last = len(lines) if count is None else first + count
    out = []
    for r in range(first, last):
        a = np.frombuffer(lines[r], dtype=np.uint8)
        n = len(a)
        nw = rows_of(n, window)
        if nw == 0:
            continue
        rows = np.zeros(nw, dtype=ROW_DTYPE)
        rows["record"] = r
        w = window if window else max(n, 1)
        rows["begin"] = np.arange(nw, dtype=np.uint64) * np.uint64(w if window else 0)
        rows["end"] = np.minimum(rows["begin"] + np.uint64(w), np.uint64(n))
        if n:
            codes = _CODE_OF[a].astype(np.int64)
            assert codes.max() < 16
            idx = np.arange(n, dtype=np.int64) // w
            rows["n"] = np.bincount(idx * 16 + codes, minlength=nw * 16).reshape(nw, 16)
            rows["masked"] = np.bincount(idx, weights=(a >= 97) & (a <= 122), minlength=nw).astype(np.uint64)
            cg = np.zeros(n, dtype=bool)
            cg[[m.start() for m in re.finditer(b"C(?=G)", lines[r].upper())]] = True
            rows["cpg"] = np.bincount(idx, weights=cg, minlength=nw).astype(np.uint64)
        out.append(rows)
    return np.concatenate(out) if out else np.zeros(0, dtype=ROW_DTYPE)


def expected_total(lines, rows, first=0, count=None):
    """(record, begin, end, n[16], masked, cpg) of h_total: the records covered, 0, their bases, and the sums of the rows."""
    last = len(lines) if count is None else first + count
    return (last - first, 0, sum(len(x) for x in lines[first:last]), [int(v) for v in rows["n"].sum(axis=0)] if len(rows) else [0] * 16,
            int(rows["masked"].sum()), int(rows["cpg"].sum()))


def brute_rows(lines, windows, first=0, count=None):
    """{window: [(record, begin, end, (n0 .. n15), masked, cpg)]} by one walk over the bases (no numpy, no regex)."""
    last = len(lines) if count is None else first + count
    out = {w: [] for w in windows}
    letters = {ch: k for k, ch in enumerate(CODES)}
    letters["U"] = 1
    for r in range(first, last):
        t = lines[r].decode("latin1")
        n = len(t)
        acc = {}
        for w in windows:
            acc[w] = [[r, k * w, min((k + 1) * w, n) if w else n, [0] * 16, 0, 0] for k in range(rows_of(n, w))]
        for i, ch in enumerate(t):
            up = ch.upper()
            code = letters[up]
            low = ch != up
            cg = up == "C" and i + 1 < n and t[i + 1] in "Gg"
            for w in windows:
                row = acc[w][i // w if w else 0]
                row[3][code] += 1
                row[4] += low
                row[5] += cg
        for w in windows:
            out[w] += [(a, b, e, tuple(c), m, g) for a, b, e, c, m, g in acc[w]]
    return out


def as_tuples(rows):
    return [(int(x["record"]), int(x["begin"]), int(x["end"]), tuple(int(v) for v in x["n"]), int(x["masked"]), int(x["cpg"])) for x in rows]


# ---- texts -------------------------------------------------------------------------------------------------------------------------
class Seams:
    """A stream of 600001 bases (it ends on an odd base), background upper-case ACGT, cut into records.

    seams[kind]: the seam positions of the kind that carry plants; per kind, in this order:
      [0:3]    record ends at seam - 1, seam, seam + 1 (for `block`: 262143, 262144, 262145 -- two records of one base -- and 524288)
      [3:6]    CG with its C at seam - 1 (across the seam), at seam (starts on it), at seam - 2 (ends on it)
      [6:9]    lower-case runs that end at seam - 1, start at seam, start at seam + 1 -- and a run that ends at seam on [3]
      [9:25]   code j of CODES as the last base before the seam and code (j + 5) mod 16 as the first base behind it
    (`block`: a text of this size has two such seams.  The first is the record ends and one code pair chosen by the seed, the second a
    CG across it -- the code pair (C, G); toggles lie at -1 of the first and at 0 and +1 of the second.  The sixteen codes at a block
    seam would need sixteen block seams, 4 M bases: the tile seams carry them, and a block seam is a tile seam to the count kernel.)
    Empty records: in front, two in the middle, one at the end.  C as a record's last base with G opening the next (no CpG): at three
    record ends.  The stream's last base is a C (behind it the padding nibble)."""
    TOTAL = 600001

    def __init__(self, seed):
        rng = np.random.default_rng(8000 + seed)
        T = self.TOTAL
        s = np.frombuffer(_random(rng, T, "ACGT").encode(), dtype=np.uint8).copy()
        low = np.zeros(T, dtype=bool)
        step = {"lane": 64, "load32": 64, "tile": 4096}
        off = {"lane": 0, "load32": 32, "tile": 0}
        first = {"lane": 1001, "load32": 3001, "tile": 3}
        self.seams = {}
        for kind in ("lane", "load32", "tile"):
            ks = [first[kind] + (3 if kind == "tile" else 38) * j for j in range(25)]
            self.seams[kind] = [off[kind] + step[kind] * k for k in ks]
            assert all(p % 4096 for p in self.seams[kind]) or kind == "tile"
        self.seams["block"] = [BLOCK, 2 * BLOCK]
        runs = []                                                                    # the planted lower-case runs, laid last
        cuts, self.cg, self.code_pairs, self.toggles_near, self.c_then_g = [], [], [], [], []
        for kind in ("lane", "load32", "tile"):
            p = self.seams[kind]
            cuts += [p[0] - 1, p[1], p[2] + 1]
            for q, d in ((p[3], -1), (p[4], 0), (p[5], -2)):
                s[q + d], s[q + d + 1] = ord("C"), ord("G")
                self.cg.append((kind, q, d))
            for a, b in ((p[6] - 9, p[6] - 1), (p[7], p[7] + 7), (p[8] + 1, p[8] + 4), (p[3] - 5, p[3])):
                runs.append((a, b))
            self.toggles_near += [(kind, p[6], -1), (kind, p[7], 0), (kind, p[8], 1), (kind, p[3], 0)]
            for j in range(16):
                q = p[9 + j]
                s[q - 1], s[q] = ord(CODES[j]), ord(CODES[(j + 5) % 16])
                self.code_pairs.append((kind, q, j, (j + 5) % 16))
        b1, b2 = self.seams["block"]
        cuts += [b1 - 1, b1, b1 + 1]
        j1 = int(rng.integers(0, 16))
        s[b1 - 1], s[b1] = ord(CODES[j1]), ord(CODES[(j1 + 5) % 16])                  # (b1 - 1 and b1 are records of one base)
        self.code_pairs.append(("block", b1, j1, (j1 + 5) % 16))
        s[b2 - 1], s[b2] = ord("C"), ord("G")                                        # a CG across the second block seam: code pair (4, 2)
        self.cg.append(("block", b2, -1))
        self.code_pairs.append(("block", b2, 4, 2))
        s[b2 + 4095], s[b2 + 4096] = ord("C"), ord("G")                              # and across the tile seam right behind it
        self.cg.append(("tile", b2 + 4096, -1))
        runs += [(b1 - 7, b1 - 1), (b2 + 1, b2 + 9), (b2 - 3, b2)]
        self.toggles_near += [("block", b1, -1), ("block", b2, 1), ("block", b2, 0)]
        cuts += [7, 150003, 150003, 150003, 400001, 401024, 598000]                  # (7: a short first record; 150003 three times: two empty records)
        cuts = sorted(cuts)
        for e in (cuts[5], 400001, 598000):                                          # C ends a record, G opens the next: no CpG
            if s[e - 1] in b"ACGT" and s[e] in b"ACGT" and not any(abs(e - q) < 3 for _, q, _, _ in self.code_pairs):
                s[e - 1], s[e] = ord("C"), ord("G")
                self.c_then_g.append(e)
        s[T - 1] = ord("C")
        for _ in range(60):
            a = int(rng.integers(0, T)); low[a:a + int(rng.integers(1, 3000))] = True
        # toggles within one base of window ends of the longest record, for the small and the tile-sized windows
        bounds = [0, 0] + cuts + [T, T]
        self.bounds = bounds
        lens = [b - a for a, b in zip(bounds[:-1], bounds[1:])]
        self.longest = int(np.argmax(lens))
        rb = bounds[self.longest]
        self.window_toggles = []
        for wi, w in enumerate((63, 64, 65, 100, 4095, 4096, 4097)):
            for k, d in ((2 + 7 * wi, -1), (3 + 7 * wi, 0), (4 + 7 * wi, 1)):      # (a k of its own per window: the runs stay apart)
                at = rb + k * w + d
                runs.append((at, at + 5))
                self.window_toggles.append((w, k, d, at))
        for a, b in runs:                                                            # (no random run swallows a planted toggle)
            low[a - 12:b + 12] = False
        for a, b in runs:
            low[a:b] = True
        letters = (s >= 65) & (s <= 90)
        s[low & letters] += 32
        self.stream = s.tobytes().decode()
        self.records = [self.stream[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
        self.text = fasta(self.records, 61)


class Case:
    def __init__(self, name, text, windows, seq_type=0, no_mask=False, records=None, r7=False):
        self.name, self.text, self.windows, self.seq_type, self.no_mask, self.records, self.r7 = name, text, windows, seq_type, no_mask, records, r7


def _cut(stream, rng, n_records, empty_at=()):
    cuts = sorted(int(x) for x in rng.integers(1, len(stream), n_records - 1))
    bounds = [0] + cuts + [len(stream)]
    recs = [stream[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    for k in empty_at:
        recs.insert(k, "")
    return recs


def seams_case(seed):
    S = Seams(seed)
    c = Case("seams", S.text, WINDOWS_BIG, records=S.records)
    c.seams = S
    return c


def plain_case(seed):
    rng = np.random.default_rng(8100 + seed)
    recs = _cut(_random(rng, 200001, "ACGT"), rng, 7, empty_at=(2,))
    return Case("plain", fasta(recs, 80), WINDOWS_BIG, records=recs)


def sparse_iupac_case(seed):
    rng = np.random.default_rng(8100 + seed)                                        # `plain` again ...
    stream = list(_random(rng, 200001, "ACGT"))
    recs_plain = _cut("".join(stream), rng, 7, empty_at=(2,))
    for k, p in enumerate(range(5000, len(stream), 3 * 4096 + 17)):                  # ... with one ambiguity code every few tiles
        stream[p] = "RYSWKMBDHVN-"[k % 12]
    out, at = [], 0
    for r in recs_plain:
        out.append("".join(stream[at:at + len(r)])); at += len(r)
    return Case("sparse_iupac", fasta(out, 80), WINDOWS_BIG, records=out)


def _mask_runs(rng, s, n_runs, longest):
    b = bytearray(s.encode())
    for _ in range(n_runs):
        a = int(rng.integers(0, max(len(b), 1))); e = min(len(b), a + int(rng.integers(1, longest)))
        b[a:e] = bytes(b[a:e]).lower()
    return b.decode()


def all16_case(seed):
    rng = np.random.default_rng(8200 + seed)
    stream = _mask_runs(rng, _random(rng, 20011, CODES), 80, 200)
    recs = _cut(stream, rng, 9, empty_at=(0, 4))
    return Case("all16", fasta(recs, 50), WINDOWS_BIG + WINDOWS_SMALL, records=recs)


def rna_case(seed):
    rng = np.random.default_rng(8300 + seed)
    stream = _mask_runs(rng, _random(rng, 60003, "ACGU" * 8 + "NRY"), 30, 900)
    recs = _cut(stream, rng, 5)
    return Case("rna", fasta(recs, 70), WINDOWS_BIG, seq_type=1, records=recs)


def fastq_case(seed):
    rng = np.random.default_rng(8400 + seed)
    lens = [int(x) for x in rng.integers(1, 301, 3000)]
    lens[:6] = [1, 2, 63, 64, 65, 300]
    recs = []
    for k, n in enumerate(lens):
        r = list(_random(rng, n, "ACGT" * 6 + "N"))
        if k % 3 == 0:
            r[-1] = "C"                                                             # C ends a read ...
        if k % 3 == 1:
            r[0] = "G"                                                              # ... and G opens the next: no CpG
        recs.append("".join(r))
    text = "".join("@read%d x\n%s\n+\n%s\n" % (k, r, "I" * len(r)) for k, r in enumerate(recs)).encode()
    return Case("fastq", text, WINDOWS_BIG + WINDOWS_SMALL, records=recs)


def r7_case(seed):
    c = _locate_r7(seed)                                                            # bases behind the last record; the text ends in ...GGTG
    return Case("r7", c.text, WINDOWS_BIG, records=None, r7=True)


def nomask_case(seed):
    rng = np.random.default_rng(8500 + seed)
    stream = _mask_runs(rng, _random(rng, 50001, "ACGTN"), 20, 2000)                # lower case in the text, no mask section in the archive
    recs = _cut(stream, rng, 4)
    return Case("nomask", fasta(recs, 60), WINDOWS_BIG, no_mask=True, records=[r.upper() for r in recs])


def no_records_case(seed):
    return Case("no_records", b"", (0, 100), records=[])


def planned(seed=0):
    return [seams_case(seed), plain_case(seed), sparse_iupac_case(seed), all16_case(seed), rna_case(seed), fastq_case(seed), r7_case(seed),
            nomask_case(seed), no_records_case(seed)]


# ---- the command line's table --------------------------------------------------------------------------------------------------------
def table(rows, names, rna=False):
    """The lines unnaf --composition prints for the rows."""
    out = ["#seq\tstart\tend\tA\tC\tG\t%s\tN\tother\tgap\tmasked\tCpG\tGC\n" % ("U" if rna else "T")]
    for x in rows:
        n = [int(v) for v in x["n"]]
        A, Cc, G, T, N, gap = n[8], n[4], n[2], n[1], n[15], n[0]
        other = sum(n) - (A + Cc + G + T + N + gap)
        gc = "%.6f" % ((Cc + G) / (A + Cc + G + T)) if A + Cc + G + T else "NA"
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (names[int(x["record"])], x["begin"], x["end"], A, Cc, G, T, N, other, gap,
                                                                         x["masked"], x["cpg"], gc))
    return "".join(out).encode("latin1")
