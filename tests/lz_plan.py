"""The plan of the match-finder tests (test_lz_plan_cpu.py holds it to its claims and runs it through the serial models,
test_gpu_lz_plan.py runs it on the kernels): byte streams that carry PLANTED copies on the seams of the encoder's LZ stages, and the
checks a frame made of such a stream has to pass.  Pure numpy; nothing here comes from the code under test.

A plant is (target_begin, length, distance): the plan copied `length` bytes from target_begin - distance.  The background is seeded
(NAF_TEST_SEED): uniform bytes by the direct route (Context.zstd_compress), printable letters without line ends by the archive route
(Context.ennaf of one record with one line, whose sequence stream is that line).  Behind a plant and in front of its source lie bytes
that differ from what the copy would go on with, so the planted length is exact -- wherever the class does not ask for the opposite.

Seams are taken from the encoder's split of a stream into blocks, restated here (`split_even`); the serial models split by multiples of
the block size (`split_multiple`), and a case is built for the split it is run with.  Every list of numbers below comes from RFC 8878
(code boundaries) or from a constant the kernels name (ROUND, LANE_EXT, WAVE_STEP, MINMATCH, the anchor rule of k_ldm_insert).

A cell with `exempt` set is one the finders cannot reach by their design; the reason is one of EXEMPT_KINDS.  A case may carry
`probes`: copies that no sequence can code by design (a source in the block in front, four bytes at a block's end, a stream below the
64 bytes the match finder starts at) -- they ride in cells that also hold a plant, and are decoded and bounds-checked like the rest.
Such a cell is listed in PROBE_CELLS with what is expected AT the probe, `check_probes` asserts that on the kernels' frames, and the
table marks the cell: its found count is the neighbour plant's, not the probe's.
`ballast` is a 64-byte copy in the same block as a short plant: a block is coded with its sequences only where that comes out smaller
than its literals alone (k_lz_choose), which one match of five bytes never does.  Ballast is not counted as found.
"""
import os
import zlib
from collections import namedtuple

import numpy as np

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
SEEDS = (SEED, SEED + 1, SEED + 2)
MAX_STREAM = 3 << 20

# constants the kernels name (naf_amd/csrc/zstd_enc.hip)
MINMATCH = 5              # LZ_MINMATCH
ROUND = 64                # positions a wavefront tests per round
LANE_EXT = 32             # LZ_LANE_EXT: a lane hands its match to the wave here
WAVE_STEP = 256           # bytes the wave compares per step
LEN_CAP = 65535           # emit() of k_lzx_parse: lengths are kept in 16 bits
LZ_BLOCK_LOGS = (10, 12, 13, 15)
LZX_BLOCK_LOG = 16
LDM_MIX = 0x9E3779B185EBCA87      # ldm_mix; an anchor is a position whose 8 bytes hash to three zero top bits

# RFC 8878 3.1.1.3.2.1.1: the first value of every code that carries extra bits
LL_FIRST = (16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
ML_FIRST = (35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387)

LENGTHS = (4, 5, 6, 7, 8, 11, 12, 13, LANE_EXT - 1, LANE_EXT, LANE_EXT + 1, LANE_EXT + WAVE_STEP - 1, LANE_EXT + WAVE_STEP,
           LANE_EXT + WAVE_STEP + 1, LANE_EXT + 2 * WAVE_STEP - 1, LANE_EXT + 2 * WAVE_STEP, LANE_EXT + 2 * WAVE_STEP + 1) \
    + tuple(v for f in ML_FIRST for v in (f - 1, f))
LITERALS = tuple(sorted(set((0, 1, 15) + tuple(v for f in LL_FIRST for v in (f - 1, f)))))
ROUND_STARTS = tuple(ROUND + k for k in range(-2, 3)) + tuple(2 * ROUND + k for k in range(-2, 3))
PERIODS = (1, 2, 3, 4, 5, 7, 8, 9)
PERIOD_RUNS = (5, 40, 1000)
DISTANCES = tuple((1 << k) + j for k in range(3, 15) for j in (-4, -3, -2))       # the offset code changes at d + 3 = 2^k
COUNTS = (0, 1, 127, 128, 129)                                                   # the Number_of_Sequences byte boundary
TINY_LZ = (63, 64, 65, 68, 69, 70)
TINY_LZX = (64, 65, 79, 80, 87, 88)
WINDOW_DELTAS = (-2, -1, 0, 1, 2)
WINDOW_LOGS_ARCHIVE = (10, 11, 12, 15, 16)
WINDOW_LOG_DIRECT = 20                                                           # zenc_level_window(2)
CAPS = (65534, 65535, 65536, 65537, 200000)
EXEMPT_KINDS = ("shorter than the minimum match", "distance of W or more", "no match required")
NEVER_EXEMPT = ("end", "rep", "cap", "blockseam", "independent")
# cells that carry a probe, and what the kernels' frame has to show at it (check_probes)
PROBE_CELLS = {("end", "begins_bn-4"): "no sequence begins",          # in the last four bytes of the probe's block
               ("end", "all_zero"): "RLE block",                     # the probe's block is an RLE block
               ("end", "tiny"): "no sequence in the frame",          # streams of 63 to 70 bytes
               ("count", "n0"): "no sequence in the block",
               ("independent", "source_in_block_in_front"): "no sequence begins",     # anywhere in the copy of the block in front's bytes
               ("epoch", "src+1_after"): "window", ("epoch", "src+2_after"): "window"}   # W - 1 and W - 2 back, two epochs on: check_window's

Case = namedtuple("Case", "name stage cls cell route data level env long_log wlog bs seams plants cells alts probes ballast exempt claims guards")
# stage: "lz" (k_lz_parse), "lines" (k_lz_parse_lines in front of it), "lzx" (k_ldm_insert + k_lzx_parse + k_lzx_seqenc)
# cells[i]: the cell of plants[i] (case.cell where a case is one cell); alts: {plant index: other distances that code the same bytes}
# claims: (position, kind, index, delta) -- position == seam(kind, index) + delta; kinds "block" (a block's first byte; index nblk is
#         the stream's end), "epoch" (index * 2^(wlog-1)), "round" (block index: its first byte; delta is the offset in the block)
# guards: (position a, position b): the plan made data[a] != data[b]


class Reject(AssertionError):
    """A frame failed one of the checks; .reason names which."""

    def __init__(self, reason, detail=""):
        AssertionError.__init__(self, "%s: %s" % (reason, detail))
        self.reason = reason


class Redraw(Exception):
    """Two bytes a guard needs to differ are both fixed by plants and happen to be equal: the stream is drawn again."""


def _drawn(make):
    for salt in range(16):
        try:
            return make(salt)
        except Redraw:
            pass
    raise AssertionError("no stream after 16 draws")


# ---- the split ---------------------------------------------------------------------------------------------------------------------
def split_even(n, bs):
    """zenc_block_lo: nblk = ceil(n / bs) blocks of n // nblk bytes, the first n % nblk one byte longer."""
    nblk = max(1, -(-n // bs))
    q, r = divmod(n, nblk)
    return [b * q + min(b, r) for b in range(nblk + 1)]


def split_multiple(n, bs):
    """The serial models: blocks begin on multiples of the block size."""
    nblk = max(1, -(-n // bs))
    return [min(b * bs, n) for b in range(nblk + 1)]


SPLITS = {"even": split_even, "multiple": split_multiple}


def lzx_block(wlog, split):
    """Block size of the cross-block stage: min(2^16, window); the serial model keeps lengths below 2^16 by a block of 65535."""
    bs = min(1 << LZX_BLOCK_LOG, 1 << wlog)
    return min(bs, 65535) if split == "multiple" else bs


def is_anchor(b8):
    return ((int.from_bytes(bytes(b8), "little") * LDM_MIX) & ((1 << 64) - 1)) >> 61 == 0


# ---- a stream under construction -------------------------------------------------------------------------------------------------------
class Stream:
    def __init__(self, name, seed, n, route, bs, split, salt=0):
        assert n <= MAX_STREAM, (name, n)
        self.name, self.route, self.n, self.bs = name, route, n, bs
        self.rng = np.random.default_rng([seed, zlib.crc32(name.encode()), salt])
        # printable, and neither of the two letters that begin a record's header line
        self.alpha = np.array([v for v in range(33, 127) if v not in b">@"] if route == "archive" else range(256), dtype=np.uint8)
        self.d = self.draw(n)
        self.lock = np.zeros(n, dtype=bool)
        self.seams = SPLITS[split](n, bs)
        self.plants, self.cells, self.alts, self.probes, self.ballast, self.claims, self.guards = [], [], {}, [], [], [], []

    def block(self, b):
        return self.seams[b], self.seams[b + 1] - self.seams[b]

    def draw(self, n, nonzero=False):
        a = self.alpha[1:] if nonzero and self.alpha[0] == 0 else self.alpha
        return a[self.rng.integers(0, len(a), n)]

    def other(self, *avoid):
        while True:
            v = int(self.draw(1, nonzero=True)[0])
            if v not in avoid:
                return v

    def fresh(self, at, n, anchored=False, nonzero=True):
        """New background at [at, at + n); anchored: its first 8 bytes are an anchor of the long-distance table."""
        u = self.draw(n, nonzero)
        while anchored and n >= 8 and not is_anchor(u[:8]):
            u[:8] = self.draw(8, nonzero)
        self.d[at:at + n] = u

    def differ(self, a, b):
        """data[a] != data[b], changing whichever of the two no plant has fixed (a first)."""
        if a < 0 or b < 0 or a >= self.n or b >= self.n:
            return
        if self.d[a] == self.d[b]:
            k = a if not self.lock[a] else b
            if self.lock[k]:
                raise Redraw("%s: both bytes of a guard are fixed (%d, %d)" % (self.name, a, b))
            self.d[k] = self.other(int(self.d[a]))
        self.lock[a] = self.lock[b] = True
        self.guards.append((a, b))

    def copy(self, t, l, d):
        assert 0 < d <= t and t + l <= self.n, (self.name, t, l, d)
        self.d[t:t + l] = np.resize(self.d[t - d:t], l) if d < l else self.d[t - d:t - d + l]
        self.lock[t - d:t + l] = True

    def plant(self, t, l, d, cell=None, front=True, back=True, alts=(), kind="plant"):
        self.copy(t, l, d)
        if back:
            self.differ(t + l, t + l - d)
        if front:
            self.differ(t - d - 1, t - 1)
        if kind == "plant":
            if alts:
                self.alts[len(self.plants)] = tuple(alts)
            self.plants.append((t, l, d)); self.cells.append(cell)
        elif kind == "probe":
            self.probes.append((t, l, d))
        else:
            self.ballast.append((t, l, d))

    def add_ballast(self, at):
        """A 64-byte copy, source at `at`, target two rounds on."""
        self.plant(at + 2 * ROUND, 64, 2 * ROUND, kind="ballast")

    def claim(self, pos, kind, index, delta):
        self.claims.append((pos, kind, index, delta))

    def case(self, stage, cls, cell, level=1, env=None, long_log=0, wlog=0, exempt=None):
        assert exempt is None or exempt in EXEMPT_KINDS
        return Case(self.name, stage, cls, cell, self.route, self.d.tobytes(), level, dict(env or {}), long_log, wlog, self.bs, list(self.seams),
                    list(self.plants), [c if c is not None else cell for c in self.cells], dict(self.alts), list(self.probes), list(self.ballast),
                    exempt, list(self.claims), list(self.guards))


def lz_env(blog, lines="0"):
    e = {"NAF_GPU_LZ": "all", "NAF_GPU_BLOCK_LOG": str(blog)}
    if lines is not None:
        e["NAF_GPU_LZ_LINES"] = lines
    return e


def text_of(case):
    """What the archive route hands to Context.ennaf: one record, one line."""
    return b">r\n" + case.data + b"\n"


# ---- the in-block stage (k_lz_parse) ------------------------------------------------------------------------------------------------------
def _lz(seed, split, cls, cell, blog, fill, nblk=3, exempt=None, n=None):
    """A stream of nblk blocks that the even split does NOT cut on multiples of the block size; fill(S, b) plants in block b = 1."""
    bs = 1 << blog

    def make(salt):
        S = Stream("lz.%s.%s" % (cls, cell), seed, n if n is not None else nblk * bs - 5, "direct", bs, split, salt)
        fill(S, 1 if len(S.seams) > 2 else 0)
        return S.case("lz", cls, cell, env=lz_env(blog), exempt=exempt)
    return _drawn(make)


def _blog_for(need):
    for k in LZ_BLOCK_LOGS:
        if need + 16 <= (1 << k) - 2:
            return k
    return None


def lz_cases(seed, split="even"):
    out = []
    # round: the target's first byte around the seams of the 64-position rounds; the source in the round before (the first streak has
    # only the first round in front of it), and the same phases many rounds on with the source seven rounds back
    for off in ROUND_STARTS:
        def fill(S, b, off=off):
            lo, bn = S.block(b)
            d = 40 if off < ROUND + 8 else ROUND
            S.plant(lo + off, 24, d)
            S.claim(lo + off, "round", b, off)
        out.append(_lz(seed, split, "round", "t%d_near" % off, 10, fill))
    for ph in range(-2, 3):
        def fill(S, b, ph=ph):
            lo, bn = S.block(b)
            S.plant(lo + 8 * ROUND + ph, 24, 7 * ROUND - 5)
            S.claim(lo + 8 * ROUND + ph, "round", b, 8 * ROUND + ph)
        out.append(_lz(seed, split, "round", "t%d_far" % (8 * ROUND + ph), 10, fill))

    def two_in_round(S, b):
        lo, bn = S.block(b)
        S.plant(lo + 4 * ROUND + 3, 12, 3 * ROUND); S.plant(lo + 4 * ROUND + 30, 12, 2 * ROUND + 7)
        S.claim(lo + 4 * ROUND + 3, "round", b, 4 * ROUND + 3); S.claim(lo + 4 * ROUND + 30, "round", b, 4 * ROUND + 30)
    out.append(_lz(seed, split, "round", "two_in_one", 10, two_in_round))

    def three_rounds(S, b):
        lo, bn = S.block(b)
        S.plant(lo + 6 * ROUND + 50, ROUND + 20, 5 * ROUND)         # begins in round 6, ends in round 8
        S.claim(lo + 6 * ROUND + 50, "round", b, 6 * ROUND + 50); S.claim(lo + 6 * ROUND + 50 + ROUND + 20, "round", b, 8 * ROUND + 6)
    out.append(_lz(seed, split, "round", "r_to_r2", 10, three_rounds))

    def back_to_back(S, b):
        lo, bn = S.block(b)
        t = lo + 5 * ROUND + 9
        S.plant(t, 20, 4 * ROUND); S.plant(t + 20, 20, 2 * ROUND + 5, front=False)
        S.differ(t + 20 - (2 * ROUND + 5) - 1, t + 19)
    out.append(_lz(seed, split, "round", "back_to_back", 10, back_to_back))

    # length: the planted length at the hand-over to the wave, its 256-byte steps, and every Match_Length code boundary
    # (the source is the 128 bytes in front of the target, repeated: the 2^12 entries of the hash table forget a source that lies
    # thousands of positions back, whatever the length of its copy)
    for l in LENGTHS:
        blog = _blog_for(l + 6 * ROUND + 200)

        def fill(S, b, l=l):
            lo, bn = S.block(b)
            t = lo + 3 * ROUND
            S.plant(t, l, 2 * ROUND)
            if l < 24:
                S.add_ballast(t + l + 2 * ROUND + 1 - (t + l - lo) % ROUND)
        out.append(_lz(seed, split, "length", "l%d" % l, blog, fill, exempt="shorter than the minimum match" if l < MINMATCH else None))

    # literal: the run in front of a plant at every Literals_Length code boundary
    for r in LITERALS + (None,):
        blog = 15 if r is None else _blog_for(r + 600)

        def fill(S, b, r=r):
            lo, bn = S.block(b)
            first = lo + 3 * ROUND + 40
            run = r if r is not None else bn - (first + 24 - lo) - 24     # the longest a block of 2^15 leaves behind that sequence
            S.plant(first, 24, 2 * ROUND + 1, back=run > 0)        # the sequence in front: the run begins behind it
            t = first + 24 + run
            # its source: the block's first bytes, or -- the hash table forgets over a long run -- 24 bytes of the run itself
            S.plant(t, 24, t - (lo + 1) if run < 4 * ROUND else 2 * ROUND, front=run > 0)
            if run == 0:
                S.differ(lo, first + 23); S.differ(first + 24 - (2 * ROUND + 1), first + 24)
        out.append(_lz(seed, split, "literal", "ll%s" % ("max" if r is None else r), blog, fill))

    # end: the clamp at the block's end, the zero padding behind it, the last valid start
    for back in (2, 1, 0):
        def fill(S, b, back=back):
            lo, bn = S.block(b)
            t = lo + bn - back - 40
            S.plant(t, 40, t - (lo + 2 * ROUND))
            S.claim(t + 40, "block", b + 1, -back)
        out.append(_lz(seed, split, "end", "ends_bn-%d" % back, 10, fill))

    def cut(S, b):
        lo, bn = S.block(b)
        t = lo + bn - 40
        S.copy(t, 80, t - (lo + 2 * ROUND))                          # the copy goes on for 40 bytes into the next block
        S.plant(t, 40, t - (lo + 2 * ROUND), back=False)
        S.claim(t + 40, "block", b + 1, 0)
    out.append(_lz(seed, split, "end", "cut_at_bn", 10, cut))
    for start in (6, 5, 4):
        def fill(S, b, start=start):
            lo, bn = S.block(b)
            t = lo + bn - start
            if start >= MINMATCH:
                S.plant(t, start, t - (lo + 2 * ROUND))
            else:                                                   # four bytes are left: nothing to code; the cell's plant lies a block on
                S.copy(t, 20, t - (lo + 2 * ROUND))
                S.probes.append((t, 20, t - (lo + 2 * ROUND)))
                lo2, bn2 = S.block(b + 1)
                t2 = lo2 + bn2 - MINMATCH
                S.plant(t2, MINMATCH, t2 - (lo2 + 2 * ROUND))
                S.add_ballast(lo2 + 4 * ROUND)
            S.add_ballast(lo + 4 * ROUND)
            S.claim(t, "block", b + 1, -start)
        out.append(_lz(seed, split, "end", "begins_bn-%d" % start, 10, fill))
    for z in tuple(range(1, 17)):
        def fill(S, b, z=z):
            lo, bn = S.block(b)
            src = lo + 2 * ROUND
            S.fresh(src, 20); S.d[src + 20:src + 20 + 40] = 0        # the source is followed by more zero bytes than the block's end has
            t = lo + bn - z - 20
            S.plant(t, 20 + z, t - src, back=False)
            S.claim(t + 20 + z, "block", b + 1, 0)
        out.append(_lz(seed, split, "end", "zeros%d" % z, 10, fill))

    def all_zero(S, b):
        lo, bn = S.block(b)
        S.d[lo:lo + bn] = 0
        S.lock[lo:lo + bn] = True
        S.probes.append((lo + 1, bn - 1, 1))                         # one byte a block long is an RLE block, whatever the finder makes of it
        lo2, bn2 = S.block(b + 1)                                    # the cell's plant: the block behind ends in zero bytes as well
        src = lo2 + 2 * ROUND
        S.fresh(src, 20); S.d[src + 20:src + 60] = 0
        S.plant(lo2 + bn2 - 28, 28, lo2 + bn2 - 28 - src, back=False)
    out.append(_lz(seed, split, "end", "all_zero", 10, all_zero))
    for n in TINY_LZ + (3 * ROUND + 8,):
        def fill(S, b, n=n):
            if n < 2 * ROUND + MINMATCH + 16:                        # one round, or a second of a few bytes: no sequence pays; decoded only
                S.copy(n - 20, 20, n - 24)
                S.probes.append((n - 20, 20, n - 24))
            else:
                S.plant(2 * ROUND, 40, 2 * ROUND - 4)
        out.append(_lz(seed, split, "end", "tiny", 10, fill, n=n)._replace(name="lz.end.tiny%d" % n))

    # overlap: runs of a short period; the target begins a round (a round sees the rounds in front of it only)
    for p in PERIODS:
        for run in PERIOD_RUNS:
            def fill(S, b, p=p, run=run):
                lo, bn = S.block(b)
                t = lo + 2 * ROUND
                if p > 1:
                    S.differ(t - 1, t - 2)                           # the unit is not itself a shorter period
                S.plant(t, run, p, front=False)
                S.claim(t, "round", b, 2 * ROUND)
                if run < 24:
                    S.add_ballast(lo + 5 * ROUND)
            out.append(_lz(seed, split, "overlap", "p%d_x%d" % (p, run), 12, fill))

    # distance: around every Offset code boundary, and the largest a block has
    for d in DISTANCES + (None,):
        blog = 15 if d is None else _blog_for(d + 400)

        def fill(S, b, d=d):
            lo, bn = S.block(b)
            if d is None:
                d = bn - 24
                t = lo + d
            else:
                t = lo + max(d, 2 * ROUND) + ROUND
            if d > 8 * ROUND:                                        # one byte over and over between the two: nothing the hash table
                S.d[t - d + 24:t] = 0x55                              # could forget the source over
                S.lock[t - d + 24:t] = True
            S.plant(t, 24, d)
        out.append(_lz(seed, split, "distance", "d%s" % ("max" if d is None else d), blog, fill))

    # count: blocks of 0, 1, 127, 128 and 129 sequences; and as many as 5-byte plants a literal apart make
    for k in COUNTS + (None,):
        blog = 12 if k is not None else 15

        def fill(S, b, k=k):
            lo, bn = S.block(b)
            if k is None:                                           # five bytes from 66 back, a literal, five bytes from 66 back, ...: every
                d, at, g = ROUND + 2, lo + 2 * ROUND, []               # source a round away, where the hash table still knows it
                while at + MINMATCH + 1 < lo + bn:
                    S.copy(at, MINMATCH, d)
                    S.plants.append((at, MINMATCH, d)); S.cells.append(None)
                    g.append(at + MINMATCH)
                    at += MINMATCH + 1
                for a in g:                                           # (the literals, once every copy is made: they are copied from too)
                    S.lock[a] = False
                for a in g:
                    S.differ(a, a - d)
                return
            l = 40 if k == 1 else 8
            kk = k
            src, t = lo + 1, lo + 1 + max(kk * l + 3, 2 * ROUND)
            for i in range(kk):                                     # sources side by side, targets a literal apart
                S.plant(t + i * (l + 1), l, t + i * (l + 1) - (src + i * l), front=False, back=False)
            for i in range(kk):
                g = t + i * (l + 1) + l                               # the literal behind target i: not what source i goes on with, and not
                S.d[g] = S.other(int(S.d[src + i * l + l]), int(S.d[src + i * l + l - 1]))     # what lies in front of source i + 1
                S.guards += [(g, src + i * l + l), (g, src + i * l + l - 1)]
            if kk:
                S.differ(src - 1, t - 1)
            if kk == 0:                                             # nothing repeats in this block; the cell's plant lies a block on
                S.probes.append((lo + 1, 0, 1))
                lo2, bn2 = S.block(b + 1)
                S.plant(lo2 + 4 * ROUND, 40, 3 * ROUND)
        out.append(_lz(seed, split, "count", "n%s" % ("max" if k is None else k), blog, fill))

    # independent: a source in the block in front is no source for this stage
    def own_block(S, b):
        lo, bn = S.block(b)
        S.plant(lo + 3 * ROUND, 40, 3 * ROUND, front=False)          # its source is the block's first bytes
        S.claim(lo + 3 * ROUND - 3 * ROUND, "block", b, 0)
    out.append(_lz(seed, split, "independent", "source_at_block_start", 10, own_block))

    def in_front(S, b):
        lo, bn = S.block(b)
        t = lo + 3 * ROUND
        S.fresh(lo - 100, 40)
        S.copy(t, 40, t - (lo - 100)); S.probes.append((t, 40, t - (lo - 100)))
        S.plant(lo + 6 * ROUND, 40, 2 * ROUND)
        S.claim(lo - 100, "block", b, -100)
    out.append(_lz(seed, split, "independent", "source_in_block_in_front", 10, in_front))
    return out


# ---- the lines parser (k_lz_parse_lines) ---------------------------------------------------------------------------------------------------
LINE_CELLS = ("both", "prefix_only", "suffix_only", "equal_join", "suffix_then_prefix", "prefix_of_front", "short_1_2", "long_127_128_129",
              "term0", "term1", "term2", "lines_at_div", "lines_over_div", "mean_at_128", "mean_over_128", "half_at", "half_under")


def _line_block(S, lo, bn, cell, line_div):
    """Fill [lo, lo + bn) with zero-terminated lines of the kind `cell`; a line that does not fit runs on into the next block."""
    rng = S.rng
    nz = lambda n: rng.integers(1, 256, n, dtype=np.uint8)

    def put(pos, line, prev_len, pre=0, suf=0, full=False):
        n = len(line)
        if pos + n > lo + bn:
            return None
        S.d[pos:pos + n] = line
        if pre >= MINMATCH:
            if pre < n:
                S.differ(pos + pre, pos + pre - prev_len)
            S.plants.append((pos, pre, prev_len)); S.cells.append(cell)
        if suf >= MINMATCH:
            S.differ(pos + n - suf - 1, pos - suf - 1)
            S.plants.append((pos + n - suf, suf, n)); S.cells.append(cell)
        S.lock[pos:pos + n] = True
        return pos + n

    P, Q = nz(16), nz(12)
    z = np.zeros(1, np.uint8)
    pos, prev, i = lo, None, 0
    if cell in ("term0", "term1", "term2"):
        S.d[lo:lo + bn] = nz(bn)
        k = int(cell[-1])
        for j in range(k):
            S.d[lo + (j + 1) * bn // (k + 1)] = 0
        S.plant(lo + 6 * ROUND, 64, 3 * ROUND, cell=cell)
        return
    if cell in ("lines_at_div", "lines_over_div"):
        over = cell == "lines_over_div"
        L = bn // line_div + over                                    # bn / line_div lines are the parser's, one more is not
        unit, h = np.concatenate([nz(line_div - 1), z]), line_div // 2
        parts = [np.concatenate([unit[:h - 1], z])] * 2 if over else []          # two lines in the room of one
        nfull = L - 1 - 2 * over
        parts += [unit] * nfull
        used = sum(len(q) for q in parts)
        parts.append(np.concatenate([unit[:line_div - 1], nz(bn - used - line_div), z]))
        S.d[lo:lo + bn] = np.concatenate(parts)
        S.lock[lo:lo + bn] = True
        start = lo + (line_div if over else 0)
        # one line over and over: counted from the block's third round, where the hash table's walk (which has the block when the lines
        # are one too many) has a round in front of it; that walk may take any multiple of the line a round holds as its distance
        S.alts[len(S.plants)] = tuple(line_div * j for j in range(2, ROUND // line_div + 1))
        S.plants.append((lo + 2 * ROUND, start + nfull * line_div + line_div - 1 - (lo + 2 * ROUND), line_div)); S.cells.append(cell)
        return
    if cell in ("mean_at_128", "mean_over_128"):
        L = -(-bn // 128) - (cell == "mean_over_128")
        P = nz(100)
        each = bn // L
        for j in range(L):
            n = each if j + 1 < L else lo + bn - pos
            line = np.concatenate([P, nz(n - 101), z])
            pos = put(pos, line, prev, pre=100 if prev else 0); prev = n
        return
    if cell in ("half_at", "half_under"):
        L = bn // 32
        want = -(-bn // 2) - (cell == "half_under")                 # matched * 2 >= bn keeps the block, one byte less hands it on
        base, extra = divmod(want, L - 1)
        for j in range(L):
            n = 32 if j + 1 < L else lo + bn - pos
            m = base + (1 if j - 1 < extra else 0) if j else 0
            line = np.concatenate([nz(n - 1), z])
            if j:
                line[:m] = S.d[pos - prev:pos - prev + m]
            pos = put(pos, line, prev, pre=m); prev = n
        return
    while True:
        mid = nz(4)
        if cell == "both":
            line, pre, suf = np.concatenate([P, mid, nz(int(rng.integers(0, 3))), Q, z]), 16, 13
        elif cell == "prefix_only":
            line, pre, suf = np.concatenate([P, nz(8 + i % 3), z]), 16, 0
        elif cell == "suffix_only":
            line, pre, suf = np.concatenate([nz(8 + i % 3), Q, z]), 0, 13
        elif cell == "equal_join":
            line, pre, suf = np.concatenate([P, Q, z]), 29, 0
        elif cell == "suffix_then_prefix":                           # equally long lines: the suffix match ends on the terminator at the offset the next prefix has
            line, pre, suf = np.concatenate([P[:6], mid, Q, z]), 6, 13
        elif cell == "prefix_of_front":
            line, pre, suf = (np.concatenate([P, mid, Q, z]), 16, 0) if i % 2 == 0 else (np.concatenate([P, mid[:2], z]), 18, 0)
            if i % 2:
                line[16:18] = S.d[pos - prev + 16:pos - prev + 18]
        elif cell == "short_1_2":
            line, pre, suf = [(np.concatenate([P, mid, Q, z]), 16, 13), (z, 0, 0), (np.concatenate([nz(1), z]), 0, 0), (np.concatenate([P, mid, Q, z]), 0, 0)][i % 4]
        else:                                                       # long_127_128_129
            n = (127, 128, 129)[i % 3]
            if i == 0:
                P = nz(100)
            line, pre, suf = np.concatenate([P, nz(n - 101), z]), 100, 0
        if prev is None:
            pre = suf = 0
        if suf and prev is not None and prev < suf + 1:
            suf = 0
        nxt = put(pos, line, prev, pre=min(pre, len(line)), suf=suf)
        if nxt is None:
            break
        pos, prev, i = nxt, len(line), i + 1
    # the rest of the block: a line that runs on across the seam (its terminator lies in the next block, or nowhere)
    S.d[pos:lo + bn] = nz(lo + bn - pos)


def lines_cases(seed, split="even"):
    out = []
    for blog, nblk in ((13, 68), (15, 64)):
        bs = 1 << blog
        def make(salt, blog=blog, nblk=nblk, bs=bs):
            S = Stream("lines.b%d" % blog, seed, nblk * bs - 37, "direct", bs, split, salt)
            for b in range(len(S.seams) - 1):
                lo, bn = S.block(b)
                _line_block(S, lo, bn, LINE_CELLS[b % len(LINE_CELLS)], 16 if bs > 16384 else 8)
            return S.case("lines", "lines", "blocks", env=lz_env(blog, None))
        c = _drawn(make)
        out.append(c)                                                # the lines parser in front of the hash table's walk, as by default
        out.append(c._replace(name=c.name + ".hash", env=lz_env(blog, "0")))     # and every block by the walk
    return out


# ---- the cross-block stage (k_ldm_insert, k_lzx_parse, k_lzx_seqenc) -----------------------------------------------------------------------
def _lzx(seed, split, cls, cell, wlog, n, fill, route=None, exempt=None):
    route = route or ("direct" if wlog == WINDOW_LOG_DIRECT else "archive")

    def make(salt):
        S = Stream("lzx.%s.%s" % (cls, cell), seed, n, route, lzx_block(wlog, split), split, salt)
        fill(S)
        if route == "direct":
            return S.case("lzx", cls, cell, level=2, wlog=wlog, exempt=exempt)
        return S.case("lzx", cls, cell, long_log=wlog, wlog=wlog, exempt=exempt)
    return _drawn(make)


def _unit(S, at, n):
    S.fresh(at, n, anchored=True)


def lzx_cases(seed, split="even"):
    out = []
    # window: 512 bytes at distance W - 2 .. W + 2, the source on an epoch seam (the table looks at the target's epoch and the one in
    # front of it: a source at W - 1 is in reach only where it begins its epoch), a plant at W / 2 beside it
    for k in WINDOW_LOGS_ARCHIVE + (WINDOW_LOG_DIRECT,):
        W, E = 1 << k, 1 << (k - 1)
        tries = 2 if k == WINDOW_LOG_DIRECT else 4
        stride = 1 if k == WINDOW_LOG_DIRECT else 6              # (an even stride: no target lies on the seam of two blocks of W bytes)
        n = (1 + stride * (tries - 1)) * E + (3 * E + 1400 if stride > 1 else 2 * E + 2000)
        for dl in WINDOW_DELTAS:
            def fill(S, W=W, E=E, dl=dl, tries=tries, stride=stride):
                for i in range(tries):
                    src = (1 + stride * i) * E
                    _unit(S, src, 512)
                    S.plant(src + W + dl, 512, W + dl)
                    S.claim(src, "epoch", src // E, 0)
                    c = src + 600 + (700 * i if stride == 1 else 0) if E >= 2048 else src + W + 600     # the control: W / 2 back, clear of the others
                    _unit(S, c, 512)
                    S.plant(c + E, 512, E, cell="control_w%d" % (W.bit_length() - 1))
            out.append(_lzx(seed, split, "window", "w%d_%+d" % (k, dl), k, n, fill, exempt="distance of W or more" if dl >= 0 else None))

    # epoch: the source at -2 .. +2 of an epoch seam; the target in the same epoch, the next, the one after
    k = 12; W, E = 1 << k, 1 << (k - 1)
    for dl in WINDOW_DELTAS:
        for where, toff in (("same", 1024), ("next", E + 300), ("after", 2 * E + 300)):
            def fill(S, dl=dl, toff=toff):
                src = 3 * E + dl
                _unit(S, src, 256)
                S.plant(3 * E + toff, 256, toff - dl)
                if toff >= 2 * E and dl > 0:                          # and the unit again on that epoch's first bytes: W - dl back, where a
                    S.copy(5 * E, 256, 2 * E - dl)                    # wrong bound of the window would show; the table cannot reach it
                    S.probes.append((5 * E, 256, 2 * E - dl))
                    S.claim(5 * E, "epoch", 5, 0)
                S.claim(src, "epoch", 3, dl); S.claim(3 * E + toff, "epoch", 3 + toff // E, toff % E)
            out.append(_lzx(seed, split, "epoch", "src%+d_%s" % (dl, where), k, 7 * E + 100, fill,
                            exempt="distance of W or more" if toff - dl >= W else None))

    def four_copies(S):
        u = 3 * E + 100
        _unit(S, u, 256)
        S.plant(u + 500, 256, 500); S.plant(u + 1000, 256, 1000, alts=(500,))
        S.plant(4 * E + 1500, 256, E + 1400, alts=(E + 900, E + 400))    # the table kept the first copy; all three lie inside the window
    out.append(_lzx(seed, split, "epoch", "four_copies", k, 7 * E + 100, four_copies))

    # blockseam
    k = 13; W, E = 1 << k, 1 << (k - 1)
    n = 4 * W - 11

    for dl in WINDOW_DELTAS:
        def fill(S, dl=dl):
            t = S.seams[2] + dl
            _unit(S, t - 3000, 300)
            S.plant(t, 300, 3000)
            S.claim(t, "block", 2, dl)
        out.append(_lzx(seed, split, "blockseam", "target%+d" % dl, k, n, fill))

    def across(S):
        t = S.seams[2] - 150
        _unit(S, t - 3000, 300)
        S.plant(t, 300, 3000)
        S.claim(t + 150, "block", 2, 0)
    out.append(_lzx(seed, split, "blockseam", "across", k, n, across))

    def stream_start(S):
        t = S.seams[1] + 500
        _unit(S, 0, 300)
        S.plant(t, 300, t, front=False)                              # nothing lies in front of the stream's first byte
        S.claim(t - t, "block", 0, 0)
    out.append(_lzx(seed, split, "blockseam", "source_at_stream_start", WINDOW_LOG_DIRECT, 3 * 46000, stream_start))

    def to_anchor(S):
        t0 = S.seams[1] + 700
        _unit(S, t0 - 2000, 100)
        S.plant(t0, 100, 2000)                                       # the sequence in front: the anchor is its end
        s1 = t0 + 100 - 3500
        _unit(S, s1, 300)
        S.d[s1 - 20:s1] = S.d[t0 + 80:t0 + 100]                      # the 20 bytes in front of the source equal those in front of the target
        S.lock[s1 - 20:s1] = True
        S.plant(t0 + 100, 300, 3500, front=False)
    out.append(_lzx(seed, split, "blockseam", "back_to_anchor", k, n, to_anchor))

    # streamend
    for n in TINY_LZX:
        def fill(S, n=n):
            _unit(S, 4, 24)
            S.plant(n - 24, 24, n - 28)
            S.claim(n, "block", 1, 0)
        out.append(_lzx(seed, split, "streamend", "n%d" % n, 12, n, fill))
    k = 12; W, E = 1 << k, 1 << (k - 1)
    n = 3 * W - 7

    def target_last(S):
        _unit(S, n - 1500 - 300, 300)
        S.plant(n - 300, 300, 1500)
    out.append(_lzx(seed, split, "streamend", "target_ends_stream", k, n, target_last))

    def source_last(S):                                              # a run of period 7 to the last byte: the source ends 7 bytes short of it
        S.plant(n - 300, 300, 7, front=False)
    out.append(_lzx(seed, split, "streamend", "source_ends_stream", k, n, source_last))
    for j in range(16, 25):
        def fill(S, j=j):
            _unit(S, n - j - 1500, j)
            S.plant(n - j, j, 1500)
            S.claim(n - j, "block", len(S.seams) - 1, -j)
        out.append(_lzx(seed, split, "streamend", "begins_end-%d" % j, k, n, fill))

    # rep: the direct route at level 2 (a window of 2^20, blocks of 2^16); sources in the block in front
    k = WINDOW_LOG_DIRECT
    n = 3 * 46000
    for sub in (1, 2, 3, 4):
        def fill(S, sub=sub):
            t = S.seams[1] + 3000
            d = 40000
            _unit(S, t - d, 2000)
            S.copy(t, 2000, d)
            for at in range(40 - sub, 2000, 40):                     # `sub` substituted bytes close every 40
                for j in range(sub):
                    S.lock[t + at + j] = False
                    S.differ(t + at + j, t + at + j - d)
            for at in range(0, 2000, 40):
                S.plants.append((t + at, 40 - sub, d)); S.cells.append(None)
        out.append(_lzx(seed, split, "rep", "substituted%d" % sub, k, n, fill))

    for name, dists, gap in (("alternate", (30000, 31000), 0), ("rotate", (30000, 31000, 32000), 0), ("minus1", tuple(30000 - i for i in range(24)), 0),
                             ("alternate_lit", (30000, 31000), 1), ("rotate_lit", (30000, 31000, 32000), 1), ("minus1_lit", tuple(30000 - i for i in range(24)), 1)):
        def fill(S, dists=dists, gap=gap):
            t = S.seams[1] + 2000
            for i in range(24):
                d = dists[i % len(dists)]
                at = t + i * (48 + gap)
                S.copy(at, 48, d)
                S.plants.append((at, 48, d)); S.cells.append(None)
            for i in range(24):
                d = dists[i % len(dists)]
                at = t + i * (48 + gap)
                S.differ(at - d - 1, at - 1); S.differ(at + 48 - d, at + 48)
        out.append(_lzx(seed, split, "rep", name, k, n, fill))

    def new_block(S):
        t = S.seams[2] - 400
        _unit(S, t - 35000, 800)
        S.plant(t, 800, 35000)                                       # the block's first sequence repeats the last distance of the block in front
        S.claim(t + 400, "block", 2, 0)
    out.append(_lzx(seed, split, "rep", "first_of_block", k, n, new_block))

    # cap: lengths around 2^16; blocks of exactly 2^16 bytes, so that a match can reach the cap
    for l in CAPS:
        def fill(S, l=l):
            _unit(S, 64, l)
            S.plant(64 + l + 50, l, l + 50)
        nn = 2 * l + 300
        nn = -(-nn // 65536) * 65536
        out.append(_lzx(seed, split, "cap", "l%d" % l, k, nn, fill))

    def thrice(S):
        _unit(S, 0, 70000)
        S.plant(70000, 70000, 70000, front=False, back=False); S.plant(140000, 70000, 70000, front=False, alts=(140000,))
    out.append(_lzx(seed, split, "cap", "unit70000_x3", k, 210000, thrice))

    # tables
    def rle_tables(S):
        lo = S.seams[1]
        dd = (40000, 40002, 40004, 40006)
        for i in range((S.seams[2] - lo) // 50 - 1):                 # every sequence: 10 literals, 40 bytes, a distance of one Offset code
            at = lo + 50 * i + 10
            S.fresh(at - dd[i % 4], 40, anchored=True)
        for i in range((S.seams[2] - lo) // 50 - 1):
            at = lo + 50 * i + 10
            S.copy(at, 40, dd[i % 4])
            S.plants.append((at, 40, dd[i % 4])); S.cells.append(None)
    out.append(_lzx(seed, split, "tables", "one_code_each", k, 2 * 40000, rle_tables))

    def few(S):
        lo = S.seams[1]
        for i in range(3):
            _unit(S, lo + 1000 * i - 20000, 60 + 30 * i)
            S.plant(lo + 1000 * i + 500, 60 + 30 * i, 20500)
    out.append(_lzx(seed, split, "tables", "few_sequences", k, 2 * 40000, few))

    def varied(S):
        at = S.seams[1] + 100
        while at + 200 < S.seams[2]:
            l = int(S.rng.integers(8, 48)); d = int(S.rng.integers(200, 40000))     # sources in this block and in the one in front
            S.plant(at, l, d, front=False, back=False)
            at += l + int(S.rng.integers(0, 16))
    out.append(_lzx(seed, split, "tables", "varied_thousands", k, 3 * 60000, varied))
    return out


def all_cases(seed, split="even", lines=True):
    return lz_cases(seed, split) + (lines_cases(seed, split) if lines else []) + lzx_cases(seed, split)


def coverage_cells(cases):
    """{(class, cell): exempt reason or None} of a list of cases."""
    t = {}
    for c in cases:
        for cell in set(c.cells) | {c.cell}:
            if cell == "blocks":
                continue
            t[(c.cls, cell)] = c.exempt if cell == c.cell else None
    return t


# ---- claims the CPU test holds the plan to -----------------------------------------------------------------------------------------------------
def verify_case(c, split="even"):
    d = np.frombuffer(c.data, dtype=np.uint8)
    assert len(d) <= MAX_STREAM, c.name
    assert c.seams == SPLITS[split](len(d), c.bs), c.name
    for t, l, dist in c.plants + c.probes + c.ballast:
        assert 0 < dist <= t and t + l <= len(d), (c.name, t, l, dist)
        assert np.array_equal(d[t:t + l], d[t - dist:t - dist + l]), (c.name, t, l, dist)
    for a, b in c.guards:
        assert d[a] != d[b], (c.name, a, b)
    if c.route == "archive":
        assert d.min() >= 33 and d.max() <= 126 and not np.isin(d, list(b">@")).any(), c.name
    for pos, kind, index, delta in c.claims:
        if kind in ("block", "round"):
            ref = c.seams[index]
        else:
            ref = index << (c.wlog - 1)
        assert pos == ref + delta, (c.name, pos, kind, index, delta)
    assert c.exempt is None or (c.exempt in EXEMPT_KINDS and c.cls not in NEVER_EXEMPT), c.name


# ---- the checks on a frame ---------------------------------------------------------------------------------------------------------------------
def frame_window_log(frame):
    """Window_Descriptor of a frame with magic (RFC 8878 3.1.1.1.2); these encoders write no Single_Segment frames."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd" and not frame[4] & 0x20, "not a windowed zstd frame"
    assert frame[5] & 7 == 0
    return 10 + (frame[5] >> 3)


def check_decodes(oracle, frame, data):
    try:
        got = oracle.zstd_decompress(frame, len(data) + 16)
    except ValueError as e:
        raise Reject("decode", str(e))
    if got != data:
        k = next((i for i in range(min(len(got), len(data))) if got[i] != data[i]), min(len(got), len(data)))
        raise Reject("decode", "%d bytes for %d, first difference at %d" % (len(got), len(data), k))


def check_window(frame, seqs, wlog=None):
    """No distance beyond the announced window (the reference's streaming decoder keeps a ring of exactly that size), no source in
    front of the stream; wlog: the window the frame has to announce."""
    w = frame_window_log(frame)
    if wlog is not None and w != wlog:
        raise Reject("window", "the frame announces 2^%d, not 2^%d" % (w, wlog))
    if len(seqs):
        k = int(np.argmax(seqs.distance))
        if seqs.distance[k] > (1 << w):
            raise Reject("window", "distance %d at %d under a window of 2^%d" % (seqs.distance[k], seqs.pos[k], w))
        if (seqs.distance > seqs.pos).any():
            raise Reject("window", "a source in front of the stream")


def check_independent(seqs, seams=None):
    """Frames of the in-block stage: no source in front of its own block (the block starts are the frame's own)."""
    starts = np.concatenate([[0], np.cumsum(seqs.block_size)])[:-1] if seams is None else np.asarray(seams[:-1])
    if len(seqs):
        bad = np.nonzero(seqs.pos - seqs.distance < starts[seqs.block])[0]
        if len(bad):
            k = int(bad[0])
            raise Reject("dependent", "the match at %d reaches %d bytes back, in front of its block at %d" % (seqs.pos[k], seqs.distance[k], starts[seqs.block[k]]))


def check_first_offsets(seqs):
    """Frames of the cross-block stage: a block knows nothing of the repeat offsets in front of it, so its first sequence is a new offset."""
    if len(seqs):
        first = np.concatenate([[True], seqs.block[1:] != seqs.block[:-1]])
        bad = np.nonzero(first & (seqs.offset_value <= 3))[0]
        if len(bad):
            raise Reject("repeat", "the first sequence of block %d is repeat code %d" % (seqs.block[bad[0]], seqs.offset_value[bad[0]]))


def check_probes(c, seqs):
    """What PROBE_CELLS says of the cell, on a frame of the kernels (the serial models take matches of four bytes and weigh nothing)."""
    what = PROBE_CELLS.get((c.cls, c.cell))
    if what is None or what == "window":
        return
    starts = np.asarray(c.seams)
    for t, l, d in c.probes:
        b = int(np.searchsorted(starts, t, "right")) - 1
        lo, hi = c.seams[b], c.seams[b + 1]
        if what == "no sequence begins":
            k = np.nonzero((seqs.pos >= t) & (seqs.pos < min(t + l, hi)))[0]
            if len(k):
                raise Reject("probe", "%s: a sequence begins at %d, inside the probe at %d" % (c.name, seqs.pos[k[0]], t))
        elif what == "RLE block":
            if seqs.block_type[b] != 1:
                raise Reject("probe", "%s: block %d of one byte over and over has type %d" % (c.name, b, seqs.block_type[b]))
        elif what == "no sequence in the block":
            if (seqs.block == b).any():
                raise Reject("probe", "%s: block %d holds %d sequences" % (c.name, b, int((seqs.block == b).sum())))
    if what == "no sequence in the frame" and c.probes and len(seqs):
        raise Reject("probe", "%s: %d sequences in a stream of %d bytes" % (c.name, len(seqs), len(c.data)))


def lines_kept(c, seqs):
    """Per block of a lines case: does every sequence look like the lines parser's -- it begins on a line's first byte with the length
    of the line in front as its distance, or it ends on a line's last byte with the line's own length?  (Blocks without a sequence:
    None.)  The hash table's walk begins where its rounds let it and takes what distance it finds; a block of one line over and
    over looks the same by either path."""
    d = np.frombuffer(c.data, dtype=np.uint8)
    ends = np.nonzero(d == 0)[0]
    out = []
    for b in range(len(c.seams) - 1):
        m = seqs.block == b
        if not m.any():
            out.append(None); continue
        pos, ml, dist = seqs.pos[m], seqs.ml[m], seqs.distance[m]
        lo = c.seams[b]
        i = np.searchsorted(ends, pos, "left")                        # the line that holds pos ends at ends[i]
        start = np.where(i > 0, ends[np.maximum(i - 1, 0)] + 1, 0); start = np.maximum(start, lo)
        prev_start = np.where(i > 1, ends[np.maximum(i - 2, 0)] + 1, 0); prev_start = np.maximum(prev_start, lo)
        j = np.searchsorted(ends, pos + ml - 1, "left"); j = np.minimum(j, len(ends) - 1)
        own_start = np.maximum(np.where(j > 0, ends[np.maximum(j - 1, 0)] + 1, 0), lo)
        prefix = (pos == start) & (dist == start - prev_start)
        suffix = (pos + ml - 1 == ends[j]) & (dist == ends[j] + 1 - own_start)
        out.append(bool((prefix | suffix).all()))
    return out


def check_size(frame, plain):
    if len(frame) > len(plain):
        raise Reject("larger", "%d bytes with the match finder, %d without" % (len(frame), len(plain)))


def check_split(seqs, seams):
    want = np.diff(np.asarray(seams))
    if len(seqs.block_size) != len(want) or not np.array_equal(seqs.block_size, want):
        raise Reject("plan out of date", "the frame's blocks are %s..., the plan's split %s..." % (list(seqs.block_size[:4]), list(want[:4])))


def found(c, seqs):
    """Per plant: do sequences with the plant's distance (or one of its alternatives) cover its bytes from target_begin + 3 to its end?
    A plant longer than a sequence can be -- one that crosses a block seam or passes the 16-bit cap -- is covered by several; the byte a
    block of 2^16 has beyond the cap is not asked for."""
    by_d = {}
    order = np.argsort(seqs.pos, kind="stable")
    pos, end, dist = seqs.pos[order], (seqs.pos + seqs.ml)[order], seqs.distance[order]
    for dv in np.unique(dist):
        m = dist == dv
        by_d[int(dv)] = (pos[m], end[m])
    holes = [lo + LEN_CAP for lo, hi in zip(c.seams[:-1], c.seams[1:]) if hi - lo > LEN_CAP]
    out = np.zeros(len(c.plants), dtype=bool)
    for i, (t, l, d) in enumerate(c.plants):
        a, b = t + min(3, l - 1), t + l
        iv = []
        for dv in (d,) + tuple(c.alts.get(i, ())):
            if dv in by_d:
                p, e = by_d[dv]
                lo_i, hi_i = np.searchsorted(e, a, "right"), np.searchsorted(p, b, "left")
                iv += list(zip(p[lo_i:hi_i], e[lo_i:hi_i]))
        iv.sort()
        at = a
        for p, e in iv:
            while at in holes and p > at:
                at += 1
            if p > at:
                break
            at = max(at, int(e))
        while at in holes:
            at += 1
        out[i] = at >= b
    return out


class Tally:
    """The coverage table: found / total per (class, cell), and what the frames held."""

    def __init__(self):
        self.cell, self.exempt = {}, {}
        self.rep = {(v, z): 0 for v in (1, 2, 3) for z in ("ll0", "ll")}
        self.modes = {}                                               # class -> [LL, OF, ML][predefined, rle, fse, repeat]
        self.longest_match = self.longest_literals = 0
        self.first_ll0 = 0
        self.stage = {}
        self.kept = {}                                                # lines cell -> {run: [blocks that look like the lines parser's, blocks with sequences]}
        self.over_plain = {}                                          # class -> most bytes a frame had over the same call without the match finder

    def add_plain(self, c, frame, plain):
        self.over_plain[c.cls] = max(self.over_plain.get(c.cls, -(1 << 30)), len(frame) - len(plain))

    def add(self, c, seqs, info=None):
        f = found(c, seqs)
        for (cell, ok) in zip(c.cells, f):
            a = self.cell.setdefault((c.cls, cell), [0, 0])
            a[0] += int(ok); a[1] += 1
            if cell == c.cell:
                self.exempt[(c.cls, cell)] = c.exempt
        self.cell.setdefault((c.cls, c.cell), [0, 0]) if c.cell != "blocks" else None
        s = self.stage.setdefault(c.stage, [0, 0])
        s[0] += int(f.sum()); s[1] += len(f)
        if len(seqs):
            for v in (1, 2, 3):
                m = seqs.offset_value == v
                self.rep[(v, "ll0")] += int((m & (seqs.ll == 0)).sum()); self.rep[(v, "ll")] += int((m & (seqs.ll > 0)).sum())
            self.longest_match = max(self.longest_match, int(seqs.ml.max())); self.longest_literals = max(self.longest_literals, int(seqs.ll.max()))
            first = np.concatenate([[True], seqs.block[1:] != seqs.block[:-1]])
            self.first_ll0 += int((first & (seqs.ll == 0) & (seqs.pos > 0)).sum())
        if c.stage == "lines":
            run = "walk only" if c.env.get("NAF_GPU_LZ_LINES") == "0" else "default"
            for b, k in enumerate(lines_kept(c, seqs)):
                a = self.kept.setdefault(LINE_CELLS[b % len(LINE_CELLS)], {}).setdefault(run, [0, 0])
                a[0] += int(bool(k)); a[1] += int(k is not None)
        if info is not None:
            m = self.modes.setdefault(c.cls, np.zeros((3, 4), dtype=np.int64))
            m += np.array([[info.mode_count[t][k] for k in range(4)] for t in range(3)])
        return f

    def empty_cells(self):
        return sorted(k for k, (f, n) in self.cell.items() if f == 0 and not self.exempt.get(k))

    def table(self, title):
        rows = ["%s: found / planted per cell (seeds %s)" % (title, ", ".join(map(str, SEEDS)))]
        for cls in sorted({k[0] for k in self.cell}):
            cells = ["%s %d/%d%s%s" % (k[1], f, n, " (exempt: %s)" % self.exempt[k] if self.exempt.get(k) else "",
                                       " (a neighbour's; the probe: %s)" % PROBE_CELLS[k] if k in PROBE_CELLS else "")
                     for k, (f, n) in sorted(self.cell.items()) if k[0] == cls]
            rows.append("  %-12s %s" % (cls, "; ".join(cells)))
            if cls in self.modes:
                rows.append("  %-12s table modes [predefined, rle, fse, repeat]: LL %s OF %s ML %s" % ("", *(list(map(int, r)) for r in self.modes[cls])))
        if self.kept:
            rows.append("  lines: blocks whose every sequence is a line's prefix or suffix at the line's distance / blocks with sequences, by default and with NAF_GPU_LZ_LINES=0:")
            rows.append("    " + "; ".join("%s %s" % (cell, ", ".join("%d/%d %s" % (a[0], a[1], run) for run, a in sorted(v.items()))) for cell, v in sorted(self.kept.items())))
        if self.over_plain:
            rows.append("  most bytes over the SAME call with NAF_GPU_LZ=0 (which cuts 32 KiB blocks under a window of 2^19): " + ", ".join("%s %+d" % kv for kv in sorted(self.over_plain.items())))
        rows.append("  per stage: " + ", ".join("%s %d/%d (%.1f %%)" % (k, f, n, 100.0 * f / max(n, 1)) for k, (f, n) in sorted(self.stage.items())))
        rows.append("  repeat codes: " + ", ".join("value %d %s: %d" % (v, "with ll == 0" if z == "ll0" else "with ll > 0", self.rep[(v, z)]) for v in (1, 2, 3) for z in ("ll0", "ll")))
        rows.append("  longest match %d, longest literal run %d, first sequences of a block with literal length 0: %d" % (self.longest_match, self.longest_literals, self.first_ll0))
        return "\n".join(rows)

    def floor(self, need_reps=True, need_cap=True):
        """What is asserted about coverage: a floor, not a rate."""
        assert not self.empty_cells(), "cells without a found plant: %s" % self.empty_cells()
        if need_reps:
            missing = [k for k, v in self.rep.items() if v == 0]
            assert not missing, "repeat variants never seen: %s" % missing
        if need_cap:
            assert self.longest_match == LEN_CAP, "longest match %d, not %d" % (self.longest_match, LEN_CAP)
            assert self.first_ll0 > 0, "no block begins with a match"
