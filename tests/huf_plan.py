"""The plan of the literals-planner tests (test_huf_plan_cpu.py holds it to its claims and runs it through the host build of the
planner, test_gpu_huf_plan.py runs it on the kernels): blocks whose HISTOGRAM and PLACEMENT are planted on every edge of the zstd
encoder's entropy stage (naf_amd/csrc/zstd_enc.hip: k_zenc_plan, k_zenc_tree, k_zenc_flat_scan, k_zenc_frame_*; zstd_enc_core.h:
huf_lengths_sorted, huf_write_tree_w, zenc_plan_finish), models of what that stage documents, in exact integers, and the checks a
frame made of such blocks has to pass block by block (from oracle.zstd_literals).  Pure Python and numpy; nothing here comes from the
code under test.

A CELL is one block: counts (a profile), the symbols that carry them (an alphabet rule) and a placement.  A CASE packs cells into one
stream, one cell per block of the encoder's even split (lz_plan.split_even, shared, not copied); every block of a case has the same
length bn, so n = nblk * bn and the split is the same whether blocks are cut evenly or on multiples of bn (the host build's way).
NAF_TEST_SEED moves the letters (which symbols carry the counts, where the bytes lie inside their quarter), never the structure.

A CARRIER brings a stream to one parameter set of the planner (read from zstd_encode_begin and enc.hip):

    z1    Context.zstd_compress(level=1)                       11 bits, direct weights where the format allows them
    z2    level=2 with NAF_GPU_LZ=0                            11 bits, FSE-coded weights tried
    qual  ennaf of a FASTQ, its quality stream                 7 bits up to 64 symbols and 9 above, symbols 33..126, the frame's tree
    mask  ennaf of a FASTA, its mask stream                    9 bits, an eighth of gain wanted, `mine + 16 >= bn` stays Raw; units 1..255
    seq   ennaf of a FASTA, its packed sequence stream         7 / 9 bits, flat preference 1/16, the flat scan, the frame's tree
    emul  tests/emul emul_zstd_compress (no GPU)               zenc_plan_block: 11 bits, FSE tried

NAF_GPU_BLOCK_LOG sets the block size of every carrier.  What a carrier cannot reach it says in EXEMPT, and the table prints it.

Paths, as the table names them (the MODEL says which path a block takes; the GPU test proves the launches from Context.get_timing and
the treeless sections from the oracle): F flat shortcut, R register construction (up to 64 symbols), S serial routine, L length
limiting ran, P flat preferred, Q settled by the flat scan, C weights found in the sampled cache, M looked up and missed, D tree
description deferred to k_zenc_tree, T coded with the frame's code, W Raw, E RLE.

Out of this plan's reach: the sequences section's FSE tables (zenc_write_sequences_x, fse_normalize as the sequence tables use it,
zenc_fse_cost) -- every carrier here runs without the match finder; tests/seq_plan.py holds them to a model of their own, block by
block.  The next gap: the literals of a block that DOES carry sequences (the second k_zenc_plan over the match finder's literal
buffer, with per-block lengths and no cache, and k_lz_choose's weighing of the two plans) are held by no model -- seq_plan.py looks at
such a block's sequences section and at its size against the literal-only block, not at its Huffman code; and the direct blocks of a
one-pass FASTA (k_zenc_direct_plans), which zstd_encode_begin refuses next to NAF_GPU_BLOCK_LOG and which need 8 MiB of packed bases."""
import heapq
import zlib
from collections import namedtuple

import numpy as np

from lz_plan import SEED, SEEDS, Reject, split_even            # the even split is lz_plan's: shared, not copied

MAX_STREAM = 6 << 20
PAIR_CODES = tuple(h << 4 | l for h in (1, 2, 4, 8) for l in (1, 2, 4, 8))      # packed A C G T pairs: both nibbles one-hot
FLAT16 = np.zeros(256, dtype=np.int64)
FLAT16[list(PAIR_CODES)] = 4


# ---- models -------------------------------------------------------------------------------------------------------------------------
def huffman_cost(hist):
    """sum(count * length) of an optimal prefix code: a heap construction."""
    h = [int(c) for c in hist if c]
    if len(h) < 2:
        return 0
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    return cost


def limited_cost(hist, L):
    """sum(count * length) of an optimal code with no length above L: package-merge (the cost is the weight of the 2n - 2 cheapest
    items of the last list).  None when 2^L codes do not hold the alphabet."""
    w = sorted(int(c) for c in hist if c)
    n = len(w)
    if n < 2:
        return 0
    if (1 << L) < n:
        return None
    pk = []
    for _ in range(L - 1):
        m = sorted(w + pk)
        pk = [m[i] + m[i + 1] for i in range(0, len(m) - 1, 2)]
    return sum(sorted(w + pk)[:2 * n - 2])


def fixed_width_cost(hist):
    n = sum(1 for c in hist if c)
    return int(sum(hist)) * max(1, (n - 1).bit_length())


def two_queue_depths(w):
    """Depths of the leaves of the two-queue construction over ascending weights; on a tie a leaf is taken before a node."""
    n = len(w)
    wt, parent = list(w) + [0] * (n - 1), [0] * (2 * n - 1)
    leaf, inode, nxt = 0, n, n
    while (n - leaf) + (nxt - inode) > 1:
        pick = []
        for _ in range(2):
            if leaf < n and (inode >= nxt or wt[leaf] <= wt[inode]):
                pick.append(leaf)
                leaf += 1
            else:
                pick.append(inode)
                inode += 1
        wt[nxt] = wt[pick[0]] + wt[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nxt
        nxt += 1
    depth = [0] * (2 * n - 1)
    for i in range(nxt - 2, -1, -1):
        depth[i] = depth[parent[i]] + 1
    return depth[:n]


def plan_lengths(hist, L):
    """The construction the encoder documents: symbols sorted by (count, symbol), the two-queue merge, lengths clamped to L, the rarest
    symbols lengthened (a pass over all of them, one bit each) until the Kraft sum is no more than 1, the most frequent that fit
    shortened until it is 1.  Returns (256 lengths, the largest, the unlimited depth); (zeros, 0, depth) when that does not end at 1."""
    order = sorted((s for s in range(256) if hist[s]), key=lambda s: (int(hist[s]), s))
    n, lens = len(order), [0] * 256
    if n < 2:
        return lens, 0, 0
    l = two_queue_depths([int(hist[s]) for s in order])
    depth = max(l)
    if depth > L:
        l = [min(x, L) for x in l]
        K, full = sum(1 << (L - x) for x in l), 1 << L
        while K > full:
            grew = False
            for i in range(n):
                if K <= full:
                    break
                if l[i] < L:
                    K -= 1 << (L - l[i] - 1)
                    l[i] += 1
                    grew = True
            if not grew:
                return lens, 0, depth
        while K < full:
            moved = False
            for i in range(n - 1, -1, -1):
                if K >= full:
                    break
                if l[i] > 1 and K + (1 << (L - l[i])) <= full:
                    K += 1 << (L - l[i])
                    l[i] -= 1
                    moved = True
            if not moved:
                break
        if K != full:
            return lens, 0, depth
    for s, x in zip(order, l):
        lens[s] = x
    return lens, max(l), depth


def direct_tree_bytes(n_weights):
    """Header byte 127 + n, then a nibble per weight."""
    return 1 + (n_weights + 1) // 2


def quarter_bounds(bn):
    """The four streams of a block: per = (bn + 3) // 4 bytes each, the last one what is left."""
    per = (bn + 3) // 4
    return [min(k * per, bn) for k in range(4)] + [bn]


def hist4_of(block):
    """The four quarter histograms of a block's bytes (4 x 256)."""
    b = np.frombuffer(bytes(block), dtype=np.uint8)
    q = quarter_bounds(len(b))
    return np.stack([np.bincount(b[q[k]:q[k + 1]], minlength=256) for k in range(4)]).astype(np.int64)


def stream_bytes(h4, lens):
    """ceil((bits + 1) / 8) per quarter: the code's bits and the end mark."""
    bits = h4 @ np.asarray(lens, dtype=np.int64)
    return [int((b + 1 + 7) // 8) for b in bits]


def lit_header_bytes(regen, comp):
    return 3 if regen < 1024 and comp < 1024 else 4 if regen < 16384 and comp < 16384 else 5


# ---- carriers -----------------------------------------------------------------------------------------------------------------------------
Params = namedtuple("Params", "name limit min_gain try_fse prefer_flat flat_scan frame_tree alphabet route")
CARRIERS = {
    "z1": Params("z1", 11, 0, False, 0, False, False, tuple(range(256)), "direct"),
    "z2": Params("z2", 11, 0, True, 0, False, False, tuple(range(256)), "direct"),
    "qual": Params("qual", 7, 0, False, 0, False, True, tuple(range(33, 127)), "fastq"),
    "mask": Params("mask", 9, 32, False, 0, False, False, tuple(range(1, 256)), "fasta_mask"),
    "seq": Params("seq", 7, 0, False, 16, True, True, tuple(range(256)), "fasta_seq"),
    "emul": Params("emul", 11, 0, True, 0, False, False, tuple(range(256)), "emul"),
}
GPU_CARRIERS = ("z1", "z2", "qual", "mask", "seq")
FRAME_BLOCKS = 4096               # 16 * ZENC_CACHE_ENTRIES: the sampled cache, the frame's tree, k_zenc_frame_quick
DEFER_BLOCKS = 256                # k_zenc_tree
FRAME_BLOCK = 32768               # ZENC_FRAME_BLOCK: the block the frame's code is made of


def limit_of(P, distinct):
    """The length limit in force: above 64 symbols the serial routine runs with at least 9 bits (7 would not hold every alphabet)."""
    return P.limit if distinct <= 64 else max(P.limit, 9)


Model = namedtuple("Model", "kind lens log depth limit ssz lastw tb_lo tb_hi csize_lo csize_hi path distinct")
# kind: "rle" | "raw" | "huf" | "either" (the description's size, which only the encoder's FSE coder knows, decides)


def code_of(hist, bn, P):
    """(lens, log, depth, limit, path letters) of a block of at least 64 bytes and two symbols: the three constructions as one rule."""
    present = [int(c) for c in hist if c]
    distinct = len(present)
    limit = limit_of(P, distinct)
    pow2 = distinct & (distinct - 1) == 0
    two = sorted(present)[:2]
    if pow2 and two[0] + two[1] > max(present):
        k = distinct.bit_length() - 1
        return [k if c else 0 for c in hist], k, k, limit, "F"
    lens, log, depth = plan_lengths(hist, limit)
    path = ("R" if distinct <= 64 else "S") + ("L" if depth > limit else "")
    if P.prefer_flat and log and pow2:
        k = distinct.bit_length() - 1
        hb, fb = sum(int(c) * l for c, l in zip(hist, lens)), bn * k
        if fb >= hb and (fb - hb) * P.prefer_flat < fb:
            return [k if c else 0 for c in hist], k, depth, limit, path + "P"
    return lens, log, depth, limit, path


def model_block(h4, P):
    """What the planner documents for a block with these quarter histograms."""
    hist = h4.sum(axis=0)
    bn, distinct = int(hist.sum()), int((hist > 0).sum())
    none = dict(lens=[0] * 256, log=0, depth=0, limit=0, ssz=None, lastw=0, tb_lo=0, tb_hi=0, csize_lo=3 + bn, csize_hi=3 + bn, distinct=distinct)
    if bn and distinct == 1:
        return Model(kind="rle", path="E", **dict(none, csize_lo=4, csize_hi=4))
    if bn < 64:
        return Model(kind="raw", path="W", **none)
    if P.min_gain and int(hist.max()) + 16 >= bn:                  # the mask's own rule: one unit but for a few bytes stays Raw
        return Model(kind="raw", path="W", **none)
    lens, log, depth, limit, path = code_of(hist, bn, P)
    if not log:
        return Model(kind="raw", path=path + "W", **none)
    ssz = stream_bytes(h4, lens)
    lastw = max(s for s in range(256) if hist[s])
    direct = direct_tree_bytes(lastw)
    if not P.try_fse and lastw <= 128:
        tb_lo = tb_hi = direct
    elif lastw <= 128:
        tb_lo, tb_hi = 3, direct                                    # FSE-coded only where that is smaller
    else:
        tb_lo, tb_hi = 3, 128                                       # FSE-coded or not at all: a description of 128 bytes or more cannot be written

    def size(tb):
        body = tb + 6 + sum(ssz)
        return 3 + lit_header_bytes(bn, body) + body + 1

    gain = (bn * P.min_gain) >> 8
    lo, hi = size(tb_lo), size(tb_hi)
    if max(ssz) > 0xFFFF:
        kind = "raw"
    elif hi + gain < 3 + bn:
        kind = "huf"
    elif lo + gain >= 3 + bn:
        kind = "raw"
    else:
        kind = "either"
    return Model(kind, lens, log, depth, limit, ssz, lastw, tb_lo, tb_hi, lo, hi, path + ("W" if kind == "raw" else ""), distinct)


def frame_code_model(sampled_hists, P):
    """The frame's code: the sum of the sampled blocks' histograms scaled to ZENC_FRAME_BLOCK - 256 bytes, every symbol that occurred
    at least once; then the planner's construction without the flat preference."""
    tot = np.sum(sampled_hists, axis=0).astype(np.int64)
    s = int(tot.sum())
    cnt = [max(1, int(h) * (FRAME_BLOCK - 256) // s) if h else 0 for h in tot]
    Q = P._replace(prefer_flat=0)
    lens, log, depth, limit, path = code_of(cnt, sum(cnt), Q)
    return lens, log, limit


def frame_rule(hist, flen, ratio):
    """Whether a block takes the frame's code, and by what margin: the code covers its symbols and costs no more than 3 % (+ 8 bytes)
    above `ratio` / 1024 of the block's own entropy -- ratio is what the frame's code loses on the histogram it was made of, clamped
    to [1024, 1229].  Returns (takes it, |cost - bound| / bound); the kernel's entropies are single-precision."""
    import math
    hist = np.asarray(hist, dtype=np.int64)
    if (np.asarray(flen)[hist > 0] == 0).any():
        return False, 1.0
    bn = int(hist.sum())
    fbits = int((hist * np.asarray(flen)).sum())
    ebits = sum(int(int(h) * math.log2(bn / int(h)) + 0.5) for h in hist if h)
    lhs, rhs = fbits * 1024 * 100, ebits * ratio * 103 + 6400 * 1024
    return lhs <= rhs, abs(lhs - rhs) / rhs


def frame_ratio(sampled_hists, flen):
    import math
    tot = np.sum(sampled_hists, axis=0).astype(np.int64)
    s = int(tot.sum())
    e = sum(int(int(h) * math.log2(s / int(h)) + 0.5) for h in tot if h)
    r = int((tot * np.asarray(flen)).sum()) * 1024 // e if e else 1024
    return min(1229, max(1024, r))


# ---- profiles: counts that sum to bn, most frequent first ---------------------------------------------------------------------------------
def _fit(weights, bn):
    """Integer counts in proportion to the weights, every one at least 1, summing to bn; the order of the weights is kept."""
    w = [float(x) for x in weights]
    n, tot = len(w), sum(w)
    assert n <= bn
    c = [max(1, int(bn * x / tot)) for x in w]
    d = bn - sum(c)
    i = 0
    while d != 0:
        k = i % n
        if d > 0:
            c[k] += 1
            d -= 1
        elif c[k] > 1:
            c[k] -= 1
            d += 1
        i += 1
    return c


def prof_equal(n, bn):
    return [bn // n + (1 if i < bn % n else 0) for i in range(n)]


def prof_pow2(n, bn):
    """2^-i: 1, 1, 2, 4, ... (depth n - 1) scaled up by a power of two as far as bn allows, what is left to the commonest symbol.
    Where the block is too short for the true counts (from the fourteenth symbol on, in this plan) the rarest symbols occur once."""
    base = [1, 1] + [1 << i for i in range(1, n - 1)]
    if sum(base) > bn:
        c = _fit([2.0 ** -i for i in range(n)], bn)
    else:
        k = (bn // sum(base)).bit_length() - 1
        c = [x << k for x in base]
    c = sorted(c, reverse=True)
    c[0] += bn - sum(c)
    return c


def prof_geo(n, bn, r=0.7):
    return _fit([r ** i for i in range(n)], bn)


def prof_fib(n, bn):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    f = f[:n][::-1]
    assert sum(f) <= bn, (n, bn)
    k = bn // sum(f)
    c = [x * k for x in f]
    c[0] += bn - sum(c)
    return c


def prof_pairs(n, bn):
    """Pairs of equal counts: n / 2 levels of a linear ramp, each twice."""
    half = (n + 1) // 2
    w = [half - i // 2 for i in range(n)]
    c = _fit(w, bn - bn % 2)
    for i in range(0, n - 1, 2):                                  # make each pair exactly equal
        s = c[i] + c[i + 1]
        c[i] = c[i + 1] = s // 2
    c[0] += bn - sum(c)
    return c


def prof_dominant(k, bn):
    return [bn - k] + [1] * k


def prof_linear(n, bn):
    return _fit([n - i for i in range(n)], bn)


def prof_quadratic(n, bn):
    return _fit([(n - i) ** 2 for i in range(n)], bn)


def prof_edge(n, bn, delta):
    """The flat shortcut's edge: the two rarest symbols a bytes each, the commonest 2 a + delta, the n - 3 others between them."""
    assert n >= 4
    a = (2 * (bn - delta)) // (3 * n - 1)
    top = 2 * a + delta
    mid = prof_equal(n - 3, bn - top - 2 * a)
    c = [top] + mid + [a, a]
    assert sum(c) == bn and all(a <= m <= top for m in mid) and a > 0, (n, bn, delta, c)
    return c


# ---- cells ------------------------------------------------------------------------------------------------------------------------------------
Cell = namedtuple("Cell", "cls name counts rule place")
# rule: how the symbols are chosen -- ("any", span) with span "low" (at most index 128: direct weights) or "full"; ("last", index): the
#   largest present symbol is that index; ("ends",): symbols 0 and 255 both present; ("pairs",): the packed pair codes first
# place: "shuffle" | ("only_quarter", q) | ("quarter_first", q) | ("quarter_last", q) | ("block_last",) | ("marker", residue): the first
#   quarter's bits under the model's lengths are residue mod 8; the rule applies to the RAREST symbol of the counts
ALPHABET_SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)
LAST_INDICES = (127, 128, 129, 255)
POW2_SIZES = (8, 9, 12, 13, 40, 64)
PACK_BN = 4096
SEAM_BNS = (1001, 1002, 1003)     # 4k + 1, 2, 3 with per = 251: the histogram's 8-byte words straddle every quarter seam
LENGTHS = (1, 63, 64, 65, 255, 256, 1023, 1024, 1025, 16383, 16384, 16385, 32768, 131072)
BIG_BN = 1024


def pack_cells(bn=PACK_BN):
    """The alphabet and profile cells: one block each, any length."""
    cells = []
    for n in ALPHABET_SIZES:
        span = "low" if n <= 100 else "full"
        cells.append(Cell("alphabet", "equal_%d" % n, prof_equal(n, bn), ("any", span), "shuffle"))
        if n >= 3:
            cells.append(Cell("alphabet", "linear_%d" % n, prof_linear(n, bn), ("any", "full" if n > 100 or n % 2 else "low"), "shuffle"))
    for last in LAST_INDICES:
        cells.append(Cell("alphabet", "last_at_%d" % last, prof_geo(20, bn), ("last", last), "shuffle"))
    cells.append(Cell("alphabet", "0_and_255", prof_linear(12, bn), ("ends",), "shuffle"))
    for n in (4, 8, 16, 32, 64):
        for d, nm in ((0, "equal"), (-1, "below"), (1, "above")):
            cells.append(Cell("profile", "edge_%d_%s" % (n, nm), prof_edge(n, bn, d), ("any", "low"), "shuffle"))
    for n in POW2_SIZES:
        cells.append(Cell("profile", "pow2_%d" % n, prof_pow2(n, bn), ("any", "low"), "shuffle"))
    for n in (10, 30, 60, 90):
        cells.append(Cell("profile", "geo0.7_%d" % n, prof_geo(n, bn), ("any", "low" if n < 60 else "full"), "shuffle"))
    for n in (8, 12, 15, 16):
        cells.append(Cell("profile", "fib_%d" % n, prof_fib(n, bn), ("any", "low"), "shuffle"))
    for n in (6, 24, 64, 80):
        cells.append(Cell("profile", "pairs_%d" % n, prof_pairs(n, bn), ("any", "low" if n < 80 else "full"), "shuffle"))
    for k in (15, 16, 17, 40, 200):
        cells.append(Cell("profile", "dominant_%d" % k, prof_dominant(k, bn), ("any", "low" if k < 100 else "full"), "shuffle"))
    for n in (20, 70, 200):
        cells.append(Cell("profile", "quadratic_%d" % n, prof_quadratic(n, bn), ("any", "low" if n < 100 else "full"), "shuffle"))
    # the flat preference (the sequence carrier's) and the flat scan: the sixteen pair codes
    cells.append(Cell("flat", "pairs16_uniform", prof_equal(16, bn), ("pairs",), "shuffle"))
    cells.append(Cell("flat", "pairs15_uniform", prof_equal(15, bn), ("pairs",), "shuffle"))
    cells.append(Cell("flat", "pairs16_skewed", prof_geo(16, bn, 0.8), ("pairs",), "shuffle"))
    below, above = flat_edge(bn)
    cells.append(Cell("flat", "sixteenth_not_saved", below, ("any", "low"), "shuffle"))
    cells.append(Cell("flat", "sixteenth_saved", above, ("any", "low"), "shuffle"))
    return cells


def flat_edge(bn):
    """Two histograms of sixteen symbols on either side of the flat preference's threshold: Huffman coding saves just less than, and
    at least, a sixteenth of the four bits per symbol.  Mass moves from the fifteen others to one symbol until the rule flips."""
    P = CARRIERS["seq"]
    last = None
    for d in range(0, bn - 16 * 8, 4):
        rest = prof_equal(15, bn - bn // 16 - d)
        c = [bn // 16 + d] + rest
        path = code_of(c + [0] * 240, bn, P)[4]
        if "F" in path:
            continue
        if "P" not in path:
            assert last is not None
            return last, c
        last = c
    raise AssertionError("no edge")


def seam_cells(bn):
    """Placement cells of a block whose quarters do not end on 8-byte words."""
    cells = []
    base = prof_geo(12, bn - 1) + [1]                             # the rarest symbol occurs once: the placed one
    for q in range(4):
        cells.append(Cell("seam", "first_byte_of_quarter_%d" % q, base, ("any", "low"), ("quarter_first", q)))
        cells.append(Cell("seam", "last_byte_of_quarter_%d" % q, base, ("any", "full"), ("quarter_last", q)))
    several = prof_geo(12, bn - 9) + [9]
    for q in range(4):
        cells.append(Cell("seam", "only_in_quarter_%d" % q, several, ("any", "low"), ("only_quarter", q)))
    for r, nm in ((7, "8m-1"), (0, "8m"), (1, "8m+1")):
        cells.append(Cell("seam", "marker_bits_%s" % nm, prof_linear(9, bn), ("any", "low"), ("marker", r)))
    cells.append(Cell("seam", "shuffled", prof_linear(40, bn), ("any", "full"), "shuffle"))
    return cells


def length_cells(bn):
    if bn == 1:
        return [Cell("length", "bn_1", [1], ("any", "low"), "shuffle")]
    cells = [Cell("length", "bn_%d_geo8" % bn, prof_geo(8, bn), ("any", "low"), "shuffle")]
    if bn >= 255:
        cells.append(Cell("length", "bn_%d_linear40" % bn, prof_linear(40, bn), ("any", "low"), "shuffle"))
    if bn >= 1023:
        cells.append(Cell("length", "bn_%d_block_last" % bn, prof_geo(12, bn - 1) + [1], ("any", "full"), ("block_last",)))
        cells.append(Cell("length", "bn_%d_one_symbol" % bn, [bn], ("any", "low"), "shuffle"))
    return cells


# the shapes the large cases cycle through (BIG_BN bytes each): A is what a frame looks like, B and C occur at sampled block numbers too,
# the others only between them
def big_shapes(bn=BIG_BN):
    return {
        "A": Cell("big", "A_geo0.85_30", prof_geo(30, bn, 0.85), ("fixed", 0, 30), "shuffle"),
        "A2": Cell("big", "A2_geo0.85_30_tilted", prof_geo(30, bn, 0.84), ("fixed", 0, 30), "shuffle"),
        "B": Cell("big", "B_fib14_sampled_only", prof_fib(14, bn), ("fixed", 4, 14), "shuffle"),
        "C": Cell("big", "C_linear20", prof_linear(20, bn), ("fixed", 8, 20), "shuffle"),
        "D": Cell("big", "D_reversed_A", prof_geo(30, bn, 0.85)[::-1], ("fixed", 0, 30), "shuffle"),
        "E": Cell("big", "E_symbols_the_frame_lacks", prof_geo(12, bn, 0.7), ("fixed", 34, 12), "shuffle"),
        "F": Cell("big", "F_equal16", prof_equal(16, bn), ("fixed", 2, 16), "shuffle"),
        "G": Cell("big", "G_near_uniform_wide", prof_equal(256, bn), ("wide",), "shuffle"),
        "H": Cell("big", "H_one_symbol", [bn], ("fixed", 1, 1), "shuffle"),
        "I": Cell("big", "I_linear65", prof_linear(65, bn), ("fixed", 0, 65), "shuffle"),
        "J": Cell("big", "J_pow2_10_high_symbols", prof_pow2(10, bn), ("high", 10), "shuffle"),
        "K": Cell("big", "K_dominant17", prof_dominant(17, bn), ("fixed", 3, 18), "shuffle"),
    }


def big_layout(nblk):
    """Which shape block b of a large case holds.  With 4096 blocks every 16th block is sampled (nblk / 256)."""
    between = ("A", "A", "A2", "A", "J", "A", "A2", "A", "I", "C", "D", "E", "F", "G", "K")
    out = []
    for b in range(nblk):
        if b % 16 == 0:
            k = (b // 16) % 8
            out.append("B" if k == 3 else "C" if k == 5 else "A")
        else:
            out.append(between[b % 16 - 1] if b != nblk - 1 else "H")
    return out


# ---- symbols and bytes --------------------------------------------------------------------------------------------------------------------------
class Unreachable(Exception):
    """The carrier's alphabet does not hold the cell; .why goes into the table."""

    def __init__(self, why):
        Exception.__init__(self, why)
        self.why = why


def _rng(seed, *names):
    return np.random.default_rng([seed] + [zlib.crc32(str(x).encode()) for x in names])


def symbols_of(cell, P, seed):
    """The symbols that carry the cell's counts (most frequent first), by the cell's rule and the seed."""
    n, alpha = len(cell.counts), list(P.alphabet)
    rng = _rng(seed, "symbols", P.route == "fasta_mask", cell.name)
    kind = cell.rule[0]
    if n > len(alpha):
        raise Unreachable("an alphabet of %d symbols" % len(alpha))
    if kind == "fixed":                                           # the large cases: the same symbols at every seed but for a rotation
        lo, k = cell.rule[1], cell.rule[2]
        base = alpha[:64] if len(alpha) > 64 else alpha
        if lo + k > len(base):
            base = alpha
        pool = base[lo:lo + k]
        rot = seed % k
        return (pool[rot:] + pool[:rot])[:n]
    if kind == "wide":
        pool = alpha[:]
        rng.shuffle(pool)
        return pool[:n] if n <= len(pool) else pool
    if kind == "high":
        pool = [s for s in alpha if s > 128][:cell.rule[1] * 2] or alpha[-cell.rule[1] * 2:]
        rng.shuffle(pool)
        return pool[:n]
    if kind == "last":
        last = cell.rule[1]
        if last not in alpha:
            raise Unreachable("no symbol %d" % last)
        pool = [s for s in alpha if s < last]
        rng.shuffle(pool)
        syms = pool[:n - 1] + [last]
        rng.shuffle(syms)
        return syms
    if kind == "ends":
        if 0 not in alpha or 255 not in alpha:
            raise Unreachable("no symbol 0" if 0 not in alpha else "no symbol 255")
        pool = [s for s in alpha if 0 < s < 255]
        rng.shuffle(pool)
        syms = pool[:n - 2] + [0, 255]
        rng.shuffle(syms)
        return syms
    if kind == "pairs":
        pool = [s for s in PAIR_CODES if s in alpha]
        if len(pool) < 16:
            raise Unreachable("no pair codes")
        rng.shuffle(pool)
        return pool[:n]
    span = cell.rule[1]
    pool = [s for s in alpha if s <= 128] if span == "low" and sum(1 for s in alpha if s <= 128) >= n else alpha[:]
    if P.route == "fasta_mask" and n < 100:                       # the mask's units are run lengths: small ones keep the text small
        pool = pool[:max(2 * n, 24)]
    rng.shuffle(pool)
    syms = pool[:n]
    if P.route == "fasta_mask":                                   # the commonest symbols the shortest runs
        syms = sorted(syms)
    return syms


def block_of(cell, P, seed, variant=0):
    """The cell's bytes for a carrier: the counts on the symbols, shuffled, then the placement."""
    if cell.rule[0] == "wide" and len(cell.counts) > len(P.alphabet):     # near-uniform over whatever the carrier has
        cell = cell._replace(counts=prof_equal(len(P.alphabet), sum(cell.counts)))
    syms = symbols_of(cell, P, seed)
    bn = sum(cell.counts)
    rng = _rng(seed, "bytes", cell.name if cell.cls != "gain" else "gain", variant)     # (a gain cell is searched before it has its name)
    b = np.repeat(np.array(syms, dtype=np.uint8), cell.counts[:len(syms)])
    assert len(b) == bn, (cell.name, len(b), bn)
    rng.shuffle(b)
    place = cell.place
    if place == "shuffle":
        return b
    q = quarter_bounds(bn)
    rare = syms[-1]
    at = np.flatnonzero(b == rare)

    if place[0] == "quarter_first":
        return _swap_to(b, at, [q[place[1]]])
    if place[0] == "quarter_last":
        return _swap_to(b, at, [q[place[1] + 1] - 1])
    if place[0] == "block_last":
        return _swap_to(b, at, [bn - 1])
    if place[0] == "only_quarter":
        lo, hi = q[place[1]], q[place[1] + 1]
        free = [i for i in range(lo, hi) if b[i] != rare]
        inside = [i for i in at if lo <= i < hi]
        need = len(at) - len(inside)
        pick = list(rng.choice(free, need, replace=False)) if need else []
        return _swap_to(b, at, inside + pick)
    if place[0] == "marker":
        h = np.bincount(b, minlength=256)
        lens = np.array(code_of(h, bn, P)[0], dtype=np.int64)
        for _ in range(64):
            bits = int(lens[b[q[0]:q[1]]].sum())
            d = (place[1] - bits) % 8
            if d == 0:
                return b
            want = 1 if d <= 4 else -1                           # a swap between the first two quarters that moves the sum one bit
            l0, l1 = lens[b[q[0]:q[1]]], lens[b[q[1]:q[2]]]
            done = False
            for delta in (want, 2 * want, 3 * want):
                for i in range(len(l0)):
                    j = np.flatnonzero(l1 - l0[i] == delta)
                    if len(j):
                        x, y = q[0] + i, q[1] + int(j[0])
                        b[x], b[y] = b[y], b[x]
                        done = True
                        break
                if done:
                    break
            assert done, cell.name
        raise AssertionError("marker placement did not settle: " + cell.name)
    raise AssertionError(place)


def _swap_to(b, at, targets):
    """Move the occurrences of one symbol (at positions `at`) onto `targets` by swaps: the histogram stays."""
    at, targets = [int(i) for i in at], [int(t) for t in targets]
    assert len(at) == len(targets)
    src = [i for i in at if i not in targets]
    dst = [t for t in targets if t not in at]
    for s, t in zip(src, dst):
        b[s], b[t] = b[t], b[s]
    return b


# ---- texts of the archive carriers ------------------------------------------------------------------------------------------------------------------
READ_LEN = 256
LINE = 80
CODE_LETTERS = np.frombuffer(b"-TGKCYSBAWRDMHVN", dtype=np.uint8)            # the letter of a 4-bit code (IUPAC, the container's order)


def fastq_text(stream):
    """A FASTQ whose quality stream is `stream` (bytes 33..126): reads of READ_LEN bases, the last one shorter."""
    q = bytes(stream)
    out = []
    for i in range(0, len(q), READ_LEN):
        part = q[i:i + READ_LEN]
        out.append(b"@r\n" + b"A" * len(part) + b"\n+\n" + part + b"\n")
    return b"".join(out)


def _lines(bases):
    n = len(bases)
    full = n // LINE
    body = np.empty(full * (LINE + 1), dtype=np.uint8)
    if full:
        v = body.reshape(full, LINE + 1)
        v[:, :LINE] = bases[:full * LINE].reshape(full, LINE)
        v[:, LINE] = 10
    tail = bases[full * LINE:].tobytes()
    return body.tobytes() + (tail + b"\n" if tail else b"")


def mask_text(stream):
    """A FASTA whose mask stream is `stream`: runs of A and a in turn, upper case first; a unit of 255 goes on in the next unit."""
    u = np.frombuffer(bytes(stream), dtype=np.uint8).astype(np.int64)
    assert len(u) and u[-1] != 255, "a mask stream cannot end on a unit of 255"
    ends = np.flatnonzero(u < 255)
    csum = np.cumsum(u)
    runs = np.diff(np.concatenate(([0], csum[ends])))
    assert (runs > 0).all() or (runs[1:] > 0).all(), "only the first run can be empty"
    lower = (np.arange(len(runs)) & 1).astype(np.uint8)
    bases = np.repeat(np.uint8(65) + lower * np.uint8(32), runs)
    return b">m\n" + _lines(bases)


def seq_text(stream):
    """A FASTA in upper case whose packed sequence stream is `stream`: two bases a byte, the low nibble first."""
    s = np.frombuffer(bytes(stream), dtype=np.uint8)
    codes = np.empty(2 * len(s), dtype=np.uint8)
    codes[0::2] = s & 15
    codes[1::2] = s >> 4
    return b">s\n" + _lines(CODE_LETTERS[codes])


def text_of(case):
    route = CARRIERS[case.carrier].route
    return {"fastq": fastq_text, "fasta_mask": mask_text, "fasta_seq": seq_text}[route](case.data)


STREAM_INDEX = {"fastq": 5, "fasta_mask": 3, "fasta_seq": 4}     # oracle.QUAL, MASK, SEQ


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name carrier data bn nblk blog env cells exempt frame_tree")
# cells[b]: the Cell of block b; exempt: {(cls, name): why} for the cells the carrier cannot hold; frame_tree: the frame's tree is on


def block_log_for(bn, nblk):
    """The smallest NAF_GPU_BLOCK_LOG at which the even split of nblk * bn bytes is nblk blocks of bn."""
    for blog in range(10, 18):
        bs = 1 << blog
        if bs >= bn and -(-(nblk * bn) // bs) == nblk:
            return blog
    raise AssertionError("no block size cuts %d blocks of %d bytes" % (nblk, bn))


def carrier_env(P, blog):
    env = {"NAF_GPU_BLOCK_LOG": str(blog), "NAF_GPU_LZ": "0"}
    if P.route != "direct":
        env["NAF_GPU_PROBE"] = "0"                                # the look at the sequence stream would turn its match finder on
    return env


def _case(name, carrier, cells, seed, env=None, variants=None):
    P = CARRIERS[carrier]
    blocks, kept, exempt = [], [], {}
    for i, c in enumerate(cells):
        try:
            blocks.append(block_of(c, P, seed, variants[i] if variants else 0))
            kept.append(c)
        except Unreachable as e:
            exempt[(c.cls, c.name)] = e.why
    if not kept:
        return Case(name, carrier, b"", 0, 0, 10, {}, [], exempt, False)
    bn = len(blocks[0])
    assert all(len(b) == bn for b in blocks), name
    data = np.concatenate(blocks)
    if P.route == "fasta_mask":
        data = _mask_legal(data, bn)
    nblk = len(kept)
    assert len(data) <= MAX_STREAM, (name, len(data))
    blog = block_log_for(bn, nblk)
    e = carrier_env(P, blog)
    e.update(env or {})
    ft = P.frame_tree and nblk >= FRAME_BLOCKS and e.get("NAF_GPU_FRAME_TREE") != "0"
    return Case(name, carrier, data.tobytes(), bn, nblk, blog, e, kept, exempt, ft)


def _mask_legal(data, bn):
    """A mask stream cannot end on 255 (the run would go on): swap the last byte with one in front of it in the same quarter."""
    if data[-1] == 255:
        lo = len(data) - bn + quarter_bounds(bn)[3]
        j = lo + int(np.flatnonzero(data[lo:] != 255)[-1])
        data[-1], data[j] = data[j], data[-1]
    return data


def gain_cells(P, bn_range=range(64, 1000)):
    """Single blocks of near-equal counts whose model size is one byte below, at and one byte above what makes the block Raw: the
    threshold is 3 + bn, less the gain the carrier asks for.  Searched over the block length and a tilt of the histogram."""
    low = [s for s in P.alphabet if s <= 128]
    n = min(len(low), 60 if P.min_gain else 120)     # (a carrier that wants an eighth saved never codes 120 near-equal symbols)
    found = {}
    for bn in bn_range:
        for tilt in (0, 1, 2, 3, 5, 8):
            c = prof_equal(n, bn)
            if tilt:
                c = sorted(c, reverse=True)
                c[0] += tilt
                c[-1] -= tilt
                if c[-1] < 1:
                    continue
            syms = low[:n]
            hist = np.zeros(256, dtype=np.int64)
            hist[syms] = c
            # the quarters' sizes depend on the placement; the cell is searched with the bytes it will have
            cell = Cell("gain", "", c, ("fixed", 0, n), "shuffle")
            m = model_block(hist4_of(block_of(cell, P, 0)), P._replace(try_fse=False))
            if m.ssz is None:
                continue
            d = m.csize_hi + ((bn * P.min_gain) >> 8) - (3 + bn)
            if d in (-1, 0, 1) and d not in found:
                found[d] = Cell("gain", {-1: "one_byte_gained", 0: "no_byte_gained", 1: "one_byte_lost"}[d], c, ("fixed", 0, n), "shuffle")
        if len(found) == 3:
            break
    assert len(found) == 3, (P.name, sorted(found))
    return [found[-1], found[0], found[1]]


_GAIN = {}


def small_cases(seed, carrier):
    P = CARRIERS[carrier]
    out = [_case("%s.pack" % carrier, carrier, pack_cells(), seed)]
    for bn in SEAM_BNS:
        out.append(_case("%s.seam%d" % (carrier, bn), carrier, seam_cells(bn), seed))
    for bn in LENGTHS:
        cells = length_cells(bn)
        if bn < 1023:                                             # (a block this short is a stream of its own: the split cuts no block under half a KiB)
            for c in cells:
                out.append(_case("%s.len.%s" % (carrier, c.name), carrier, [c], seed))
        elif block_fits(bn, len(cells)):
            out.append(_case("%s.len.bn_%d" % (carrier, bn), carrier, cells, seed))
        else:
            for k in range(0, len(cells), 2):
                out.append(_case("%s.len.bn_%d.%d" % (carrier, bn, k // 2), carrier, cells[k:k + 2], seed))
    if carrier not in _GAIN:
        _GAIN[carrier] = gain_cells(P)
    for c in _GAIN[carrier]:
        # (the search fixed the bytes at seed 0: a gain cell is the same block at every seed -- one byte decides it)
        out.append(_case("%s.gain.%s" % (carrier, c.name), carrier, [c], 0))
    shapes = big_shapes()
    out.append(_case("%s.shapes" % carrier, carrier, [shapes[k] for k in sorted(shapes)], seed))
    return [c for c in out if c.nblk or c.exempt]


def block_fits(bn, nblk):
    try:
        block_log_for(bn, nblk)
        return True
    except AssertionError:
        return False


def big_case(seed, carrier, nblk, env=None, tag=""):
    shapes = big_shapes()
    layout = big_layout(nblk)
    if CARRIERS[carrier].route == "fasta_mask":                   # units are run lengths: the shapes of long runs only in the first 256 blocks keep the text near 30 MB
        layout = [k if b < DEFER_BLOCKS or k not in ("G", "J", "I", "E", "D") else "A2" for b, k in enumerate(layout)]
    return _case("%s.big%d%s" % (carrier, nblk, tag), carrier, [shapes[k] for k in layout], seed, env=env, variants=[b % 3 for b in range(nblk)])


def big_cases(seed, carrier):
    out = [big_case(seed, carrier, DEFER_BLOCKS), big_case(seed, carrier, FRAME_BLOCKS)]
    if CARRIERS[carrier].frame_tree:
        out.append(big_case(seed, carrier, FRAME_BLOCKS, env={"NAF_GPU_FRAME_TREE": "0"}, tag=".own_trees"))
    return out


def all_cases(seed, carrier, big=True):
    return small_cases(seed, carrier) + (big_cases(seed, carrier) if big else [])


def all_cells():
    """Every (cls, name) the plan holds."""
    cells = [(c.cls, c.name) for c in pack_cells()]
    for bn in SEAM_BNS:
        cells += [(c.cls, "%s_bn%d" % (c.name, bn)) for c in seam_cells(bn)]
    for bn in LENGTHS:
        cells += [(c.cls, c.name) for c in length_cells(bn)]
    cells += [("gain", nm) for nm in ("one_byte_gained", "no_byte_gained", "one_byte_lost")]
    sh = big_shapes()
    for tag in ("small", "256", "4096"):
        cells += [("big", "%s@%s" % (sh[k].name, tag)) for k in sorted(sh)]
    return cells


def cell_key(case, b):
    c = case.cells[b]
    if c.cls == "seam":
        return (c.cls, "%s_bn%d" % (c.name, case.bn))
    if c.cls == "big":
        tag = "small" if case.nblk < DEFER_BLOCKS else "256" if case.nblk < FRAME_BLOCKS else "4096"
        return (c.cls, "%s@%s" % (c.name, tag))
    return (c.cls, c.name)


# ---- the checks ---------------------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def block_model(block, P):
    key = (P, bytes(block))
    if key not in _MODELS:
        h4 = hist4_of(block)
        _MODELS[key] = (h4, model_block(h4, P))
    return _MODELS[key]


def sampled_blocks(nblk):
    """The blocks k_zenc_plan's sample launch plans: ZENC_CACHE_ENTRIES evenly spaced ones, from 16 * that many blocks on."""
    if nblk < FRAME_BLOCKS:
        return []
    stride = nblk // 256
    return [i * stride for i in range(256)]


def check_decodes(oracle, frame, data):
    try:
        out = oracle.zstd_decompress(frame, len(data) + 64)
    except ValueError as e:
        raise Reject("decode", str(e))
    if out != data:
        raise Reject("decode", "%d bytes, not the %d planned" % (len(out), len(data)))


def _weights(lens, log):
    return tuple(int(log + 1 - l) if l else 0 for l in lens)


def check_frame(case, frame, lits, descriptions=None):
    """Every block of a frame against the model.  Raises Reject; returns the path letters of each block.
    descriptions: {(FSE tried, weights): description bytes} kept across frames -- the same weights, the same bytes, whoever wrote them."""
    P = CARRIERS[case.carrier]
    data = np.frombuffer(case.data, dtype=np.uint8)
    bn, nblk = case.bn, case.nblk
    if len(lits) != nblk or [int(x) for x in lits.decoded_size] != [bn] * nblk:
        raise Reject("plan out of date", "%s: %d blocks of %s, planned %d of %d" % (case.name, len(lits), sorted(set(int(x) for x in lits.decoded_size)), nblk, bn))
    assert split_even(len(data), 1 << case.blog) == [b * bn for b in range(nblk + 1)]
    if int(lits.n_sequences.sum()):
        raise Reject("sequences", "a carrier of this plan runs without the match finder")
    sampled = sampled_blocks(nblk)
    cached = set()
    for b in sampled:
        m = block_model(data[b * bn:(b + 1) * bn], P)[1]
        if m.kind != "rle" and m.log:
            cached.add(_weights(m.lens, m.log))
    flen = None                                                   # the frame's code, as its first treeless block shows it
    paths, raws = [], []
    for b in range(nblk):
        blk = data[b * bn:(b + 1) * bn]
        h4, m = block_model(blk, P)
        where = "%s block %d (%s)" % (case.name, b, case.cells[b].name)
        bt, fsz = int(lits.block_type[b]), int(lits.frame_size[b])
        if fsz > 3 + bn:
            raise Reject("larger than Raw", "%s: %d bytes for %d" % (where, fsz, bn))
        if m.kind == "rle":
            if bt != 1:
                raise Reject("rle", "%s: one distinct symbol, block type %d" % (where, bt))
            paths.append("E")
            continue
        if bn < 64 or (P.min_gain and int(h4.sum(axis=0).max()) + 16 >= bn):
            if bt != 0:
                raise Reject("tiny", "%s: block type %d where the planner keeps the block Raw" % (where, bt))
            paths.append("W")
            continue
        if bt == 1:
            raise Reject("rle", "%s: an RLE block of %d distinct symbols" % (where, m.distinct))
        if bt == 0:
            if m.kind == "huf" and case.frame_tree:
                raws.append((b, where, m, h4))                     # (settled below, once the frame's code is known)
            elif m.kind == "huf":
                raise Reject("raw/huffman", "%s: Raw, the model's Huffman block is at most %d + %d of %d" % (where, m.csize_hi, (bn * P.min_gain) >> 8, 3 + bn))
            paths.append(m.path if m.path.endswith("W") else m.path + "W")
            continue
        lt = int(lits.lit_type[b])
        if lt not in (2, 3):
            raise Reject("literals", "%s: a Compressed block with literals type %d" % (where, lt))
        lens = lits.len[b]
        regen, comp, hb = int(lits.regen[b]), int(lits.comp[b]), int(lits.header_bytes[b])
        if regen != bn or fsz != 3 + hb + comp + 1:
            raise Reject("sizes", "%s: regenerated %d, block %d, header %d + literals %d" % (where, regen, fsz, hb, comp))
        if hb != lit_header_bytes(regen, comp):
            raise Reject("header", "%s: %d header bytes for sizes %d and %d" % (where, hb, regen, comp))
        if int(lits.n_streams[b]) != 4:
            raise Reject("streams", "%s: %d streams" % (where, int(lits.n_streams[b])))
        if (lens[h4.sum(axis=0) > 0] == 0).any():
            raise Reject("lengths", "%s: a symbol of the block without a code" % where)
        want = stream_bytes(h4, lens)
        if [int(x) for x in lits.stream_size[b]] != want:
            raise Reject("stream size", "%s: %s, the listed lengths give %s" % (where, [int(x) for x in lits.stream_size[b]], want))
        tb = int(lits.tree_bytes[b])
        if comp != tb + 6 + sum(want):
            raise Reject("sizes", "%s: literals of %d bytes, tree %d + 6 + streams %d" % (where, comp, tb, sum(want)))
        kraft = sum(1 << (11 - int(l)) for l in lens if l)
        limit = limit_of(P, int((lens > 0).sum()))
        framed = False
        if lt == 3:
            if not case.frame_tree:
                raise Reject("treeless", "%s: a treeless section outside a frame with a frame's tree" % where)
            framed = True
        elif case.frame_tree and not np.array_equal(lens, np.asarray(m.lens)) and (flen is None or np.array_equal(lens, flen)):
            framed = True                                         # a block that carries the frame's tree
        if framed:
            if flen is None:
                flen = lens.copy()
            if not np.array_equal(lens, flen):
                raise Reject("frame code", "%s: a second code without a symbol that asks for it" % where)
            if kraft != 1 << 11 or int(lens.max()) > limit:
                raise Reject("frame code", "%s: Kraft sum %d / 2048, longest code %d under a limit of %d" % (where, kraft, int(lens.max()), limit))
            paths.append("T")
            continue
        # a Huffman block with its own tree
        if kraft != 1 << 11:
            raise Reject("kraft", "%s: Kraft sum %d / 2048" % (where, kraft))
        if int(lens.max()) > m.limit:
            raise Reject("limit", "%s: a code of %d bits under a limit of %d" % (where, int(lens.max()), m.limit))
        hist = h4.sum(axis=0)
        flat16 = P.flat_scan and bn >= 2048 and np.array_equal(lens, FLAT16) and not (hist[FLAT16 == 0]).any()
        if not flat16:
            if (lens[hist == 0] != 0).any():
                raise Reject("lengths", "%s: a code for a symbol the block does not hold" % where)
            present = np.flatnonzero(hist)
            o = present[np.lexsort((present, hist[present]))]
            if (np.diff(lens[o]) > 0).any():
                raise Reject("order", "%s: a more frequent symbol with the longer code" % where)
        cost, hc = int((hist * lens).sum()), huffman_cost(hist)
        flat_pref = flat16 or "P" in m.path
        if flat_pref:
            k = int(lens.max())
            fb = bn * k
            if not ((lens[hist > 0] == k).all() and (fb - hc) * P.prefer_flat < fb):
                raise Reject("cost", "%s: flat codes of %d bits where Huffman coding saves %d of %d bits" % (where, k, fb - hc, fb))
        elif m.depth <= m.limit:
            if cost != hc:
                raise Reject("cost", "%s: %d bits, an optimal code has %d" % (where, cost, hc))
        else:
            lc = limited_cost(hist, m.limit)
            if not lc <= cost <= fixed_width_cost(hist):
                raise Reject("cost", "%s: %d bits, package-merge %d, fixed width %d" % (where, cost, lc, fixed_width_cost(hist)))
        if not flat16 and not np.array_equal(lens, np.asarray(m.lens)):
            raise Reject("lengths", "%s: not the documented construction's (first difference at symbol %d)" % (where, int(np.flatnonzero(lens != np.asarray(m.lens))[0])))
        # the tree description
        nw, fse = int(lits.n_weights[b]), int(lits.tree_fse[b])
        lastw = int(np.flatnonzero(lens)[-1])
        if nw != lastw:
            raise Reject("tree", "%s: %d weights written, the last symbol is %d" % (where, nw, lastw))
        if not P.try_fse and lastw <= 128 and not flat16:
            if fse or tb != direct_tree_bytes(lastw):
                raise Reject("tree", "%s: %s description of %d bytes, direct weights take %d" % (where, "an FSE-coded" if fse else "a direct", tb, direct_tree_bytes(lastw)))
        if lastw > 128 and not fse:
            raise Reject("tree", "%s: direct weights for %d symbols" % (where, lastw))
        if lastw <= 128 and tb > direct_tree_bytes(lastw):
            raise Reject("tree", "%s: %d bytes, direct weights take %d" % (where, tb, direct_tree_bytes(lastw)))
        if descriptions is not None:
            key = (bool(P.try_fse or flat16), _weights(lens, int(lens.max())))
            desc = bytes(frame[int(lits.tree_offset[b]):int(lits.tree_offset[b]) + tb])
            if descriptions.setdefault(key, desc) != desc:
                raise Reject("tree", "%s: the same weights, another description (%d and %d bytes)" % (where, len(descriptions[key]), len(desc)))
        # Raw against Huffman, with the description's size as the frame shows it
        if fsz + ((bn * P.min_gain) >> 8) >= 3 + bn:
            raise Reject("raw/huffman", "%s: a Huffman block of %d + %d bytes where Raw is %d" % (where, fsz, (bn * P.min_gain) >> 8, 3 + bn))
        if m.kind == "raw":
            raise Reject("raw/huffman", "%s: Huffman, the model's block is at least %d of %d" % (where, m.csize_lo, 3 + bn))
        w = _weights(m.lens, m.log)
        path = "Q" if flat16 and "F" not in m.path and "P" not in m.path else m.path
        if flat16 and np.array_equal(lens, np.asarray(m.lens)):
            path = m.path                                         # (the scan or the planner: the same block either way)
        direct_w = not P.try_fse and lastw <= 128
        if sampled and path != "Q":
            path += "C" if w in cached else "M"
        if nblk >= DEFER_BLOCKS and not direct_w and not (sampled and w in cached) and path != "Q":
            path += "D"
        paths.append(path)
    if case.frame_tree:
        # the frame's code: complete, within the limit, and the documented construction's over the sampled blocks' summed histogram
        if flen is None:
            raise Reject("frame code", "%s: no block is coded with the frame's code" % case.name)
        want, wlog, wlimit = frame_code_model([block_model(data[b * bn:(b + 1) * bn], P)[0].sum(axis=0) for b in sampled], P)
        if not np.array_equal(flen, np.asarray(want)):
            raise Reject("frame code", "%s: not the documented construction's over the sample (first difference at symbol %d)" % (case.name, int(np.flatnonzero(flen != np.asarray(want))[0])))
        # which blocks take the frame's code: the 3 % rule, which the plan's shapes pass or miss by a per cent at least (the CPU test holds that)
        ratio = frame_ratio([block_model(data[b * bn:(b + 1) * bn], P)[0].sum(axis=0) for b in sampled], flen)
        prev_t = False
        ftb = next(int(lits.tree_bytes[b]) for b in range(nblk) if paths[b] == "T" and int(lits.lit_type[b]) == 2)   # (the first block of the frame's code carries its tree)
        for b in range(nblk):
            if int(lits.block_type[b]) != 2:
                continue
            h4, m = block_model(data[b * bn:(b + 1) * bn], P)
            takes = frame_rule(h4.sum(axis=0), flen, ratio)[0]
            took = paths[b] == "T"
            # (a block the rule accepts still goes the general way where it would not stay below Raw with the tree on board)
            body = ftb + 6 + sum(stream_bytes(h4, flen)) if takes else 0
            stays_below_raw = takes and 3 + lit_header_bytes(bn, body) + body + 1 <= 3 + bn
            if took and not takes or stays_below_raw and not took:
                raise Reject("frame code", "%s block %d (%s): the rule says %s, the block is %s" % (case.name, b, case.cells[b].name, takes, paths[b]))
            if took and (int(lits.lit_type[b]) == 3) != prev_t:
                raise Reject("treeless", "%s block %d: literals type %d behind a block %s the frame's code" % (case.name, b, int(lits.lit_type[b]), "of" if prev_t else "without"))
            prev_t = took
        # a Raw block of such a frame where the model's own code pays: only if the frame's code covers it and does not pay
        for b, where, m, h4 in raws:
            covered = not (flen[h4.sum(axis=0) > 0] == 0).any()
            body = 6 + sum(stream_bytes(h4, flen)) if covered else 0
            if not covered or 3 + lit_header_bytes(bn, body) + body + 1 < 3 + bn:
                raise Reject("raw/huffman", "%s: Raw, the model's Huffman block is at most %d of %d and the frame's code does not say otherwise" % (where, m.csize_hi, 3 + bn))
    return paths


# ---- the coverage table -----------------------------------------------------------------------------------------------------------------------------
class Coverage:
    def __init__(self):
        self.seen = {}            # (cell key, carrier) -> set of path strings
        self.why = {}             # (cell key, carrier) -> reason

    def add(self, case, paths):
        for b, p in enumerate(paths):
            self.seen.setdefault((cell_key(case, b), case.carrier), set()).add(p)
        for k, why in case.exempt.items():
            self.why[(k, case.carrier)] = why

    def exempt(self, case):
        for k, why in case.exempt.items():
            self.why[(k, case.carrier)] = why

    def empty(self, carriers):
        """Cells of a carrier with neither a checked block nor a reason."""
        out = []
        for key in all_cells():
            for c in carriers:
                if (key, c) not in self.seen and not self._why(key, c):
                    out.append((key, c))
        return out

    def _why(self, key, carrier):
        if (key, carrier) in self.why:
            return self.why[(key, carrier)]
        if carrier == "emul" and key[0] == "big" and not key[1].endswith("@small"):
            return "no host build of large frames"
        if key[0] == "big":                                       # the shapes share their exemptions over the three sizes
            base = key[1].split("@")[0]
            for (k, c), why in self.why.items():
                if c == carrier and k[0] == "big" and k[1].split("@")[0] == base:
                    return why
        return None

    def letters(self):
        return set("".join(p for v in self.seen.values() for p in v))

    def table(self, carriers, title):
        rows = ["coverage, cell by carrier -- %s" % title,
                "  (F flat shortcut, R register construction, S serial routine, L length limiting, P flat preferred, Q flat scan, C cache hit,",
                "   M cache miss, D description deferred to k_zenc_tree, T the frame's code, W Raw, E RLE; a reason where the carrier cannot hold the cell)",
                "  %-44s %s" % ("cell", " ".join("%-14s" % c for c in carriers))]
        for key in all_cells():
            cols = []
            for c in carriers:
                v = self.seen.get((key, c))
                cols.append("%-14s" % (",".join(sorted(v)) if v else ("(" + (self._why(key, c) or "EMPTY") + ")")))
            rows.append("  %-44s %s" % ("%s.%s" % key, " ".join(cols)))
        return "\n".join(rows)


def excess_table(limits=(7, 9, 11)):
    """What the documented length limiting costs over package-merge, per cell of the pack whose unlimited depth is above the limit."""
    rows, worst = [], (0.0, "")
    for c in pack_cells() + [big_shapes()[k] for k in ("B",)]:
        hist = list(c.counts) + [0] * (256 - len(c.counts))
        n = len(c.counts)
        for L in limits:
            L2 = L if n <= 64 else max(L, 9)
            if L2 != L:
                continue
            lens, log, depth = plan_lengths(hist, L)
            if depth <= L or not log:
                continue
            cost, lc = sum(a * b for a, b in zip(hist, lens)), limited_cost(hist, L)
            ex = 100.0 * (cost - lc) / lc
            rows.append((c.name, n, L, depth, cost, lc, ex, cost <= fixed_width_cost(hist)))
            if ex > worst[0]:
                worst = (ex, "%s at %d bits" % (c.name, L))
    return rows, worst
