"""The conformance corpus: zstd frames whose every encoding choice is made on purpose (tests/zstd_compose.py), in families.

  format  -- every header, literals and sequences choice of RFC 8878 at its boundaries;
  state   -- what a block inherits from the blocks in front of it (Huffman tree, FSE tables, repeat offsets);
  each of those as composed ("full"), and at three sizes: "small" (within the limits of the one-wavefront small-frame decoder:
  the family with smaller lengths, cut into several frames where its blocks do not depend on each other), "mid" (between
  16 KiB and 4 MiB: the every-byte block index) and "big" (over 4 MiB: the 1 MiB-chunk index), by Raw blocks of random bytes
  around the full form;
  look    -- lookalikes of the flat fast paths: a control frame of identical flat 4-bit blocks of packed A C G T bytes and
  variants that differ from it in exactly one legal way, at chosen block positions.  lookalike_content() is the content
  they all share, so that they can stand in for the sequence section of an archive of that text.

corpus() yields (name, frame, content, features); everything is deterministic (CORPUS_SHA256 in the tests pins it).
"""
import numpy as np

import zstd_compose as Z

ACGT4 = bytes(lo | (hi << 4) for hi in (1, 2, 4, 8) for lo in (1, 2, 4, 8))     # the packed bytes of two of A C G T (4-bit codes 1 2 4 8)
RUN4 = 0x11                                                                     # "AA"
LOOK_BLOCK = 32 * 1024
LOOK_N = 280                                                                    # > 4 MiB of compressed blocks
STRIDE_TAIL = 64
# what the one-wavefront small-frame decoder takes: frames of at most SMALL_SRC bytes, at most SMALL_OUT bytes of output buffer
# (the content and the 64 bytes of slack the tests give), at most SMALL_SEQ sequences in a block
SMALL_SRC, SMALL_OUT, SMALL_SEQ = 16384, 32768, 2048
# the frames whose shape cannot fit those limits (content of 65791 bytes or more, 0x7EFF or more sequences in a block): no small form
NOT_SMALL = ("fcs_ss_65791", "fcs_ss_65792", "fcs_win_70000_w8", "nseq_32511", "nseq_32512", "nseq_32812")


def _rng(seed):
    return np.random.default_rng(seed)


def _hist(xs):
    h = {}
    for x in xs:
        h[x] = h.get(x, 0) + 1
    return h


def weights_for(lengths):
    """Huffman weights of symbols 0..max from {symbol: code length} (a complete prefix code)."""
    mb = max(lengths.values())
    w = [0] * (max(lengths) + 1)
    for s, L in lengths.items():
        w[s] = mb + 1 - L
    return w


def flat_tree(symbols, bits):
    """All symbols with one code length: 2**bits of them (symbols beyond those given are filled in from 0 up)."""
    syms = set(symbols)
    s = 0
    while len(syms) < (1 << bits):
        if s not in syms:
            syms.add(s)
        s += 1
    return Z.HufTree(weights_for({x: bits for x in syms}))


def tree_of(data, max_bits=11):
    """A non-flat tree for data: code lengths from a Huffman construction over its histogram, limited to max_bits."""
    import heapq
    h = _hist(data)
    if len(h) == 1:
        h[(next(iter(h)) + 1) % 256] = 1
    heap = [(c, i, [s]) for i, (s, c) in enumerate(sorted(h.items()))]
    heapq.heapify(heap)
    depth = {s: 0 for s in h}
    k = len(heap)
    while len(heap) > 1:
        c1, _, a = heapq.heappop(heap); c2, _, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (c1 + c2, k, a + b)); k += 1
    # limit to max_bits, then make the Kraft sum exactly 1 (in units of 2**-max_bits)
    for x in depth:
        depth[x] = min(max(depth[x], 1), max_bits)
    kraft = lambda: sum(1 << (max_bits - d) for d in depth.values())
    while kraft() > 1 << max_bits:
        x = max((d, x) for x, d in depth.items() if d < max_bits)[1]
        depth[x] += 1
    while kraft() < 1 << max_bits:
        x = max((d, x) for x, d in depth.items())[1]          # the deepest code: one level up adds the smallest amount
        depth[x] -= 1
    return Z.HufTree(weights_for(depth))


def spec(blocks, split=None, **kw):
    """A family's blocks and compose() arguments.  split: the number of leading blocks every part needs when the blocks behind them
    do not depend on each other, so that the small form may cut the family into several frames (None: one frame)."""
    return blocks, kw, split


def fse_mode(codes, log, lt1=()):
    return ("fse", Z.normalize(_hist(codes), log, lt1), log)


def _codes(seqs):
    return ([Z.ll_code(a) for a, b, c in seqs], [Z.of_code(c) for a, b, c in seqs], [Z.ml_code(b) for a, b, c in seqs])


# ---- format edges ------------------------------------------------------------------------------------------------------------
def format_frames(small=False):
    """small: the form that fits the one-wavefront small-frame decoder (SMALL_SRC, SMALL_OUT, SMALL_SEQ); shapes that cannot fit it
    (a content size of 65791 or more, 0x7EFF or more sequences in a block, literal lengths from 32768 and match lengths from 32771
    up: LL codes 34, 35 and ML codes 51, 52) are left to the full form."""
    r = _rng(1)
    rb = lambda n: r.integers(0, 256, n, dtype=np.uint8).tobytes()
    text = lambda n, alpha=b"ACGTN acgt": bytes(np.frombuffer(alpha, np.uint8)[r.integers(0, len(alpha), n)])
    # Frame_Content_Size at the edges of its widths, single segment and with a window descriptor
    for n in (0, 1, 255, 256) + (() if small else (65791, 65792)):
        yield "fcs_ss_%d" % n, spec([Z.raw(text(n))] if n < 65536 else [Z.raw(text(65536)), Z.raw(text(n - 65536))], single_segment=True)
    for n, w in ((300, 2), (300, 4), (300, 8), (255, 0)) + (() if small else ((70000, 8),)):
        yield "fcs_win_%d_w%d" % (n, w), spec([Z.rle(7, n)] if n < 65536 else [Z.rle(7, 65536), Z.raw(text(n - 65536))], fcs=w, window_log=17)
    yield "checksum_mantissa", spec([Z.raw(text(5000)), Z.rle(65, 20000 if small else 70000)], checksum=True, window_log=16, window_mantissa=5)
    # literals: Raw / RLE in every header form (1 byte for even and odd sizes, 2, 3 bytes; wider forms than needed too)
    blocks = []
    for kind in ("raw", "rle"):
        for n, fmt in ((0, 2), (30, 1), (31, 1), (31, 2), (32, 2), (4095, 2), (4096, 3), (100, 3), (3000 if small else 70000, 3)):
            if kind == "rle" and n == 0:
                continue
            lits = bytes([65 + n % 26]) * n if kind == "rle" else text(n)
            blocks.append(Z.comp(lits, lit=kind, lit_fmt=fmt))
    yield "lits_raw_rle_forms", spec(blocks, split=0, checksum=True, window_log=20)
    # Huffman literals: 1 / 4 streams, 10 / 14 / 18-bit sizes, direct / FSE weights, max bits 1..11, 2 and 256 symbols
    blocks = []
    two = Z.HufTree([0] * 70 + [1, 1])                                          # 2 symbols, 1 bit each
    blocks.append(Z.comp(r.choice([70, 71], 900).astype(np.uint8).tobytes(), lit="huf", tree=two, streams=1))
    blocks.append(Z.comp(r.choice([70, 71], 900).astype(np.uint8).tobytes(), lit="huf", tree=two, fse_tree=True, streams=4, lit_fmt=10))
    big = 3000 if small else 9000
    for mb in range(2, 12):
        n_sym = min(256, (1 << (mb - 1)) + 1)
        data = bytes(r.choice((np.arange(n_sym) * (255 // max(1, n_sym - 1)) % 256).astype(np.uint8), 9000,
                              p=np.arange(1, n_sym + 1) ** 2.0 / np.sum(np.arange(1, n_sym + 1) ** 2.0)).astype(np.uint8))[:big]
        t = tree_of(data, mb)
        direct = len(t.weights) <= 129
        blocks.append(Z.comp(data, lit="huf", tree=t, fse_tree=not direct or mb % 2 == 0, streams=4, lit_fmt=14))
        blocks.append(Z.comp(data[:1000], lit="huf", tree=t, fse_tree=not direct or mb % 2 == 1, streams=1, lit_fmt=10))
    all256 = bytes(range(256)) + r.choice(256, 12000 if small else 60000, p=np.arange(1, 257) / np.sum(np.arange(1, 257))).astype(np.uint8).tobytes()
    blocks.append(Z.comp(all256, lit="huf", tree=tree_of(all256, 11), fse_tree=True, streams=4, lit_fmt=18))
    # (a flat tree of 256 symbols has no description: one weight value leaves FSE nothing to code, and 255 weights are too many
    # to store directly; 128 symbols of 7 bits are the widest flat tree stored directly)
    blocks.append(Z.comp(bytes(x & 127 for x in all256[:6000 if small else 20000]), lit="huf", tree=flat_tree(range(128), 7), streams=4, lit_fmt=18))
    yield "huffman_forms", spec(blocks, split=0, checksum=True, window_log=20)
    # sequence counts in every form, at their edges
    base = text(4096, b"ACGT")
    for n in (1, 5, 127, 128) + (() if small else (0x7EFF, 0x7F00, 0x7F00 + 300)):
        seqs = [(int(r.integers(0, 2)), 3, 4 + int(r.integers(1, 400))) for _ in range(n)]
        nl = sum(s[0] for s in seqs) + 7
        form = 2 if n == 5 else None
        lits = text(nl, b"ACGT")
        yield "nseq_%d" % n, spec([Z.raw(base), Z.comp(lits, seqs, lit="raw", nseq_form=form)], window_log=17)
    # every LL code and every ML code, under every table mode and accuracy log
    lls = [Z.LL_BASE[c] for c in range(36)]
    mls = [Z.ML_BASE[c] for c in range(53)]
    blocks = [Z.raw(text(2000))]
    lit_pool = text(131072)
    for c, ll in enumerate(lls):                                               # one block per long literal length
        if ll >= 1024 and not (small and ll >= 32768):
            v = min(ll + int(r.integers(0, 1 << Z.LL_BITS[c])), 30000 if small else 131000)
            if small:                                                          # (Huffman literals: the frame stays within 16 KiB)
                blocks.append(Z.comp(lit_pool[:v], [(v, 3, 5)], lit="huf", tree=tree_of(lit_pool[:v], 11)))
            else:
                blocks.append(Z.comp(lit_pool[:v], [(v, 3, 5)], lit="raw"))
    short = [(ll, 4 + i % 5, 3 + 1 + i % 600) for i, ll in enumerate(l for l in lls if l < 1024)]
    blocks.append(Z.comp(text(sum(s[0] for s in short)), short, lit="raw"))
    for c, ml in enumerate(mls):
        if small and ml >= 32771:
            continue
        extra = int(r.integers(0, 1 << Z.ML_BITS[c]))
        blocks.append(Z.comp(text(3), [(3, min(ml + extra, 20000 if small else 131068), 3 + 1 + c % 16)], lit="raw"))
    if not small:
        blocks.append(Z.comp(b"", [(0, 131072, 3 + 1)], lit="raw"))             # the longest match a block holds (code 52), overlapping
    yield "every_ll_ml_code", spec(blocks, split=1, window_log=17)
    # FSE-compressed tables at every accuracy log, with "less than 1" counts and zero runs (short and > 3 long)
    blocks = [Z.raw(text(1024, b"ACGT"))]
    for log in range(5, 10):
        seqs = []
        for i in range(150 if small else 600):
            ll = [0, 1, 2, 3, 17, 40, 70][i % 7] if i % 11 else 300
            seqs.append((ll, [3, 4, 5, 6, 40, 100, 300][i % 5], [1, 2, 3, 4 + 7, 4 + 100, 4 + 1000][i % 6]))
        lc, oc, mc = _codes(seqs)
        modes = (fse_mode(lc, log, lt1=(25,)), fse_mode(oc, min(log, 8), lt1=(1,)), fse_mode(mc, log, lt1=(38,)))
        blocks.append(Z.comp(text(sum(s[0] for s in seqs)), seqs, lit="raw", modes=modes))
    yield "fse_logs_lt1_zero_runs", spec(blocks, split=1, window_log=17)
    # RLE mode for each field, predefined for the others, and all RLE
    blocks = [Z.raw(text(1000))]
    for k in range(3):
        seqs = [(5, 9 + (i % 3 if k != 2 else 0), 4 + 20 + (0 if k == 1 else i % 4)) for i in range(40)]
        modes = ["pre"] * 3
        modes[k] = "rle"
        blocks.append(Z.comp(text(5 * 40), seqs, lit="raw", modes=modes))
    blocks.append(Z.comp(text(6 * 50), [(6, 131, 4 + 32)] * 50, lit="raw", modes=("rle",) * 3))
    yield "rle_modes", spec(blocks, split=1, window_log=17)
    # overlapping matches, offsets 1..16, lengths up to the block's end; matches exactly the window back and into Raw / RLE blocks
    blocks = [Z.raw(text(64))]
    for off in range(1, 17):
        blocks.append(Z.comp(text(off + 1), [(off, 3 + off * 7, off + 3), (1, 1000 + off, off + 3)], lit="raw"))
    blocks.append(Z.comp(b"", [(0, 20000 if small else 131072, 1 + 3)], lit="raw"))
    yield "overlaps", spec(blocks, split=1, window_log=17)
    W = 1 << 10
    blocks = [Z.raw(text(W)), Z.rle(66, W), Z.comp(text(10), [(10, 100, W + 3), (0, 50, W + 3 - 1)], lit="raw"),
              Z.comp(b"", [(0, W, W + 3)], lit="raw"), Z.raw(text(200)), Z.comp(b"", [(0, 300, W + 3), (0, 300, 200 + 300 + 3)], lit="raw")]
    yield "window_back_small", spec(blocks, window_log=10)
    Wm = (1 << 10) + (1 << 7) * 3                                             # a Window_Descriptor with a mantissa; blocks capped by it
    blocks = [Z.raw(text(Wm)), Z.rle(9, Wm), Z.comp(text(Wm - 300), [(Wm - 300, 300, Wm + 3)], lit="raw"),
              Z.comp(b"", [(0, Wm, Wm + 3)], lit="raw")]
    yield "window_capped_mantissa", spec(blocks, window_log=10, window_mantissa=3, checksum=True)
    # a Compressed block of nothing, a zero-size last Raw block, skippable frames and several frames
    # (a Compressed block is at least 3 bytes for libzstd: the empty literals in their 2 and 3-byte forms)
    yield "empty_blocks", spec([Z.raw(text(100)), Z.comp(b"", [], lit="raw", lit_fmt=2), Z.comp(b"", [], lit="raw", lit_fmt=3),
                                     Z.raw(text(10)), Z.raw(b"")], window_log=17)
    f1 = Z.compose([Z.raw(text(500)), Z.comp(text(20), [(20, 30, 3 + 100)], lit="raw")], single_segment=True, checksum=True)
    f2 = Z.compose([Z.rle(3, 1000), Z.comp(text(5), [(5, 30, 3 + 1)], lit="raw")], window_log=12)
    yield "frames_and_skippables", Z.concat([Z.skippable(b"skip me", 0), f1, Z.skippable(rb(300), 15), f2, f1, Z.skippable(b"", 7)])


# ---- state carried across blocks ---------------------------------------------------------------------------------------------
def state_frames(small=False):
    r = _rng(2)
    text = lambda n, alpha=b"ACGT": bytes(np.frombuffer(alpha, np.uint8)[r.integers(0, len(alpha), n)])
    t1 = tree_of(text(5000, b"AAAACCGT"))
    t2 = tree_of(text(5000, b"ACGTTTTTTTTTTTTT"))
    # treeless literals behind raw literals, RLE literals, Raw and RLE blocks; trees that repeat a non-adjacent one or the
    # previous one with another stream count
    L = lambda n, a=b"AAAACCGT": text(n // 2 if small else n, a)
    blocks = [Z.comp(L(3000), lit="huf", tree=t1), Z.comp(L(200), lit="raw"), Z.comp(L(3000), lit="treeless"),
              Z.comp(b"G" * 300, lit="rle"), Z.comp(L(900), lit="treeless", streams=1),
              Z.raw(L(700)), Z.comp(L(2000), lit="treeless"), Z.rle(67, 2000 if small else 5000), Z.comp(L(2500), lit="treeless"),
              Z.comp(L(3000, b"ACGTTTTTTTTTTTTT"), lit="huf", tree=t2), Z.comp(L(3000), lit="huf", tree=t1),       # t1 again, not adjacent
              Z.comp(L(800), lit="huf", tree=t1, streams=1), Z.comp(L(3000), lit="huf", tree=t1, streams=4),          # same tree, 1 then 4 streams
              Z.comp(L(3000), lit="huf", tree=t1, fse_tree=True), Z.comp(L(3000), lit="treeless")]
    yield "tree_state", spec(blocks, window_log=17, checksum=True)
    # FSE Repeat mode behind blocks without sequences, and Repeat of an RLE table
    base = text(2000)
    seqs = [(i % 9, 4 + i % 30, 4 + 1 + (i * 37) % 1500) for i in range(150 if small else 300)]
    lc, oc, mc = _codes(seqs)
    modes = (fse_mode(lc, 6), fse_mode(oc, 5), fse_mode(mc, 7))
    nl = lambda s: text(sum(x[0] for x in s) + 3)
    seqs2 = [(3, 7, 4 + 100)] * 30
    blocks = [Z.raw(base), Z.comp(nl(seqs), seqs, modes=modes), Z.comp(text(50), [], lit="raw"), Z.raw(text(10)),
              Z.comp(nl(seqs), seqs, modes=("rep",) * 3), Z.comp(nl(seqs2), seqs2, modes=("rle", "rle", "rle")),
              Z.comp(text(3), []), Z.comp(nl(seqs2), seqs2, modes=("rep", "rep", "rep")),
              Z.comp(nl(seqs), seqs, modes=(modes[0], "pre", modes[2])), Z.comp(nl(seqs), seqs, modes=("rep", "rep", "rep"))]
    yield "fse_repeat_state", spec(blocks, window_log=17, checksum=True)
    # long scripted repeat-code walks: every transition of section 3.1.2.5, with ll == 0 and ll > 0, over dozens of blocks
    for seed, nblk in ((3, 12), (4, 16)) if small else ((3, 40), (4, 60)):
        rr = _rng(seed)
        blocks = [Z.raw(text(4000))]
        rep = [1, 4, 8]
        for b in range(nblk):
            seqs = []
            n = int(rr.integers(20, 50) if small else rr.integers(50, 200))
            for i in range(n):
                ll = 0 if rr.random() < 0.5 else int(rr.integers(1, 5))
                ov = int(rr.choice([1, 2, 3, 4], p=[0.3, 0.25, 0.25, 0.2]))
                if ov == 4:
                    ov = 3 + int(rr.integers(1, 3000))
                if ll == 0 and ov == 3 and rep[0] == 1:
                    ov = 2
                ml = int(rr.integers(3, 40))
                # the executor's rule, to keep offsets within what is there
                if ov > 3:
                    rep = [ov - 3, rep[0], rep[1]]
                else:
                    idx = ov - 1 if ll else ov
                    if idx == 3:
                        rep = [rep[0] - 1, rep[0], rep[1]]
                    elif idx == 1:
                        rep = [rep[1], rep[0], rep[2]]
                    elif idx == 2:
                        rep = [rep[2], rep[0], rep[1]]
                seqs.append((ll, ml, ov))
            lc, oc, mc = _codes(seqs)
            k = b % 4
            # (tables that code every value the walk draws: the Repeat blocks behind them use them as they are)
            wide = (fse_mode(lc + list(range(5)), 6), fse_mode(oc + list(range(12)), 5), fse_mode(mc + list(range(37)), 6))
            modes = [("pre",) * 3, wide, ("rep",) * 3, ("pre", fse_mode(oc + list(range(12)), 8), "rep")][k]
            if k == 3 and b < 4:
                modes = ("pre",) * 3
            blocks.append(Z.comp(text(sum(s[0] for s in seqs) + 2), seqs, modes=modes))
        yield "rep_walk_%d" % seed, spec(blocks, window_log=17)




# ---- lookalikes of the flat fast paths ---------------------------------------------------------------------------------------
def lookalike_content():
    """LOOK_N blocks of LOOK_BLOCK packed bases, random A C G T but for runs of A in the blocks the variants change."""
    r = _rng(7)
    c = np.frombuffer(ACGT4, np.uint8)[r.integers(0, 16, LOOK_N * LOOK_BLOCK)].copy()
    for p in look_positions() + seq_block_positions(LOOK_N // 8) + seq_block_positions(LOOK_N // 8 + 2):
        c[p * LOOK_BLOCK:(p + 1) * LOOK_BLOCK] = RUN4
    return c.tobytes()


def look_positions():
    """0, 1, the middle, the last two, and where the blocks behind the changed one are one more than, exactly and one fewer
    than the STRIDE_TAIL blocks the stride index walks behind its prefix."""
    return sorted({0, 1, LOOK_N // 2, LOOK_N - STRIDE_TAIL - 2, LOOK_N - STRIDE_TAIL - 1, LOOK_N - STRIDE_TAIL, LOOK_N - 2, LOOK_N - 1})


def seq_block_positions(k):
    return [3 + (i * (LOOK_N - 6)) // k for i in range(k)]


def lookalike_frames():
    """The control (every block: Huffman literals under one flat 4-bit tree, FSE-coded weights, 4 streams, no sequences) and its
    variants: (name, blocks) with the blocks as compose() takes them."""
    content = lookalike_content()
    flat4 = flat_tree(ACGT4, 4)
    blk = lambda i: content[i * LOOK_BLOCK:(i + 1) * LOOK_BLOCK]
    ctrl = [Z.comp(blk(i), lit="huf", tree=flat4, fse_tree=True) for i in range(LOOK_N)]
    yield "look_control", ctrl
    run = bytes([RUN4]) * LOOK_BLOCK
    flat5 = flat_tree(ACGT4, 5)
    skew = Z.HufTree(weights_for({s: (3 if i == 0 else 5 if i >= 14 else 4) for i, s in enumerate(ACGT4)}))
    alt = [("size18", lambda i: Z.comp(blk(i), lit="huf", tree=flat4, fse_tree=True, lit_fmt=18)),
           ("treeless", lambda i: Z.comp(blk(i), lit="treeless")),
           ("raw_lits", lambda i: Z.comp(blk(i), lit="raw")),
           ("rle_lits", lambda i: Z.comp(blk(i), lit="rle")),
           ("raw_block", lambda i: Z.raw(blk(i))),
           ("rle_block", lambda i: Z.rle(RUN4, LOOK_BLOCK)),
           ("one_seq", lambda i: Z.comp(blk(i)[:1], [(1, LOOK_BLOCK - 1, 1 + 3)], lit="huf", tree=flat4, fse_tree=True, streams=1)),
           ("flat5", lambda i: Z.comp(blk(i), lit="huf", tree=flat5, fse_tree=True)),
           ("skewed", lambda i: Z.comp(blk(i), lit="huf", tree=skew, fse_tree=True)),
           # (the control's own tree cannot be written with direct weights: its last symbol, 0x88, needs 136 weights and the
           # direct form holds at most 128; so the direct-weights variant is another tree, of two symbols)
           ("direct_tree", lambda i: Z.comp(blk(i), lit="huf", tree=Z.HufTree([0] * 0x11 + [1, 1]), fse_tree=False))]
    for p in look_positions():
        assert blk(p) == run
        for name, mk in alt:
            if name == "treeless" and p == 0:
                continue
            b = list(ctrl)
            b[p] = mk(p)
            yield "look_%s@%d" % (name, p), b
        # one shorter block: the blocks behind it carry the rest (the frame's end then holds a short block)
        b = ctrl[:p] + [Z.comp(blk(p)[:LOOK_BLOCK // 2], lit="huf", tree=flat4, fse_tree=True)]
        rest = content[p * LOOK_BLOCK + LOOK_BLOCK // 2:]
        b += [Z.comp(rest[i:i + LOOK_BLOCK], lit="huf", tree=flat4, fse_tree=True) for i in range(0, len(rest), LOOK_BLOCK)]
        yield "look_short_block@%d" % p, b
    # a short last block: the last block split in two
    b = ctrl[:-1] + [Z.comp(blk(LOOK_N - 1)[:LOOK_BLOCK - 100], lit="huf", tree=flat4, fse_tree=True), Z.raw(blk(LOOK_N - 1)[-100:])]
    yield "look_short_last", b
    # mostly flat: sequence blocks at 1/8 of the blocks and just over
    for k in (LOOK_N // 8, LOOK_N // 8 + 2):
        b = list(ctrl)
        for p in seq_block_positions(k):
            b[p] = Z.comp(bytes([RUN4]) * 7, [(3, 1000, 1 + 3), (2, LOOK_BLOCK - 1000 - 7, 1)], lit="huf", tree=flat4, fse_tree=True)
        yield "look_seq_blocks_%d" % k, b


LOOK_VARIANTS = ("size18", "treeless", "raw_lits", "rle_lits", "raw_block", "rle_block", "one_seq", "flat5", "skewed", "direct_tree",
                 "short_block")


def look_features(name):
    if name == "look_control":
        return {"look:control"}
    if name.startswith("look_seq_blocks_"):
        k = int(name.rsplit("_", 1)[1])
        return {"look:seq_blocks:" + ("eighth" if k * 8 == LOOK_N else "over_eighth" if k * 8 > LOOK_N else "under")}
    if name == "look_short_last":
        return {"look:short_last"}
    v, p = name[5:].split("@")
    return {"look:variant:" + v, "look:pos:%s" % p}


# ---- a section's own bytes in the corpus's shapes ------------------------------------------------------------------------------
def recode(data, style):
    """A frame of data (any bytes) whose blocks take the corpus's shapes in turn: Raw and RLE blocks, raw literals in the 3-byte
    form, Huffman literals (1 or 4 streams, direct or FSE-coded weights, treeless where the last tree codes the block) and, where
    the bytes hold runs, sequences (ll, run - 1, offset 1) under predefined, FSE-compressed and Repeat tables with the repeat code
    1 carried across blocks."""
    sizes = (120000, 777, 32768, 4101, 65537, 20000, 6)
    blocks, pos, i, tree, have_rep, prev_mode = [], 0, 0, None, False, None
    arr = np.frombuffer(data, np.uint8)
    while pos < len(data):
        part = data[pos:pos + sizes[(i + style) % len(sizes)]]
        kind = (i * 3 + style) % 7
        a = arr[pos:pos + len(part)]
        pos += len(part)
        i += 1
        if kind == 0:
            blocks.append(Z.raw(part)); continue
        if kind == 1:
            blocks.append(Z.rle(part[0], len(part)) if part == part[:1] * len(part) else Z.comp(part, lit="raw", lit_fmt=3)); continue
        seqs, lits, c = [], bytearray(), 0
        if kind >= 4:                                           # runs of 8 or more equal bytes: a literal, then a match one back
            edge = np.flatnonzero(np.diff(a) != 0) + 1
            starts = np.concatenate(([0], edge)); ends = np.concatenate((edge, [len(a)]))
            for s0, e0 in zip(starts.tolist(), ends.tolist()):
                if e0 - s0 >= 8:
                    lits += part[c:s0 + 1]
                    seqs.append((s0 + 1 - c, e0 - s0 - 1, 1 if have_rep else 4))
                    have_rep = True
                    c = e0
            lits += part[c:]
        else:
            lits = bytearray(part)
        lits = bytes(lits)
        modes = ("pre",) * 3
        if seqs:
            m = i % 3
            if m == 1:
                lc, oc, mc = _codes(seqs)
                modes = (fse_mode(lc, 6), fse_mode(oc, 5), fse_mode(mc, 6))
            elif m == 2 and prev_mode == "pre":
                modes = ("rep",) * 3                            # Repeat of the predefined tables: they code every value
            prev_mode = "pre" if modes[0] == "pre" else "rep" if modes[0] == "rep" else "fse"
            if modes[0] == "rep":
                prev_mode = "pre"
        if len(lits) < 6:
            blocks.append(Z.comp(lits, seqs, lit="raw", modes=modes)); continue
        if tree is not None and kind in (3, 6) and all(tree.len[x] > 0 for x in set(lits)):
            blocks.append(Z.comp(lits, seqs, lit="treeless", streams=1 if len(lits) <= 1023 and kind == 3 else 4, modes=modes)); continue
        t = tree_of(lits, 11)
        ws = t.weights[:-1]
        fse = len(ws) > 129 or (kind % 2 == 0 and len(set(ws)) > 1)
        if int(np.sum(t.len[np.frombuffer(lits, np.uint8)])) // 8 > 110000:
            blocks.append(Z.comp(lits, seqs, lit="raw", modes=modes)); continue
        tree = t
        blocks.append(Z.comp(lits, seqs, lit="huf", tree=t, fse_tree=fse, streams=1 if len(lits) <= 1023 else 4, modes=modes))
    return blocks


def compose_look(blocks):
    return Z.compose(blocks, window_log=23)


# ---- the corpus ----------------------------------------------------------------------------------------------------------------
def _pad(blocks, kw, size, seed):
    r = _rng(seed)
    kw = dict(kw)
    kw.pop("fcs", None)
    win = (1 << kw.get("window_log", 17)) + ((1 << kw.get("window_log", 17)) >> 3) * kw.get("window_mantissa", 0)
    bmax = Z.BLOCK_MAX if kw.get("single_segment") else min(Z.BLOCK_MAX, win)
    total = {"mid": 40 * 1024, "big": (4 << 20) + 200 * 1024}[size]
    def raws(n):
        out = []
        while n > 0:
            k = min(n, bmax)
            out.append(Z.raw(r.integers(0, 256, k, dtype=np.uint8).tobytes()))
            n -= k
        return out
    front = raws(total // 2)
    # (the family's blocks end in a zero-size Raw block at times: it stays last)
    if blocks and blocks[-1]["type"] == "raw" and not blocks[-1]["data"]:
        return front + blocks[:-1] + raws(total - total // 2) + blocks[-1:], kw
    return front + blocks + raws(total - total // 2), kw


def small_frames(blocks, kw, split):
    """The blocks as frames within the small-frame decoder's limits: one frame, or -- split leading blocks in front of each part --
    as many as it takes."""
    def fits(b):
        fr, content, feat = Z.compose(b, **kw)
        ok = len(fr) <= SMALL_SRC and len(content) + 64 <= SMALL_OUT and all(len(x.get("seqs", ())) <= SMALL_SEQ for x in b)
        return ok, (fr, content, feat)
    ok, one = fits(blocks)
    if ok:
        return [one]
    assert split is not None, "a family that must stay one frame does not fit the small-frame decoder"
    out, cur, done = [], list(blocks[:split]), None
    for b in blocks[split:]:
        ok, got = fits(cur + [b])
        if ok:
            cur, done = cur + [b], got
            continue
        assert done is not None, "a block that does not fit the small-frame decoder alone"
        out.append(done)
        cur = list(blocks[:split]) + [b]
        ok, done = fits(cur)
        assert ok, "a block that does not fit the small-frame decoder alone"
    out.append(done)
    return out


def corpus(sizes=("full", "small", "mid", "big"), look=True):
    """(name, frame, content, features) for every frame; format and state families at each of sizes, then the lookalikes."""
    seed = 100
    for fam, gen in (("format", format_frames), ("state", state_frames)):
        if "small" in sizes:
            for name, sp in gen(small=True):
                if isinstance(sp[0], bytes):                    # a concatenation, composed already
                    continue
                blocks, kw, split = sp
                parts = small_frames(blocks, kw, split)
                for j, (fr, content, feat) in enumerate(parts):
                    yield name + "@small" + (".%d" % j if len(parts) > 1 else ""), fr, content, set(feat) | {"family:" + fam, "size:small"}
        for name, sp in gen():
            if isinstance(sp[0], bytes):
                fr, content, feat = sp
                yield name, fr, content, set(feat) | {"family:" + fam, "size:small"}
                continue
            blocks, kw, split = sp
            for size in sizes:
                if size == "small":
                    continue
                seed += 1
                if size == "full":
                    fr, content, feat = Z.compose(blocks, **kw)
                else:
                    if size == "big":
                        kw = dict(kw, checksum=False)           # (the checksum of 4 MiB in plain Python: the smaller frames have it)
                    pb, pkw = _pad(blocks, kw, size, seed)
                    fr, content, feat = Z.compose(pb, **pkw)
                yield name + "@" + size, fr, content, set(feat) | {"family:" + fam, "size:" + size}
    if look:
        for name, blocks in lookalike_frames():
            fr, content, feat = compose_look(blocks)
            yield name, fr, content, set(feat) | {"family:look"} | look_features(name)
