"""The plan of the literals-planner tests (tests/huf_plan.py) held to its own claims, its models held to each other, its streams run
through the host build of the planner (tests/emul: emul_zstd_compress, zenc_plan_block behind the encoder's own stream writer -- 11
bits, FSE-coded weights tried), the oracle's listing of literals sections held to what zstd_compose composed and to libzstd's frames,
and the checks shown to reject frames composed to be wrong in the ways test_gpu_huf_plan.py looks for.  No GPU.

A code of 12 bits cannot be written into a zstd frame at all (Max_Number_of_Bits is 11: RFC 8878 4.2.1): the frame composed with one is
rejected by the decode, and the length limit's own check is shown on a 10-bit code under the mask's limit of 9 and an 8-bit code
under the 7 of the sequence and quality streams."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import huf_plan as P
import zstd_compose as Z
import zstd_corpus
from conftest import ROOT


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(ROOT, "tests", "emul", "libzstd_emul.so")
    if not os.path.exists(so):
        env = dict(os.environ, PATH="/opt/rocm/bin:" + os.environ.get("PATH", ""))
        subprocess.check_call(["make", "-s", "-C", ROOT, "emul"], env=env)
    L = ctypes.CDLL(so)
    L.emul_zstd_compress.restype = ctypes.c_longlong
    L.emul_zstd_compress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
    return L


@pytest.fixture(scope="module")
def libzstd():
    for cand in ("/opt/conda/lib/libzstd.so", "libzstd.so.1"):
        try:
            z = ctypes.CDLL(cand)
        except OSError:
            continue
        z.ZSTD_compress.restype = ctypes.c_size_t
        z.ZSTD_compress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
        z.ZSTD_compressBound.restype = ctypes.c_size_t
        z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        return z
    return None


# ---- the models against each other ----------------------------------------------------------------------------------------------------------
def _profiles():
    """(name, counts) of every profile of the plan at the sizes the issue's throwaway run used, and the pack's own cells."""
    out = [("pack." + c.name, list(c.counts)) for c in P.pack_cells()]
    out += [("shape." + c.name, list(c.counts)) for c in P.big_shapes().values()]
    for bn in P.SEAM_BNS:
        out += [("seam%d.%s" % (bn, c.name), list(c.counts)) for c in P.seam_cells(bn)]
    for n in range(2, 65):
        out.append(("linear_%d" % n, P.prof_linear(n, 32768)))
        out.append(("geo0.7_%d" % n, P.prof_geo(n, 32768)))
        out.append(("quadratic_%d" % n, P.prof_quadratic(n, 32768)))
        if n >= 4:
            out.append(("pairs_%d" % n, P.prof_pairs(n, 32768)))
        if n <= 21:
            out.append(("fib_%d" % n, P.prof_fib(n, 32768)))
        if n <= 23:
            f = [1, 1]
            while len(f) < n:
                f.append(f[-1] + f[-2])
            out.append(("true_fib_%d" % n, f[::-1]))
    for n in range(65, 255, 7):
        out.append(("linear_%d" % n, P.prof_linear(n, 32768)))
        out.append(("geo0.97_%d" % n, P.prof_geo(n, 32768, 0.97)))
        out.append(("quadratic_%d" % n, P.prof_quadratic(n, 32768)))
    return out


def test_the_documented_construction_against_heap_and_package_merge(capsys):
    """plan_lengths is an optimal code wherever the unlimited depth fits the limit (its cost is the heap's) and lies between
    package-merge and fixed width wherever it does not; the lengths are complete and ordered by count.  The excess over package-merge
    is printed per cell, not bounded: DESIGN.md has the table."""
    worst, limited, never_zero = (0.0, ""), 0, 0
    for name, counts in _profiles():
        hist = counts + [0] * (256 - len(counts))
        n = len(counts)
        if n < 2:
            continue
        hc = P.huffman_cost(hist)
        for L in (7, 9, 11):
            if n > 64 and L < 9:
                continue
            lens, log, depth = P.plan_lengths(hist, L)
            assert log, (name, L)                                  # the documented rule always ends on a complete code on these inputs
            never_zero += 1
            assert sum(1 << (L - l) for l in lens if l) == 1 << L and max(lens) == log <= L, (name, L)
            order = sorted(range(n), key=lambda s: (counts[s], s))
            assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:])), (name, L)
            cost = sum(c * l for c, l in zip(hist, lens))
            if depth <= L:
                assert cost == hc, (name, L, cost, hc)
            else:
                lc = P.limited_cost(hist, L)
                assert hc <= lc <= cost <= P.fixed_width_cost(hist), (name, L, hc, lc, cost, P.fixed_width_cost(hist))
                limited += 1
                ex = 100.0 * (cost - lc) / lc
                if ex > worst[0]:
                    worst = (ex, "%s at %d bits" % (name, L))
    assert limited > 100 and never_zero > 1000
    rows, _ = P.excess_table()
    with capsys.disabled():
        print("\nlength limiting against package-merge, the cells of the pack whose unlimited depth is above the limit:")
        print("  %-24s %7s %5s %5s %9s %9s %7s" % ("cell", "symbols", "limit", "depth", "cost", "optimal", "excess"))
        for name, n, L, depth, cost, lc, ex, _ok in rows:
            print("  %-24s %7d %5d %5d %9d %9d %6.2f%%" % (name, n, L, depth, cost, lc, ex))
        print("  worst over %d limited runs of the profiles (2..64 symbols at 7, 9 and 11 bits, 65..254 in steps of 7 at 9 and 11): %.2f%% (%s)" % (limited, worst[0], worst[1]))
    assert all(ok for *_x, ok in rows)


def test_package_merge_is_optimal_on_small_alphabets():
    """limited_cost against every length assignment of up to six symbols that satisfies Kraft's inequality."""
    import itertools
    rng = np.random.default_rng(1)
    for _ in range(40):
        n = int(rng.integers(2, 7))
        w = [int(x) for x in rng.integers(1, 50, n)]
        for L in (3, 4):
            if (1 << L) < n:
                continue
            best = min(sum(a * b for a, b in zip(w, ls)) for ls in itertools.product(range(1, L + 1), repeat=n) if sum(1 << (L - l) for l in ls) <= 1 << L)
            assert P.limited_cost(w, L) == best, (w, L)
        assert P.limited_cost(w, 11) == P.huffman_cost(w)


def test_the_split_and_the_quarters():
    for bn, nblk in ((4096, 100), (1001, 40), (1025, 2), (16385, 2), (131072, 2), (1024, 4096), (255, 1), (1, 1)):
        blog = P.block_log_for(bn, nblk)
        assert P.split_even(bn * nblk, 1 << blog) == [b * bn for b in range(nblk + 1)]
    for bn in (1, 5, 63, 64, 65, 1001, 1002, 1003, 4096):
        q = P.quarter_bounds(bn)
        per = (bn + 3) // 4
        assert q[0] == 0 and q[4] == bn and all(q[k] == min(k * per, bn) for k in range(4))
    assert all(((bn + 3) // 4) % 8 for bn in P.SEAM_BNS) and [bn % 4 for bn in P.SEAM_BNS] == [1, 2, 3]
    assert [P.direct_tree_bytes(n) for n in (1, 2, 127, 128)] == [2, 2, 65, 65]
    assert [P.lit_header_bytes(a, b) for a, b in ((1023, 1023), (1024, 10), (10, 1024), (16383, 16383), (16384, 5), (5, 16384))] == [3, 4, 4, 4, 5, 5]


# ---- the cells and texts are what the plan says -------------------------------------------------------------------------------------------------
def test_every_cell_is_what_the_plan_says(oracle):
    """Every block has its cell's histogram on the symbols the rule allows, the placed symbol lies where the cell says, the archive
    routes' texts give the planned stream back under the oracle's split, the cases are the same at every seed but for the letters."""
    names = None
    for seed in P.SEEDS:
        cases = [c for car in P.CARRIERS for c in P.small_cases(seed, car)]
        for c in cases:
            Pm = P.CARRIERS[c.carrier]
            d = np.frombuffer(c.data, dtype=np.uint8)
            assert len(d) == c.bn * c.nblk <= P.MAX_STREAM
            if c.nblk:
                assert P.split_even(len(d), 1 << c.blog) == [b * c.bn for b in range(c.nblk + 1)], c.name
                assert set(np.unique(d)) <= set(Pm.alphabet), c.name
            for b, cell in enumerate(c.cells):
                blk = d[b * c.bn:(b + 1) * c.bn]
                h = np.bincount(blk, minlength=256)
                want = cell.counts if not (cell.rule[0] == "wide" and len(cell.counts) > len(Pm.alphabet)) else P.prof_equal(len(Pm.alphabet), c.bn)
                assert sorted(h[h > 0]) == sorted(want), (c.name, cell.name)
                q = P.quarter_bounds(c.bn)
                rare = np.flatnonzero(blk == P.symbols_of(cell, Pm, seed if c.cells[0].cls != "gain" else 0)[-1]) if cell.place != "shuffle" and cell.place[0] != "marker" else None
                if cell.rule[0] == "last":
                    assert int(np.flatnonzero(h)[-1]) == cell.rule[1]
                if cell.rule[0] == "ends":
                    assert h[0] and h[255]
                if cell.rule[0] == "pairs":
                    assert set(np.flatnonzero(h)) <= set(P.PAIR_CODES)
                if cell.place == "shuffle":
                    continue
                if cell.place[0] == "quarter_first":
                    assert list(rare) == [q[cell.place[1]]]
                elif cell.place[0] == "quarter_last":
                    assert list(rare) == [q[cell.place[1] + 1] - 1]
                elif cell.place[0] == "block_last":
                    assert list(rare) == [c.bn - 1]
                elif cell.place[0] == "only_quarter":
                    assert len(rare) == 9 and all(q[cell.place[1]] <= i < q[cell.place[1] + 1] for i in rare)
                elif cell.place[0] == "marker":
                    lens = np.array(P.code_of(h, c.bn, Pm)[0])
                    assert int(lens[blk[q[0]:q[1]]].sum()) % 8 == cell.place[1], (c.name, cell.name)
            if Pm.route in P.STREAM_INDEX and c.nblk:
                text = P.text_of(c)
                s = oracle.split_text(text)
                got = (s.ids, s.comments, s.lengths, s.mask, s.seq, s.qual)[P.STREAM_INDEX[Pm.route]]
                assert got == c.data, (c.name, len(got), len(c.data))
        assert names is None or names == [c.name for c in cases]
        names = [c.name for c in cases]
    assert len(set(names)) == len(names)


def test_the_large_cases_are_what_the_plan_says(oracle):
    """256 and 4096 blocks of the dozen shapes: sampled blocks hold A, B and C only, B nowhere else; a shape the frame's code lacks
    lies between the samples; the texts give the streams back."""
    lay = P.big_layout(P.FRAME_BLOCKS)
    sampled = P.sampled_blocks(P.FRAME_BLOCKS)
    assert len(sampled) == 256 and sampled[1] == 16 and {lay[b] for b in sampled} == {"A", "B", "C"}
    assert "B" not in {lay[b] for b in range(P.FRAME_BLOCKS) if b % 16} and {"C", "D", "E", "F", "G", "I", "J", "K"} <= {lay[b] for b in range(P.FRAME_BLOCKS) if b % 16}
    assert P.sampled_blocks(P.DEFER_BLOCKS) == []
    sh = P.big_shapes()
    for car in ("qual", "seq", "mask", "z1"):
        Pm = P.CARRIERS[car]
        used = lambda k: set(P.symbols_of(sh[k], Pm, P.SEED))
        assert not used("E") & (used("A") | used("B") | used("C")), car
        assert used("D") <= used("A") and used("A2") == used("A")
    for car in ("qual", "mask", "seq"):
        for c in P.big_cases(P.SEED, car):
            assert len(c.data) == c.nblk * P.BIG_BN <= P.MAX_STREAM and c.blog == 10
            if c.nblk == P.FRAME_BLOCKS and "own_trees" in c.name:
                continue
            text = P.text_of(c)
            assert len(text) < 48 << 20, (c.name, len(text))
            s = oracle.split_text(text)
            assert (s.ids, s.comments, s.lengths, s.mask, s.seq, s.qual)[P.STREAM_INDEX[P.CARRIERS[car].route]] == c.data, c.name
    # the shapes pass or miss the frame's 3 % rule by a per cent at least: single-precision entropies decide the same way
    for car in ("qual", "seq"):
        Pm = P.CARRIERS[car]
        c = P.big_case(P.SEED, car, P.FRAME_BLOCKS)
        d = np.frombuffer(c.data, dtype=np.uint8)
        hs = [P.hist4_of(d[b * c.bn:(b + 1) * c.bn]).sum(axis=0) for b in P.sampled_blocks(c.nblk)]
        flen, flog, flimit = P.frame_code_model(hs, Pm)
        assert flog <= flimit == 7 and sum(1 << (11 - l) for l in flen if l) == 1 << 11
        ratio, took = P.frame_ratio(hs, flen), {}
        for b in range(64):
            takes, margin = P.frame_rule(P.hist4_of(d[b * c.bn:(b + 1) * c.bn]).sum(axis=0), flen, ratio)
            assert margin > 0.01, (car, lay[b], margin)
            took[lay[b]] = takes
        assert took["A"] and took["A2"] and not any(took[k] for k in "BCDEFGIJK"), took
    assert P.big_case(P.SEED, "qual", P.FRAME_BLOCKS).frame_tree and not P.big_cases(P.SEED, "qual")[2].frame_tree and not P.big_case(P.SEED, "mask", P.FRAME_BLOCKS).frame_tree


# ---- the host build of the planner ------------------------------------------------------------------------------------------------------------------
def run_emul(emul, c):
    cap = len(c.data) + 3 * c.nblk + 64
    out = ctypes.create_string_buffer(cap)
    n = emul.emul_zstd_compress(c.data, len(c.data), c.bn, out, cap)
    assert n > 0, (c.name, n)
    return out.raw[:n]


def test_the_host_build_of_the_planner_block_by_block(emul, oracle, capsys):
    """Every small case through zenc_plan_block: the same per-block assertions the GPU test makes, and the coverage table of every
    carrier by the model's paths -- no cell of a carrier without a block or a reason."""
    cov, desc, n = P.Coverage(), {}, 0
    for seed in P.SEEDS:
        for c in P.small_cases(seed, "emul"):
            frame = run_emul(emul, c)
            P.check_decodes(oracle, frame, c.data)
            paths = P.check_frame(c, frame, oracle.zstd_literals(frame), desc)
            cov.add(c, paths)
            n += len(paths)
    assert n > 500
    # the cells of the large cases and of the GPU carriers, by the model alone (nothing is compressed here)
    for car in P.GPU_CARRIERS:
        Pm = P.CARRIERS[car]
        for c in P.all_cases(P.SEED, car):
            d = np.frombuffer(c.data, dtype=np.uint8)
            cached = set()
            for b in P.sampled_blocks(c.nblk):
                m = P.block_model(d[b * c.bn:(b + 1) * c.bn], Pm)[1]
                if m.log:
                    cached.add(P._weights(m.lens, m.log))
            paths = []
            for b in range(c.nblk):
                m = P.block_model(d[b * c.bn:(b + 1) * c.bn], Pm)[1]
                p = m.path
                if m.log and not p.endswith("W"):
                    w = P._weights(m.lens, m.log)
                    direct_w = not Pm.try_fse and m.lastw <= 128
                    if c.nblk >= P.FRAME_BLOCKS:
                        p += "C" if w in cached else "M"
                    if c.nblk >= P.DEFER_BLOCKS and not direct_w and w not in cached:
                        p += "D"
                paths.append(p)
            cov.add(c, paths)
    with capsys.disabled():
        print("\n" + cov.table(("emul",) + P.GPU_CARRIERS, "the host build ran the emul column (%d blocks over seeds %s); the others are the model's paths" % (n, list(P.SEEDS))))
        print("  (the large cases have no host build: blocks of the frame's code, T, and of the flat scan, Q, show on the kernels' table only)")
    holes = cov.empty(("emul",) + P.GPU_CARRIERS)
    assert not holes, holes[:10]
    assert set("FRSLWE") <= cov.letters() and {"P", "C", "M", "D"} <= cov.letters()


# ---- the oracle's listing ---------------------------------------------------------------------------------------------------------------------------
def test_the_listing_against_what_was_composed(oracle):
    """oracle.zstd_literals on every frame of the corpus of composed frames: what it lists is what the feature strings say was composed
    (literals types, header forms, 1 or 4 streams, direct or FSE-coded trees, the longest code)."""
    seen = set()
    def listed(f):
        return (f.startswith(("lit:raw:h", "lit:rle:h")) and f.count(":") == 2) or f.startswith(("huf:streams:", "huf:size:", "huf:maxbits:")) \
            or f in ("huf:tree:fse", "huf:tree:direct", "lit:treeless")

    for name, frame, content, feats in zstd_corpus.corpus(sizes=("full",), look=False):
        frames = Z.split_frames(frame)
        try:
            L = oracle.zstd_literals(frame)
        except ValueError:
            continue                                               # (a frame the corpus holds for what is wrong with it)
        got = set()
        for b in range(len(L)):
            if L.block_type[b] != 2:
                continue
            lt = int(L.lit_type[b])
            if lt in (0, 1):
                got.add("lit:%s:h%d" % ("raw" if lt == 0 else "rle", int(L.header_bytes[b])))
                continue
            got.add("huf:streams:%d" % int(L.n_streams[b]))
            got.add("huf:size:%d" % {3: 10, 4: 14, 5: 18}[int(L.header_bytes[b])])
            if lt == 2:
                got.add("huf:tree:%s" % ("fse" if L.tree_fse[b] else "direct"))
                got.add("huf:maxbits:%d" % int(L.len[b].max()))
                assert sum(1 << (11 - int(l)) for l in L.len[b] if l) == 1 << 11
            else:
                got.add("lit:treeless")
        if len(frames) == 1:
            want = {f for f in feats if listed(f)}
            assert got == want, (name, sorted(want - got), sorted(got - want))
        seen |= got
    assert {"huf:streams:1", "huf:streams:4", "huf:size:10", "huf:size:14", "huf:size:18", "huf:tree:fse", "huf:tree:direct", "lit:treeless", "huf:maxbits:11"} <= seen, sorted(seen)


def test_the_listing_field_by_field(oracle):
    tree = Z.HufTree([3, 2, 1, 1])
    lits = bytes(np.random.default_rng(0).choice(4, 2000, p=[.5, .25, .125, .125]).astype("u1"))
    frame, content, _ = Z.compose([Z.comp(lits=lits, lit="huf", tree=tree, streams=4), Z.comp(lits=lits[:500], lit="treeless", streams=1), Z.raw(b"abc"),
                                   Z.rle(7, 9), Z.comp(lits=lits[:300], lit="huf", tree=tree, fse_tree=True, streams=4, seqs=[(10, 5, 4 + 3)]),
                                   Z.comp(lits=b"xyz"), Z.comp(lits=b"q" * 40, lit="rle")])
    L = oracle.zstd_literals(frame)
    assert L.size == len(content)
    assert list(L.block_type) == [2, 2, 0, 1, 2, 2, 2] and list(L.decoded_size) == [2000, 500, 3, 9, 305, 3, 40]
    assert list(L.lit_type) == [2, 3, -1, -1, 2, 0, 1] and list(L.regen) == [2000, 500, 0, 0, 300, 3, 40] and list(L.n_streams) == [4, 1, 0, 0, 4, 0, 0]
    assert list(L.header_bytes) == [4, 3, 0, 0, 3, 1, 2] and list(L.n_sequences) == [0, 0, 0, 0, 1, 0, 0]
    assert list(L.tree_bytes) == [3, 0, 0, 0, 7, 0, 0] and list(L.tree_fse) == [0, 0, 0, 0, 1, 0, 0] and list(L.n_weights) == [3, 0, 0, 0, 3, 0, 0]
    assert frame[int(L.tree_offset[0]):][:3] == tree.describe() and frame[int(L.tree_offset[4]):][:7] == tree.describe(fse=True)
    for b in (0, 1, 4):
        assert list(L.len[b][:5]) == [1, 2, 3, 3, 0]
        n = int(L.regen[b])
        if L.n_streams[b] == 4:
            h4 = P.hist4_of(lits[:n])
            assert [int(x) for x in L.stream_size[b]] == P.stream_bytes(h4, L.len[b])
            assert int(L.comp[b]) == int(L.tree_bytes[b]) + 6 + int(L.stream_size[b].sum())
        assert int(L.frame_size[b]) == 3 + int(L.header_bytes[b]) + int(L.comp[b]) + (1 if b != 4 else int(L.frame_size[b]) - 3 - int(L.header_bytes[b]) - int(L.comp[b]))
    assert list(L.frame_size[[2, 3]]) == [6, 4] and not L.len[2].any()


def test_the_listing_against_libzstd_frames(oracle, libzstd):
    """libzstd's own frames of the plan's streams: the listing decodes them, the stream sizes follow from the listed lengths, every tree
    is complete, and a treeless section shows the lengths of the tree in front of it."""
    if libzstd is None:
        return                                                     # (no libzstd on this machine: the composed frames above are the listing's reference)
    checked = 0
    for c in P.small_cases(P.SEED, "z1")[:6]:
        for level in (1, 3):
            cap = libzstd.ZSTD_compressBound(len(c.data))
            out = ctypes.create_string_buffer(cap)
            n = libzstd.ZSTD_compress(out, cap, c.data, len(c.data), level)
            frame = out.raw[:n]
            L = oracle.zstd_literals(frame)
            assert L.size == len(c.data) and int(L.decoded_size.sum()) == len(c.data)
            prev = None
            for b in range(len(L)):
                if L.block_type[b] != 2 or L.lit_type[b] < 2:
                    continue
                lens = L.len[b]
                assert sum(1 << (11 - int(l)) for l in lens if l) == 1 << 11
                assert int(L.header_bytes[b]) >= P.lit_header_bytes(int(L.regen[b]), int(L.comp[b]))
                if L.lit_type[b] == 3:
                    assert prev is not None and np.array_equal(lens, prev) and L.tree_bytes[b] == 0
                else:
                    assert L.tree_bytes[b] > 0 and int(L.n_weights[b]) == int(np.flatnonzero(lens)[-1])
                prev = lens
                streams = int(L.n_streams[b])
                assert int(L.comp[b]) == int(L.tree_bytes[b]) + (6 if streams == 4 else 0) + int(L.stream_size[b].sum())
                checked += 1
    assert checked > 5


# ---- frames composed to be wrong ----------------------------------------------------------------------------------------------------------------------
def _tree_of(lens):
    """A zstd_compose tree of 256 code lengths (weights up to the last present symbol)."""
    lens = [int(l) for l in lens]
    log, last = max(lens), max(s for s in range(256) if lens[s])
    return Z.HufTree([log + 1 - l if l else 0 for l in lens[:last + 1]])


def _composed_case(carrier, blocks_bytes, trees, lit_fmt=None, name="composed"):
    """A frame of Huffman blocks with the given trees (None: the model's own), four streams each, and the Case that describes it."""
    Pm = P.CARRIERS[carrier]
    bn = len(blocks_bytes[0])
    cells = [P.Cell("composed", "block%d" % i, [], ("any", "low"), "shuffle") for i in range(len(blocks_bytes))]
    blocks = []
    for blk, t in zip(blocks_bytes, trees):
        h4, m = P.block_model(np.frombuffer(blk, dtype=np.uint8), Pm)
        blocks.append(Z.comp(lits=blk, lit="huf", tree=t or _tree_of(m.lens), streams=4, lit_fmt=lit_fmt))
    frame, content, _ = Z.compose(blocks, window_log=17)
    nblk = len(blocks_bytes)
    c = P.Case(name, carrier, b"".join(blocks_bytes), bn, nblk, P.block_log_for(bn, nblk), {}, cells, {}, False)
    assert content == c.data
    return c, frame


def test_the_checks_reject_composed_bad_frames(oracle, capsys):
    seen = {}

    def rejected(name, fn):
        with pytest.raises(P.Reject) as e:
            fn()
        seen[name] = e.value.reason
        return e.value.reason

    def check(c, frame):
        P.check_decodes(oracle, frame, c.data)
        return P.check_frame(c, frame, oracle.zstd_literals(frame))

    cell = P.Cell("composed", "geo12", P.prof_geo(12, 2048), ("any", "low"), "shuffle")
    blk = P.block_of(cell, P.CARRIERS["z1"], 0).tobytes()
    good, f_good = _composed_case("z1", [blk, blk], [None, None])
    assert check(good, f_good) == ["R", "R"]                       # the model's own code passes every check

    # 1. a complete code that is not the cheapest: two symbols of unequal counts trade their lengths
    m = P.block_model(np.frombuffer(blk, dtype=np.uint8), P.CARRIERS["z1"])[1]
    lens = list(m.lens)
    hist = np.bincount(np.frombuffer(blk, dtype=np.uint8), minlength=256)
    order = [int(s) for s in np.argsort(-hist)[:12]]
    a, b = next((x, y) for x in order for y in order if lens[x] < lens[y] and hist[x] > hist[y])
    lens[a], lens[b] = lens[b], lens[a]
    c1, f1 = _composed_case("z1", [blk, blk], [None, _tree_of(lens)])
    assert rejected("a complete code with two lengths traded", lambda: check(c1, f1)) == "order"
    # ... and one that keeps the order of the counts but is deeper than it has to be: a fixed-width code of 4 bits for 12 symbols is
    # not complete, so 4 symbols take 3 bits and 8 take 4 (complete, ordered, not optimal for geometric counts)
    srt = sorted(order, key=lambda s: (-int(hist[s]), s))
    lens2 = [0] * 256
    for i, s in enumerate(srt):
        lens2[s] = 3 if i < 4 else 4
    c1b, f1b = _composed_case("z1", [blk], [_tree_of(lens2)])
    assert rejected("a suboptimal complete code", lambda: check(c1b, f1b)) == "cost"

    # 2. a 12-bit length: no zstd frame can say it -- weights that sum to 2^12 are rejected by the decode
    deep = Z.HufTree([11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1])
    lits = bytes([0] * 40 + list(range(12)) * 2)
    f12, content12, _ = Z.compose([Z.comp(lits=lits, lit="huf", tree=deep, streams=1)], window_log=17)
    P.check_decodes(oracle, f12, content12)
    L12 = oracle.zstd_literals(f12)
    at = int(L12.tree_offset[0])
    assert f12[at] == 127 + 11 and f12[at + 1] == 0xBA
    bad12 = f12[:at + 1] + bytes([0xBB]) + f12[at + 2:]           # weights 11, 11, 9, ...: the sum passes 2^11, the depth would be 12
    assert rejected("a 12-bit length", lambda: P.check_decodes(oracle, bad12, content12)) == "decode"
    # ... and a length above the carrier's limit: ten bits under the mask's 9, eight under the quality stream's 7
    for car, n, r in (("mask", 14, 0.5), ("qual", 12, 0.5)):
        Pm = P.CARRIERS[car]
        cellL = P.Cell("composed", "pow2", P.prof_pow2(n, 4096), ("any", "low"), "shuffle")
        blkL = P.block_of(cellL, Pm, 0).tobytes()
        mL = P.block_model(np.frombuffer(blkL, dtype=np.uint8), Pm)[1]
        assert mL.depth > Pm.limit == mL.log
        free = P.plan_lengths(np.bincount(np.frombuffer(blkL, dtype=np.uint8), minlength=256), Pm.limit + 1)[0]
        assert max(free) == Pm.limit + 1
        cL, fL = _composed_case(car, [blkL], [_tree_of(free)])
        assert rejected("a code of %d bits on the %s carrier" % (Pm.limit + 1, car), lambda: check(cL, fL)) == "limit"
        cLg, fLg = _composed_case(car, [blkL], [None])
        assert check(cLg, fLg) == ["RL"]

    # 3. a literals header one form too wide
    c3, f3 = _composed_case("z1", [blk[:900], blk[900:1800]], [None, None], lit_fmt=14)
    assert rejected("a header one form too wide", lambda: check(c3, f3)) == "header"
    c3g, f3g = _composed_case("z1", [blk[:900], blk[900:1800]], [None, None])
    check(c3g, f3g)

    # 4. a Huffman block one byte larger than Raw: near-equal counts at the model's own edge
    g = {c.name: c for c in P.gain_cells(P.CARRIERS["z1"])}
    for nm, ok in (("one_byte_gained", True), ("no_byte_gained", False), ("one_byte_lost", False)):
        blkG = P.block_of(g[nm], P.CARRIERS["z1"], 0).tobytes()
        cG, fG = _composed_case("z1", [blkG], [None])
        L = oracle.zstd_literals(fG)
        mG = P.block_model(np.frombuffer(blkG, dtype=np.uint8), P.CARRIERS["z1"])[1]
        assert int(L.frame_size[0]) == mG.csize_hi == 3 + len(blkG) + {"one_byte_gained": -1, "no_byte_gained": 0, "one_byte_lost": 1}[nm]
        if ok:
            check(cG, fG)
        else:
            assert rejected("a Huffman block %s" % nm.replace("_", " "), lambda: check(cG, fG)) == ("larger than Raw" if nm == "one_byte_lost" else "raw/huffman")
    # ... and a Raw block where Huffman coding pays
    raw_frame, _, _ = Z.compose([Z.raw(blk), Z.raw(blk)], window_log=17)
    assert rejected("a Raw block where Huffman coding pays", lambda: check(good, raw_frame)) == "raw/huffman"

    # 5. a stream size that the listed lengths do not give cannot be composed into a frame that decodes; blocks that are not the plan's can
    other = good._replace(bn=1024, nblk=4, cells=good.cells * 2)
    assert rejected("blocks that are not the plan's split", lambda: P.check_frame(other, f_good, oracle.zstd_literals(f_good))) == "plan out of date"
    # a direct description where FSE-coded weights are smaller is fine at level 1, an FSE-coded one is not
    blocks = [Z.comp(lits=blk, lit="huf", tree=_tree_of(m.lens), fse_tree=True, streams=4)] * 2
    f_fse, _, _ = Z.compose(blocks, window_log=17)
    assert rejected("FSE-coded weights at level 1", lambda: check(good, f_fse)) == "tree"
    with capsys.disabled():
        print("\ncomposed bad frames, and what rejected them:")
        for k, v in seen.items():
            print("  %-52s %s" % (k, v))
    assert {"order", "cost", "decode", "limit", "header", "larger than Raw", "raw/huffman", "plan out of date", "tree"} <= set(seen.values())
