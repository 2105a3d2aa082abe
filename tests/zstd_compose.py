"""A zstd frame composer written from RFC 8878 alone -- TEST HELPER, not a test.

Every encoding choice of a frame is stated by the caller as data: the frame header (Frame_Content_Size width, single segment or a
Window_Descriptor, checksum), the blocks (Raw, RLE, Compressed), a Compressed block's literals (Raw / RLE with the size format
picked, Huffman with 1 or 4 streams, a size format, the tree as weights written direct or FSE-coded, or treeless) and its
sequences ((ll, ml, offset_value) with offset_value 1..3 the repeat codes; the count in its 1/2/3-byte form; LL / OF / ML each
Predefined, RLE, FSE-compressed with the caller's normalized counts, or Repeat).  compose() returns the frame bytes, the content
(from a small executor of the sequences of its own) and a feature record: which of those choices the frame uses.

Nothing here reads the package under test: the decoder's own headers are not the specification.  Bit streams are built from the
decoder's side: the fields a decoder reads, in the order it reads them, are collected and then written backwards, and an FSE
state chain is walked from its last state to its first through the decoding table itself.
"""
import bisect

import numpy as np

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 128 * 1024

# ---- RFC 8878 section 3.1.1.3.2.1: codes, baselines, extra bits ------------------------------------------------------------
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = [i + 3 for i in range(32)] + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                         16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
# predefined distributions (section 3.1.1.3.2.2)
LL_PRE = ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_PRE = ([1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
           1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1], 6)
OF_PRE = ([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1], 5)
MAX_LOG = (9, 8, 9)                     # LL, OF, ML
PRE = (LL_PRE, OF_PRE, ML_PRE)
KIND = ("ll", "of", "ml")


def ll_code(v):
    if v < 16:
        return v
    for c in range(35, 15, -1):
        if v >= LL_BASE[c]:
            return c


def ml_code(v):
    assert 3 <= v <= 131074, v
    if v < 35:
        return v - 3
    for c in range(52, 31, -1):
        if v >= ML_BASE[c]:
            return c


def of_code(ov):
    assert ov >= 1
    return ov.bit_length() - 1


# ---- XXH64 (plain Python; the frame checksum is its low 32 bits) -------------------------------------------------------------
_P1, _P2, _P3, _P4, _P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261
_M = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, v):
    return (_rotl((acc + v * _P2) & _M, 31) * _P1) & _M


def xxh64(data, seed=0):
    n = len(data)
    p = 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M]
        w = np.frombuffer(data, dtype="<u8", count=(n // 32) * 4).tolist()
        for i in range(0, len(w), 4):
            v[0] = _round(v[0], w[i]); v[1] = _round(v[1], w[i + 1]); v[2] = _round(v[2], w[i + 2]); v[3] = _round(v[3], w[i + 3])
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for x in v:
            h = ((h ^ _round(0, x)) * _P1 + _P4) & _M
        p = (n // 32) * 32
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[p:p + 8], "little")), 27) * _P1 + _P4) & _M
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5 & _M), 11) * _P1) & _M
        p += 1
    h ^= h >> 33; h = (h * _P2) & _M; h ^= h >> 29; h = (h * _P3) & _M; h ^= h >> 32
    return h


# ---- bit streams ---------------------------------------------------------------------------------------------------------------
class FwdBits:
    """Little-endian forward bit stream (FSE table descriptions)."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, nb):
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0
        self.acc |= v << self.n
        self.n += nb

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def backward_stream(fields):
    """fields: (value, nbits) in the order a decoder reads them from the end of the stream.  Written last-read first, closed
    by the 1 bit that marks the start."""
    out = bytearray()
    acc, n = 0, 0
    for v, nb in reversed(fields):
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0, (v, nb)
        acc |= v << n
        n += nb
        while n >= 8:
            out.append(acc & 0xFF); acc >>= 8; n -= 8
    acc |= 1 << n
    n += 1
    while n > 0:
        out.append(acc & 0xFF); acc >>= 8; n -= 8
    return bytes(out)


# ---- FSE (section 4.1) ---------------------------------------------------------------------------------------------------------
def fse_decode_table(counts, log):
    """(symbol, nb, baseline) per state, built as section 4.1.1 builds it."""
    size = 1 << log
    assert sum(abs(c) for c in counts) == size, (sum(abs(c) for c in counts), size)
    sym = [None] * size
    high = size - 1
    for s, c in enumerate(counts):
        if c == -1:
            sym[high] = s
            high -= 1
    step = (size >> 1) + (size >> 3) + 3
    pos = 0
    for s, c in enumerate(counts):
        for _ in range(c if c > 0 else 0):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nxt = [1 if c == -1 else max(c, 0) for c in counts]
    table = []
    for x in range(size):
        s = sym[x]
        ns = nxt[s]; nxt[s] += 1
        nb = log - (ns.bit_length() - 1)
        table.append((s, nb, (ns << nb) - size))
    return table


class FseTable:
    """A decoding table and, per symbol, the state a decoder must be in to reach state Y next."""

    def __init__(self, counts=None, log=None, rle=None):
        self.rle = rle
        if rle is not None:
            self.log, self.table = 0, [(rle, 0, 0)]
        else:
            self.counts, self.log = list(counts), log
            self.table = fse_decode_table(counts, log)
        self.prev = {}
        for x, (s, nb, base) in enumerate(self.table):
            arr = self.prev.setdefault(s, [None] * len(self.table))
            for y in range(base, base + (1 << nb)):
                assert arr[y] is None
                arr[y] = x
        for s, arr in self.prev.items():
            assert None not in arr, "symbol %d: its states do not tile the table" % s

    def first_state(self, s, min_bits=0):
        for x, (t, nb, _) in enumerate(self.table):
            if t == s and nb >= min_bits:
                return x
        raise ValueError("no state for symbol %d" % s)

    def chain(self, syms, last_min_bits=0):
        """States x_0..x_{n-1} decoding syms, x_{i+1} reached from x_i; returns (states, transition fields)."""
        n = len(syms)
        xs = [0] * n
        xs[-1] = self.first_state(syms[-1], last_min_bits)
        for i in range(n - 2, -1, -1):
            xs[i] = self.prev[syms[i]][xs[i + 1]]
        bits = []
        for i in range(n - 1):
            _, nb, base = self.table[xs[i]]
            bits.append((xs[i + 1] - base, nb))
        return xs, bits


def normalize(hist, log, lt1=()):
    """Normalized counts summing to 2**log from a histogram {symbol: count}; symbols in lt1 get the "less than 1" -1."""
    size = 1 << log
    n = max(hist) + 1
    total = sum(hist.values())
    counts = [0] * n
    for s, c in hist.items():
        if c > 0:
            counts[s] = -1 if s in lt1 else max(1, c * size // total)
    used = sum(abs(c) for c in counts)
    assert used <= size + len(hist) * 2
    while used != size:
        big = max((c, s) for s, c in enumerate(counts))[1]
        if used > size:
            assert counts[big] > 1
            counts[big] -= 1; used -= 1
        else:
            counts[big] += 1; used += 1
    return counts


def fse_describe(counts, log, feat=None):
    """FSE table description (section 4.1.1): accuracy log, then the counts with their zero-run repeat flags."""
    bw = FwdBits()
    bw.put(log - 5, 4)
    remaining = (1 << log) + 1
    threshold = 1 << log
    nbits = log + 1
    s = 0
    n = len(counts)
    while remaining > 1:
        assert s < n, "counts end before the table is full"
        c = counts[s]
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        v = c + 1
        if v >= threshold:
            v += mx
        if v < mx:
            bw.put(v, nbits - 1)
        else:
            bw.put(v, nbits)
        if feat is not None:
            if c == -1:
                feat.add("fse:lt1")
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
        s += 1
        if c == 0:                                              # a run of zeros behind a zero: 2-bit repeat flags
            run = 0
            while s + run < n and counts[s + run] == 0:
                run += 1
            if feat is not None:
                feat.add("fse:zero_run" + ("_ext" if run >= 3 else ""))
            r = run
            while r >= 3:
                bw.put(3, 2); r -= 3
            bw.put(r, 2)
            s += run
    assert remaining == 1 and all(c == 0 for c in counts[s:])
    return bw.bytes()


# ---- Huffman (section 4.2) -----------------------------------------------------------------------------------------------------
class HufTree:
    def __init__(self, weights):
        """weights: one per symbol 0..last (last > 0 and non-zero); the last one is what the others leave."""
        self.weights = list(weights)
        assert len(self.weights) >= 2 and self.weights[-1] > 0
        expl = sum(1 << (w - 1) for w in self.weights[:-1] if w)
        assert expl > 0
        self.max_bits = expl.bit_length()
        left = (1 << self.max_bits) - expl
        assert left == 1 << (self.weights[-1] - 1), "the last weight is not the one the others leave"
        assert self.max_bits <= 11
        code_len = np.zeros(256, dtype=np.int64)
        code = np.zeros(256, dtype=np.int64)
        c = 0
        for w in range(1, self.max_bits + 1):
            for s, ws in enumerate(self.weights):
                if ws == w:
                    code[s] = c
                    code_len[s] = self.max_bits + 1 - w
                    c += 1
            c >>= 1
        self.code, self.len = code, code_len

    def describe(self, fse=False, log=6, feat=None):
        ws = self.weights[:-1]
        if not fse:
            assert len(ws) <= 128
            b = bytearray([127 + len(ws)])
            for i in range(0, len(ws), 2):
                b.append((ws[i] << 4) | (ws[i + 1] if i + 1 < len(ws) else 0))
            return bytes(b)
        hist = {}
        for w in ws:
            hist[w] = hist.get(w, 0) + 1
        counts = normalize(hist, log)
        t = FseTable(counts, log)
        n = len(ws)
        chains = [ws[0::2], ws[1::2]]
        # the chain that decodes the next-to-last weight must read past the end (that is how the decoder stops): a state of >= 1 bit
        xs0, b0 = t.chain(chains[0], last_min_bits=1 if (n - 2) % 2 == 0 else 0)
        xs1, b1 = t.chain(chains[1], last_min_bits=1 if (n - 2) % 2 == 1 else 0)
        fields = [(xs0[0], log), (xs1[0], log)]
        for j in range(n - 2):
            fields.append((b0 if j % 2 == 0 else b1)[j // 2])
        body = fse_describe(counts, log, feat) + backward_stream(fields)
        assert len(body) < 128
        return bytes([len(body)]) + body

    def stream(self, syms):
        s = np.frombuffer(bytes(syms), dtype=np.uint8)[::-1]
        assert (self.len[s] > 0).all(), "a literal without a code"
        ln, cd = self.len[s], self.code[s]
        start = np.concatenate(([0], np.cumsum(ln)[:-1])) if len(ln) else np.zeros(0, np.int64)
        total = int(ln.sum())
        bits = np.zeros(((total + 1 + 7) // 8) * 8, dtype=np.uint8)
        for b in range(self.max_bits):
            m = ln > b
            bits[start[m] + b] = (cd[m] >> b) & 1
        bits[total] = 1
        return np.packbits(bits, bitorder="little").tobytes()


# ---- the frame ---------------------------------------------------------------------------------------------------------------
def raw(data):
    return {"type": "raw", "data": bytes(data)}


def rle(byte, n):
    return {"type": "rle", "byte": byte, "n": n}


def comp(lits=b"", seqs=(), lit="raw", lit_fmt=None, tree=None, fse_tree=False, streams=None, nseq_form=None, modes=("pre",) * 3):
    """A Compressed block.  lit: "raw" | "rle" | "huf" | "treeless"; lit_fmt: the Size_Format (raw / RLE: 1, 2 or 3 bytes of header;
    Huffman: 10, 14 or 18 bits); modes: per LL / OF / ML "pre" | "rle" | ("fse", counts, log) | "rep"."""
    return {"type": "comp", "lits": bytes(lits), "seqs": list(seqs), "lit": lit, "lit_fmt": lit_fmt, "tree": tree,
            "fse_tree": fse_tree, "streams": streams, "nseq_form": nseq_form, "modes": tuple(modes)}


def skippable(data, nibble=0):
    return {"type": "skip", "data": bytes(data), "nibble": nibble}


def _lit_section(b, st, feat):
    lits, kind = b["lits"], b["lit"]
    n = len(lits)
    if kind in ("raw", "rle"):
        t = 0 if kind == "raw" else 1
        fmt = b["lit_fmt"] or (1 if n < 32 else 2 if n < 4096 else 3)
        feat.add("lit:%s:h%d" % (kind, fmt))
        if fmt == 1:
            assert n < 32
            feat.add("lit:%s:h1:%s" % (kind, "10" if n & 1 else "00"))
            hdr = bytes([t | (n << 3)])
        elif fmt == 2:
            assert n < 4096
            hdr = bytes([t | 4 | ((n & 15) << 4), n >> 4])
        else:
            assert n < (1 << 20)
            hdr = bytes([t | 12 | ((n & 15) << 4), (n >> 4) & 255, n >> 12])
        if kind == "rle":
            assert n > 0 and lits == lits[:1] * n
            return hdr + lits[:1]
        return hdr + lits
    tree = b["tree"] if kind == "huf" else st["huf"]
    assert tree is not None, "treeless literals without an earlier tree"
    streams = b["streams"] or (1 if n <= 1023 else 4)
    if kind == "huf":
        desc = tree.describe(fse=b["fse_tree"], feat=feat)
        st["huf"] = tree
        st["desc"] = (desc, b["streams"] or (1 if n <= 1023 else 4))
        feat.add("huf:tree:%s" % ("fse" if b["fse_tree"] else "direct"))
        feat.add("huf:maxbits:%d" % tree.max_bits)
        nsym = sum(1 for w in tree.weights if w)
        feat.add("huf:symbols:%s" % ("2" if nsym == 2 else "256" if nsym == 256 else "other"))
    else:
        desc = b""
        feat.add("lit:treeless")
        feat.add("lit:treeless_after:" + st["last_lit"])
    if streams == 1:
        body = tree.stream(lits)
    else:
        assert n >= 6
        per = (n + 3) // 4
        parts = [tree.stream(lits[i * per:(i + 1) * per]) for i in range(3)] + [tree.stream(lits[3 * per:])]
        assert all(len(p) < 65536 for p in parts[:3])
        body = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
    feat.add("huf:streams:%d" % streams)
    csize = len(desc) + len(body)
    fmt = b["lit_fmt"] or (10 if max(n, csize) < 1024 else 14 if max(n, csize) < 16384 else 18)
    assert max(n, csize) < (1 << fmt)
    sf = {10: 0 if streams == 1 else 1, 14: 2, 18: 3}[fmt]
    assert streams == 1 and sf == 0 or streams == 4 and sf > 0 or streams == 4 and fmt == 10
    feat.add("huf:size:%d" % fmt)
    t = 2 if kind == "huf" else 3
    v = t | (sf << 2) | (n << 4) | (csize << (4 + fmt))
    hdr = v.to_bytes((4 + 2 * fmt + 7) // 8, "little")
    return hdr + desc + body


def _seq_section(b, st, feat):
    seqs = b["seqs"]
    n = len(seqs)
    form = b["nseq_form"] or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    feat.add("nseq:%dbyte" % form)
    if n in (127, 128, 0x7EFF, 0x7F00):
        feat.add("nseq:edge:%d" % n)
    if form == 2 and n < 128:
        feat.add("nseq:2byte_small")
    if form == 1:
        assert n < 128
        out = bytearray([n])
    elif form == 2:
        assert 0 < n < 0x7F00
        out = bytearray([128 + (n >> 8), n & 255])
    else:
        assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
        out = bytearray([255, (n - 0x7F00) & 255, (n - 0x7F00) >> 8])
    if n == 0:
        return bytes(out)
    codes = [[ll_code(ll) for ll, ml, ov in seqs], [of_code(ov) for ll, ml, ov in seqs], [ml_code(ml) for ll, ml, ov in seqs]]
    for k in range(3):
        for c in codes[k]:
            feat.add("code:%s:%d" % (KIND[k], c))
    tabs, mb, desc = [], 0, bytearray()
    for k in range(3):
        m = b["modes"][k]
        if m == "pre":
            t = FseTable(*PRE[k]); mode = 0
        elif m == "rle":
            assert len(set(codes[k])) == 1
            t = FseTable(rle=codes[k][0]); mode = 1; desc.append(codes[k][0])
        elif m == "rep":
            t = st["fse"][k]; mode = 3
            assert t is not None, "Repeat mode with no table before it"
            feat.add("mode:%s:rep_of_%s" % (KIND[k], "rle" if t.rle is not None else "table"))
            if st["nseq0_since"][k]:
                feat.add("mode:rep_after_nseq0")
        else:
            _, counts, log = m
            assert 5 <= log <= MAX_LOG[k]
            t = FseTable(counts, log); mode = 2
            desc += fse_describe(counts, log, feat)
            feat.add("fse:log:%s:%d" % (KIND[k], log))
        feat.add("mode:%s:%s" % (KIND[k], ("pre", "rle", "fse", "rep")[mode]))
        st["fse"][k] = t
        st["nseq0_since"][k] = False
        tabs.append(t)
        mb |= mode << (6 - 2 * k)
    out.append(mb)
    out += desc
    chains = [tabs[k].chain(codes[k]) for k in range(3)]
    fields = [(chains[0][0][0], tabs[0].log), (chains[1][0][0], tabs[1].log), (chains[2][0][0], tabs[2].log)]
    for i, (ll, ml, ov) in enumerate(seqs):
        lc, oc, mc = codes[0][i], codes[1][i], codes[2][i]
        fields.append((ov - (1 << oc), oc))
        fields.append((ml - ML_BASE[mc], ML_BITS[mc]))
        fields.append((ll - LL_BASE[lc], LL_BITS[lc]))
        if i + 1 < n:
            fields.append(chains[0][1][i]); fields.append(chains[2][1][i]); fields.append(chains[1][1][i])
    out += backward_stream(fields)
    return bytes(out)


def _execute(b, st, out, feat, window):
    """Section 3.1.2.5: the sequences run against what the frame has produced so far."""
    lits, pos = b["lits"], 0
    rep = st["rep"]
    for ll, ml, ov in b["seqs"]:
        out += lits[pos:pos + ll]; pos += ll
        assert pos <= len(lits), "sequences use more literals than the block has"
        if ov > 3:
            off = ov - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            feat.add("rep:%s:ov%d" % ("ll0" if ll == 0 else "ll", ov))
            idx = ov - 1 if ll else ov                          # ll == 0 shifts the codes by one; 3 then means rep1 - 1
            if idx == 3:
                off = rep[0] - 1
                assert off > 0
                rep[:] = [off, rep[0], rep[1]]
            elif idx == 0:
                off = rep[0]
            elif idx == 1:
                off = rep[1]; rep[:] = [rep[1], rep[0], rep[2]]
            else:
                off = rep[2]; rep[:] = [rep[2], rep[0], rep[1]]
        assert 0 < off <= len(out) and off <= window, (off, len(out), window)
        srcs = st["srcs"]
        if srcs:                                                # a match that copies from an earlier Raw or RLE block
            k = bisect.bisect_right(srcs, (len(out) - off, 1 << 62, "")) - 1
            if k >= 0 and srcs[k][0] <= len(out) - off < srcs[k][1]:
                feat.add("match:into_%s_block" % srcs[k][2])
        if off == window:
            feat.add("match:window_back")
        if off < ml:
            feat.add("match:overlap")
            if off <= 16:
                feat.add("match:overlap_off:%d" % off)
        src = len(out) - off
        if off >= ml:
            out += out[src:src + ml]
        else:
            pat = bytes(out[src:])
            out += (pat * (ml // off + 1))[:ml]
        if ml >= 131072:
            feat.add("match:ml_max")
    out += lits[pos:]


def compose(blocks, fcs=None, single_segment=False, window_log=17, window_mantissa=0, checksum=False, fcs_value=None):
    """One frame.  fcs: width of the Frame_Content_Size field (0, 1, 2, 4 or 8; 1 only with single_segment); None: the smallest
    that holds the size (or none for frames with a Window_Descriptor).  Returns (frame, content, features)."""
    feat = set()
    st = {"huf": None, "fse": [None, None, None], "rep": [1, 4, 8], "last_lit": "none", "nseq0_since": [False] * 3,
          "descs": [], "srcs": []}
    if single_segment:
        window = None
    else:
        window = (1 << window_log) + ((1 << window_log) >> 3) * window_mantissa
    content = bytearray()
    body = bytearray()
    for i, b in enumerate(blocks):
        last = i + 1 == len(blocks)
        start = len(content)
        win = window if window is not None else (1 << 62)
        bmax = min(BLOCK_MAX, win)
        if b["type"] == "raw":
            payload, size = b["data"], len(b["data"])
            content += payload
            st["srcs"].append((start, len(content), "raw"))
            feat.add("block:raw" + (":empty_last" if size == 0 and last else ""))
            st["last_lit"] = "raw_block"
        elif b["type"] == "rle":
            payload, size = bytes([b["byte"]]), b["n"]
            content += payload * size
            st["srcs"].append((start, len(content), "rle"))
            feat.add("block:rle")
            st["last_lit"] = "rle_block"
        else:
            memo = b.get("_memo")                               # a block without sequences reused in many frames: its bytes once
            if memo and not b["seqs"] and memo[0] is st["huf"]:
                payload, f, desc = memo[1], memo[2], memo[3]
                feat |= f
                if b["lit"] == "huf":
                    st["huf"] = b["tree"]
            else:
                prev, f = st["huf"], set()
                st["desc"] = None
                payload = _lit_section(b, st, f)
                desc = st["desc"]
                payload += _seq_section(b, st, f)
                feat |= f
                if not b["seqs"]:
                    b["_memo"] = (prev, payload, f, desc)
            if desc is not None:                                # a tree description that repeats an earlier one byte for byte
                ds = st["descs"]
                if ds and ds[-1][0] == desc[0]:
                    feat.add("huf:tree_repeat:prev" + (":other_streams" if ds[-1][1] != desc[1] else ""))
                if any(d == desc[0] for d, _ in ds[:-1]) and (not ds or ds[-1][0] != desc[0]):
                    feat.add("huf:tree_repeat:nonadjacent")
                ds.append(desc)
            if not b["seqs"]:
                for k in range(3):
                    st["nseq0_since"][k] = st["fse"][k] is not None
                if not b["lits"]:
                    feat.add("block:comp:empty")
            _execute(b, st, content, feat, win)
            size = len(payload)
            feat.add("block:comp")
            st["last_lit"] = {"raw": "raw_lits", "rle": "rle_lits", "huf": "huf", "treeless": "huf"}[b["lit"]]
        assert size <= bmax and len(content) - start <= bmax, (size, len(content) - start, bmax)
        if bmax < BLOCK_MAX and len(content) - start == bmax:
            feat.add("block:window_capped")
        h = int(last) | ({"raw": 0, "rle": 1, "comp": 2}[b["type"]] << 1) | (size << 3)
        body += h.to_bytes(3, "little") + payload
    n = len(content) if fcs_value is None else fcs_value
    if single_segment:
        assert window is None
    if fcs is None:
        fcs = 0 if not single_segment else 1 if n < 256 else 2 if n < 65792 else 4 if n < (1 << 32) else 8
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs]
    assert fcs != 1 or single_segment
    assert not (fcs == 0 and single_segment)
    fhd = (flag << 6) | (int(single_segment) << 5) | (int(checksum) << 2)
    hdr = bytearray([fhd])
    if not single_segment:
        assert 10 <= window_log <= 41 and 0 <= window_mantissa < 8
        hdr.append(((window_log - 10) << 3) | window_mantissa)
        feat.add("hdr:window" + (":mantissa" if window_mantissa else ""))
    else:
        feat.add("hdr:single_segment")
    if fcs == 1:
        assert n < 256
        hdr.append(n)
    elif fcs == 2:
        assert 256 <= n < 65792
        hdr += (n - 256).to_bytes(2, "little")
    elif fcs in (4, 8):
        hdr += n.to_bytes(fcs, "little")
    feat.add("hdr:fcs%d" % fcs)
    if fcs and n in (255, 256, 65791, 65792):
        feat.add("fcs:edge:%d" % n)
    frame = MAGIC + bytes(hdr) + bytes(body)
    if checksum:
        frame += (xxh64(bytes(content)) & 0xFFFFFFFF).to_bytes(4, "little")
        feat.add("hdr:checksum")
    return frame, bytes(content), feat


def concat(parts):
    """Frames and skippable frames one after the other: parts are compose() results or skippable() dicts."""
    data, content, feat = bytearray(), bytearray(), set()
    for p in parts:
        if isinstance(p, dict):
            data += (0x184D2A50 + p["nibble"]).to_bytes(4, "little") + len(p["data"]).to_bytes(4, "little") + p["data"]
            feat.add("frame:skippable")
        else:
            data += p[0]; content += p[1]; feat |= p[2]
    feat.add("frame:concat")
    return bytes(data), bytes(content), feat


def split_frames(data):
    """The frames of a concatenation (skippable ones dropped), by walking the block headers."""
    out, p = [], 0
    while p < len(data):
        m = int.from_bytes(data[p:p + 4], "little")
        if m & 0xFFFFFFF0 == 0x184D2A50:
            p += 8 + int.from_bytes(data[p + 4:p + 8], "little")
            continue
        assert data[p:p + 4] == MAGIC
        fhd = data[p + 4]
        ss, flag, ck = (fhd >> 5) & 1, fhd >> 6, (fhd >> 2) & 1
        q = p + 5 + (0 if ss else 1) + (fhd & 3 and (1, 2, 4)[(fhd & 3) - 1] or 0) + ((1 if ss else 0), 2, 4, 8)[flag]
        while True:
            h = int.from_bytes(data[q:q + 3], "little")
            q += 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)
            if h & 1:
                break
        q += 4 * ck
        out.append(data[p:q])
        p = q
    return out
