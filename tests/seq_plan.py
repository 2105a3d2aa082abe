"""The plan and the model of the sequence-table tests (test_seq_plan_cpu.py holds both to their claims and drives the host build of the
writers, test_gpu_seq_plan.py runs the plan on the kernels): what the encoder's Sequences_Section of one block has to look like, table by
table, and byte streams whose planted copies steer a block's three code histograms (Literals_Length, Offset, Match_Length) onto the
seams of that decision.  Pure numpy; nothing here comes from the code under test -- the constants are RFC 8878's (by way of
tests/zstd_compose.py, which is written from the RFC alone) and the rules are the ones naf_amd/csrc/zstd_enc_core.h documents in prose.

The model, in exact integers, of the per-block planner of the cross-block stage (zenc_seq_table, levels >= 2 and --long):
  * one code occurs: RLE_Mode;
  * Predefined_Mode is usable when every code that occurs has a probability in the predefined distribution;
  * FSE_Compressed_Mode at Accuracy_Log hibit(nseq) + 1, at least 5, at most 9 / 8 / 9 (LL / OF / ML), raised until 2^log holds the codes that
    occur; probabilities floor(count * 2^log / nseq), at least 1; the sum repaired on the FIRST most frequent code (topped up, or taken
    down while that leaves it a probability above the excess; else one from every code above 1 in turn);
  * cost in 1/256 bit: count * (log * 256 - log2_256(probability)), log2_256 linear between powers of two, plus 8 * 256 per byte of the
    table description (RFC 8878 4.1.1); FSE only where it is strictly cheaper.
The in-block stage (level 1, zenc_write_sequences) has no planner: three predefined tables, a modes byte of 0.

The checks (each raises lz_plan.Reject with its own reason) apply to every Compressed block with sequences: check_planner (the listed
mode, log, probabilities and description bytes are the model's), check_form (what holds whatever the model says), check_size (the
section's bytes are header + modes + descriptions + ceil((bits + 1) / 8), bits counted from this file's own decoding tables walked back
from the listed final states), check_parity (the section is what the host build of the same writer makes of the listed sequences),
check_economy (no block larger than the same block of the frame made without the match finder).

A cell is a property of ONE block's histogram for one table; it is reached when a block of a frame shows it (`block_cells`), not when
a stream asked for it: the match finders do not promise every plant.  EXEMPT lists what no frame of the kernels can show, and why.
"""
from collections import namedtuple

import numpy as np

import lz_plan as P
import zstd_compose as Z
from lz_plan import SEED, SEEDS, Reject, split_even, Stream, LL_FIRST, ML_FIRST     # shared, not copied (re-exported for the tests)

KIND = ("LL", "OF", "ML")
ALPHABET = (36, 32, 53)
MAX_LOG = Z.MAX_LOG                     # 9, 8, 9
PRE = tuple((tuple(c) + (0,) * (64 - len(c)), log, len(c)) for c, log in Z.PRE)      # LL, OF, ML: probabilities (64), log, codes
LL_BASE, ML_BASE = np.array(Z.LL_BASE, dtype=np.int64), np.array(Z.ML_BASE, dtype=np.int64)
LL_BITS, ML_BITS = np.array(Z.LL_BITS, dtype=np.int64), np.array(Z.ML_BITS, dtype=np.int64)

COUNTS = (1, 2, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512)
THOUSANDS = 1000
LARGEST = 40          # Match_Length codes in one block: lengths of 5 to 65535 have 50 codes, the 49 below 32771 fit a block of 2^16 bytes
#                       together; the finders do not promise every plant, so the cell asks for 40 of them
OF_TOP = 19           # the largest Offset code under the direct route's window of 2^20: distances of 2^19 - 3 and more

EXEMPT = {
    ("range", "LL35"): "literal lengths are kept in 16 bits: 65536 and more never leave the parsers",
    ("range", "ML52"): "match lengths are kept in 16 bits (65539 and more are cut at 65535)",
    ("range", "OF%d+" % (OF_TOP + 1)): "Offset codes above the window's: no distance of 2^20 - 3 or more under the largest window a test stream has",
    ("count", "three_byte_form"): "0x7F00 sequences and more: a block's sequence slot holds a quarter of its bytes, 16384 at most",
    ("outcome", "predefined_impossible"): "a table Predefined_Mode cannot code needs Offset code 29 or more",
    ("norm", "round_robin"): "the second repair of fse_normalize: no histogram under the planner's log rule reaches it (test_seq_plan_cpu.py repeats the search)",
}


# ---- values to codes (RFC 8878 3.1.1.3.2.1.1) -----------------------------------------------------------------------------------------
def codes_of(ll, ml, ofv):
    """(LL codes, OF codes, ML codes) of arrays of literal lengths, match lengths and Offset_Values."""
    ll, ml, ofv = (np.asarray(a, dtype=np.int64) for a in (ll, ml, ofv))
    assert (ml >= 3).all() and (ofv >= 1).all() and (ll >= 0).all()
    return (np.searchsorted(LL_BASE, ll, "right") - 1, np.frexp(ofv.astype(np.float64))[1].astype(np.int64) - 1,
            np.searchsorted(ML_BASE, ml, "right") - 1)


def extra_bits(codes):
    """Bits the three fields of the sequences carry beside their codes."""
    return int(LL_BITS[codes[0]].sum() + codes[1].sum() + ML_BITS[codes[2]].sum())


def hists_of(codes):
    return [np.bincount(c, minlength=64)[:64].astype(np.int64) for c in codes]


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------
def hibit(v):
    return int(v).bit_length() - 1


def log2_256(v):
    """256 * log2(v), v >= 1, linear between powers of two."""
    h = hibit(v)
    return h * 256 + ((v >> (h - 8)) if h >= 8 else (v << (8 - h))) - 256


def cost_256(hist, norm, log):
    """Cost in 1/256 bit of coding `hist` with probabilities norm / 2^log (-1 counts as 1); None when a code that occurs has none."""
    c = 0
    for s in np.nonzero(hist)[0]:
        if norm[s] == 0:
            return None
        c += int(hist[s]) * (log * 256 - log2_256(1 if norm[s] < 0 else int(norm[s])))
    return c


def accuracy_log(k, nseq, present):
    log = min(max(hibit(nseq) + 1, 5), MAX_LOG[k])
    while (1 << log) < present:
        log += 1
    return log if log <= MAX_LOG[k] else None


def normalise(hist, nseq, log):
    """(probabilities (64), repair) or (None, None); repair: "exact", "topup", "takedown" or "round_robin"."""
    size = 1 << log
    occ = [int(s) for s in np.nonzero(hist)[0]]
    if len(occ) > size or len(occ) < 2:
        return None, None
    norm = [0] * 64
    for s in occ:
        norm[s] = max(1, int(hist[s]) * size // nseq)
    big = occ[int(np.argmax([hist[s] for s in occ]))]                 # the first of the most frequent
    total, repair = sum(norm), "exact"
    while total != size:
        if total < size:
            norm[big] += size - total; total = size
            repair = "topup" if repair == "exact" else repair
        elif norm[big] > total - size:
            norm[big] -= total - size; total = size
            repair = "takedown" if repair == "exact" else repair
        else:
            repair, any_ = "round_robin", False
            for s in occ:
                if total > size and norm[s] > 1:
                    norm[s] -= 1; total -= 1; any_ = True
            if not any_:
                return None, None
    return norm, repair


def describe(norm, log):
    """The table description of RFC 8878 4.1.1 for probabilities norm[0 .. last code that occurs]."""
    acc, n = log - 5, 4
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    last = max(s for s in range(64) if norm[s] != 0)
    s = 0
    while remaining > 1 and s <= last:
        c = norm[s]; s += 1
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        v = c + 1
        if v >= threshold:
            v += mx
        w = nbits - (1 if v < mx else 0)
        acc |= v << n; n += w
        if c == 0:
            run = 0
            while s <= last and norm[s] == 0:
                s += 1; run += 1
            while run >= 3:
                acc |= 3 << n; n += 2; run -= 3
            acc |= run << n; n += 2
        while remaining < threshold and threshold > 1:
            nbits -= 1; threshold >>= 1
    assert remaining == 1, "the probabilities do not fill the table"
    return acc.to_bytes((n + 7) // 8, "little")


TablePlan = namedtuple("TablePlan", "mode log norm desc rle present cost_pre cost_fse fse_log fse_norm repair tie")
# mode: 0 Predefined, 1 RLE, 2 FSE_Compressed, None: no table can be made (the writer returns 0, the block stays literal-only)
# cost_pre / cost_fse: 1/256 bit (None: not usable); fse_*: what FSE_Compressed_Mode would be, chosen or not


def plan_table(k, hist, nseq, stage="lzx"):
    occ = np.nonzero(hist)[0]
    present = len(occ)
    assert int(hist.sum()) == nseq and present >= 1
    pre_norm, pre_log, pre_n = PRE[k]
    if stage == "lz":                                                   # zenc_write_sequences: predefined, whatever occurs
        return TablePlan(0, pre_log, pre_norm, b"", 0, present, cost_256(hist, pre_norm, pre_log), None, None, None, None, False)
    if present == 1:
        return TablePlan(1, 0, (0,) * 64, bytes([int(occ[0])]), int(occ[0]), 1, None, None, None, None, None, False)
    cost_pre = cost_256(hist, pre_norm, pre_log) if int(occ[-1]) < pre_n else None
    log = accuracy_log(k, nseq, present)
    norm, repair = normalise(hist, nseq, log) if log is not None else (None, None)
    cost_fse = desc = None
    if norm is not None:
        desc = describe(norm, log)
        cost_fse = cost_256(hist, norm, log) + len(desc) * 8 * 256
    tie = bool((hist == hist.max()).sum() > 1)
    if cost_fse is not None and (cost_pre is None or cost_fse < cost_pre):
        return TablePlan(2, log, tuple(norm), desc, 0, present, cost_pre, cost_fse, log, tuple(norm), repair, tie)
    if cost_pre is None:
        return TablePlan(None, None, None, None, 0, present, None, None, None, None, None, tie)
    return TablePlan(0, pre_log, pre_norm, b"", 0, present, cost_pre, cost_fse, log, tuple(norm) if norm else None, repair, tie)


# ---- the decoding table (RFC 8878 4.1.1), to count the bits of the state chain ------------------------------------------------------------
_TABLES = {}


def decode_table(norm, log):
    """(symbol, bits, baseline per state; per symbol the state that leads to each next state)."""
    key = (tuple(int(v) for v in norm), log)
    if key not in _TABLES:
        size = 1 << log
        if sum(abs(v) for v in key[0]) != size:
            raise Reject("form: sum", "probabilities that sum to %d under an Accuracy_Log of %d" % (sum(abs(v) for v in key[0]), log))
        sym, high = [0] * size, size - 1
        for s, c in enumerate(key[0]):
            if c == -1:
                sym[high] = s; high -= 1
        step, pos = (size >> 1) + (size >> 3) + 3, 0
        for s, c in enumerate(key[0]):
            for _ in range(max(c, 0)):
                sym[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        nxt = [1 if c == -1 else c for c in key[0]]
        nb, base, prev = [0] * size, [0] * size, {}
        for x in range(size):
            s = sym[x]
            v = nxt[s]; nxt[s] += 1
            nb[x] = log - hibit(v); base[x] = (v << nb[x]) - size
            prev.setdefault(s, [None] * size)[base[x]:base[x] + (1 << nb[x])] = [x] * (1 << nb[x])
        _TABLES[key] = (sym, nb, base, prev)
    return _TABLES[key]


def chain_bits(norm, log, codes, final_state):
    """Bits the decoder reads for one table's states: the initial state and every update, walked back from the state it holds last."""
    if log == 0:
        return 0
    sym, nb, base, prev = decode_table(norm, log)
    x = int(final_state)
    if x >= len(sym) or sym[x] != codes[-1]:
        raise Reject("size", "the final state %d does not decode the last code %d" % (x, codes[-1]))
    bits = log
    for c in codes[-2::-1].tolist():
        if c not in prev:
            raise Reject("size", "code %d has no state in its table" % c)
        x = prev[c][x]
        bits += nb[x]
    return bits


# ---- a block as the oracle lists it ----------------------------------------------------------------------------------------------------------
class Block:
    def __init__(self, frame, tabs, seqs, b, lo, hi):
        self.b = b
        self.ll, self.ml, self.ofv = seqs.ll[lo:hi], seqs.ml[lo:hi], seqs.offset_value[lo:hi]
        self.nseq = int(tabs.n_sequences[b])
        self.codes = codes_of(self.ll, self.ml, self.ofv)
        self.hist = hists_of(self.codes)
        self.hdr, self.off, self.size, self.stream = (int(v[b]) for v in (tabs.nseq_header_bytes, tabs.section_offset, tabs.section_bytes, tabs.bitstream_bytes))
        self.mode, self.log, self.rle, self.desc_bytes = (v[b].tolist() for v in (tabs.mode, tabs.accuracy_log, tabs.rle_symbol, tabs.desc_bytes))
        self.norm, self.final = tabs.norm[b].tolist(), tabs.final_state[b].tolist()
        self.consumed, self.marker = int(tabs.bits_consumed[b]), int(tabs.marker_bit[b])
        self.section = frame[self.off:self.off + self.size]

    def desc(self, k):
        at = self.hdr + 1 + sum(self.desc_bytes[:k])
        return self.section[at:at + self.desc_bytes[k]]


def blocks_of(oracle, frame):
    """The Compressed blocks with sequences of a frame."""
    try:
        tabs, seqs = oracle.zstd_seq_tables(frame, with_sequences=True)
    except ValueError as e:
        raise Reject("decode", str(e))
    edges = np.searchsorted(seqs.block, np.arange(len(tabs) + 1), "left")
    out = []
    for b in np.nonzero((tabs.block_type == 2) & (tabs.n_sequences > 0))[0].tolist():
        if edges[b + 1] - edges[b] != tabs.n_sequences[b]:
            raise Reject("decode", "block %d: %d sequences listed for a count of %d" % (b, edges[b + 1] - edges[b], tabs.n_sequences[b]))
        out.append(Block(frame, tabs, seqs, b, int(edges[b]), int(edges[b + 1])))
    return out


# ---- cells --------------------------------------------------------------------------------------------------------------------------------------
def table_cells(k, hist, nseq, plan):
    """The cells one table of one block of the cross-block stage shows."""
    out = []
    cnt = np.sort(hist[hist > 0])
    n = len(cnt)
    if n == 1:
        out.append(("codes", "1"))
    elif n == 2:
        out.append(("codes", "2_equal" if cnt[0] == cnt[1] else "2_skewed"))
    elif n <= 8:
        out.append(("codes", "3_to_8"))
    elif n > 16:
        out.append(("codes", "over_16"))
    if k == 2 and n >= LARGEST:
        out.append(("codes", "largest"))
    if plan.mode == 2:
        out.append(("norm", plan.repair))
        if plan.tie and plan.repair != "exact":
            out.append(("norm", "tie_first_takes_it"))
        out.append(("outcome", "fse"))
    elif plan.mode == 1:
        out.append(("outcome", "rle"))
    elif plan.mode == 0 and n >= 2:
        out.append(("outcome", "predefined_kept"))
    elif plan.mode is None:
        out.append(("outcome", "predefined_impossible"))
    return out


def block_cells(blk, stage, plans):
    """Every cell a block shows: (group, name) -> table index it was seen on (None: the block as a whole)."""
    out = {}
    if stage == "lzx":
        for k in range(3):
            for c in table_cells(k, blk.hist[k], blk.nseq, plans[k]):
                out.setdefault(c, k)
        if blk.nseq in COUNTS:
            out[("count", "n%d" % blk.nseq)] = None
        if blk.nseq >= THOUSANDS:
            out[("count", "thousands")] = None
        if all(p.mode == 1 for p in plans):
            out[("outcome", "all_three_rle")] = None
    if blk.nseq >= 0x7F00:
        out[("count", "three_byte_form")] = None
    for c in np.nonzero(blk.hist[0])[0].tolist():
        if c == 0 or c >= 16:
            out[("range", "LL%d" % c)] = 0
    for c in np.nonzero(blk.hist[2])[0].tolist():
        if c >= 31:
            out[("range", "ML%d" % c)] = 2
    for c in np.nonzero(blk.hist[1])[0].tolist():
        if c >= 2:
            out[("range", "OF%d" % c if c <= OF_TOP else "OF%d+" % (OF_TOP + 1))] = 1
    for c in (0, 1):
        m = blk.codes[1] == c
        if (m & (blk.ll == 0)).any():
            out[("range", "OF%d_no_literals" % c)] = 1
        if (m & (blk.ll > 0)).any():
            out[("range", "OF%d_literals" % c)] = 1
    return out


def all_cells():
    """Every cell of the issue, exempt ones included."""
    cells = [("codes", v) for v in ("1", "2_equal", "2_skewed", "3_to_8", "over_16", "largest")]
    cells += [("count", "n%d" % v) for v in COUNTS] + [("count", "thousands"), ("count", "three_byte_form")]
    cells += [("norm", v) for v in ("exact", "topup", "takedown", "tie_first_takes_it", "round_robin")]
    cells += [("outcome", v) for v in ("predefined_kept", "fse", "rle", "all_three_rle", "predefined_impossible")]
    cells += [("range", "LL%d" % c) for c in [0] + list(range(16, 36))] + [("range", "ML%d" % c) for c in range(31, 53)]
    cells += [("range", "OF%d_%s" % (c, z)) for c in (0, 1) for z in ("no_literals", "literals")]
    cells += [("range", "OF%d" % c) for c in range(2, OF_TOP + 1)] + [("range", "OF%d+" % (OF_TOP + 1))]
    assert all(k in cells for k in EXEMPT)
    return cells


# ---- the checks -------------------------------------------------------------------------------------------------------------------------------------
def _cells_text(k, blk, plan):
    return ", ".join("%s %s" % c for c in table_cells(k, blk.hist[k], blk.nseq, plan)) or "-"


def check_planner(blk, stage, plans=None):
    """1: mode, Accuracy_Log, probabilities and description bytes of every table are the model's.  Returns the model's three plans."""
    plans = plans or [plan_table(k, blk.hist[k], blk.nseq, stage) for k in range(3)]
    for k, p in enumerate(plans):
        where = "block %d, %s of %d sequences (cells: %s)" % (blk.b, KIND[k], blk.nseq, _cells_text(k, blk, p))
        if p.mode is None:
            raise Reject("planner: no table", "%s: a table for a histogram no mode can code" % where)
        if blk.mode[k] != p.mode:
            raise Reject("planner: mode", "%s: mode %d, the model's %d (cost predefined %s, FSE %s)" % (where, blk.mode[k], p.mode, p.cost_pre, p.cost_fse))
        if p.mode == 1 and blk.rle[k] != p.rle:
            raise Reject("planner: rle symbol", "%s: RLE symbol %d, the model's %d" % (where, blk.rle[k], p.rle))
        if p.mode != 1 and blk.log[k] != p.log:
            raise Reject("planner: accuracy log", "%s: Accuracy_Log %d, the model's %d" % (where, blk.log[k], p.log))
        if p.mode != 1 and tuple(blk.norm[k]) != tuple(p.norm):
            s = next(i for i in range(64) if blk.norm[k][i] != p.norm[i])
            raise Reject("planner: probabilities", "%s: probability %d of code %d, the model's %d" % (where, blk.norm[k][s], s, p.norm[s]))
        if blk.desc(k) != p.desc:
            raise Reject("planner: description", "%s: description %s, the model's %s" % (where, blk.desc(k).hex(), p.desc.hex()))
    return plans


def check_form(blk):
    """2: what holds of a section whatever the model says."""
    b = blk.b
    for k in range(3):
        occ = np.nonzero(blk.hist[k])[0]
        if blk.mode[k] == 3:
            raise Reject("form: repeat mode", "block %d, %s: Repeat_Mode in a block coded without knowledge of the one in front" % (b, KIND[k]))
        if blk.mode[k] == 1:
            if len(occ) != 1 or blk.rle[k] != occ[0]:
                raise Reject("form: rle symbol", "block %d, %s: RLE symbol %d for the codes %s" % (b, KIND[k], blk.rle[k], occ.tolist()))
            continue
        if blk.mode[k] == 2 and not 5 <= blk.log[k] <= MAX_LOG[k]:
            raise Reject("form: log limits", "block %d, %s: Accuracy_Log %d" % (b, KIND[k], blk.log[k]))
        if sum(abs(v) for v in blk.norm[k]) != 1 << blk.log[k]:
            raise Reject("form: sum", "block %d, %s: probabilities sum to %d under an Accuracy_Log of %d" % (b, KIND[k], sum(abs(v) for v in blk.norm[k]), blk.log[k]))
        bare = [int(s) for s in occ if blk.norm[k][s] == 0]
        if bare:
            raise Reject("form: no probability", "block %d, %s: codes %s occur without a probability" % (b, KIND[k], bare))
    if blk.hdr != (1 if blk.nseq < 128 else 2 if blk.nseq < 0x7F00 else 3):
        raise Reject("form: count form", "block %d: Number_of_Sequences %d in %d bytes" % (b, blk.nseq, blk.hdr))
    if blk.hdr + 1 + sum(blk.desc_bytes) + blk.stream != blk.size:
        raise Reject("form: gap", "block %d: %d bytes between the parts of a section of %d" % (b, blk.size - blk.hdr - 1 - sum(blk.desc_bytes) - blk.stream, blk.size))
    if blk.consumed != blk.marker:
        raise Reject("form: unread bits", "block %d: the decoder read %d of the bitstream's %d bits: bytes in front of it that belong to nothing" % (b, blk.consumed, blk.marker))
    if blk.section[-1] == 0:
        raise Reject("form: zero end", "block %d: the section's last byte is zero" % b)


def model_bits(blk):
    """Bits of the block's bitstream without its marker, per table (states) and for the extra bits, from the listed tables."""
    per = [chain_bits(blk.norm[k], blk.log[k], blk.codes[k], blk.final[k]) for k in range(3)]
    return per, extra_bits(blk.codes)


def check_size(blk):
    """3: the section has the bytes its parts need and none beside."""
    per, extra = model_bits(blk)
    bits = sum(per) + extra
    want = blk.hdr + 1 + sum(blk.desc_bytes) + (bits + 1 + 7) // 8
    if blk.size != want:
        raise Reject("size", "block %d: a section of %d bytes, %d by its parts (%d bits)" % (blk.b, blk.size, want, bits))
    return per, extra


def host_section(emul, blk, stage):
    """What the host build of the stage's writer makes of the block's sequences."""
    import ctypes
    n = blk.nseq
    ll, ml = blk.ll.astype(np.uint16), blk.ml.astype(np.uint16)
    if (ll != blk.ll).any() or (ml != blk.ml).any():
        raise Reject("parity", "block %d: a length beyond 16 bits" % blk.b)
    cap = 64 * n + 1024
    out = ctypes.create_string_buffer(cap)
    if stage == "lz":
        if (blk.ofv <= 3).any():
            raise Reject("parity", "block %d: a repeat code from the stage that codes every offset as a new one" % blk.b)
        of = (blk.ofv - 3).astype(np.uint16)
        if (of != blk.ofv - 3).any():
            raise Reject("parity", "block %d: a distance beyond 16 bits" % blk.b)
        got = emul.emul_write_sequences(ll.tobytes(), ml.tobytes(), of.tobytes(), n, out, cap)
    else:
        got = emul.emul_write_sequences_x(ll.tobytes(), ml.tobytes(), blk.ofv.astype(np.uint32).tobytes(), n, out, cap)
    return out.raw[:got]


def check_parity(emul, blk, stage):
    """4: byte for byte the section of the host build; the in-block stage's modes byte is 0."""
    if stage == "lz" and blk.section[blk.hdr] != 0:
        raise Reject("parity", "block %d: modes byte %#x from the stage that writes predefined tables only" % (blk.b, blk.section[blk.hdr]))
    want = host_section(emul, blk, stage)
    if want != blk.section:
        k = next((i for i in range(min(len(want), len(blk.section))) if want[i] != blk.section[i]), min(len(want), len(blk.section)))
        raise Reject("parity", "block %d: %d bytes, the host build's %d; first difference at byte %d" % (blk.b, len(blk.section), len(want), k))


def check_economy(lits, twin):
    """5: no block larger than the same block of the frame made without the match finder (both listed by oracle.zstd_literals)."""
    if len(lits) != len(twin) or not np.array_equal(lits.decoded_size, twin.decoded_size):
        raise Reject("plan out of date", "the twin's blocks are not the frame's: %d and %d" % (len(twin), len(lits)))
    over = np.nonzero(lits.frame_size > twin.frame_size)[0]
    if len(over):
        b = int(over[0])
        raise Reject("larger block", "block %d: %d bytes with its sequences, %d without (%d sequences)" % (b, lits.frame_size[b], twin.frame_size[b], lits.n_sequences[b]))


def load_emul(so):
    import ctypes
    L = ctypes.CDLL(so)
    for f in (L.emul_write_sequences_x, L.emul_write_sequences):
        f.restype = ctypes.c_uint32
        f.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    L.emul_zstd_compress_lzx.restype = ctypes.c_longlong
    L.emul_zstd_compress_lzx.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    L.emul_zstd_compress_lz.restype = ctypes.c_longlong
    L.emul_zstd_compress_lz.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
    return L


def check_frame(oracle, emul, frame, stage, tally=None, where=""):
    """Checks 1 to 4 on every block with sequences; returns the reasons it failed for (texts)."""
    bad = []
    try:
        blocks = blocks_of(oracle, frame)
    except Reject as e:
        return [str(e)]
    for blk in blocks:
        plans = [plan_table(k, blk.hist[k], blk.nseq, stage) for k in range(3)]
        got = {}
        for name, chk in (("planner", lambda: check_planner(blk, stage, plans)), ("form", lambda: check_form(blk)), ("size", lambda: check_size(blk)),
                          ("parity", lambda: check_parity(emul, blk, stage))):
            try:
                got[name] = chk()
            except Reject as e:
                bad.append(str(e))
        bits = got.get("size")                                        # (per table, extra): what the table prints beside the estimates
        if tally is not None:
            tally.add(blk, stage, plans, bits, where)
    return bad


# ---- the coverage table -----------------------------------------------------------------------------------------------------------------------------
class Tally:
    """cell -> [blocks that showed it, where first, real bits, the planner's estimate, the cheapest other mode's] (bits of the table the
    cell was seen on: states and description; of all three for a cell of the block as a whole)."""

    def __init__(self):
        self.cell = {c: [0, "", 0, 0.0, 0.0, 0] for c in all_cells()}
        self.blocks = {"lz": 0, "lzx": 0}
        self.modes = np.zeros((3, 4), dtype=np.int64)
        self.most_codes = [0, 0, 0]
        self.searched = None                                          # (histograms drawn, how many reached the round-robin repair)

    def add(self, blk, stage, plans, bits=None, where=""):
        self.blocks[stage] += 1
        if stage == "lzx":
            for k in range(3):
                self.modes[k][blk.mode[k]] += 1
                self.most_codes[k] = max(self.most_codes[k], plans[k].present)
        for c, k in block_cells(blk, stage, plans).items():
            a = self.cell[c]
            a[0] += 1
            a[1] = a[1] or "%s block %d" % (where, blk.b)
            if bits is not None and stage == "lzx":
                for t in (range(3) if k is None else (k,)):
                    p = plans[t]
                    if p.mode is None:
                        continue
                    est = {0: p.cost_pre, 1: 8 * 256, 2: p.cost_fse}[p.mode]
                    other = {0: p.cost_fse, 1: None, 2: p.cost_pre}[p.mode]
                    a[2] += bits[0][t] + 8 * len(p.desc); a[3] += est / 256.0
                    if other is not None:
                        a[4] += other / 256.0; a[5] += 1

    def empty_cells(self):
        return sorted(c for c, a in self.cell.items() if a[0] == 0 and c not in EXEMPT)

    def table(self, title):
        rows = ["%s (seeds %s): blocks that showed each cell; bits of the table as written / as the planner estimated / by the cheapest other mode"
                % (title, ", ".join(map(str, SEEDS)))]
        for grp in ("codes", "count", "norm", "outcome", "range"):
            cells = []
            for c, a in self.cell.items():
                if c[0] != grp:
                    continue
                t = "%s %d" % (c[1], a[0])
                if c in EXEMPT:
                    t += " (exempt: %s)" % EXEMPT[c]
                elif a[0] and grp != "range" and a[2]:
                    t += " [%d / %.0f / %s]" % (a[2], a[3], "%.0f" % a[4] if a[5] else "-")
                if a[0] and grp != "range":
                    t += " @%s" % a[1]
                cells.append(t)
            rows.append("  %-8s %s" % (grp, "; ".join(cells)))
        rows.append("  blocks with sequences: in-block stage %d, cross-block stage %d; its table modes [predefined, rle, fse, repeat]: LL %s OF %s ML %s; most codes in one table: LL %d OF %d ML %d"
                    % (self.blocks["lz"], self.blocks["lzx"], *(list(map(int, r)) for r in self.modes), *self.most_codes))
        if self.searched:
            rows.append("  round-robin repair: reached by %d of %d drawn histograms" % (self.searched[1], self.searched[0]))
        return "\n".join(rows)

    def floor(self):
        assert not self.empty_cells(), "cells no block showed: %s" % self.empty_cells()


# ---- the streams ---------------------------------------------------------------------------------------------------------------------------------------
FALLBACK = (15, 14, 13, 16, None)


def _alloc(S, zb, at, ml, code, avoid=()):
    """A free run of ml + 2 bytes in block zb whose distance from `at` has Offset code `code` (None: any) and is none of `avoid`;
    None when there is none."""
    zlo, zn = S.block(zb)
    dmin, dmax = ((1 << code) - 3, (2 << code) - 4) if code is not None else (ml, at)
    a, top = max(zlo + 1, at - dmax), min(zlo + zn - ml - 1, at - dmin)
    u = max(a, S.ptr.get((zb, code), 0))
    while u <= top:
        hit = np.nonzero(S.used[u - 1:u + ml + 1])[0]
        if not len(hit) and at - u in avoid:
            hit = [0]
        if not len(hit):
            S.used[u - 1:u + ml + 1] = True
            S.ptr[(zb, code)] = u + ml + 1
            return u
        u += int(hit[-1]) + 1
    return None


def zone_fill(S, recipe, tb=1, zb=None, x0=0):
    """Sequences for block tb, laid from its byte x0 on.  recipe: (kind, ll, ml, code) -- ll fresh bytes, then ml bytes copied from
      "far":  a fresh unit of its own in block zb (the block in front), anchors of the long-distance table every 8 bytes, at a
              distance of Offset code `code` where block zb has room for that (else of a code of FALLBACK);
      "near": the first ml bytes of its own literal run (ll >= ROUND + ml: a round the hash table's walk has behind it), distance ll.
    Behind each copy and in front of it lie bytes that differ from its source's, so the planted length is exact."""
    zb = tb - 1 if zb is None else zb
    if not hasattr(S, "used"):
        S.used, S.ptr = np.zeros(S.n, dtype=bool), {}
    lo, bn = S.block(tb)
    at, todo, last = lo + x0, [], []
    for kind, ll, ml, code in recipe:
        run, at = at, at + ll
        assert at + ml <= lo + bn, (S.name, "the recipe does not fit its block")
        if kind == "near":
            assert ll >= P.ROUND + ml, (S.name, ll, ml)
            u = run
            S.fresh(u, ml)
        else:
            u = None
            for c in (code,) + tuple(c for c in FALLBACK if c != code):
                u = _alloc(S, zb, at, ml, c, last[-3:])               # (none of the three distances a repeat code would stand for)
                if u is not None:
                    break
            assert u is not None, (S.name, "no room for a source")
            S.fresh(u, ml)
            for j in range(0, max(ml - 15, 1), 8):                    # an anchor every 8 bytes while 16 bytes follow: a source whose
                while ml >= 8 and not P.is_anchor(S.d[u + j:u + j + 8]):      # slot of the table another anchor holds has others
                    S.d[u + j:u + j + 8] = S.draw(8, nonzero=True)
        S.d[at:at + ml] = S.d[u:u + ml]                               # (Stream.copy locks all that lies between the two as well)
        S.lock[u:u + ml] = S.lock[at:at + ml] = True
        todo.append((at, ml, at - u)); last.append(at - u)
        at += ml
    for t, l, d in todo:
        S.differ(t - d + l, t + l); S.differ(t - d - 1, t - 1)
        S.plants.append((t, l, d)); S.cells.append(None)
    S.claim(lo + x0, "block", tb, x0)
    return at - lo


def chain_fill(S, tb, ml=8, d=8 * (8 + 1), far=()):
    """Block tb from its third round on: ml bytes from d back, one literal, over and over (every sequence but the first a repeat code);
    `far`: (index, ml, code) -- sequences in between whose source is a unit of their own in the block in front.  d and the lengths of the
    far ones keep every literal a multiple of ml + 1 from the first: a literal is copied from by nothing but literals."""
    assert d % (ml + 1) == 0 and all((m - ml) % (ml + 1) == 0 for _, m, _ in far)
    lo, bn = S.block(tb)
    at, lits, i, far = lo + 2 * P.ROUND, [], 0, {k: (m, c) for k, m, c in far}
    while at + 80 < lo + bn:
        if i in far:
            zone_fill(S, [("far", 0, far[i][0], far[i][1])], tb=tb, x0=at - lo)
            at += far[i][0]
            S.claims.pop()
        else:
            S.copy(at, ml, d)
            S.plants.append((at, ml, d)); S.cells.append(None)
            at += ml
        lits.append(at); at += 1; i += 1
    for a in lits:                                                    # (once every copy is made: the literals are copied from too)
        S.lock[a] = False
    for a in lits:
        S.differ(a, a - d)
    S.claim(lo + 2 * P.ROUND, "round", tb, 2 * P.ROUND)


def _stream(seed, name, fill, route="direct", n=2 * 46000, wlog=P.WINDOW_LOG_DIRECT, stage="lzx", env=None):
    bs = min(1 << P.LZX_BLOCK_LOG, 1 << wlog) if stage == "lzx" else 1 << int(env["NAF_GPU_BLOCK_LOG"])

    def make(salt):
        S = Stream("seq." + name, seed, n, route, bs, "even", salt)
        fill(S)
        if stage == "lz":
            return S.case("lz", "seq", name, level=1, env=env)
        return S.case("lzx", "seq", name, level=2, wlog=wlog) if route == "direct" else S.case("lzx", "seq", name, long_log=wlog, wlog=wlog)
    return P._drawn(make)


def _count_recipe(rng, k, bn=None):
    """k sequences with lengths and codes drawn.  Sources in the block in front: literal runs of 0 to 24 bytes, matches of 32 to 56 (one
    or two sequences: 500 and 300), Offset codes 13 to 15.  bn given: sources in the literal runs, which share a block of bn bytes."""
    out = []
    for _ in range(k):
        if bn is not None:
            per = bn // k
            ml = int(rng.integers(5, min(30, (per - P.ROUND) // 2 - 1)))
            out.append(("near", P.ROUND + ml + int(rng.integers(0, per - P.ROUND - 2 * ml + 1)), ml, None))
        elif k > 2:
            out.append(("far", int(rng.integers(0, 25)), int(rng.integers(32, 57)), int(rng.choice([13, 14, 15], p=[0.2, 0.2, 0.6]))))
        else:
            out.append(("far", 500, 300, 15))
    return out


def seq_cases(seed):
    out = []
    add = lambda *a, **kw: out.append(_stream(seed, *a, **kw))
    # count: exactly k sequences in the block behind the sources', every change of the planner's log and of the header's form
    for k in COUNTS:
        add("count.n%d" % k, lambda S, k=k: zone_fill(S, _count_recipe(S.rng, k)))
    # ... and thousands: 8 bytes from 72 back, a literal; three sources of their own between them, so that Offset codes occur once
    # among thousands of repeat codes and the sum of the probabilities has to be taken down
    add("count.thousands", lambda S: chain_fill(S, 1, far=((700, 44, 13), (1400, 53, 14), (2100, 62, 15))))
    # two and three Offset codes: equal, skewed, a tie that needs topping up; one Literals_Length and one Match_Length code beside them
    two = lambda a, b: [("far", 10, 40, 14 if i % 2 else 15) for i in range(2 * min(a, b))] + [("far", 10, 40, 15)] * (a - min(a, b)) + [("far", 10, 40, 14)] * (b - min(a, b))
    add("codes.two_equal", lambda S: zone_fill(S, two(32, 32)))
    add("codes.two_skewed", lambda S: zone_fill(S, two(60, 4)))
    add("norm.tie_topup", lambda S: zone_fill(S, [("far", 10, 40, (13, 14)[i % 2]) for i in range(40)] + [("far", 10, 40, 15)] * 10))
    add("outcome.all_rle", lambda S: zone_fill(S, [("far", 10, 40, 15)] * 300))
    # the code ranges
    ll_small = [v for f in LL_FIRST[:-1] for v in (f - 1, f)]
    add("range.ll_small", lambda S: zone_fill(S, [("far", v, 40, 15) for v in ll_small] + [("far", 0, 44, 14), ("far", 0, 48, 13)]))
    for name, v in (("ll_16383_16384", (16383, 16384)), ("ll_32767", (32767,)), ("ll_32768", (32768,)), ("ll_65000", (65000,))):
        add("range." + name, lambda S, v=v: zone_fill(S, [("far", x, 60, None) for x in v]), n=2 * 65536)
    ml_small = [v for f in ML_FIRST[:-1] for v in (f - 1, f)]
    add("range.ml_small", lambda S: zone_fill(S, [("far", 5, v, None) for v in ml_small]))
    for name, v in (("ml_16386_16387", (16386, 16387)), ("ml_32770", (32770,)), ("ml_32771", (32771,))):
        add("range." + name, lambda S, v=v: zone_fill(S, [("far", 7, x, None) for x in v]), n=2 * 65536)
    largest = [("near", P.ROUND + 2 * v, v, None) for v in range(5, 24)] + [("far", 3, v, None) for v in range(24, 35)] + [("far", 3, f, None) for f in ML_FIRST]
    add("codes.largest", lambda S: zone_fill(S, largest), n=2 * 65536)

    def of_far(S):                                                   # Offset codes 16 to 19: sources in the stream's first block, targets 2 to 9 blocks on
        for tb, code in ((2, 16), (3, 17), (5, 18), (9, 19)):
            zone_fill(S, [("far", 20 + 3 * i, 60 + i, code) for i in range(4)], tb=tb, zb=0)
    add("range.of_far", of_far, n=10 * 65536)
    # the archive route: blocks of 1, 4 and 64 KiB of printable letters, where few sequences pay
    def arch(counts):                                                # counts[b] sequences in block b
        def fill(S):
            for tb, k in enumerate(counts):
                if k:
                    zone_fill(S, _count_recipe(S.rng, k, S.block(tb)[1]) if k > 2 else [("near", 170, 100, None), ("near", 120, 50, None)][:k], tb=tb)
        return fill
    add("arch.w10", arch((0, 1, 0, 2, 0, 1, 2, 0)), route="archive", n=8 * 1024, wlog=10)
    add("arch.w12", arch((0, 31, 32, 0, 31, 32)), route="archive", n=6 * 4096, wlog=12)
    add("arch.w16", arch((63, 64, 127, 128)), route="archive", n=4 * 65536, wlog=16)
    # the in-block stage by the archive route (level 1; the direct route's in-block cases are lz_plan's)
    add("arch.level1", arch((0, 20, 0)), route="archive", n=3 * 4096 - 5, stage="lz", env=P.lz_env(12))
    return out


LZ_PLAN_CLASSES = ("literal", "length", "distance", "count", "rep", "cap", "tables")


def carried_cases(seed):
    """Cases of lz_plan.py that ride along: Literals_Length, Match_Length and Offset codes of the in-block stage at every code seam, the
    repeat codes, the 16-bit cap and the three `tables` cases of the cross-block stage."""
    return [c for c in P.all_cases(seed, "even", lines=False) if c.cls in LZ_PLAN_CLASSES]


def all_cases(seed):
    return seq_cases(seed) + carried_cases(seed)


# ---- sections for the host driver: sequence lists with a given histogram per table ---------------------------------------------------------------
def lists_from(rng, ll_codes, of_codes, ml_codes):
    """(ll, ml, ofv) arrays with the given code per sequence (arrays of equal length, in order), extra bits drawn; lengths within 16 bits."""
    llc, ofc, mlc = (np.asarray(a, dtype=np.int64) for a in (ll_codes, of_codes, ml_codes))
    n = len(llc)
    ll = LL_BASE[llc] + rng.integers(0, 1 << 16, n) % (1 << LL_BITS[llc])
    ml = ML_BASE[mlc] + rng.integers(0, 1 << 16, n) % (1 << ML_BITS[mlc])
    ofv = (1 << ofc) + rng.integers(0, 1 << 30, n) % (1 << ofc)
    ofv = np.where(ofc == 1, 2 + rng.integers(0, 2, n), ofv)
    return np.minimum(ll, 65535), np.minimum(ml, 65535), ofv


def spread(rng, counts):
    """An array of codes with counts[code] of each, shuffled; counts: {code: count}."""
    a = np.concatenate([np.full(c, s, dtype=np.int64) for s, c in counts.items()])
    rng.shuffle(a)
    return a


def wrap_section(section, ll, ml, ofv, rng):
    """A frame of Raw blocks of history and one Compressed block with Raw literals around `section`; returns (frame, content).  The
    history is as long as the largest distance needs; the content comes from zstd_compose's executor of sequences."""
    ofv = np.asarray(ofv, dtype=np.int64)
    need = int(max(ofv.max() - 3, 8)) + 1
    hist = rng.integers(0, 256, need, dtype=np.uint8).tobytes()
    lits = rng.integers(0, 256, int(np.sum(ll)) + 5, dtype=np.uint8).tobytes()
    out = bytearray(hist)
    Z._execute({"lits": lits, "seqs": list(zip(np.asarray(ll).tolist(), np.asarray(ml).tolist(), ofv.tolist()))},
               {"rep": [1, 4, 8], "srcs": []}, out, set(), 1 << 62)
    assert len(out) - len(hist) <= Z.BLOCK_MAX
    n = len(lits)
    lh = bytes([n << 3]) if n < 32 else bytes([4 | ((n & 15) << 4), n >> 4]) if n < 4096 else bytes([12 | ((n & 15) << 4), (n >> 4) & 255, n >> 12])
    body = bytearray()
    for i in range(0, len(hist), Z.BLOCK_MAX):
        part = hist[i:i + Z.BLOCK_MAX]
        body += (len(part) << 3).to_bytes(3, "little") + part
    payload = lh + lits + section
    body += (1 | (2 << 1) | (len(payload) << 3)).to_bytes(3, "little") + payload
    window_log = max(17, (len(out)).bit_length())
    return Z.MAGIC + bytes([0, (window_log - 10) << 3]) + bytes(body), bytes(out)


def model_prefix(ll, ml, ofv):
    """What the cross-block stage's section has to begin with, by the model: Number_of_Sequences, the modes byte, the three tables'
    bytes; None where the model says that no table can be made."""
    codes = codes_of(ll, ml, ofv)
    n = len(codes[0])
    plans = [plan_table(k, h, n) for k, h in enumerate(hists_of(codes))]
    if any(p.mode is None for p in plans):
        return None, plans
    hdr = bytes([n]) if n < 128 else bytes([128 + (n >> 8), n & 255]) if n < 0x7F00 else bytes([255, (n - 0x7F00) & 255, (n - 0x7F00) >> 8])
    return hdr + bytes([(plans[0].mode << 6) | (plans[1].mode << 4) | (plans[2].mode << 2)]) + b"".join(p.desc for p in plans), plans


def search_round_robin(rng, draws, sample=64):
    """Histograms drawn under the planner's log rule: how many reach the second repair of the normalisation (the excess is not below
    the first most frequent code's probability).  Vectorised; `sample` of them per batch are held to `normalise` itself."""
    reached, done = 0, 0
    for batch in range(8):
        m, k = draws // 8, batch % 3
        A = ALPHABET[k]
        present = rng.integers(2, A + 1, m)
        nseq = np.maximum((2.0 ** rng.uniform(1, 15, m)).astype(np.int64), present)
        here = np.argsort(rng.random((m, A)), axis=1) < present[:, None]
        w = np.where(here, rng.random((m, A)) ** rng.choice([1, 4, 16, 64], (m, 1)), 0.0)
        cnt = np.where(here, 1 + np.floor(w / w.sum(axis=1, keepdims=True) * (nseq - present)[:, None]).astype(np.int64), 0)
        first = np.argmax(here, axis=1)
        cnt[np.arange(m), first] += nseq - cnt.sum(axis=1)             # what the floors left, to one code that occurs
        log = np.clip(np.floor(np.log2(nseq)).astype(np.int64) + 1, 5, MAX_LOG[k])
        log = np.where((1 << log) < present, 6, log)
        norm = np.where(cnt > 0, np.maximum(1, (cnt << log[:, None]) // nseq[:, None]), 0)
        over = norm.sum(axis=1) - (1 << log)
        rr = (over > 0) & (norm[np.arange(m), np.argmax(cnt, axis=1)] <= over)
        reached += int(rr.sum()); done += m
        for i in rng.integers(0, m, sample):
            h = np.zeros(64, dtype=np.int64); h[:A] = cnt[i]
            assert accuracy_log(k, int(nseq[i]), int(present[i])) == log[i]
            want = "round_robin" if rr[i] else "exact" if over[i] == 0 else "topup" if over[i] < 0 else "takedown"
            assert normalise(h, int(nseq[i]), int(log[i]))[1] == want
    return done, reached
