// payload.h -- what every reader of an archive's payload streams shares on the host.  Part of emit.hip (included by it, in front of
// unnaf_run): it uses that file's UnnafPlan, unnaf_prepare and unnaf_sections.  The device parts of the scanners are packed.h's.
//   payload_range      bytes [lo, hi) of the sequence or quality stream, or the whole stream, decoded into the arena
//   records_front      the front of a call that addresses records [first, first + count) of an archive
//   piece_plan         those records cut into pieces of whole records
//   PieceSweep         a piece's part of a stream (its bytes; the packed one's tile geometry); the arena is given back piece by piece
//   rows_out, rows_copy  a call's rows in the arena and their copy to the caller's table
//   lever_u64          a strict whole-number lever
//   count_then_write   the sweeps of a call that lists what it finds: too small a capacity is found before anything is written
#pragma once
#include <algorithm>

// n things of `per` u64 each, a lane per u64 in workgroups of 256 (2^31 - 1 of them at the most): the caller's message when that is no launch
#define LAUNCH_LIMIT(c, n, per, ...) do { if ((u64)(n) > 0x7FFFFFFFull * 256 / (per)) return ctx_fail((c), NAF_GPU_EARG, __VA_ARGS__); } while (0)

// letter -> its 4-bit code in "-TGKCYSBAWRDMHVN", either case, U = T; -1: no code
static int base_code(char ch)
{
    static const char tab[] = "-TGKCYSBAWRDMHVN";
    if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 32);
    if (ch == 'U') ch = 'T';
    const char *q = (const char *)memchr(tab, ch, 16);
    return q ? (int)(q - tab) : -1;
}

// What a range decode may bring beside the bytes asked for -- the rest of the zstd blocks (128 KiB at the most) at its two ends --
// and the 64 bytes every caller of the decoder leaves behind its output.
#define PAYLOAD_SLACK (2 * 131072 + 64)

enum PayloadMode { PAYLOAD_WHOLE,          // the whole stream (no range is handed to the decoder: c->zsplit / c->zflat may take the frame)
                   PAYLOAD_RANGE,          // the range; a frame of dependent blocks, whose closure is the whole stream, is decoded whole
                   PAYLOAD_RANGE_ONLY };   // the range; such a frame is the caller's: NAF_GPU_ECAP comes back as the decoder left it
struct PayloadSpan { const u8 *base; u64 got_lo, got_hi; bool ranged; };   // base: pointer to stream byte 0; [got_lo, got_hi) of it may be read

// section: S_SEQ or S_QUAL.  c: the context the stream is decoded on; its arena holds the bytes, its err an error's text.
static int payload_range(naf_gpu_ctx *c, const u8 *d_naf, const UnnafPlan &pl, int section, u64 want_lo, u64 want_hi, PayloadMode mode, PayloadSpan *out)
{
    const naf_gpu_header &h = pl.h;
    const u64 bytes = section == S_SEQ ? pl.seq_bytes : h.orig_size[section];
    ZRange zr; memset(&zr, 0, sizeof zr);
    zr.want_lo = want_lo; zr.want_hi = want_hi;
    ZRange *rg = mode == PAYLOAD_WHOLE ? nullptr : &zr;
    u8 *buf = nullptr; size_t n = 0;
    auto decode = [&](u64 need, const u8 *head) -> int {                         // need: the buffer, the 64 bytes behind the output among them
        if (need > bytes + 64) need = bytes + 64;
        buf = (u8 *)arena_alloc(c, need); if (!buf) return NAF_GPU_ENOMEM;
        return zstd_decode_range(c, d_naf + h.payload_off[section], h.comp_size[section], 0, buf, need - 64, &n, rg, head);
    };
    int r = decode(rg ? (want_hi - want_lo) + PAYLOAD_SLACK : bytes + 64, pl.frame_head[section]);
    if (r == NAF_GPU_ECAP && mode == PAYLOAD_RANGE_ONLY) return r;
    if (r == NAF_GPU_ECAP && rg) { rg = nullptr; r = decode(bytes + 64, nullptr); }
    if (r == NAF_GPU_ECAP || (r == 0 && n != bytes)) return ctx_fail(c, NAF_GPU_EFORMAT, section == S_SEQ ? "can't decompress sequence\n" : "can't decompress quality\n");
    if (r) return r;
    out->ranged = rg && rg->ranged;
    out->got_lo = out->ranged ? rg->got_lo : 0; out->got_hi = out->ranged ? rg->got_hi : bytes;
    out->base = out->ranged ? (rg->own_buf ? rg->own_buf : buf) - rg->got_lo : buf;
    return 0;
}

// arena_reset, the record tables of --sequences (lengths only, no ids; the mask with FRONT_MASK) and the checks of first / count.
// who: the caller's name in the messages; cannot: what it cannot do "in protein sequences" when it needs FRONT_4BIT.  FRONT_QUALITY: a
// quality section, and a sequence section of any type for its lengths.  *count comes back resolved (NAF_GPU_WHOLE = to the last
// record); 0 = nothing to do, and the side sections were then not made.  reset = false: the front of a call's SECOND archive, whose
// tables go behind the first's.
enum { FRONT_4BIT = 1, FRONT_MASK = 2, FRONT_QUALITY = 4 };
static int records_front(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, int needs, const char *who, const char *cannot, u64 first, u64 *count, UnnafPlan &pl,
                         bool reset = true)
{
    if (reset) arena_reset(c);
    naf_gpu_unnaf_opts o = { NAF_OUT_SEQUENCES, needs & FRONT_MASK ? 1 : 0, -1 };
    int rc = unnaf_prepare(c, d_naf, naf_len, &o, pl); if (rc) return rc;
    const naf_gpu_header &h = pl.h;
    if ((needs & FRONT_4BIT) && !pl.fourbit) return ctx_fail(c, NAF_GPU_EARG, "%s: %s in %s sequences", who, cannot, h.seq_type == NAF_SEQ_PROTEIN ? "protein" : "text");
    const u64 N = h.n_sequences;
    if (first > N) return ctx_fail(c, NAF_GPU_EARG, "%s: first record %llu, the archive has %llu", who, (unsigned long long)first, (unsigned long long)N);
    if (*count == NAF_GPU_WHOLE) *count = N - first;
    if (*count > N - first) return ctx_fail(c, NAF_GPU_EARG, "%s: records %llu..%llu of %llu", who, (unsigned long long)first, (unsigned long long)(first + *count), (unsigned long long)N);
    if (N == 0) { *count = 0; return 0; }
    if ((needs & FRONT_QUALITY) && !(h.flags & 1)) return ctx_fail(c, NAF_GPU_EARG, "%s: the archive has no quality section", who);
    if (!((h.flags >> 1) & 1)) return ctx_fail(c, NAF_GPU_EARG, "%s: the archive stores no sequence%s", who, needs & FRONT_QUALITY ? " to hold its lengths against" : "");
    if (*count == 0) return 0;
    return unnaf_sections(c, d_naf, pl);
}

// Records [r_lo, r_hi), bases [p_lo, p_hi) of the stream: rec_base[r_lo] = p_lo, rec_base[r_hi] = p_hi.
struct RecPiece { u64 r_lo, r_hi, p_lo, p_hi; };

// Records [first, first + count) as pieces of whole records, as many as stay within the piece size -- NAF_GPU_<opt>, else dflt bases;
// a longer record is a piece of its own.  d_scan (may be null): an exclusive scan over these records (count + 1 values on the device,
// scan_total the last); at then gets its value at every piece's first record, and scan_total behind them.
static int piece_plan(naf_gpu_ctx *c, const EmitP &P, u64 first, u64 count, const char *opt, u64 dflt, std::vector<RecPiece> &pieces,
                      const u64 *d_scan = nullptr, u64 scan_total = 0, std::vector<u64> *at = nullptr)
{
    u64 piece = dflt;
    { const char *e = ctx_opt(c, opt); if (e && e[0]) { const u64 v = strtoull(e, nullptr, 10); if (v) piece = v; } }
    u64 ends[2] = { 0, 0 };
    int rc = ctx_readback2(c, &ends[0], P.rec_base + first, 8, &ends[1], P.rec_base + first + count, 8); if (rc) return rc;
    if (ends[1] - ends[0] <= piece) { pieces.push_back({ first, first + count, ends[0], ends[1] }); if (at) at->push_back(0); }
    else {
        std::vector<u64> base(count + 1), sc(d_scan ? count + 1 : 0);
        HIP_TRY(c, hipMemcpyAsync(base.data(), P.rec_base + first, (count + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        if (d_scan) HIP_TRY(c, hipMemcpyAsync(sc.data(), d_scan, (count + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (u64 a = 0; a < count; ) {
            u64 b = (u64)(std::upper_bound(base.begin() + a, base.end(), base[a] + piece) - base.begin()) - 1;   // last record end within the piece
            if (b <= a) b = a + 1;
            pieces.push_back({ first + a, first + b, base[a], base[b] });
            if (at) at->push_back(sc[a]);
            a = b;
        }
    }
    if (at) at->push_back(scan_total);
    return 0;
}

// One payload stream under the pieces of one call, piece by piece: a piece's bytes are decoded alone where the frame allows it and
// given back with everything else the piece took from the arena (release, once its kernels were waited for); a frame of dependent
// blocks is decoded whole ONCE, and that stream then stays in front of the mark for the pieces -- and the sweeps -- that follow.
struct PieceSweep {
    naf_gpu_ctx *c; const u8 *d_naf; const UnnafPlan &pl; const char *who; int section;
    std::vector<size_t> mark;
    const u8 *whole = nullptr;
    u64 decoded = 0;                                                              // bytes of the stream decoded so far (the trace lines)
    PieceSweep(naf_gpu_ctx *c_, const u8 *d_naf_, const UnnafPlan &pl_, const char *who_, int section_ = S_SEQ)
        : c(c_), d_naf(d_naf_), pl(pl_), who(who_), section(section_), mark(arena_mark(c_)) {}
    // the byte view: sp->base points to stream byte 0, bytes [got_lo, got_hi) of it may be read (all of [lo, hi) unless the stream is shorter than its header says)
    int bytes_for(u64 lo, u64 hi, PayloadSpan *sp)
    {
        if (!whole) {
            int rc = payload_range(c, d_naf, pl, section, lo, hi, PAYLOAD_RANGE, sp); if (rc) return rc;
            decoded += sp->got_hi - sp->got_lo;
            if (sp->ranged) return 0;
            whole = sp->base; mark = arena_mark(c);
        }
        sp->base = whole; sp->got_lo = 0; sp->got_hi = section == S_SEQ ? pl.seq_bytes : pl.h.orig_size[section]; sp->ranged = false;
        return 0;
    }
    // the 4-bit view of a piece that has bases (p_hi > p_lo): seq points to packed byte 0, bytes [.., b_hi) of it may be read; tile 0
    // starts at base t0 (even, <= p_lo), ntiles of `tile` bases reach p_hi
    struct Tiles { const u8 *seq; u64 b_hi, t0, ntiles; };
    int seq_for(const RecPiece &pc, u64 tile, Tiles *t)
    {
        t->b_hi = (pc.p_hi + 1) / 2; t->t0 = pc.p_lo & ~1ull; t->ntiles = (pc.p_hi - t->t0 + tile - 1) / tile;
        if (t->ntiles > 0x7FFFFFFFull) return ctx_fail(c, NAF_GPU_EARG, "%s: a piece of %llu bases is too long for one launch", who, (unsigned long long)(pc.p_hi - pc.p_lo));
        PayloadSpan sp;
        int rc = bytes_for(pc.p_lo / 2, t->b_hi, &sp); if (rc) return rc;
        t->seq = sp.base;
        return 0;
    }
    void release() { arena_release(c, mark); }
};

// The table of a call's rows in the arena (n rows of `per` u64, 8-byte aligned, written by the kernels), and its copy to the caller's
// table of any alignment under the launch name given; bad: k_row_copy's
static int rows_out(naf_gpu_ctx *c, u64 **rows, u64 n, u32 per) { *rows = arena_new<u64>(c, n * per); return *rows ? 0 : NAF_GPU_ENOMEM; }
static void rows_copy(naf_gpu_ctx *c, const char *name, const u64 *rows, u8 *d_rows, u64 n, u32 per, const unsigned long long *bad = nullptr)
{
    LAUNCH(c, name, k_row_copy, cdiv(n * per, 256), 256, 0, rows, d_rows, n * per, bad);
}

// A lever NAF_GPU_<name> that is a whole number from 0 to max: *value when it is given, and *set (may be null) says whether.  Returns
// false when what is given is none (the caller has the message: it knows the range's words)
static bool lever_u64(naf_gpu_ctx *c, const char *name, u64 max, bool *set, u64 *value)
{
    const char *e = ctx_opt(c, name);
    if (set) *set = false;
    if (!e || !e[0]) return true;
    char *end = nullptr; const unsigned long long v = strtoull(e, &end, 10);
    if (*end || v > max) return false;
    if (set) *set = true;
    *value = v;
    return true;
}

static int cap_fail(naf_gpu_ctx *c, const char *who, const char *things, u64 n, size_t cap) { return ctx_fail(c, NAF_GPU_ECAP, "%s: %llu %s, capacity %zu", who, (unsigned long long)n, things, cap); }

// A piece's tile counts a[0 .. ntiles) (a[ntiles] = 0) become their exclusive scan, and the total comes back; b: a second table, or null.
static int tile_totals(naf_gpu_ctx *c, u64 ntiles, u64 *a, u64 *na, u64 *b = nullptr, u64 *nb = nullptr)
{
    int r = scan_exclusive_u64(c, a, ntiles + 1, (u64 *)nullptr); if (r) return r;
    if (!b) return ctx_readback(c, na, a + ntiles, 8);
    if ((r = scan_exclusive_u64(c, b, ntiles + 1, (u64 *)nullptr))) return r;
    return ctx_readback2(c, na, a + ntiles, 8, nb, b + ntiles, 8);
}

// A call that lists `things` (write: into `cap` places) or only counts them, piece by piece.  body(pc, tl, writing, before, &here) gives
// a piece's count as `here` and, when writing, stores its things behind the `before` of the pieces in front -- or returns a bare
// NAF_GPU_ECAP when before + here > cap.  With several pieces a counting sweep goes first, so that nothing is written when `cap` is too
// small.  d_sums: device bytes every sweep starts from zero.  *n_out: the things in all, behind NAF_GPU_ECAP too.
struct ListCall { const char *things; bool write; size_t cap; void *d_sums; size_t sums_bytes; };
template <typename Body>
static int count_then_write(PieceSweep &sw, const std::vector<RecPiece> &pieces, u64 tile, const ListCall &L, u64 *n_out, Body body)
{
    naf_gpu_ctx *c = sw.c;
    u64 total = 0;
    auto sweep = [&](bool writing) -> int {
        total = 0;
        HIP_TRY(c, hipMemsetAsync(L.d_sums, 0, L.sums_bytes, c->stream));
        for (const RecPiece &pc : pieces) {
            if (pc.p_hi == pc.p_lo) continue;
            PieceSweep::Tiles tl; u64 here = 0;
            int r = sw.seq_for(pc, tile, &tl); if (r) return r;
            r = body(pc, tl, writing, total, &here);
            total += here;
            if (r) return r;
            sw.release();
        }
        return 0;
    };
    int rc = 0;
    if (!L.write || pieces.size() > 1) { if ((rc = sweep(false))) return rc; }
    *n_out = total;
    if (!L.write) return 0;
    if (total <= L.cap) rc = sweep(true);                                         // (one piece: not counted yet, its own count decides)
    if (rc && !(rc == NAF_GPU_ECAP && total > L.cap)) return rc;
    *n_out = total;
    return total > L.cap ? cap_fail(c, sw.who, L.things, total, L.cap) : 0;
}
