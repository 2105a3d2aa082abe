// payload.h -- what every reader of an archive's payload streams shares on the host.  Part of emit.hip (included by it, in front of
// unnaf_run): it uses that file's UnnafPlan, unnaf_prepare and unnaf_sections.
//   payload_range   bytes [lo, hi) of the sequence or quality stream, or the whole stream, decoded into the arena
//   records_front   the front of a call that addresses records [first, first + count) of a 4-bit archive
//   piece_plan      those records cut into pieces of whole records
//   PieceSweep      a piece's part of the packed stream and its tile geometry; the arena is given back piece by piece
#pragma once
#include <algorithm>

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

// arena_reset, the record tables of --sequences (lengths only, no ids; the mask when use_mask) and the checks of first / count.
// who: the caller's name in the messages; cannot: what it cannot do "in protein sequences".  *count comes back resolved
// (NAF_GPU_WHOLE = to the last record); 0 = nothing to do, and the side sections were then not made.
static int records_front(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, int use_mask, const char *who, const char *cannot, u64 first, u64 *count, UnnafPlan &pl)
{
    arena_reset(c);
    naf_gpu_unnaf_opts o = { NAF_OUT_SEQUENCES, use_mask, -1 };
    int rc = unnaf_prepare(c, d_naf, naf_len, &o, pl); if (rc) return rc;
    const naf_gpu_header &h = pl.h;
    if (!pl.fourbit) return ctx_fail(c, NAF_GPU_EARG, "%s: %s in %s sequences", who, cannot, h.seq_type == NAF_SEQ_PROTEIN ? "protein" : "text");
    const u64 N = h.n_sequences;
    if (first > N) return ctx_fail(c, NAF_GPU_EARG, "%s: first record %llu, the archive has %llu", who, (unsigned long long)first, (unsigned long long)N);
    if (*count == NAF_GPU_WHOLE) *count = N - first;
    if (*count > N - first) return ctx_fail(c, NAF_GPU_EARG, "%s: records %llu..%llu of %llu", who, (unsigned long long)first, (unsigned long long)(first + *count), (unsigned long long)N);
    if (N == 0) { *count = 0; return 0; }
    if (!((h.flags >> 1) & 1)) return ctx_fail(c, NAF_GPU_EARG, "%s: the archive stores no sequence", who);
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

// The packed sequence stream under the pieces of one call, piece by piece: a piece's bytes are decoded alone where the frame allows it
// and given back with everything else the piece took from the arena (release, once its kernels were waited for); a frame of dependent
// blocks is decoded whole ONCE, and that stream then stays in front of the mark for the pieces -- and the sweeps -- that follow.
struct PieceSweep {
    naf_gpu_ctx *c; const u8 *d_naf; const UnnafPlan &pl; const char *who;
    std::vector<size_t> mark;
    const u8 *whole_seq = nullptr;
    u64 decoded = 0;                                                              // bytes of the stream decoded so far (the trace lines)
    PieceSweep(naf_gpu_ctx *c_, const u8 *d_naf_, const UnnafPlan &pl_, const char *who_) : c(c_), d_naf(d_naf_), pl(pl_), who(who_), mark(arena_mark(c_)) {}
    // seq: pointer to packed byte 0, bytes [.., b_hi) of it may be read; tile 0 starts at base t0 (even, <= p_lo), ntiles of `tile` bases reach p_hi
    struct Tiles { const u8 *seq; u64 b_hi, t0, ntiles; };
    int seq_for(const RecPiece &pc, u64 tile, Tiles *t)                          // a piece that has bases: p_hi > p_lo
    {
        t->b_hi = (pc.p_hi + 1) / 2; t->t0 = pc.p_lo & ~1ull; t->ntiles = (pc.p_hi - t->t0 + tile - 1) / tile;
        if (t->ntiles > 0x7FFFFFFFull) return ctx_fail(c, NAF_GPU_EARG, "%s: a piece of %llu bases is too long for one launch", who, (unsigned long long)(pc.p_hi - pc.p_lo));
        if (!whole_seq) {
            PayloadSpan sp;
            int rc = payload_range(c, d_naf, pl, S_SEQ, pc.p_lo / 2, t->b_hi, PAYLOAD_RANGE, &sp); if (rc) return rc;
            decoded += sp.got_hi - sp.got_lo;
            if (sp.ranged) { t->seq = sp.base; return 0; }
            whole_seq = sp.base; mark = arena_mark(c);
        }
        t->seq = whole_seq;
        return 0;
    }
    void release() { arena_release(c, mark); }
};
