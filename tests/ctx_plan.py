"""What the tests of the context share (test_ctx_plan_cpu.py shows the judges can see; test_gpu_streams.py, test_gpu_scratch.py and
test_gpu_io.py use them): a table of probes, a late producer, and a byte pattern that depends on the position.

A probe is one family of entry points with the smallest input that still takes the family's real path: `real` is that input, `bait` a
valid input of the same kind and the same number of bytes (a shorter one has zero bytes behind it) whose result differs, `run` the
raw call on device buffers, `reference` what the oracle, a *_plan.py brute force or numpy says the result is.  A library that looked at
its input before the producer on the stream had written it finds the bait there and returns the bait's result: a wrong answer, never
garbage.  Plain helpers, no fixtures; nothing here needs a GPU until a probe's run is called."""
import ctypes as C

import numpy as np

import composition_plan as CP
import kmers_plan as KP
import locate_near_plan as NP
import locate_plan as LP
import orfs_plan as OP
import quality_plan as QP
import runs_plan as RP
import select_plan as SP
from conftest import golden_bytes

FASTA, FASTQ, SEQUENCES = 0, 1, 3
EOL = (0x0A, 0x0B, 0x0C, 0x0D)
WHOLE = 2 ** 64 - 1
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


# ---- the position-dependent pattern ------------------------------------------------------------------------------------------------
def pattern(n, off=0, salt=0):
    """Bytes [off, off + n) of a pattern in which every power-of-two shift up to 2^31 changes the byte: fenced.Arena.pattern's idea
    (i * 131 + 89) ^ salt repeats after 256 bytes, so the higher bytes of the position are mixed in -- a chunk that lands 4, 8 or 16 MiB
    off, two swapped chunks and a chunk written twice all differ from what belongs there."""
    out = np.empty(n, dtype=np.uint8)
    step = 1 << 22
    for a in range(0, n, step):
        i = np.arange(off + a, off + min(n, a + step), dtype=np.int64)
        out[a:a + len(i)] = ((i * 131 + 89 + (i >> 8) * 37 + (i >> 16) * 101 + (i >> 24) * 59) & 0xFF) ^ salt
    return out


def pattern_diff(got, n, off=0, salt=0, shifts=(1, -1, 1 << 22, -(1 << 22), 1 << 23, -(1 << 23), 1 << 24, -(1 << 24))):
    """None when `got` is bytes [off, off + n) of the pattern; else a sentence: the length, or the first wrong byte, how many are wrong,
    and -- when the bytes from there on are the pattern of another place -- which shift they carry."""
    got = np.frombuffer(bytes(got), dtype=np.uint8) if not isinstance(got, np.ndarray) else got
    if len(got) != n:
        return "%d bytes, not %d (%s by %d)" % (len(got), n, "short" if len(got) < n else "long", abs(n - len(got)))
    bad = np.flatnonzero(got != pattern(n, off, salt))
    if not len(bad):
        return None
    k, m = int(bad[0]), min(64, n - int(bad[0]))
    for s in shifts:
        if off + k + s >= 0 and np.array_equal(got[k:k + m], pattern(m, off + k + s, salt)):
            return "byte %d of %d is wrong, %d in all; from there the bytes are those of a place %+d bytes away" % (k, n, len(bad), s)
    return "byte %d of %d is wrong (0x%02x, not 0x%02x), %d in all" % (k, n, int(got[k]), int(pattern(1, off + k, salt)[0]), len(bad))


# ---- the late producer -----------------------------------------------------------------------------------------------------------
class Delay:
    """About `target_ms` of work for a stream, calibrated once with events: torch.cuda._sleep where it is usable, else a chain of device
    copies.  ms is what one enqueue() measured; the modules that use it assert ms >= 20 and print it."""

    def __init__(self, target_ms=50.0):
        import torch
        self.torch, self.spin, self.copies, self.buf = torch, 0, 0, None
        try:
            torch.cuda._sleep(1000)                                     # (the first call of a kernel pays for loading it)
            spin = 10_000_000
            for _ in range(3):                                          # the count is in cycles of a clock the test does not know: measure, rescale, measure again
                one = self._time(lambda: torch.cuda._sleep(spin))
                if one <= 0.5:
                    spin = 0
                    break
                spin = max(1, int(spin * target_ms / one))
            self.spin = spin
        except Exception:
            self.spin = 0
        if not self.spin:
            self.buf = torch.empty(2, 128 << 20, dtype=torch.uint8, device="cuda")
            one = self._time(lambda: [self.buf[1].copy_(self.buf[0]) for _ in range(16)]) / 16
            self.copies = max(1, int(target_ms / max(one, 1e-3)))
        self.ms = self._time(self._work)

    def _time(self, work):
        torch = self.torch
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); work(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def _work(self):
        if self.spin:
            self.torch.cuda._sleep(self.spin)
        else:
            for _ in range(self.copies):
                self.buf[1].copy_(self.buf[0])

    def enqueue(self, stream):
        with self.torch.cuda.stream(stream):
            self._work()


def late(stream, buf, real, delay):
    """buf holds a bait.  Enqueues the delay on `stream`, then the copy of `real` (a device tensor) over the front of buf, and returns
    without a host wait: whoever reads buf in stream order finds `real`, whoever reads it now finds the bait."""
    import torch
    delay.enqueue(stream)
    with torch.cuda.stream(stream):
        buf[:real.numel()].copy_(real, non_blocking=True)


def padded(bait, n):
    assert len(bait) <= n, "a bait is no longer than the real input (%d > %d)" % (len(bait), n)
    return bait + b"\0" * (n - len(bait))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _fasta_bait(text):
    """The records behind the first with every base complemented: record numbers shift, ids stay, every base differs."""
    recs = text.split(b">")[2:]
    out = []
    for r in recs:
        head, _, body = r.partition(b"\n")
        out.append(b">" + head + b"\n" + body.translate(_COMP))
    return b"".join(out)


def _fastq_bait(text):
    lines = text.split(b"\n")[4:-1]
    out = []
    for k in range(0, len(lines), 4):
        q = bytes(33 + (c - 33 + 7) % 41 for c in lines[k + 3])
        out += [lines[k], lines[k + 1].translate(_COMP), lines[k + 2], q]
    return b"\n".join(out) + b"\n"


def _same_length_text_bait(text):
    """A text of the same length and line structure with every base complemented (header lines keep their bytes)."""
    return b"\n".join(ln if ln[:1] in b">@+" else ln.translate(_COMP) for ln in text.split(b"\n"))


def count_line_starts(data, prev_is_eol):
    """numpy: the non-EOL bytes that stand behind an EOL-class byte (the byte in front of the slice counts through prev_is_eol)."""
    a = np.frombuffer(data, dtype=np.uint8)
    if not len(a):
        return 0
    e = np.isin(a, EOL)
    return int((np.concatenate([[bool(prev_is_eol)], e[:-1]]) & ~e).sum())


LINE_SLICES = (0, 1, 4095, 4096, 4097, None)         # prefixes of the slice the line-count probe asks about (None: all of it)


def _rows_bytes(rows, dtype):
    out = np.zeros(len(rows), dtype=dtype)
    for k, name in enumerate(n for n, *_ in dtype):
        out[name] = [r[k] for r in rows] if len(rows) else []
    return out.tobytes()


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t.numel() else 0)


def _lines(oracle, naf):
    return CP.lines_of(oracle.unnaf(naf, SEQUENCES, True), oracle.parse_naf(naf).n_sequences)


def _streams(oracle, naf):
    """What an archive holds, as the oracle reads it: the five (six) decoded streams and the framing."""
    h = oracle.parse_naf(naf)
    return tuple(None if h.payload_off[i] is None else oracle.zstd_decompress(h.frame(naf, i), h.orig[i] + 16) for i in range(6)) + (h.n_sequences, h.line_length)


def _split(oracle, text):
    sp = oracle.split_text(text)
    return (sp.ids, sp.comments, sp.lengths, sp.mask, sp.seq, sp.qual if sp.format == oracle.FMT_FASTQ else None, sp.n_sequences, sp.longest_line)


class Probe:
    """name; entries: the C-ABI functions run() calls; real, bait: input bytes of one length; cap: bytes of the output buffer;
    run(ctx, d_in, d_out) -> (rc, host results, bytes of d_out that are the result); reference(oracle, data) -> (host results, output) for
    any valid input; digest(oracle, out bytes): what of an output is compared (the bytes themselves, or what the oracle reads from
    them); env: switches the probe runs under; side: the call is to use streams of the context besides the caller's."""

    def __init__(self, name, entries, real, bait, cap, run, reference, digest=None, env=None, side=False, contexts=1):
        self.name, self.entries, self.real, self.bait, self.cap = name, tuple(entries), real, padded(bait, len(real)), cap
        self.run, self.reference, self.env, self.side, self.contexts = run, reference, env or {}, side, contexts
        self.digest = digest or (lambda oracle, out: out)
        self._ref = None

    def ref(self, oracle):
        """computed once, left unchanged"""
        if self._ref is None:
            self._ref = self.reference(oracle, self.real)
        return self._ref

    def judge(self, oracle, rc, host, out):
        want_host, want_out = self.ref(oracle)
        assert rc == 0, (self.name, rc)
        assert host == want_host, (self.name, "host results", host, want_host)
        got = self.digest(oracle, out)
        assert got == want_out, (self.name, "output", len(out), got[:80] if isinstance(got, bytes) else None)

    def __repr__(self):
        return self.name


NAMES = ("zstd_compress", "zstd_decompress", "unnaf_fasta", "unnaf_fastq", "unnaf_size", "unnaf_range", "unnaf_select_stranded", "unnaf_find_record_table",
         "unnaf_locate", "unnaf_locate_near", "unnaf_composition", "unnaf_quality", "unnaf_runs", "unnaf_kmers", "unnaf_orfs", "ennaf_overlap", "ennaf_shards",
         "histogram", "count_lines_lf", "count_lines_crlf")
SIDE_NAMES = ("unnaf_fasta", "unnaf_fastq", "ennaf_overlap", "ennaf_shards")      # the probes that are to use more streams than the caller's
TALLY, ENTRIES = {}, {}                                                            # (probe, mode) -> runs; entry point -> calls made from tests/


def count(name, mode, entries=()):
    TALLY[(name, mode)] = TALLY.get((name, mode), 0) + 1
    for e in entries:
        ENTRIES[e] = ENTRIES.get(e, 0) + 1


def report(modes):
    """What a module prints when it is done (and writes to NAF_TEST_TALLY when that is set; the counts are the process's, so the last
    module's file holds them all): every probe under every mode, and the calls each entry point got."""
    import json
    import os
    text = tally_table(TALLY, modes) + "\n" + "\n".join("%-34s %d" % (e, n) for e, n in sorted(ENTRIES.items()))
    print("\n" + text)
    if os.environ.get("NAF_TEST_TALLY"):
        with open(os.environ["NAF_TEST_TALLY"], "w") as f:
            json.dump({"probes": {"%s/%s" % k: v for k, v in sorted(TALLY.items())}, "entries": dict(sorted(ENTRIES.items()))}, f, indent=1)


_PROBES = None


def probes(oracle):
    """The table, made once (the archives come from the oracle's ennaf)."""
    global _PROBES
    if _PROBES is None:
        _PROBES = _make(oracle)
    return _PROBES


def by_name(oracle):
    return {p.name: p for p in probes(oracle)}


def _make(O):
    from naf_amd import capi, synth
    L = capi.load()
    P = []
    text_fa = synth.fasta_mixed(7, 2100, 60, seed=22)
    text_fq = synth.fastq_reads(100, 120, seed=3, var_len=True)
    naf_fa, naf_fq = O.ennaf(text_fa), O.ennaf(text_fq)
    bait_fa, bait_fq = O.ennaf(_fasta_bait(text_fa)), O.ennaf(_fastq_bait(text_fq))

    # ---- zstd
    def run_compress(ctx, d_in, d_out):
        n = C.c_size_t(1 << 40)
        rc = ctx.L.naf_gpu_zstd_compress(ctx.h, _ptr(d_in), d_in.numel(), 1, _ptr(d_out), d_out.numel(), C.byref(n))
        return rc, (), n.value
    P.append(Probe("zstd_compress", ["naf_gpu_zstd_compress"], text_fa, _same_length_text_bait(text_fa), L.naf_gpu_zstd_compress_bound(len(text_fa)), run_compress,
                   lambda O, data: ((), data), digest=lambda O, out: O.zstd_decompress(out, len(text_fa) + 16)))

    frame = golden_bytes("zstd", "ids_l3.zst")
    raw_bait = next(f for f in (O.zstd_store_raw(bytes(pattern(k, salt=0x5A))) for k in range(len(frame), max(len(frame) - 32, 0), -1)) if len(f) == len(frame))
    plain = O.zstd_decompress(frame)

    def run_decompress(ctx, d_in, d_out):
        n = C.c_size_t(1 << 40)
        rc = ctx.L.naf_gpu_zstd_decompress(ctx.h, _ptr(d_in), d_in.numel(), 1, _ptr(d_out), d_out.numel(), C.byref(n))
        return rc, (n.value,), n.value
    P.append(Probe("zstd_decompress", ["naf_gpu_zstd_decompress"], frame, raw_bait, len(plain), run_decompress,
                   lambda O, data: (lambda p: ((len(p),), p))(O.zstd_decompress(data))))

    # ---- unnaf: whole texts, a size, a range, a selection, the tables
    def run_unnaf(mode, begin=None, end=None, size_only=False):
        def run(ctx, d_in, d_out):
            o, n = capi.UnnafOpts(mode, 1, -1), C.c_size_t(1 << 40)
            if size_only:
                rc = ctx.L.naf_gpu_unnaf_size(ctx.h, _ptr(d_in), d_in.numel(), C.byref(o), C.byref(n))
                return rc, (n.value,), 0
            if begin is None:
                rc = ctx.L.naf_gpu_unnaf(ctx.h, _ptr(d_in), d_in.numel(), C.byref(o), _ptr(d_out), d_out.numel(), C.byref(n))
            else:
                rc = ctx.L.naf_gpu_unnaf_range(ctx.h, _ptr(d_in), d_in.numel(), C.byref(o), begin, end, _ptr(d_out), d_out.numel(), C.byref(n))
            return rc, (n.value,), n.value
        return run

    def ref_unnaf(mode, begin=None, end=None, size_only=False):
        def ref(O, naf):
            t = O.unnaf(naf, mode, True, -1)
            t = t if begin is None else t[begin:end]
            return ((len(t),), b"" if size_only else t)
        return ref
    fa_text, fq_text = O.unnaf(naf_fa, FASTA), O.unnaf(naf_fq, FASTQ)
    P.append(Probe("unnaf_fasta", ["naf_gpu_unnaf"], naf_fa, bait_fa, len(fa_text), run_unnaf(FASTA), ref_unnaf(FASTA), side=True))
    P.append(Probe("unnaf_fastq", ["naf_gpu_unnaf"], naf_fq, bait_fq, len(fq_text), run_unnaf(FASTQ), ref_unnaf(FASTQ), side=True))
    P.append(Probe("unnaf_size", ["naf_gpu_unnaf_size"], naf_fa, bait_fa, 0, run_unnaf(FASTA, size_only=True), ref_unnaf(FASTA, size_only=True)))
    b, e = 1003, 1003 + 4097
    assert e < len(fa_text)
    P.append(Probe("unnaf_range", ["naf_gpu_unnaf_range"], naf_fa, bait_fa, e - b, run_unnaf(FASTA, b, e), ref_unnaf(FASTA, b, e)))

    segs = [(1, 7, 40, 0), (1, 0, None, 1), (2, 5, 38, 1)]

    def run_select(ctx, d_in, d_out):
        o, n = capi.UnnafOpts(FASTA, 1, -1), C.c_size_t(1 << 40)
        sa = ctx._segments([(r, s, WHOLE if t is None else t) for r, s, t, _ in segs])
        st = (C.c_uint8 * len(segs))(*[rv for _, _, _, rv in segs])
        rc = ctx.L.naf_gpu_unnaf_select_stranded(ctx.h, _ptr(d_in), d_in.numel(), C.byref(o), sa, st, len(segs), _ptr(d_out), d_out.numel(), C.byref(n))
        return rc, (n.value,), n.value

    def ref_select(O, naf):
        t = SP.Records(O, naf, FASTA).expect(segs)
        return (len(t),), t
    P.append(Probe("unnaf_select_stranded", ["naf_gpu_unnaf_select_stranded"], naf_fa, bait_fa, len(ref_select(O, naf_fa)[1]), run_select, ref_select))

    R = SP.Records(O, naf_fa, FASTA)
    asked = [R.ids[2], b"no such id", R.ids[0], R.ids[R.n - 1]]

    def run_tables(ctx, d_in, d_out):
        blob = b"".join(i + b"\0" for i in asked)
        rec = (C.c_uint64 * len(asked))()
        rc = ctx.L.naf_gpu_unnaf_find(ctx.h, _ptr(d_in), d_in.numel(), blob, len(blob), len(asked), rec)
        if rc:
            return rc, (), 0
        o = capi.UnnafOpts(FASTA, 1, -1)
        nb, off = (C.c_uint64 * 3)(), (C.c_uint64 * 4)()
        rc = ctx.L.naf_gpu_unnaf_record_table(ctx.h, _ptr(d_in), d_in.numel(), C.byref(o), 1, 3, nb, off)
        return rc, (tuple(rec), tuple(nb), tuple(off)), 0

    def ref_tables(O, naf):
        R = SP.Records(O, naf, FASTA)
        first = {}
        for k, i in enumerate(R.ids):
            first.setdefault(i, k)
        starts = np.concatenate([[0], np.cumsum([len(w) for w in R.whole])])
        return (tuple(first.get(i, WHOLE) for i in asked), tuple(len(R.bases[r]) for r in (1, 2, 3)), tuple(int(starts[r]) for r in (1, 2, 3, 4))), b""
    P.append(Probe("unnaf_find_record_table", ["naf_gpu_unnaf_find", "naf_gpu_unnaf_record_table"], naf_fa, bait_fa, 0, run_tables, ref_tables))

    # ---- the scanners that write device rows
    def upper(O, naf):
        return [x.decode("latin1").upper() for x in _lines(O, naf)]
    pats = ["ACG", "GRT"]
    blob = b"".join(p.encode() + b"\0" for p in pats)

    def run_locate(ctx, d_in, d_out):
        n = C.c_uint64()
        rc = ctx.L.naf_gpu_unnaf_locate(ctx.h, _ptr(d_in), d_in.numel(), blob, len(blob), len(pats), 3, 0, WHOLE, _ptr(d_out), d_out.numel() // 24, C.byref(n))
        return rc, (n.value,), 24 * n.value

    def ref_locate(O, naf):
        rows = LP.expected_hits(upper(O, naf), pats, 3)
        return (len(rows),), _rows_bytes(rows, capi.HIT_DTYPE)
    P.append(Probe("unnaf_locate", ["naf_gpu_unnaf_locate"], naf_fa, bait_fa, len(ref_locate(O, naf_fa)[1]), run_locate, ref_locate))

    near = ["ACGTAC[GT]", "TTNAGGC"]
    nblob = b"".join(p.encode() + b"\0" for p in near)

    def run_near(ctx, d_in, d_out):
        n, bud = C.c_uint64(), (C.c_uint32 * 2)(1, 2)
        rc = ctx.L.naf_gpu_unnaf_locate_near(ctx.h, _ptr(d_in), d_in.numel(), nblob, len(nblob), len(near), bud, 3, 0, WHOLE, _ptr(d_out), d_out.numel() // 32, C.byref(n))
        return rc, (n.value,), 32 * n.value

    def ref_near(O, naf):
        rows = NP.near_hits(upper(O, naf), near, [1, 2], 3)
        return (len(rows),), _rows_bytes([tuple(int(v) for v in r) for r in rows], capi.NEAR_HIT_DTYPE)
    P.append(Probe("unnaf_locate_near", ["naf_gpu_unnaf_locate_near"], naf_fa, bait_fa, len(ref_near(O, naf_fa)[1]), run_near, ref_near))

    def run_comp(ctx, d_in, d_out):
        n, tot = C.c_uint64(), capi.CompRow()
        rc = ctx.L.naf_gpu_unnaf_composition(ctx.h, _ptr(d_in), d_in.numel(), 100, capi.COMP_MASK, 0, WHOLE, _ptr(d_out), d_out.numel() // 168, C.byref(n), C.byref(tot))
        return rc, (n.value, (tot.record, tot.begin, tot.end, list(tot.n), tot.masked, tot.cpg)), 168 * n.value

    def ref_comp(O, naf):
        lines = _lines(O, naf)
        rows = CP.expected_rows(lines, 100)
        return (len(rows), CP.expected_total(lines, rows)), rows.tobytes()
    P.append(Probe("unnaf_composition", ["naf_gpu_unnaf_composition"], naf_fa, bait_fa, len(ref_comp(O, naf_fa)[1]), run_comp, ref_comp))

    W = 16
    n_rec = O.parse_naf(naf_fq).n_sequences

    def run_quality(ctx, d_in, d_out):
        nr, nc, tot, hist = C.c_uint64(), C.c_uint64(), capi.QualRow(), (C.c_uint64 * 256)()
        rec, cyc = d_out[:56 * n_rec], d_out[56 * n_rec:]
        rc = ctx.L.naf_gpu_unnaf_quality(ctx.h, _ptr(d_in), d_in.numel(), W, 0, WHOLE, _ptr(rec), n_rec, _ptr(cyc), cyc.numel() // 56, C.byref(nr), C.byref(nc), hist, C.byref(tot))
        return rc, (nr.value, nc.value, [int(v) for v in hist], (tot.key, tot.n, tot.sum, tot.ee, tot.n_q20, tot.n_q30, tot.min, tot.max)), 56 * (n_rec + nc.value)

    def ref_quality(O, naf):
        q = QP.quals_of(O.unnaf(naf, FASTQ), O.parse_naf(naf).n_sequences)
        rec, cyc = QP.record_rows(q), QP.cycle_rows(q, W)
        return (len(rec), len(cyc), QP.hist_of(q), QP.total_of(q)), rec.tobytes() + cyc.tobytes()
    P.append(Probe("unnaf_quality", ["naf_gpu_unnaf_quality"], naf_fq, bait_fq, len(ref_quality(O, naf_fq)[1]), run_quality, ref_quality))

    acgt = RP.set_of("ACGT")

    def run_runs(ctx, d_in, d_out):
        n, nb = C.c_uint64(), C.c_uint64()
        rc = ctx.L.naf_gpu_unnaf_runs(ctx.h, _ptr(d_in), d_in.numel(), acgt, capi.RUNS_EACH, 3, 0, WHOLE, _ptr(d_out), d_out.numel() // 32, C.byref(n), C.byref(nb))
        return rc, (n.value, nb.value), 32 * n.value

    def ref_runs(O, naf):
        rows = RP.expected_runs(_lines(O, naf), acgt, True, 3)
        return (len(rows), int((rows["end"] - rows["begin"]).sum())), rows.tobytes()
    P.append(Probe("unnaf_runs", ["naf_gpu_unnaf_runs"], naf_fa, bait_fa, len(ref_runs(O, naf_fa)[1]), run_runs, ref_runs))

    K = 3
    n_fa = O.parse_naf(naf_fa).n_sequences

    def run_kmers(ctx, d_in, d_out):
        n, nc, tot = C.c_uint64(), C.c_uint64(), capi.KmerRow()
        counts, rows = d_out[:8 * n_fa * 4 ** K], d_out[8 * n_fa * 4 ** K:]
        rc = ctx.L.naf_gpu_unnaf_kmers(ctx.h, _ptr(d_in), d_in.numel(), K, capi.KMER_PER_RECORD, 0, WHOLE, _ptr(counts), counts.numel() // 8, _ptr(rows), rows.numel() // 40,
                                       C.byref(n), C.byref(nc), C.byref(tot))
        return rc, (n.value, nc.value, (tot.record, tot.begin, tot.end, tot.positions, tot.counted)), 8 * n_fa * 4 ** K + 40 * n.value

    def ref_kmers(O, naf):
        lines = _lines(O, naf)
        counts, rows = KP.expected_counts(lines, K, False, True), KP.expected_rows(lines, K)
        return (len(rows), counts.size, KP.expected_total(lines, K)), counts.tobytes() + rows.tobytes()
    P.append(Probe("unnaf_kmers", ["naf_gpu_unnaf_kmers"], naf_fa, bait_fa, len(ref_kmers(O, naf_fa)[1]), run_kmers, ref_kmers))

    stops, starts = OP.codon_set("TAA,TAG,TGA"), OP.codon_set("ATG")

    def run_orfs(ctx, d_in, d_out):
        n, nb = C.c_uint64(), C.c_uint64()
        rc = ctx.L.naf_gpu_unnaf_orfs(ctx.h, _ptr(d_in), d_in.numel(), stops, starts, 30, 3, 0, 0, WHOLE, _ptr(d_out), d_out.numel() // 32, C.byref(n), C.byref(nb))
        return rc, (n.value, nb.value), 32 * n.value

    def ref_orfs(O, naf):
        rows = OP.expected_rows(_lines(O, naf), stops, starts, 30)
        return (len(rows), int((rows["end"] - rows["begin"]).sum())), rows.tobytes()
    P.append(Probe("unnaf_orfs", ["naf_gpu_unnaf_orfs"], naf_fa, bait_fa, len(ref_orfs(O, naf_fa)[1]), run_orfs, ref_orfs))

    # ---- ennaf: one call with the sections beside each other, and the three-shard round with a shard's sections beside each other
    def run_ennaf(ctx, d_in, d_out):
        o = capi.EnnafOpts(capi.FMT_AUTO, 0, 0, 0, 1, -1, None, 0)
        n, rep = C.c_size_t(1 << 40), capi.EnnafReport()
        rc = ctx.L.naf_gpu_ennaf(ctx.h, _ptr(d_in), d_in.numel(), C.byref(o), _ptr(d_out), d_out.numel(), C.byref(n), C.byref(rep))
        return rc, (rep.n_sequences, rep.n_bases, rep.longest_line), n.value

    def ref_ennaf(O, text):
        sp = O.split_text(text)
        return (sp.n_sequences, sp.n_bases, sp.longest_line), _split(O, text)
    text_bait = _same_length_text_bait(text_fa)
    P.append(Probe("ennaf_overlap", ["naf_gpu_ennaf"], text_fa, text_bait, L.naf_gpu_ennaf_bound(len(text_fa)), run_ennaf, ref_ennaf, digest=_streams,
                   env={"NAF_GPU_ENC_OVERLAP": "2"}, side=True))

    def run_shards(ctx, d_in, d_out, others):
        """the round of test_gpu_buffers.py; others: two more contexts on the stream of ctx (or, each on a private one, waited for)"""
        from naf_amd import shard
        ctxs = [ctx] + list(others)
        opts = shard.make_opts()
        fmt, p0 = ctx.ennaf_sniff(d_in, opts.format)
        cuts = shard.cuts_local(ctx, d_in, fmt, p0, 3)
        slices = [d_in[cuts[k]:cuts[k + 1]] for k in range(3)]
        infos = [ctxs[k].ennaf_shard_begin(slices[k], opts, fmt, k, 3) for k in range(3)]
        bufs, pieces = [], []
        for k in range(3):
            buf, pc = ctxs[k].ennaf_shard_finish(opts, infos, slices[k].numel())
            bufs.append(buf); pieces.append(pc)
        segs, lit, naf_len, rep = capi.stitch_plan(opts, infos, pieces)
        if naf_len > d_out.numel():
            return capi.E_CAP, (), 0
        for c in others:
            if getattr(c, "private_stream", False):
                c.synchronize()
        ctx.ennaf_stitch(segs, lit, bufs, d_out[:naf_len])
        return 0, (rep.n_sequences, rep.n_bases, rep.longest_line), naf_len
    P.append(Probe("ennaf_shards", ["naf_gpu_ennaf_sniff", "naf_gpu_ennaf_find_cut", "naf_gpu_ennaf_shard_begin", "naf_gpu_ennaf_shard_finish", "naf_gpu_ennaf_stitch"],
                   text_fa, text_bait, L.naf_gpu_ennaf_bound(len(text_fa)), run_shards, ref_ennaf, digest=_streams, env={"NAF_GPU_SHARD_OVERLAP": "1"}, side=True, contexts=3))

    # ---- histogram, line starts
    def run_hist(ctx, d_in, d_out):
        cnt = (C.c_uint64 * 256)()
        rc = ctx.L.naf_gpu_histogram(ctx.h, _ptr(d_in), d_in.numel(), cnt)
        return rc, ([int(v) for v in cnt],), 0
    P.append(Probe("histogram", ["naf_gpu_histogram"], text_fa, bytes(x ^ 0x20 for x in text_fa), 0, run_hist,
                   lambda O, data: ((np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256).tolist(),), b"")))

    reads = synth.fastq_reads(1500, 120, seed=5)
    assert 200_000 < len(reads) < 600_000

    def run_lines(ctx, d_in, d_out):
        got = []
        for m in LINE_SLICES:
            for prev in (0, 1):
                v = d_in if m is None else d_in[:m]
                n = C.c_uint64(1 << 60)
                rc = ctx.L.naf_gpu_ennaf_count_lines(ctx.h, _ptr(v), v.numel(), prev, C.byref(n))
                if rc:
                    return rc, (), 0
                got.append(n.value)
        return 0, (got,), 0

    def ref_lines(O, data):
        return ([count_line_starts(data if m is None else data[:m], prev) for m in LINE_SLICES for prev in (0, 1)],), b""
    for name, text in (("count_lines_lf", reads), ("count_lines_crlf", reads.replace(b"\n", b"\r\n"))):
        a = np.frombuffer(text, dtype=np.uint8).copy()
        a[:len(a) // 2][np.isin(a[:len(a) // 2], EOL)] = 0x41          # the bait: the first half is one line
        P.append(Probe(name, ["naf_gpu_ennaf_count_lines"], text, a.tobytes(), 0, run_lines, ref_lines))
    return P


def companions(probe, stream):
    """The further contexts a probe needs: each on `stream` (a torch stream or None for the null stream), or with stream "private" on
    the stream it was born with."""
    from naf_amd import capi
    out = []
    for _ in range(probe.contexts - 1):
        c = capi.Context(0, use_torch_stream=False)
        c.private_stream = isinstance(stream, str)
        if not c.private_stream:
            c.set_stream(stream)
        out.append(c)
    return out


def call(probe, ctx, d_in, d_out, others=()):
    return probe.run(ctx, d_in, d_out, others) if probe.contexts > 1 else probe.run(ctx, d_in, d_out)


def buffers(probe, ctx, data=None):
    """(d_in, d_out) of a probe as plain torch tensors: the input (default: the real one) and an output of exactly the capacity."""
    import torch
    d_in = ctx.to_device(probe.real if data is None else data)
    d_out = torch.empty(max(probe.cap, 1), dtype=torch.uint8, device=ctx.device)[:probe.cap]
    return d_in, d_out


def run_ready(probe, ctx, oracle, stream="private"):
    """The probe on an input that is ready and host-synchronised: call, wait, judge.  stream: where the probe's further contexts run."""
    import torch
    d_in, d_out = buffers(probe, ctx)
    torch.cuda.synchronize()
    others = companions(probe, stream)
    try:
        rc, host, n = call(probe, ctx, d_in, d_out, others)
        for c in [ctx] + others:
            c.synchronize()
        probe.judge(oracle, rc, host, d_out[:n].cpu().numpy().tobytes())
    finally:
        for c in others:
            c.close()


def with_env(monkeypatch, probe):
    for k, v in probe.env.items():
        monkeypatch.setenv(k, v)


def tally_table(tally, modes):
    """The printed table: one line per probe, one column per mode, the calls made."""
    names = sorted({n for n, _ in tally})
    lines = ["%-26s" % "probe" + "".join("%8s" % m for m in modes)]
    for n in names:
        lines.append("%-26s" % n + "".join("%8d" % tally.get((n, m), 0) for m in modes))
    return "\n".join(lines)
