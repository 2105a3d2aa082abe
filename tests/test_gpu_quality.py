"""GPU tests of the quality statistics (naf_gpu_unnaf_quality_rows, naf_gpu_unnaf_quality, unnaf --quality).  Expected rows never come from
the code under test: they are what quality_plan gives -- numpy over the quality lines of the oracle's --fastq text of the same archive.
Every planned text is counted in the oracle's archive and, where the tolerant parser takes it (codes 33..126, no empty reads), in this
library's own ennaf at level 1; the reference-made golden archive repeat_fastq_l19 (a frame whose blocks depend on each other) takes the
whole-decode fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import quality_plan as QP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_FORMAT, E_CAP, E_ARG = -4, -6, -8
CASES = [c.name for c in QP.planned(0)]
GOLDEN = ("fastq_4k", "fastq_var", "repeat_fastq_l19")
TRACE = re.compile(r"\[quality\] records (\d+) cycle rows (\d+) pieces (\d+) quality bytes decoded (\d+) of (\d+) lds bins (\d+) global bins (\d+)\n")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


class Archive:
    def __init__(self, oracle, gpu, naf):
        self.naf = naf
        self.h = oracle.parse_naf(naf)
        N = self.h.n_sequences
        self.quals = QP.quals_of(oracle.unnaf(naf, oracle.MODE_FASTQ), N) if N else []
        self.d_naf = gpu.to_device(naf)
        self._want = {}

    def want(self, W, first=0, count=None):
        """(record rows, cycle rows, hist, total), computed once per question and left unchanged"""
        key = (W, first, count)
        if key not in self._want:
            rkey = (None, first, count)
            if rkey not in self._want:
                rec = QP.record_rows(self.quals, first, count)
                rec.setflags(write=False)
                self._want[rkey] = (rec, QP.hist_of(self.quals, first, count), QP.total_of(self.quals, first, count))
            rec, hist, total = self._want[rkey]
            cyc = QP.cycle_rows(self.quals, W, first, count) if W else np.zeros(0, dtype=QP.ROW_DTYPE)
            cyc.setflags(write=False)
            self._want[key] = (rec, cyc, hist, total)
        return self._want[key]


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive})"""
    out = {}
    for c in QP.planned(SEED):
        arc = {"oracle": Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type, well_formed=c.well_formed))}
        assert arc["oracle"].quals == c.quals, c.name
        if c.own_text is not None:
            own, _ = gpu.ennaf(gpu.to_device(c.own_text), seq_type=c.seq_type, level=1)
            arc["own"] = Archive(oracle, gpu, own.cpu().numpy().tobytes())
            assert arc["own"].quals == c.own_quals, c.name
        out[c.name] = (c, arc)
    return out


@pytest.fixture(scope="module")
def goldens(oracle, gpu):
    return {name: Archive(oracle, gpu, golden_bytes("naf", name + ".naf")) for name in GOLDEN}


def total_tuple(t):
    return (int(t.key), int(t.n), int(t.sum), int(t.ee), int(t.n_q20), int(t.n_q30), int(t.min), int(t.max))


def differ(what, got, want, where):
    if got.tobytes() != want.tobytes():
        k = next((i for i in range(min(len(got), len(want))) if got[i].tobytes() != want[i].tobytes()), min(len(got), len(want)))
        raise AssertionError("%s %s: first difference at row %d of %d / %d: got %s, expected %s" % (what, where, k, len(got), len(want), QP.as_tuples(got[k:k + 2]), QP.as_tuples(want[k:k + 2])))


def check(gpu, A, W, first=0, count=None, records=True, cycles=True):
    rec_w, cyc_w, hist_w, total_w = A.want(W, first, count)
    where = "W %d records %d+%s tables %d %d" % (W, first, count, records, cycles)
    rec, cyc, hist, total = gpu.unnaf_quality(A.d_naf, W, first, count, records=records, cycles=cycles)
    if records:
        differ("record rows", rec, rec_w, where)
    else:
        assert rec is None
    if cycles and W:
        differ("cycle rows", cyc, cyc_w, where)
    else:
        assert cyc is None
    assert hist == hist_w, where
    assert total_tuple(total) == total_w, where
    assert gpu.unnaf_quality_rows(A.d_naf, W, first, count) == (len(rec_w), len(cyc_w)), where
    return rec, cyc


# ---- 1. the rows of the planned texts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_rows_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    if which not in arc:
        assert name in ("allbytes", "no_records")
        return
    A = arc[which]
    n = 0
    for W in (0,) + c.widths:
        for records in (True, False):
            for cycles in (True, False):
                rec, cyc = check(gpu, A, W, 0, None, records, cycles)
                n += len(rec) if rec is not None else 0
    assert (n > 0) == (name != "no_records")


def traced(gpu, A, W, first, count, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    rec, cyc, hist, total = gpu.unnaf_quality(A.d_naf, W, first, count)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = TRACE.findall(err)
    assert len(m) == 1, err
    return rec, cyc, [int(x) for x in m[0]]


def test_the_long_text_lies_around_the_bins_kept_in_lds(gpu, planned, monkeypatch, capfd):
    c, arc = planned["long"]
    for which in ("oracle", "own"):
        A = arc[which]
        rec, cyc, (R, Cn, pieces, dec, of, K, G) = traced(gpu, A, 1, 0, None, monkeypatch, capfd)
        assert K == QP.LDS_BINS and K + 4096 < 70000 == Cn == K + G and R == len(A.quals)
        differ("cycle rows", cyc, A.want(1)[1], which)
        assert int(cyc[K - 1]["n"]) >= 3 and int(cyc[K]["n"]) >= 2 and int(cyc[K + 1]["n"]) == 1


# ---- 2. first and count ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
def test_first_and_count(gpu, planned, which):
    c, arc = planned["seams"]
    A = arc[which]
    N = len(A.quals)
    whole = A.want(0)[0]
    empty = [r for r in range(N) if not A.quals[r]]
    assert bool(empty) == (which == "oracle")
    runs = [(0, 1), (N - 1, 1), (3, 9), (5, 0), (N, 0), (N, None), (N // 2, None)] + [(r, 1) for r in empty[:2]] + ([(empty[0], 2)] if empty else [])
    for first, count in runs:
        for W in (1, 100, 4097):
            if W == 1 and (count is None or count > 1):
                W = 64
            rec, cyc = check(gpu, A, W, first, count)
            last = N if count is None else first + count
            assert rec.tobytes() == whole[first:last].tobytes()
            far = max([len(q) for q in A.quals[first:last]] + [0])
            assert len(cyc) == -(-far // W)                                         # the longest SELECTED read
    lens = [len(q) for q in A.quals]
    r = int(np.argmin([n if n else 1 << 30 for n in lens]))
    assert len(check(gpu, A, 1, r, 1)[1]) == lens[r] < max(lens)


# ---- 3. golden archives, and what is decoded ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN)
def test_rows_of_the_golden_archives(gpu, goldens, name, monkeypatch, capfd):
    A = goldens[name]
    for W in (1, 1000):
        rec, cyc = check(gpu, A, W)
        assert len(rec) > 0 and len(cyc) > 0
    if name == "repeat_fastq_l19":
        last = max(r for r in range(len(A.quals)) if A.quals[r])
        rec, cyc, tr = traced(gpu, A, 1000, last, 1, monkeypatch, capfd)
        differ("record rows", rec, A.want(1000, last, 1)[0], name)
        assert tr[3] == tr[4] == A.h.orig[5]                                        # dependent blocks: the whole stream, once


def test_a_restricted_count_decodes_only_the_blocks_behind_its_records(gpu, planned, monkeypatch, capfd):
    A = planned["seams"][1]["own"]
    last = len(A.quals) - 1
    rec, cyc, tr = traced(gpu, A, 100, last, 1, monkeypatch, capfd)
    differ("record rows", rec, A.want(100, last, 1)[0], "last")
    differ("cycle rows", cyc, A.want(100, last, 1)[1], "last")
    assert tr[0] == 1 and tr[2] == 1 and tr[3] < tr[4] == A.h.orig[5], tr
    rec, cyc, tr = traced(gpu, A, 100, 0, None, monkeypatch, capfd)
    assert tr[3] == tr[4]


# ---- 4. the piece size does not show --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [1, 1000, 70000])
def test_the_result_does_not_depend_on_the_piece_size(gpu, planned, goldens, piece, monkeypatch, capfd):
    gpu.set_option("QUALITY_PIECE", piece)
    try:
        for name, widths in (("seams", (1, 100, 4097)), ("long", (1, 64)), ("short", (1, 65)), ("allbytes", (2,))):
            if name == "short" and piece == 1:
                continue                                                            # (3000 pieces of one read each: seams and long cover piece = 1)
            c, arc = planned[name]
            for which in arc:
                for W in widths:
                    check(gpu, arc[which], W)
                N = len(arc[which].quals)
                check(gpu, arc[which], widths[-1], min(2, N - 1), min(5, N - min(2, N - 1)))
        A = planned["seams"][1]["own"]
        rec, cyc, tr = traced(gpu, A, 100, 0, None, monkeypatch, capfd)
        differ("cycle rows", cyc, A.want(100)[1], "pieces")
        assert tr[2] > 1                                                            # it was counted in pieces
        check(gpu, goldens["repeat_fastq_l19"], 1000)
    finally:
        gpu.set_option("QUALITY_PIECE", None)


@pytest.mark.parametrize("grid,flush", [(1, 1), (3, 2), (2, 1024)])
def test_the_result_does_not_depend_on_the_grid_or_on_the_flushes(gpu, planned, grid, flush):
    """Few workgroups: each loops over many tiles; QUALITY_FLUSH: its LDS bins and histogram are flushed between the rounds."""
    gpu.set_option("QUALITY_GRID", grid)
    gpu.set_option("QUALITY_FLUSH", flush)
    try:
        for name, widths in (("seams", (1, 100, 1 << 40)), ("long", (1, 64)), ("short", (1, 65))):
            for which, A in planned[name][1].items():
                for W in widths:
                    check(gpu, A, W)
                check(gpu, A, 0, 1, 7, records=False)
    finally:
        gpu.set_option("QUALITY_GRID", None)
        gpu.set_option("QUALITY_FLUSH", None)


# ---- 5. buffers -------------------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, W, first, count, d_rec, rec_cap, d_cyc, cyc_cap, hist=True, total=True):
    from naf_amd import capi
    nr, nc, tot, h = C.c_uint64(12345), C.c_uint64(54321), capi.QualRow(), (C.c_uint64 * 256)()

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None
    rc = gpu.L.naf_gpu_unnaf_quality(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), W, first, capi.WHOLE if count is None else count, ptr(d_rec), rec_cap,
                                     ptr(d_cyc), cyc_cap, C.byref(nr), C.byref(nc), h if hist else None, C.byref(tot) if total else None)
    return rc, nr.value, nc.value, [int(v) for v in h], tot


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    arena = fenced.Arena("cuda", salt=0x51, size=8 << 20)
    for name, W in (("short", 1), ("seams", 100), ("long", 4097)):
        A = planned[name][1][which]
        rec_w, cyc_w, hist_w, total_w = A.want(W)
        nr, nc = len(rec_w), len(cyc_w)
        assert nr >= 2 and nc >= 2
        for phase in range(8):
            # exactly enough: 56 rows bytes of each table and nothing outside them
            arena.reset()
            d_rec, d_cyc = arena.out(56 * nr, phase), arena.out(56 * nc, (phase * 3 + 1) % 8)
            rc, gr, gc, hist, tot = raw(gpu, A.d_naf, W, 0, None, d_rec, nr, d_cyc, nc, hist=phase % 2 == 0, total=phase % 3 == 0)
            torch.cuda.synchronize()
            assert rc == 0 and (gr, gc) == (nr, nc)
            arena.check()
            assert d_rec.cpu().numpy().tobytes() == rec_w.tobytes() and d_cyc.cpu().numpy().tobytes() == cyc_w.tobytes(), (name, phase)
            assert hist == (hist_w if phase % 2 == 0 else [0] * 256)
            assert phase % 3 or total_tuple(tot) == total_w
        # one row too few on either table: both whole counts, and nothing written to either
        for short_rec, short_cyc in ((1, 0), (0, 1)):
            arena.reset()
            d_rec, d_cyc = arena.out(56 * (nr - short_rec), 5), arena.out(56 * (nc - short_cyc), 3)
            b_rec, b_cyc = d_rec.clone(), d_cyc.clone()
            rc, gr, gc, _, _ = raw(gpu, A.d_naf, W, 0, None, d_rec, nr - short_rec, d_cyc, nc - short_cyc)
            torch.cuda.synchronize()
            assert rc == E_CAP and (gr, gc) == (nr, nc) and torch.equal(d_rec, b_rec) and torch.equal(d_cyc, b_cyc)
            arena.check()
            assert "rows" in gpu.L.naf_gpu_last_error(gpu.h).decode()
        # a table that is not wanted has no capacity to be short of
        arena.reset()
        d_cyc = arena.out(56 * nc, 4)
        rc, gr, gc, _, _ = raw(gpu, A.d_naf, W, 0, None, None, 0, d_cyc, nc)
        torch.cuda.synchronize()
        assert rc == 0 and (gr, gc) == (nr, nc) and d_cyc.cpu().numpy().tobytes() == cyc_w.tobytes()
        arena.check()
    # the archive in an arena, other bytes around it: the same rows
    A = planned["short"][1][which]
    rec_w, cyc_w, _, _ = A.want(65)
    for run, in_phase in ((0, 0), (1, 1), (0, 65)):
        arena.reset()
        before, after = fenced.stream_bait(A.naf, run)
        d_in = arena.put(A.naf, in_phase, before, after)
        d_rec, d_cyc = arena.out(56 * len(rec_w), 16), arena.out(56 * len(cyc_w), 9)
        rc, gr, gc, _, _ = raw(gpu, d_in, 65, 0, None, d_rec, len(rec_w), d_cyc, len(cyc_w))
        torch.cuda.synchronize()
        assert rc == 0 and d_rec.cpu().numpy().tobytes() == rec_w.tobytes() and d_cyc.cpu().numpy().tobytes() == cyc_w.tobytes()
        arena.check()
    # the binding's own form with the caller's buffers
    from naf_amd import capi
    b_rec = torch.zeros(56 * len(rec_w) + 56, dtype=torch.uint8, device="cuda")
    b_cyc = torch.zeros(56 * len(cyc_w), dtype=torch.uint8, device="cuda")
    v_rec, v_cyc, hist, tot = gpu.unnaf_quality(A.d_naf, 65, out_records=b_rec, out_cycles=b_cyc)
    assert v_rec.numel() == 56 * len(rec_w) and not bool(b_rec[56 * len(rec_w):].any()) and v_rec.cpu().numpy().tobytes() == rec_w.tobytes()
    assert v_cyc.cpu().numpy().tobytes() == cyc_w.tobytes()
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_quality(A.d_naf, 65, out_records=b_rec, out_cycles=b_cyc[:56 * (len(cyc_w) - 1)])
    assert e.value.code == E_CAP


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    import torch
    from naf_amd import capi
    A = planned["short"][1]["own"]
    N = A.h.n_sequences

    def fails(d_naf, code, first=0, count=None, words=()):
        b_rec, b_cyc = torch.zeros(56 * 64, dtype=torch.uint8, device="cuda"), torch.zeros(56 * 64, dtype=torch.uint8, device="cuda")
        rc, nr, nc, hist, tot = raw(gpu, d_naf, 10, first, count, b_rec, 64, b_cyc, 64)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == code and (nr, nc) == (0, 0) and not bool(b_rec.any()) and not bool(b_cyc.any()) and not any(hist), (rc, msg)
        for w in words:
            assert w in msg, msg
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_quality_rows(d_naf, 10, first, count)
        assert e.value.code == code and all(w in e.value.msg for w in words)

    fails(A.d_naf, E_ARG, first=N + 1, words=("record", str(N + 1)))
    fails(A.d_naf, E_ARG, first=1, count=N, words=("records", str(N)))
    for name in ("acgt_10k", "protein_small"):
        fails(gpu.to_device(golden_bytes("naf", name + ".naf")), E_ARG, words=("no quality",))
    fails(gpu.to_device(short_quality_archive(oracle)), E_FORMAT, words=("corrupted quality",))


def short_quality_archive(oracle):
    """An archive whose quality section is three codes shorter than its bases: the oracle's archive of a small FASTQ with its last
    section -- the quality: its two sizes, then its frame without the magic -- written again from fewer bytes."""
    naf = oracle.ennaf(b"@a x\nACGTAC\n+\nIIIIII\n@b\nACGT\n+\n5555\n")
    h = oracle.parse_naf(naf)
    assert h.flags & 1 and h.orig[5] == 10 == h.orig[4]
    start = h.payload_off[5] - len(vle(oracle, h.orig[5])) - len(vle(oracle, h.comp[5]))
    assert h.payload_off[5] + h.comp[5] == len(naf) and naf[start:h.payload_off[5]] == vle(oracle, h.orig[5]) + vle(oracle, h.comp[5])
    frame = oracle.zstd_store_raw(b"IIIIII5")
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    out = naf[:start] + vle(oracle, 7) + vle(oracle, len(frame) - 4) + frame[4:]
    h2 = oracle.parse_naf(out)
    assert h2.n_sequences == 2 and h2.orig[5] == 7 and h2.orig[4] == 10 and oracle.zstd_decompress(h2.frame(out, 5)) == b"IIIIII5"
    return out


def vle(oracle, v):
    buf = C.create_string_buffer(16)
    n = oracle.lib().nafo_vle_write(v, buf)
    return buf.raw[:n]


# ---- 7. the same bytes on every run ---------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(gpu, planned):
    from naf_amd import capi
    for name, W in (("seams", 100), ("short", 1), ("long", 1)):
        A = planned[name][1]["own"]
        a = gpu.unnaf_quality(A.d_naf, W)
        gpu.unnaf(planned["short"][1]["oracle"].d_naf, capi.OUT_FASTQ)              # an unrelated call on the same context in between
        b = gpu.unnaf_quality(A.d_naf, W)
        want = A.want(W)
        assert a[0].tobytes() == b[0].tobytes() == want[0].tobytes() and a[1].tobytes() == b[1].tobytes() == want[1].tobytes()
        assert a[2] == b[2] == want[2] and total_tuple(a[3]) == total_tuple(b[3]) == want[3]


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_quality_writes_the_tables(gpu, oracle, planned):
    A = planned["long"][1]["own"]
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    assert len(ids) == A.h.n_sequences
    far = QP.longest(A.quals)
    p = unnaf_cli(["--quality"], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == QP.table(A.want(0)[0], ids)
    assert p.stdout.count(b"\n") == 1 + len(A.quals)
    p = unnaf_cli(["--quality", "--cycles", "1"], A.naf)
    assert p.returncode == 0 and p.stdout == QP.cycle_table(A.want(1)[1], 1, far) and p.stdout.count(b"\n") == 1 + far
    p = unnaf_cli(["--quality", "--cycles", "4,097"], A.naf)
    assert p.returncode == 0 and p.stdout == QP.cycle_table(A.want(4097)[1], 4097, far)
    assert p.stdout.split(b"\n")[-2].split(b"\t")[1] == b"%d" % far                  # the last bin is cut at the longest read
    p = unnaf_cli(["--quality", "--records", "2-4"], A.naf)
    assert p.returncode == 0 and p.stdout == QP.table(A.want(0, 1, 3)[0], ids)
    p = unnaf_cli(["--quality", "--cycles", "100", "--records", "4-6"], A.naf)
    assert p.returncode == 0 and p.stdout == QP.cycle_table(A.want(100, 3, 3)[1], 100, QP.longest(A.quals, 3, 3))
    r = 5
    p = unnaf_cli(["--quality", "--region", ids[r]], A.naf)
    assert p.returncode == 0 and p.stdout == QP.table(A.want(0, r, 1)[0], ids)
    for args in (["--quality", "--region", "nosuch"], ["--quality", "--records", "1-99"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    p = unnaf_cli(["--quality"], golden_bytes("naf", "acgt_10k.naf"))
    assert p.returncode == 1 and b"no quality" in p.stderr and p.stdout == b""
    A = planned["allbytes"][1]["oracle"]                                              # an empty read: NA
    p = unnaf_cli(["--quality"], A.naf)
    names = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    assert p.returncode == 0 and p.stdout == QP.table(A.want(0)[0], names) and b"\t0\tNA\tNA\tNA\t0\t0\t0.000000\n" in p.stdout
