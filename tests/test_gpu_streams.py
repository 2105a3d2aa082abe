"""Stream order: what include/naf_gpu.h and INTEGRATION.md section 5 promise about the stream a context runs on.

Every probe of ctx_plan.py runs three ways: (a) on a context bound to torch's default stream with an input that a late producer on
that stream writes -- a delay of about 50 ms, then the copy of the real input over a bait, no host wait -- and with a copy of the
output enqueued on the same stream directly behind the call; (b) the same on a context constructed under a fresh torch.cuda.Stream,
producer and consumer on that stream, the null stream idle; (c) on the context's private stream with a ready input.  The entry points
documented as asynchronous (copy, upload, download_async, gather_ranges) must in addition return while the producer is still pending,
and write_file / write_fd must write what the producer made.  One live context is moved from stream to stream.  The judge is the
probe's reference (the oracle, a *_plan.py brute force, numpy) or the bytes the test wrote, never a second call of the library.

Known limit.  Most calls begin with a read-back on the context's stream (the header, a size), so the late producer sharpens only the
first device read of a call and the asynchronous entry points; everything behind that first read is ordered by the read-back's wait.
The rest of this module pins results on streams other than the null stream.  With four hardware queues two streams can share a queue
and be ordered by accident: that can hide a missing wait, it cannot make a correct library fail.  No queue setting is touched."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import ctx_plan as X

pytestmark = pytest.mark.gpu
MODES = ("a", "b", "c")


@pytest.fixture(scope="module")
def table(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield X.by_name(oracle)
    X.report(MODES + ("switch",))


@pytest.fixture(scope="module")
def delay(table):
    d = X.Delay(50.0)
    print("\nlate producer: %.1f ms (%s)" % (d.ms, "torch.cuda._sleep" if d.spin else "%d device copies" % d.copies))
    assert d.ms >= 20.0, d.ms
    return d


@pytest.fixture(scope="module")
def on_default(table):
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def on_fresh(table):
    import torch
    from naf_amd import capi
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        ctx = capi.Context(0)
    yield ctx, S
    ctx.close()


@pytest.fixture(scope="module")
def private(table):
    from naf_amd import capi
    ctx = capi.Context(0, use_torch_stream=False)
    yield ctx
    ctx.close()


def host(t):
    return t.cpu().numpy().tobytes()


def late_run(probe, oracle, ctx, stream, delay, idle=None):
    """(a) and (b): bait in place, producer pending, the call, the consumer's copy behind it, one synchronise, the judgement."""
    import torch
    with torch.cuda.stream(stream):
        buf, real = ctx.to_device(probe.bait), ctx.to_device(probe.real)
        d_out = torch.empty(max(probe.cap, 1), dtype=torch.uint8, device=ctx.device)[:probe.cap]
    torch.cuda.synchronize()
    others = X.companions(probe, stream)
    try:
        X.late(stream, buf, real, delay)
        assert not stream.query(), "the producer was to be pending when the call is made"
        with torch.cuda.stream(stream):
            rc, hres, n = X.call(probe, ctx, buf, d_out, others)
            keep = d_out.clone()                                       # the consumer: enqueued with no host wait in between
        assert idle is None or idle.query(), "the null stream was given work"
        torch.cuda.synchronize()
        probe.judge(oracle, rc, hres, host(keep[:n]))
    finally:
        for c in others:
            c.close()


@pytest.mark.parametrize("name", X.NAMES)
def test_a_default_stream_late_input(name, oracle, table, on_default, delay, monkeypatch):
    import torch
    X.with_env(monkeypatch, table[name])
    late_run(table[name], oracle, on_default, torch.cuda.current_stream(), delay)
    X.count(name, "a", table[name].entries)


@pytest.mark.parametrize("name", X.NAMES)
def test_b_fresh_stream_late_input(name, oracle, table, on_fresh, delay, monkeypatch):
    import torch
    ctx, S = on_fresh
    X.with_env(monkeypatch, table[name])
    late_run(table[name], oracle, ctx, S, delay, idle=torch.cuda.default_stream())
    X.count(name, "b", table[name].entries)


@pytest.mark.parametrize("name", X.NAMES)
def test_c_private_stream(name, oracle, table, private, monkeypatch):
    X.with_env(monkeypatch, table[name])
    X.run_ready(table[name], private, oracle, "private")
    X.count(name, "c", table[name].entries)


@pytest.mark.parametrize("name", X.SIDE_NAMES)
def test_the_side_streams_ran(name, oracle, table, monkeypatch):
    """The probes that are in the table for their side chains: kernel time was measured on a stream of the context besides the caller's."""
    import torch
    from naf_amd import capi
    assert table[name].side
    X.with_env(monkeypatch, table[name])
    ctx = capi.Context(0)
    try:
        ctx.set_timing(True)
        X.run_ready(table[name], ctx, oracle, torch.cuda.current_stream())
        names = [n for n, _, _ in ctx.get_timing()]
        ms = ctx.get_timing_streams()
        print("\n%s: kernel ms per stream %s" % (name, ["%.3f" % v for v in ms]))
        assert ms[0] > 0 and sum(ms[1:]) > 0 and any(n.startswith("side:") for n in names), (ms, names)
        if name == "unnaf_fastq":
            assert ms[2] > 0, ms                                       # the quality stream on the third context
    finally:
        ctx.close()


# ---- the asynchronous entry points ------------------------------------------------------------------------------------------------
N_ASYNC = (1 << 20) + 1


def stream_of(kind, on_default, on_fresh):
    import torch
    return (on_default, torch.cuda.current_stream()) if kind == "default" else on_fresh


def late_source(ctx, stream, delay, n=N_ASYNC, phase=1):
    """A device buffer at an odd address that holds a bait now and the pattern once the producer on `stream` has run; and the pattern."""
    import torch
    want = X.pattern(n, 0, 0xD1)
    with torch.cuda.stream(stream):
        buf = torch.from_numpy(X.pattern(n + phase, 7, 0x2E)).to(ctx.device)[phase:]
        real = torch.from_numpy(want).to(ctx.device)
    torch.cuda.synchronize()
    X.late(stream, buf, real, delay)
    assert not stream.query()
    return buf, want


def host_view(addr, n):
    return np.ctypeslib.as_array((C.c_uint8 * n).from_address(addr))


@pytest.mark.parametrize("kind", ["default", "fresh"])
def test_copy_returns_at_once_and_runs_in_order(kind, on_default, on_fresh, delay):
    import torch
    ctx, S = stream_of(kind, on_default, on_fresh)
    src, want = late_source(ctx, S, delay)
    dst = torch.zeros(N_ASYNC + 3, dtype=torch.uint8, device=ctx.device)[3:]
    ctx.copy(dst, src, N_ASYNC)
    assert not S.query(), "naf_gpu_copy waited for the stream"
    ctx.synchronize()
    assert X.pattern_diff(host(dst), N_ASYNC, 0, 0xD1) is None
    X.count("copy", kind, ["naf_gpu_copy", "naf_gpu_synchronize"])


@pytest.mark.parametrize("kind", ["default", "fresh"])
def test_download_async_returns_at_once_and_runs_in_order(kind, on_default, on_fresh, delay):
    ctx, S = stream_of(kind, on_default, on_fresh)
    h = ctx.host_alloc(N_ASYNC)
    try:
        host_view(h, N_ASYNC)[:] = 0
        src, want = late_source(ctx, S, delay)
        ctx.download_async(h, src, N_ASYNC)
        assert not S.query(), "naf_gpu_download_async waited for the stream"
        ctx.synchronize()
        assert X.pattern_diff(host_view(h, N_ASYNC).copy(), N_ASYNC, 0, 0xD1) is None
    finally:
        ctx.host_free(h)
    X.count("download_async", kind, ["naf_gpu_download_async", "naf_gpu_host_alloc", "naf_gpu_host_free", "naf_gpu_synchronize"])


@pytest.mark.parametrize("kind", ["default", "fresh"])
def test_upload_returns_at_once_and_lands_behind_what_was_queued(kind, on_default, on_fresh, delay):
    """The late producer writes the DESTINATION: an upload that ran ahead of the stream would be overwritten by it."""
    import torch
    ctx, S = stream_of(kind, on_default, on_fresh)
    h = ctx.host_alloc(N_ASYNC)
    try:
        host_view(h, N_ASYNC)[:] = X.pattern(N_ASYNC, 0, 0xD1)
        with torch.cuda.stream(S):
            dst = torch.zeros(N_ASYNC + 1, dtype=torch.uint8, device=ctx.device)[1:]
            other = torch.from_numpy(X.pattern(N_ASYNC, 7, 0x2E)).to(ctx.device)
        torch.cuda.synchronize()
        X.late(S, dst, other, delay)
        assert not S.query()
        ctx.upload(dst, h, N_ASYNC)
        assert not S.query(), "naf_gpu_upload waited for the stream"
        ctx.synchronize()
        assert X.pattern_diff(host(dst), N_ASYNC, 0, 0xD1) is None
    finally:
        ctx.host_free(h)
    X.count("upload", kind, ["naf_gpu_upload", "naf_gpu_host_alloc", "naf_gpu_host_free", "naf_gpu_synchronize"])


@pytest.mark.parametrize("kind", ["default", "fresh"])
def test_gather_ranges_the_root_waits_for_a_late_source(kind, on_default, on_fresh, delay):
    """Two contexts on two streams of the one device: the producer is on the SOURCE's stream, the consumer's copy on the ROOT's.  A root
    that did not wait for the source's event would hand the consumer the bait."""
    import torch
    from naf_amd import capi
    root, S_root = stream_of(kind, on_default, on_fresh)
    S_src = torch.cuda.Stream()
    with torch.cuda.stream(S_src):
        src_ctx = capi.Context(0)
    try:
        n1, n2 = 4099, 1001
        own = torch.from_numpy(X.pattern(n2, 0, 0x11)).to(root.device)
        total = 1 + n1 + 2 + n2 + 3
        with torch.cuda.stream(S_root):
            out = torch.zeros(total + 1, dtype=torch.uint8, device=root.device)[1:]
        src, want = late_source(src_ctx, S_src, delay, n1)
        root.gather_ranges(out, [(src_ctx, src, 1), (root, own, 3 + n1)])         # one range to an odd offset of an odd address
        with torch.cuda.stream(S_root):
            keep = out.clone()
        assert not S_src.query(), "naf_gpu_gather_ranges waited for the source's stream"
        root.synchronize()
        got = np.frombuffer(host(keep), dtype=np.uint8)
        assert X.pattern_diff(got[1:1 + n1], n1, 0, 0xD1) is None, "the root's stream did not wait for the source"
        assert X.pattern_diff(got[3 + n1:3 + n1 + n2], n2, 0, 0x11) is None
        assert not got[0] and not got[1 + n1:3 + n1].any() and not got[3 + n1 + n2:].any()
        torch.cuda.synchronize()
    finally:
        src_ctx.close()
    X.count("gather_ranges", kind, ["naf_gpu_gather_ranges", "naf_gpu_synchronize"])


@pytest.mark.parametrize("kind", ["default", "fresh"])
def test_write_file_and_write_fd_behind_a_late_producer(kind, on_default, on_fresh, delay, tmp_path):
    ctx, S = stream_of(kind, on_default, on_fresh)
    src, want = late_source(ctx, S, delay)
    path = str(tmp_path / "late.bin")
    fd = os.open(path, os.O_RDWR | os.O_CREAT, 0o600)
    try:
        ctx.write_file(fd, 0, src)
    finally:
        os.close(fd)
    with open(path, "rb") as f:
        assert X.pattern_diff(f.read(), N_ASYNC, 0, 0xD1) is None
    src, want = late_source(ctx, S, delay)
    r, w = os.pipe()
    got = bytearray()

    def drain():
        while True:
            b = os.read(r, 1 << 20)
            if not b:
                return
            got.extend(b)
    t = threading.Thread(target=drain)
    t.start()
    try:
        ctx.write_fd(w, src)
    finally:
        os.close(w)
        t.join()
        os.close(r)
    assert X.pattern_diff(bytes(got), N_ASYNC, 0, 0xD1) is None
    X.count("write_file/write_fd", kind, ["naf_gpu_write_file", "naf_gpu_write_fd"])


# ---- one live context from stream to stream ---------------------------------------------------------------------------------------
def test_one_context_moves_from_stream_to_stream(oracle, table, delay, monkeypatch):
    """private -> S1 -> S2 -> NULL through naf_gpu_set_stream, a probe with a late input after each move; after close() the caller's
    streams still work: the context has not destroyed what it did not own."""
    import torch
    from naf_amd import capi
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    null = torch.cuda.default_stream()
    assert null.cuda_stream == 0
    ctx = capi.Context(0, use_torch_stream=False)
    try:
        for stream, names in ((S1, ("unnaf_fasta", "histogram")), (S2, ("unnaf_fastq", "unnaf_runs")), (null, ("unnaf_fasta", "zstd_decompress", "ennaf_overlap"))):
            ctx.set_stream(None if stream is null else stream)
            for name in names:
                with monkeypatch.context() as m:
                    X.with_env(m, table[name])
                    late_run(table[name], oracle, ctx, stream, delay)
                X.count(name, "switch", table[name].entries + ("naf_gpu_set_stream",))
    finally:
        ctx.close()
    for stream in (S1, S2, null):
        with torch.cuda.stream(stream):
            a = torch.arange(4096, dtype=torch.int32, device="cuda")
            b = a.clone()
        stream.synchronize()
        assert torch.equal(a.cpu(), b.cpu())
    torch.cuda.synchronize()
