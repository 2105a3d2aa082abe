"""File <-> HBM (naf_amd/csrc/io.hip) at its chunk, lane, slot and ring seams, and the host <-> device copies of the C-ABI.

Files hold ctx_plan.pattern, which differs at every power-of-two shift, so a chunk that lands 4 MiB off, two swapped chunks, a chunk
written twice and a short tail all show; device buffers sit in a fenced arena (tests/fenced.py) at phases 0, 1 and 65 and the fences
are checked after every call.  read_file in its small mode cuts 4 MiB chunks, a lane per 64 MiB, two slots a lane; write_file cuts
16 MiB chunks on one lane; write_fd keeps three of four 8 MiB ring buffers in flight; a lane's pinned buffers are allocated again when
a later transfer needs larger ones.  IO_THREADS is read when a context's pool is first made: the tests that set it use a fresh context.
The judge is the pattern the test itself wrote."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import ctx_plan as X
from fenced import Arena

pytestmark = pytest.mark.gpu
MIB = 1 << 20
PHASES = (0, 1, 65)
FILE_SALT, DEV_SALT, OLD_SALT = 0x77, 0xD1, 0x2E
BIG = 128 * MIB + 5
E_ARG = -8


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()
    X.report(())


def called(entry, n=1):
    X.ENTRIES[entry] = X.ENTRIES.get(entry, 0) + n


@pytest.fixture(scope="module")
def arenas(gpu):
    """arena(n): one that holds a buffer of n bytes -- a small one for most transfers, a large one made when a test first needs it"""
    made = {}

    def arena(n):
        size = 40 * MIB if n <= 33 * MIB else BIG + 4 * MIB
        if size not in made:
            made[size] = Arena("cuda", 0x3C, size)
        made[size].reset()
        return made[size]
    return arena


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    """a file of the pattern, long enough for every read at either offset"""
    path = str(tmp_path_factory.mktemp("io") / "pattern.bin")
    with open(path, "wb") as f:
        f.write(pat(BIG + 4097 + 3, 0, FILE_SALT).tobytes())
    fd = os.open(path, os.O_RDONLY)
    yield fd
    os.close(fd)


def host(t):
    return t.cpu().numpy()


_HOST, _DEV = {}, {}


def pat(n, off, salt):
    """bytes [off, off + n) of the pattern of a salt, cut from one copy that is made once"""
    if salt not in _HOST or len(_HOST[salt]) < off + n:
        _HOST[salt] = X.pattern(max(off + n, BIG + 4097 + 3 if salt == FILE_SALT else 41 * MIB), 0, salt)
        _HOST[salt].setflags(write=False)
        _DEV.pop(salt, None)
    return _HOST[salt][off:off + n]


def dev_pat(n, off, salt):
    import torch
    pat(n, off, salt)
    if salt not in _DEV:
        _DEV[salt] = torch.from_numpy(_HOST[salt].copy()).cuda()
    return _DEV[salt][off:off + n]


def same(got, n, off, salt, what=""):
    """host bytes are bytes [off, off + n) of the pattern; pattern_diff names the damage"""
    got = np.frombuffer(bytes(got), dtype=np.uint8) if not isinstance(got, np.ndarray) else got
    if not (len(got) == n and np.array_equal(got, pat(n, off, salt))):
        raise AssertionError(what + X.pattern_diff(got, n, off, salt))


def holds(t, n, off, salt):
    """the device bytes are bytes [off, off + n) of the pattern (compared on the device; the host names the damage)"""
    import torch
    if not (t.numel() == n and torch.equal(t, dev_pat(n, off, salt))):
        raise AssertionError(X.pattern_diff(host(t), n, off, salt))


def read_and_check(ctx, A, fd, n, off, phase):
    import torch
    d = A.out(n, phase)
    ctx.read_file(fd, off, d)
    torch.cuda.synchronize()
    A.check()
    holds(d, n, off, FILE_SALT)
    called("naf_gpu_read_file")


# ---- read_file -------------------------------------------------------------------------------------------------------------------
# one chunk and its edges; one lane whose first slot is used a second time; two lanes; three lanes and many rounds
@pytest.mark.parametrize("n", (0, 1, 4 * MIB - 1, 4 * MIB, 4 * MIB + 1, 12 * MIB + 1, 64 * MIB, BIG))
def test_read_file(gpu, arenas, source, n):
    for off in (0, 4097):
        for phase in PHASES:
            read_and_check(gpu, arenas(n), source, n, off, phase)


def test_read_file_with_one_thread(arenas, source, monkeypatch):
    from naf_amd import capi
    monkeypatch.setenv("NAF_GPU_IO_THREADS", "1")
    ctx = capi.Context(0)
    try:
        for off, phase in ((0, 1), (4097, 65)):
            read_and_check(ctx, arenas(BIG), source, BIG, off, phase)
    finally:
        ctx.close()


def test_read_file_in_16_mib_chunks(arenas, source, monkeypatch):
    from naf_amd import capi
    monkeypatch.setenv("NAF_GPU_IO_SMALL", "0")
    ctx = capi.Context(0)
    try:
        for off in (0, 4097):
            for phase in PHASES:
                read_and_check(ctx, arenas(33 * MIB), source, 33 * MIB, off, phase)       # three chunks: a slot used twice, a short last one
    finally:
        ctx.close()


def test_read_file_of_a_file_that_is_too_short(gpu, arenas, tmp_path):
    import torch
    from naf_amd.capi import NafGpuError
    path = str(tmp_path / "short.bin")
    n = 5 * MIB
    with open(path, "wb") as f:
        f.write(pat(n, 0, FILE_SALT).tobytes())
    fd = os.open(path, os.O_RDONLY)
    try:
        A = arenas(n + 7)
        d = A.out(n + 7, 1)
        with pytest.raises(NafGpuError) as ei:
            gpu.read_file(fd, 0, d)
        assert ei.value.code == E_ARG and "can't read the input" in str(ei.value), str(ei.value)
        torch.cuda.synchronize()
        A.check()
        called("naf_gpu_read_file")
        for phase in PHASES:
            read_and_check(gpu, arenas(n), fd, n, 0, phase)
    finally:
        os.close(fd)


# ---- write_file ------------------------------------------------------------------------------------------------------------------
def device_pattern(A, n, phase):
    return A.put(dev_pat(n, 0, DEV_SALT), phase)


@pytest.mark.parametrize("n", (0, 1, 16 * MIB - 1, 16 * MIB, 16 * MIB + 1, 32 * MIB + 1))
def test_write_file(gpu, arenas, tmp_path, n):
    import torch
    path = str(tmp_path / "out.bin")
    old_len = n + 4097 + 1000 if n % 2 else n // 2                     # a file longer than what is written, and a shorter one that grows
    for off in (0, 4097):
        for phase in PHASES:
            with open(path, "wb") as f:
                f.write(pat(old_len, 0, OLD_SALT).tobytes())
            A = arenas(n)
            d = device_pattern(A, n, phase)
            fd = os.open(path, os.O_RDWR)
            try:
                gpu.write_file(fd, off, d)
            finally:
                os.close(fd)
            torch.cuda.synchronize()
            A.check()
            called("naf_gpu_write_file")
            with open(path, "rb") as f:
                got = np.frombuffer(f.read(), dtype=np.uint8)
            want_len = max(old_len, off + n) if n else old_len
            assert len(got) == want_len, (len(got), want_len)
            same(got[off:off + n], n, 0, DEV_SALT)
            head = min(off, old_len)
            same(got[:head], head, 0, OLD_SALT, "bytes in front of the range changed: ")
            if off > old_len:
                assert not got[old_len:off].any()                      # (the hole of a file that grew past its end)
            if old_len > off + n:
                same(got[off + n:], old_len - off - n, off + n, OLD_SALT, "bytes behind the range changed: ")


# ---- write_fd ----------------------------------------------------------------------------------------------------------------------
def through_pipe(ctx, d):
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
        ctx.write_fd(w, d)
    finally:
        os.close(w)
        t.join()
        os.close(r)
    return bytes(got)


# one chunk and its edges; three chunks (all in flight at once); 32 MiB + 1: the first reuse of a ring buffer; 40 MiB + 3
@pytest.mark.parametrize("n", (0, 1, 8 * MIB - 1, 8 * MIB, 8 * MIB + 1, 24 * MIB, 32 * MIB + 1, 40 * MIB + 3))
def test_write_fd(gpu, arenas, tmp_path, n):
    import torch
    path = str(tmp_path / "appended.bin")
    for phase in PHASES:
        A = arenas(n)
        d = device_pattern(A, n, phase)
        got = through_pipe(gpu, d)
        torch.cuda.synchronize()
        A.check()
        same(got, n, 0, DEV_SALT)
        with open(path, "wb") as f:
            f.write(pat(1001, 0, OLD_SALT).tobytes())
        fd = os.open(path, os.O_WRONLY | os.O_APPEND)
        try:
            gpu.write_fd(fd, d)
        finally:
            os.close(fd)
        torch.cuda.synchronize()
        A.check()
        with open(path, "rb") as f:
            got = np.frombuffer(f.read(), dtype=np.uint8)
        assert len(got) == 1001 + n
        same(got[:1001], 1001, 0, OLD_SALT)
        same(got[1001:], n, 0, DEV_SALT)
        called("naf_gpu_write_fd", 2)


# ---- the lanes' pinned buffers grow between transfers ----------------------------------------------------------------------------
def test_lane_buffers_grow_between_transfers_on_one_context(arenas, source, tmp_path):
    """4 MiB buffers for lane 0, then 16 MiB ones for it (write_file), the small read again through the larger buffers, 16 MiB ones for
    lane 1 as well (write_fd), then three lanes of which the third is new and small."""
    import torch
    from naf_amd import capi
    ctx = capi.Context(0)
    try:
        read_and_check(ctx, arenas(5 * MIB), source, 5 * MIB, 4097, 1)
        A = arenas(17 * MIB)
        d = device_pattern(A, 17 * MIB, 65)
        path = str(tmp_path / "grown.bin")
        fd = os.open(path, os.O_RDWR | os.O_CREAT, 0o600)
        try:
            ctx.write_file(fd, 0, d)
        finally:
            os.close(fd)
        torch.cuda.synchronize()
        A.check()
        with open(path, "rb") as f:
            same(f.read(), 17 * MIB, 0, DEV_SALT)
        read_and_check(ctx, arenas(9 * MIB + 1), source, 9 * MIB + 1, 0, 65)
        A = arenas(33 * MIB)
        d = device_pattern(A, 33 * MIB, 1)
        got = through_pipe(ctx, d)
        torch.cuda.synchronize()
        A.check()
        same(got, 33 * MIB, 0, DEV_SALT)
        read_and_check(ctx, arenas(BIG), source, BIG, 4097, 1)
        called("naf_gpu_write_file"); called("naf_gpu_write_fd")
    finally:
        ctx.close()


# ---- upload, download, download_async --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 4097, MIB + 1))
def test_upload_download_round_trips(gpu, arenas, n):
    import torch
    A = arenas(n)
    d = A.out(n, 1)
    h_src, h_dst, h_pin = gpu.host_alloc(n + 1), gpu.host_alloc(n + 1), gpu.host_alloc(n + 1)
    view = lambda p: np.ctypeslib.as_array((C.c_uint8 * (n + 1)).from_address(p))
    try:
        view(h_src)[:n] = pat(n, 0, DEV_SALT)
        view(h_dst)[:] = 0xEE
        view(h_pin)[:] = 0xEE
        gpu.upload(d, h_src, n)
        gpu.download(h_dst, d, n)                                      # returns after completion
        same(view(h_dst)[:n].copy(), n, 0, DEV_SALT)
        assert view(h_dst)[n] == 0xEE
        gpu.download_async(h_pin, d, n)
        gpu.synchronize()
        same(view(h_pin)[:n].copy(), n, 0, DEV_SALT)
        assert view(h_pin)[n] == 0xEE
        torch.cuda.synchronize()
        A.check()
        holds(d, n, 0, DEV_SALT)
    finally:
        for p in (h_src, h_dst, h_pin):
            gpu.host_free(p)
    for e in ("naf_gpu_upload", "naf_gpu_download", "naf_gpu_download_async", "naf_gpu_synchronize"):
        called(e)
    called("naf_gpu_host_alloc", 3); called("naf_gpu_host_free", 3)
