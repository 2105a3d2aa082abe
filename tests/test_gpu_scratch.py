"""Scratch history: a context's answers do not depend on what its arenas went through before the call.

One fresh context per test, so that the history is what the test says it is.  The probe table of ctx_plan.py runs on a fresh context,
directly after naf_gpu_reserve, directly after naf_gpu_release_scratch, after a whole unnaf that grew the arena past one 64 MiB chunk,
and directly after each kind of error return (the corrupt inputs are those test_gpu_decode.py and test_gpu_encode.py use); every result
equals the probe's reference.  naf_gpu_release_scratch between a shard's begin and its finish makes the finish an argument error and
leaves the context good for a whole round; and it gives back what naf_gpu_reserve took, the side contexts' eighths included."""
import ctypes as C
import time

import pytest

import ctx_plan as X
from conftest import golden_bytes

pytestmark = pytest.mark.gpu
E_FORMAT, E_ZSTD, E_CAP, E_INPUT, E_ARG = -4, -5, -6, -7, -8
MIB = 1 << 20
HISTORIES = ("fresh", "reserved", "released", "grown", "ecap", "earg", "eformat", "ezstd", "einput")


@pytest.fixture(scope="module")
def table(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield X.by_name(oracle)
    X.report(HISTORIES)


@pytest.fixture(scope="module")
def big(table):
    """(archive, text) on the device: about 3 x 64 MiB of text, made once"""
    import torch
    from naf_amd import capi, synth
    text = synth.fasta_acgt_device(3 * 64 * MIB, n_records=100)
    ctx = capi.Context(0)
    try:
        naf = ctx.ennaf(text)[0].clone()
        ctx.synchronize()
    finally:
        ctx.close()
    torch.cuda.synchronize()
    assert text.numel() > 190 * MIB
    return naf, text


@pytest.fixture()
def ctx():
    from naf_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def fails(code, call):
    from naf_amd.capi import NafGpuError
    with pytest.raises(NafGpuError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, code, str(ei.value))
    return str(ei.value)


def history(name, ctx, oracle, table, big):
    """(once, before each): what is done to the context once, and directly in front of every probe"""
    import torch
    nothing = lambda: None
    if name == "fresh":
        return nothing, nothing
    if name == "reserved":
        def again():
            ctx.release_scratch()
            ctx.reserve(256 * MIB)
        return nothing, again
    if name == "released":
        return nothing, ctx.release_scratch
    if name == "grown":
        def grow():
            naf, text = big
            free0 = ctx.mem_info()[0]
            out = torch.empty(text.numel(), dtype=torch.uint8, device=ctx.device)
            got = ctx.unnaf(naf, 0, out=out)
            ctx.synchronize()
            assert torch.equal(got, text)                              # (the text is what the test wrote)
            print("\nfree memory went down by %d MiB in the growing call" % ((free0 - ctx.mem_info()[0]) // MIB))
        return grow, nothing
    if name == "ecap":
        p = table["unnaf_fasta"]
        d = ctx.to_device(p.real)
        small = torch.empty(p.cap - 1, dtype=torch.uint8, device=ctx.device)
        return nothing, lambda: fails(E_CAP, lambda: ctx.unnaf(d, 0, out=small))
    if name == "earg":
        d = ctx.to_device(table["unnaf_fasta"].real)
        return nothing, lambda: fails(E_ARG, lambda: ctx.unnaf_runs(d, "N", min_len=0))
    if name == "eformat":
        naf = golden_bytes("naf", "mixed_60.naf")                       # truncated inside its sequence section, as test_unnaf_survives_corrupt_sections does
        h = oracle.parse_naf(naf)
        d = ctx.to_device(naf[: h.payload_off[4] + h.comp[4] // 2])
        return nothing, lambda: fails(E_FORMAT, lambda: ctx.unnaf(d, 0))
    if name == "ezstd":
        frame = golden_bytes("zstd", "ids_l3.zst")                      # the half frame of test_zstd_rejects_corrupt_frames
        d = ctx.to_device(frame[: len(frame) // 2])
        return nothing, lambda: fails(E_ZSTD, lambda: ctx.zstd_decompress(d, 1 << 20))
    if name == "einput":
        d = ctx.to_device(b"@r1\nACGT\n+\n!!!\n")                      # test_ennaf_fastq_against_oracle: quality length
        return nothing, lambda: "doesn't match sequence length" in fails(E_INPUT, lambda: ctx.ennaf(d))
    raise KeyError(name)


@pytest.mark.parametrize("name", HISTORIES)
def test_probes_do_not_depend_on_the_history(name, ctx, oracle, table, big, monkeypatch):
    import torch
    once, before = history(name, ctx, oracle, table, big)
    once()
    for p in table.values():
        with monkeypatch.context() as m:
            before()
            X.with_env(m, p)
            X.run_ready(p, ctx, oracle, torch.cuda.current_stream())
        X.count(p.name, name, p.entries + (("naf_gpu_reserve",) if name == "reserved" else ()) + (("naf_gpu_release_scratch",) if name in ("reserved", "released") else ()))


def test_release_scratch_between_shard_begin_and_shard_finish(ctx, oracle, table):
    import torch
    from naf_amd import capi, shard
    p = table["ennaf_shards"]
    d = ctx.to_device(p.real)
    opts = shard.make_opts()
    fmt, p0 = ctx.ennaf_sniff(d, opts.format)
    info = ctx.ennaf_shard_begin(d, opts, fmt, 0, 1)
    ctx.release_scratch()
    buf = torch.empty(ctx.L.naf_gpu_ennaf_shard_bound(d.numel()), dtype=torch.uint8, device=ctx.device)
    arr, pc = (capi.ShardInfo * 1)(info), capi.ShardPieces()
    rc = ctx.L.naf_gpu_ennaf_shard_finish(ctx.h, C.byref(opts), arr, C.c_void_p(buf.data_ptr()), buf.numel(), C.byref(pc))
    assert rc == E_ARG and b"shard_finish without shard_begin" in ctx.L.naf_gpu_last_error(ctx.h), (rc, ctx.L.naf_gpu_last_error(ctx.h))
    X.run_ready(p, ctx, oracle, torch.cuda.current_stream())           # (the probe's own switches are off here: the round in order)
    X.count(p.name, "released", p.entries + ("naf_gpu_release_scratch",))


def test_release_scratch_gives_the_memory_back(ctx, oracle, table):
    """R = 2 GiB: the main arena and an eighth for each of the four side contexts.  After a whole unnaf (the side contexts exist and
    hold their eighths) and the release, free memory is back to within R / 16 of the start -- half of ONE side arena, so a single
    arena that stays fails.  Other tenants of the device may take memory meanwhile: three readings a second apart, any one passes."""
    import torch
    R = 2 << 30
    p = table["unnaf_fastq"]
    d_in, d_out = X.buffers(p, ctx)
    X.call(p, ctx, d_in, d_out)                                        # (code objects, queues and the side contexts are there before the first reading)
    ctx.release_scratch()
    torch.cuda.synchronize()
    before = ctx.mem_info()[0]
    ctx.reserve(R)
    held = ctx.mem_info()[0]
    assert before - held >= R, "reserve(%d) took %d bytes" % (R, before - held)
    rc, hres, n = X.call(p, ctx, d_in, d_out)
    ctx.synchronize()
    p.judge(oracle, rc, hres, d_out[:n].cpu().numpy().tobytes())
    ctx.release_scratch()
    readings = []
    for k in range(3):
        readings.append(ctx.mem_info()[0])
        if readings[-1] >= before - R // 16:
            break
        time.sleep(1)
    print("\nfree before %d MiB, reserved %d MiB, after release %s MiB" % (before // MIB, held // MIB, [r // MIB for r in readings]))
    assert readings[-1] >= before - R // 16, "release_scratch kept %d MiB of the %d MiB reserved" % ((before - max(readings)) // MIB, (before - held) // MIB)
    X.run_ready(p, ctx, oracle, torch.cuda.current_stream())           # and the context grows its arenas again
    X.count(p.name, "released", ("naf_gpu_mem_info", "naf_gpu_reserve", "naf_gpu_release_scratch"))
