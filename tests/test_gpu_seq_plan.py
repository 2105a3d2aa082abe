"""The sequence tables the encoder's kernels write (k_lzx_seqenc: predefined, RLE or FSE_Compressed per block and table; k_lz_seqenc:
predefined) held to the model of tests/seq_plan.py, block by block (run with -m gpu on an MI355X).

The planned streams go through Context.zstd_compress(level=2), Context.ennaf(seq_type=SEQ_TEXT, long_log=10 / 12 / 16) and, for the
in-block stage, level 1 of both routes.  Every frame is decoded by the from-spec oracle, by this machine's libzstd where it loads and
by the HIP decoder; every Compressed block with sequences passes the planner, form, size and parity checks (the last against the host
build of the same writer: byte equality of the kernels' compile of zstd_enc_core.h with the host's); no block is larger than the same
block of the frame the same call makes without the match finder.  What is asserted about coverage is a floor: over the three seeds
every cell outside seq_plan.EXEMPT is shown by at least one block.  The table is printed."""
import ctypes
import os
import subprocess
import time

import pytest

import lz_plan as P
import seq_plan as Q
from conftest import ROOT
from test_gpu_lz_plan import host, make                              # the two routes, as the match-finder tests take them

pytestmark = pytest.mark.gpu
GROUPS = ("seq.count", "seq.codes", "seq.norm", "seq.outcome", "seq.range", "seq.arch") + Q.LZ_PLAN_CLASSES


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def libzstd():
    for cand in ("/opt/conda/lib/libzstd.so", "libzstd.so.1"):
        try:
            z = ctypes.CDLL(cand)
        except OSError:
            continue
        z.ZSTD_decompress.restype = ctypes.c_size_t
        z.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        return z
    return None


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(ROOT, "tests", "emul", "libzstd_emul.so")
    env = dict(os.environ, PATH="/opt/rocm/bin:" + os.environ.get("PATH", ""))
    subprocess.check_call(["make", "-s", "-C", ROOT, "emul"], env=env)
    return Q.load_emul(so)


_PLANS, _TALLY, _RAN = {}, Q.Tally(), {}


def cases_of(seed, group):
    if seed not in _PLANS:
        _PLANS[seed] = Q.all_cases(seed)
    return [c for c in _PLANS[seed] if (c.name.startswith(group + ".") if c.cls == "seq" else c.cls == group)]


def run_case(gpu, oracle, libzstd, emul, c):
    """The decoders, checks 1 to 4 on every block, check 5 on the frame's blocks; returns the reasons the case failed for."""
    bad = []
    frame, naf = make(gpu, oracle, c)
    twin_env = {"NAF_GPU_LZ": "0"}
    if c.stage == "lzx":
        twin_env["NAF_GPU_BLOCK_LOG"] = str(min(P.LZX_BLOCK_LOG, c.wlog))   # the twin cut into the same blocks, as test_gpu_lz_plan.py builds it
    twin, _ = make(gpu, oracle, c, **twin_env)
    try:
        P.check_decodes(oracle, frame, c.data)
    except P.Reject as e:
        return [str(e)]
    if libzstd is not None:
        out = ctypes.create_string_buffer(len(c.data) + 64)
        r = libzstd.ZSTD_decompress(out, len(c.data) + 64, frame, len(frame))
        if r != len(c.data) or out.raw[:len(c.data)] != c.data:
            bad.append("libzstd: %d" % r)
    if host(gpu.zstd_decompress(gpu.to_device(frame), len(c.data) + 64)) != c.data:
        bad.append("HIP decoder")
    bad += Q.check_frame(oracle, emul, frame, c.stage, _TALLY, c.name)       # 1 to 4
    try:
        Q.check_economy(oracle.zstd_literals(frame), oracle.zstd_literals(twin))   # 5
    except P.Reject as e:
        bad.append(str(e))
    return bad


def run_group(gpu, oracle, libzstd, emul, group):
    if group not in _RAN:
        t0, bad, n = time.perf_counter(), [], 0
        for seed in Q.SEEDS:
            for c in cases_of(seed, group):
                n += 1
                bad += ["%s seed %d: %s" % (c.name, seed, b) for b in run_case(gpu, oracle, libzstd, emul, c)]
        _RAN[group] = (bad, n, time.perf_counter() - t0)
    return _RAN[group]


@pytest.mark.parametrize("group", GROUPS)
def test_planned_streams(gpu, oracle, libzstd, emul, group, capsys):
    bad, n, dt = run_group(gpu, oracle, libzstd, emul, group)
    with capsys.disabled():
        print("\n  %s: %d cases over seeds %s, %.1f s, %d failures" % (group, n, list(Q.SEEDS), dt, len(bad)))
    assert n > 0
    assert not bad, "\n".join(bad[:20])


def test_coverage_floor(gpu, oracle, libzstd, emul, capsys):
    """Every cell outside seq_plan.EXEMPT is shown by a block of the kernels' frames; the bits beside the cells are printed, not asserted:
    nothing fixes how far the planner's estimate may lie from the bits written."""
    for group in GROUPS:
        run_group(gpu, oracle, libzstd, emul, group)
    with capsys.disabled():
        print("\n" + _TALLY.table("kernels"))
        print("  seconds per group: " + ", ".join("%s %.1f" % (k, _RAN[k][2]) for k in GROUPS))
    assert _TALLY.blocks["lz"] and _TALLY.blocks["lzx"]
    _TALLY.floor()
