"""The encoder's literals planner (k_zenc_plan, k_zenc_tree, k_zenc_flat_scan, k_zenc_frame_*; huf_lengths_sorted, huf_write_tree_w,
zenc_plan_finish) on the blocks of tests/huf_plan.py: histograms and placements planted on every alphabet, profile, length, seam and
gain edge, brought to the planner's five parameter sets by five carriers (run with -m gpu on an MI355X).

Every frame this build makes of a planned stream is decoded by the from-spec oracle, by this machine's libzstd where it loads and by
the HIP decoder with either sequence executor; an archive also by this build's unnaf and, where it is built, the reference's.  Then
every BLOCK of the frame, as oracle.zstd_literals lists it, is held to the model (huf_plan.check_frame): the plan's split, no block
above 3 + bn, RLE and Raw where the planner says so, the narrowest literals header, four streams of exactly the bytes the listed
lengths give, a complete code within the carrier's limit that is the documented construction's to the bit, the tree description's
form and size, the same description for the same weights whoever wrote it, Raw against Huffman by the model's bracket, and the
frame's code where a frame has one.  Which launches ran comes from Context.get_timing, which sections are treeless from the oracle."""
import ctypes
import os
import subprocess
import time
from contextlib import contextmanager

import numpy as np
import pytest

import huf_plan as P

pytestmark = pytest.mark.gpu


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


def host(t):
    return t.cpu().numpy().tobytes()


@contextmanager
def switches(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


_COV, _DESC, _RAN = P.Coverage(), {}, {}


def make(gpu, oracle, c, timing=False):
    """(frame with magic, archive or None, text or None, names of the kernels that ran) of a case by its carrier's route."""
    Pm = P.CARRIERS[c.carrier]
    names = set()
    with switches(**c.env):
        if timing:
            gpu.set_timing(True)
        try:
            if Pm.route == "direct":
                frame, naf, text = host(gpu.zstd_compress(gpu.to_device(c.data), level=2 if Pm.try_fse else 1)), None, None
            else:
                text = P.text_of(c)
                naf = host(gpu.ennaf(gpu.to_device(text))[0])
                frame = oracle.parse_naf(naf).frame(naf, P.STREAM_INDEX[Pm.route])
            if timing:
                names = {nm for nm, ms, k in gpu.get_timing()}
        finally:
            if timing:
                gpu.set_timing(False)
    return frame, naf, text, names


def ran(names, kernel):
    return any(nm.endswith(kernel) for nm in names)


def ref_unnaf(oracle, naf):
    """The reference's decode, None where it does not return (it waits for ever on some archives: a failure, not a wait of two minutes)."""
    old, oracle.REF_TIMEOUT = oracle.REF_TIMEOUT, 20
    try:
        return oracle.ref_unnaf(naf)
    except (subprocess.TimeoutExpired, ValueError):
        return None
    finally:
        oracle.REF_TIMEOUT = old


def run_case(gpu, oracle, libzstd, c, timing=False):
    """Every check of one case; returns (the reasons it failed for, the listing, the kernel names)."""
    bad, Pm = [], P.CARRIERS[c.carrier]
    frame, naf, text, names = make(gpu, oracle, c, timing)
    try:
        P.check_decodes(oracle, frame, c.data)
    except P.Reject as e:
        return [str(e)], None, names
    if libzstd is not None:
        out = ctypes.create_string_buffer(len(c.data) + 64)
        r = libzstd.ZSTD_decompress(out, len(c.data) + 64, frame, len(frame))
        if r != len(c.data) or out.raw[:len(c.data)] != c.data:
            bad.append("libzstd: %d" % r)
    d_frame = gpu.to_device(frame)
    for lds in ("1", "0"):
        with switches(NAF_GPU_EXEC_LDS=lds):
            if host(gpu.zstd_decompress(d_frame, len(c.data) + 64)) != c.data:
                bad.append("HIP decoder, NAF_GPU_EXEC_LDS=%s" % lds)
    if naf is not None:
        if host(gpu.unnaf(gpu.to_device(naf))) != text:
            bad.append("unnaf of the archive")
        # (the reference's unnaf never returns from a FASTQ whose sequence frame ends on a block of 4 bytes or fewer of content -- its own
        # ennaf's archive of a FASTQ of a few bases included: such a text has no reference decode)
        if oracle.have_ref() and not (Pm.route == "fastq" and len(c.data) < 16) and ref_unnaf(oracle, naf) != text:
            bad.append("the reference's unnaf of the archive")
    lits = oracle.zstd_literals(frame)
    try:
        paths = P.check_frame(c, frame, lits, _DESC.setdefault(c.carrier, {}))
        _COV.add(c, paths)
    except P.Reject as e:
        bad.append(str(e))
        _COV.exempt(c)
    return bad, lits, names


def run_small(gpu, oracle, libzstd, carrier):
    if ("small", carrier) not in _RAN:
        t0, bad, n = time.perf_counter(), [], 0
        for seed in P.SEEDS:
            for c in P.small_cases(seed, carrier):
                if not c.nblk:
                    _COV.exempt(c)
                    continue
                n += 1
                b, _, names = run_case(gpu, oracle, libzstd, c, timing=c.name.endswith(".pack") and seed == P.SEEDS[0])
                bad += ["%s seed %d: %s" % (c.name, seed, x) for x in b]
                if names and carrier == "seq" and not ran(names, "zenc_flat_scan"):
                    bad.append("%s: k_zenc_flat_scan did not run" % c.name)
                # (an archive's timing holds the launches of all of its streams: what did NOT run is asked of the direct route only)
                if names and P.CARRIERS[carrier].route == "direct" and (ran(names, "zenc_plan_sample") or ran(names, "zenc_tree") or ran(names, "zenc_frame_quick")):
                    bad.append("%s: a kernel of the large frames ran on %d blocks" % (c.name, c.nblk))
        _RAN[("small", carrier)] = (bad, n, time.perf_counter() - t0)
    return _RAN[("small", carrier)]


def run_large(gpu, oracle, libzstd, carrier, seed):
    if ("large", carrier, seed) not in _RAN:
        t0, bad, n = time.perf_counter(), [], 0
        Pm = P.CARRIERS[carrier]
        for c in P.big_cases(seed, carrier):
            n += 1
            b, lits, names = run_case(gpu, oracle, libzstd, c, timing=True)
            bad += ["%s seed %d: %s" % (c.name, seed, x) for x in b]
            if lits is None:
                continue
            treeless = int((lits.lit_type == 3).sum())
            want = ["zenc_plan", "zenc_tree"] + (["zenc_plan_sample"] if c.nblk >= P.FRAME_BLOCKS else []) + (["zenc_flat_scan"] if Pm.flat_scan else []) \
                + (["zenc_frame_quick", "zenc_plan_frame", "zenc_frame_fix"] if c.frame_tree else [])
            bad += ["%s: %s did not run (%s)" % (c.name, k, sorted(names)) for k in want if not ran(names, k)]
            if Pm.route == "direct" and c.nblk < P.FRAME_BLOCKS and ran(names, "zenc_plan_sample"):
                bad.append("%s: the sample launch ran on %d blocks" % (c.name, c.nblk))
            if not c.frame_tree and (treeless or (Pm.route == "direct" and ran(names, "zenc_frame_quick"))):
                bad.append("%s: %d treeless sections, zenc_frame_quick %s, in a frame without a frame's tree" % (c.name, treeless, ran(names, "zenc_frame_quick")))
            if c.frame_tree and not treeless:             # (which sections are treeless is check_frame's: the frame's code in the block in front)
                bad.append("%s: no treeless section" % c.name)
        _RAN[("large", carrier, seed)] = (bad, n, time.perf_counter() - t0)
    return _RAN[("large", carrier, seed)]


@pytest.mark.parametrize("carrier", P.GPU_CARRIERS)
def test_planted_blocks(gpu, oracle, libzstd, carrier, capsys):
    """The pack of alphabet and profile cells, the seam packs, every block length, the gain cells and the dozen shapes, at three seeds."""
    bad, n, dt = run_small(gpu, oracle, libzstd, carrier)
    with capsys.disabled():
        print("\n  %s: %d frames over seeds %s, %.1f s, %d failures" % (carrier, n, list(P.SEEDS), dt, len(bad)))
        print("".join("    %s\n" % x[:400] for x in bad[:8]), end="")
    assert n > 0
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("seed", P.SEEDS)
@pytest.mark.parametrize("carrier", P.GPU_CARRIERS)
def test_large_frames(gpu, oracle, libzstd, carrier, seed, capsys):
    """256 blocks (k_zenc_tree) and 4096 blocks (the sampled cache; the frame's tree and k_zenc_frame_quick for the quality and sequence
    streams, and the same stream with NAF_GPU_FRAME_TREE=0): the dozen shapes, some at sampled block numbers only, some between them."""
    bad, n, dt = run_large(gpu, oracle, libzstd, carrier, seed)
    with capsys.disabled():
        print("\n  %s seed %d: %d frames, %.1f s, %d failures" % (carrier, seed, n, dt, len(bad)))
        print("".join("    %s\n" % x[:400] for x in bad[:8]), end="")
    assert not bad, "\n".join(bad[:20])


def test_a_fastq_whose_sequence_stream_ends_constant(gpu, oracle):
    """The quality carrier's texts have one base, A, throughout: the packed sequence stream is constant, and as RLE blocks to the end its
    frame would end on a block of 3 + 1 bytes, which the reference's FASTQ reader never feeds to its decoder (it stops 4 bytes short
    and waits).  The frame's last block is a Raw block (ZENC_LONG_LAST), the ones in front stay RLE, and the reference reads the archive."""
    for n in (40, 4096, 300000):
        text = P.fastq_text(bytes(33 + (i * 7) % 60 for i in range(n)))
        naf = host(gpu.ennaf(gpu.to_device(text))[0])
        h = oracle.parse_naf(naf)
        L = oracle.zstd_literals(h.frame(naf, oracle.SEQ))
        # (with the look at the stream on, the last block of a long constant stream is coded with a match instead: more than 4 bytes too)
        assert L.size == n // 2 and int(L.block_type[-1]) != 1 and int(L.frame_size[-1]) > 3 + 4, (n, list(L.block_type))
        assert all(int(t) == 1 for t in L.block_type[:-1])
        assert host(gpu.unnaf(gpu.to_device(naf))) == text
        if oracle.have_ref():
            assert ref_unnaf(oracle, naf) == text, n
        with switches(NAF_GPU_PROBE="0", NAF_GPU_BLOCK_LOG="10"):
            naf = host(gpu.ennaf(gpu.to_device(text))[0])
        L = oracle.zstd_literals(oracle.parse_naf(naf).frame(naf, oracle.SEQ))
        assert len(L) == -(-(n // 2) // 1024) and int(L.block_type[-1]) == 0 and all(int(t) == 1 for t in L.block_type[:-1]), (n, list(L.block_type[-3:]))
        if oracle.have_ref():
            assert ref_unnaf(oracle, naf) == text, n
    # a FASTA has no such reader in front of it: its constant stream stays RLE blocks to the end
    fa = b">s\n" + b"A" * 300000 + b"\n"
    naf = host(gpu.ennaf(gpu.to_device(fa))[0])
    L = oracle.zstd_literals(oracle.parse_naf(naf).frame(naf, oracle.SEQ))
    assert int(L.block_type[-1]) == 1
    if oracle.have_ref():
        assert ref_unnaf(oracle, naf) == fa


def test_the_same_weights_the_same_description(gpu, oracle, libzstd):
    """Blocks of equal weights across the small case (the planner's own lane), 256 blocks (k_zenc_tree) and 4096 blocks (the cache hit):
    check_frame kept one description per weight table over all frames of a carrier; here it is shown that tables were met again."""
    for carrier in P.GPU_CARRIERS:
        run_small(gpu, oracle, libzstd, carrier)
        run_large(gpu, oracle, libzstd, carrier, P.SEEDS[0])
        assert len(_DESC.get(carrier, {})) > 20, carrier
    sh = {c.name for c in P.big_shapes().values()}
    for carrier in P.GPU_CARRIERS:
        for name in sh:
            sizes = [tag for tag in ("small", "256", "4096") if (("big", "%s@%s" % (name, tag)), carrier) in _COV.seen]
            assert len(sizes) == 3 or _COV._why(("big", name + "@small"), carrier), (carrier, name, sizes)


def test_coverage(gpu, oracle, libzstd, capsys):
    """Every cell of every carrier has a block that passed every check, or the reason why the carrier cannot hold it; every path
    letter of the planner was met."""
    for carrier in P.GPU_CARRIERS:
        run_small(gpu, oracle, libzstd, carrier)
        for seed in P.SEEDS:
            run_large(gpu, oracle, libzstd, carrier, seed)
    with capsys.disabled():
        print("\n" + _COV.table(P.GPU_CARRIERS, "kernels, seeds %s" % list(P.SEEDS)))
        print("  seconds: " + ", ".join("%s %.1f" % ("/".join(str(x) for x in k), v[2]) for k, v in sorted(_RAN.items(), key=str)))
    holes = _COV.empty(P.GPU_CARRIERS)
    assert not holes, holes[:20]
    assert set("FRSLPQCMDTWE") <= _COV.letters(), sorted(_COV.letters())
