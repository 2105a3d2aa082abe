"""GPU tests of the translation (naf_gpu_unnaf_translate_size, naf_gpu_unnaf_translate, unnaf --translate).  Expected bytes never come from the
code under test: they are what translate_plan.protein_text -- plain Python over the oracle's --sequences text, ids and names of the same
archive -- gives.  Every planned text is asked in two archives, the oracle's (raw blocks of 128 KiB) and this library's own ennaf at level
1.  An output is always compared WHOLE, byte for byte."""
import ctypes as C
import os
import re
import subprocess

import pytest

import orfs_plan as OP
import translate_plan as TP
from conftest import ROOT, golden_bytes

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
CASES = [c.name for c in TP.planned(0)]
TRACE = re.compile(r"\[translate\] segments (\d+) codons (\d+) ranges (\d+) sequence bytes decoded (\d+) of (\d+)\n")


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
        self.lines = TP.lines_of(oracle.unnaf(naf, oracle.MODE_SEQUENCES, True), self.h.n_sequences)
        self.ids = oracle.zstd_decompress(self.h.frame(naf, 0)).decode("latin1").split("\0")[:-1]
        self.names = oracle.zstd_decompress(self.h.frame(naf, 1)).decode("latin1").split("\0")[:-1]
        self.d_naf = gpu.to_device(naf)
        self._want = {}

    def want(self, segs, code=1, line_length=60, key=None):
        """the model's bytes, computed once per call and left unchanged"""
        key = key or (tuple(segs), code, line_length)
        if key not in self._want:
            self._want[key] = TP.protein_text(self.lines, self.ids, self.names, segs, code, self.h.line_length if line_length < 0 else line_length)
        return self._want[key]


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive}); the two archives of a text hold the same records, ids and names"""
    out = {}
    for c in TP.planned(TP.SEED):
        arc = {"oracle": Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type))}
        own, _ = gpu.ennaf(gpu.to_device(c.text), seq_type=c.seq_type, level=1)
        arc["own"] = Archive(oracle, gpu, own.cpu().numpy().tobytes())
        a, b = arc["oracle"], arc["own"]
        assert (a.lines, a.ids, a.names) == (b.lines, b.ids, b.names) and [x.decode("latin1") for x in a.lines] == c.records, c.name
        b._want = a._want
        out[c.name] = (c, arc)
    return out


def bytes_of(t):
    return t.cpu().numpy().tobytes()


def check(gpu, A, call):
    want = A.want(call.segs, call.code, call.line_length, key=("call", call.tag))
    assert gpu.unnaf_translate_size(A.d_naf, call.segs, call.code, call.line_length) == len(want), call.tag
    got = bytes_of(gpu.unnaf_translate(A.d_naf, call.segs, call.code, call.line_length))
    if got != want:
        at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        raise AssertionError("%s: %d bytes, %d expected; first difference at byte %d: got %r, expected %r" % (call.tag, len(got), len(want), at, got[max(0, at - 20):at + 20], want[max(0, at - 20):at + 20]))
    return want


# ---- 1. the planned texts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_the_calls_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    total = 0
    for call in c.calls:
        want = check(gpu, arc[which], call)
        for kind, d, rc, at in call.plants:
            assert want[at:at + 1] == b"M"
        total += len(want)
    assert total > 0


def test_the_rna_twin_reads_the_same_letters(gpu, planned):
    (c, a), (d, b) = planned["small"], planned["rna"]
    assert b["own"].h.seq_type == 1 and any(b"U" in x for x in b["own"].lines)
    for x, y in zip(c.calls, d.calls):
        assert a["own"].want(x.segs, x.code, x.line_length) == b["own"].want(y.segs, y.code, y.line_length)
        assert bytes_of(gpu.unnaf_translate(a["own"].d_naf, x.segs, x.code, x.line_length)) == bytes_of(gpu.unnaf_translate(b["own"].d_naf, y.segs, y.code, y.line_length))


def test_the_stored_line_length_and_no_segments(gpu, planned):
    A = planned["output"][1]["own"]
    assert A.h.line_length == 70
    segs = [(0, 0, 3000, 0), (1, 5, 3000, 1)]
    assert bytes_of(gpu.unnaf_translate(A.d_naf, segs)) == A.want(segs, 1, -1) == A.want(segs, 1, 70)
    assert gpu.unnaf_translate_size(A.d_naf, []) == 0 and bytes_of(gpu.unnaf_translate(A.d_naf, [])) == b""
    three = [(0, 0, 3), (0, 1, 3), 0]                                               # 3-tuples and record numbers, as unnaf_select takes them
    assert bytes_of(gpu.unnaf_translate(A.d_naf, three, line_length=0)) == A.want(three, 1, 0)


def test_two_calls_give_identical_bytes(gpu, planned):
    c, arc = planned["records"]
    for call in c.calls[-3:]:
        a = bytes_of(gpu.unnaf_translate(arc["own"].d_naf, call.segs, call.code, call.line_length))
        assert a == bytes_of(gpu.unnaf_translate(arc["own"].d_naf, call.segs, call.code, call.line_length)) == arc["own"].want(call.segs, call.code, call.line_length, key=("call", call.tag))


# ---- 2. what is decoded ---------------------------------------------------------------------------------------------------------------------
def traced(gpu, A, segs, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    got = bytes_of(gpu.unnaf_translate(A.d_naf, segs))
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = TRACE.findall(err)
    assert len(m) == 1, err
    assert got == A.want(segs, 1, -1)
    return [int(x) for x in m[0]]


def test_far_apart_segments_decode_only_their_blocks(gpu, planned, monkeypatch, capfd):
    c, arc = planned["far"]
    far = next(x for x in c.calls if x.tag == "far").segs
    for which in ("oracle", "own"):
        A = arc[which]
        T = (A.h.orig[4] + 1) // 2
        S, codons, ranges, D, Tt = traced(gpu, A, far, monkeypatch, capfd)
        assert (S, Tt) == (len(far), T) and ranges == 2 and 0 < D < T, (which, ranges, D, T)
        assert codons == sum((min(e, len(A.lines[r])) - b) // 3 for r, b, e, _ in far)
        S, codons, ranges, D, Tt = traced(gpu, A, [1, (5, 0, TP.WHOLE, 1)], monkeypatch, capfd)
        assert ranges == 2 and D < T


# ---- 3. buffers -----------------------------------------------------------------------------------------------------------------------------
def raw(gpu, d_naf, segs, code, line_length, d_out, cap, strands="auto", n_segs=None):
    from naf_amd import capi
    o = capi.UnnafOpts(capi.OUT_SEQ, 1, line_length)                               # (the output type and the mask of the options are not used)
    g = capi.genetic_code(code)
    n = C.c_size_t(12345)
    sg = gpu._segments(segs)
    st = gpu._strands(segs) if strands == "auto" else strands
    rc = gpu.L.naf_gpu_unnaf_translate(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), C.byref(o), C.byref(g), sg, st, len(segs) if n_segs is None else n_segs,
                                       C.c_void_p(d_out.data_ptr() if d_out is not None and d_out.numel() else 0), cap, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_buffers(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x71, size=4 << 20)
    for name, tag in (("records", "mix"), ("records", "seams_L17"), ("small", "small_L16"), ("output", "whole1"), ("reads", "parts")):
        c, arc = planned[name]
        A = arc[which]
        call = next(x for x in c.calls if x.tag == tag)
        want = A.want(call.segs, call.code, call.line_length, key=("call", tag))
        n = len(want)
        for phase in (0, 1, 65):
            # exactly enough, and nothing outside it
            arena.reset()
            out = arena.out(n, phase)
            rc, got = raw(gpu, A.d_naf, call.segs, call.code, call.line_length, out, n)
            torch.cuda.synchronize()
            assert (rc, got) == (0, n), (name, tag, phase, rc)
            arena.check()
            assert bytes_of(out) == want, (name, tag, phase)
            # one byte too few: the whole size, and nothing written
            arena.reset()
            out = arena.out(n - 1, phase)
            before = out.clone()
            rc, got = raw(gpu, A.d_naf, call.segs, call.code, call.line_length, out, n - 1)
            torch.cuda.synchronize()
            assert rc == E_CAP and got == n and torch.equal(out, before), (name, tag, phase, rc, got)
            arena.check()
            assert str(n) in gpu.L.naf_gpu_last_error(gpu.h).decode()
    # the binding's own form with a caller's buffer
    buf = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
    text = gpu.unnaf_translate(A.d_naf, call.segs, call.code, call.line_length, out=buf)
    assert text.data_ptr() == buf.data_ptr() and bytes_of(text) == want and not bool(buf[n:].any())
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_translate(A.d_naf, call.segs, call.code, call.line_length, out=buf[:n - 1])
    assert e.value.code == E_CAP


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    import torch
    from naf_amd import capi
    from test_gpu_orfs import no_sequence_archive
    A = planned["records"][1]["own"]
    N = A.h.n_sequences
    L5 = len(A.lines[5])

    def fails(d_naf, segs, words=(), code=1, strands="auto"):
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        rc, n = raw(gpu, d_naf, segs, code, 60, buf, 4096, strands)
        msg = gpu.L.naf_gpu_last_error(gpu.h).decode("latin1")
        assert rc == E_ARG and n == 0 and not bool(buf.any()), (rc, n, msg)
        for w in words:
            assert w in msg, msg
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_translate_size(d_naf, segs, code) if strands == "auto" else gpu._check(rc)
        assert e.value.code == E_ARG

    ok = (5, 0, 30, 0)
    fails(A.d_naf, [ok, (N, 0, 10, 0)], ("segment 1", "record %d" % N))
    fails(A.d_naf, [ok, ok, (N + 7, 0, TP.WHOLE, 1)], ("segment 2", "record %d" % (N + 7)))
    fails(A.d_naf, [(5, 10, 10, 0)], ("segment 0", "10..10"))
    fails(A.d_naf, [ok, (5, 20, 10, 1)], ("segment 1", "20..10"))
    fails(A.d_naf, [ok, ok, ok, (5, L5, L5 + 10, 0)], ("segment 3", "record 5"))
    fails(A.d_naf, [(0, 1, 5, 0)], ("segment 0", "record 0"))                        # a part of an empty record
    st = (C.c_uint8 * 3)(0, 1, 2)
    fails(A.d_naf, [ok, ok, ok], ("segment 2", "strand 2"), strands=st)
    for name, word in (("protein_small", "protein"), ("text_small", "text")):
        d = gpu.to_device(golden_bytes("naf", name + ".naf"))
        fails(d, [0], (word, "translate"))
        fails(d, [], (word,))
    fails(gpu.to_device(no_sequence_archive(oracle)), [0], ("no sequence",))
    z = capi.GeneticCode()
    fails(A.d_naf, [ok], ("genetic code",), code=z)
    with pytest.raises(ValueError):
        gpu.unnaf_translate(A.d_naf, [ok], code=7)
    n = C.c_size_t(9)
    o = capi.UnnafOpts(0, 0, 60)
    assert gpu.L.naf_gpu_unnaf_translate_size(gpu.h, C.c_void_p(A.d_naf.data_ptr()), A.d_naf.numel(), C.byref(o), None, gpu._segments([ok]), None, 1, C.byref(n)) == E_ARG
    assert gpu.L.naf_gpu_unnaf_translate_size(gpu.h, C.c_void_p(A.d_naf.data_ptr()), A.d_naf.numel(), None, C.byref(capi.genetic_code(1)), gpu._segments([ok]), None, 1, C.byref(n)) == E_ARG
    # an archive with qualities is translated, parts of reads too, and the text is FASTA's
    F = planned["reads"][1]["own"]
    assert F.h.flags & 1 and bytes_of(gpu.unnaf_translate(F.d_naf, [(3, 1, 3, 1), 7], line_length=0)) == F.want([(3, 1, 3, 1), 7], 1, 0) and F.want([7], 1, 0).startswith(b">read7 x\n")


# ---- 5. the cross-check through the selection ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [0, 1])
def test_the_letters_are_the_translation_of_the_selected_text(gpu, planned, rc):
    from naf_amd import capi
    c, arc = planned["small"]
    A = arc["own"]
    segs = [(r, b, e, rc) for r, b, e, s in TP.small_segments(240) if s == rc] + [(2, 0, TP.WHOLE, rc), (2, 7, 9000, rc), (1, 0, TP.WHOLE, rc)]
    prot = bytes_of(gpu.unnaf_translate(A.d_naf, segs, line_length=0)).decode().split("\n")
    text = bytes_of(gpu.unnaf_select(A.d_naf, segs, capi.OUT_FASTA, use_mask=False, line_length=0)).decode().split("\n")
    assert len(prot) <= len(text) == 2 * len(segs) + 1 and prot[-1] == text[-1] == ""      # (a segment of fewer than three bases has no line of letters)
    p = t = 0
    for seg in segs:
        assert prot[p] == text[t] and prot[p].startswith(">") and ("/rc" in prot[p]) == bool(rc)      # the same header line
        want = TP.translate(text[t + 1].upper())
        assert len(text[t + 1]) == min(seg[2], len(A.lines[seg[0]])) - seg[1]
        if want:
            assert prot[p + 1] == want, seg
            p += 2
        else:
            p += 1
        t += 2
    assert p == len(prot) - 1 and t == len(text) - 1


# ---- 6. the command line -------------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_translate_writes_the_frames(gpu, planned):
    c, arc = planned["records"]
    A = arc["own"]
    lens = [len(x) for x in A.lines]
    six = [1, 2, 3, -1, -2, -3]
    for args, segs, code, L in ((["--frame", "6"], TP.frame_segments(lens, six), 1, -1),
                                ([], TP.frame_segments(lens, [1]), 1, -1),
                                (["--frame", "-2,3", "--code", "2", "--line-length", "17", "--records", "2-4", "--records", "1-1"], TP.frame_segments(lens, [-2, 3], [1, 2, 3, 0]), 2, 17),
                                (["--code-table", TP.CUSTOM_ACGT.lower(), "--line-length", "0", "--region", "r5:11-300", "--rc-region", "r5:11-300", "--region", "r7"],
                                 [(5, 10, 300, 0), (5, 10, 300, 1), (7, 0, TP.WHOLE, 0)], TP.CUSTOM_ACGT, 0),
                                (["--frame", "2,-1", "--region", "r5:11-300", "--rc-region", "r6:1-4", "--region", "r0"],
                                 [(5, 11, 300, 0), (5, 10, 300, 1), (6, 0, 3, 1), (6, 0, 4, 0), (0, 0, TP.WHOLE, 1)], 1, -1),
                                (["--revcomp", "--records", "3-3", "--frame", "1,-3"], [(2, 0, TP.WHOLE, 1), (2, 2, lens[2], 0)], 1, -1)):
        p = unnaf_cli(["--translate"] + args, A.naf)
        want = A.want(segs, code, L)
        assert p.returncode == 0 and p.stderr == b"" and p.stdout == want and want, (args, p.stderr, p.stdout[:200], want[:200])
    F = planned["reads"][1]["own"]                                                  # FASTQ: still protein FASTA
    p = unnaf_cli(["--translate", "--frame", "6", "--line-length", "20"], F.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == F.want(TP.frame_segments([len(x) for x in F.lines], six), 1, 20)
    for args in (["--translate", "--region", "nosuch"], ["--translate", "--records", "1-9999"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    p = unnaf_cli(["--translate"], golden_bytes("naf", "protein_small.naf"))
    assert p.returncode == 1 and p.stdout == b"" and b"protein" in p.stderr


def test_cli_orfs_translate_writes_the_proteins_of_the_table(gpu, oracle, planned):
    A = planned["records"][1]["own"]
    D = Archive(oracle, gpu, bytes_of(gpu.ennaf(gpu.to_device(OP.dense_case(TP.SEED).text), level=1)[0]))
    for B in (D, A):
        for args, q, code in ((["--code", "4"], OP.Q("TAA,TAG", "ATG", 75), 4), ([], OP.DEFAULTS, 1), (["--code", "4", "--stops", "TAA,TAG,TGA", "--min-orf", "30", "--strand", "-"], OP.Q(OP.STD_STOPS, "ATG", 30, 2), 4),
                              (["--code-table", TP.letters_acgt(6), "--stop-to-stop", "--min-orf", "150", "--line-length", "0"], OP.Q("TGA", None, 150), 6)):
            st, sa = q.sets()
            assert st == TP.stops_of(code) or "--stops" in args
            rows = OP.expected_rows(B.lines, st, sa, q.min_len, q.strands, q.flags)
            segs = [(int(x["record"]), int(x["begin"]), int(x["end"]), int(x["strand"])) for x in rows]
            p = unnaf_cli(["--orfs", "--translate"] + args, B.naf)
            want = B.want(segs, code, 0 if "--line-length" in args else -1)
            assert p.returncode == 0 and p.stderr == b"" and p.stdout == want, (args, len(rows), p.stderr)
    assert len(rows) > 5
