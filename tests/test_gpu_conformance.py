"""GPU conformance (run with -m gpu on an MI355X): the frames of tests/zstd_corpus.py -- every encoding choice of RFC 8878 made on
purpose, their content known by construction and confirmed by libzstd in tests/test_zstd_compose.py -- through the HIP decoder under
every executor, sequence walk and fast-path lever, alone and spliced into oracle-made archives in place of their sequence section."""
import re

import numpy as np
import pytest

import zstd_corpus as K

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
def frames():
    return [(n, f, c) for n, f, c, feat in K.corpus(look=False)]


def host(t):
    return t.cpu().numpy().tobytes()


EXECUTORS = {"auto": {}, "hbm": {"NAF_GPU_EXEC_LDS": "0"}, "hbm-nocollapse": {"NAF_GPU_EXEC_LDS": "0", "NAF_GPU_EXEC_COLLAPSE": "0"},
             "hbm-nearcollapse": {"NAF_GPU_EXEC_LDS": "0", "NAF_GPU_EXEC_COLLAPSE": "n"},
             "hbm-smallcollapse": {"NAF_GPU_EXEC_LDS": "0", "NAF_GPU_EXEC_COLLAPSE": "s"},
             "batch": {"NAF_GPU_EXEC_LDS": "0", "NAF_GPU_EXEC": "batch"}, "serial": {"NAF_GPU_EXEC_LDS": "0", "NAF_GPU_EXEC": "serial"},
             "seq-wave-l": {"NAF_GPU_SEQ_WAVE": "l"}, "seq-wave-all": {"NAF_GPU_SEQ_WAVE": "all"}, "seq-rep-walk": {"NAF_GPU_SEQ_REP": "walk"},
             "flat0": {"NAF_GPU_FLAT": "0"}, "uniform0": {"NAF_GPU_UNIFORM": "0"}, "stride0": {"NAF_GPU_STRIDE_INDEX": "0"},
             "huf-part-64-8": {"NAF_GPU_HUF_PART": "64", "NAF_GPU_HUF_MARGIN": "8"}, "huf-part-4096": {"NAF_GPU_HUF_PART": "4096"},
             "huf-par0": {"NAF_GPU_HUF_PAR": "0"}, "spec-min-8": {"NAF_GPU_SPEC_MIN": "8"}}


@pytest.mark.parametrize("how", list(EXECUTORS))
def test_corpus_frames_alone(gpu, frames, how, monkeypatch):
    """Every format and state frame, at each of its three sizes, decodes to the composer's content."""
    for k, v in EXECUTORS[how].items():
        monkeypatch.setenv(k, v)
    bad = []
    for name, fr, content in frames:
        got = host(gpu.zstd_decompress(gpu.to_device(fr), len(content) + 64))
        if got != content:
            bad.append((name, len(got), len(content)))
    assert not bad, bad


# ---- the lookalikes as the sequence section of an archive ----------------------------------------------------------------------
def _vle(v):
    out = [v & 127]
    v >>= 7
    while v:
        out.append(128 | (v & 127))
        v >>= 7
    return bytes(reversed(out))


def splice(oracle, naf, section, frame):
    """naf with section's frame replaced by frame (written without its magic), its compressed-size VLE rewritten."""
    h = oracle.parse_naf(naf)
    off, size = h.payload_off[section], h.comp[section]
    old = _vle(size)
    assert naf[off - len(old):off] == old
    body = frame[4:]
    return naf[:off - len(old)] + _vle(len(body)) + body + naf[off + size:]


@pytest.fixture(scope="module")
def look_archive(oracle):
    content = K.lookalike_content()
    bases = oracle.unpack_4bit(content, 2 * len(content))
    lines = [bases[i:i + 80] for i in range(0, len(bases), 80)]
    text = b">lookalike\n" + b"\n".join(lines) + b"\n"
    naf = oracle.ennaf(text)
    assert oracle.zstd_decompress(oracle.parse_naf(naf).frame(naf, oracle.SEQ)) == content
    return text, naf


MODES = [(0, True, -1), (0, False, -1), (2, True, -1), (3, True, -1), (4, True, -1), (0, True, 61)]
EMIT_PATHS = {"fused": {"NAF_GPU_FUSE": "1", "NAF_GPU_EMIT": "", "NAF_GPU_FORCE_SLOW": "0"},
              "long": {"NAF_GPU_FUSE": "0", "NAF_GPU_EMIT": "long", "NAF_GPU_FORCE_SLOW": "0"},
              "span": {"NAF_GPU_FUSE": "0", "NAF_GPU_EMIT": "span", "NAF_GPU_FORCE_SLOW": "0"},
              "short": {"NAF_GPU_FUSE": "0", "NAF_GPU_EMIT": "short", "NAF_GPU_FORCE_SLOW": "0"},
              "slow": {"NAF_GPU_FUSE": "0", "NAF_GPU_EMIT": "", "NAF_GPU_FORCE_SLOW": "1"}}


def _set(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_small_frames_take_the_small_frame_decoder(gpu):
    """Positive control of the small forms: each is decoded by k_small_frame alone (no fallback to the general front)."""
    bad = []
    for name, fr, content, feat in K.corpus(sizes=("small",), look=False):
        if "@small" not in name:
            continue
        gpu.set_timing(True)
        got = host(gpu.zstd_decompress(gpu.to_device(fr), len(content) + 64))
        ran = {n for n, ms, k in gpu.get_timing()}
        gpu.set_timing(False)
        if got != content or not ran or not all(n.endswith("zstd_small_frame") for n in ran):
            bad.append((name, got == content, sorted(ran)))
    assert not bad, bad


@pytest.mark.parametrize("how", ["auto", "flat0", "uniform0", "stride0", "spec-min-8"])
def test_lookalike_frames_alone(gpu, how, monkeypatch):
    """The lookalikes through gpu.zstd_decompress (the stride index and the frame fronts without an emit behind them)."""
    import torch
    _set(monkeypatch, EXECUTORS[how])
    look = torch.frombuffer(bytearray(K.lookalike_content()), dtype=torch.uint8).to("cuda")
    bad = []
    for name, blocks in K.lookalike_frames():
        fr = K.compose_look(blocks)[0]
        out = gpu.zstd_decompress(gpu.to_device(fr), look.numel() + 64)
        if out.numel() != look.numel() or not torch.equal(out, look):
            bad.append(name)
    assert not bad, bad


def _want(oracle, naf, modes):
    import torch
    out = {}
    for m in modes:
        try:
            out[m] = torch.frombuffer(bytearray(oracle.unnaf(naf, *m)), dtype=torch.uint8).to("cuda")
        except ValueError:
            pass
    return out


def _same(t, want):
    import torch
    return t.numel() == want.numel() and torch.equal(t, want)


def test_lookalike_frames_spliced_into_an_archive(gpu, oracle, look_archive, monkeypatch, capfd):
    """The control frame (identical flat 4-bit blocks) and each variant that differs from it in one legal way, at the block
    positions of K.look_positions(), as the sequence section of an archive: unnaf in each output mode of MODES (default emit) and
    in FASTA and sequence mode through each emit path, unnaf_range around the changed block, against the oracle's output of the
    original archive.  Positive controls: the control frame takes the stride index (verdict 1), the uniform front (ok 1 bad 0)
    and the in-place emit (unnaf_emit_flat); the frame with sequence blocks at exactly 1/8 of its blocks takes the mostly-flat
    way with sequences ([flat mixed], unnaf_emit_flat, the sequence executor)."""
    import torch
    text, naf = look_archive
    look = K.lookalike_content()
    monkeypatch.setenv("NAF_GPU_SPEC_MIN", "8")
    want = _want(oracle, naf, MODES)
    hdr = text.index(b"\n") + 1
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda")
    bad = []
    for name, blocks in K.lookalike_frames():
        fr, content, _ = K.compose_look(blocks)
        assert content == look, name                                    # (the frame stands in for the section: same bytes)
        d = gpu.to_device(splice(oracle, naf, oracle.SEQ, fr))
        if name in ("look_control", "look_seq_blocks_%d" % (K.LOOK_N // 8)):
            capfd.readouterr()
            monkeypatch.setenv("NAF_GPU_DEBUG_FLAT", "1"); monkeypatch.setenv("NAF_GPU_DEBUG_STRIDE", "1")
            gpu.set_timing(True)
            got = gpu.unnaf(d, 0)
            ran = {x for x, ms, k in gpu.get_timing()}
            gpu.set_timing(False)
            monkeypatch.delenv("NAF_GPU_DEBUG_FLAT"); monkeypatch.delenv("NAF_GPU_DEBUG_STRIDE")
            err = capfd.readouterr().err
            assert _same(got, want[MODES[0]]), name
            assert "unnaf_emit_flat" in ran, (name, sorted(ran))
            if name == "look_control":
                assert re.search(r"\[stride\] len \d+ S \d+ nmax \d+ prefix \d+ verdict 1 err 0", err), err
                assert re.search(r"\[uniform\?\] ok 1 bad 0", err), err
            else:
                m = re.search(r"\[flat mixed\] nblk (\d+) decoded (\d+) main \d+ \(blocks with sequences (\d+)\)", err)
                assert m and int(m.group(3)) == K.LOOK_N // 8 and int(m.group(2)) * 2 <= int(m.group(1)), err
                assert any(x.endswith("zstd_exec_seq") for x in ran), sorted(ran)
        for m in MODES:
            if not _same(gpu.unnaf(d, *m), want[m]):
                bad.append((name, m))
        for path, env in EMIT_PATHS.items():
            _set(monkeypatch, env)
            for m in (MODES[0], MODES[3]):
                if not _same(gpu.unnaf(d, *m), want[m]):
                    bad.append((name, path, m))
            for k in env:
                monkeypatch.delenv(k)
        p = int(name.split("@")[1]) if "@" in name else K.LOOK_N - 1
        b0 = p * 2 * K.LOOK_BLOCK
        for a, b in ((b0 - 7, b0 + 5), (b0, b0 + 2 * K.LOOK_BLOCK), (b0 + 1000, b0 + 3 * 2 * K.LOOK_BLOCK + 3)):
            a = max(0, a); b = min(2 * K.LOOK_N * K.LOOK_BLOCK, b)
            oa, ob = hdr + a + a // 80, hdr + b + b // 80                 # the FASTA text's offsets of those bases
            if not _same(gpu.unnaf_range(d, oa, ob, 0), d_text[oa:ob]):
                bad.append((name, "range", oa, ob))
    assert not bad, bad


def _archives(oracle):
    """A masked multi-record DNA FASTA of a few MB, a FASTQ, and the golden mixed_60 (reference-made)."""
    from naf_amd import synth
    from conftest import golden_bytes
    yield "fasta", oracle.ennaf(synth.fasta_mixed(500, 6000, 60, seed=3)), [(0, True, -1), (0, False, -1), (2, True, -1), (3, True, -1), (0, True, 17)]
    yield "fastq", oracle.ennaf(synth.fastq_reads(12000, 150, seed=5, var_len=True)), [(0, True, -1), (1, True, -1), (2, True, -1)]
    yield "mixed_60", golden_bytes("naf", "mixed_60.naf"), [(0, True, -1), (0, False, -1), (2, True, -1), (3, True, -1), (0, True, 13)]


def test_sections_recoded_in_corpus_shapes(gpu, oracle, monkeypatch):
    """The sequence, ids, lengths and mask sections of three archives re-coded by K.recode (Raw / RLE blocks, raw literals, Huffman
    literals of every form and treeless, sequences from the runs in the bytes under predefined, FSE and Repeat tables, repeat
    code 1 across blocks), one section at a time and all at once: unnaf in each mode through each emit path, and unnaf_range at
    the re-coded sequence section's block seams, against the oracle's output of the original archive."""
    import zstd_compose as Z
    for aname, naf, modes in _archives(oracle):
        h = oracle.parse_naf(naf)
        want = _want(oracle, naf, modes)
        fasta = want[modes[0]]
        variants = []
        for style in range(3):
            all_at_once = naf
            for sec in (oracle.SEQ, oracle.IDS, oracle.LENGTHS, oracle.MASK):
                if h.payload_off[sec] is None:
                    continue
                data = oracle.zstd_decompress(h.frame(naf, sec))
                fr = Z.compose(K.recode(data, style + sec), window_log=22, checksum=style == 1 and len(data) < (1 << 20))[0]
                assert oracle.zstd_decompress(fr, len(data) + 64) == data, (aname, sec, style)
                variants.append(("%s/sec%d/style%d" % (aname, sec, style), splice(oracle, naf, sec, fr)))
                all_at_once = splice(oracle, all_at_once, sec, fr)
            variants.append(("%s/all/style%d" % (aname, style), all_at_once))
        bad = []
        n = fasta.numel()
        for vname, v in variants:
            d = gpu.to_device(v)
            for m in modes:
                if m in want and not _same(gpu.unnaf(d, *m), want[m]):
                    bad.append((vname, m))
            for path, env in EMIT_PATHS.items():
                _set(monkeypatch, env)
                for m in modes[:2]:
                    if m in want and not _same(gpu.unnaf(d, *m), want[m]):
                        bad.append((vname, path, m))
                for k in env:
                    monkeypatch.delenv(k)
            for a, b in ((0, 1), (n // 3, n // 3 + 120_001), (n - 70_000, n), (n // 2 - 3, n // 2 + 3)):
                a = max(0, a)
                if not _same(gpu.unnaf_range(d, a, b, modes[0][0]), fasta[a:b]):
                    bad.append((vname, "range", a, b))
        assert not bad, bad
