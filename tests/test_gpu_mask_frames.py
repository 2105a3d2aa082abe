"""GPU tests (run with -m gpu on an MI355X) of the mask stream's shortcut, emit.hip k_mask_rle_frame / mask_rle_frame(): a mask frame of
Raw and RLE blocks of ANY compressed size becomes the toggle table in one launch -- runs of four-byte RLE blocks of 0xFF units wherever
they stand, single other blocks between them, Raw blocks through LDS in pieces -- and everything else is the decoder's.

Frames the encoder itself writes at the smallest sizes that cross the former 48 KiB limit (block sizes of 128, 64 and 32 KiB of
units), and frames composed by hand (tests/zstd_compose.py) that regenerate the units of an archive the encoder made, spliced into
its mask section: the archive's own text is the expectation, NAF_GPU_MASK_RLE=0 the second opinion, the names of the kernels of an
instrumented call say which way the frame went.  One test decodes through the tile index in the shapes its stores differ by."""
import numpy as np
import pytest

import zstd_compose as Z

pytestmark = pytest.mark.gpu

# emit.hip: the toggles the shortcut holds, the bytes of a Raw block it stages at a time, the blocks other than 0xFF runs it walks
MASK_RLE_TOG, MASK_RLE_STAGE, MASK_RLE_OTHER = 8192, 16 * 1024, 2048
W = 80
HEAD = b">mask frames\n"


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def host(t):
    return t.cpu().numpy().tobytes()


def text_of(n_bases, seed, lower=(), width=W, head=HEAD):
    """One FASTA record of n_bases random ACGT in device memory, `width` columns (0: one line); lower: [a, b) base ranges in lower case."""
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[torch.randint(0, 4, (n_bases,), device="cuda", generator=g)]
    for a, b in lower:
        bases[a:b] += 32
    nl = torch.full((1,), 10, dtype=torch.uint8, device="cuda")
    parts = [torch.tensor(list(head), dtype=torch.uint8, device="cuda")]
    if width:
        full = n_bases // width
        parts.append(torch.cat([bases[:full * width].view(full, width), nl.expand(full, 1)], dim=1).reshape(-1))
        if n_bases % width:
            parts += [bases[full * width:], nl]
    else:
        parts += [bases, nl]
    return torch.cat(parts)


def names_of(gpu, d_naf, out_type=0):
    gpu.set_timing(True)
    out = gpu.unnaf(d_naf, out_type)
    nm = {n for n, ms, k in gpu.get_timing()}
    gpu.set_timing(False)
    return out, nm


def took_shortcut(nm):
    return any(n.endswith("unnaf_mask_rle") for n in nm) and not any(n.endswith("unnaf_mask_count") for n in nm)


def took_decoder(nm):
    return any(n.endswith("unnaf_mask_count") for n in nm)


def _vle(v):
    out = [v & 127]
    v >>= 7
    while v:
        out.append(128 | (v & 127))
        v >>= 7
    return bytes(reversed(out))


def splice_mask(oracle, naf, frame_body):
    """naf with the mask section's frame replaced by frame_body (a frame without its magic), its compressed-size VLE rewritten."""
    h = oracle.parse_naf(naf)
    off, size = h.payload_off[oracle.MASK], h.comp[oracle.MASK]
    old = _vle(size)
    assert naf[off - len(old):off] == old
    return naf[:off - len(old)] + _vle(len(frame_body)) + frame_body + naf[off + size:]


def blocks_of(units, cuts):
    """units cut at `cuts` (ascending positions): a piece of two or more units of one value is an RLE block, any other a Raw block."""
    out, edges = [], [0] + list(cuts) + [len(units)]
    for a, b in zip(edges, edges[1:]):
        assert 0 <= b - a <= Z.BLOCK_MAX, (a, b)
        piece = units[a:b]
        if b - a >= 2 and piece == piece[:1] * (b - a):
            out.append(Z.rle(piece[0], b - a))
        else:
            out.append(Z.raw(piece))
    return out


def frame_of(units, blocks, **kw):
    frame, content, feat = Z.compose(blocks, **kw)
    assert content == units
    return frame[4:]


class Archive:
    """A text, the archive the encoder made of it, and the units of its mask."""

    def __init__(self, gpu, oracle, text):
        self.text = text
        self.naf = host(gpu.ennaf(text)[0])
        h = oracle.parse_naf(self.naf)
        self.units = oracle.zstd_decompress(h.frame(self.naf, oracle.MASK))

    def with_frame(self, gpu, oracle, body):
        return gpu.to_device(splice_mask(oracle, self.naf, body))


# 12 289 blocks of 16 units of 0xFF and a remainder: 50 M bases
N_UPPER = 255 * 16 * 12289 + 7


@pytest.fixture(scope="module")
def upper(gpu, oracle):
    a = Archive(gpu, oracle, text_of(N_UPPER, 11))
    assert a.units == b"\xff" * (16 * 12289) + b"\x07"
    return a


@pytest.fixture(scope="module")
def upper_big(gpu, oracle):
    a = Archive(gpu, oracle, text_of(255 * 300000 + 7, 13))
    assert a.units == b"\xff" * 300000 + b"\x07"
    return a


ISLAND_HEAD = 100000


def island_text(n_runs):
    """A long upper-case head (ISLAND_HEAD units of 0xFF and a remainder), then runs of 100 lower- and 150 upper-case bases in turn, n_runs
    runs in all: every run ends in exactly one unit that is not 0xFF."""
    head = 255 * ISLAND_HEAD + 100
    lower = [(head + 250 * i, head + 250 * i + 100) for i in range(n_runs // 2)]
    n = head + 250 * (n_runs // 2) - (150 if n_runs % 2 == 0 else 0)
    return text_of(n, 12, lower=lower)


@pytest.fixture(scope="module")
def islands(gpu, oracle):
    a = Archive(gpu, oracle, island_text(MASK_RLE_TOG))
    u = np.frombuffer(a.units, dtype=np.uint8)
    assert int((u != 255).sum()) == MASK_RLE_TOG and len(u) == ISLAND_HEAD + MASK_RLE_TOG
    return a


def check_shortcut(gpu, monkeypatch, d_naf, text):
    import torch
    out, nm = names_of(gpu, d_naf)
    assert torch.equal(out, text)
    assert took_shortcut(nm), " ".join(sorted(nm))
    monkeypatch.setenv("NAF_GPU_MASK_RLE", "0")
    out0, nm0 = names_of(gpu, d_naf)
    monkeypatch.delenv("NAF_GPU_MASK_RLE")
    assert torch.equal(out0, text)
    assert took_decoder(nm0) and not any(n.endswith("unnaf_mask_rle") for n in nm0), " ".join(sorted(nm0))


def check_fallback(gpu, d_naf, text):
    import torch
    out, nm = names_of(gpu, d_naf)
    assert torch.equal(out, text)
    assert any(n.endswith("unnaf_mask_rle") for n in nm) and took_decoder(nm), " ".join(sorted(nm))


# ---- frames the encoder writes ---------------------------------------------------------------------------------------------------
# (block log, units, blocks).  The encoder cuts a stream into ceil(units / 2^log) blocks of EQUAL size (zstd_enc.hip: zenc_block_lo), so
# the Raw tail of an upper-case text is units / blocks long, and a frame of two blocks is more than half its units -- not the
# shortcut's (n_mask >= 2 cs).  Three blocks: a tail just under and just over the 48 KiB that used to be the limit of the whole
# frame, and the tails of blocks of 128 and 64 KiB; 32 KiB blocks cannot hold 48 KiB (six of them: the frame stays small, the tail
# is two pieces of the staging buffer).
ENCODER_CASES = [(16, 3 * (49152 - 64), 3), (16, 3 * (49152 + 64), 3), (17, 3 * 118000, 3), (16, 3 * 60000, 3), (15, 6 * 32000, 6)]


@pytest.mark.parametrize("log,units,nblk", ENCODER_CASES)
def test_frames_the_encoder_writes(gpu, oracle, monkeypatch, log, units, nblk):
    """An upper-case text under NAF_GPU_MASK_BLOCK_LOG: RLE blocks of 0xFF and one Raw block of units / nblk units, in one launch."""
    assert (units + (1 << log) - 1) >> log == nblk and units % nblk == 0
    tail = units // nblk
    t = text_of(255 * (units - 1) + 9, 20 + log)
    monkeypatch.setenv("NAF_GPU_MASK_BLOCK_LOG", str(log))
    d_naf = gpu.ennaf(t)[0]
    monkeypatch.delenv("NAF_GPU_MASK_BLOCK_LOG")
    naf = host(d_naf)
    h = oracle.parse_naf(naf)
    fr = h.frame(naf, oracle.MASK)
    assert h.orig[oracle.MASK] == units and tail + 4 * (nblk - 1) < len(fr) <= tail + 4 * (nblk - 1) + 32, (h.orig, len(fr))
    check_shortcut(gpu, monkeypatch, d_naf, t)


def test_encoder_frames_with_lower_case_islands(gpu, oracle, monkeypatch):
    """The 32 KiB-block text with a lower-case island of 300 bases in the middle and one of 200 at the very end: runs of 0xFF blocks
    behind a Raw block, a tail that does not end in an upper-case run."""
    log, units = 15, 6 * 32000
    n = 255 * (units - 1) + 9
    mid = 255 * (2 * 32000) + 12345                                  # in the third of the six blocks
    t = text_of(n, 20 + log, lower=[(mid, mid + 300), (n - 200, n)])
    monkeypatch.setenv("NAF_GPU_MASK_BLOCK_LOG", str(log))
    d_naf = gpu.ennaf(t)[0]
    monkeypatch.delenv("NAF_GPU_MASK_BLOCK_LOG")
    check_shortcut(gpu, monkeypatch, d_naf, t)
    assert oracle.unnaf(host(d_naf), 0) == host(t)


# ---- frames composed by hand -----------------------------------------------------------------------------------------------------
def upper_frames(units):
    n = len(units)
    body = n - 1                                                    # units of 0xFF in front of the remainder
    F = {}
    # 12 289 RLE blocks of 16 units: 49 156 bytes of headers, the first size over 48 KiB; 12 287 blocks: just under it
    F["rle_12289"] = blocks_of(units, list(range(16, body + 1, 16)))
    F["rle_12287"] = blocks_of(units, list(range(16, 16 * 12286 + 1, 16)) + [body])
    # Raw blocks about the staging size
    for k in (MASK_RLE_STAGE - 1, MASK_RLE_STAGE, MASK_RLE_STAGE + 1, 2 * MASK_RLE_STAGE + 5):
        F["raw_%d" % k] = blocks_of(units, [70000, n - k])
    # runs of 0xFF blocks and single Raw blocks in turn, 64 times
    cuts, p = [], 0
    for i in range(64):
        for j in range(1 + 37 * (i % 5)):
            p += 16; cuts.append(p)
        p += 5; cuts.append(p)
    blocks = blocks_of(units, cuts + [body])
    for i, b in enumerate(blocks[:-2]):
        if b["n"] == 5:
            blocks[i] = Z.raw(b"\xff" * 5)
    assert sum(1 for b in blocks if b["type"] == "raw") == 65
    F["alternating_64"] = blocks
    # as many blocks other than 0xFF runs as the kernel walks, and one more (Raw blocks of 16 units of 0xFF; the remainder is one too)
    for k in (MASK_RLE_OTHER, MASK_RLE_OTHER + 1):
        rest = body - 16 * (k - 1)
        F["other_%d" % k] = [Z.raw(units[16 * i:16 * i + 16]) for i in range(k - 1)] + blocks_of(units[16 * (k - 1):], [rest // 2, rest])
    return F


def big_frames(units):
    """A Raw block of 131 072 bytes: last, first, and between two runs (300 000 units: the frame is under half of them)."""
    n = len(units)
    body = n - 1
    F = {}
    F["raw_128k_last"] = blocks_of(units, [65536, n - 131072])
    F["raw_128k_first"] = [Z.raw(units[:131072])] + blocks_of(units[131072:], [65536, body - 131072])
    F["raw_128k_mid"] = (blocks_of(units[:1600], range(16, 1600, 16)) + [Z.raw(units[1600:1600 + 131072])]
                         + blocks_of(units[1600 + 131072:], list(range(16, 3200, 16)) + [100000, body - 1600 - 131072]))
    return F


UPPER_TAKEN = ["rle_12289", "rle_12287", "raw_%d" % (MASK_RLE_STAGE - 1),
               "raw_%d" % MASK_RLE_STAGE, "raw_%d" % (MASK_RLE_STAGE + 1), "raw_%d" % (2 * MASK_RLE_STAGE + 5), "alternating_64",
               "other_%d" % MASK_RLE_OTHER]


@pytest.fixture(scope="module")
def upper_composed(upper):
    return upper_frames(upper.units)


@pytest.mark.parametrize("name", UPPER_TAKEN)
def test_composed_frames_of_an_upper_case_text(gpu, oracle, monkeypatch, upper, upper_composed, name):
    body = frame_of(upper.units, upper_composed[name])
    if name.startswith("rle_"):                                     # 49 156 bytes of block headers, and 49 148
        assert sum(4 for b in upper_composed[name] if b["type"] == "rle") == 4 * int(name[4:])
    check_shortcut(gpu, monkeypatch, upper.with_frame(gpu, oracle, body), upper.text)


@pytest.mark.parametrize("name", ["raw_128k_last", "raw_128k_first", "raw_128k_mid"])
def test_raw_blocks_of_the_largest_size(gpu, oracle, monkeypatch, upper_big, name):
    blocks = big_frames(upper_big.units)[name]
    assert sum(1 for b in blocks if b["type"] == "raw" and len(b["data"]) == 131072) == 1
    body = frame_of(upper_big.units, blocks, single_segment=name.endswith("first"))
    check_shortcut(gpu, monkeypatch, upper_big.with_frame(gpu, oracle, body), upper_big.text)


def test_one_block_more_than_the_walk_takes(gpu, oracle, upper, upper_composed):
    """MASK_RLE_OTHER + 1 blocks that are not runs of 0xFF: the kernel gives the frame up, the decoder makes the same text."""
    body = frame_of(upper.units, upper_composed["other_%d" % (MASK_RLE_OTHER + 1)])
    check_fallback(gpu, upper.with_frame(gpu, oracle, body), upper.text)


def test_toggles_at_the_seams_of_the_staging_buffer(gpu, oracle, monkeypatch, islands):
    """Raw blocks of the text with 8192 toggles cut so that toggles lie on both sides of every piece's end, behind and in front of
    runs of 0xFF blocks; exactly MASK_RLE_TOG toggles are the shortcut's."""
    u = islands.units
    for first in (ISLAND_HEAD - MASK_RLE_STAGE + 1, ISLAND_HEAD - MASK_RLE_STAGE, ISLAND_HEAD - 2 * MASK_RLE_STAGE + 3, ISLAND_HEAD):
        body = frame_of(u, blocks_of(u, [16, 48, first]))                # two short runs, a long one, one Raw block to the end
        check_shortcut(gpu, monkeypatch, islands.with_frame(gpu, oracle, body), islands.text)


def test_one_toggle_more_than_the_table_holds(gpu, oracle):
    a = Archive(gpu, oracle, island_text(MASK_RLE_TOG + 1))
    u = np.frombuffer(a.units, dtype=np.uint8)
    assert int((u != 255).sum()) == MASK_RLE_TOG + 1
    body = frame_of(a.units, blocks_of(a.units, [ISLAND_HEAD]))
    check_fallback(gpu, a.with_frame(gpu, oracle, body), a.text)


def test_damaged_frames_fail_as_the_decoder_words_it(gpu, oracle, monkeypatch, upper, upper_composed):
    """A frame cut inside a block header, one cut inside a Raw block, one whose last block does not say so."""
    from naf_amd.capi import NafGpuError
    rle = frame_of(upper.units, upper_composed["rle_12289"])
    raw = frame_of(upper.units, upper_composed["raw_%d" % (2 * MASK_RLE_STAGE + 5)])
    h = len(rle) - 4 - 4 * 12289                                    # the frame header; the final Raw block is 3 + 1 bytes
    nolast = bytearray(rle); nolast[-4] &= 0xFE
    for what, body in (("header", rle[:h + 4 * 9000 + 2]), ("raw", raw[:-1000]), ("nolast", bytes(nolast))):
        d_naf = upper.with_frame(gpu, oracle, body)
        got = []
        for v in (None, "0"):
            if v is not None:
                monkeypatch.setenv("NAF_GPU_MASK_RLE", v)
            with pytest.raises(NafGpuError) as e:
                gpu.unnaf(d_naf, 0)
            got.append((e.value.code, e.value.msg))
            if v is not None:
                monkeypatch.delenv("NAF_GPU_MASK_RLE")
        assert got[0] == got[1] and got[0][1], (what, got)


def test_range_of_a_large_frame(gpu, oracle, monkeypatch, upper, upper_composed):
    """unnaf and unnaf_range (an eighth of the text from the middle) of the archive whose mask frame is 49 KiB of headers."""
    import torch
    body = frame_of(upper.units, upper_composed["rle_12289"])
    d_naf = upper.with_frame(gpu, oracle, body)
    n = upper.text.numel()
    a, b = n // 2 - n // 16, n // 2 + n // 16
    assert torch.equal(gpu.unnaf(d_naf, 0), upper.text)
    gpu.set_timing(True)
    part = gpu.unnaf_range(d_naf, a, b)
    nm = {k for k, ms, c in gpu.get_timing()}
    gpu.set_timing(False)
    assert torch.equal(part, upper.text[a:b])
    assert took_shortcut(nm), " ".join(sorted(nm))
    monkeypatch.setenv("NAF_GPU_MASK_RLE", "0")
    assert torch.equal(gpu.unnaf_range(d_naf, a, b), upper.text[a:b])


# ---- the tile index's three consumers ----------------------------------------------------------------------------------------------
def test_tile_index_shapes(gpu, monkeypatch):
    """40 MB texts through k_tile_index and whatever reads its records (the flat emit, the list kernel, k_emit_rest): three records at
    width 80, one at width 60, the same unwrapped, and a text whose last tile is one byte long -- against the text and against the
    workgroups of 256 (NAF_GPU_EMIT_WAVE=0)."""
    import torch
    from naf_amd import synth
    one = text_of(40_000_000, 31, width=60)
    flat = text_of(40_000_000, 31, width=0)
    n1 = 40_000_000
    while (len(HEAD) + n1 + (n1 + W - 1) // W) % 4096 != 1:
        n1 += 1
    cases = [(synth.fasta_acgt_device(40_000_000, n_records=3, width=80, seed=5, device="cuda"), -1, None),
             (one, -1, None), (one, 0, flat), (text_of(n1, 32), -1, None)]
    assert cases[3][0].numel() % 4096 == 1
    for t, ll, want in cases:
        want = t if want is None else want
        d_naf = gpu.ennaf(t)[0]
        out = gpu.unnaf(d_naf, 0, line_length=ll)
        assert torch.equal(out, want)
        monkeypatch.setenv("NAF_GPU_EMIT_WAVE", "0")
        out0 = gpu.unnaf(d_naf, 0, line_length=ll)
        monkeypatch.delenv("NAF_GPU_EMIT_WAVE")
        assert torch.equal(out0, want)
