"""The encoder's fast paths at every phase of their seams: the texts of tests/seam_plan.py -- each structural feature of a FASTA or FASTQ
text planted within two bytes of a tile seam (4096), within one of a lane seam (64) and on a piece seam (16), in texts large enough for
k_enc_fused / k_pure_check, k_fq_first / k_fq_pick and k_fq_scatter_wave -- through check_ennaf: every stream against the oracle's, and
the archives of the paths that must agree byte for byte.  tests/test_seams_cpu.py holds the plan itself to what it claims.

The letters, names and qualities are drawn for seeds 0, 1 and 2 (and moved further by NAF_TEST_SEED); the plants stay where they are."""
import os

import numpy as np
import pytest

import seam_plan as P
from test_gpu_encode import check_ennaf, host

pytestmark = pytest.mark.gpu
SEEDS = (0, 1, 2)
NAMES = P.names()
FASTA = [n for n in NAMES if n.startswith("fa_")]
FASTQ = [n for n in NAMES if n.startswith("fq_") and not n.startswith("fq_die_")]
DYING = [n for n in NAMES if n.startswith("fq_die_")]
STREAMS = ("ids", "comments", "lengths", "mask", "seq", "qual")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def planned(name, seed):
    return P.texts(seed)[NAMES.index(name)]


def where(gpu, O, t, data, kw):
    """The first stream of this build's archive that differs from the oracle's, the offset it differs at, and the plants nearest to it
    (a stream offset is taken back to the text by proportion: the background is even)."""
    try:
        sp = O.split_text(data, kw.get("seq_type", 0), kw.get("no_mask", False))
        mine = host(gpu.ennaf(gpu.to_device(data), **kw)[0])
        h = O.parse_naf(mine)
        for i, want in enumerate([sp.ids, sp.comments, sp.lengths, sp.mask, sp.seq, sp.qual]):
            if h.payload_off[i] is None:
                continue
            got = O.zstd_decompress(h.frame(mine, i), len(want) + 16)
            if got != want:
                m = min(len(got), len(want))
                d = np.flatnonzero(np.frombuffer(got[:m], dtype=np.uint8) != np.frombuffer(want[:m], dtype=np.uint8))
                off = int(d[0]) if len(d) else m
                at = int(off / max(1, len(want)) * len(data))
                return "stream %s: %d bytes for %d, first differing offset %d, about text offset %d (tile %d); nearest plants: %s" % (
                    STREAMS[i], len(got), len(want), off, at, at // P.TILE, t.nearest(at))
        return "every stream as the oracle's; plants: %s" % t.plants
    except Exception as e:                                             # (the report must not hide the failure it reports on)
        return "no closer look: %r; plants: %s" % (e, t.plants)


def checked(gpu, O, t, data=None, **kw):
    data = t.data if data is None else data
    try:
        return check_ennaf(gpu, O, data, **kw)
    except AssertionError as e:
        raise AssertionError("%s: %s\n%s" % (t.name, str(e)[:2000], where(gpu, O, t, data, kw))) from e


def same(t, a, b, what):
    if a != b:
        m = min(len(a), len(b))
        d = np.flatnonzero(np.frombuffer(a[:m], dtype=np.uint8) != np.frombuffer(b[:m], dtype=np.uint8))
        raise AssertionError("%s: the archive differs under %s (%d bytes, %d bytes, first at %d); plants: %s" % (t.name, what, len(a), len(b), int(d[0]) if len(d) else m, t.plants))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", FASTA)
def test_fasta_features_at_every_seam(gpu, oracle, monkeypatch, capfd, name, seed):
    """The one pass (k_enc_fused, k_pure_check behind it) against the oracle; byte for byte the archive of the two passes; the streams
    again without direct blocks; width 61 also without a mask, width 80 also as RNA.  Every text holds one long record of plain, regular
    tiles with lower-case runs that begin and end at every delta of a tile seam: at least one block is direct, its codes and case
    bits gathered across those seams (plants a few tiles apart leave no room for a direct block elsewhere)."""
    t = planned(name, seed)
    monkeypatch.setenv("NAF_GPU_PROBE", "0"); monkeypatch.setenv("NAF_GPU_DIRECT", "2"); monkeypatch.setenv("NAF_GPU_DEBUG_DIRECT", "1")
    capfd.readouterr()
    a = checked(gpu, oracle, t)
    err = capfd.readouterr().err
    k = [int(l.split()[1]) for l in err.splitlines() if l.startswith("[direct]")]
    assert k and k[0] >= 1, (name, err[-300:])
    monkeypatch.delenv("NAF_GPU_DEBUG_DIRECT")
    if t.width == 61:
        checked(gpu, oracle, t, no_mask=True)
    if t.width == 80:
        checked(gpu, oracle, t, t.data.replace(b"T", b"U").replace(b"t", b"u"), seq_type=oracle.RNA)
    monkeypatch.setenv("NAF_GPU_ONEPASS", "0")
    same(t, a, checked(gpu, oracle, t), "NAF_GPU_ONEPASS=0")
    monkeypatch.delenv("NAF_GPU_ONEPASS"); monkeypatch.setenv("NAF_GPU_DIRECT", "0")
    checked(gpu, oracle, t)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", FASTQ)
def test_fastq_features_at_every_seam(gpu, oracle, monkeypatch, capfd, name, seed):
    """The first look beside the second (NAF_GPU_FQ_FIRST=check fails the call where they disagree) against the oracle; byte for byte the
    archive of the general kernels alone, of the second look alone and of the workgroup split; the streams again with names and side
    streams in blocks of 32 KiB; and how many tiles left the fast path (seed 0's texts: under another seed parity only)."""
    t = planned(name, seed)
    monkeypatch.setenv("NAF_GPU_FQ_FIRST", "check"); monkeypatch.setenv("NAF_GPU_DEBUG_REG", "1")
    capfd.readouterr()
    mine = checked(gpu, oracle, t)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_FQ_FIRST"); monkeypatch.delenv("NAF_GPU_DEBUG_REG")
    tiles, irregular = [int(x) for x in err.split("[fq reg] tiles ")[1].split("\n")[0].replace(", not regular", "").split()]
    back = int(err.split("[fq reg] handed back ")[1].split("\n")[0])
    for var in ("NAF_GPU_FQ_REG", "NAF_GPU_FQ_FIRST", "NAF_GPU_FQ_WAVE"):
        monkeypatch.setenv(var, "0")
        same(t, mine, host(gpu.ennaf(gpu.to_device(t.data))[0]), var + "=0")
        monkeypatch.delenv(var)
    monkeypatch.setenv("NAF_GPU_NAMES_BLOCK_LOG", "15"); monkeypatch.setenv("NAF_GPU_SIDE_BLOCK_LOG", "15")
    checked(gpu, oracle, t)
    if seed != 0 or P.SEED != 0:
        return
    print("%s: tiles %d, not regular %d, handed back %d" % (name, tiles, irregular, back))
    m = len(t.plants) - 1                                              # (the end of the text is the last tile's, irregular anyway)
    if t.family in ("regular", "alignment", "iupac") or (t.family == "segments" and t.info["count"] < 256):
        assert irregular <= 3, (name, tiles, irregular, t.plants)     # the first tile and the last ones
    elif t.family == "segments":
        assert 1 <= irregular <= 3 + 2, (name, tiles, irregular)      # FQR_MAXSEG line ends or more: not regular
    else:
        assert m / 2 <= irregular <= 3 + 2 * m, (name, tiles, irregular, t.plants)
    if t.family == "iupac":
        assert back > 0, (name, back)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", DYING)
def test_fastq_dying_texts(gpu, oracle, monkeypatch, name, seed):
    """The cause of death across a tile seam: this build's message holds the oracle's, the record's number included -- from the regular
    tiles' path and from the general kernels alone."""
    from naf_amd.capi import NafGpuError
    t = planned(name, seed)
    with pytest.raises(ValueError) as oe:
        oracle.split_text(t.data)
    msg = str(oe.value).strip()
    assert t.dies in msg
    for reg in (None, "0"):
        if reg is not None:
            monkeypatch.setenv("NAF_GPU_FQ_REG", reg)
        with pytest.raises(NafGpuError) as ei:
            gpu.ennaf(gpu.to_device(t.data))
        assert msg in str(ei.value), (name, reg, msg, str(ei.value), t.plants)
