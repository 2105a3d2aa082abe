"""GPU tests of reverse-complement selection (naf_gpu_unnaf_select_stranded, unnaf --rc-region / --revcomp).  Expected bytes never come
from the code under test: as in test_gpu_select.py they are cut in Python out of the oracle's whole text of the same archive, then
complemented with the translate table written out below and reversed (quality strings reversed), under the header of
include/naf_gpu.h.  All comparisons are byte-exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))          # other choices of the same kinds: NAF_TEST_SEED=n python -m pytest ...

from conftest import ROOT, golden_bytes, naf_cases

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
FASTA, FASTQ, SEQ, SEQUENCES = 0, 1, 2, 3
E_ARG = -8
SUB_CASES = ["mixed_60", "mask_bounds", "acgt_odd", "acgt_1m2", "rna_small", "ll_override", "tiny_many", "repeat_l19", "repeat_long27"]   # test_gpu_select.SUB_CASES that hold nucleotides

from select_plan import COMP_DNA, COMP_RNA, Records          # the expectation, from the oracle's whole text (shared with the planned tests)


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


def norm(s, reverse):
    """A segment of the generators (a record number, or (record, begin, end)) with a strand -> (record, begin, end or None, reverse)."""
    return (s, 0, None, reverse) if isinstance(s, int) else (s[0], s[1], s[2], reverse)


def run_select(gpu, d_naf, segs, mode, use_mask=True, line_length=-1):
    from naf_amd import capi
    return host(gpu.unnaf_select(d_naf, [(r, b, capi.WHOLE if e is None else e, rv) for r, b, e, rv in segs], mode, use_mask, line_length))


def select_size(gpu, d_naf, segs, mode, use_mask=True, line_length=-1):
    from naf_amd import capi
    return gpu.unnaf_select_size(d_naf, [(r, b, capi.WHOLE if e is None else e, rv) for r, b, e, rv in segs], mode, use_mask, line_length)


def nucleotide_cases():
    return [c for c in naf_cases() if c["name"] not in ("protein_small", "text_small")]


def without_ids(oracle, naf):
    """The same archive with its ids section cut out (flag 0x20 cleared): headers are the stored names alone."""
    h = oracle.parse_naf(naf)
    assert h.version == 1 and h.flags & 0x30 == 0x30 and naf[4] == h.flags
    vl = lambda v: max(1, (v.bit_length() + 6) // 7)
    names_at = h.payload_off[1] - vl(h.orig[1]) - vl(h.comp[1])
    out = bytearray(naf[:h.header_bytes] + naf[names_at:])
    out[4] &= ~0x20
    h2 = oracle.parse_naf(bytes(out))
    assert not h2.flags & 0x20 and h2.n_sequences == h.n_sequences and h2.orig[1:] == h.orig[1:]
    return bytes(out)


# ---- 1. whole records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nucleotide_cases(), ids=lambda c: c["name"])
def test_whole_records_reversed_alone_and_all_in_reverse_order(gpu, oracle, case):
    naf = golden_bytes("naf", case["name"] + ".naf")
    h = oracle.parse_naf(naf)
    assert h.seq_type in (0, 1) and h.n_sequences
    d_naf = gpu.to_device(naf)
    rng = np.random.default_rng(1100 + SEED)
    for mode in [FASTQ if h.flags & 1 else FASTA, SEQUENCES, SEQ]:
        for use_mask in (True, False):
            for ll in (-1, 0, 13):
                R = Records(oracle, naf, mode, use_mask, ll)
                alone = range(R.n) if R.n <= 40 else sorted(set([0, R.n - 1] + [int(x) for x in rng.integers(0, R.n, 30)]))
                for r in alone:
                    assert run_select(gpu, d_naf, [(r, 0, None, 1)], mode, use_mask, ll) == R.segment(r, 0, None, 1), (mode, use_mask, ll, r)
                rev = [(r, 0, None, 1) for r in range(R.n - 1, -1, -1)]
                want = R.expect(rev)
                assert run_select(gpu, d_naf, rev, mode, use_mask, ll) == want, (mode, use_mask, ll)
                assert select_size(gpu, d_naf, rev, mode, use_mask, ll) == len(want)


def test_reversed_quality_strings_of_the_fastq_archives(gpu, oracle):
    for name in ("fastq_4k", "fastq_var"):
        naf = golden_bytes("naf", name + ".naf")
        R = Records(oracle, naf, FASTQ)
        d_naf = gpu.to_device(naf)
        segs = [(r, 0, None, r & 1) for r in range(R.n)]                                 # strands interleaved
        got = run_select(gpu, d_naf, segs, FASTQ)
        assert got == R.expect(segs)
        r = 1
        rec = R.segment(r, 0, None, 1).split(b"\n")
        assert rec[0] == b"@" + R.ids[r] + b"/rc" + R.head[r][1 + len(R.ids[r]):] and rec[3] == R.qual[r][::-1] and rec[2] == R.plus[r]


def test_headers_of_an_archive_without_ids(gpu, oracle):
    naf = without_ids(oracle, golden_bytes("naf", "mixed_60.naf"))
    d_naf = gpu.to_device(naf)
    R = Records(oracle, naf, FASTA)
    assert not R.has_ids
    segs = [(0, 0, None, 1), (3, 0, None, 0), (5, 2, 40, 1), (5, 2, 40, 0), (R.n - 1, 0, None, 1)]
    want = R.expect(segs)
    assert want.startswith(R.head[0] + b"/rc\n") and b"\n>:3-40/rc\n" in want
    assert run_select(gpu, d_naf, segs, FASTA) == want


# ---- 2. sub-ranges ---------------------------------------------------------------------------------------------------------------
def seeded_segments(rng, R, n):
    """The kinds of test_gpu_select.seeded_segments -- odd and even begins and ends, length 1, ends beyond the record, repeats and
    overlaps, whole records -- and lengths 2 .. 17 at every phase of a byte and of a 16-base chunk."""
    live = [r for r in range(R.n) if len(R.bases[r])]
    segs = []
    while len(segs) < n:
        r = int(live[rng.integers(0, len(live))]); ln = len(R.bases[r])
        kind = rng.integers(0, 10)
        b = int(rng.integers(0, ln))
        if kind == 0:
            segs.append((r, b, b + 1))
        elif kind == 1:
            segs.append((r, b, ln + int(rng.integers(1, 1000))))                       # clamped
        elif kind == 2:
            segs.append(r)
        elif kind == 3 and segs:
            segs.append(segs[int(rng.integers(0, len(segs)))])                          # a repeat
        elif kind == 4:
            segs.append((r, b | 1 if (b | 1) < ln else b, ln))                          # odd begin: a low nibble
        elif kind in (5, 6):
            e = min(ln, b + 1 + int(rng.integers(0, min(ln, 5000))))
            segs.append((r, b, e))
            if kind == 5 and e - b > 2:
                segs.append((r, b + (e - b) // 2, min(ln, e + 7)))                      # overlaps the previous one
        elif kind == 7:
            segs.append((r, b, min(ln, b + int(rng.integers(2, 18)))))                  # lengths 2 .. 17
        elif kind == 8:
            e = int(rng.integers(1, ln + 1)); segs.append((r, max(0, e - int(rng.integers(2, 18))), e))      # the same, placed by their ends
        else:
            e = min(ln, (b | 1) + 1 + 2 * int(rng.integers(0, 40))) ; segs.append((r, min(b | 1, e - 1), e))   # odd begin, odd or even end
    return segs[:n]


def toggle_crossers(R, Rn):
    """Segments around every change of case of the masked text (R: masked, Rn: the same records unmasked): the toggles."""
    segs = []
    for r in range(R.n):
        s = R.bases[r]
        for k in range(1, len(s)):
            if s[k - 1:k].islower() != s[k:k + 1].islower() and len(segs) < 400:
                segs += [(r, max(0, k - 3), min(len(s), k + 2)), (r, max(0, k - 17), min(len(s), k + 18)), (r, k, min(len(s), k + 16)), (r, max(0, k - 16), k)]
    return segs


@pytest.mark.parametrize("name", SUB_CASES)
def test_sub_ranges_on_both_strands(gpu, oracle, name):
    naf = golden_bytes("naf", name + ".naf")
    d_naf = gpu.to_device(naf)
    rng = np.random.default_rng(1200 + SEED)
    n_reverse = 0
    for mode, use_mask, ll in [(FASTA, True, -1), (FASTA, True, 0), (FASTA, False, 1), (FASTA, True, 1), (FASTA, True, 13), (SEQUENCES, True, -1), (SEQ, True, -1), (SEQ, False, -1)]:
        R = Records(oracle, naf, mode, use_mask, ll)
        base = seeded_segments(rng, R, 60 if ll == 1 else 300)
        if name == "mask_bounds" and use_mask:
            base += toggle_crossers(R, None)
        if ll == 1:
            base = [s if isinstance(s, int) or s[2] - s[1] < 3000 else (s[0], s[1], s[1] + 3000) for s in base]
        segs = []
        for s in base:                                                                   # every segment once forward and once reverse, interleaved
            segs += [norm(s, 0), norm(s, 1)]
        assert run_select(gpu, d_naf, segs, mode, use_mask, ll) == R.expect(segs), (mode, use_mask, ll)
        assert select_size(gpu, d_naf, segs, mode, use_mask, ll) == len(R.expect(segs))
        for s in base[:12]:
            assert run_select(gpu, d_naf, [norm(s, 1)], mode, use_mask, ll) == R.expect([norm(s, 1)]), (mode, use_mask, ll, s)
        n_reverse += len(base)
    assert n_reverse >= 200


def test_mask_bounds_has_toggles_inside_the_segments(oracle):
    R = Records(oracle, golden_bytes("naf", "mask_bounds.naf"), FASTA)
    assert len(toggle_crossers(R, None)) >= 8


# ---- 3. strand = NULL and all zeros are naf_gpu_unnaf_select ---------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("mixed_60", FASTA), ("mixed_60", SEQ), ("fastq_var", FASTQ), ("protein_small", FASTA), ("rna_small", SEQUENCES)])
def test_no_strand_and_all_zeros_give_the_bytes_of_select(gpu, oracle, name, mode):
    import torch
    from naf_amd import capi
    naf = golden_bytes("naf", name + ".naf")
    d_naf = gpu.to_device(naf)
    n_rec = oracle.parse_naf(naf).n_sequences
    lens = [len(x) for x in oracle.unnaf(naf, SEQUENCES).split(b"\n")[:-1]]
    segs = list(range(n_rec - 1, -1, -1))
    if mode != FASTQ:
        segs += [(r, 1, max(2, lens[r] // 2)) for r in range(n_rec) if lens[r] >= 2]
    want = host(gpu.unnaf_select(d_naf, segs, mode))
    assert want
    arr = gpu._segments(segs)
    o = capi.UnnafOpts(mode, 1, -1)
    for strand in (None, (C.c_uint8 * len(segs))()):
        n = C.c_size_t()
        assert gpu.L.naf_gpu_unnaf_select_stranded_size(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), C.byref(o), arr, strand, len(segs), C.byref(n)) == 0
        assert n.value == len(want)
        out = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        assert gpu.L.naf_gpu_unnaf_select_stranded(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), C.byref(o), arr, strand, len(segs), C.c_void_p(out.data_ptr()), out.numel(), C.byref(n)) == 0
        assert host(out[:n.value]) == want
    # 4-tuples with reverse = 0 through the binding
    assert host(gpu.unnaf_select(d_naf, [(s, 0, capi.WHOLE, 0) if isinstance(s, int) else (*s, 0) for s in segs], mode)) == want


# ---- 4. size ------------------------------------------------------------------------------------------------------------------
def traced_select(gpu, d_naf, segs, mode, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    got = run_select(gpu, d_naf, segs, mode)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = re.findall(r"\[select\] segments (\d+) ranges (\d+) sequence bytes decoded (\d+) of (\d+) side sections (\d+)\n", err)
    assert len(m) == 1, err
    return got, [int(x) for x in m[0]]


def test_reverse_regions_of_a_256_mb_genome_decode_only_their_blocks(gpu, oracle, monkeypatch, capfd):
    from naf_amd import synth
    t = synth.realistic_genome_device(256 << 20, device="cuda")
    d_naf, _ = gpu.ennaf(t)
    d_naf = d_naf.clone()
    naf = host(d_naf)
    del t
    R = Records(oracle, naf, FASTA)
    assert R.n == 24
    rng = np.random.default_rng(1400 + SEED)
    b3 = int(rng.integers(0, len(R.bases[3]) - 1_000_000))
    scattered = []
    for k in range(20):
        r = (k * 7 + SEED) % R.n
        b = int(rng.integers(0, len(R.bases[r]) - 10_000))
        scattered.append((r, b, b + 10_000, 1))
    for segs in ([(3, b3, b3 + 1_000_000, 1)], scattered):
        got, (K, ranges, D, T, side) = traced_select(gpu, d_naf, segs, FASTA, monkeypatch, capfd)
        assert got == R.expect(segs)
        stream = sum((s[2] - s[1] + 1) // 2 + 1 for s in segs)
        assert side == 1 and K == len(segs) and ranges <= K
        assert D <= stream + 4 * 131072 * K, (D, stream, K)                              # the bound of the forward test
        assert D < T
        fwd, (K2, ranges2, D2, T2, side2) = traced_select(gpu, d_naf, [s[:3] + (0,) for s in segs], FASTA, monkeypatch, capfd)
        assert (K2, ranges2, D2, T2, side2) == (K, ranges, D, T, side)                   # a reverse segment decodes the blocks of its forward twin
        assert fwd == R.expect([s[:3] + (0,) for s in segs])


def test_reverse_reads_of_a_64_mb_read_set(gpu, oracle, monkeypatch, capfd):
    from naf_amd import synth
    t = synth.fastq_reads_device(64 << 20, device="cuda")
    d_naf, _ = gpu.ennaf(t)
    d_naf = d_naf.clone()
    naf = host(d_naf)
    del t
    R = Records(oracle, naf, FASTQ)
    assert R.n >= 200_000
    segs = [(r, 0, None, 1) for r in range(100_000, 200_000)]
    got, (K, ranges, D, T, side) = traced_select(gpu, d_naf, segs, FASTQ, monkeypatch, capfd)
    assert got == R.expect(segs)
    stream = sum((len(R.bases[r]) + 1) // 2 + 1 for r in range(100_000, 200_000))
    assert side == 1 and K == 100_000 and ranges == 1
    assert D <= stream + 4 * 131072 * K and D < T


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_segment_and_leave_the_context_usable(gpu, oracle):
    from naf_amd import capi
    naf = golden_bytes("naf", "mixed_60.naf")
    d_naf = gpu.to_device(naf)
    R = Records(oracle, naf, FASTA)
    d_fq = gpu.to_device(golden_bytes("naf", "fastq_var.naf"))
    d_prot = gpu.to_device(golden_bytes("naf", "protein_small.naf"))
    d_text = gpu.to_device(golden_bytes("naf", "text_small.naf"))
    W = capi.WHOLE
    for d, segs, mode, words in [(d_prot, [(0, 0, W, 0), (1, 0, W, 1)], FASTA, ("segment 1", "no reverse complement")),
                                 (d_text, [(0, 0, W, 0), (0, 0, 3, 0), (1, 1, 4, 1)], SEQ, ("segment 2", "no reverse complement")),
                                 (d_naf, [(0, 0, W, 1), (1, 0, W, 2)], FASTA, ("segment 1", "strand")),
                                 (d_fq, [(0, 0, W, 1), (2, 0, W, 0), (1, 2, 5, 1)], FASTQ, ("segment 2", "FASTQ")),
                                 (d_naf, [(0, 0, W, 1), (R.n, 0, W, 1)], FASTA, ("segment 1",)),
                                 (d_naf, [(1, 5, 5, 1)], SEQUENCES, ("segment 0",))]:
        with pytest.raises(capi.NafGpuError) as ei:
            gpu.unnaf_select(d, segs, mode)
        assert ei.value.code == E_ARG and all(w in ei.value.msg for w in words), ei.value.msg
        with pytest.raises(capi.NafGpuError) as ei:
            gpu.unnaf_select_size(d, segs, mode)
        assert ei.value.code == E_ARG and all(w in ei.value.msg for w in words), ei.value.msg
        ok = [(2, 0, None, 1), (3, 10, 500, 1), (3, 10, 500, 0)]                          # a following valid call on the same context
        assert run_select(gpu, d_naf, ok, FASTA) == R.expect(ok)
    assert host(gpu.unnaf(d_naf, FASTA)) == oracle.unnaf(naf, FASTA)
    assert host(gpu.unnaf_select(d_prot, [(1, 0, W, 0)], FASTA)) == host(gpu.unnaf_select(d_prot, [1], FASTA)) != b""


# ---- 6. command line -------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_rc_region_and_revcomp(gpu, oracle):
    naf = golden_bytes("naf", "mixed_60.naf")
    R = Records(oracle, naf, FASTA)
    ids = [i.decode() for i in R.ids]
    a, b = 101, min(2500, len(R.bases[4]))
    reg = "%s:%d-%d" % (ids[4], a, b)
    # the three selecting options mixed, in command-line order
    p = unnaf_cli(["--fasta", "--region", reg, "--rc-region", reg, "--records", "2-3", "--rc-region", ids[2], "--region", ids[2]], naf)
    assert p.returncode == 0 and p.stderr == b""
    assert p.stdout == R.expect([(4, a - 1, b, 0), (4, a - 1, b, 1), (1, 0, None, 0), (2, 0, None, 0), (2, 0, None, 1), (2, 0, None, 0)])
    # --revcomp: the whole text reversed record by record
    p = unnaf_cli(["--revcomp", "--records", "1-%d" % R.n], naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == R.expect([(r, 0, None, 1) for r in range(R.n)])
    # ... an --rc-region stays reverse, a --region becomes one; other options as for forward segments
    R13 = Records(oracle, naf, FASTA, False, 13)
    p = unnaf_cli(["--rc-region", reg, "--revcomp", "--region", ids[0] + ":7-19", "--line-length", "13", "--no-mask"], naf)
    assert p.returncode == 0 and p.stdout == R13.expect([(4, a - 1, b, 1), (0, 6, 19, 1)])
    Rs = Records(oracle, naf, SEQ)
    p = unnaf_cli(["--seq", "--rc-region", ids[0] + ":7-19", "--region", ids[0] + ":7"], naf)
    assert p.returncode == 0 and p.stdout == Rs.expect([(0, 6, 19, 1), (0, 6, 7, 0)])
    fq = golden_bytes("naf", "fastq_var.naf")
    Rq = Records(oracle, fq, FASTQ)
    p = unnaf_cli(["--fastq", "--revcomp", "--records", "3-7", "--region", Rq.ids[0].decode()], fq)
    assert p.returncode == 0 and p.stdout == Rq.expect([(r, 0, None, 1) for r in (2, 3, 4, 5, 6, 0)])
    # a protein archive has no reverse complement: said before anything is written
    prot = golden_bytes("naf", "protein_small.naf")
    pid = oracle.zstd_decompress(oracle.parse_naf(prot).frame(prot, 0)).split(b"\0")[0].decode()
    for args in (["--rc-region", pid], ["--revcomp", "--records", "1"]):
        p = unnaf_cli(args, prot)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"unnaf error: protein sequences have no reverse complement\n"
    p = unnaf_cli(["--region", pid], prot)
    assert p.returncode == 0 and p.stdout.startswith(b">" + pid.encode())
