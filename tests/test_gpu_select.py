"""GPU tests of the selection path (naf_gpu_unnaf_find / _record_table / _select, unnaf --region / --records).  Expected bytes never
come from the code under test: they are cut in Python out of the oracle's whole text of the same archive (records split, line ends
stripped, [begin, end) sliced, re-wrapped, the header of include/naf_gpu.h written).  All comparisons are byte-exact."""
import os
import re
import subprocess

import numpy as np
import pytest

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))          # other choices of the same kinds: NAF_TEST_SEED=n python -m pytest ...

from conftest import ROOT, golden_bytes, naf_cases

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
FASTA, FASTQ, SEQ, SEQUENCES, FOURBIT = 0, 1, 2, 3, 4
E_ARG, E_CAP = -8, -6


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


# ---- the expectation, from the oracle's whole text ----------------------------------------------------------------------------
class Records:
    """The records of an archive as the oracle prints them under (mode, use_mask, line_length)."""

    def __init__(self, oracle, naf, mode, use_mask=True, line_length=-1):
        h = oracle.parse_naf(naf)
        self.mode, self.fastq = mode, bool(h.flags & 1)
        self.L = line_length if line_length >= 0 else h.line_length
        self.ids = oracle.zstd_decompress(h.frame(naf, 0)).split(b"\0")[:-1] if h.flags & 0x20 else [b""] * h.n_sequences
        text_mode = FASTQ if mode == FASTQ else FASTA if mode == FASTA else SEQUENCES
        self.text = oracle.unnaf(naf, text_mode, use_mask, line_length)
        self.whole, self.bases = [], []
        t = self.text
        if mode == FASTQ:
            lines = t.split(b"\n")[:-1]
            assert len(lines) == 4 * h.n_sequences
            for k in range(0, len(lines), 4):
                self.whole.append(b"\n".join(lines[k:k + 4]) + b"\n"); self.bases.append(lines[k + 1])
        elif mode == FASTA:
            # a text archive may hold '>' at a line start, so the records are walked by the lengths of the oracle's --sequences lines
            lens = [len(x) for x in oracle.unnaf(naf, SEQUENCES, use_mask, line_length).split(b"\n")[:-1]]
            assert len(lens) == h.n_sequences
            a = 0
            for ln in lens:
                assert t[a:a + 1] == b">"
                body = t.index(b"\n", a) + 1
                b = body + (0 if ln == 0 else ln + ((ln + self.L - 1) // self.L if self.L else 1))
                rec = t[a:b]
                self.whole.append(rec); self.bases.append(t[body:b].replace(b"\n", b"")); a = b
                assert len(self.bases[-1]) == ln and rec.endswith(b"\n")
            assert a == len(t)
        else:
            lines = t.split(b"\n")[:-1]
            assert len(lines) == h.n_sequences
            for ln in lines:
                self.bases.append(ln); self.whole.append(ln + (b"\n" if mode == SEQUENCES else b""))
            if mode == SEQ:
                assert b"".join(lines) == oracle.unnaf(naf, SEQ, use_mask, line_length)
        self.n = len(self.whole)

    def segment(self, rec, begin=0, end=None):
        if begin == 0 and end is None:
            return self.whole[rec]
        s = self.bases[rec][begin:min(end, len(self.bases[rec]))]
        assert s, "the test asks for an empty sub-range"
        if self.mode == SEQ:
            return s
        if self.mode == SEQUENCES:
            return s + b"\n"
        assert self.mode == FASTA
        hdr = b">" + self.ids[rec] + b":%d-%d\n" % (begin + 1, begin + len(s))
        if self.L == 0:
            return hdr + s + b"\n"
        return hdr + b"".join(s[i:i + self.L] + b"\n" for i in range(0, len(s), self.L))

    def expect(self, segs):
        return b"".join(self.segment(*((s,) if isinstance(s, int) else s)) for s in segs)


def seg_arg(s):
    from naf_amd import capi
    return s if isinstance(s, int) else (s[0], s[1], capi.WHOLE if s[2] is None else s[2])


def run_select(gpu, d_naf, segs, mode, use_mask=True, line_length=-1):
    return host(gpu.unnaf_select(d_naf, [seg_arg(s) for s in segs], mode, use_mask, line_length))


def modes_of(h):
    return [FASTQ if h.flags & 1 else FASTA, SEQUENCES, SEQ]


# ---- 1. whole records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", naf_cases(), ids=lambda c: c["name"])
def test_whole_records_alone_and_all_in_reverse(gpu, oracle, case):
    naf = golden_bytes("naf", case["name"] + ".naf")
    h = oracle.parse_naf(naf)
    if h.n_sequences == 0:
        pytest.skip("no records")
    d_naf = gpu.to_device(naf)
    rng = np.random.default_rng(100 + SEED)
    for mode in modes_of(h):
        for use_mask in (True, False):
            for ll in (-1, 0, 13):
                R = Records(oracle, naf, mode, use_mask, ll)
                alone = range(R.n) if R.n <= 40 else sorted(set([0, R.n - 1] + list(rng.integers(0, R.n, 30))))
                for r in alone:
                    assert run_select(gpu, d_naf, [int(r)], mode, use_mask, ll) == R.whole[r], (mode, use_mask, ll, r)
                rev = list(range(R.n - 1, -1, -1))
                assert run_select(gpu, d_naf, rev, mode, use_mask, ll) == R.expect(rev), (mode, use_mask, ll)
                assert gpu.unnaf_select_size(d_naf, rev, mode, use_mask, ll) == len(R.expect(rev))


# ---- 2. / 3. sub-ranges ----------------------------------------------------------------------------------------------------------
def seeded_segments(rng, R, n):
    """Odd and even begins, length 1, ends beyond the record, repeats and overlaps, whole records among them."""
    live = [r for r in range(R.n) if len(R.bases[r])]
    segs = []
    while len(segs) < n:
        r = int(live[rng.integers(0, len(live))]); ln = len(R.bases[r])
        kind = rng.integers(0, 8)
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
        else:
            e = min(ln, b + 1 + int(rng.integers(0, min(ln, 5000))))
            segs.append((r, b, e))
            if kind == 5 and e - b > 2:
                segs.append((r, b + (e - b) // 2, min(ln, e + 7)))                      # overlaps the previous one
    return segs[:n]


SUB_CASES = ["mixed_60", "mask_bounds", "acgt_odd", "acgt_1m2", "rna_small", "protein_small", "text_small", "ll_override", "tiny_many", "repeat_l19", "repeat_long27"]


@pytest.mark.parametrize("name", SUB_CASES)
def test_sub_ranges(gpu, oracle, name, monkeypatch, capfd):
    naf = golden_bytes("naf", name + ".naf")
    d_naf = gpu.to_device(naf)
    rng = np.random.default_rng(200 + SEED)
    n_checked = 0
    for mode, use_mask, ll in [(FASTA, True, -1), (FASTA, True, 0), (FASTA, False, 1), (FASTA, True, 13), (SEQUENCES, True, -1), (SEQ, True, -1), (SEQ, False, -1)]:
        R = Records(oracle, naf, mode, use_mask, ll)
        segs = seeded_segments(rng, R, 60 if ll == 1 else 300)
        if ll == 1:
            segs = [s if isinstance(s, int) or s[2] - s[1] < 3000 else (s[0], s[1], s[1] + 3000) for s in segs]
        assert run_select(gpu, d_naf, segs, mode, use_mask, ll) == R.expect(segs), (mode, use_mask, ll)
        for s in segs[:12]:
            assert run_select(gpu, d_naf, [s], mode, use_mask, ll) == R.expect([s]), (mode, use_mask, ll, s)
        n_checked += len(segs)
    assert n_checked >= 200
    if name.startswith("repeat_l"):
        # frames with dependent blocks: whatever the decoder takes (closure or the whole stream), one pass over the side sections
        R = Records(oracle, naf, FASTA)
        monkeypatch.setenv("NAF_GPU_TRACE", "1")
        capfd.readouterr()
        ln = len(R.bases[R.n - 1])
        got = run_select(gpu, d_naf, [(R.n - 1, ln - 1000, ln)], FASTA)
        err = capfd.readouterr().err
        monkeypatch.delenv("NAF_GPU_TRACE")
        assert got == R.expect([(R.n - 1, ln - 1000, ln)])
        assert re.search(r"\[select\] segments 1 ranges 1 sequence bytes decoded \d+ of \d+ side sections 1\n", err), err


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


def test_regions_of_a_256_mb_genome_decode_only_their_blocks(gpu, oracle, monkeypatch, capfd):
    from naf_amd import synth
    t = synth.realistic_genome_device(256 << 20, device="cuda")
    d_naf, _ = gpu.ennaf(t)
    d_naf = d_naf.clone()
    naf = host(d_naf)
    del t
    R = Records(oracle, naf, FASTA)
    assert R.n == 24
    rng = np.random.default_rng(400 + SEED)
    b3 = int(rng.integers(0, len(R.bases[3]) - 1_000_000))
    scattered = []
    for k in range(20):
        r = (k * 7 + SEED) % R.n
        b = int(rng.integers(0, len(R.bases[r]) - 10_000))
        scattered.append((r, b, b + 10_000))
    for segs in ([17], [(3, b3, b3 + 1_000_000)], scattered):
        got, (K, ranges, D, T, side) = traced_select(gpu, d_naf, segs, FASTA, monkeypatch, capfd)
        assert got == R.expect(segs)
        stream = sum((len(R.segment(*((s,) if isinstance(s, int) else s)).split(b"\n", 1)[1].replace(b"\n", b"")) + 1) // 2 + 1 for s in segs)
        assert side == 1 and K == len(segs) and ranges <= K
        assert D <= stream + 4 * 131072 * K, (D, stream, K)
        assert D < T


def test_a_range_of_reads_of_a_64_mb_read_set(gpu, oracle, monkeypatch, capfd):
    from naf_amd import synth
    t = synth.fastq_reads_device(64 << 20, device="cuda")
    d_naf, _ = gpu.ennaf(t)
    d_naf = d_naf.clone()
    naf = host(d_naf)
    del t
    R = Records(oracle, naf, FASTQ)
    assert R.n >= 200_000
    segs = list(range(100_000, 200_000))
    got, (K, ranges, D, T, side) = traced_select(gpu, d_naf, segs, FASTQ, monkeypatch, capfd)
    assert got == b"".join(R.whole[100_000:200_000])
    stream = sum((len(R.bases[r]) + 1) // 2 + 1 for r in segs)
    assert side == 1 and K == 100_000 and ranges == 1
    assert D <= stream + 4 * 131072 * K and D < T


def test_reads_of_a_fastq_archive_whose_blocks_depend_on_each_other(gpu, oracle, monkeypatch, capfd):
    """repeat_fastq_l19 (tests/golden/make_golden.py: 71 reads of 30 000 bases, the reference's -19): the last block of its sequence frame
    reaches back to the first (offsets up to 1 032 831 in a stream of 1 052 885 bytes), so the range of a read at the end cannot be had
    alone.  The call then gives up every range, the one of read 5 that could, and decodes sequence AND quality whole, once: one range,
    D == T, and the bytes of the whole decode."""
    naf = golden_bytes("naf", "repeat_fastq_l19.naf")
    d_naf = gpu.to_device(naf)
    R = Records(oracle, naf, FASTQ)
    assert R.n == 71 and host(gpu.unnaf(d_naf, FASTQ)) == R.text
    for segs in ([5, R.n - 1, R.n - 3], [R.n - 2]):
        got, (K, ranges, D, T, side) = traced_select(gpu, d_naf, segs, FASTQ, monkeypatch, capfd)
        assert got == R.expect(segs)
        assert (K, ranges, side) == (len(segs), 1, 1) and D == T == (sum(len(b) for b in R.bases) + 1) // 2


# ---- 5. find -------------------------------------------------------------------------------------------------------------------
def ids_of(oracle, naf):
    h = oracle.parse_naf(naf)
    return oracle.zstd_decompress(h.frame(naf, 0)).split(b"\0")[:-1]


def first_index(ids):
    d = {}
    for k, i in enumerate(ids):
        d.setdefault(i, k)
    return d


@pytest.mark.parametrize("name", ["tiny_many", "fastq_4k"])
def test_find_every_id_shuffled(gpu, oracle, name):
    naf = golden_bytes("naf", name + ".naf")
    ids = ids_of(oracle, naf)
    want = first_index(ids)
    rng = np.random.default_rng(500 + SEED)
    q = [ids[k] for k in rng.permutation(len(ids))] + [b"no such id", b"", ids[0] + b"x", ids[0][:-1]]
    got = gpu.unnaf_find(gpu.to_device(naf), q)
    assert got == [want.get(i) for i in q]
    assert gpu.unnaf_find(gpu.to_device(naf), []) == []


def test_find_prefixes_duplicates_and_long_ids(gpu, oracle):
    long_a, long_b = b"L" * 5000 + b"a", b"L" * 5000 + b"b"
    names = [b"chr1", b"chr10", b"chr1 with a comment", b"dup", b"chr2", b"dup second", long_a.decode().encode() + b" c", long_b, b"dup", b"x" * 33, b"x" * 32, b"x" * 31]
    text = b"".join(b">" + n + b"\nACGTNACGTTGCA\n" for n in names)
    d_naf, _ = gpu.ennaf(gpu.to_device(text))
    naf = host(d_naf)
    ids = ids_of(oracle, naf)
    assert ids == [n.split(b" ")[0] for n in names]
    want = first_index(ids)
    q = [b"chr1", b"chr10", b"chr", b"chr100", b"dup", b"dup", long_a, long_b, b"L" * 5000, b"L" * 5001, b"x" * 33, b"x" * 32, b"x" * 31, b"x" * 30, b"chr2"]
    assert gpu.unnaf_find(d_naf, q) == [want.get(i) for i in q]
    assert want[b"chr1"] == 0 and want[b"dup"] == 3
    # a region by name through the whole path
    R = Records(oracle, naf, FASTA)
    rec = gpu.unnaf_find(d_naf, ["chr10"])[0]
    assert run_select(gpu, d_naf, [(rec, 2, 9)], FASTA) == R.expect([(1, 2, 9)]) == b">chr10:3-9\nGTNACGT\n"


def test_find_a_thousand_ids_among_two_million_reads(gpu, oracle):
    from naf_amd import synth
    t = synth.fastq_reads_device(2_000_000 * 330, device="cuda")
    d_naf, rep = gpu.ennaf(t)
    d_naf = d_naf.clone()
    del t
    naf = host(d_naf)
    ids = ids_of(oracle, naf)
    assert len(ids) >= 1_900_000
    want = first_index(ids)
    rng = np.random.default_rng(550 + SEED)
    q = [ids[int(k)] for k in rng.integers(0, len(ids), 1000)] + [b"read0", b"readX"]
    assert gpu.unnaf_find(d_naf, q) == [want.get(i) for i in q]


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_segment_and_leave_the_context_usable(gpu, oracle):
    import torch
    from naf_amd import capi
    naf = golden_bytes("naf", "mixed_60.naf")
    d_naf = gpu.to_device(naf)
    R = Records(oracle, naf, FASTA)
    fq = golden_bytes("naf", "fastq_var.naf")
    d_fq = gpu.to_device(fq)
    ln1 = len(R.bases[1])
    for d, segs, mode, word in [(d_naf, [0], FOURBIT, "4-bit"), (d_fq, [0, (1, 2, 5)], FASTQ, "segment 1"), (d_naf, [0, 1, R.n], FASTA, "segment 2"),
                                (d_naf, [(1, 5, 5)], FASTA, "segment 0"), (d_naf, [0, (1, ln1, ln1 + 5)], SEQ, "segment 1"), (d_naf, [(1, 9, 3)], SEQUENCES, "segment 0")]:
        with pytest.raises(capi.NafGpuError) as ei:
            run_select(gpu, d, segs, mode)
        assert ei.value.code == E_ARG and word in ei.value.msg, ei.value.msg
        with pytest.raises(capi.NafGpuError) as ei:
            gpu.unnaf_select_size(d, [seg_arg(s) for s in segs], mode)
        assert ei.value.code == E_ARG
    segs = [2, (3, 10, 500)]
    need = gpu.unnaf_select_size(d_naf, segs, FASTA)
    assert need == len(R.expect(segs))
    small = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    import ctypes as C
    o = capi.UnnafOpts(FASTA, 1, -1)
    n = C.c_size_t()
    rc = gpu.L.naf_gpu_unnaf_select(gpu.h, C.c_void_p(d_naf.data_ptr()), d_naf.numel(), C.byref(o), gpu._segments(segs), 2, C.c_void_p(small.data_ptr()), small.numel(), C.byref(n))
    assert rc == E_CAP and n.value == need
    assert run_select(gpu, d_naf, [], FASTA) == b"" and gpu.unnaf_select_size(d_naf, [], FASTA) == 0
    assert host(gpu.unnaf(d_naf, FASTA)) == oracle.unnaf(naf, FASTA)
    assert host(gpu.unnaf(d_fq, FASTQ)) == oracle.unnaf(fq, FASTQ)


# ---- 7. record table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_60", "tiny_many", "fastq_var", "protein_small"])
def test_record_table_feeds_unnaf_range(gpu, oracle, name):
    naf = golden_bytes("naf", name + ".naf")
    d_naf = gpu.to_device(naf)
    h = oracle.parse_naf(naf)
    lens = [len(x) for x in oracle.unnaf(naf, SEQUENCES).split(b"\n")[:-1]]
    for mode in modes_of(h):
        R = Records(oracle, naf, mode)
        nb, off = gpu.unnaf_record_table(d_naf, 0, None, mode)
        assert nb == lens and len(off) == R.n + 1 and off[0] == 0
        for r in sorted(set([0, R.n // 2, R.n - 1])):
            assert host(gpu.unnaf_range(d_naf, off[r], off[r + 1], mode)) == R.whole[r] if off[r + 1] > off[r] else R.whole[r] == b""
        first, count = R.n // 3, min(5, R.n - R.n // 3)
        nb2, off2 = gpu.unnaf_record_table(d_naf, first, count, mode)
        assert nb2 == lens[first:first + count] and off2 == off[first:first + count + 1]
    from naf_amd import capi
    with pytest.raises(capi.NafGpuError):
        gpu.unnaf_record_table(d_naf, 1, h.n_sequences, FASTA)


# ---- 8. command line -------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_regions_and_records(gpu, oracle, tmp_path):
    naf = golden_bytes("naf", "mixed_60.naf")
    R = Records(oracle, naf, FASTA)
    ids = [i.decode() for i in R.ids]
    a, b = 101, min(2500, len(R.bases[4]))
    p = unnaf_cli(["--fasta", "--region", "%s:%d-%d" % (ids[4], a, b), "--region", ids[2]], naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == R.expect([(4, a - 1, b), 2])
    p = unnaf_cli(["--records", "2-3"], naf)
    assert p.returncode == 0 and p.stdout == R.expect([1, 2])
    big = max(range(R.n), key=lambda r: len(R.bases[r]))
    assert len(R.bases[big]) > 1001
    p = unnaf_cli(["--region", ids[big] + ":1,001-", "--records", "1", "--line-length", "13", "--no-mask"], naf)
    R13 = Records(oracle, naf, FASTA, False, 13)
    assert p.returncode == 0 and p.stdout == R13.expect([(big, 1000, len(R13.bases[big])), 0])
    Rs = Records(oracle, naf, SEQ)
    p = unnaf_cli(["--seq", "--region", ids[0] + ":7-19", "--region", ids[0] + ":7"], naf)
    assert p.returncode == 0 and p.stdout == Rs.expect([(0, 6, 19), (0, 6, 7)])
    # pieces of whole segments when the selection is larger than the range buffer; to a file
    out = tmp_path / "sel.fa"
    f = tmp_path / "in.naf"
    f.write_bytes(naf)
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--fasta", "--records", "1-%d" % R.n, "--region", ids[3], "-o", str(out), str(f)],
                       env=dict(os.environ, NAF_GPU_RANGE_BYTES="8192"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and out.read_bytes() == R.text + R.whole[3]
    # an id that is not there: nothing written
    p = unnaf_cli(["--fasta", "--region", ids[0], "--region", "nosuch:1-5"], naf)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == b'unnaf error: sequence "nosuch" not found\n'
    p = unnaf_cli(["--records", "%d" % (R.n + 1)], naf)
    assert p.returncode == 1 and p.stdout == b""
    fq = golden_bytes("naf", "fastq_var.naf")
    Rq = Records(oracle, fq, FASTQ)
    p = unnaf_cli(["--fastq", "--records", "3-7", "--records", "1"], fq)
    assert p.returncode == 0 and p.stdout == Rq.expect([2, 3, 4, 5, 6, 0])
    p = unnaf_cli(["--region", Rq.ids[5].decode()], fq)
    assert p.returncode == 0 and p.stdout == Rq.whole[5]
