"""GPU tests of the motif search (naf_gpu_unnaf_locate_count, naf_gpu_unnaf_locate, unnaf --locate).  Expected hits never come from the
code under test: they are what locate_plan.expected_hits -- look-ahead regexes per record -- finds in the oracle's --sequences text of the
same archive.  Every planned text is searched in two archives, the oracle's and this library's own ennaf at level 1; the reference-made
golden archives repeat_l19 and repeat_long27 (frames whose blocks depend on each other) are searched for pieces of their own text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import locate_plan as LP
from conftest import ROOT, golden_bytes

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))
pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "naf_amd", "bin")
E_CAP, E_ARG = -6, -8
SEQ, SEQUENCES = 2, 3
CASES = [c.name for c in LP.planned(0)]
GOLDEN_REPEATS = ("repeat_l19", "repeat_long27")


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
        self.records = LP.records_from_sequences_text(oracle.unnaf(naf, oracle.MODE_SEQUENCES, False), self.h.n_sequences)
        self.d_naf = gpu.to_device(naf)
        self._want = {}

    def want(self, patterns, strands, first=0, count=None):
        """expected_hits, computed once per question and left unchanged"""
        key = (tuple(patterns), strands, first, count)
        if key not in self._want:
            self._want[key] = LP.expected_hits(self.records, patterns, strands, first, count)
        return self._want[key]


@pytest.fixture(scope="module")
def planned(oracle, gpu):
    """name -> (case, {"oracle": Archive, "own": Archive}); the two archives of a text hold the same records"""
    out = {}
    for c in LP.planned(SEED):
        a = Archive(oracle, gpu, oracle.ennaf(c.text, c.seq_type))
        own, _ = gpu.ennaf(gpu.to_device(c.text), seq_type=c.seq_type, level=1)
        b = Archive(oracle, gpu, own.cpu().numpy().tobytes())
        assert a.records == b.records and (c.r7 or a.records == c.records_upper), c.name
        b._want = a._want
        out[c.name] = (c, {"oracle": a, "own": b})
    return out


@pytest.fixture(scope="module")
def repeats(oracle, gpu):
    out = {}
    for name in GOLDEN_REPEATS:
        a = Archive(oracle, gpu, golden_bytes("naf", name + ".naf"))
        big = max(range(len(a.records)), key=lambda r: len(a.records[r]))
        t = a.records[big]
        assert len(t) > 1000
        pats = [t[100:132], t[len(t) // 2:len(t) // 2 + 17], t[-20:], LP.revcomp(t[5:30]), "NGG", "GAATTC"]
        out[name] = (a, pats, big)
    return out


def tuples(hits):
    return [tuple(row) for row in table(hits).tolist()]


def table(hits):
    return np.stack([hits[f].astype(np.int64) for f in ("record", "begin", "pattern", "strand")], axis=1) if len(hits) else np.zeros((0, 4), dtype=np.int64)


def check_query(gpu, A, patterns, strands, first, count):
    want = A.want(patterns, strands, first, count)
    hits, total = gpu.unnaf_locate(A.d_naf, patterns, strands, first, count)
    assert total == len(want)
    if not np.array_equal(table(hits), np.asarray(want, dtype=np.int64).reshape(-1, 4)):
        got = tuples(hits)
        k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        raise AssertionError("first difference at hit %d: got %s, expected %s (%d / %d hits)" % (k, got[k:k + 3], want[k:k + 3], len(got), len(want)))
    n, per = gpu.unnaf_locate_count(A.d_naf, patterns, strands, first, count)
    assert n == len(want)
    sums = [[0, 0] for _ in patterns]
    for _, _, p, s in want:
        sums[p][s] += 1
    assert per == sums


# ---- 1, 2. the hit tables and the counts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["oracle", "own"])
@pytest.mark.parametrize("name", CASES)
def test_hits_and_counts_of_the_planned_texts(gpu, planned, name, which):
    c, arc = planned[name]
    n_hits = 0
    for patterns, strands, first, count in c.queries:
        check_query(gpu, arc[which], patterns, strands, first, count)
        n_hits += len(arc[which].want(patterns, strands, first, count))
    assert n_hits > 0


@pytest.mark.parametrize("name", GOLDEN_REPEATS)
def test_hits_in_the_reference_made_archives(gpu, repeats, name):
    A, pats, big = repeats[name]
    check_query(gpu, A, pats, 3, 0, None)
    assert all(any(p == k for _, _, p, _ in A.want(pats, 3)) for k in range(len(pats) - 1))       # (GAATTC may be absent)
    check_query(gpu, A, pats[:3], 1, big, 1)


# ---- 3. restricted searches decode what they need ---------------------------------------------------------------------------------------
def traced_locate(gpu, A, patterns, strands, first, count, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_TRACE", "1")
    capfd.readouterr()
    hits, total = gpu.unnaf_locate(A.d_naf, patterns, strands, first, count)
    err = capfd.readouterr().err
    monkeypatch.delenv("NAF_GPU_TRACE")
    m = re.findall(r"\[locate\] patterns (\d+) records (\d+)\.\.(\d+) pieces (\d+) sequence bytes decoded (\d+) of (\d+) hits (\d+)\n", err)
    # the binding counts, then takes the table: two calls with one verdict -- but for the bytes decoded when the search runs in pieces,
    # which the second call sweeps twice (once to know that the table fits, once to write it)
    assert len(m) == 2 and m[0][:4] + m[0][5:] == m[1][:4] + m[1][5:] and (m[0][4] == m[1][4] or int(m[0][3]) > 1), err
    return tuples(hits), [int(x) for x in m[0]]


def test_a_restricted_search_decodes_only_the_blocks_behind_its_records(gpu, planned, repeats, monkeypatch, capfd):
    c, arc = planned["planted_odd"]
    pats = [t for _, _, _, t in c.planted.patterns()][100:110]
    for first, count in ((1, 2), (3, 1), (9, 3)):
        for which in ("oracle", "own"):
            A = arc[which]
            got, (np_, r0, r1, pieces, D, T, H) = traced_locate(gpu, A, pats, 3, first, count, monkeypatch, capfd)
            assert got == A.want(pats, 3, first, count) and (np_, r0, r1, pieces, H) == (len(pats), first, first + count, 1, len(got))
            assert T == (A.h.orig[4] + 1) // 2
            if which == "own":
                assert D < T, (first, count, D, T)                                     # independent blocks: a range of them
    # the reference's frames: blocks that depend on each other.  The last record's blocks reach back to the first: the whole stream, once
    for name in GOLDEN_REPEATS:
        A, rp, big = repeats[name]
        last = max(r for r in range(len(A.records)) if A.records[r])
        got, (np_, r0, r1, pieces, D, T, H) = traced_locate(gpu, A, rp, 3, last, 1, monkeypatch, capfd)
        assert got == A.want(rp, 3, last, 1)
        print("%s: record %d of %d, sequence bytes decoded %d of %d" % (name, last, len(A.records), D, T))
        assert D == T, (name, D, T)


# ---- 4. the piece size does not show --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [1001, 4097, 33333])
def test_the_result_does_not_depend_on_the_piece_size(gpu, planned, repeats, piece, monkeypatch, capfd):
    monkeypatch.setenv("NAF_GPU_LOCATE_PIECE", str(piece))
    for name in ("planted_odd", "fastq_reads", "dense"):
        c, arc = planned[name]
        for patterns, strands, first, count in c.queries[-3:]:
            for which in ("oracle", "own"):
                check_query(gpu, arc[which], patterns, strands, first, count)
    c, arc = planned["fastq_reads"]
    patterns, strands, first, count = c.queries[0]
    got, tr = traced_locate(gpu, arc["own"], patterns, strands, first, count, monkeypatch, capfd)
    assert got == arc["own"].want(patterns, strands, first, count) and tr[3] > 1          # it was searched in pieces
    A, rp, big = repeats["repeat_l19"]
    check_query(gpu, A, rp, 3, 0, None)
    monkeypatch.delenv("NAF_GPU_LOCATE_PIECE")


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------------------
def raw_locate(gpu, A, patterns, strands, first, count, d_hits, cap):
    from naf_amd import capi
    blob = b"".join(p.encode() + b"\0" for p in patterns)
    n = C.c_uint64(12345)
    rc = gpu.L.naf_gpu_unnaf_locate(gpu.h, C.c_void_p(A.d_naf.data_ptr()), A.d_naf.numel(), blob, len(blob), len(patterns), strands, first,
                                    capi.WHOLE if count is None else count, C.c_void_p(d_hits.data_ptr() if d_hits is not None and d_hits.numel() else 0), cap, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("which", ["oracle", "own"])
def test_capacity(gpu, planned, which):
    import torch
    import fenced
    from naf_amd import capi
    arena = fenced.Arena("cuda", salt=0x5A, size=4 << 20)
    for name, qi, phase in (("dense", 1, 1), ("planted_even", 0, 0), ("fastq_reads", 1, 65), ("dense", 3, 8)):
        c, arc = planned[name]
        A = arc[which]
        patterns, strands, first, count = c.queries[qi]
        want = A.want(patterns, strands, first, count)
        n = len(want)
        assert n >= 2
        # one entry too few: the whole count, and nothing written
        arena.reset()
        out = arena.out(24 * (n - 1), phase)
        before = out.clone()
        rc, total = raw_locate(gpu, A, patterns, strands, first, count, out, n - 1)
        torch.cuda.synchronize()
        assert rc == E_CAP and total == n
        assert torch.equal(out, before)
        arena.check()
        # exactly enough: n entries and nothing behind them
        arena.reset()
        out = arena.out(24 * n, phase)
        rc, total = raw_locate(gpu, A, patterns, strands, first, count, out, n)
        torch.cuda.synchronize()
        assert rc == 0 and total == n
        arena.check()
        assert tuples(np.frombuffer(out.cpu().numpy().tobytes(), dtype=capi.HIT_DTYPE)) == want
    # the binding's own form with a caller's buffer
    c, arc = planned["dense"]
    patterns, strands, first, count = c.queries[1]
    want = arc[which].want(patterns, strands, first, count)
    buf = torch.zeros(24 * len(want) + 24, dtype=torch.uint8, device="cuda")
    view, total = gpu.unnaf_locate(arc[which].d_naf, patterns, strands, first, count, out=buf)
    assert total == len(want) and view.numel() == 24 * total and not bool(buf[24 * total:].any())
    with pytest.raises(capi.NafGpuError) as e:
        gpu.unnaf_locate(arc[which].d_naf, patterns, strands, first, count, out=buf[:24 * (len(want) - 1)])
    assert e.value.code == E_CAP


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_contract(gpu, planned, oracle):
    from naf_amd import capi
    c, arc = planned["ambiguity"]
    A = arc["own"]
    N = A.h.n_sequences

    def fails(patterns, strands=3, first=0, count=None, words=()):
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_locate_count(A.d_naf, patterns, strands, first, count)
        assert e.value.code == E_ARG, e.value
        for w in words:
            assert w in e.value.msg, e.value.msg
        with pytest.raises(capi.NafGpuError) as e2:
            gpu.unnaf_locate(A.d_naf, patterns, strands, first, count)
        assert e2.value.code == E_ARG

    fails(["ACGT", "ACXT"], words=("pattern 1", "'X'"))
    fails(["AC-T"], words=("pattern 0", "'-'"))
    fails(["NGG", "GG", "A5"], words=("pattern 2", "'5'"))
    fails(["NGG", ""], words=("pattern 1",))
    fails(["A" * 33], words=("pattern 0", "33"))
    fails([], words=("patterns",))
    fails(["A"] * 17, words=("17",))
    fails(["A"], strands=0, words=("strand",))
    fails(["A"], strands=4, words=("strand",))
    fails(["A"], first=N + 1, words=("record",))
    fails(["A"], first=1, count=N, words=("records",))
    assert gpu.unnaf_locate_count(A.d_naf, ["A"], 3, N, 0)[0] == 0 and gpu.unnaf_locate_count(A.d_naf, ["A"], 3, N, None)[0] == 0
    assert gpu.unnaf_locate_count(A.d_naf, ["A"], 3, 1, 0)[0] == 0
    # protein and text archives are refused; an archive without records has no hits
    for name, word in (("protein_small", "protein"), ("text_small", "text")):
        d = gpu.to_device(golden_bytes("naf", name + ".naf"))
        with pytest.raises(capi.NafGpuError) as e:
            gpu.unnaf_locate_count(d, ["A"])
        assert e.value.code == E_ARG and word in e.value.msg
    empty = gpu.to_device(oracle.ennaf(b""))
    assert gpu.unnaf_locate_count(empty, ["A", "NGG"]) == (0, [[0, 0], [0, 0]])
    hits, total = gpu.unnaf_locate(empty, ["A"])
    assert total == 0 and len(hits) == 0


# ---- 7. composition with the selection path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planted_odd", "ambiguity", "rna", "fastq_reads"])
def test_every_hit_selects_bases_that_match_its_pattern(gpu, planned, name):
    from naf_amd import capi
    c, arc = planned[name]
    A = arc["own"]
    rng = np.random.default_rng(7800 + SEED)
    for patterns, strands, first, count in c.queries[:3]:
        hits, total = gpu.unnaf_locate(A.d_naf, patterns, 3, first, count)
        assert total == len(A.want(patterns, 3, first, count)) and total > 0
        pick = hits if total <= 3000 else hits[np.sort(rng.choice(total, 3000, replace=False))]
        segs = capi.hits_to_segments(pick, patterns)
        text = gpu.unnaf_select(A.d_naf, segs, SEQ, use_mask=False).cpu().numpy().tobytes().decode("latin1")
        at = 0
        for h, (r, b, e, rv) in zip(pick, segs):
            p = LP.canon(patterns[int(h["pattern"])])
            got = text[at:at + len(p)].upper().replace("U", "T")
            at += len(p)
            assert re.fullmatch("".join(LP.CLASS[ch] for ch in p), got), (r, b, e, rv, p, got)
        assert at == len(text)
        # with flanks clamped to the record the hit sits inside what is selected
        lens, _ = gpu.unnaf_record_table(A.d_naf, out_type=SEQUENCES)
        wide = capi.hits_to_segments(pick[:50], patterns, flank=7, lengths=lens)
        assert all(0 <= b < e <= lens[r] for r, b, e, _ in wide)
        assert len(gpu.unnaf_select(A.d_naf, wide, SEQ, use_mask=False)) == sum(e - b for _, b, e, _ in wide)


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------------
def unnaf_cli(args, naf, env=None):
    return subprocess.run([os.path.join(BIN, "unnaf"), *args, "-c"], input=naf, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                          env=dict(os.environ, **(env or {})))


def bed(A, ids, patterns, strands, first=0, count=None):
    return "".join("%s\t%d\t%d\t%s\t0\t%s\n" % (ids[r], b, b + len(patterns[p]), patterns[p], "-" if s else "+")
                   for r, b, p, s in A.want(patterns, strands, first, count)).encode("latin1")


def test_cli_locate_writes_bed(gpu, oracle, planned, tmp_path):
    c, arc = planned["ambiguity"]
    A = arc["own"]
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    assert len(ids) == A.h.n_sequences
    pats = ["RY", "nGg", "BDHV"]
    p = unnaf_cli(["--locate", pats[0], "--locate", pats[1], "--locate", pats[2]], A.naf)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == bed(A, ids, pats, 3)
    assert p.stdout.count(b"\n") > 10 and b"\tnGg\t0\t-\n" in p.stdout
    for flag, mask in (("+", 1), ("-", 2), ("both", 3)):
        p = unnaf_cli(["--locate", "RY", "--strand", flag], A.naf)
        assert p.returncode == 0 and p.stdout == bed(A, ids, ["RY"], mask)
    p = unnaf_cli(["--locate", "N", "--records", "2-3", "--strand", "+"], A.naf)
    assert p.returncode == 0 and p.stdout == bed(A, ids, ["N"], 1, 1, 2)
    p = unnaf_cli(["--locate", "N", "--region", ids[1]], A.naf)
    assert p.returncode == 0 and p.stdout == bed(A, ids, ["N"], 3, 1, 1)
    # a FASTQ archive, to a file, in pieces
    c, arc = planned["fastq_reads"]
    A = arc["oracle"]
    ids = oracle.zstd_decompress(A.h.frame(A.naf, 0)).decode("latin1").split("\0")[:-1]
    patterns, strands, first, count = c.queries[0]
    f, out = tmp_path / "reads.naf", tmp_path / "hits.bed"
    f.write_bytes(A.naf)
    p = subprocess.run([os.path.join(BIN, "unnaf"), *sum((["--locate", x] for x in patterns), []), "-o", str(out), str(f)],
                       env=dict(os.environ, NAF_GPU_LOCATE_PIECE="20001"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout == b"" and out.read_bytes() == bed(A, ids, patterns, 3)
    # what cannot be: nothing on stdout, exit 1
    A = planned["ambiguity"][1]["own"]
    for args in (["--locate", "N", "--region", "nosuch"], ["--locate", "N", "--records", "1-99"], ["--locate", "N", "--fasta"],
                 ["--locate", "N", "--region", "r1:1-5"], ["--locate", "N", "--rc-region", "r1"], ["--locate", "N", "--records", "1", "--revcomp"],
                 ["--locate", "N", "--records", "1", "--records", "2"], ["--locate", "NX"]):
        p = unnaf_cli(args, A.naf)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"unnaf error: "), args
    p = unnaf_cli(["--locate", "A"], golden_bytes("naf", "protein_small.naf"))
    assert p.returncode == 1 and p.stdout == b"" and b"protein" in p.stderr
