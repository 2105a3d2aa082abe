"""naf_gpu_unnaf_range at every phase of tile against record, line, nibble pair, group of 16, stream and block seam, mask toggle and
the bases behind the last record (run with -m gpu on an MI355X).

Every emit kernel anchors its 4096-byte tiles at the first byte of the range, so a whole-text decode runs each at one phase only.
Here the range begins and ends within two bytes of every kind of place where something changes (tests/range_plan.py lists them from
the oracle's text), and -- on small archives -- at every byte.  What a call must return is always a slice of the ORACLE's text of the
same archive, never of this library's.  Each sweep counts its calls per class and holds itself to a floor at its end.  Nothing here
reads the reference tree."""
import os
from collections import defaultdict
from functools import lru_cache

import numpy as np
import pytest

import range_plan as RP
from conftest import golden_bytes, naf_cases

SEED = int(os.environ.get("NAF_TEST_SEED", "0"))          # other texts of the same kinds: NAF_TEST_SEED=n python -m pytest ...

pytestmark = pytest.mark.gpu


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


def set_path(mp, path):
    """One emit path: "" the kernel the library picks, "fused" with NAF_GPU_FUSE=1 (whole texts only: a range must not care), "long" the
    tile-indexed kernel, "span" the older one, "short" the segment-composing one, "slow" per-byte emit."""
    mp.setenv("NAF_GPU_FORCE_SLOW", "1" if path == "slow" else "0")
    mp.setenv("NAF_GPU_EMIT", path if path in ("long", "span", "short") else "")
    mp.setenv("NAF_GPU_FUSE", "1" if path == "fused" else "0")


class Tally:
    """Range calls against slices of the oracle's text; mismatches are collected (class, position, cut, view, path, first differing
    offset -- not the bytes) and the sweep fails with the first twenty of them at its end."""

    def __init__(self, gpu):
        self.gpu, self.calls, self.where, self.bad = gpu, defaultdict(int), defaultdict(set), []

    def check(self, d, want, a, b, view, cls, p, path, label):
        mode, um, ll = view
        got = host(self.gpu.unnaf_range(d, a, b, mode, um, ll))
        exp = want[a:b] if a <= b else b""
        self.calls[cls] += 1
        self.where[cls].add(p)
        if got != exp and len(self.bad) < 20:
            self.bad.append("%s: class %s p %s range (%d, %d) mode %d mask %d ll %d path %r: %s" % (label, cls, p, a, b, mode, um, ll, path, RP.first_diff(got, exp)))
        return got == exp

    def run(self, mp, d, want, view, jobs, label, set_paths=True):
        by_path = defaultdict(list)
        for j in jobs:
            by_path[j[4]].append(j)
        for path in sorted(by_path):
            if set_paths:
                set_path(mp, path)
            for cls, p, a, b, _ in by_path[path]:
                self.check(d, want, a, b, view, cls, p, path, label)

    def done(self):
        assert not self.bad, "%d range calls, first mismatches:\n%s" % (sum(self.calls.values()), "\n".join(self.bad))


# ---- (a) every begin of the small archives -------------------------------------------------------------------------------------
A_LENGTHS = (1, 2, 15, 16, 17, 64, None)                   # None: to the end of the text
A_PATHS = ("fused", "long", "span", "short", "slow")       # the paths test_unnaf_matches_reference_outputs names
A_FULL, A_FULL_FIRST, A_EVERY_VIEW = 64, 600, 4096         # text sizes (FASTA): the whole product in every view / in the first view / every begin of every view
_F, _S, _Q = (RP.FASTA, True, -1), (RP.SEQUENCES, True, -1), (RP.FASTQ, True, -1)
# larger archives: (view, paths taken at every begin -- None: one, rotating) ..., then the window and the stride: every begin of the
# first and last `window` bytes and every stride-th between (None: every begin of the text)
A_LARGE = {"mask_bounds": ([(_F, None), ((RP.FASTA, False, 13), None), ((RP.SEQ, True, -1), None), (_S, None), ((RP.FOURBIT, True, -1), None)], None, 1),
           "acgt_10k": ([(_F, None)], None, 1),
           "acgt_ll1": ([(_F, None)], None, 1),                        # lines of one base
           "tiny_many": ([(_F, ("short", "long"))], 4096, 29),              # 3000 records of 18 bytes: every phase of header against tile
           "acgt_odd": ([(_F, None)], 8192, 7),
           "fastq_var": ([(_Q, None)], 2048, 211)}                      # (a range call of 4600 reads costs 3 ms)


def _small_cases():
    names = [c["name"] for c in naf_cases() if c["outputs"]["fasta"]["len"] <= A_EVERY_VIEW or c["name"] in A_LARGE]
    return names + ["fastq_small"]


def _views_of_case(outputs):
    v = []
    if "fastq" in outputs:
        v.append((RP.FASTQ, True, -1))
    v += [(RP.FASTA, um, ll) for um in (True, False) for ll in (-1, 0, 1, 13)]
    v += [(RP.SEQ, True, -1), (RP.SEQ, False, -1), (RP.SEQUENCES, True, -1), (RP.SEQUENCES, False, -1)]
    return v + ([(RP.FOURBIT, True, -1)] if "4bit" in outputs else [])


def _begins(n, window, stride):
    if window is None or n <= 2 * window:
        return list(range(n + 1))
    return list(range(window + 1)) + list(range(window + 1, n - window, stride)) + list(range(n - window, n + 1))


@pytest.mark.parametrize("name", _small_cases())
def test_every_begin_of_a_small_archive(gpu, oracle, name, monkeypatch):
    """Begins a of [0, n] with b - a in (1, 2, 15, 16, 17, 64, to the end) under the five emit paths, against the oracle's text.  The
    whole product (every begin x 7 lengths x 5 paths x 13 views) is 5.8 million calls for the archives of up to 4 KiB alone, so:
    texts of at most 64 bytes take it whole in every view (mode, mask on / off, line length -1, 0, 1, 13); texts of up to 600 bytes
    (title) whole in their first view; texts of up to 4 KiB every begin of every view, with all five paths at every begin of the first
    view and one length and one path per begin elsewhere, rotating with the begin (periods 7 and 5: every pair within 35 consecutive
    begins).  Larger archives (A_LARGE) take few views: mask_bounds, acgt_10k, acgt_ll1 at every begin; tiny_many (under the short
    and the long kernel), acgt_odd and fastq_var at every begin of their first and last 4, 8 and 2 KiB and a stride between.
    A FASTQ archive of 1 KiB the oracle makes here gets every view at every begin.  Then the calls that ask for nothing or for too
    much, as the code answers them today: a == b, a > b and a > n give an empty text, b > n is clamped to n."""
    if name == "fastq_small":
        from naf_amd import synth
        naf, outputs = oracle.ennaf(synth.fastq_reads(14, 60, seed=140 + SEED, var_len=True)), {"fastq": 1, "4bit": 1}
    else:
        naf, outputs = golden_bytes("naf", name + ".naf"), [c for c in naf_cases() if c["name"] == name][0]["outputs"]
    views, window, stride = A_LARGE.get(name) or ([(v, None) for v in _views_of_case(outputs)], None, 1)
    d = gpu.to_device(naf)
    tally = Tally(gpu)
    for v, (view, fixed_paths) in enumerate(views):
        want = oracle.unnaf(naf, *view)
        n = len(want)
        begins = _begins(n, window, stride)
        jobs = []
        for a in begins:
            if n <= A_FULL or (v == 0 and n <= A_FULL_FIRST):
                combos = [(ln, path) for ln in A_LENGTHS for path in A_PATHS]
            elif fixed_paths or (v == 0 and name not in A_LARGE):
                combos = [(A_LENGTHS[(a + k) % 7], path) for k, path in enumerate(fixed_paths or A_PATHS)]
            else:
                combos = [(A_LENGTHS[(a + v) % 7], A_PATHS[(a + v) % 5])]
            for ln, path in combos:
                jobs.append(("begin", (v, a), a, n if ln is None else min(n, a + ln), path))
        tally.run(monkeypatch, d, want, view, jobs, name)
        assert {p[1] for p in tally.where["begin"] if p[0] == v} == set(begins) and (window is not None or len(begins) == n + 1)   # the floor
        set_path(monkeypatch, "")
        for a, b in ((0, 0), (n // 2, n // 2), (n, n), (max(n - 5, 0), n + 100), (0, n + 1), (n + 1, n + 9), (n + 1, n + 1), (min(5, n), min(3, n)), (n, 0)):
            want_ab = b"" if a > b else want[a:b]
            got = host(gpu.unnaf_range(d, a, b, *view))
            assert got == want_ab, (name, view, a, b, len(got))
    print("\n[ranges a] %s: %d calls" % (name, sum(tally.calls.values())))
    tally.done()


def test_four_bit_mode_of_an_archive_without_packed_bases_is_refused(gpu, oracle):
    """--4bit of a protein archive: the oracle refuses (unnaf.c), and so does a range call."""
    from naf_amd.capi import NafGpuError
    naf = golden_bytes("naf", "protein_small.naf")
    with pytest.raises(ValueError):
        oracle.unnaf(naf, RP.FOURBIT)
    with pytest.raises(NafGpuError):
        gpu.unnaf_range(gpu.to_device(naf), 0, 8, RP.FOURBIT)


# ---- (b) planned cuts of texts of 1 .. 3 MB ---------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _planned_texts():
    return RP.planned_texts(SEED)


def _floor(tally, plan, classes, label):
    """At least K_MAIN positions of every class the text can have, all of them where it has fewer."""
    for cls in classes:
        have = len(tally.where[cls])
        assert have >= RP.K_MAIN or have >= plan.count(cls), (label, cls, have)
        assert tally.calls[cls] >= have


@pytest.mark.parametrize("k", range(len(RP.PLANNED_NAMES)), ids=lambda k: RP.PLANNED_NAMES[k])
def test_planned_cuts_of_own_archives(gpu, oracle, k, monkeypatch):
    """An archive this build makes of: mixed long records (soft-masked runs, N runs, IUPAC, empty records) / mixed short ones / A C G T
    wrapped at 60, 61, 80, 4095, 4096, 4097 and not at all / case changes every 1..40 bases with runs of 254, 255, 256 and 70 000 /
    bases behind the last record / proteins / --text / reads of fixed and of variable length.  Views: FASTA (FASTQ) with line lengths
    -1, 0, 1, 15, 16, 17, 33 and the mask on / off, --seq, --sequences, --4bit.  For every class of place the planner finds, K_MAIN
    positions in the first view and K_OTHER in each other; around each, a begin and an end at p-2 .. p+2, the length (1, 16, 4095,
    4096, 4097, 3 * 4096 + 5) and the emit path ("", long, span, short, NAF_GPU_FORCE_SLOW=1) rotating from cut to cut."""
    from naf_amd import capi
    name, text, st = _planned_texts()[k]
    d_naf, _ = gpu.ennaf(gpu.to_device(text), seq_type={RP.O.DNA: capi.SEQ_DNA, RP.O.PROTEIN: capi.SEQ_PROTEIN, RP.O.TEXT: capi.SEQ_TEXT}[st])
    naf = host(d_naf)
    rng = np.random.default_rng(50 + k + 1000 * SEED)
    tally, c = Tally(gpu), 0
    for v, view in enumerate(RP.views_of(text, st, k)):
        want = oracle.unnaf(naf, *view)
        plan = RP.Plan(naf, want, *view, own=True)
        if v == 0:
            plan0, classes0 = plan, sorted(plan.possible())
            if name != "surplus" and text[:1] == b">":
                assert want == text                                            # (the archive holds the text it was made of; FASTQ output drops the case)
        jobs, c = RP.planned_jobs(plan, sorted(plan.possible()), RP.K_MAIN if v == 0 else RP.K_OTHER, rng, counter=c)
        tally.run(monkeypatch, d_naf, want, view, jobs, name)
        if v == 0:
            _floor(tally, plan0, classes0, name)
    print("\n[ranges b] %s: %d calls, per class %s" % (name, sum(tally.calls.values()), dict(tally.calls)))
    tally.done()


# ---- (c) the frame read in place -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(RP.FLAT_TEXTS)), ids=lambda k: "flat%d" % k)
def test_planned_cuts_of_a_frame_read_in_place(gpu, oracle, k, monkeypatch):
    """30 M bases of uniform A C G T (an odd count, an even one, one that ends on a block): with NAF_GPU_SPEC_MIN=8 the frame of the
    sequence stream is not decoded, k_emit_tile_flat* read its four streams per block in place.  Cuts around nibble pairs, groups of
    16, stream seams (16 384 bases), block seams (65 536), line ends, record headers and the end of the text, lengths as above and one
    of a block and a half; FASTA with the archive's width, 50 and none, mask on / off, --seq, --sequences.  Every call must have run
    unnaf_emit_flat; then the same cuts with NAF_GPU_UNIFORM=0 (the general front) and NAF_GPU_FLAT=0 (the frame decoded).  The fourth
    text's odd base shares the last block with others: that block has a tree of its own, the whole-text call reads the frame mostly
    in place, and a range call does so only where the blocks under the range are all of the first tree (the cuts at the text's
    first pairs are: at least one call must run the in-place kernel); the others decode the blocks they need.  Its bytes are held to
    the oracle's like the others'."""
    monkeypatch.setenv("NAF_GPU_SPEC_MIN", "8")
    text = RP.flat_text(k, SEED)
    d_naf, _ = gpu.ennaf(gpu.to_device(text))
    naf = host(d_naf)
    assert oracle.unnaf(naf, RP.FASTA) == text
    rng = np.random.default_rng(70 + k + 1000 * SEED)
    tally, c, plans = Tally(gpu), 0, []
    for v, view in enumerate(RP.FLAT_VIEWS):
        want = text if view == RP.FLAT_VIEWS[0] else oracle.unnaf(naf, *view)
        plan = RP.Plan(naf, want, *view, own=True)
        classes = [x for x in RP.FLAT_CLASSES if x in plan.possible()]
        jobs, c = RP.planned_jobs(plan, classes, RP.K_MAIN if v == 0 else RP.K_OTHER, rng, lengths=RP.FLAT_LENGTHS, paths=("",), counter=c)
        plans.append((view, want, plan, classes, jobs))
    not_flat, n_flat = [], 0
    for setting in ("", "UNIFORM", "FLAT"):
        if setting:
            monkeypatch.setenv("NAF_GPU_" + setting, "0")
        for v, (view, want, plan, classes, jobs) in enumerate(plans):
            for cls, p, a, b, _ in jobs:
                if not setting:
                    gpu.set_timing(True)
                tally.check(d_naf, want, a, b, view, cls, p, setting and setting + "=0", "flat%d" % k)
                if not setting:
                    ran = {nm for nm, ms, cnt in gpu.get_timing()}
                    gpu.set_timing(False)
                    n_flat += "unnaf_emit_flat" in ran
                    if RP.FLAT_TEXTS[k][3] and "unnaf_emit_flat" not in ran:
                        not_flat.append((view, cls, a, b, sorted(ran)))
            if v == 0 and not setting:
                _floor(tally, plan, classes, "flat%d" % k)
        if setting:
            monkeypatch.delenv("NAF_GPU_" + setting)
    print("\n[ranges c] flat%d: %d calls, per class %s" % (k, sum(tally.calls.values()), dict(tally.calls)))
    assert not not_flat, "%d calls did not run unnaf_emit_flat, the first: %s" % (len(not_flat), not_flat[:3])
    assert n_flat >= 1                                                # (the fourth text: the ranges over its first blocks are read in place)
    tally.done()


# ---- (d) frames with matches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RP.MATCH_GOLDEN + ("own_sparse",))
def test_planned_cuts_of_frames_with_matches(gpu, oracle, name, monkeypatch):
    """Reference-made archives whose sequence frames hold matches (levels 1 and 19, --long 27, reads, mixed records) and an archive of
    this build at level 5: a range decodes the blocks under it and what their matches reach (k_range_closure), or -- with
    NAF_GPU_RANGE_CLOSURE=0 -- the whole stream.  Cuts around block seams, records, line ends and nibble pairs, both ways."""
    if name == "own_sparse":
        naf = host(gpu.ennaf(gpu.to_device(RP.sparse_text(SEED)), level=5)[0])
        assert oracle.zstd_frame_info(oracle.parse_naf(naf).frame(naf, RP.O.SEQ)).n_sequences > 0          # (it does hold matches)
    else:
        naf = golden_bytes("naf", name + ".naf")
    d = gpu.to_device(naf)
    rng = np.random.default_rng(90 + 1000 * SEED)
    tally, c = Tally(gpu), 0
    for v, view in enumerate(RP.match_views(name)):
        want = oracle.unnaf(naf, *view)
        plan = RP.Plan(naf, want, *view, own=name == "own_sparse")
        classes = [x for x in RP.MATCH_CLASSES if x in plan.possible()]
        jobs, c = RP.planned_jobs(plan, classes, RP.K_MAIN if v == 0 else RP.K_OTHER, rng, paths=("",), counter=c)
        for closure in ("1", "0"):
            monkeypatch.setenv("NAF_GPU_RANGE_CLOSURE", closure)
            tally.run(monkeypatch, d, want, view, [j[:4] + ("closure=" + closure,) for j in jobs], name, set_paths=False)
        if v == 0:
            _floor(tally, plan, classes, name)
    print("\n[ranges d] %s: %d calls, per class %s" % (name, sum(tally.calls.values()), dict(tally.calls)))
    tally.done()


# ---- (e) partitions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["planned", "flat", "matches"])
def test_partitions_concatenate_to_the_text(gpu, oracle, which, monkeypatch):
    """The ranges naf_amd.shard.byte_range deals to 2, 3, 7, 8 and 64 ranks, on 4096-byte boundaries and on none (align=1), laid end
    to end are the oracle's text: on an archive of each of the sweeps above."""
    from naf_amd.shard import byte_range
    if which == "planned":
        name, text, st = _planned_texts()[0]
        naf = host(gpu.ennaf(gpu.to_device(text))[0])
        views = [(RP.FASTA, True, -1), (RP.FASTA, False, 17), (RP.SEQUENCES, True, -1)]
    elif which == "flat":
        monkeypatch.setenv("NAF_GPU_SPEC_MIN", "8")
        naf = host(gpu.ennaf(gpu.to_device(RP.flat_text(0, SEED)))[0])
        views = [(RP.FASTA, True, -1), (RP.SEQ, True, -1)]
    else:
        naf = golden_bytes("naf", "repeat_l19.naf")
        views = [(RP.FASTA, True, -1), (RP.FOURBIT, True, -1)]
    d = gpu.to_device(naf)
    calls = 0
    for view in views:
        want = oracle.unnaf(naf, *view)
        n = len(want)
        for K in (2, 3, 7, 8, 64):
            for align in (4096, 1):
                parts = [byte_range(n, r, K, align) for r in range(K)]
                assert parts[0][0] == 0 and parts[-1][1] == n and all(x[1] == y[0] for x, y in zip(parts, parts[1:]))
                off = 0
                for r, (a, b) in enumerate(parts):
                    got = host(gpu.unnaf_range(d, a, b, *view)) if b > a else b""
                    calls += b > a
                    assert got == want[a:b], "%s: class partition K %d align %d rank %d range (%d, %d) mode %d mask %d ll %d: %s" % (
                        (which, K, align, r, a, b) + view + (RP.first_diff(got, want[a:b]),))
                    off += len(got)
                assert off == n
    assert calls >= len(views) * 2 * (2 + 3 + 7 + 8)
