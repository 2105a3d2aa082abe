"""The cut planner of the byte-range sweeps (tests/range_plan.py), without a GPU: its base-index -> text-offset arithmetic against a
plain walk of the text, and -- for every archive and view tests/test_gpu_ranges.py cuts, built from seed 0 -- at least one position of
every class the archive can have and the sweeps' floors per class: the guard against a sweep that silently covers nothing."""
import numpy as np
import pytest

import range_plan as RP
from conftest import golden_bytes, naf_cases

MODE_OF = {"fasta": (RP.FASTA, True, -1), "fasta_nomask": (RP.FASTA, False, -1), "fasta_ll13": (RP.FASTA, True, 13), "fasta_ll0": (RP.FASTA, True, 0),
           "seq": (RP.SEQ, True, -1), "sequences": (RP.SEQUENCES, True, -1), "fastq": (RP.FASTQ, True, -1), "4bit": (RP.FOURBIT, True, -1)}


@pytest.mark.parametrize("name", ["mixed_60", "fastq_var", "mask_bounds", "tiny_many", "ll_override"])
def test_base_map_against_a_walk_of_the_text(oracle, name):
    naf = golden_bytes("naf", name + ".naf")
    case = [c for c in naf_cases() if c["name"] == name][0]
    bases = oracle.unnaf(naf, RP.SEQ)
    for m, (mode, um, ll) in MODE_OF.items():
        if m not in case["outputs"] or mode == RP.FOURBIT:
            continue
        want = oracle.unnaf(naf, mode, um, ll)
        plan = RP.Plan(naf, want, mode, um, ll)
        walk, end = RP.brute_base_map(want, bases, plan.lens, mode)
        assert end == plan.main_total == len(want), m
        assert plan.base_pos(np.arange(plan.T)).tolist() == walk, m
        # every listed position lies where its class says
        w = np.frombuffer(want, dtype=np.uint8)
        if mode in (RP.FASTA, RP.FASTQ):
            assert (w[plan.hdr] == (62 if mode == RP.FASTA else 64)).all() and (w[plan.body - 1] == 10).all(), m
        line = plan.positions("line", None, None)
        assert (w[line] == 10).all(), m
        if mode == RP.FASTA:
            hdr_nl = set((plan.body - 1).tolist())
            assert sorted(set(np.flatnonzero(w == 10).tolist()) - hdr_nl) == line.tolist(), m      # every line end of the bodies, nothing else
        tog = plan.positions("mask", None, None)
        low = (w >= 97) & (w <= 122)
        seq_low = low[np.asarray(walk, dtype=np.int64)]
        assert tog.tolist() == [walk[i] for i in (np.flatnonzero(seq_low[1:] != seq_low[:-1]) + 1)], m
        odd = plan.positions("pair", None, None)
        assert odd.tolist() == walk[1::2], m


def test_bases_behind_the_last_record_are_the_tail(oracle):
    name, text, st = [t for t in RP.planned_texts(0) if t[0] == "surplus"][0]
    naf = oracle.ennaf(text, st)
    for mode, um, ll in RP.views_of(text, st, 10):
        want = oracle.unnaf(naf, mode, um, ll)
        plan = RP.Plan(naf, want, mode, um, ll, own=True)
        assert plan.surplus == 133
        if mode != RP.FOURBIT:
            assert plan.main_total < plan.n and plan.positions("tail", None, None).tolist() == [plan.main_total, plan.n]
            walk, end = RP.brute_base_map(want, oracle.unnaf(naf, RP.SEQ), plan.lens, mode)
            assert end == plan.main_total


HAVE_LOWER_CASE = ("mixed_long", "mixed_short", "short_runs", "surplus", "protein", "text")      # by construction


def _floors(plan, classes, label):
    rng = np.random.default_rng(0)
    for cls in classes:
        pos = plan.positions(cls, RP.K_MAIN, rng)
        assert len(pos) >= 1, (label, cls)
        assert len(pos) >= RP.K_MAIN or len(pos) == plan.count(cls), (label, cls, len(pos))
        assert ((pos >= 0) & (pos <= plan.n)).all()


def test_every_small_archive_has_every_class_it_can_have(oracle):
    seen = set()
    for case in naf_cases():
        naf = golden_bytes("naf", case["name"] + ".naf")
        for m, (mode, um, ll) in MODE_OF.items():
            if m in case["outputs"]:
                plan = RP.Plan(naf, oracle.unnaf(naf, mode, um, ll), mode, um, ll)
                _floors(plan, plan.possible(), (case["name"], m))
                seen |= plan.possible()
    assert seen == set(RP.CLASSES) - {"stream"}                     # (the seams of four streams are this build's frames' alone)


def test_planned_texts_meet_the_floors(oracle):
    """Sweep (b): every text, every view; the first view must hold K_MAIN positions of a class where the text has them."""
    seen, pairings = {}, set()
    assert tuple(t[0] for t in RP.planned_texts(0)) == RP.PLANNED_NAMES          # (the GPU module is parametrised by these names)
    for k, (name, text, st) in enumerate(RP.planned_texts(0)):
        assert 1_000_000 <= len(text) <= 3_000_000, (name, len(text))
        naf = oracle.ennaf(text, st)
        for v, (mode, um, ll) in enumerate(RP.views_of(text, st, k)):
            pairings.add((mode, um, ll))
            plan = RP.Plan(naf, oracle.unnaf(naf, mode, um, ll), mode, um, ll, own=True)
            if um and mode != RP.FOURBIT and mode != RP.FASTQ and name in HAVE_LOWER_CASE:
                assert "mask" in plan.possible(), (name, mode, um, ll)
            _floors(plan, plan.possible(), (name, mode, um, ll))
            if v == 0:
                seen[name] = plan.possible()
                jobs, _ = RP.planned_jobs(plan, sorted(plan.possible()), RP.K_MAIN, np.random.default_rng(0))
                per = {c: len({j[1] for j in jobs if j[0] == c}) for c in plan.possible()}
                assert all(per[c] >= min(RP.K_MAIN, plan.count(c)) for c in per), (name, per)
                for cls in ("record", "line"):
                    if cls in per:
                        anch = plan.anchors(cls, plan.positions(cls, None, None) if cls == "record" else [j[1] for j in jobs if j[0] == cls])
                        assert len(anch) >= (6 if cls == "record" and plan.N > 1 and plan.mode != RP.SEQUENCES else 2) and set(anch.tolist()) <= {j[1] for j in jobs if j[0] == cls}, (name, cls)
                assert {j[4] for j in jobs} == set(RP.PATHS) and {j[3] - j[2] for j in jobs} >= set(RP.LENGTHS), name
    assert all("mask" in seen[n] for n in HAVE_LOWER_CASE) and "fastq" in seen["fastq_var"] and "fastq" in seen["fastq_fixed"]
    assert {(RP.FASTA, um, ll) for um in (True, False) for ll in (-1, 0, 1, 15, 16, 17, 33)} <= pairings      # every line length with the mask on and off
    assert all({"record", "tail", "block"} <= s for s in seen.values()), seen
    assert all({"pair", "group", "stream", "line"} <= seen[n] for n in seen if n.startswith(("acgt", "mixed", "short", "surplus"))), seen


def test_flat_and_match_texts_meet_the_floors(oracle):
    """Sweeps (c) and (d)."""
    for k in range(len(RP.FLAT_TEXTS)):
        text = RP.flat_text(k, 0)
        naf = oracle.ennaf(text)
        for mode, um, ll in RP.FLAT_VIEWS:
            want = text if (mode, ll) == (RP.FASTA, -1) else oracle.unnaf(naf, mode, um, ll)
            plan = RP.Plan(naf, want, mode, um, ll, own=True)
            assert plan.possible() >= set(RP.FLAT_CLASSES) - (set() if mode in (RP.FASTA, RP.SEQUENCES) else {"line"}), (k, mode)
            _floors(plan, [c for c in RP.FLAT_CLASSES if c in plan.possible()], ("flat", k, mode, um, ll))
        if k == 2:
            assert plan.T % plan.block_bases == 0                   # the count that ends on a block
    arcs = [(n, golden_bytes("naf", n + ".naf"), False) for n in RP.MATCH_GOLDEN] + [("own_sparse", oracle.ennaf(RP.sparse_text(0)), True)]
    for name, naf, own in arcs:
        for mode, um, ll in RP.match_views(name):
            plan = RP.Plan(naf, oracle.unnaf(naf, mode, um, ll), mode, um, ll, own=own)
            have = [c for c in RP.MATCH_CLASSES if c in plan.possible()]
            expect = {"record", "pair"} | ({"line"} if mode != RP.FASTQ else set()) | ({"block"} if name != "mixed_60" else set())   # (mixed_60: one block)
            assert set(have) == expect, (name, mode, have)
            _floors(plan, have, (name, mode))
