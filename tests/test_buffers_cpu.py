"""The fence of tests/fenced.py can see: numpy stand-ins of a correct call and of the ways a kernel goes wrong around its buffers,
on a CPU arena.  Every planted fault must be reported with the view it belongs to and its distance."""
import numpy as np
import pytest

import fenced
from fenced import Arena, FenceError, PHASES


def np_of(view):
    return view.numpy()                                   # shares the arena's memory


def whole(arena):
    return arena.buf.numpy()


def start_of(arena, view):
    return fenced.address(view) - fenced.address(arena.buf)


DATA = bytes(range(1, 200)) * 3                           # 597 bytes, no multiple of anything


def copy_honest(arena, src, dst):
    np_of(dst)[:] = np_of(src)


def copy_one_behind(arena, src, dst):
    copy_honest(arena, src, dst)
    whole(arena)[start_of(arena, dst) + dst.numel()] ^= 0xFF


def copy_one_in_front(arena, src, dst):
    copy_honest(arena, src, dst)
    whole(arena)[start_of(arena, dst) - 1] ^= 0xFF


def copy_wide_tail(arena, src, dst):
    """The last store is 16 bytes wide and starts at n - 3."""
    copy_honest(arena, src, dst)
    a = start_of(arena, dst) + dst.numel() - 3
    whole(arena)[a + 3:a + 16] ^= 0xFF


@pytest.mark.parametrize("phase", PHASES)
def test_honest_copy_passes_at_every_phase(phase):
    A = Arena("cpu", salt=0x5A)
    src = A.put(DATA, phase, b"front", b"behind")
    dst = A.out(len(DATA), (7 * phase + 3) % 128)
    copy_honest(A, src, dst)
    A.check()
    assert bytes(np_of(dst)) == DATA


@pytest.mark.parametrize("phase", (0, 5, 16, 127))
@pytest.mark.parametrize("fault, distance, span, count", [(copy_one_behind, 1, 1, 1), (copy_one_in_front, -1, -1, 1), (copy_wide_tail, 1, 13, 13)])
def test_planted_stores_are_reported_with_view_and_distance(phase, fault, distance, span, count):
    A = Arena("cpu", salt=3)
    first = A.out(40, 9)                                  # a neighbour, so that the damage has to be given to the right view
    src = A.put(DATA, 0)
    dst = A.out(len(DATA), phase)
    np_of(first)[:] = 7
    fault(A, src, dst)
    with pytest.raises(FenceError) as ei:
        A.check()
    e = ei.value
    assert (e.view, e.distance, e.span, e.count) == ("out#2", distance, span, count)
    word = "1 byte behind out#2" if distance > 0 else "1 byte in front of out#2"
    assert word in str(e) and ("13 bytes away" in str(e)) == (span == 13)


def test_three_bytes_behind_and_a_written_input_are_named():
    A = Arena("cpu")
    src = A.put(DATA, 1)
    dst = A.out(16, 2)
    whole(A)[start_of(A, dst) + 16 + 2] ^= 1
    with pytest.raises(FenceError, match="3 bytes behind out#1"):
        A.check()
    A.reset()
    src = A.put(DATA, 1)
    np_of(src)[10] ^= 1
    with pytest.raises(FenceError) as ei:
        A.check()
    assert ei.value.view == "in#1" and ei.value.distance == 0
    A.reset()
    A.check()


def test_a_store_of_the_pattern_s_own_kind_is_seen():
    """Zeros and 0xA5 everywhere behind the output: the pattern is no constant, so at most 1 byte in 256 of such a store hides."""
    for value in (0x00, 0xA5):
        A = Arena("cpu", salt=value)
        dst = A.out(100, 3)
        s = start_of(A, dst)
        whole(A)[s + 100:s + 100 + 512] = value
        with pytest.raises(FenceError) as ei:
            A.check()
        assert ei.value.view == "out#1" and 1 <= ei.value.distance <= 2 and ei.value.count >= 500


# ---- results that depend on bytes outside the input ------------------------------------------------------------------------------
def sum_honest(src, n):
    return int(src[:n].sum())


def outside(d_in, offset):
    """The byte at d_in[offset] for an offset outside the view (what a kernel reaches through the pointer it was given)."""
    import torch
    return int(torch.as_strided(d_in, (1,), (1,), d_in.storage_offset() + offset)[0])


def folds_the_byte_behind(d_in):
    return int(np_of(d_in).sum()) + outside(d_in, d_in.numel())       # src[len] counts


def folds_the_byte_in_front(d_in):
    prev_is_eol = outside(d_in, -1) == 10                 # text[-1] decides "the text starts a line"
    return int(np_of(d_in).sum()) + (0 if prev_is_eol else 1)


@pytest.mark.parametrize("phase", fenced.BAIT_PHASES)
def test_two_fills_catch_a_result_that_reads_outside_its_input(phase):
    arenas = [Arena("cpu", salt=0x11), Arena("cpu", salt=0xC3)]
    want = sum(DATA)
    for bait in (fenced.text_bait, lambda run: fenced.stream_bait(DATA, run)):
        honest = fenced.fenced_runs(arenas, DATA, None, phase, 0, bait, lambda d_in, d_out: sum_honest(np_of(d_in), len(DATA)))
        assert honest == [want, want]
        # (a parser that asks "is the byte in front a line end" tells the two fills of a text's bait apart: it is one in the first only)
        for k, stand_in in enumerate((folds_the_byte_behind, folds_the_byte_in_front) if bait is fenced.text_bait else (folds_the_byte_behind,)):
            got = fenced.fenced_runs(arenas, DATA, None, phase, 0, bait, lambda d_in, d_out: stand_in(d_in))
            assert len(got) == 2 and got[0] != got[1], (k, got)             # the two fills disagree ...
            assert got != [want, want]                                       # ... and at least one is not the reference's
    assert len(fenced.fenced_runs(arenas, DATA, None, 5, 0, fenced.text_bait, lambda d_in, d_out: 0)) == 1      # other phases: one run


def test_bait_lies_directly_around_the_data():
    A = Arena("cpu", salt=1)
    before, after = fenced.text_bait(0)
    v = A.put(DATA, 65, before, after)
    s = start_of(A, v)
    assert bytes(whole(A)[s - len(before):s]) == before and before.endswith(b"ACGT\n") and b"ACGT>bait" in before
    assert bytes(whole(A)[s + len(DATA):s + len(DATA) + len(after)]) == after
    b1, a1 = fenced.text_bait(1)
    assert b1 == fenced.complement(before) and a1 == fenced.complement(after) and b1[-1] not in b"\n\r"
    fb, fa = fenced.stream_bait(DATA, 0)
    assert fb == DATA[-64:] and fa == DATA[:64] and fenced.stream_bait(DATA, 1) == (fenced.complement(fb), fenced.complement(fa))
    A.check()                                             # bait is part of what was put there
    whole(A)[s - 1] ^= 0xFF                               # and stays guarded
    with pytest.raises(FenceError, match="1 byte in front of in#1"):
        A.check()


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def test_put_and_out_deliver_every_phase_and_nothing_overlaps():
    A = Arena("cpu", salt=9, size=1 << 20)
    spans = []
    for k, phase in enumerate(PHASES):
        n = (0, 1, 15, 16, 17, 130, 4095)[k % 7]
        vi = A.put(bytes(n), phase, b"xy", b"z")
        vo = A.out(n, phase)
        for v in (vi, vo):
            assert v.numel() == n and v.dtype.itemsize == 1
            assert fenced.address(v) % 128 == phase
            s = start_of(A, v)
            assert s >= fenced.FENCE and s + n + fenced.FENCE <= A.size
            spans.append((s - fenced.FENCE, s, s + n, s + n + fenced.FENCE))
    spans.sort()
    for a, b in zip(spans, spans[1:]):
        assert a[3] <= b[0]                               # view and both fences of one end before the next one's front fence starts
    assert [v.name for v in A.views[:4]] == ["in#1", "out#1", "in#2", "out#2"]
    A.check()
    pattern = ((np.arange(A.size) * 131 + 89) ^ 9) & 0xFF
    o = A.views[1]
    assert (whole(A)[o.start:o.end] == pattern[o.start:o.end]).all()          # an output region carries the pattern
    assert (whole(A)[:fenced.FENCE - 2] == pattern[:fenced.FENCE - 2]).all()  # (the two bytes of `before` lie nearest the first view)
    with pytest.raises(MemoryError):
        Arena("cpu", size=3 * fenced.FENCE).put(bytes(fenced.FENCE * 2), 0)


def test_sweep_of_phases():
    assert set(p % 16 for p in PHASES) == set(range(16)) and {63, 65, 127, 0, 1} <= set(PHASES)
    c = fenced.combos()
    assert len(c) == len(set(c)) == 3 * len(PHASES) - 2           # (0, 0) and (0, 3) come twice
    assert all((0, p) in c and (p, 0) in c and (p, (7 * p + 3) % 128) in c for p in PHASES)
