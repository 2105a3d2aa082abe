"""Fenced buffers for the tests of the C-ABI (test_buffers_cpu.py proves the fence can see, test_gpu_buffers.py uses it).

An Arena is ONE uint8 tensor filled with a pattern that depends on the position, so a store of zeros, of 0xA5 or of a copy of the
data is seen wherever it lands.  put() and out() hand out views of it at a chosen address phase (address mod 128) with at least FENCE
untouched bytes on either side; check() compares everything that was not handed out as an output with what was put there and names
the nearest view and the distance of the damage.  Every view and every fence lies inside the one live allocation: the worst a wrong
kernel can do to such a buffer is write a wrong byte.  Plain helpers, no fixtures."""
import numpy as np
import torch

PHASES = tuple(range(17)) + (31, 33, 63, 65, 127)      # every residue mod 16, the 64- and 128-byte line edges from both sides
BIG_PHASES = (0, 1, 15, 16, 63, 65)                    # for inputs of hundreds of KB
BAIT_PHASES = (0, 1, 16, 65)                           # input phases at which a call is repeated in a second arena
FENCE = 4096
LINE = 128

TEXT_BEHIND = b"ACGTNacgtn\n>bait record\nACGT\n@bait\nAC\n+\nII\n"
TEXT_FRONT = b">bait\nACGT" + b">bait\nACGT\n"         # a record without a line end, then the same with one: the text starts a line


def complement(b):
    return bytes(x ^ 0xFF for x in b)


def text_bait(run):
    """(before, after) around a text: run 0 the bait, run 1 its complement -- the byte in front is an EOL once and none once."""
    return (TEXT_FRONT, TEXT_BEHIND) if run == 0 else (complement(TEXT_FRONT), complement(TEXT_BEHIND))


def stream_bait(data, run):
    """(before, after) around an archive, a frame or plain bytes: its own last and first 64 bytes, a plausible continuation of a bit
    stream, a tree description or a block header; run 1 the complement."""
    before, after = bytes(data[-64:]), bytes(data[:64])
    if not data:
        before = after = b"\x28\xb5\x2f\xfd\x20\x00\x01\x00\x00"
    return (before, after) if run == 0 else (complement(before), complement(after))


def combos(phases=PHASES):
    """(input phase, output phase) of a destination sweep: every output phase with the input at 0, every input phase with the output
    at 0, and the pairs (p, (7 p + 3) mod 128)."""
    c = [(0, p) for p in phases] + [(p, 0) for p in phases] + [(p, (7 * p + 3) % LINE) for p in phases]
    return sorted(set(c), key=c.index)


def address(view):
    """The address of a view's first byte; also for a view of no bytes, whose data_ptr() torch gives as 0."""
    return view.untyped_storage().data_ptr() + view.storage_offset()


def fenced_runs(arenas, data, cap, in_phase, out_phase, bait, call):
    """One call with its buffers in arenas[0] and, when the input phase is one of BAIT_PHASES, the same call in arenas[1] (another
    salt, bait(1) around the input): call(d_in, d_out) -> what the call gave, as something that compares (d_out is None when cap
    is).  The fences are checked after each; the caller holds every result to its reference and, being equal to one reference, the
    two runs are equal to each other -- a result that depends on a byte outside the input cannot be both."""
    res = []
    for run, A in enumerate(arenas[:2 if in_phase in BAIT_PHASES else 1]):
        A.reset()
        before, after = bait(run)
        d_in = A.put(data, in_phase, before, after)
        d_out = None if cap is None else A.out(cap, out_phase)
        res.append(call(d_in, d_out))
        if A.device.type == "cuda":
            torch.cuda.synchronize()
        A.check()
    return res


class FenceError(AssertionError):
    """view: the name of the nearest view; distance: of the nearest damaged byte, negative in front of the view, positive behind it,
    0 inside it (an input that was written); span: the same for the farthest damaged byte of that side; count: damaged bytes in all."""

    def __init__(self, msg, view, distance, span, count):
        super().__init__(msg)
        self.view, self.distance, self.span, self.count = view, distance, span, count


class View:
    def __init__(self, name, start, n, is_out):
        self.name, self.start, self.end, self.is_out = name, start, start + n, is_out

    def distance(self, i):
        return i - self.start if i < self.start else i - self.end + 1 if i >= self.end else 0


def _plural(d):
    return "%d byte%s" % (d, "" if d == 1 else "s")


class Arena:
    def __init__(self, device="cpu", salt=0, size=1 << 20):
        i = np.arange(size, dtype=np.int64)
        self.device, self.salt, self.size = torch.device(device), salt, size
        self.pattern = torch.from_numpy((((i * 131 + 89) ^ salt) & 0xFF).astype(np.uint8)).to(self.device)
        self.buf = self.pattern.clone()                   # what the calls see
        self.expect = self.pattern.clone()                # what every guarded byte must still be
        self.guard = torch.ones(size, dtype=torch.bool, device=self.device)
        self.views, self.top = [], 0

    def reset(self):
        """The pattern again, no views: one arena serves many calls."""
        self.buf.copy_(self.pattern)
        self.expect.copy_(self.pattern)
        self.guard.fill_(True)
        self.views, self.top = [], 0

    def _place(self, n, phase, kind):
        assert 0 <= phase < LINE
        s = self.top + FENCE
        s += (phase - (address(self.buf) + s)) % LINE
        if s + n + FENCE > self.size:
            raise MemoryError("arena of %d bytes is full" % self.size)
        self.top = s + n + FENCE                          # fences are not shared between neighbours
        v = View("%s#%d" % (kind, 1 + sum(1 for w in self.views if w.is_out == (kind == "out"))), s, n, kind == "out")
        self.views.append(v)
        return v

    def _fill(self, at, data):
        if len(data):
            t = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy())
            t = t.to(self.device)
            self.buf[at:at + len(data)] = t
            self.expect[at:at + len(data)] = t

    def put(self, data, phase, before=None, after=None):
        """A view of len(data) bytes that holds data (bytes, or a uint8 tensor), its address = phase mod 128.  before / after replace
        the fence bytes nearest the data; they stay part of the fence."""
        before, after = before or b"", after or b""
        assert len(before) < FENCE and len(after) < FENCE
        v = self._place(len(data), phase, "in")
        self._fill(v.start - len(before), before)
        self._fill(v.start, data)
        self._fill(v.end, after)
        return self.buf[v.start:v.end]

    def out(self, n, phase):
        """A view of exactly n bytes for an output; it carries the pattern."""
        v = self._place(n, phase, "out")
        self.guard[v.start:v.end] = False
        return self.buf[v.start:v.end]

    def check(self):
        """Raises FenceError when a byte that was not handed out as an output differs from what was put there."""
        bad = (self.buf != self.expect) & self.guard
        if not bool(bad.any()):
            return
        idx = torch.nonzero(bad).flatten().cpu().numpy().astype(np.int64)
        assert self.views, "a damaged arena without a view"
        dist = np.stack([np.where(idx < v.start, idx - v.start, np.where(idx >= v.end, idx - v.end + 1, 0)) for v in self.views])
        owner = np.abs(dist).argmin(axis=0)                       # the view each damaged byte is nearest to
        mine = dist[owner, np.arange(len(idx))]
        k = int(np.abs(mine).argmin())
        i0, d, v = int(idx[k]), int(mine[k]), self.views[int(owner[k])]
        side = mine[(owner == owner[k]) & (np.sign(mine) == np.sign(d))]
        far = int(side[np.abs(side).argmax()])
        where = "%s behind %s" % (_plural(d), v.name) if d > 0 else "%s in front of %s" % (_plural(-d), v.name) if d < 0 else "inside %s (an input)" % v.name
        msg = "%s (arena index %d holds 0x%02x, not 0x%02x); %d damaged in all, the farthest of that side %s away" % (
            where, i0, int(self.buf[i0]), int(self.expect[i0]), len(idx), _plural(abs(far)))
        raise FenceError(msg, v.name, d, far, len(idx))
