"""Guard bands around kernel outputs: one allocation per output, filled with a canary, with the view a kernel is handed in
the middle of it.

Outputs here are laid out `[T][n][B]`.  A store past a ragged cell group lands on the next row (where that row's own store
usually hides it) or, from the last row, behind the buffer: in the allocator's slack, the free tail of a history chunk or a
neighbouring tensor, none of which a value test reads.  An element that is NOT stored at a ragged edge is as invisible: a
fresh `torch.empty` often holds the rows a previous call left there.  An arena makes both visible:

    arena = GuardArena("nan")                      # or "finite"; every case runs once with each
    rates = arena.view((T, n, B), torch.float32, device)
    ... launch the kernel on `rates` ...
    got = arena.check(rates)                       # guards untouched, interior all written -> the interior (NumPy)
    arena2.check(rates2, other=got)                # ... and the same bits whatever the memory held before

The guard on each side is at least max(4096, 64 * B) elements (64 cells: the widest chunk a workgroup of the generic rate
kernel walks), so the overrun of one cell group of any kernel stays inside the arena.

Canaries: "nan" is a quiet NaN with a payload (a kernel that reads its output before writing it, or that skips a store,
leaves or spreads it; the comparison is on bits), "finite" a value no kernel produces (-7.0: rates are clamped or sums of
non-negative terms, state rows are positions, unit vectors, speeds).  Bytes (spikes are 0 / 1) get 0xEE and 0xD7, 2-byte
elements (bin ids) 0xBEEF and 0x5A5A.

Two more modes, for the kernels whose contract is not "every element of the output, once":

    arena.check(future, written=mask)              # True: must be written; False: must still hold the canary's bits
    arena.check(state, inplace=True)               # pre-filled by the test, updated in place: guards (and `other`) only

What this cannot see: reads out of bounds; a stray store that lands INSIDE the view on an element its owner overwrites later
(the T = 1 cases exist because there every store past the last cell leaves the view); strays further than the guard."""
import numpy as np
import torch

MIN_GUARD = 4096
WIDEST_CHUNK = 64            # cells per workgroup chunk of rate_kernel_generic

# canary bit patterns by element size (bytes); the float ones are the bits of a quiet NaN with a payload / of -7.0
# 2-byte elements are the rate maps' bin ids (uint16): neither canary is RIAB_RATEMAP_DROPPED (0xFFFF) or a valid bin id
# (below RIAB_RATEMAP_MAX_BINS = 4096)
_BITS = {"nan": {1: 0xEE, 2: 0xBEEF, 4: 0x7FC0BEEF, 8: 0x7FF80000DEADBEEF},
         "finite": {1: 0xD7, 2: 0x5A5A, 4: 0xC0E00000, 8: 0xC01C000000000000}}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def canary_bits(canary, itemsize):
    """the canary's bit pattern as the signed integer `Tensor.view(int type)` shows (bytes: unsigned)"""
    bits = _BITS[canary][itemsize]
    if itemsize > 1 and bits >= 1 << (8 * itemsize - 1):
        bits -= 1 << (8 * itemsize)
    return bits


def guard_elements(shape):
    return max(MIN_GUARD, WIDEST_CHUNK * int(shape[-1]))


def coords(rel, shape):
    """flat element offset relative to the view's first element -> its index in the view's layout, the FIRST coordinate
    unbounded: for (T, n, B) an offset behind the view is (T + k, cell, b), one in front of it (-1 - k, cell, b)"""
    out = []
    for d in reversed(shape[1:]):
        rel, r = divmod(int(rel), int(d))
        out.append(r)
    out.append(rel)
    return tuple(reversed(out))


UNTOUCHED = "written where the contract says untouched"


class GuardError(AssertionError):
    """kind: "front guard" | "back guard" | "unwritten" | "canary-dependent" | UNTOUCHED; first, last: the coordinates
    (see `coords`) of the first and last offending element; count: how many"""

    def __init__(self, kind, first, last, count, shape):
        self.kind, self.first, self.last, self.count = kind, first, last, count
        super().__init__(f"{kind}: {count} element(s) of a view {tuple(shape)}, first at {first}, last at {last}")


class _Slot:
    def __init__(self, buf, front, shape, view):
        self.buf, self.front, self.shape, self.view = buf, front, tuple(shape), view


class GuardArena:
    def __init__(self, canary):
        assert canary in _BITS, canary
        self.canary = canary
        self._slots = {}

    def view(self, shape, dtype=torch.float32, device="cpu"):
        """a contiguous, 16-byte-aligned view of `shape` in the middle of ONE canary-filled allocation"""
        shape = tuple(int(d) for d in shape)
        size = torch.empty((), dtype=dtype).element_size()
        numel = int(np.prod(shape))
        guard = guard_elements(shape)
        per16 = max(16 // size, 1)
        buf = torch.empty(guard + per16 + numel + guard + per16, dtype=dtype, device=device)
        buf.view(_INT[size]).fill_(canary_bits(self.canary, size))
        addr = buf.data_ptr() + guard * size
        front = guard + ((-addr) % 16) // size
        v = buf[front:front + numel].view(shape)
        assert v.data_ptr() % 16 == 0 and v.is_contiguous() and front >= guard and len(buf) - front - numel >= guard
        self._slots[v.data_ptr()] = _Slot(buf, front, shape, v)
        return v

    def base(self, view):
        """the whole allocation behind `view` (for a control that writes into the guard on purpose)"""
        return self._slots[view.data_ptr()].buf

    def check(self, view, other=None, written=None, inplace=False):
        """Asserts: both guards of `view` are the canary, bit for bit; no interior element is; with `other` (the interior
        `check` returned for the other canary's run), the two interiors are the same bits.  -> the interior (NumPy).

        written: a boolean array of the view's shape, for an output whose contract leaves some elements alone.  Elements
        with True must not hold the canary ("unwritten"), elements with False must still hold it, bit for bit ("written
        where the contract says untouched"); `other` compares the True elements only (the others are the two canaries).
        inplace: the view is state the kernel updates in place and the test pre-filled with real values: the guards are
        checked, nothing is "unwritten" by its bits, `other` compares the whole interior."""
        assert written is None or not inplace
        s = self._slots[view.data_ptr()]
        size = s.buf.element_size()
        numel = int(np.prod(s.shape))
        word = canary_bits(self.canary, size)
        bits = s.buf.view(_INT[size])
        for kind, lo, hi in (("front guard", 0, s.front), ("back guard", s.front + numel, len(bits))):
            hit = torch.nonzero(bits[lo:hi] != word).flatten()
            if len(hit):
                first, last = int(hit[0]) + lo - s.front, int(hit[-1]) + lo - s.front
                raise GuardError(kind, coords(first, s.shape), coords(last, s.shape), len(hit), s.shape)
        is_canary = (bits[s.front:s.front + numel] == word).cpu().numpy()
        mask = None
        if written is not None:
            mask = np.asarray(written)
            assert mask.dtype == np.bool_ and mask.shape == s.shape, (mask.dtype, mask.shape, s.shape)
            mask = mask.reshape(-1)
        if not inplace:
            hit = np.nonzero(is_canary if mask is None else is_canary & mask)[0]
            if len(hit):
                raise GuardError("unwritten", coords(hit[0], s.shape), coords(hit[-1], s.shape), len(hit), s.shape)
        if mask is not None:
            hit = np.nonzero(~is_canary & ~mask)[0]
            if len(hit):
                raise GuardError(UNTOUCHED, coords(hit[0], s.shape), coords(hit[-1], s.shape), len(hit), s.shape)
        got = s.view.detach().cpu().numpy().copy()
        if other is not None:
            a = got.reshape(-1).view(f"u{size}")
            b = np.ascontiguousarray(other).reshape(-1).view(f"u{size}")
            assert a.shape == b.shape, (got.shape, np.shape(other))
            hit = np.nonzero(a != b if mask is None else (a != b) & mask)[0]
            if len(hit):
                raise GuardError("canary-dependent", coords(hit[0], s.shape), coords(hit[-1], s.shape), len(hit), s.shape)
        return got


CANARIES = ("nan", "finite")
