"""A guarded arena for the containment tests (tests/test_gpu_containment.py; the contract is DESIGN.md "Containment").

An Arena owns ONE torch.uint8 allocation.  place() carves buffers out of it at 256-byte-aligned offsets; before and behind every
buffer lies a guard band, and the columns between the valid extent and the leading dimension of a strided view (the row gaps)
count as guard too.  A kernel that indexes a little past an operand, a ragged last tile of a result or the declared size of a
workspace therefore lands in memory the test owns, and check() finds the changed bytes and says where they are.

Guard content.  The NaN arena fills everything with the 32-bit pattern 0x7FC07FC0: a quiet NaN as fp32, and each half a quiet NaN
as bf16, so a result that depends on a byte outside its operands turns NaN.  The guards of int32 INPUTS (targets, sizes, key
lengths, frame counts) are zero bytes in every arena: a stray integer read must not become a wild index.  The quiet arena
(guard_pattern = 0) is zero everywhere; two arenas built by the same sequence of place() calls have the same layout, so a case
run in both differs in nothing but the bytes it must not depend on.

Guard size: at least 64 KiB and at least 256 rows of the buffer's own leading dimension, so an overrun by a whole extra tile of
rows still lands in a guard, inside the allocation.  A flat buffer (a vector, a workspace) has no leading dimension: its guard is
64 KiB or the buffer's own size, whichever is larger, up to 4 MiB -- a second pass over the whole buffer still lands in it.

No fixtures here, and nothing that makes a kernel fault: the arena only watches legal calls."""
import numpy as np
import torch

NAN_PATTERN = 0x7FC07FC0
QUIET_PATTERN = 0
ALIGN = 256
MIN_GUARD = 64 * 1024
GUARD_ROWS = 256
KINDS = ("in", "out", "inout", "work")


def _align(n, a=ALIGN):
    return (n + a - 1) // a * a


MAX_FLAT_GUARD = 4 << 20


def guard_bytes(ld, itemsize, flat_elems=None):
    """the rule above, rounded up to the placement alignment; flat_elems: the element count of a one-dimensional buffer"""
    if flat_elems is not None:
        return _align(max(MIN_GUARD, min(flat_elems * itemsize, MAX_FLAT_GUARD)))
    return _align(max(MIN_GUARD, GUARD_ROWS * ld * itemsize))


def pattern_bytes(pattern):
    return np.array([pattern], dtype="<u4").view(np.uint8)


class Placed:
    """one buffer of an arena: `start` / `end` are byte offsets of its first byte and one past its last valid byte"""

    def __init__(self, name, kind, dtype, shape, ld, start, guard, zero_guard):
        self.name, self.kind, self.dtype, self.shape, self.ld = name, kind, dtype, tuple(shape), ld
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.cols = self.shape[-1]
        self.rows = int(np.prod(self.shape[:-1], dtype=np.int64)) if len(self.shape) > 1 else 1
        self.start, self.guard, self.zero_guard = start, guard, zero_guard
        self.span = ((self.rows - 1) * ld + self.cols) * self.itemsize
        self.end = start + self.span
        self.row_bytes, self.ld_bytes = self.cols * self.itemsize, ld * self.itemsize
        self.gap_bytes = self.ld_bytes - self.row_bytes if self.rows > 1 else 0
        self.view = None


class GuardError(AssertionError):
    pass


class Arena:
    def __init__(self, device, guard_pattern, capacity=32 << 20):
        self.device = torch.device(device)
        self.pattern = int(guard_pattern)
        self.capacity = _align(capacity)
        self._alloc = torch.empty(self.capacity + ALIGN, dtype=torch.uint8, device=self.device)   # the one allocation
        skew = -self._alloc.data_ptr() % ALIGN      # host allocations are not 256-byte aligned
        self.mem = self._alloc[skew:skew + self.capacity]
        self._fill(self.mem, 0, self.pattern)
        self.buffers = []
        self._strips = {}

    # ---- patterns ------------------------------------------------------------------------------------------------------------
    def _fill(self, region, offset, pattern):
        """region (uint8, contiguous, starting at arena byte `offset`) <- the pattern in the phase of its position"""
        if pattern == 0:
            region.zero_()
            return
        p = pattern_bytes(pattern)
        n = region.numel()
        reps = torch.from_numpy(np.roll(p, -(offset % 4)).copy()).to(self.device)
        region.copy_(reps.repeat((n + 3) // 4)[:n])

    def _strip(self, pattern, n):
        """a run of at least n pattern bytes starting in phase 0 (expected guard content, shared by all checks)"""
        have = self._strips.get(pattern)
        if have is None or have.numel() < n:
            have = torch.empty(_align(n, 1 << 16), dtype=torch.uint8, device=self.device)
            self._fill(have, 0, pattern)
            self._strips[pattern] = have
        return have

    def _pattern_of(self, b):
        return 0 if b.zero_guard else self.pattern

    # ---- placement -----------------------------------------------------------------------------------------------------------
    def place(self, shape, dtype, ld=None, kind="in", name=None, data=None):
        """carve a buffer: a view of `shape` whose rows are `ld` elements apart (default: shape[-1], no gaps) and its data_ptr().
        `data` (numpy or torch, shape `shape`) is copied into the valid elements; out / work buffers are prefilled with the guard
        pattern instead, so an element the call never writes still shows it."""
        assert kind in KINDS, kind
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        assert len(shape) >= 1 and all(s >= 1 for s in shape), shape
        ld = shape[-1] if ld is None else int(ld)
        assert ld >= shape[-1], (ld, shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        zero_guard = self.pattern == 0 or (dtype == torch.int32 and kind == "in")
        guard = guard_bytes(ld, itemsize, shape[0] if len(shape) == 1 else None)
        if self.buffers:
            prev = self.buffers[-1]
            band = max(prev.guard, guard) if prev.zero_guard == zero_guard else prev.guard + guard
            start = _align(prev.end + band)
        else:
            start = guard
        b = Placed(name or f"buf{len(self.buffers)}", kind, dtype, shape, ld, start, guard, zero_guard)
        if b.end + guard > self.capacity:
            raise MemoryError(f"arena of {self.capacity} bytes is too small for {b.name} (needs {b.end + guard})")
        if zero_guard and self.pattern != 0:
            self.mem[start - guard:b.end + guard].zero_()
        strides, acc = [1], ld
        for s in reversed(shape[1:-1]):
            strides.insert(0, acc)
            acc *= s
        if len(shape) > 1:
            strides.insert(0, acc)
        flat = self.mem[start:start + _align(b.span, itemsize)].view(dtype)
        b.view = flat.as_strided(shape, strides)
        if data is not None:
            assert kind in ("in", "inout"), kind
            src = torch.from_numpy(np.ascontiguousarray(data)) if isinstance(data, np.ndarray) else data
            assert tuple(src.shape) == shape, (tuple(src.shape), shape)
            b.view.copy_(src.to(dtype=dtype).to(self.device))
        elif kind in ("out", "work"):
            self.prefill(b)
        self.buffers.append(b)
        return b.view, b.view.data_ptr()

    def prefill(self, b):
        """the guard pattern into the valid elements of an out / work buffer"""
        b = self._find(b)
        self._fill(self.mem[b.start:b.end], b.start, self._pattern_of(b))   # the whole span: the row gaps hold the same pattern

    def _find(self, b):
        if isinstance(b, Placed):
            return b
        for c in self.buffers:
            if c.name == b or (torch.is_tensor(b) and c.view.data_ptr() == b.data_ptr() and c.view.shape == b.shape):
                return c
        raise KeyError(b)

    def buffer(self, which):
        return self._find(which)

    def unwritten(self, which):
        """number of valid elements of a buffer whose bits are still the prefill pattern (the NaN arena only: in the quiet arena
        the prefill is zero, which a result may legitimately hold)"""
        b = self._find(which)
        assert self.pattern != 0
        rows = self._rows(b.start, b.rows, b.row_bytes, b.ld_bytes)
        want = self._expected_rows(b, b.start, b.rows, b.row_bytes)
        same = (rows == want).reshape(b.rows, b.cols, b.itemsize).all(dim=2)
        return int(same.sum().item())

    def _rows(self, first, rows, width, pitch):
        """`rows` runs of `width` arena bytes, `pitch` apart, the first at arena byte `first`"""
        return self.mem.as_strided((rows, width), (pitch, 1), self.mem.storage_offset() + first)

    # ---- checking ------------------------------------------------------------------------------------------------------------
    def _expected_rows(self, b, first, rows, width):
        """expected guard bytes of `rows` runs of `width` bytes, `ld_bytes` apart, the first at arena byte `first`"""
        step = b.ld_bytes % 4
        strip = self._strip(self._pattern_of(b), first % 4 + rows * step + width + 4)
        return strip.as_strided((rows, width), (step, 1), first % 4)

    def _regions(self, b):
        """(where, offset of the region relative to the buffer, actual bytes, expected bytes), each 2-D"""
        lo = b.start - b.guard
        out = [("before", -b.guard, self.mem[lo:b.start].unsqueeze(0), self._expected_rows(b, lo, 1, b.guard))]
        if b.gap_bytes:
            first = b.start + b.row_bytes
            out.append(("between rows", b.row_bytes, self._rows(first, b.rows - 1, b.gap_bytes, b.ld_bytes),
                        self._expected_rows(b, first, b.rows - 1, b.gap_bytes)))
        out.append(("behind", b.span, self.mem[b.end:b.end + b.guard].unsqueeze(0), self._expected_rows(b, b.end, 1, b.guard)))
        return out

    def damage(self, which):
        """None when every guard byte of the buffer holds its pattern, else (where, first, last): the place of the first
        changed byte and the first and last changed byte offsets relative to the buffer's first byte"""
        b = self._find(which)
        regions = self._regions(b)
        bad = torch.cat([(got != want).reshape(-1) for _, _, got, want in regions])
        if not bool(bad.any().item()):       # the one reduction of a clean buffer
            return None
        hits = []
        for where, rel, got, want in regions:
            idx = (got != want).nonzero()
            if idx.numel():
                offs = rel + idx[:, 0] * (b.ld_bytes if where == "between rows" else 0) + idx[:, 1]
                hits.append((where, int(offs.min().item()), int(offs.max().item())))
        first = min(hits, key=lambda h: h[1])
        return first[0], first[1], max(h[2] for h in hits), hits

    def check(self):
        """every guard byte of every buffer against its pattern; raises GuardError naming each damaged buffer"""
        msgs = []
        for b in self.buffers:
            d = self.damage(b)
            if d is not None:
                where, lo, hi, hits = d
                parts = ", ".join(f"{w}: bytes {a}..{z}" for w, a, z in hits)
                msgs.append(f"guard of '{b.name}' ({b.kind}, shape {b.shape}, ld {b.ld}, {b.span} bytes) changed, first {where}: "
                            f"first changed byte at offset {lo}, last at {hi} relative to the buffer ({parts})")
        if msgs:
            raise GuardError("; ".join(msgs))
