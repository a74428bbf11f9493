"""Host tests of tests/arena.py on CPU tensors: a guard checker that never fails proves nothing, so the checker is tested first.
Alignment, disjointness, the guard-size rule, the row-gap accounting of strided views, what the patterns decode to, and the
detection of ONE scribbled byte before, between the rows of, and behind a buffer, with the buffer's name and the byte's offset."""
import numpy as np
import pytest
import torch

from tests.arena import ALIGN, GUARD_ROWS, MAX_FLAT_GUARD, MIN_GUARD, NAN_PATTERN, QUIET_PATTERN, Arena, GuardError, guard_bytes, pattern_bytes

PLACEMENTS = [  # shape, dtype, ld, kind
    ((5, 7), torch.float32, None, "in"),
    ((5, 7), torch.float32, 11, "out"),
    ((3,), torch.int32, None, "in"),
    ((2, 3, 130), torch.int16, 192, "out"),
    ((1001,), torch.uint8, None, "work"),
    ((300, 100), torch.float32, 104, "inout"),
    ((4,), torch.float64, None, "work"),
    ((2, 9), torch.int32, 12, "out"),
]


def build(pattern):
    ar = Arena("cpu", pattern, capacity=8 << 20)
    for i, (shape, dtype, ld, kind) in enumerate(PLACEMENTS):
        ar.place(shape, dtype, ld=ld, kind=kind, name=f"b{i}")
    return ar


def test_patterns_decode_as_nan_in_fp32_and_bf16():
    b = pattern_bytes(NAN_PATTERN)
    assert np.isnan(b.view("<f4")[0])
    for half in b.view("<u2"):
        assert np.isnan((np.uint32(half) << 16).astype("<u4").view("<f4"))     # a bf16 is the upper half of an fp32
        assert torch.tensor([int(half)], dtype=torch.int32).to(torch.int16).view(torch.bfloat16).isnan().all()
    ar = build(NAN_PATTERN)
    out = ar.buffer("b1").view
    assert out.isnan().all()                                 # prefilled fp32 result
    img = ar.buffer("b3").view
    assert img.view(torch.bfloat16).isnan().all()            # prefilled bf16 image (kept as int16 bits)
    assert (ar.buffer("b7").view == NAN_PATTERN).all()       # an int32 result shows the pattern as an integer
    assert pattern_bytes(QUIET_PATTERN).view("<f4")[0] == 0.0
    quiet = build(QUIET_PATTERN)
    assert int(quiet.mem.count_nonzero()) == 0


def test_alignment_and_views():
    ar = build(NAN_PATTERN)
    for b, (shape, dtype, ld, kind) in zip(ar.buffers, PLACEMENTS):
        assert b.start % ALIGN == 0 and b.view.data_ptr() % ALIGN == 0
        assert b.view.data_ptr() == ar.mem.data_ptr() + b.start
        assert tuple(b.view.shape) == shape and b.view.dtype == dtype
        assert b.view.stride(-1) == 1
        if len(shape) > 1:
            assert b.view.stride(-2) == (ld or shape[-1])
        if len(shape) == 3:
            assert b.view.stride(0) == shape[1] * ld
    view, ptr = Arena("cpu", QUIET_PATTERN, capacity=1 << 20).place((3, 5), torch.float32, ld=8)
    assert ptr == view.data_ptr() and view.stride() == (8, 1)


def test_placements_are_disjoint_and_guards_follow_the_rule():
    ar = build(NAN_PATTERN)
    spans = []
    for b in ar.buffers:
        flat = len(b.shape) == 1
        assert b.guard >= MIN_GUARD and b.guard >= (min(b.span, MAX_FLAT_GUARD) if flat else GUARD_ROWS * b.ld * b.itemsize)
        assert b.guard == guard_bytes(b.ld, b.itemsize, b.shape[0] if flat else None)
        assert b.start - b.guard >= 0 and b.end + b.guard <= ar.capacity      # a whole extra tile of rows stays inside
        spans.append((b.start - b.guard, b.start, b.end, b.end + b.guard))
    for (_, _, end, hi), (lo, start, _, _) in zip(spans, spans[1:]):
        assert hi <= start and end <= lo          # a buffer's guards never reach into its neighbour's valid bytes
    big = ar.buffer("b3")
    assert big.guard == GUARD_ROWS * 192 * 2
    assert guard_bytes(1, 4) == MIN_GUARD
    flat = Arena("cpu", QUIET_PATTERN, capacity=32 << 20)       # a flat buffer: its own size, between 64 KiB and 4 MiB
    for n, want in ((10, MIN_GUARD), (100000, 100096), (3 << 20, 3 << 20), (5 << 20, MAX_FLAT_GUARD)):
        flat.place((n,), torch.uint8, kind="work", name=f"w{n}")
        assert flat.buffer(f"w{n}").guard == want


def test_guards_of_int32_inputs_are_zero_and_others_hold_the_pattern():
    ar = build(NAN_PATTERN)
    for b in ar.buffers:
        before = ar.mem[b.start - b.guard:b.start]
        behind = ar.mem[b.end:b.end + b.guard]
        if b.dtype == torch.int32 and b.kind == "in":
            assert b.zero_guard and int(before.count_nonzero()) == 0 and int(behind.count_nonzero()) == 0
        else:
            assert not b.zero_guard
            for off, region in ((b.start - b.guard, before), (b.end, behind)):
                want = np.resize(np.roll(pattern_bytes(NAN_PATTERN), -(off % 4)), region.numel())
                assert np.array_equal(region.numpy(), want)
    ar.check()
    build(QUIET_PATTERN).check()


def test_row_gaps_count_as_guard():
    ar = Arena("cpu", NAN_PATTERN, capacity=1 << 20)
    v, _ = ar.place((4, 5), torch.float32, ld=8, kind="out", name="c")
    b = ar.buffer("c")
    assert (b.rows, b.cols, b.ld, b.row_bytes, b.ld_bytes, b.gap_bytes) == (4, 5, 8, 20, 32, 12)
    assert b.span == (3 * 8 + 5) * 4          # the last row has no gap: what follows it is "behind"
    assert ar.unwritten("c") == 20
    v.copy_(torch.arange(20, dtype=torch.float32).reshape(4, 5))      # writing every valid element ...
    assert ar.unwritten("c") == 0
    ar.check()                                                        # ... leaves every gap alone
    v[2, 3] = float("nan")
    assert ar.unwritten("c") == 0             # an honest NaN has other bits than the pattern's low half ... unless it is the pattern
    flat = ar.mem[b.start:b.end].view(torch.float32)
    gaps = torch.stack([flat[r * 8 + 5:r * 8 + 8] for r in range(3)])
    assert gaps.isnan().all()
    one_d = Arena("cpu", NAN_PATTERN, capacity=1 << 20)
    one_d.place((7,), torch.float32, name="v")
    assert one_d.buffer("v").gap_bytes == 0


SCRIBBLES = [  # buffer, byte offset relative to the buffer, where
    ("b1", -1, "before"), ("b1", -65536, "before"),
    ("b1", 7 * 4, "between rows"), ("b1", 3 * 44 + 43, "between rows"),
    ("b1", (4 * 11 + 7) * 4, "behind"), ("b1", (4 * 11 + 7) * 4 + 65535, "behind"),
    ("b2", -3, "before"), ("b2", 12, "behind"),
    ("b3", 130 * 2, "between rows"), ("b3", 5 * 384 - 1, "between rows"), ("b3", (5 * 192 + 130) * 2, "behind"),
    ("b4", 1001, "behind"), ("b4", -1, "before"),
    ("b7", 9 * 4 + 5, "between rows"),
]


@pytest.mark.parametrize("pattern", [NAN_PATTERN, QUIET_PATTERN])
@pytest.mark.parametrize("name,offset,where", SCRIBBLES)
def test_one_scribbled_byte_is_found(pattern, name, offset, where):
    ar = build(pattern)
    ar.check()
    b = ar.buffer(name)
    at = b.start + offset
    ar.mem[at] = ar.mem[at] ^ 0x01
    assert ar.damage(name)[:3] == (where, offset, offset)
    with pytest.raises(GuardError) as e:
        ar.check()
    msg = str(e.value)
    assert f"'{name}'" in msg and where in msg and f"offset {offset}," in msg and f"last at {offset} " in msg
    for other in ar.buffers:       # a byte in one buffer's guard is charged to that buffer (and to a neighbour whose band it shares)
        if other.name != name and ar.damage(other) is not None:
            assert other.start - other.guard <= at < other.end + other.guard
    ar.mem[at] = ar.mem[at] ^ 0x01
    ar.check()


def test_a_run_of_bytes_reports_first_and_last():
    ar = build(NAN_PATTERN)
    b = ar.buffer("b5")            # [300][100] floats, ld 104
    ar.mem[b.start + 100 * 4 + 2] = 0                          # row 0's gap
    ar.mem[b.start + 200 * 416 + 415] = 0                      # row 200's gap, its last byte
    ar.mem[b.end + 9] = 1                                      # and behind
    where, first, last, hits = ar.damage("b5")
    assert (where, first, last) == ("between rows", 402, b.span + 9)
    assert hits == [("between rows", 402, 200 * 416 + 415), ("behind", b.span + 9, b.span + 9)]


def test_writes_inside_a_buffer_are_not_damage():
    ar = build(NAN_PATTERN)
    for b in ar.buffers:
        b.view.zero_()
    ar.check()


def test_arena_refuses_to_outgrow_its_allocation():
    ar = Arena("cpu", QUIET_PATTERN, capacity=1 << 20)
    with pytest.raises(MemoryError):
        ar.place((1024, 1024), torch.float32)
