"""The arena of tests/redzone_common.py checks what it claims to (no GPU: the 'kernels' here are torch stores on the CPU)."""
import pytest
import torch

import redzone_common as RZ

CPU = torch.device('cpu')


def arena(fill=RZ.FILL_NAN):
    ar = RZ.Arena(CPU, fill, capacity=1 << 20)
    x = ar.inp(torch.arange(12, dtype=torch.float32).view(3, 4), 'x', ld=6)
    y = ar.out((3, 5), 'y', ld=7)
    ws = ar.scratch(100, 'workspace')
    ar.out((7,), 'vector').fill_(2.0)           # one-dimensional and three-dimensional buffers carve too
    ar.inp(torch.zeros(2, 3, 4, dtype=torch.int64), 'ids')
    return ar, x, y, ws


def flat(ar, view):
    """The arena as floats from a view's first element on."""
    off = view.data_ptr() - ar.mem.data_ptr()
    return ar.mem[off:off + (ar.mem.numel() - off) // 4 * 4].view(torch.float32)


@pytest.mark.parametrize('fill', RZ.FILLS)
def test_layout_and_a_clean_call(fill):
    ar, x, y, ws = arena(fill)
    for t in (x, y, ws):
        assert t.data_ptr() % RZ.ALIGN == 0
    assert y.data_ptr() - (x.data_ptr() + (2 * 6 + 4) * 4) >= RZ.ZONE and ws.numel() == 100
    assert x.stride() == (6, 1) and y.stride() == (7, 1) and torch.equal(x, torch.arange(12.).view(3, 4))
    assert (RZ.bits(y) == RZ._i32(fill)).all() and (RZ.bits(flat(ar, x)[4:6]) == RZ._i32(fill)).all()
    assert not ar.untouched()                    # the vector above was written
    y.copy_(torch.ones(3, 5))
    ws.fill_(7)
    ar.check()


def test_a_store_past_the_end_of_an_output_is_caught():
    ar, x, y, ws = arena()
    y.copy_(torch.ones(3, 5))
    flat(ar, y)[2 * 7 + 5] = 1.0                    # one element past the last row
    with pytest.raises(AssertionError, match="past the end of 'y'"):
        ar.check()


def test_a_store_before_a_workspace_and_a_whole_stray_tile_row_are_caught():
    ar, x, y, ws = arena()
    y.copy_(torch.ones(3, 5))
    off = ws.data_ptr() - ar.mem.data_ptr()
    ar.mem[off - 1] = 0
    with pytest.raises(AssertionError, match="before 'workspace'"):
        ar.check()
    ar, x, y, ws = arena()
    y.copy_(torch.ones(3, 5))
    flat(ar, y)[3 * 7:3 * 7 + 64 * 64] = 0.0         # 16 KiB right behind the buffer: inside the zone, not in the next buffer
    with pytest.raises(AssertionError, match='red zone'):
        ar.check()
    assert torch.equal(ws, ar._pristine[off:off + 100])


def test_a_changed_input_and_overwritten_input_padding_are_caught():
    ar, x, y, ws = arena()
    y.copy_(torch.ones(3, 5))
    x[1, 2] = -0.0 if float(x[1, 2]) == 0.0 else -float(x[1, 2])
    with pytest.raises(AssertionError, match="inside input 'x'"):
        ar.check()
    ar, x, y, ws = arena()
    y.copy_(torch.ones(3, 5))
    flat(ar, x)[4] = 0.0                             # the padding between rows 0 and 1 of the strided input
    with pytest.raises(AssertionError, match="inside input 'x'"):
        ar.check()


def test_output_padding_and_unwritten_elements_are_caught():
    ar, x, y, ws = arena()
    y.copy_(torch.ones(3, 5))
    flat(ar, y)[5] = 1.0                             # row padding of the strided output
    with pytest.raises(AssertionError, match="row padding of 'y'"):
        ar.check()
    ar, x, y, ws = arena()
    y[:2].copy_(torch.ones(2, 5))                    # the last row never written
    with pytest.raises(AssertionError, match='5 elements of output .y. never written'):
        ar.check()


def test_the_nan_sentinel_is_not_the_nan_of_a_masked_row_and_bit_equal_sees_signed_zero():
    ar, x, y, ws = arena(RZ.FILL_NAN)
    y.copy_(torch.full((3, 5), float('nan')))        # 0x7FC00000: data, not the sentinel
    ar.check()
    assert RZ.bit_equal(torch.tensor([float('nan')]), torch.tensor([float('nan')]))
    assert not RZ.bit_equal(torch.tensor([0.0]), torch.tensor([-0.0]))


def test_an_arena_that_is_too_small_says_so():
    ar = RZ.Arena(CPU, RZ.FILL_BIG, capacity=256 << 10)
    ar.scratch(1000, 'a')
    with pytest.raises(RuntimeError, match='too small'):
        ar.scratch(200 << 10, 'b')
