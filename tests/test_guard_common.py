"""The guard-band helper of the kernel tests (tests/guard_common.py), on the CPU."""
import math

import pytest
import torch

from guard_common import (ALIGN, BUFS_LEAD, BUFS_TAIL, SENTINEL, Bufs, assert_guards_intact, guarded, guarded_like, guarded_matrix, padded_stream, poison_bits, x_tail)


def test_guarded_view_alignment_contiguity_and_poison():
    for shape, lead, tail in (((3, 300, 128), 5, x_tail(128)), ((7,), 0, 1), ((2, 33, 32), 1000, 17)):
        view, base = guarded(shape, lead, tail, device="cpu")
        assert view.shape == shape and view.dtype == torch.float32 and view.is_contiguous()
        assert view.data_ptr() % ALIGN == 0
        assert view.contiguous().data_ptr() == view.data_ptr()
        s = view.storage_offset() - base.storage_offset()
        assert s >= lead and base.numel() - s - view.numel() >= tail
        assert torch.isnan(base).all()                      # the view too, until filled
        view.fill_(1.0)
        assert torch.isnan(base[:s]).all() and torch.isnan(base[s + view.numel():]).all()
        assert int((base == 1.0).sum()) == math.prod(shape)
    assert x_tail(128) == (1 << 20) // 4 and x_tail(1024) == 512 * 1024


def test_guarded_like_and_sentinel_bits():
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    view, base = guarded_like(t, 4, 4, poison=SENTINEL)
    assert torch.equal(view, t)
    assert_guards_intact(base, view)
    assert poison_bits(SENTINEL) == SENTINEL and poison_bits(0xffffffff) == -1
    assert poison_bits(float("nan")) == 0x7fc00000 and poison_bits(1.0) == 0x3f800000


def test_padded_stream_layout():
    B, N, ld, stride = 3, 5, 12, 5 * 12 + 8
    st, base = padded_stream(B, N, ld, stride, poison=SENTINEL, device="cpu")
    assert st.shape == (B, N, ld) and st.stride() == (stride, ld, 1) and st.data_ptr() % ALIGN == 0
    s = st.storage_offset() - base.storage_offset()
    assert s >= stride and base.numel() - s - B * stride >= stride
    st[..., :N] = 2.0
    bits = base.view(torch.int32)
    assert int((base == 2.0).sum()) == B * N * N
    assert int((bits == SENTINEL).sum()) == base.numel() - B * N * N
    for b in range(B):                                      # element (b, i, j) at b * stride + i * ld + j
        for i in range(N):
            row = base[s + b * stride + i * ld:s + b * stride + (i + 1) * ld]
            assert (row[:N] == 2.0).all() and (row[N:].view(torch.int32) == SENTINEL).all()
        gap = base[s + b * stride + N * ld:s + (b + 1) * stride]
        assert gap.numel() == stride - N * ld and (gap.view(torch.int32) == SENTINEL).all()
    assert_guards_intact(base, st[..., :N])
    with pytest.raises(AssertionError):
        padded_stream(B, N, N - 1, stride, device="cpu")


@pytest.mark.parametrize("where", ["lead", "tail", "pad", "gap"])
def test_assert_guards_intact_catches_one_word(where):
    if where in ("lead", "tail"):
        view, base = guarded((4, 8), 16, 16, poison=SENTINEL, device="cpu")
        view.zero_()
        s = view.storage_offset()
        at = s - 1 if where == "lead" else s + view.numel()
        inner = view
    else:
        N, ld, stride = 4, 8, 4 * 8 + 4
        st, base = padded_stream(2, N, ld, stride, poison=SENTINEL, device="cpu")
        inner = st[..., :N]
        inner.zero_()
        s = st.storage_offset()
        at = s + 2 * ld + N + 1 if where == "pad" else s + N * ld + 2
    assert_guards_intact(base, inner)
    base.view(torch.int32)[at] = SENTINEL ^ 1              # still a NaN, one bit off
    with pytest.raises(AssertionError, match="1 guard word"):
        assert_guards_intact(base, inner)
    base.view(torch.int32)[at] = SENTINEL
    assert_guards_intact(base, inner)
    inner[(0,) * inner.dim()] = float("nan")                 # the view itself is not a guard
    assert_guards_intact(base, inner)


def test_guarded_matrix_layout():
    for P, C, ld, lead, tail in ((300, 12, 20, 7, 129 * 20), (1, 4, 4, 0, 1), (5, 8, 1032, 64, 129 * 1032)):
        m, base = guarded_matrix(P, C, ld, lead, tail, poison=SENTINEL, device="cpu")
        assert m.shape == (P, C) and m.stride() == (ld, 1) and m.data_ptr() % ALIGN == 0
        s = m.storage_offset() - base.storage_offset()
        assert s >= lead and base.numel() - s - P * ld >= tail
        bits = base.view(torch.int32)
        assert (bits == SENTINEL).all()                     # the view too, until filled
        m.fill_(3.0)
        assert int((base == 3.0).sum()) == P * C and int((bits == SENTINEL).sum()) == base.numel() - P * C
        for r in range(P):                                  # element (r, c) at r * ld + c; the pad columns of EVERY row hold poison
            row = base[s + r * ld:s + (r + 1) * ld]
            assert (row[:C] == 3.0).all() and (row[C:].view(torch.int32) == SENTINEL).all()
        assert (bits[:s] == SENTINEL).all() and (bits[s + P * ld:] == SENTINEL).all()
        assert_guards_intact(base, m)
        if ld > C:
            bits[s + (P - 1) * ld + C] = SENTINEL ^ 1       # a pad column of the last row
            with pytest.raises(AssertionError, match="1 guard word"):
                assert_guards_intact(base, m)
    with pytest.raises(AssertionError):
        guarded_matrix(4, 8, 7, 0, 0, device="cpu")


def test_bufs_put_every_tensor_in_guards_of_the_asked_size_and_see_one_word():
    for lead, tail in ((BUFS_LEAD, BUFS_TAIL), (64 * 152, 128 * 152)):
        g = Bufs(lead, tail, device="cpu")
        t = torch.arange(15, dtype=torch.float32).view(5, 3)
        a, b = g.fin(t), g.fin(t, ld=7)
        ix = g.iin(torch.tensor([3, 1, 2]), 9)
        d = g.din(torch.ones(2, 3, dtype=torch.float64))
        o, m = g.fout((4, 3)), g.mout(5, 3, 12, col0=4, wide=8)
        z, i, dd = g.fout((2,), zero=True), g.iout((3,)), g.dout((2, 2))
        assert torch.equal(a, t) and torch.equal(b, t) and b.stride() == (7, 1) and m.stride() == (12, 1)
        assert ix.dtype == torch.int32 and ix.tolist() == [3, 1, 2] and d.dtype == torch.float64 and bool((d == 1).all())
        assert i.dtype == torch.int32 and dd.dtype == torch.float64 and dd.shape == (2, 2) and not bool(z.any())
        assert len(g.items) == 9
        for base, v, poison in g.items:
            s = v.storage_offset() - base.storage_offset()
            assert s >= lead and (v.data_ptr() % ALIGN == 0 or v.data_ptr() == m.data_ptr())
            last = s + sum((n - 1) * st for n, st in zip(v.shape, v.stride()))
            assert base.numel() - 1 - last >= tail
        assert (o.view(torch.int32) == SENTINEL).all()          # outputs hold the sentinel until written
        pads = [x for x in g.items if x[1].data_ptr() == b.data_ptr()][0][0]
        assert int(torch.isnan(pads).sum()) == pads.numel() - 15        # the pad columns of an input are NaN
        guards = [x for x in g.items if x[1].data_ptr() == ix.data_ptr()][0][0]
        assert int((guards.view(torch.int32) == 9).sum()) == guards.numel() - 3      # the in-range index poison
        g.intact()
        o.zero_()
        m.zero_()
        g.intact()                                               # the views themselves are not guards
        base = [x for x in g.items if x[1].data_ptr() == m.data_ptr()][0][0]
        at = m.storage_offset() - base.storage_offset() + 3      # the column behind the slice, first row
        base.view(torch.int32)[at] = 0
        with pytest.raises(AssertionError, match="1 guard word"):
            g.intact()


def test_bufs_int64_views_sit_in_guards_and_see_half_a_word():
    g = Bufs(64, 128, device="cpu")
    li, lo = g.lin(torch.tensor([[5, 1 << 40, -2]]), 7), g.lout((2, 3))
    assert li.dtype == lo.dtype == torch.int64 and li.shape == (1, 3) and lo.shape == (2, 3)
    assert li.tolist() == [[5, 1 << 40, -2]] and li.data_ptr() % ALIGN == 0 and lo.data_ptr() % ALIGN == 0
    unwritten = (SENTINEL << 32) | SENTINEL
    assert bool((lo == unwritten).all()) and unwritten > (1 << 31)      # an unwritten entry is no index
    (ibase, iv, ipoison), (obase, ov, _) = g.items
    assert ipoison == 7 and int((ibase.view(torch.int32) == 7).sum()) == ibase.numel() - 6
    for base, v in ((ibase, iv), (obase, ov)):
        s = v.storage_offset() - base.storage_offset()
        assert s >= 64 and base.numel() - s - v.numel() >= 128
    g.intact()
    lo.fill_(3)
    g.intact()
    at = ov.storage_offset() - obase.storage_offset() + ov.numel()       # the low half of the int64 behind the last entry
    obase.view(torch.int32)[at] = 3
    with pytest.raises(AssertionError, match="1 guard word"):
        g.intact()
