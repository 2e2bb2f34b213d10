"""Guard bands for kernel tests: every tensor a kernel reads or writes sits inside a larger buffer of its own whose other
words hold a poison value.

- inputs: NaN guards.  A read past the extent the kernel owns returns NaN, and NaN survives `0 * x` (a masked key whose
  weight is zero still poisons an accumulator through `fma(0, x, acc)`), so a stray read shows up as a non-finite result;
- outputs: a recognisable NaN bit pattern (SENTINEL).  `assert_guards_intact` compares every guard word with it bit for
  bit, so a stray write shows up even when it writes a NaN.

Guards are sized by the caller so that the worst over-read of the code under test lands inside the buffer: a stray access
turns into a poisoned result, never into an access outside an allocation.  Views start 256-byte aligned (every tile
alignment the kernels ask for) and are contiguous where the shape allows, so `.contiguous()` in a wrapper passes the
guarded view itself to the kernel."""
import math
import struct

import torch

SENTINEL = 0x7fc0dead       # a quiet NaN whose payload no kernel produces
ALIGN = 256                 # bytes
X_TAIL_MIN = (1 << 20) // 4  # floats: the least guard behind an [N, D] input (x_tail)


def x_tail(D):
    """Guard behind an [.., N, D] input: max(512 rows, 1 MiB)."""
    return max(512 * D, X_TAIL_MIN)


def poison_bits(poison):
    """The int32 bit pattern a guard word holds: an int is a bit pattern, a float its fp32 encoding."""
    if isinstance(poison, int):
        u = poison & 0xffffffff
    else:
        u = struct.unpack("<I", struct.pack("<f", float(poison)))[0]
    return u - (1 << 32) if u >= (1 << 31) else u


def _poisoned(numel, poison, device):
    base = torch.empty(numel, dtype=torch.float32, device=device)
    base.view(torch.int32).fill_(poison_bits(poison))
    return base


def _start(base, lead):
    """First float of a view whose guard in front holds at least `lead` floats, at an ALIGN-byte address."""
    lead_b = -(-lead * 4 // ALIGN) * ALIGN
    at = base.data_ptr() + lead_b
    at = -(-at // ALIGN) * ALIGN
    return (at - base.data_ptr()) // 4


def guarded(shape, lead, tail, poison=float("nan"), device="cuda"):
    """-> (view, base): a contiguous float32 view of `shape` inside `base`, with at least `lead` floats of poison in front
    and `tail` behind.  The view holds poison too until the caller fills it."""
    numel = math.prod(shape)
    base = _poisoned(lead + numel + tail + 2 * ALIGN // 4, poison, device)
    s = _start(base, lead)
    view = base[s:s + numel].view(*shape)
    assert view.is_contiguous() and view.contiguous().data_ptr() == view.data_ptr()
    return view, base


def guarded_like(t, lead, tail, poison=float("nan")):
    """`t` copied into a guarded view (see guarded)."""
    view, base = guarded(tuple(t.shape), lead, tail, poison, t.device)
    view.copy_(t)
    return view, base


def padded_stream(B, N, ld, stride, poison=float("nan"), device="cuda", lead=None, tail=None):
    """-> (stream, base): a [B][N][ld] float32 view with strides (stride, ld, 1) inside `base`, for the [B] x N x N streams
    the kernels address with a leading dimension and a batch stride.  Everything but the N x N elements of each shape --
    the pad columns N .. ld - 1, the gap between shapes, the guards in front and behind (default: one whole shape's slice
    each) -- holds poison; so does the N x N part until the caller fills it (`stream[..., :N]`)."""
    assert ld >= N and stride >= (N - 1) * ld + N
    lead = stride if lead is None else lead
    tail = stride if tail is None else tail
    base = _poisoned(lead + B * stride + tail + 2 * ALIGN // 4, poison, device)
    s = _start(base, lead)
    stream = base.as_strided((B, N, ld), (stride, ld, 1), base.storage_offset() + s)
    return stream, base


def guarded_matrix(P, C, ld, lead, tail, poison=float("nan"), device="cuda"):
    """-> (view, base): a [P, C] float32 view with row stride `ld` >= C inside `base`, for the channels-last matrices the
    kernels address with a leading dimension (any P, unlike padded_stream).  The pad columns C .. ld - 1 of every row (the last
    row's too), the guards of at least `lead` floats in front and `tail` behind, and the view itself until the caller fills
    it, hold poison."""
    assert ld >= C > 0 and P > 0
    base = _poisoned(lead + P * ld + tail + 2 * ALIGN // 4, poison, device)
    s = _start(base, lead)
    view = base.as_strided((P, C), (ld, 1), base.storage_offset() + s)
    return view, base


def _outside(base, view):
    """bool [base.numel()]: True on the words of `base` that `view` does not cover."""
    off = view.storage_offset() - base.storage_offset()
    idx = torch.arange(base.numel(), device=base.device)
    mask = torch.ones(base.numel(), dtype=torch.bool, device=base.device)
    mask[torch.as_strided(idx, view.shape, view.stride(), off).reshape(-1)] = False
    return mask


def assert_guards_intact(base, view, poison=SENTINEL):
    """Every word of `base` outside `view` still holds `poison`, bit for bit."""
    assert view.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
    bits = base.view(torch.int32)
    bad = (bits != poison_bits(poison)) & _outside(base, view)
    n = int(bad.sum())
    if n:
        first = int(bad.nonzero()[0])
        raise AssertionError("%d guard word(s) overwritten; first at float %d of the buffer (view: floats %d ..): 0x%08x"
                             % (n, first, view.storage_offset() - base.storage_offset(), int(bits[first]) & 0xffffffff))


BUFS_LEAD = 4096
BUFS_TAIL = 129 * 1056      # 129 rows of the widest leading dimension the norm / pool / gather cases use (1028 + 28)


class Bufs:
    """Guarded buffers of one case: *in = inputs in NaN guards, *out = outputs in SENTINEL guards; `lead` / `tail` floats of
    guard in front of and behind every one of them."""

    def __init__(self, lead=BUFS_LEAD, tail=BUFS_TAIL, device="cuda"):
        self.items = []
        self.lead, self.tail, self.device = lead, tail, device

    def _guarded(self, shape, poison):
        v, base = guarded(tuple(shape), self.lead, self.tail, poison, self.device)
        self.items.append((base, v, poison))
        return v

    def _mat(self, P, C, ld, poison):
        v, base = guarded_matrix(P, C, ld, self.lead, self.tail, poison, self.device)
        self.items.append((base, v, poison))
        return v

    def fin(self, t, ld=None):
        t = t.detach().to(torch.float32)
        v = self._guarded(t.shape, float("nan")) if ld is None else self._mat(t.shape[0], t.shape[1], ld, float("nan"))
        v.copy_(t)
        return v

    def iin(self, t, poison):
        """int32 input; `poison` is an IN-RANGE value whose use shows in the results (a NaN's bit pattern read as an index is
        out of range everywhere, and the kernels drop such an index silently)"""
        v = self._guarded(t.shape, int(poison))
        v.view(torch.int32).copy_(t.to(torch.int32))
        return v.view(torch.int32)

    def din(self, t):
        v = self._guarded(tuple(t.shape[:-1]) + (2 * t.shape[-1],), float("nan"))
        v.view(torch.float64).copy_(t.to(torch.float64))
        return v.view(torch.float64)

    def fout(self, shape, zero=False, init=None):
        v = self._guarded(shape, SENTINEL)
        if zero:
            v.zero_()
        if init is not None:
            v.copy_(init)
        return v

    def mout(self, P, C, ld, col0=0, wide=None):
        """[P, C] output at column col0 of a [P, wide] matrix with row stride ld: the other columns are guards too"""
        m, base = guarded_matrix(P, wide or C, ld, self.lead, self.tail, SENTINEL, self.device)
        v = m[:, col0:col0 + C]
        self.items.append((base, v, SENTINEL))
        return v

    def iout(self, shape):
        return self.fout(shape).view(torch.int32)

    def dout(self, shape):
        return self.fout(tuple(shape[:-1]) + (2 * shape[-1],)).view(torch.float64)

    def lin(self, t, poison):
        """int64 input; both halves of every guard word pair hold `poison` (see iin), so a kernel that narrows a stray entry
        to 32 bits finds the in-range value `poison`"""
        v = self._guarded(tuple(t.shape[:-1]) + (2 * t.shape[-1],), int(poison))
        v.view(torch.int64).copy_(t.to(torch.int64))
        return v.view(torch.int64)

    def lout(self, shape):
        """int64 output: an entry the kernel did not write reads SENTINEL in both halves, far outside any index range"""
        return self.fout(tuple(shape[:-1]) + (2 * shape[-1],)).view(torch.int64)

    def intact(self):
        if self.device != "cpu":
            torch.cuda.synchronize()
        for base, v, poison in self.items:
            assert_guards_intact(base, v, poison)
