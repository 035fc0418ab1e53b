"""Guarded, patterned device buffers for tests/test_gpu_memory_contract.py.

One uint8 allocation of ``guard + align256(nbytes) + guard`` bytes: a leading guard, the body (256-
byte aligned, exactly ``nbytes`` long) and a trailing guard that starts at the body's last byte + 1,
so the alignment tail up to the next 256 bytes belongs to it.  The guards hold one byte value
(0xA5 for the write checks); the body holds ``fill``:

  0x00  what a fresh allocation usually shows
  0xFF  NaN as f16, f32 and f64, -1 as an integer
  0x7B  large but finite in all three float types (f16 6.1e4, f32 1.3e36, f64 2.7e286)

Everything a kernel may legally touch lies inside the body, and everything it could touch by an
off-by-a-row or off-by-a-plane error lies inside the same allocation, so nothing here can fault.
"""
import numpy as np

GUARD = 1 << 20
GUARD_BYTE = 0xA5
FILLS = (0x00, 0xFF, 0x7B)


def align256(n):
    return (n + 255) & ~255


class Guarded:
    def __init__(self, nbytes, fill, guard=GUARD, guard_byte=GUARD_BYTE):
        import torch
        assert nbytes >= 0 and guard > 0 and guard % 256 == 0
        self.nbytes, self.guard, self.guard_byte = int(nbytes), guard, guard_byte
        self.buf = torch.empty(guard + align256(self.nbytes) + guard, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.buf.fill_(guard_byte)
        self.body = self.buf[guard:guard + self.nbytes]
        self.body.fill_(fill)
        assert self.body.data_ptr() % 256 == 0 and self.body.numel() == self.nbytes

    def refill(self, fill):
        """stream-ordered, on the current stream"""
        self.body.fill_(fill)

    def view(self, dtype, shape):
        """the body as a typed tensor (it must hold exactly that many bytes)"""
        t = self.body.view(dtype).view(shape)
        assert t.numel() * t.element_size() == self.nbytes
        return t

    def check(self, what="buffer"):
        """both guards still hold the guard byte everywhere"""
        lead, trail = self.buf[:self.guard], self.buf[self.guard + self.nbytes:]
        for name, g in (("before", lead), ("after", trail)):
            bad = g != self.guard_byte
            if bool(bad.any()):
                idx = bad.nonzero().flatten()
                first, last = int(idx[0]), int(idx[-1])
                if name == "before":
                    first, last = first - self.guard, last - self.guard        # relative to the body's start
                raise AssertionError(f"{what}: {int(idx.numel())} guard bytes {name} the body changed, offsets "
                                     f"{first}..{last} from the body's {'start' if name == 'before' else 'end'}")


def guarded(nbytes, fill, guard=GUARD):
    """(body, check): the issue's plain form of ``Guarded``"""
    g = Guarded(nbytes, fill, guard)
    return g.body, g.check


def guarded_out(shape, fill=0xFF, dtype=None):
    """(tensor, Guarded): a float32 (or ``dtype``) output tensor as the body of a guarded buffer"""
    import torch
    dtype = dtype or torch.float32
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    g = Guarded(n, fill)
    return g.view(dtype, tuple(shape)), g


def guarded_input(tensor, guard_byte):
    """(copy of ``tensor`` as the body of a guarded buffer whose guards hold ``guard_byte``, Guarded)"""
    t = tensor.contiguous()
    g = Guarded(t.numel() * t.element_size(), 0x00, guard_byte=guard_byte)
    v = g.view(t.dtype, tuple(t.shape))
    v.copy_(t)
    return v, g


def same_bits(a, b):
    """bit-identical arrays (NaN payloads included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
