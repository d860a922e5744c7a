"""The one buffer type of the tests and the constants that go with it.

A `Buf` is a buffer the `_dev` entry points read or write: a numpy uint8 array on the CPU harness (its "device" is host memory), a
torch.uint8 device tensor on the GPU.  Every dtype travels as its bits, so float16, uint32 and int16 need no torch dtype.  On the GPU
the batch runs on a stream of its own and torch copies on its default stream: every upload is followed by, every read preceded by,
torch.cuda.synchronize()."""
import numpy as np

U8 = np.uint8
MIRROR = 1 << 31          # bit 31 of a trajectory entry: the mirrored sample (the tests' own statement of the header's bit)
PAD = 64                  # guard bytes behind every guarded output buffer
GUARD = 0xCD


class Buf:
    """Buf(kind, values, offset=0, guard=0): 16-byte aligned plus `offset` bytes, `guard` bytes of GUARD behind the data;
    .ptr (int), .shape, .dtype, .nbytes, .put(values) -> self, .get() -> a numpy copy (asserts the guard bytes are intact)."""

    def __init__(self, kind, values, offset=0, guard=0):
        values = np.ascontiguousarray(values)
        self.kind, self.dtype, self.shape, self.nbytes, self.guard = kind, values.dtype, values.shape, values.nbytes, guard
        if kind == "hip":
            import torch
            self.raw = torch.zeros(offset + self.nbytes + guard + 16, dtype=torch.uint8, device="cuda")
            base, self.at = self.raw.data_ptr(), offset
        else:
            self.raw = np.zeros(offset + self.nbytes + guard + 32, U8)
            self.at = (-self.raw.ctypes.data) % 16 + offset
            base = self.raw.ctypes.data + self.at - offset
        assert base % 16 == 0, f"the buffer's base {base:#x} is not 16-byte aligned"
        self.ptr = base + offset
        if guard:
            self._upload(self.nbytes, np.full(guard, GUARD, U8))
        self.put(values)

    @classmethod
    def full(cls, kind, shape, dtype, fill=0, offset=0, guard=0):
        return cls(kind, np.full(shape, fill, dtype), offset, guard)

    def _upload(self, start, flat):
        lo = self.at + start
        if self.kind == "hip":
            import torch
            self.raw[lo:lo + flat.size] = torch.from_numpy(flat.copy()).cuda()
            torch.cuda.synchronize()
        else:
            self.raw[lo:lo + flat.size] = flat

    def put(self, values):
        """broadcast to the buffer's shape, cast to its dtype"""
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(values), self.shape)).astype(self.dtype, copy=False)
        self._upload(0, v.view(U8).reshape(-1))
        return self

    def get(self):
        lo, size = self.at, self.nbytes + self.guard
        if self.kind == "hip":
            import torch
            torch.cuda.synchronize()
            flat = self.raw[lo:lo + size].cpu().numpy()
        else:
            flat = self.raw[lo:lo + size].copy()
        assert (flat[self.nbytes:] == GUARD).all(), "wrote past the buffer"
        return flat[:self.nbytes].copy().view(self.dtype).reshape(self.shape)


def out(kind, shape, dtype):
    """an output buffer: GUARD bytes throughout, so what a call did not write shows, and PAD guard bytes behind it"""
    dt = np.dtype(dtype)
    return Buf(kind, np.full(int(np.prod(shape)) * dt.itemsize, GUARD, U8).view(dt).reshape(shape), guard=PAD)


def bits(a):
    """float32 -> its uint32 bits"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sync(kind, b):
    if kind == "hip":
        b.sync()
