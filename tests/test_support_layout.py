"""Where the tests' scaffolding lives.  What more than one test file needs is in a support module (a module under tests/ whose
name does not start with `test_`): no test file and no profile script imports a test file.  And the one buffer type of the
tests (tests/buffers.py) itself: round trips of every dtype the suite uses, broadcasting and casting puts, the byte offset and
the guard bytes, on the CPU harness's host memory and on the GPU."""
import ast
import ctypes
import glob
import os

import numpy as np
import pytest

from tests import engines
from tests.buffers import GUARD, PAD, Buf, out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.uint8, np.int8, np.int16, np.int32, np.uint32, np.float16, np.float32)


def test_no_test_file_is_imported():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py")) + glob.glob(os.path.join(ROOT, "profiles", "*.py")))
    assert len(files) > 40, f"only {len(files)} files found under {ROOT}"
    bad = []
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):                               # function bodies included
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""] + [f"{node.module or ''}.{a.name}" for a in node.names]
            else:
                continue
            bad += [f"{os.path.relpath(path, ROOT)}:{node.lineno}: imports {n}" for n in names if n.split(".")[-1].startswith("test_")]
    assert not bad, "a test file is imported; what is shared belongs in a support module:\n" + "\n".join(bad)


def random_bits(dtype, seed):
    """(3, 5) distinct random bit patterns of `dtype`"""
    size = 15 * np.dtype(dtype).itemsize
    raw = np.random.default_rng(seed).permutation(256)[:size].astype(np.uint8)
    return raw.view(dtype).reshape(3, 5)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
@pytest.mark.parametrize("offset", [0, 4])
def test_round_trip(kind, dtype, offset):
    values = random_bits(dtype, 7 + offset)
    b = Buf(kind, values, offset=offset)
    assert isinstance(b.ptr, int) and b.ptr % 16 == offset
    assert b.shape == (3, 5) and b.dtype == np.dtype(dtype) and b.nbytes == values.nbytes
    got = b.get()
    assert got.dtype == np.dtype(dtype) and got.shape == (3, 5)
    assert got.tobytes() == values.tobytes()
    got[...] = 0
    assert b.get().tobytes() == values.tobytes(), "get() returns a copy"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
def test_full_and_put_broadcast_and_cast(kind, dtype):
    b = Buf.full(kind, (3, 5), dtype, 7)
    assert b.shape == (3, 5) and b.dtype == np.dtype(dtype)
    assert np.array_equal(b.get(), np.full((3, 5), 7, dtype))
    assert b.put(np.int64(-3) if np.dtype(dtype).kind != "u" else np.int64(200)) is b
    want = np.full((3, 5), -3 if np.dtype(dtype).kind != "u" else 200, dtype)
    assert b.get().tobytes() == want.tobytes(), "a scalar of another type broadcasts and is cast"
    row = np.arange(5, dtype=np.float64) + 1.0
    b.put(row)
    want = np.broadcast_to(row, (3, 5)).astype(dtype)
    assert b.get().tobytes() == want.tobytes(), "a (5,) row of another type broadcasts over (3, 5) and is cast"


def test_guard_bytes_on_the_harness():
    values = random_bits(np.float32, 3)
    b = Buf("harness", values, guard=PAD)
    b.put(values[::-1])
    assert b.get().tobytes() == values[::-1].tobytes(), "the guard is intact after put and get"
    guard = (ctypes.c_uint8 * PAD).from_address(b.ptr + b.nbytes)
    assert bytes(guard) == bytes([GUARD]) * PAD
    ctypes.memset(b.ptr + b.nbytes, 0, 1)                         # the first byte behind the data: inside the buffer's own allocation
    with pytest.raises(AssertionError, match="wrote past the buffer"):
        b.get()
    ctypes.memset(b.ptr + b.nbytes, GUARD, 1)
    ctypes.memset(b.ptr + b.nbytes + PAD - 1, 0, 1)               # and the last
    with pytest.raises(AssertionError, match="wrote past the buffer"):
        b.get()


@pytest.mark.gpu
def test_guard_bytes_on_the_gpu():
    """(overwriting the guard would take a write from the device side: only the round trip and the guard's bytes)"""
    values = random_bits(np.float16, 5)
    b = Buf("hip", values, offset=4, guard=PAD)
    assert b.get().tobytes() == values.tobytes()
    behind = b.raw[b.at + b.nbytes:b.at + b.nbytes + PAD].cpu().numpy()
    assert behind.size == PAD and (behind == GUARD).all()
    o = out("hip", (3, 5), np.int32)
    assert (o.get().view(np.uint8) == GUARD).all() and o.guard == PAD and o.ptr % 16 == 0
