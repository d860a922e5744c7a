"""What the network-input tests (tests/test_net_input.py) share: the numpy model of the padded plane stack, written from the header's
definition (include/tetris_hip.h: tetris_net_input_dev) on top of the uint8 arrays tetris_traj_batch_dev gives, the reference's own
two functions transcribed in torch, guarded output buffers and the call wrapper.  The model owes nothing to
drl-tetris_amd/csrc/tetris_input.h."""
import ctypes as C

import numpy as np

from tests.buffers import GUARD, PAD, Buf, sync

F32, F16, U8, U32, I32 = np.float32, np.float16, np.uint8, np.uint32, np.int32
ITEMS = ("cumsum", "shadow", "height", "holes")
BLOCK = 8                 # INPUT_BLOCK of drl-tetris_amd/csrc/tetris_input.h: samples of one slot per workgroup of k_net_input
# one sample; the block less one, exact and plus one; two blocks plus one; many blocks with a partial last
SIZES = (1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, 257)


# ---------------------------------------------------------------- the model, from the header's text
def model_stack(f, items, pad, valid=None):
    """f: the bytes tetris_traj_batch_dev gives, uint8 [..., H, 10]; items: names in channel order; valid [...] or None
    -> int64 [..., C, Hp, Wp], channels first"""
    f = np.asarray(f).astype(np.int64)
    H = f.shape[-2]
    if pad:
        P = np.ones(f.shape[:-2] + (H + 2, 12), np.int64)       # ones left, right and below; the walls cover the top row too
        P[..., 0, 1:11] = 0                                     # a zero row on top
        P[..., 1:H + 1, 1:11] = f
    else:
        P = f
    cumsum = np.cumsum(P, axis=-2)
    shadow = np.minimum(cumsum, 1)
    height = np.broadcast_to(np.arange(P.shape[-2])[:, None], P.shape)
    by_name = dict(cumsum=cumsum, shadow=shadow, height=height, holes=shadow - P)
    out = np.stack([P] + [by_name[i] for i in items], axis=-3)
    if valid is not None:
        out = out * np.asarray(valid).astype(np.int64)[..., None, None, None]      # no sample: zeros, height and the walls included
    assert out.min() >= 0 and out.max() <= 33
    return out


def model_inputs(batch, items, pad, dtype, channels_last):
    """batch: visual uint8 [S, M, H, 10], vector uint8 [S, M, 12], piece uint8 [S, M], valid uint8 [M] as tetris_traj_batch_dev
    gives them -> the four outputs of tetris_net_input_dev"""
    vis = model_stack(batch["visual"], items, pad, batch["valid"][None, :])
    if channels_last:
        vis = np.moveaxis(vis, -3, -1)
    return dict(visual=np.ascontiguousarray(vis).astype(dtype), vector=batch["vector"].astype(dtype), piece=batch["piece"].astype(U8),
                valid=batch["valid"].astype(U8))


def visual_shape(S, M, H, n_items, pad, channels_last):
    Cn, Hp, Wp = 1 + n_items, H + (2 if pad else 0), 10 + (2 if pad else 0)
    return (S, M, Hp, Wp, Cn) if channels_last else (S, M, Cn, Hp, Wp)


# ---------------------------------------------------------------- the reference's lines (agents/networks/network_utils.py:71-93) in torch
def ref_apply_visual_pad(x):
    """x float32 [N, H, W, 1]"""
    import torch.nn.functional as F
    x = F.pad(x, (0, 0, 0, 0, 1, 0, 0, 0), value=0.0)             # tf.pad(x, [[0,0],[1,0],[0,0],[0,0]], constant_values=0.0)
    x = F.pad(x, (0, 0, 1, 1, 0, 1, 0, 0), value=1.0)             # tf.pad(x, [[0,0],[0,1],[1,1],[0,0]], constant_values=1.0)
    return x


def ref_visual_stack(x, items=None):
    """x float32 [N, H, W, 1] -> [N, H, W, 1 + len(items)]"""
    import torch
    x_cumsum = torch.cumsum(x, dim=1)
    x_shadow = torch.minimum(x_cumsum, torch.tensor(1.0))
    _x_height = torch.arange(x.shape[1], dtype=torch.float32).reshape(1, -1, 1, 1)
    x_height = torch.tile(_x_height, (1, 1, x.shape[2], 1)) + torch.zeros_like(x)
    x_holes = x_shadow - x
    item_dict = {"cumsum": x_cumsum, "shadow": x_shadow, "height": x_height, "holes": x_holes}
    if items is None:
        items = item_dict.keys()
    x_stack = [x] + [item_dict[key] for key in items]
    return torch.cat(x_stack, dim=3)


# ---------------------------------------------------------------- guarded outputs and the call
class Guarded:
    """An output of `shape` / `dtype` with GUARD bytes in front of it, throughout it and behind it; `lead` bytes past a 16-byte
    boundary.  get() asserts both guards are intact."""

    def __init__(self, kind, shape, dtype, lead=0):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape)) * self.dtype.itemsize
        self.front = 32 + lead
        self.buf = Buf(kind, np.full(self.front + self.n + PAD, GUARD, U8))
        self.ptr = self.buf.ptr + self.front

    def raw(self):
        return self.buf.get()

    def get(self):
        raw = self.buf.get()
        assert (raw[:self.front] == GUARD).all(), "wrote in front of the buffer"
        assert (raw[self.front + self.n:] == GUARD).all(), "wrote past the buffer"
        return raw[self.front:self.front + self.n].copy().view(self.dtype).reshape(self.shape)


OUTPUTS = ("visual", "vector", "piece", "valid")


class InputCall:
    """One tetris_net_input_dev call into guarded buffers.  source: dict(obs=traj_obs struct, index=array or None, row=int) or
    dict(replay=replay struct, index=array, steps=int or step_mask=int); n: the number of samples the outputs hold; lead: elements the
    visual and vector outputs start past a 16-byte boundary; only: the outputs that are given (others NULL)."""

    def __init__(self, kind, b, source, n, items=ITEMS, pad=True, dtype=F32, channels_last=False, lead=0, only=OUTPUTS):
        self.kind, self.b = kind, b
        S, H = b.n_players, b.height
        dt = np.dtype(dtype)
        shapes = dict(visual=(visual_shape(S, n, H, len(items), pad, channels_last), dt, lead * dt.itemsize), vector=((S, n, 12), dt, lead * dt.itemsize),
                      piece=((S, n), U8, lead), valid=((n,), U8, lead))
        self.out = {k: Guarded(kind, *shapes[k]) for k in only}
        index = source.get("index")
        self.index = None if index is None else Buf(kind, np.asarray(index).astype(np.int64).astype(U32).view(I32))
        m = source.get("m", n if index is None else len(index))
        self.arg = b.net_input(m, obs=source.get("obs"), replay=source.get("replay"), index=None if self.index is None else self.index.ptr,
                               row=source.get("row", 0), steps=source.get("steps", 1), step_mask=source.get("step_mask", 0), items=items, pad=pad,
                               f16=dt == np.dtype(F16), channels_last=channels_last, **{k: v.ptr for k, v in self.out.items()})

    def run(self):
        self.b.net_input_dev(self.arg)
        sync(self.kind, self.b)
        return self.get()

    def get(self):
        return {k: v.get() for k, v in self.out.items()}

    def untouched(self):
        sync(self.kind, self.b)
        return all((v.raw() == GUARD).all() for v in self.out.values())


def assert_outputs(got, want, where):
    for k, v in got.items():
        w = want[k]
        assert v.shape == w.shape, f"{where}: '{k}' has shape {v.shape}, the model {w.shape}"
        same = v.view(np.uint16 if v.dtype == F16 else U32 if v.dtype == F32 else U8) == w.view(np.uint16 if w.dtype == F16 else U32 if w.dtype == F32 else U8)
        assert same.all(), f"{where}: '{k}' differs at {np.argwhere(~same)[:4].tolist()}"


def raw_call(b, arg):
    """the return code and the message of a call, below the Python layer's exception"""
    rc = b.lib.tetris_net_input_dev(b._h, C.byref(arg) if arg is not None else None)
    return rc, b.lib.tetris_last_error().decode()
