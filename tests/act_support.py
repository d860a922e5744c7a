"""Acting on a network's (r, t, piece) evaluation: the numpy model written from the header's definitions (tests/test_act_eval.py
describes it), mid-game boards, and the buffers of one selection with the argument struct over them."""
import numpy as np

from oracle import oracle as orc
from tests import engines
from tests.buffers import Buf, bits

F32 = np.float32
TWO_M24 = F32(2.0 ** -24)


# ---------------------------------------------------------------- the model
def words(seed, ids, draw):
    """Philox4x32-10, key (seed, 0), counter (global game id, draw low, draw high, 0) -> uint32 [n, 4]"""
    return np.stack([orc.philox(int(seed), 0, int(g) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFF, int(draw) >> 32, 0) for g in ids])


def unit(w):
    return F32(int(w) >> 8) * TWO_M24


def m_argmax(x):
    ok = np.nonzero(~np.isnan(x))[0]
    return int(ok[np.argmax(x[ok])]) if len(ok) else 0            # numpy's first maximum is the lowest candidate


def m_ranks(x):
    order = np.argsort(-x, kind="stable")                          # higher first, among equals the lower index
    return np.argsort(order, kind="stable") + 1


def m_draw(m, u):
    """the inverse-CDF draw; None: the total is not a positive finite number"""
    total, partial = F32(0.0), []
    for c in range(40):
        total = F32(total + m[c])
        partial.append(total)
    if not (total > 0 and np.isfinite(total)):
        return None
    target = F32(u * total)
    for c in range(40):
        if partial[c] > target:
            return c
    return int(np.nonzero(m > 0)[0][-1])


def model(action_eval, piece_idx, ids, mode, seed=0, draw=0, epsilon=0.0, table=None, state_eval=None):
    """action_eval [n, 4, 10, K] (float32 or float16), piece_idx [n] = the acting players' piece indices (observe()'s `piece`),
    ids = global game ids -> dict of rot, trans, piece, eval, value [2, n], entropy (float64), random [n] (EPSILON: drew)"""
    n, K = action_eval.shape[0], action_eval.shape[3]
    piece = np.minimum(piece_idx, K - 1).astype(np.uint8)
    x_all = action_eval.reshape(n, 40, K)[np.arange(n), :, piece].astype(F32)
    w = words(seed, ids, draw) if mode != "argmax" else np.zeros((n, 4), np.uint32)
    c_out, rnd = np.zeros(n, np.int64), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            x = x_all[i]
            c = None
            if mode == "epsilon":
                if unit(w[i, 1]) < F32(epsilon):
                    c, rnd[i] = 10 * (int(w[i, 2]) & 3) + int(w[i, 3]) % 10, True
            elif mode == "pi":
                c = m_draw(np.where(x > 0, x, F32(0.0)).astype(F32), unit(w[i, 0]))
            elif mode == "rank":
                c = m_draw(np.asarray(table, F32)[m_ranks(x) - 1], unit(w[i, 0]))
            c_out[i] = m_argmax(x) if c is None else c
        out = dict(c=c_out, rot=(c_out // 10).astype(np.uint8), trans=(c_out % 10).astype(np.uint8), piece=piece,
                   eval=x_all[np.arange(n), c_out], random=rnd)
        q = x_all.astype(np.float64) + 1e-6
        out["entropy"] = -(q * np.log(q + 1e-8)).sum(axis=1)
        if state_eval is not None:
            V = state_eval.shape[1]
            se = state_eval.astype(F32)
            mean = np.zeros(n, F32)
            for k in range(V):
                mean = (mean + se[:, k]).astype(F32)
            out["value"] = np.stack([se[np.arange(n), np.minimum(piece, V - 1)] if V > 1 else se[:, 0], (mean / F32(V)).astype(F32)])
    return out


# ---------------------------------------------------------------- boards and calls
def midgame(kind, n, P, height=20, steps=30, seed=1, colours=False, extra=0):
    """`1 + extra` batches of the engine under test and an oracle holding the same games after `steps` random step_rt steps"""
    seeds = orc.episode_seed(np.arange(n), 0)
    bs = [engines.make(kind, n, P, height=height, seeds=seeds, colours=colours) for _ in range(1 + extra)]
    o = engines.make("oracle", n, P, height=height, seeds=seeds)
    rng = np.random.default_rng(seed)
    for s in range(steps):
        player = rng.integers(0, P, n).astype(np.uint8)
        r, t = rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 10, n).astype(np.uint8)
        done = o.step_rt(r, t, player)
        for b in bs:
            assert np.array_equal(b.step_rt(r, t, player), done), f"midgame step {s}: the engine's done flags differ from the oracle's"
        d = np.nonzero(done)[0].astype(np.int32)
        if len(d):
            sd = orc.episode_seed(d, s + 1)
            for e in [o] + bs:
                e.reset(d, seeds=sd)
    return bs + [o]


def pieces_of(o, player):
    return o.observe()[0]["piece"][np.arange(o.n_games), player]


class Call:
    """The buffers of one selection and the argument struct over them"""

    def __init__(self, kind, b, action_eval, mode, player=None, state_eval=None, seed=0, draw=0, epsilon=0.0, table=None, entropy=None, flags=0):
        n = b.n_games
        self.kind = kind
        self.ae = Buf(kind, action_eval)
        self.se = None if state_eval is None else Buf(kind, state_eval)
        self.pl = None if player is None else Buf(kind, np.asarray(player, np.uint8))
        self.out = dict(rot=Buf(kind, np.full(n, 9, np.uint8)), trans=Buf(kind, np.full(n, 99, np.uint8)), piece=Buf(kind, np.full(n, 9, np.uint8)),
                        eval=Buf(kind, np.full(n, -7.0, F32)))
        if state_eval is not None:
            self.out["value"] = Buf(kind, np.full((2, n), -7.0, F32))
        if mode == "pi" if entropy is None else entropy:
            self.out["entropy"] = Buf(kind, np.full(n, -7.0, F32))
        p = lambda name: self.out[name].ptr if name in self.out else None            # noqa: E731
        self.e = b.act_eval(self.ae.ptr, p("rot"), p("trans"), n_pieces=action_eval.shape[3], f16=action_eval.dtype == np.float16,
                            state_eval=None if self.se is None else self.se.ptr, n_values=1 if state_eval is None else state_eval.shape[1],
                            value_f16=state_eval is not None and state_eval.dtype == np.float16, mode=mode,
                            player=None if self.pl is None else self.pl.ptr, seed=seed, draw=draw, epsilon=epsilon, table=table,
                            piece=p("piece"), eval=p("eval"), value=p("value"), entropy=p("entropy"), flags=flags)

    def get(self):
        return {k: v.get() for k, v in self.out.items()}


def assert_outputs(got, want, where):
    for name in ("rot", "trans", "piece"):
        assert np.array_equal(got[name], want[name]), f"{where}: '{name}' differs in games {np.nonzero(got[name] != want[name])[0][:8]}"
    assert np.array_equal(bits(got["eval"]), bits(want["eval"])), f"{where}: 'eval' differs"
    if "value" in got:
        assert np.array_equal(bits(got["value"]), bits(want["value"])), f"{where}: 'value' differs"


def random_maps(rng, n, K, dtype, kind):
    if kind == "normal":
        a = rng.standard_normal((n, 4, 10, K))
    elif kind == "levels":                            # a few levels: ties are the normal case
        a = rng.integers(0, 4, (n, 4, 10, K)) / 4.0
    else:                                             # "pi": zeros and negative entries among the probabilities
        a = rng.random((n, 4, 10, K))
        sel = rng.random((n, 4, 10, K))
        a = np.where(sel < 0.3, 0.0, np.where(sel < 0.5, -a, a))
    return a.astype(dtype)
