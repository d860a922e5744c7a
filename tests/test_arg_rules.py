"""The argument rules of the entry points that no other test refuses a call of: create / create_ex / create_split, reset, step_keys,
make_actions / finish_actions, get_actions, the three planning calls, plan_deltas, rollout_launch and debug_table_limit.  One row
per bad call: (name, call, a substring of tetris_last_error()); every row returns TETRIS_E_ARG, and the text is the one
drl-tetris_amd/csrc (tetris_host.h, shared by the product and the CPU harness) gives.  Nearly every row is refused before anything
is launched; the batches are 3 games of height 8 with one and with two players, and one split pair."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import engines
from tests.buffers import Buf

E_ARG = -1
N, H = 3, 8


class Ctx:
    def __init__(self, kind):
        pkg = ge.package()
        self.kind = kind
        path = ge.build_harness() if kind == "harness" else None
        self.b1 = engines.make(kind, N, 1, height=H)
        self.b2 = engines.make(kind, N, 2, height=H)
        self.s0 = pkg.TetrisBatch(N, 2, H, 10, lib_path=path, split_side=0)
        self.s1 = pkg.TetrisBatch(N, 2, H, 10, lib_path=path, split_side=1)
        self.lib = self.b1.lib
        self.map = np.arange(7, dtype=np.uint8)
        self.bad_map = np.array([0, 1, 2, 7, 4, 5, 6], np.uint8)
        # what the _dev calls take for "device" memory: 1 MiB, 16-byte aligned
        self.dev = Buf.full(kind, (1 << 20,), np.uint8)
        # host arrays of the synchronous calls
        self.keys = np.zeros((N, 2, 4), np.uint8)
        self.lens = np.zeros((N, 2), np.uint8)
        self.long_lens = np.full((N, 2), 5, np.uint8)
        self.out = np.zeros((N, 2), np.uint8)
        self.idx_high = np.array([0, N], np.int32)
        self.idx_neg = np.array([-1], np.int32)
        self.player2 = np.array([0, 2, 1], np.uint8)
        self.ga_keys = np.zeros((N, 64, 48), np.uint8)
        self.ga_lens = np.zeros((N, 64), np.uint8)
        self.ga_count = np.full(N, -7, np.int32)

    def close(self):
        for b in (self.b1, self.b2, self.s0, self.s1):
            b.close()
        self.dev = None

    def create(self, fn, *args):
        """a create call; a batch it made against expectation is destroyed again"""
        h = C.c_void_p()
        rc = getattr(self.lib, fn)(C.byref(h), *args)
        if h.value:
            self.lib.tetris_destroy(h)
        return rc


@pytest.fixture(scope="module")
def contexts():
    """one Ctx per engine for the whole table; its batches are closed when the module is done"""
    made = {}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture
def ctx(kind, contexts):
    if kind not in contexts:
        contexts[kind] = Ctx(kind)
    return contexts[kind]


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def d(c, offset=0):
    return C.c_void_p(c.dev.ptr + offset)


SPLIT = " is not available on split batches"

ROWS = [
    # ---- create
    ("create out NULL", lambda c: c.lib.tetris_create(None, N, 1, H, 10, p(c.map), 0, None), "out is NULL"),
    ("create n_games 0", lambda c: c.create("tetris_create", 0, 1, H, 10, p(c.map), 0, None), "n_games must be >= 1"),
    ("create n_players 0", lambda c: c.create("tetris_create", N, 0, H, 10, p(c.map), 0, None), "n_players must be 1..4"),
    ("create n_players 5", lambda c: c.create("tetris_create", N, 5, H, 10, p(c.map), 0, None), "n_players must be 1..4"),
    ("create too many boards", lambda c: c.create("tetris_create", (1 << 21) + 1, 4, H, 10, p(c.map), 0, None), "n_games * n_players must be <= 2^23"),
    ("create height 3", lambda c: c.create("tetris_create", N, 1, 3, 10, p(c.map), 0, None), "height must be in [4, 31]"),
    ("create height 32", lambda c: c.create("tetris_create", N, 1, 32, 10, p(c.map), 0, None), "height must be in [4, 31]"),
    ("create width 9", lambda c: c.create("tetris_create", N, 1, H, 9, p(c.map), 0, None), "width must be 10 (the reference hard-codes 10"),
    ("create piece_map NULL", lambda c: c.create("tetris_create", N, 1, H, 10, None, 0, None), "piece_map is NULL"),
    ("create piece_map 7", lambda c: c.create("tetris_create", N, 1, H, 10, p(c.bad_map), 0, None), "piece_map entries must be 0..6"),
    ("create_ex flag 2", lambda c: c.create("tetris_create_ex", N, 1, H, 10, p(c.map), 0, None, 2), "unknown flag"),
    ("create_ex height 3", lambda c: c.create("tetris_create_ex", N, 1, 3, 10, p(c.map), 0, None, 1), "height must be in [4, 31]"),
    ("create_split side 2", lambda c: c.create("tetris_create_split", N, 2, H, 10, p(c.map), 0, None), "side must be 0 or 1"),
    ("create_split side -1", lambda c: c.create("tetris_create_split", N, -1, H, 10, p(c.map), 0, None), "side must be 0 or 1"),
    ("create_split n_games 0", lambda c: c.create("tetris_create_split", 0, 1, H, 10, p(c.map), 0, None), "n_games must be >= 1"),
    # ---- reset
    ("reset n -1", lambda c: c.lib.tetris_reset(c.b1._h, None, -1, None), "n out of range"),
    ("reset n > N", lambda c: c.lib.tetris_reset(c.b2._h, None, N + 1, None), "n out of range"),
    ("reset idx N", lambda c: c.lib.tetris_reset(c.b2._h, p(c.idx_high), 2, None), "game index out of range"),
    ("reset idx -1", lambda c: c.lib.tetris_reset(c.s0._h, p(c.idx_neg), 1, None), "game index out of range"),
    # ---- step_keys
    ("step_keys n -1", lambda c: c.lib.tetris_step_keys(c.b2._h, None, -1, p(c.keys), p(c.lens), 4, 400, None, None, None), "n out of range"),
    ("step_keys idx N", lambda c: c.lib.tetris_step_keys(c.b2._h, p(c.idx_high), 2, p(c.keys), p(c.lens), 4, 400, None, None, None), "game index out of range"),
    ("step_keys keys NULL", lambda c: c.lib.tetris_step_keys(c.b2._h, None, N, None, p(c.lens), 4, 400, None, None, None), "keys/lens/max_keys"),
    ("step_keys lens NULL", lambda c: c.lib.tetris_step_keys(c.b2._h, None, N, p(c.keys), None, 4, 400, None, None, None), "keys/lens/max_keys"),
    ("step_keys max_keys 0", lambda c: c.lib.tetris_step_keys(c.b2._h, None, N, p(c.keys), p(c.lens), 0, 400, None, None, None), "keys/lens/max_keys"),
    ("step_keys lens > max_keys", lambda c: c.lib.tetris_step_keys(c.b2._h, None, N, p(c.keys), p(c.long_lens), 4, 400, None, None, None), "lens[i][p] > max_keys"),
    ("step_keys lens > max_keys P1", lambda c: c.lib.tetris_step_keys(c.b1._h, None, N, p(c.keys), p(c.long_lens), 4, 400, None, None, None), "lens[i][p] > max_keys"),
    # ---- make_actions / finish_actions
    ("make_actions n > N", lambda c: c.lib.tetris_make_actions(c.b2._h, None, N + 1, p(c.keys), p(c.lens), 4), "n out of range"),
    ("make_actions idx -1", lambda c: c.lib.tetris_make_actions(c.b2._h, p(c.idx_neg), 1, p(c.keys), p(c.lens), 4), "game index out of range"),
    ("make_actions keys NULL", lambda c: c.lib.tetris_make_actions(c.b2._h, None, N, None, p(c.lens), 4), "keys/lens/max_keys"),
    ("make_actions max_keys -1", lambda c: c.lib.tetris_make_actions(c.b1._h, None, N, p(c.keys), p(c.lens), -1), "keys/lens/max_keys"),
    ("make_actions lens > max_keys", lambda c: c.lib.tetris_make_actions(c.b2._h, None, N, p(c.keys), p(c.long_lens), 4), "lens[i][p] > max_keys"),
    ("finish_actions n -1", lambda c: c.lib.tetris_finish_actions(c.b2._h, None, -1, 400, None, None, None), "n out of range"),
    ("finish_actions idx N", lambda c: c.lib.tetris_finish_actions(c.b1._h, p(c.idx_high), 2, 400, None, None, None), "game index out of range"),
    # ---- get_actions
    ("get_actions keys NULL", lambda c: c.lib.tetris_get_actions(c.b2._h, None, N, None, None, p(c.ga_lens), p(c.ga_count), 64, 48), "keys/lens/count/max_*"),
    ("get_actions lens NULL", lambda c: c.lib.tetris_get_actions(c.b2._h, None, N, None, p(c.ga_keys), None, p(c.ga_count), 64, 48), "keys/lens/count/max_*"),
    ("get_actions count NULL", lambda c: c.lib.tetris_get_actions(c.b2._h, None, N, None, p(c.ga_keys), p(c.ga_lens), None, 64, 48), "keys/lens/count/max_*"),
    ("get_actions max_lists 0", lambda c: c.lib.tetris_get_actions(c.b2._h, None, N, None, p(c.ga_keys), p(c.ga_lens), p(c.ga_count), 0, 48), "keys/lens/count/max_*"),
    ("get_actions max_keys 0", lambda c: c.lib.tetris_get_actions(c.b2._h, None, N, None, p(c.ga_keys), p(c.ga_lens), p(c.ga_count), 64, 0), "keys/lens/count/max_*"),
    ("get_actions max_keys 256", lambda c: c.lib.tetris_get_actions(c.b2._h, None, 1, None, p(c.ga_keys), p(c.ga_lens), p(c.ga_count), 8, 256), "keys/lens/count/max_*"),
    ("get_actions n -1", lambda c: c.lib.tetris_get_actions(c.b2._h, None, -1, None, p(c.ga_keys), p(c.ga_lens), p(c.ga_count), 64, 48), "n out of range"),
    ("get_actions n > N", lambda c: c.lib.tetris_get_actions(c.b1._h, None, N + 1, None, p(c.ga_keys), p(c.ga_lens), p(c.ga_count), 64, 48), "n out of range"),
    ("get_actions idx N", lambda c: c.lib.tetris_get_actions(c.b2._h, p(c.idx_high), 2, None, p(c.ga_keys), p(c.ga_lens), p(c.ga_count), 64, 48), "game index out of range"),
    ("get_actions player 2", lambda c: c.lib.tetris_get_actions(c.b2._h, None, N, p(c.player2), p(c.ga_keys), p(c.ga_lens), p(c.ga_count), 64, 48), "player index out of range"),
    # ---- planning
    ("action_lists split", lambda c: c.lib.tetris_action_lists_dev(c.s0._h, None, 64, 48, 0, d(c), d(c), d(c)), "tetris_action_lists_dev" + SPLIT),
    ("action_lists count NULL", lambda c: c.lib.tetris_action_lists_dev(c.b2._h, None, 64, 48, 0, None, d(c), d(c)), "count/lens/keys are NULL"),
    ("action_lists keys NULL", lambda c: c.lib.tetris_action_lists_dev(c.b1._h, None, 64, 48, 0, d(c), d(c), None), "count/lens/keys are NULL"),
    ("action_lists max_lists 0", lambda c: c.lib.tetris_action_lists_dev(c.b2._h, None, 0, 48, 0, d(c), d(c), d(c)), "max_lists >= 1, 1 <= max_keys <= 254"),
    ("action_lists max_keys 255", lambda c: c.lib.tetris_action_lists_dev(c.b2._h, None, 64, 255, 0, d(c), d(c), d(c)), "max_lists >= 1, 1 <= max_keys <= 254"),
    ("action_lists flag 2", lambda c: c.lib.tetris_action_lists_dev(c.b2._h, None, 64, 48, 2, d(c), d(c), d(c)), "unknown flag"),
    ("simulate_lists split", lambda c: c.lib.tetris_simulate_lists_dev(c.s1._h, None, d(c), d(c), d(c), 64, 48, 400, 0, d(c), None, None, None), "tetris_simulate_lists_dev" + SPLIT),
    ("simulate_lists cols NULL", lambda c: c.lib.tetris_simulate_lists_dev(c.b2._h, None, d(c), d(c), d(c), 64, 48, 400, 0, None, None, None, None), "count/lens/keys/cols are NULL"),
    ("simulate_lists count NULL", lambda c: c.lib.tetris_simulate_lists_dev(c.b2._h, None, None, d(c), d(c), 64, 48, 400, 0, d(c), None, None, None), "count/lens/keys/cols are NULL"),
    ("simulate_lists max_lists 65536", lambda c: c.lib.tetris_simulate_lists_dev(c.b2._h, None, d(c), d(c), d(c), 65536, 48, 400, 0, d(c), None, None, None), "1 <= max_lists <= 65535, 1 <= max_keys <= 255"),
    ("simulate_lists max_keys 0", lambda c: c.lib.tetris_simulate_lists_dev(c.b1._h, None, d(c), d(c), d(c), 64, 0, 400, 0, d(c), None, None, None), "1 <= max_lists <= 65535, 1 <= max_keys <= 255"),
    ("simulate_lists flag 2", lambda c: c.lib.tetris_simulate_lists_dev(c.b2._h, None, d(c), d(c), d(c), 64, 48, 400, 2, d(c), None, None, None), "unknown flag"),
    ("step_lists split", lambda c: c.lib.tetris_step_lists_dev(c.s0._h, None, d(c), d(c), d(c), d(c), 64, 48, 400, 0, None, None, None), "tetris_step_lists_dev" + SPLIT),
    ("step_lists choice NULL", lambda c: c.lib.tetris_step_lists_dev(c.b2._h, None, None, d(c), d(c), d(c), 64, 48, 400, 0, None, None, None), "choice/count/lens/keys are NULL"),
    ("step_lists lens NULL", lambda c: c.lib.tetris_step_lists_dev(c.b2._h, None, d(c), d(c), None, d(c), 64, 48, 400, 0, None, None, None), "choice/count/lens/keys are NULL"),
    ("step_lists max_keys 256", lambda c: c.lib.tetris_step_lists_dev(c.b2._h, None, d(c), d(c), d(c), d(c), 64, 256, 400, 0, None, None, None), "max_lists >= 1, 1 <= max_keys <= 255"),
    ("step_lists max_lists 0", lambda c: c.lib.tetris_step_lists_dev(c.b1._h, None, d(c), d(c), d(c), d(c), 0, 48, 400, 0, None, None, None), "max_lists >= 1, 1 <= max_keys <= 255"),
    ("step_lists flag 2", lambda c: c.lib.tetris_step_lists_dev(c.b2._h, None, d(c), d(c), d(c), d(c), 64, 48, 400, 2, None, None, None), "unknown flag"),
    ("plan_deltas split", lambda c: c.lib.tetris_plan_deltas_dev(c.s0._h, None, d(c), d(c), 64, 1e-3, 0, d(c), None, None), "tetris_plan_deltas_dev" + SPLIT),
    ("plan_deltas deltas NULL", lambda c: c.lib.tetris_plan_deltas_dev(c.b2._h, None, d(c), d(c), 64, 1e-3, 0, None, None, None), "count/cols/deltas are NULL"),
    ("plan_deltas count NULL", lambda c: c.lib.tetris_plan_deltas_dev(c.b2._h, None, None, d(c), 64, 1e-3, 0, d(c), None, None), "count/cols/deltas are NULL"),
    ("plan_deltas max_lists 0", lambda c: c.lib.tetris_plan_deltas_dev(c.b2._h, None, d(c), d(c), 0, 1e-3, 0, d(c), None, None), "1 <= max_lists <= 256"),
    ("plan_deltas max_lists 257", lambda c: c.lib.tetris_plan_deltas_dev(c.b1._h, None, d(c), d(c), 257, 1e-3, 0, d(c), None, None), "1 <= max_lists <= 256"),
    ("plan_deltas flag 4", lambda c: c.lib.tetris_plan_deltas_dev(c.b2._h, None, d(c), d(c), 64, 1e-3, 4, d(c), None, None), "unknown flag"),
    ("plan_deltas deltas + 4", lambda c: c.lib.tetris_plan_deltas_dev(c.b2._h, None, d(c), d(c), 64, 1e-3, 0, d(c, 4), None, None), "deltas / sums must be 16-byte aligned"),
    ("plan_deltas sums + 8", lambda c: c.lib.tetris_plan_deltas_dev(c.b2._h, None, d(c), d(c), 64, 1e-3, 0, d(c), d(c, 8), None), "deltas / sums must be 16-byte aligned"),
    ("plan_deltas cols + 2", lambda c: c.lib.tetris_plan_deltas_dev(c.b2._h, None, d(c), d(c, 2), 64, 1e-3, 0, d(c), None, None), "cols must be 4-byte aligned"),
    # ---- rollout_launch, debug_table_limit
    ("rollout_launch launches 0", lambda c: c.lib.tetris_rollout_launch(c.b1._h, 0, 1, 1, 0, 400, None), "launches must be >= 1, steps_per_launch >= 0"),
    ("rollout_launch steps -1", lambda c: c.lib.tetris_rollout_launch(c.b2._h, 1, -1, 1, 0, 400, None), "launches must be >= 1, steps_per_launch >= 0"),
    ("rollout_launch steps 257", lambda c: c.lib.tetris_rollout_launch(c.b2._h, 1, 257, 1, 0, 400, None), "steps_per_launch must be <= 256"),
    ("table_limit -1", lambda c: c.lib.tetris_debug_table_limit(c.b1._h, -1), "chunks must be 0..64"),
    ("table_limit 65", lambda c: c.lib.tetris_debug_table_limit(c.b2._h, 65), "chunks must be 0..64"),
]


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("row", ROWS, ids=[r[0].replace(" ", "_") for r in ROWS])
def test_bad_call_is_refused(kind, row, ctx):
    name, call, text = row
    rc = call(ctx)
    msg = ctx.lib.tetris_last_error().decode()
    print(f"{kind}: {name}: rc {rc}, '{msg}'")
    assert rc == E_ARG, f"{name}: rc {rc} ('{msg}')"
    assert text in msg, f"{name}: '{msg}' lacks '{text}'"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
def test_get_actions_counts_before_it_refuses(kind, P, ctx):
    """More lists than max_lists: TETRIS_E_ARG, and count[i] of the game that overflowed has been written (max_lists of them
    were stored) — a caller sizes its next call from it."""
    b = ctx.b1 if P == 1 else ctx.b2
    keys, lens, count = np.zeros((N, 2, 48), np.uint8), np.zeros((N, 2), np.uint8), np.full(N, -7, np.int32)
    rc = ctx.lib.tetris_get_actions(b._h, None, N, None, p(keys), p(lens), p(count), 2, 48)
    msg = ctx.lib.tetris_last_error().decode()
    assert rc == E_ARG and "more than max_lists key lists for one game" in msg, f"rc {rc} ('{msg}')"
    assert count.tolist() == [2, -7, -7], count.tolist()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_refused_calls_leave_the_batches_usable(kind, ctx):
    """after the table: no sticky error, the limits a good call takes are accepted, and the games still step"""
    for b in (ctx.b1, ctx.b2, ctx.s0, ctx.s1):
        b.sync()
        assert b.take_errors() == 0
    assert ctx.lib.tetris_debug_table_limit(ctx.b1._h, 64) == 0 and ctx.lib.tetris_debug_table_limit(ctx.b1._h, 0) == 0
    assert ctx.lib.tetris_rollout_launch(ctx.b2._h, 1, 256, 1, 0, 400, None) == 0
    assert ctx.lib.tetris_reset(ctx.b2._h, None, 0, None) == 0
    lists = ctx.b2.get_actions(player=[0, 1, 1], max_lists=64, max_keys=255)
    assert all(len(l) >= 1 for l in lists)
    done, _, _ = ctx.b2.step_keys(ctx.keys, ctx.lens)
    assert done.shape == (N,)
