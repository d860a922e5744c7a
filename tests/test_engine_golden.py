"""The bitboard engine against the compiled reference's golden traces (tests/golden, made by
make_golden.py from oracle/_ref): every event, every field the reference can show (cells compared
as occupancy).  `harness` = same kernel bodies built by g++ (CPU suite); `hip` = the product on GPU."""
import numpy as np
import pytest

from tests import engines, replay

FIELDS = replay.VISIBLE + replay.HIDDEN


@pytest.mark.parametrize("name", replay.trace_names())
def test_engine_replays_reference_trace(name):
    """Every trace on its own, full length, through a 1-game batch of the CPU harness build (the HIP path replays the same
    traces at full length as the games of one batch per geometry: test_all_traces_full_length_in_one_batch)."""
    trace = replay.load_trace(name)

    def factory(P, H, W, pieces, seed):
        return engines.make("harness", 1, P, H, pieces, seeds=seed)

    n = replay.replay(trace, factory, fields=FIELDS, occupancy_only=True, check_actions=True)
    assert n > 0


GROUPS = sorted(replay.trace_groups().items())


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("colours", [False, True])
@pytest.mark.parametrize("key,names", GROUPS, ids=["-".join(names) for _, names in GROUPS])
def test_all_traces_full_length_in_one_batch(kind, colours, key, names):
    """All 31 reference traces at FULL length (no event cut): the traces of one geometry and elapsed time per action are the games
    of ONE batch, so every event index is one reset call + one make/finish pair + one observe for all of them — 49 000 reference
    events through the batched entry points with index lists, `get_actions` lists included where the reference recorded them.  With
    colours: State.field values 0..8 and garbageCleared exactly (gamePlay.cpp:146,202; gameField.cpp:120-145)."""
    def factory(n, P, H, W, pieces, seeds):
        return engines.make(kind, n, P, H, pieces, seeds=seeds, colours=colours)

    pairs = replay.replay_batch(names, factory, fields=FIELDS + (replay.COLOUR_ONLY if colours else []), occupancy_only=not colours,
                                check_actions=not colours)
    assert pairs == sum(len(replay.load_trace(n)["ev_kind"]) for n in names)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("name", ["greedy_2p", "keys_2p_22", "greedy_2p_o", "rt_2p", "garbage_flood_2p"])
def test_colour_planes_give_the_reference_field_values(kind, name):
    """TETRIS_FLAG_COLOURS: State.field with tile values 1..7 / garbage 8 and GameplayData.garbageCleared exactly as the
    compiled reference shows them (gamePlay.cpp:146,202; gameField.cpp:120-145), over traces with garbage traffic."""
    trace = replay.load_trace(name)

    def factory(P, H, W, pieces, seed):
        return engines.make(kind, 1, P, H, pieces, seeds=seed, colours=True)

    n = replay.replay(trace, factory, fields=FIELDS + replay.COLOUR_ONLY, occupancy_only=False,
                      max_events=None if kind == "harness" else 300)
    assert n > 0


def test_golden_traces_reach_the_rare_paths():
    """The fixtures are only worth their bytes if replaying them runs the branches they were recorded for: counted in the
    CPU harness build (tetris_engine.h TE_COUNT) over the traces that were made for garbage and lock-down."""
    engines.harness_path_counts()                      # clear
    total = dict.fromkeys(engines.PATH_COUNTERS, 0)
    for name in ("garbage_flood_2p", "garbage_flood_2p_12", "greedy_2p", "keys_2p", "greedy_1p"):
        trace = replay.load_trace(name)
        replay.replay(trace, lambda P, H, W, pieces, seed: engines.make("harness", 1, P, H, pieces, seeds=seed), fields=FIELDS,
                      occupancy_only=True)
        for k, v in engines.harness_path_counts().items():
            total[k] += v
    for name in ("garbage_row", "death_garbage", "death_spawn", "timer_lock", "key_kick", "key_kick_failed"):
        assert total[name] > 0, (name, total)
    # gamePlay.cpp:184-190: the second lift cannot happen — a piece lifted with the stack keeps its position relative to it
    assert total["garbage_lift2"] == 0
    _traces_at_other_elapsed_times_reach_their_regimes()


def _traces_at_other_elapsed_times_reach_their_regimes():
    """The traces recorded at other elapsed times per action than 400 ms, by what the REFERENCE's records show: the drop delay
    through all its reduction tiers down to the floor (3001), combos longer than any 400 ms trace has (50), packets queued several
    deep and blocked (100), half lines between three players (1500), a clock that never moves (0), many lines from one expired
    combo (60000), a clock past 2^24 with odd values, which the int -> float conversion of Combo.cpp:40 rounds (60001).  And by
    what replaying them runs in the CPU harness build: the lock-down timer locking pieces (170, 401)."""
    rec = {name: replay.load_trace(name)["records"] for name in replay.trace_names()}
    ms = {name: int(replay.load_trace(name)["ms"]) for name in replay.trace_names()}
    assert sorted(set(ms.values())) == [0, 50, 100, 170, 400, 401, 1500, 3001, 60000, 60001]
    assert max(int(r["fifo_len"].max()) for r in rec.values()) <= 6             # clear of the engine's capacity of 8
    delay = rec["greedy_1p_ms3001"]["drop_delay"]
    assert delay.min() == 10
    for lo, hi in ((100, 200), (50, 100), (10, 50)):
        assert ((delay > lo) & (delay <= hi)).any(), (lo, hi)
    combo_400 = max(int(rec[n]["combo_count"].max()) for n in rec if ms[n] == 400)
    combo_50 = int(rec["greedy_1p_ms50"]["combo_count"].max())
    print(f"longest combo: {combo_400} at 400 ms, {combo_50} at 50 ms")
    assert combo_50 > combo_400 and combo_50 >= 17
    r = rec["greedy_2p_ms100"]
    assert r["fifo_len"].max() >= 4 and r["lines_blocked"].max() > 0
    assert (rec["greedy_3p_io_ms1500"]["incoming"] % 1 == 0.5).any()
    assert (rec["rt_2p_ms0"]["time_ms"] == 0).all() and (rec["rt_2p_ms0"]["drop_delay"][2:] == 1000).all()

    def most_sent(r):
        return int(np.diff(r["lines_sent"].astype(np.int64), axis=0).max())

    # a combo of ONE clear sends five lines and more: 1 + t / 60000 * 0.1 has grown to several times its value at the start
    assert rec["greedy_2p_ms60000"]["combo_count"].max() == 1 and most_sent(rec["greedy_2p_ms60000"]) >= 5
    t = rec["greedy_1p_ms60001"]["time_ms"]
    assert ((t > 2 ** 24) & (t % 2 == 1)).sum() > 20 and most_sent(rec["greedy_1p_ms60001"]) > 10
    for name in ("keys_2p_ms401", "keys_2p_ms170"):
        engines.harness_path_counts()                  # clear
        replay.replay(replay.load_trace(name), lambda P, H, W, pieces, seed: engines.make("harness", 1, P, H, pieces, seeds=seed), fields=FIELDS,
                      occupancy_only=True)
        counts = engines.harness_path_counts()
        print(f"{name}: timer_lock {counts['timer_lock']}")
        assert counts["timer_lock"] > 0, (name, counts)
