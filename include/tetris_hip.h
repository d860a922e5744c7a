/* tetris_hip.h — C ABI of the MI355X-native batched Tetris environment (libtetris_hip.so).
 *
 * This is the drop-in boundary for the environment-step path of mightypirate1/DRL-Tetris.
 * In the reference that boundary is the pybind11 module `tetris_env`
 * (environment/game_backend/source/PythonHandle.h:113-340) consumed by
 * environment/tetris_environment.py and environment/tetris_environment_vector.py; one
 * `PythonHandle` = one game.  Here one `tetris_batch` = N games resident in HBM on one GPU and
 * every entry point works on a list of game indices, so the per-env Python loops of
 * tetris_environment_vector.py:55-120 become one kernel launch.  Each function below names the
 * reference interface it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - plain C types only; caller owns every host buffer, the library owns all device memory.
 *  - return value: 0 = OK, negative = error (TETRIS_E_*); tetris_last_error() gives the text
 *    (thread-local).  There is no CPU fallback: without a HIP device tetris_create fails.
 *  - `idx` = int32 game indices (unique within one call), NULL = games 0..n-1.
 *  - per-player arrays are [n][P] (game-major) on the host side.
 *  - a batch is not thread-safe; different batches are independent (one HIP stream each).
 *  - functions ending in _dev take DEVICE pointers, enqueue on the batch's stream and return
 *    without synchronising (zero-copy callers, benchmarks); all others are synchronous.
 *    Host index / player arrays are validated (TETRIS_E_ARG); device-resident ones cannot be, so an
 *    out-of-range game index or player in a d_idx / d_player array is clamped into the batch by the kernel.
 *  - board height 4..31, width 10 (the reference hard-codes 10, gamePlay.cpp:202), 1..4 players per game (the reference
 *    takes any n_players, PythonHandle.cpp:5-25; none of its presets or agents uses more than two).  Three and four players
 *    run through the general one-lane-per-game kernel (all of a game's players in one lane); the packed observation
 *    (own / opponent planes), the one-launch step + observation, split batches and chained launches are one- and
 *    two-player features.
 *  - `ms` (every stepping entry point) = the game time that passes per action: the reference's
 *    settings["time_elapsed_each_action"] (400 in its presets), which tetris_environment.py:110 hands to finish_action(ms).  Any
 *    non-negative int; 0 (time stands still) to 60 000 is tested against the compiled reference and the oracle.
 *    The episode clock is an int32 as in the reference (gamePlay.h:64) and starts at 0 with every reset: one episode
 *    may last 2^31 ms of game time, 35 791 actions at 60 000 ms.  A small `ms` makes one capacity limit easier to hit: garbage
 *    packets wait 1000 ms of game time in the queue, so the fewer milliseconds pass per action the more packets are pending at
 *    once — 8 per board at most (TETRIS_ERR_FIFO below; strong two-player play reaches 8 at 0..1 ms, 7 at 50 ms, 4 at 100 ms
 *    and above).
 */
#ifndef TETRIS_HIP_H
#define TETRIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TETRIS_OK 0
#define TETRIS_E_ARG (-1)        /* bad argument */
#define TETRIS_E_HIP (-2)        /* a HIP runtime call failed (no device, out of memory, ...) */
#define TETRIS_E_STREAM (-3)     /* (no longer returned: see TETRIS_ERR_STREAM) */
#define TETRIS_E_FIFO (-4)       /* (no longer returned: see TETRIS_ERR_FIFO) */

/* Capacity errors are confined to the game they happen in.  The reference's garbage queue is an unbounded vector
 * (Garbage.h:27) and its generators never run out (randomizer.h:44-50); here a board holds at most 8 pending garbage
 * packets and an episode at most 39 936 piece draws.  A game that exceeds either ends its round in that step (`done`), its
 * boards carry the bits below in tetris_record.fifo_overflow until the game is reset, and every other game of the batch
 * goes on untouched.  tetris_take_errors tells whether any game of the batch was ended this way since the last call.
 * THE RULE.  Draws: the step in which a board's piece_draws REACHES the limit (tetris_record.piece_draws: two at the reset, one
 * more with every piece dealt; every live board is dealt one per step) — the piece that appears in that step is still right,
 * the `next` behind it is the first that is not.  TETRIS_ERR_STREAM is set on EVERY board of the game: the seed, and with it the
 * tables, is the game's.  Queue: the step in which a packet arrives at a board that has 8 pending; TETRIS_ERR_FIFO is set on that
 * board and on no other, the packet is dropped, the eight stay.
 * WHAT THE STEP SHOWS.  done = 1; `lines` and `dead`, the boards' lines_cleared / lines_sent and the per-game counters of the
 * built-in rollouts (lines cleared, lines sent, one episode) are what the step did before it was cut short — the reference's
 * numbers for that step.  Nobody need be dead: a game ended this way has done = 1 with all its `dead` flags 0 (a player who dies
 * in that very step is dead as usual), so tetris_traj_record_dev's reward for it is 0, and the reset that follows leaves
 * last_winner as for any round that is reset with more than one player alive: -1 (one-player games: 0).
 * AFTERWARDS.  Without auto-reset the game is round-over: stepping calls leave it exactly as it is (done = 1 every time) until
 * tetris_reset / tetris_reset_dev, after which it is an ordinary game again.  With TETRIS_STEP_AUTO_RESET and in the built-in
 * rollouts it is reset inside the same launch like any finished game, so the bits are gone from its boards when the call
 * returns, and tetris_take_errors is the only witness.  (State.inc_count of a board is refreshed by a step, not by a reset —
 * here as in the reference: until its next step a board reset after TETRIS_ERR_FIFO shows the total of the eight packets it held.)
 * A SIMULATION ENDS NO GAME: a list of tetris_simulate_lists_dev whose afterstate runs over either limit has done = 1 in the
 * simulation's own output; the batch's state is not written and tetris_take_errors is not told.                            */
#define TETRIS_ERR_FIFO 1u       /* a 9th garbage packet arrived while 8 were pending: it was dropped */
#define TETRIS_ERR_STREAM 2u     /* the episode ran past the RNG tables: the pieces dealt in that step are wrong */
/* Not a capacity error and nothing is wrong with any game: reported once by tetris_take_errors after a chained rollout call had
 * to finish some of its games un-chained (see tetris_set_chained) — the results are the same, the call was slow, and chained
 * launches are off for the batch from then on.                                                                          */
#define TETRIS_ERR_CHAIN_FELL_BACK 4u
#define TETRIS_ERR_LISTS 8u      /* tetris_action_lists_dev: a game had more lists / keys than the caller's buffers (its count is -1) */

#define TETRIS_MAX_H 32
#define TETRIS_MAX_PLAYERS 4   /* players per game (PythonHandle(n_players, ...): PythonHandle.cpp:5-25) */
#define TETRIS_W 10
#define TETRIS_FIFO_CAP 16

/* Everything the reference can show about one player-board (State views PythonHandle.h:54-82 and
 * the pickled members PythonHandle.h:123-308), flattened.  Same layout as the test oracle's record. */
typedef struct tetris_record {
    uint8_t  field[TETRIS_MAX_H][TETRIS_W]; /* State.field (occupancy: 0 / 1)                  */
    uint8_t  grid[4][4];                    /* State.piece                                      */
    int8_t   x, y;                          /* State.x, State.y                                 */
    uint8_t  piece, tile, spawn_rot, cur_rot, big;   /* basePieces (pieces.h:7-28)             */
    uint8_t  next, dead, reward, inc_count, combo_count;   /* State.*                           */
    uint16_t combo_remaining;               /* State.combo_time                                 */
    uint8_t  lock_armed, fifo_len, line_count, fifo_overflow;
    int32_t  time_ms;
    float    incoming;
    int32_t  drop_delay, drop_time, speedup_time, lock_time;   /* DropDelay.h:6-18              */
    int32_t  min_remaining;
    int32_t  combo_start, combo_time;
    int32_t  fifo_delay[TETRIS_FIFO_CAP];
    int16_t  fifo_count[TETRIS_FIFO_CAP];
    uint16_t lines_sent, lines_cleared, lines_blocked, garbage_cleared, max_combo, lines_cleared_seen;
    float    weights[7];                    /* not tracked on the GPU (always 0)                */
    uint32_t piece_draws, hole_draws;
} tetris_record;

typedef struct tetris_batch tetris_batch;

const char *tetris_last_error(void);
int         tetris_device_count(void);                 /* < 0 on error                          */
int         tetris_device_name(int device, char *buf, int len);   /* "<name> (<arch>, <n> CUs)"  */
int         tetris_record_size(void);
int         tetris_snapshot_words(const tetris_batch *b);   /* uint32 words per game in a snapshot */

/* replaces: tetris_env.set_pieces(map) + PythonHandle(n_players, [H, W]) for n_games games
 * (PythonHandle.h:116-121,309; PythonHandle.cpp:5-25).  seeds[n_games] (host, NULL = all 0) stand
 * in for time(NULL) at construction (PythonHandle.cpp:68-71).                                   */
int tetris_create(tetris_batch **out, int n_games, int n_players, int height, int width,
                  const uint8_t piece_map[7], int device, const int16_t *seeds);
/* same with options.  TETRIS_FLAG_COLOURS: also track the tile value of every square (1..7 = piece index + 1,
 * gamePlay.cpp:146; 8 = garbage, gamePlay.cpp:202) in three extra bit-planes per board, so that tetris_record.field
 * holds exactly what the reference's State.field shows and GameplayData.garbageCleared is produced.  Costs 120 B more
 * state per board; off by default because state_dict only uses field > 0.                                          */
#define TETRIS_FLAG_COLOURS 1
int tetris_create_ex(tetris_batch **out, int n_games, int n_players, int height, int width,
                     const uint8_t piece_map[7], int device, const int16_t *seeds, int flags);
int tetris_destroy(tetris_batch *b);
int tetris_sync(tetris_batch *b);                      /* drain the stream, surface sticky errors */
int tetris_take_errors(tetris_batch *b, uint32_t *bits);   /* synchronises; *bits = TETRIS_ERR_* seen since the last call, then cleared */

/* replaces: PythonHandle.reset() with time(NULL) == seeds[i] (PythonHandle.cpp:49-71)           */
int tetris_reset(tetris_batch *b, const int32_t *idx, int n, const int16_t *seeds);

/* replaces: PythonHandle.make_action(list[list[int]]) (PythonHandle.cpp:138-147).
 * keys[n][P][max_keys] uint8, lens[n][P] uint8 (host).                                          */
int tetris_make_actions(tetris_batch *b, const int32_t *idx, int n, const uint8_t *keys,
                        const uint8_t *lens, int max_keys);
/* replaces: PythonHandle.finish_action(ms) (PythonHandle.cpp:149-188).  done[n]; lines[n][P] =
 * State.reward, dead[n][P] = State.dead after the call (either may be NULL).                    */
int tetris_finish_actions(tetris_batch *b, const int32_t *idx, int n, int ms, uint8_t *done,
                          uint8_t *lines, uint8_t *dead);
/* make_action + finish_action in one launch = tetris_environment.perform_action
 * (tetris_environment.py:102-116).                                                              */
int tetris_step_keys(tetris_batch *b, const int32_t *idx, int n, const uint8_t *keys,
                     const uint8_t *lens, int max_keys, int ms, uint8_t *done, uint8_t *lines,
                     uint8_t *dead);
/* perform_action on ALL games with the SVENton (rotation, translation) encoding
 * [8]*r + [2] + [3]*t + [7] for `player[g]`, [0] for the others (sventon_utils.py:9-13).
 * rot/trans/player/done [N], lines/dead [N][P]; player NULL = player 0.                         */
int tetris_step_rt(tetris_batch *b, const uint8_t *rot, const uint8_t *trans, const uint8_t *player,
                   int ms, uint8_t *done, uint8_t *lines, uint8_t *dead);
/* same, device pointers, asynchronous.  d_lines/d_dead are [P][N] (player-major) on the device. */
int tetris_step_rt_dev(tetris_batch *b, const uint8_t *d_rot, const uint8_t *d_trans,
                       const uint8_t *d_player, int ms, uint8_t *d_done, uint8_t *d_lines,
                       uint8_t *d_dead);
/* same with flags.  TETRIS_STEP_AUTO_RESET: a game whose round ended in this step is reset inside the same launch —
 * the `env.reset(env=[done idxs])` of the worker loop (drl_tetris/worker.py:157-166 -> PythonHandle.cpp:49-71) without
 * a host round trip.  The seed is the next one of the built-in schedule, seed16 = (12345 + 7919 game + 104729 episode)
 * mod 65536 with game = global game id (tetris_set_game_offset) and episode = the game's count of resets so far;
 * d_done / d_lines / d_dead report the step as it ended, BEFORE the reset.
 * The asynchronous entry points never drain the stream: requests to extend the RNG tables reach the host through
 * flag words in pinned memory, and the host lets at most 241 launches run ahead of what it has seen of them.       */
#define TETRIS_STEP_AUTO_RESET 1
int tetris_step_rt_dev_ex(tetris_batch *b, const uint8_t *d_rot, const uint8_t *d_trans,
                          const uint8_t *d_player, int ms, uint8_t *d_done, uint8_t *d_lines,
                          uint8_t *d_dead, int flags);
/* One iteration of the agent loop in ONE launch (drl_tetris/worker.py:91-118: perform_action, then get_state + the unpacker
 * for the next decision): tetris_step_rt_dev_ex followed by tetris_observe_packed_dev(b, NULL, N, d_next_player, ...) of the
 * stepped (and, with TETRIS_STEP_AUTO_RESET, reset) state — produced from the registers the step leaves behind instead of a
 * second kernel that reads the state back.  d_next_player[N] = the player each game's next decision is for (NULL: player 0;
 * out-of-range entries are clamped); d_visual [P][N][H][10], d_vector [P][N][12], d_piece [P][N] as tetris_observe_packed.
 * Same outputs, bit for bit, as the two calls.  Colour batches, odd heights and outputs that are not 4-byte aligned run
 * the two kernels back to back; not available on split batches.                                                        */
int tetris_step_rt_observe_dev(tetris_batch *b, const uint8_t *d_rot, const uint8_t *d_trans,
                               const uint8_t *d_player, int ms, uint8_t *d_done, uint8_t *d_lines,
                               uint8_t *d_dead, int flags, const uint8_t *d_next_player,
                               uint8_t *d_visual, uint8_t *d_vector, uint8_t *d_piece);
/* replaces: reset() of the games selected by a DEVICE-side mask (d_mask[N], non-zero = reset; NULL = all games),
 * asynchronous.  d_seeds[N] int16 (device) or NULL = next seed of the built-in schedule (see above).              */
int tetris_reset_dev(tetris_batch *b, const uint8_t *d_mask, const int16_t *d_seeds);

/* replaces: reading PythonHandle.states[p].* / __getstate__() (PythonHandle.h:54-82,123-308).
 * records[n][P]; round_over[n]; last_winner[n] (PythonHandle.last_winner); NULLs allowed.       */
int tetris_observe_records(tetris_batch *b, const int32_t *idx, int n, tetris_record *records,
                           uint8_t *round_over, int8_t *last_winner);

/* replaces: state_processors.state_dict + agent_utils/state_unpack.unpacker in its default SVENton configuration
 * (state_processors.py:23-54; state_unpack.py:88-137: observation_mode 'separate', player_mode 'separate',
 * separate_piece): NN-ready observations written by one kernel.  Slot 0 = the board of player[i] ("me"), slot 1 = the
 * opponent (only when n_players == 2).  All outputs uint8:
 *   visual [S][n][H][W]  field > 0
 *   vector [S][n][12]    x, y, inc_lines, min(25000, combo_time + 50) / 100, combo_count, nextpiece one-hot (7)
 *   piece  [S][n]        index of the current piece (state_dict "piece_idx")
 * Host pointers (synchronous); the _dev variant takes device pointers and only enqueues.                          */
int tetris_observe_packed(tetris_batch *b, const int32_t *idx, int n, const uint8_t *player, uint8_t *visual,
                          uint8_t *vector, uint8_t *piece);
int tetris_observe_packed_dev(tetris_batch *b, const int32_t *d_idx, int n, const uint8_t *d_player,
                              uint8_t *d_visual, uint8_t *d_vector, uint8_t *d_piece);

/* replaces: PythonHandle.copy() / .set() (PythonHandle.cpp:36-42): exact state incl. RNG position.
 * blob[n][tetris_snapshot_words()] uint32 (host).  Blobs move between batches of equal geometry
 * and piece map.                                                                                 */
int tetris_snapshot(tetris_batch *b, const int32_t *idx, int n, uint32_t *blob);
int tetris_restore(tetris_batch *b, const int32_t *idx, int n, const uint32_t *blob);
/* replaces: Python writing State.dead on a live handle (data_types/state.py:11,16). dead[n][P]  */
int tetris_set_dead(tetris_batch *b, const int32_t *idx, int n, const uint8_t *dead);

/* replaces: the drop part of PythonHandle.get_actions(player) + simulate_actions(finalize=False)
 * (TestField.cpp:64-125 getMask/findNextMove; tetris_environment.py:87-100): for every listed game, the current
 * piece of player[i] (NULL = player 0) placed at (x, 0), x = xi - 1 for xi = 0..9, with absolute rotation r = 0..3
 * (only the rotations the reference enumerates: 1 for O, 2 for I/S/Z, 4 for L/J/T); where it fits it is hard-dropped
 * and stamped.  valid/land_y/cleared [n][4][10] (cleared = rows a finalize would remove);
 * after [n][4][10][10] = the stamped board's column bitboards before line clear (NULL to skip).  One lane per
 * (game, r, x): 40 lanes per board.                                                                              */
int tetris_enumerate_drops(tetris_batch *b, const int32_t *idx, int n, const uint8_t *player, uint8_t *valid,
                           int8_t *land_y, uint8_t *cleared, uint32_t *after);

/* same with device pointers (d_idx / d_player may be NULL), asynchronous on the batch's stream                        */
int tetris_enumerate_drops_dev(tetris_batch *b, const int32_t *d_idx, int n, const uint8_t *d_player,
                               uint8_t *d_valid, int8_t *d_land_y, uint8_t *d_cleared, uint32_t *d_after);
/* same with flags.  TETRIS_ENUM_PLANAR: rotation-minor planes — d_valid / d_land_y / d_cleared are [n][10][4] (game, column
 * index xi, rotation r) and d_after is [10][n][10][4]: column c of the placement (game i, rotation r, column index xi) at
 * d_after[((c * n + i) * 10 + xi) * 4 + r].  The four rotations of a (game, column) pair are adjacent, so the kernel writes
 * each result array with one 4-byte store and each afterstate column with one 16-byte store per lane, 1 KB contiguous per
 * wavefront; a consumer that feeds the afterstates to a network reads one column plane [n][10][4] at a time.
 * d_valid / d_land_y / d_cleared must be 4-byte aligned, d_after 16-byte aligned.                                      */
#define TETRIS_ENUM_PLANAR 1
int tetris_enumerate_drops_dev_ex(tetris_batch *b, const int32_t *d_idx, int n, const uint8_t *d_player,
                                  uint8_t *d_valid, int8_t *d_land_y, uint8_t *d_cleared, uint32_t *d_after, int flags);

/* replaces: PythonHandle.get_actions(player); masks[player].action (PythonHandle.cpp:190, TestField.cpp:64-415):
 * the reference's exact ordered key lists of the "place_block" action type — every (x, rotation) drop plus the
 * tuck / spin placements found by its backwards search — for the current piece of player[i] (NULL = player 0).
 * count[n] = number of lists; list k of game i: lens[i][k] keys at keys[i][k][0..]; masks[player].mask of the reference after
 * this call is count[i] ones (TestField.cpp:113-133 pushes a 1 beside every list).  Python applies
 * data_types.action_list (dedupe, null-move policy) on top.  TETRIS_E_ARG if a game has more than max_lists lists
 * or a list more than max_keys keys (64 / 48 always suffice for 10-wide boards up to 31 rows).                   */
int tetris_get_actions(tetris_batch *b, const int32_t *idx, int n, const uint8_t *player, uint8_t *keys,
                       uint8_t *lens, int32_t *count, int max_lists, int max_keys);

/* ---- planning on the device: the afterstate loop of a planning agent without host round trips --------------------------
 * A planning agent asks, per decision and game, for the ordered key lists of the current piece, the afterstate of every list,
 * and then performs the list it picked (the reference's sherlock agent: agents/sherlock_agent/sherlock_agent.py:94-120,
 * sherlock_utils.py:9-20).  These three entry points do that for games 0..N-1 of a batch: device pointers, asynchronous on
 * the batch's stream, run-ahead bounded and RNG-table requests serviced as for tetris_step_rt_dev_ex.  Not on split batches.
 * Lists: count[N] int32, lens[N][L] uint8, keys[N][L][K] uint8 (L = max_lists, K = max_keys); entries past lens / count are
 * left as they were.  d_player[N] = acting player (NULL: player 0; out-of-range entries are clamped).                       */
#define TETRIS_LISTS_KEEP_NULL 1   /* bar_null_moves = False; default: nulls removed as action_list(remove_null=True) */
#define TETRIS_SIM_FINALIZE    1   /* simulate_actions(finalize=True): make_action + finish_action(ms) */
/* replaces: tetris_environment_vector.get_actions(player) = PythonHandle.get_actions + data_types.action_list(..., remove_null)
 * (PythonHandle.cpp:190, TestField.cpp:64-415, action_list.py:3-37): the lists tetris_get_actions gives, x-major and
 * rotation-minor, then the null action [0] in front unless present, duplicates dropped (first occurrence kept) and, without
 * TETRIS_LISTS_KEEP_NULL, nulls removed as long as something else remains — so count >= 1.  A game whose lists do not fit
 * L x K (1 <= K <= 254) gets count -1 and nothing else written; TETRIS_ERR_LISTS is raised (tetris_take_errors).          */
int tetris_action_lists_dev(tetris_batch *b, const uint8_t *d_player, int max_lists, int max_keys, int flags,
                            int32_t *d_count, uint8_t *d_lens, uint8_t *d_keys);
/* replaces: tetris_environment_vector.simulate_actions(lists, player, finalize) (tetris_environment.py:87-100): list k of
 * game i (k < count[i]) run through the key interpreter on a register copy of the game, [0] for the other players, with
 * TETRIS_SIM_FINALIZE followed by finish_action(ms).  d_cols [L][P][10][N] uint32 = every player's column bitboards
 * (bit y = row y) afterwards; with TETRIS_SIM_FINALIZE also d_done [L][N], d_lines / d_dead [L][P][N] as tetris_step_keys
 * reports them (each may be NULL).  Nothing is written for k >= count[i]; the batch's state is not written.               */
int tetris_simulate_lists_dev(tetris_batch *b, const uint8_t *d_player, const int32_t *d_count, const uint8_t *d_lens,
                              const uint8_t *d_keys, int max_lists, int max_keys, int ms, int flags,
                              uint32_t *d_cols, uint8_t *d_done, uint8_t *d_lines, uint8_t *d_dead);
/* replaces: perform_action(lists[choice[i]], player) (tetris_environment.py:102-116): bit-identical to tetris_step_keys with
 * the chosen list for the acting player and [0] for the others.  choice[N] int32 is clamped into [0, count - 1]; a game
 * with count < 1 performs [0].  flags: TETRIS_STEP_AUTO_RESET as for tetris_step_rt_dev_ex (outputs describe the step
 * before the reset).  d_done [N], d_lines / d_dead [P][N] (each may be NULL).                                             */
int tetris_step_lists_dev(tetris_batch *b, const uint8_t *d_player, const int32_t *d_choice, const int32_t *d_count,
                          const uint8_t *d_lens, const uint8_t *d_keys, int max_lists, int max_keys, int ms, int flags,
                          uint8_t *d_done, uint8_t *d_lines, uint8_t *d_dead);
/* replaces: sherlock_utils.deltas / generate_deltas (agents/sherlock_agent/sherlock_utils.py:9-20) for games 0..N-1: the
 * network input of the planning agent from the columns tetris_simulate_lists_dev wrote, in one kernel.  Device pointers,
 * asynchronous on the batch's stream like tetris_observe_packed_dev; one to four players, every height, colour batches
 * included (it reads occupancy); not on split batches.  The batch's state is read, not written, and the RNG tables are not
 * touched.  d_cols uint32 [L][P][10][N] as tetris_simulate_lists_dev without TETRIS_SIM_FINALIZE wrote it (L = max_lists,
 * 1 <= L <= 256); d_count [N] as tetris_action_lists_dev wrote it (below 0 counts as 0, above L as L); d_player as above.
 * For game i, acting player p and list k: `before` = p's ten column words in the batch's state now, `after` =
 * d_cols[k][p][c][i], both masked to rows 0..H-1; delta(y, x) = bit y of after[x] - bit y of before[x], in {-1, 0, 1};
 * s = the integer sum of the deltas of list k.  For k < count: if s < 4 the list is SMALL (the piece did not land whole, or
 * the player could not move: sherlock_utils.py:12-14) and every cell of it is small_fill, otherwise the cells are the
 * deltas; for k >= count every cell is 0 (the reference's zero padding to the longest list).  (The reference's own fields
 * are uint8, and np.full_like on them turns its 1e-3 into 0: small_fill = 0 gives those numbers.)
 *   d_deltas  [N][H][10][L] float32, the reference's layout; with TETRIS_DELTAS_LIST_MAJOR [N][L][H][10]
 *   d_sums    N x H x 10 elements ([N][H][10][1], list-major [N][1][H][10]: the same memory): the sum over the lists, defined
 *             without a reduction order as (float)(integer sum of the deltas of the lists k < count that are not small) +
 *             small_fill * (float)(number of small lists), one float32 multiply and one float32 add.  NULL: no sums.
 *   d_small   uint8 [N][L]: 1 where the small rule fired, else 0 (also for k >= count).  May be NULL.
 * With TETRIS_DELTAS_F16 d_deltas and d_sums hold IEEE binary16: the float32 value above rounded to nearest even.
 * d_deltas and d_sums must be 16-byte aligned, d_cols 4-byte aligned; TETRIS_E_ARG for that, for a max_lists out of range
 * and for a NULL d_count, d_cols or d_deltas.                                                                            */
#define TETRIS_DELTAS_F16        1   /* d_deltas / d_sums are IEEE binary16 instead of float32 */
#define TETRIS_DELTAS_LIST_MAJOR 2   /* d_deltas [N][L][H][W] instead of [N][H][W][L] */
int tetris_plan_deltas_dev(tetris_batch *b, const uint8_t *d_player, const int32_t *d_count, const uint32_t *d_cols,
                           int max_lists, float small_fill, int flags,
                           void *d_deltas, void *d_sums, uint8_t *d_small);

/* ---- choosing a planning agent's action list on the device from phi ------------------------------------------------------
 * replaces: the part of sherlock_agent.get_action between the network and perform_action (agents/sherlock_agent/
 * sherlock_agent.py:91-156 with sherlock_utils.py:34-63): the plane of the held piece out of the network's phi_eval
 * [N][H][10][K], p_unnormalized[k] = sum over (y, x) of deltas[.., k] * phi_p, the normalisation over the lists, the choice by
 * argmax or by the distribution, and (a_idx, piece, pi(a), v_piece, v_mean, delta(s, a), delta_sum(s)) for the trajectory —
 * without the [N][H][10][L] deltas tensor: the calls read the columns tetris_simulate_lists_dev (no TETRIS_SIM_FINALIZE) wrote.
 * (The PPO trainer recomputes pi(a) from delta and delta_sum alone, sherlock_agent_ppo_trainer.py:37-54: the sum over the lists
 * of p_unnormalized is sum(delta_sum * phi).)  The reference also names pareto and epsilon here, but sherlock_utils has no such
 * functions (sherlock_agent.py:124-136 would raise): they are out of scope.
 * Device pointers, asynchronous on the batch's stream, run-ahead bounded and RNG-table requests serviced as for
 * tetris_step_rt_dev_ex; one to four players, every height, colour batches included; not on split batches.
 * For game i:
 *   SETUP   p = d_player[i] (NULL: player 0; out-of-range entries are clamped).  PIECE = the index tetris_observe_packed gives
 *           for p's board now, limited to K - 1; K = n_pieces is 7 or 1.  count = d_count[i] clamped into [0, L], L = max_lists
 *           (1 <= L <= 256).  `before`, `after_k` (d_cols [L][P][10][N]), their masking to rows 0..H-1 and the list kinds
 *           (normal, SMALL, past count) are those of tetris_plan_deltas_dev.  w(y, x) = d_phi[i][y][x][PIECE], float32 or IEEE
 *           binary16 (TETRIS_ACT_F16), taken to float32 exactly.
 *   SCORES  float32 arithmetic, nothing contracted.  A normal list: score_k starts at +0.0f; columns c = 0..9 in turn, within
 *           a column rows y = 0..H-1 in turn; a cell whose delta is +1 does score += w(y, c), a cell whose delta is -1 does
 *           score -= w(y, c), a cell whose delta is 0 nothing (so the reference's 0 * inf = NaN is NOT reproduced).  A SMALL
 *           list: score_k = small_fill * W, one multiply, with C_c = the sequential sum of w(y, c) over y = 0..H-1 from +0.0f and
 *           W = ((C_0 + C_1) + C_2) + ... + C_9.  (small_fill = 0 is the reference, whose uint8 fields turn its 1e-3 into 0.)
 *           total = the sequential sum of score_k over k = 0..count-1 from +0.0f; q_k = score_k / total, correctly rounded,
 *           whatever the bits.
 *   CHOICE  count = 0: choice 0, d_prob and d_entropy 0, d_delta zeros.  If any q_k (k < count) is NaN: choice 0, entropy 0
 *           (sherlock_utils.py:49-51, 59-60).  Otherwise
 *           TETRIS_ACT_ARGMAX  the highest q_k, among equals the lowest k (compared with `>`);
 *           TETRIS_ACT_PI      weights m_k = q_k > 0 ? q_k : 0; u from Philox4x32-10 with the key and counter of
 *                              tetris_select_eval_dev — key (sample_seed, 0), counter (global game id, low word of `draw`, high
 *                              word of `draw`, 0), u = (w0 >> 8) * 2^-24; sum(m) = the float32 sum in index order; the choice is
 *                              the first k < count whose running sum (the same partial sums) is > u * sum(m), if there is none
 *                              the last k with m_k > 0, and if sum(m) is not a positive finite number ARGMAX's choice.
 *           Every path ends with 0 <= choice < max(count, 1).
 *   OUTPUTS all optional except d_choice:
 *           d_choice  int32 [N]    feeds tetris_step_lists_dev unchanged
 *           d_piece   uint8 [N]    the piece index used
 *           d_prob    float32 [N]  q_choice
 *           d_probs   float32 [N][L]  q_k for k < count, 0 from count on
 *           d_value   float32 [2][N]  from d_state_eval [N][V] exactly as in tetris_act_eval (TETRIS_ACT_VALUE_F16)
 *           d_entropy float32 [N]  PI only: -sum over k < count of q_k * logf(q_k + 1e-8f), in index order, accurate logf
 *           d_delta   [N][H][10]   the plane tetris_plan_deltas_dev would write for the chosen list
 *           d_sums    [N][H][10]   the same bits as tetris_plan_deltas_dev's d_sums
 *           d_delta and d_sums are float32, or IEEE binary16 (rounded to nearest even) with TETRIS_PLAN_OUT_F16.
 * TETRIS_E_ARG: a NULL argument struct, d_phi, d_count, d_cols or d_choice; n_pieces not 1 or 7; d_state_eval with n_values
 * not 1, 7 or 8; a mode other than ARGMAX and PI; d_value without d_state_eval; d_entropy outside PI; an unknown flag;
 * max_lists outside [1, 256]; a d_phi, d_delta or d_sums that is not 16-byte aligned; a split batch.                        */
#define TETRIS_PLAN_OUT_F16 4   /* d_delta / d_sums are IEEE binary16 instead of float32 (beside TETRIS_ACT_F16 = 1, TETRIS_ACT_VALUE_F16 = 2) */
typedef struct tetris_plan_eval {
    const void     *d_phi;          /* [N][H][10][n_pieces] float32, or binary16 with TETRIS_ACT_F16; 16-byte aligned */
    const void     *d_state_eval;   /* [N][n_values], or NULL */
    int             n_pieces;       /* K */
    int             n_values;       /* V */
    int             mode;           /* TETRIS_ACT_ARGMAX or TETRIS_ACT_PI */
    int             flags;          /* TETRIS_ACT_F16 | TETRIS_ACT_VALUE_F16 | TETRIS_PLAN_OUT_F16 */
    uint32_t        sample_seed;
    uint32_t        reserved;       /* 0 */
    uint64_t        draw;           /* the number of this draw, e.g. the agent's step */
    float           small_fill;
    const uint8_t  *d_player;       /* [N] or NULL */
    const int32_t  *d_count;        /* [N] */
    const uint32_t *d_cols;         /* [L][P][10][N] */
    int             max_lists;      /* L */
    int32_t        *d_choice;       /* [N] */
    uint8_t        *d_piece;
    float          *d_prob, *d_probs, *d_value, *d_entropy;
    void           *d_delta, *d_sums;   /* [N][H][10] each; 16-byte aligned */
} tetris_plan_eval;
/* the choice and its outputs.  The batch's state is not written.                                                          */
int tetris_select_lists_dev(tetris_batch *b, const tetris_plan_eval *e);
/* the choice and perform_action of it: tetris_select_lists_dev followed by tetris_step_lists_dev with d_choice, bit for bit
 * (d_lens / d_keys / max_keys / ms / flags / d_done / d_lines / d_dead as there; a NULL d_lens or d_keys: TETRIS_E_ARG).   */
int tetris_step_lists_eval_dev(tetris_batch *b, const tetris_plan_eval *e, const uint8_t *d_lens, const uint8_t *d_keys,
                               int max_keys, int ms, int flags, uint8_t *d_done, uint8_t *d_lines, uint8_t *d_dead);

/* ---- heuristic policy on the device: a one-piece look-ahead over the 40 SVENton (rotation, translation) actions -----------
 * The scripted player the golden traces were recorded with (tests/golden/policies.py: GreedyRT), for every game of a batch at
 * once: a fixed-strength opponent for two-player training, the inner loop of feature-based learning (one weight vector per
 * game, per-game lines cleared), and a rollout on boards that look like play.  The reference has no such player (it trains by
 * self-play: drl_tetris/worker.py:91-118); its action encoding is the SVENton one (sventon_utils.py:9-13).
 * For game i, acting player p and candidate c = 10 r + t (r = 0..3, t = 0..9) the CANDIDATE FIELD is p's occupancy after
 * make_action of [8]*r + [2] + [3]*t + [7] for p and [0] for the others, without finish_action — what
 * tetris_simulate_lists_dev without TETRIS_SIM_FINALIZE shows for that list: the piece is stamped, full rows are still
 * present (a dead player's or a finished round's field is the board as it stands).  Row 0 is the top, H the batch's height.
 * A candidate field has TETRIS_POLICY_FEATURES integer features.  Feature 0 is counted on the field as it is; for features
 * 1-7 the full rows are removed first and the rows above move down.  With h[c] = H minus the index of the topmost filled
 * row of column c (0 for an empty column):
 *   0 lines              number of full rows
 *   1 holes              empty cells with a filled cell above them in the same column
 *   2 bumpiness          sum over c = 0..8 of |h[c+1] - h[c]|
 *   3 aggregate height   sum of h[c]
 *   4 max height         max of h[c]
 *   5 row transitions    per row, changes along wall, cell 0..9, wall with both walls filled (an empty row gives 2); summed
 *   6 column transitions per column, changes along cell 0..H-1, floor with the floor filled (no ceiling); summed
 *   7 wells              sum over c of d (d + 1) / 2, d = max(0, min(h[c-1], h[c+1]) - h[c]), h[-1] = h[10] = H
 * Score of a candidate = sum of w[k] * f[k] with int16 weights, in int32 (it cannot overflow: the largest feature is 4 960).
 * The CHOICE is the candidate with the highest score, among equal scores the lowest c — ties are the normal case
 * (translations past the wall and the repeated rotations of O, I, S, Z give identical fields); all-zero weights choose
 * (0, 0).  No floating point anywhere.  d_weights: int16 [8] for the batch, or with per_game != 0 [N][8], one vector per game.
 * All entry points: device pointers, asynchronous on the batch's stream, run-ahead bounded and RNG-table requests serviced
 * as for tetris_step_rt_dev_ex; d_player[N] = acting player (NULL: player 0; out-of-range entries are clamped); one to four
 * players, every height, colour batches included (the policy reads occupancy).  Not on split batches.                     */
#define TETRIS_POLICY_FEATURES 8
/* the features of all 40 candidates of every game: d_features int16 [40][8][N] (candidate-major like d_cols of
 * tetris_simulate_lists_dev: a wavefront stores whole rows).  The batch's state is not written.                          */
int tetris_rt_features_dev(tetris_batch *b, const uint8_t *d_player, int16_t *d_features);
/* the choice: d_rot / d_trans uint8 [N] and its score d_score int32 [N] (d_score may be NULL).  The outputs feed
 * tetris_step_rt_dev unchanged.  The batch's state is not written.                                                       */
int tetris_policy_rt_dev(tetris_batch *b, const uint8_t *d_player, const int16_t *d_weights, int per_game,
                         uint8_t *d_rot, uint8_t *d_trans, int32_t *d_score);
/* the choice and perform_action of it (tetris_environment.py:102-116) in one call: bit-identical to tetris_policy_rt_dev
 * followed by tetris_step_rt_dev_ex.  flags: TETRIS_STEP_AUTO_RESET as there; d_done [N], d_lines / d_dead [P][N] describe
 * the step before the reset; d_rot / d_trans [N] (each may be NULL) report what was played.  The scripted-opponent call: the
 * learner moves player 0 with tetris_step_rt_dev, the library moves player 1.                                            */
int tetris_step_policy_dev(tetris_batch *b, const uint8_t *d_player, const int16_t *d_weights, int per_game, int ms,
                           int flags, uint8_t *d_done, uint8_t *d_lines, uint8_t *d_dead, uint8_t *d_rot, uint8_t *d_trans);
/* tetris_rollout_random with this policy in place of the Philox draw: acting player = step mod P, [0] for the others,
 * auto-reset with the built-in seed schedule keyed by global game id, the same per-game counter words, `counters` and
 * `elapsed_ms` as there (synchronous).  1 <= steps_per_launch <= 256; more than one step per launch gives the same results
 * as one (the state stays in registers inside a launch, and each game's lane evaluates its own 40 candidates).  Runs
 * un-chained on the batch's stream: tetris_rollout_is_chained and the chained / direct-dispatch paths do not apply.
 * CAPACITY: this policy clears about 0.39 lines per piece in one-player games and does not die, so an episode is not ended by
 * the game but by the 39 936-draw limit: after about 40 000 steps it is ended with TETRIS_ERR_STREAM (see above) and reset
 * like any finished game.
 * `counters[k] +=` is exactly what THIS call did, whatever the per-game words held before it (see tetris_rollout_random).  */
int tetris_rollout_policy(tetris_batch *b, int launches, int steps_per_launch, const int16_t *d_weights, int per_game,
                          uint64_t first_step, int ms, uint64_t counters[4], float *elapsed_ms);
/* the per-game words tetris_rollout_totals sums: d_totals uint32 [4][N] = {env_steps, episodes, lines_cleared, garbage_sent}
 * of every game — a population's fitness without a host loop.  Asynchronous.  The words are cumulative MODULO 2^32 and are
 * delivered as they stand (a game passes 2^32 env-steps after a few hours of the built-in rollout): the difference of two
 * readings, taken modulo 2^32, is exact as long as the game counted fewer than 2^32 in between.                          */
int tetris_rollout_game_totals_dev(tetris_batch *b, uint32_t *d_totals);

/* ---- acting on a network's (r, t, piece) evaluation on the device ---------------------------------------------------------
 * replaces: the part of sventon_agent.get_action between the network and perform_action (agents/sventon_agent/sventon_agent.py:
 * 56-98 with sventon_utils.py:15-76: action_argmax / action_distribution / action_pareto / action_epsilongreedy, value_piece,
 * value_mean) for every game of a batch at once: with the network in torch on the same GPU the agent loop is network forward,
 * one call, network forward.
 * For game i the acting player is p = d_player[i] (NULL: player 0; out-of-range entries are clamped).  PIECE is the kind held in
 * p's board now — the index tetris_observe_packed writes to `piece` (state_dict "piece_idx") — limited to K - 1.  K = n_pieces
 * is the last dimension of the evaluation: 7, or 1 when the network takes the piece in its state vector (the piece is then 0).
 * d_action_eval is a contiguous [N][4][10][K] array of float32, or of IEEE binary16 with TETRIS_ACT_F16.  Candidate c = 10 r + t
 * (r = 0..3, t = 0..9) has the value x[c] = d_action_eval[i][r][t][piece], taken to float32 exactly.
 * The CHOICE, by mode:
 *   TETRIS_ACT_ARGMAX   (action_argmax)  the highest x[c] among the candidates that are not NaN, among equals the lowest c
 *                       (values are compared with `>`, so a NaN never wins); if all 40 are NaN the choice is 0.
 *   TETRIS_ACT_PI       (action_distribution)  the inverse-CDF draw below with the weights m[c] = x[c] > 0 ? x[c] : 0.
 *   TETRIS_ACT_RANK     (action_pareto / tools.utils.pareto)  rank[c] = 1 + the number of c' with x[c'] > x[c], or x[c'] == x[c]
 *                       and c' < c (scipy.stats.rankdata(n - x, 'ordinal')); the draw below with m[c] = table[rank[c] - 1].
 *                       `table` is a HOST array of 40 float32, read during the call; the reference's pareto with temperature
 *                       theta is table[k] = (k + 1) ** -theta.  It comes from the host so that no powf runs on the device.
 *   TETRIS_ACT_EPSILON  (action_epsilongreedy)  with e = (w1 >> 8) * 2^-24: if e < epsilon then r = w2 & 3, t = w3 mod 10,
 *                       otherwise ARGMAX's choice.
 * The DRAW: w[0..3] = Philox4x32-10 with key (sample_seed, 0) and counter (global game id, low word of `draw`, high word of
 * `draw`, 0) — the function and key layout of the built-in synthetic rollout, global game id = tetris_set_game_offset + i: the
 * stream is reproducible and does not depend on how games are spread over batches.  u = (w0 >> 8) * 2^-24; total = the float32
 * sum of m[0..39] in index order; target = u * total; the choice is the first c whose running sum (the same partial sums) is
 * > target, if there is none the last c with m[c] > 0, and if total is not a positive finite number ARGMAX's choice.  No fused
 * multiply-adds.  Every path ends with 0 <= c < 40 whatever the input bits are.
 * OUTPUTS per game, all optional except d_rot and d_trans:
 *   d_rot, d_trans uint8 [N]   c / 10 and c mod 10; they feed tetris_step_rt_dev unchanged
 *   d_piece  uint8 [N]         the piece index used
 *   d_eval   float32 [N]       x[c] (the reference's a_internal[0])
 *   d_value  float32 [2][N]    from d_state_eval [N][V], V = n_values in {1, 7, 8}, float32 or binary16 (TETRIS_ACT_VALUE_F16):
 *                              [0] = V > 1 ? state_eval[i][min(piece, V - 1)] : state_eval[i][0] (value_piece),
 *                              [1] = the float32 sum of state_eval[i][0..V-1] in index order divided by (float)V (value_mean)
 *   d_entropy float32 [N]      PI only: -sum over c of q log(q + 1e-8), q = x[c] + 1e-6, in float32 with the accurate logf,
 *                              summed in index order.  (The other modes' entropies depend on epsilon or the table alone.)
 * One to four players, every height, colour batches included; not on split batches.  Device pointers (but `table`),
 * asynchronous on the batch's stream, run-ahead bounded and RNG-table requests serviced as for tetris_step_rt_dev_ex.
 * TETRIS_E_ARG: a NULL argument struct, d_action_eval, d_rot or d_trans; n_pieces not 1 or 7; d_state_eval with n_values not
 * 1, 7 or 8, or d_value without d_state_eval; an unknown mode or flag; RANK without a table; d_entropy in another mode than PI;
 * a d_action_eval that is not 16-byte aligned; a split batch.                                                              */
#define TETRIS_ACT_ARGMAX  0
#define TETRIS_ACT_PI      1
#define TETRIS_ACT_RANK    2
#define TETRIS_ACT_EPSILON 3
#define TETRIS_ACT_F16       1   /* d_action_eval is IEEE binary16 instead of float32 */
#define TETRIS_ACT_VALUE_F16 2   /* d_state_eval is IEEE binary16 instead of float32 */
typedef struct tetris_act_eval {
    const void    *d_action_eval;   /* [N][4][10][n_pieces] */
    const void    *d_state_eval;    /* [N][n_values], or NULL */
    int            n_pieces;        /* K */
    int            n_values;        /* V */
    int            mode;            /* TETRIS_ACT_ARGMAX .. TETRIS_ACT_EPSILON */
    int            flags;           /* TETRIS_ACT_F16 | TETRIS_ACT_VALUE_F16 */
    uint32_t       sample_seed;
    uint32_t       reserved;        /* 0 */
    uint64_t       draw;            /* the number of this draw, e.g. the agent's step */
    float          epsilon;
    const float   *table;           /* HOST float32 [40] (RANK), else NULL */
    const uint8_t *d_player;        /* [N] or NULL */
    uint8_t       *d_rot, *d_trans, *d_piece;
    float         *d_eval, *d_value, *d_entropy;
} tetris_act_eval;
/* the choice and its outputs.  The batch's state is not written.                                                          */
int tetris_select_eval_dev(tetris_batch *b, const tetris_act_eval *e);
/* the choice and perform_action of it (tetris_environment.py:102-116) in one call: tetris_select_eval_dev followed by
 * tetris_step_rt_dev_ex, bit for bit.  flags: TETRIS_STEP_AUTO_RESET as there; d_done [N], d_lines / d_dead [P][N] describe the
 * step before the reset (each may be NULL).                                                                               */
int tetris_step_eval_dev(tetris_batch *b, const tetris_act_eval *e, int ms, int flags, uint8_t *d_done, uint8_t *d_lines,
                         uint8_t *d_dead);
/* the same plus the packed observation of the stepped state for d_next_player, as tetris_step_rt_observe_dev gives it (one or
 * two players): the selection kernel followed by that call's launch.  d_obs_piece [P][N] is the observation's piece output. */
int tetris_step_eval_observe_dev(tetris_batch *b, const tetris_act_eval *e, int ms, int flags, uint8_t *d_done,
                                 uint8_t *d_lines, uint8_t *d_dead, const uint8_t *d_next_player, uint8_t *d_visual,
                                 uint8_t *d_vector, uint8_t *d_obs_piece);

/* ---- trajectory windows: recording what an acting call wrote, advantages and value targets on the device ----------------
 * replaces: the worker-side arithmetic between perform_action and the data packet (drl_tetris/worker.py:103-112):
 * store_experience's append to a per-env trajectory, and sventon_trajectory.process_trajectory(compute_advantages=True) with
 * its adv_and_targets (agents/datatypes/trajectory.py:56-86, 111-141) for every game of a batch at once.  With it the actor
 * loop is network forward, tetris_step_eval_observe_dev, tetris_traj_record_dev, and every T steps one
 * tetris_traj_advantages_dev; nothing in it waits for the host.
 * A WINDOW holds T = capacity rows of N games, time-major, in caller-owned device memory (struct tetris_traj below).
 * RECORD writes row `row` of every array from the outputs of a tetris_act_eval `e` that has just been used and from the
 * step's d_done [N] and d_dead [P][N].  With p = e->d_player[i] (NULL: 0; clamped as in the acting calls):
 *   d_action[row][i] = (e->d_rot[i], e->d_trans[i], e->d_piece[i], p)      (the reference's a_environment, and the player)
 *   d_prob[row][i]   = e->d_eval[i]                                         (a_internal[0])
 *   d_value[0][row][i], d_value[1][row][i] = e->d_value[0][i], e->d_value[1][i]; zeros when e->d_value is NULL
 *   d_done[row][i]   = d_done[i]
 *   d_reward[row][i] = tetris_environment.reward_fcn without extra_rewards (tetris_environment.py:135-144): 0 unless
 *                      d_done[i]; else with me = d_dead[p][i] != 0, you = d_dead[1 - p][i] != 0 (one player: you = 0):
 *                      -1 when both, otherwise (float)(you - me).
 * One and two players.  TETRIS_E_ARG: three or four players; a split batch; a row outside [0, T); a NULL e, traj, array of
 * the window, e->d_rot, e->d_trans, e->d_piece, e->d_eval, d_done or d_dead.
 * ADVANTAGES works on rows 0 .. rows-1.  Per game n it walks backward through t, all in float32, in exactly this order of
 * operations, with no fused multiply-adds and with the correctly rounded division:
 *     A1 = A2 = W1 = W2 = 0;  seen_done = 0;  vnext = d_boot ? d_boot[n] : 0
 *     for t = rows-1 .. 0:
 *         if done[t][n]: A1 = A2 = W1 = W2 = 0; seen_done = 1
 *         v0 = value[0][t][n]; v1 = value[1][t][n]
 *         td = (reward[t][n] + (gamma * vnext) * (done[t][n] ? 0 : 1)) - v0
 *         for (A, W, lam) in ((A1, W1, lambda_adv), (A2, W2, lambda_value)):
 *             A = A * (gamma * lam) + td;   W = W * lam + 1;   est = ((A + v0) - v1) / W
 *         adv[t][n] = est1;  target[t][n] = v1 + est2;  closed[t][n] = seen_done
 *         vnext = v0
 * This is adv_and_targets as sventon_trajectory.process_trajectory calls it: the call (trajectory.py:72-80) passes (v_piece,
 * v_mean) into parameters named (v_mean, v_piece) (trajectory.py:111), so the TD errors (trajectory.py:124-126) are built on
 * v(s | piece) = value[0], the estimate (trajectory.py:116-121) is (A + value[0] - value[1]) / W and the target
 * (trajectory.py:138) is mean v + adjustment = value[1] + est2.  The reference runs it once per episode; here the accumulators
 * reset at a done, which applies it to every episode of a column separately.  gamma may be negative (single-policy self-play:
 * sventon_agent_base.py:76); lambda_value is the reference's gve_lambda (default 0.95).  closed[t][n] = 1: the entry's
 * episode ended inside the window, so adv / target are the reference's numbers for it.  For the open tail d_boot [N] is the
 * value the next row's value[0] would have (the usual truncated estimate); with d_boot NULL the tail is what the reference
 * computes for a trajectory that does not end in done.  d_adv, d_target float32 [rows][N] (row stride N), d_closed uint8
 * [rows][N] or NULL.  Any N, any number of players, split batches too: the batch gives N and the stream.
 * TETRIS_E_ARG: a NULL traj, d_value, d_reward or d_done of the window, d_adv or d_target; rows outside [1, T].
 * Both calls: device pointers, asynchronous on the batch's stream; the batch's games are neither read (but the status of
 * being split) nor written.                                                                                                */
typedef struct tetris_traj {
    int      capacity;     /* T */
    int      reserved;     /* 0 */
    uint8_t *d_action;     /* [T][N][4]  r, t, piece, acting player   (a_environment + p) */
    float   *d_prob;       /* [T][N]     the chosen entry x[c]        (a_internal[0])     */
    float   *d_value;      /* [2][T][N]  [0] v(s | piece), [1] mean v(s)  (a_internal[1], [2]) */
    float   *d_reward;     /* [T][N] */
    uint8_t *d_done;       /* [T][N] */
} tetris_traj;
int tetris_traj_record_dev(tetris_batch *b, const tetris_traj *traj, int row, const tetris_act_eval *e, const uint8_t *d_done,
                           const uint8_t *d_dead);
int tetris_traj_advantages_dev(tetris_batch *b, const tetris_traj *traj, int rows, float gamma, float lambda_adv,
                               float lambda_value, const float *d_boot, float *d_adv, float *d_target, uint8_t *d_closed);

/* ---- trajectory windows: the states, the finished entries, a minibatch in the trainer's form ----------------------------
 * replaces: what lies between a processed trajectory and the trainer's model.train(...) arguments —
 * sventon_trajectory.process_trajectory(..., augment=...) with augment_data (agents/datatypes/trajectory.py:56-109),
 * experience_replay.add_samples / retrieve_all (agents/agent_utils/experience_replay.py:96-150) and the permuted minibatch
 * slices of sventon_agent_ppo_trainer.do_training (sventon_agent_ppo_trainer.py:34-62) — for the window's own sample set
 * (no priorities, no k-step views).  Three calls; device pointers, asynchronous on the batch's stream; one and two players.
 * TETRIS_E_ARG for three or four players, split batches and NULLs as for tetris_traj_record_dev.
 *
 * THE PACKED OBSERVATION RECORD (struct tetris_traj_obs): d_obs is uint32 [T][N][S][12], S = number of players, 16-byte
 * aligned: SAMPLE-major, the record of entry (t, n) is 48 S contiguous bytes, slot 0 = the board of d_player[n] at the time,
 * slot 1 = the opponent's (the perspective order of tetris_observe_packed).  Per slot:
 *   words 0..9   occupancy of columns 0..9, bit y = row y (state words 0..9; bits at and above H carry no meaning)
 *   word 10      x | y << 8 | inc_lines << 16 | combo_time << 24       the bytes tetris_observe_packed writes to vector[0..3]
 *   word 11      combo_count | next << 8 | piece << 16                 vector[4]; the index of the one-hot of vector[5..11]
 *                                                                      (7: none); the byte tetris_observe_packed writes to `piece`
 * 48 bytes per player-board against the 213 of the byte planes.  (Sample-major so that a gather touches one or two cache
 * lines per sample; a word-major layout has not been measured against it.)
 * OBSERVE (replaces: keeping trajectory.s, the states state_fcn later unpacks — trajectory.py:24-31, 62) writes row `row`
 * from the batch's current state, which it only reads; d_player [N] or NULL as for tetris_observe_packed_dev.  Colour
 * batches give the same records (occupancy).  In the actor loop: observe(row), tetris_step_eval_observe_dev, record(row).
 * TETRIS_E_ARG: a NULL obs or d_obs, d_obs not 16-byte aligned, row outside [0, T).
 *
 * SELECT (replaces: the choice of the entries that reach the replay, experience_replay.py:96-150, in the order of
 * augment_data's np.concatenate([x, x2]), trajectory.py:102-106): d_mask uint8 [rows][N] (typically d_closed of
 * tetris_traj_advantages_dev; any non-zero byte counts).  d_index int32 [cap] receives the flat indices t N + n of the
 * non-zero entries in ascending order; with TETRIS_SELECT_AUGMENT the same list follows once more with bit 31 set.  d_count
 * int32 [1] receives the length of the full list (k or 2 k) even when it exceeds cap; then the first cap entries are written.
 * Entries past the list, up to cap, are set to -1.  Stable and deterministic; three launches, no workgroup waits for another.
 * TETRIS_E_ARG: NULL d_mask, d_index or d_count; rows < 1; cap < 0; rows N >= 2^31; an unknown flag.
 *
 * BATCH (replaces: state_fcn(self.s, player=self.p[, mirrored=True]) of the chosen entries — state_dict's `aug`,
 * environment/env_utils/state_processors.py:44-53, through unpacker(..., mirrored=True), agents/agent_utils/
 * state_unpack.py:88-105 — augment_data's mirrored action, trajectory.py:88-99, and the trainer's slices): d_index int32 [M],
 * any order, repeats allowed.  Outputs, each NULL to skip it:
 *   d_visual uint8 [S][M][H][10], d_vector uint8 [S][M][12], d_piece uint8 [S][M]     as tetris_observe_packed
 *   d_action uint8 [M][3] (r, t, piece); d_prob, d_adv, d_target, d_reward float32 [M]; d_done, d_valid uint8 [M]
 * (struct tetris_traj_batch).  d_adv_in / d_target_in: float32 [T][N] like the window (row stride N; rows no index names
 * are not read), either may be NULL: zeros.  With e = d_index[j] & 0x7FFFFFFF = t N + n:
 *   bit 31 clear: the bytes tetris_observe_packed gave for that state, the row entry of the window; floats bit for bit.
 *   bit 31 set: the reference's mirrored sample, both slots: field column c is column 9 - c; piece is piece_swap[piece],
 *     piece_swap = (1, 0, 3, 2, 4, 5, 6), 7 stays 7; the seven nextpiece bytes are piece_swap[int(p == next)], that is
 *     1 - one-hot — THE REFERENCE'S QUIRK (state_processors.py:50 indexes piece_swap with the one-hot's values), kept;
 *     x, y, inc_lines, combo_time, combo_count unchanged; action r unchanged, t -> 9 - t, piece -> piece_swap[piece].
 *   e outside [0, T N) — -1 among them: zeros everywhere and d_valid = 0 (else 1).
 * TETRIS_E_ARG: NULL traj, obs, out, d_index, d_obs or d_action / d_prob / d_reward / d_done of the window; capacities of
 * traj and obs that differ; d_obs not 16-byte aligned; M < 0; T N >= 2^31.                                                  */
#define TETRIS_SELECT_AUGMENT 1
typedef struct tetris_traj_obs {
    int       capacity;    /* T */
    int       reserved;    /* 0 */
    uint32_t *d_obs;       /* [T][N][S][12], 16-byte aligned */
} tetris_traj_obs;
typedef struct tetris_traj_batch {
    uint8_t *d_visual;     /* [S][M][H][10] */
    uint8_t *d_vector;     /* [S][M][12] */
    uint8_t *d_piece;      /* [S][M] */
    uint8_t *d_action;     /* [M][3] */
    float   *d_prob;       /* [M] */
    float   *d_adv;        /* [M] */
    float   *d_target;     /* [M] */
    float   *d_reward;     /* [M] */
    uint8_t *d_done;       /* [M] */
    uint8_t *d_valid;      /* [M] */
} tetris_traj_batch;
int tetris_traj_observe_dev(tetris_batch *b, const tetris_traj_obs *obs, int row, const uint8_t *d_player);
int tetris_traj_select_dev(tetris_batch *b, const uint8_t *d_mask, int rows, int flags, int32_t *d_index, long long cap,
                           int32_t *d_count);
int tetris_traj_batch_dev(tetris_batch *b, const tetris_traj *traj, const tetris_traj_obs *obs, const float *d_adv_in,
                          const float *d_target_in, const int32_t *d_index, int M, const tetris_traj_batch *out);

/* ---- trajectory windows of a planning agent: the packed deltas of a step, a minibatch of them in the trainer's form --------
 * replaces: what the planning agent keeps per step and what its trainer reads back — the seven things
 * sherlock_agent.get_action stores (agents/sherlock_agent/sherlock_agent.py:137-146: a_idx, piece, pi(a), v_piece, v_mean,
 * delta(s, a), delta_sum(s)), sherlock_trajectory's add / process_trajectory (agents/datatypes/trajectory.py) and the permuted
 * minibatch slices of sherlock_agent_ppo_trainer.do_training (sherlock_agent_ppo_trainer.py:36-63).  The reference's
 * process_trajectory passes (v_piece, v_mean) into adv_and_targets in the same swapped order as the sventon trajectory and
 * gives the same numbers for the same inputs, so tetris_traj_advantages_dev, tetris_traj_select_dev and tetris_traj_batch_dev
 * serve a planning window unchanged; the two calls here add the two [H][10] planes.  Device pointers, asynchronous on the
 * batch's stream; one and two players; the batch's games are neither read nor written.
 *
 * THE PLAN RECORD (struct tetris_traj_plan): d_rec is uint32 [T][N][112], 16-byte aligned: SAMPLE-major, 448 bytes per entry
 * for every height, against the 1 600 bytes of two float32 planes of a 20-row board.  All column words are masked to rows
 * 0..H-1.  With p, count (clamped into [0, L]) and the list kinds exactly those of tetris_plan_deltas_dev, and choice =
 * e->d_choice[i] clamped into [0, max(count, 1) - 1]:
 *   words 0..9     `before`: the slot-0 column words of obs->d_obs[row][i], i.e. what tetris_traj_observe_dev(row, d_player)
 *                  stored from the state the lists were simulated on (copied, so that the record stands alone)
 *   words 10..19   `after`: the columns of the chosen list, e->d_cols[choice][p][c][i]; zero unless that list is NORMAL
 *   word 20        the chosen list's kind: 0 NORMAL, 1 SMALL, 2 NONE (count = 0)
 *   word 21        n_small | n_normal << 16, counted over the lists k < count
 *   word 22+9c+j   bit-plane j = 0..8 of column c: bit y = bit j of the number of NORMAL lists k < count whose `after` column
 *                  c has bit y set
 * RECORD (replaces: store_experience's append of the seven-tuple, sherlock_agent.py:137-146, worker.py:103-112) writes row
 * `row` of the plan records and of `traj` from a tetris_plan_eval `e` that has just been used and the step's d_done [N] and
 * d_dead [P][N].  The caller's order is tetris_traj_observe_dev(row), simulate / choose / step, then this call.  It re-reads
 * e->d_count and e->d_cols and never e->d_phi, e->d_delta or e->d_sums: a caller that records need not ask the choosing call
 * for the float planes.  The row arrays, as tetris_traj_record_dev writes them:
 *   d_action[row][i] = (choice & 255, 0, e->d_piece[i], p)     a_idx in place of r; byte 1 of a planning row carries no meaning
 *   d_prob[row][i]   = e->d_prob[i]
 *   d_value[0][row][i], d_value[1][row][i] = e->d_value[0][i], e->d_value[1][i]; zeros when e->d_value is NULL
 *   d_done[row][i]   = d_done[i];  d_reward[row][i] as tetris_traj_record_dev
 * With plan NULL only the row arrays are written, obs is not read, and choice is e->d_choice[i] unclamped.
 * TETRIS_E_ARG, and nothing is written: three or four players; a split batch; a row outside [0, T); capacities of traj, plan
 * and obs that differ; a NULL e, traj, array of the window, e->d_choice, e->d_piece, e->d_prob, d_done or d_dead; with a plan
 * also a NULL obs, d_obs, d_rec, e->d_count or e->d_cols, a max_lists outside [1, 256], a d_rec or d_obs that is not 16-byte
 * aligned.
 *
 * BATCH (replaces: the slices delta[idx], delta_sum[idx] of sherlock_agent_ppo_trainer.do_training,
 * sherlock_agent_ppo_trainer.py:36-63): d_index int32 [M] with the meaning it has for tetris_traj_batch_dev, at = d_index[j] &
 * 0x7FFFFFFF = t N + n.  d_delta, d_sums: [M][H][10] float32, or IEEE binary16 (rounded to nearest even) with
 * TETRIS_PLAN_BATCH_F16; 16-byte aligned; either may be NULL.
 *   delta(y, c) = the value tetris_plan_deltas_dev gives a cell of a list of the record's kind whose delta is bit y of
 *                 after[c] minus bit y of before[c] (NORMAL: that delta; SMALL: small_fill; NONE: 0)
 *   sums(y, c)  = (float)(cnt(y, c) - n_normal * bit y of before[c]) + small_fill * (float)n_small, one float32 multiply and
 *                 one float32 add, cnt read out of the nine planes
 * — for a given small_fill the bits tetris_plan_deltas_dev and tetris_select_lists_dev write.
 *   bit 31 set: output column c is taken from the record's column 9 - c (before, after, planes): the image that matches
 *     tetris_traj_batch_dev's mirrored state and swapped piece.  THE REFERENCE HAS NO SUCH SAMPLE: its augment_data unpacks
 *     the seven arrays of this trajectory into two and raises ValueError (trajectory.py:88-109), so process_trajectory(
 *     augment=True) fails for a planning agent.  tetris_traj_batch_dev's mirrored action byte 1 (9 - t) carries no meaning for
 *     a planning row either.
 *   at outside [0, T N) — -1 among them: zeros.
 * M = 0 succeeds and does nothing.  TETRIS_E_ARG: NULL plan, d_rec or d_index; both outputs NULL; M < 0; T N >= 2^31; an
 * unknown flag; a d_rec, d_delta or d_sums that is not 16-byte aligned; three or four players; a split batch.              */
#define TETRIS_PLAN_REC_WORDS 112
typedef struct tetris_traj_plan {
    int       capacity;    /* T */
    int       reserved;    /* 0 */
    uint32_t *d_rec;       /* [T][N][112], 16-byte aligned */
} tetris_traj_plan;
int tetris_traj_record_plan_dev(tetris_batch *b, const tetris_traj *traj, const tetris_traj_plan *plan,
                                const tetris_traj_obs *obs, int row, const tetris_plan_eval *e,
                                const uint8_t *d_done, const uint8_t *d_dead);
#define TETRIS_PLAN_BATCH_F16 1   /* d_delta / d_sums are IEEE binary16 instead of float32 */
int tetris_traj_plan_batch_dev(tetris_batch *b, const tetris_traj_plan *plan, const int32_t *d_index, int M,
                               float small_fill, int flags, void *d_delta, void *d_sums);

/* ---- experience replay: a prioritised ring on the device — add, rank sample, update_prios, k-step gather -----------------
 * replaces: agents/agent_utils/experience_replay.py as sventon_agent_dqn_trainer.do_training drives it
 * (agents/sventon_agent/sventon_agent_dqn_trainer.py:30-100) in its 'rank' sample mode (the only one the reference can run:
 * experience_replay.py:52 reads an undefined name in the other).  Four calls; device pointers, asynchronous on the batch's
 * stream; one and two players; the batch's games are neither read nor written.  TETRIS_E_ARG for three or four players, split
 * batches and NULLs, as for the trajectory windows.
 *
 * THE BUFFER (struct tetris_replay, caller-owned device memory): capacity C is the reference's max_size argument (_max_size),
 * k_step >= 0, max_size = C - k_step with 1 <= max_size <= 2^24 (a rank stays exact as a float32).  Positions are handed out
 * below max_size only; rows max_size .. C-1 are never written (experience_replay.py:17-18, 26-30), so they hold what the
 * caller put there — zeros — and a k-step view near the end reads them, as the reference's does.
 *   d_obs uint32 [C][S][12] the packed observation record of tetris_traj_obs, 16-byte aligned; d_action uint8 [C][4];
 *   d_prob, d_adv, d_target, d_reward float32 [C]; d_done uint8 [C]; d_flags uint8 [C] (bit 0: the mirrored sample);
 *   d_prio float32 [max_size]; d_cursor int32 [4] = current_idx, current_size, samples offered so far modulo 2^32, entries
 *   dropped.  The cursor lives on the device: no call reads it on the host.  The caller zeroes everything once.
 *
 * ADD (replaces: add_samples / add_indices, experience_replay.py:108-138, fed with process_trajectory(augment=...)'s output,
 * trajectory.py:56-109): the entries of d_mask uint8 [rows][N] (typically d_closed; any non-zero byte counts) of the window
 * (traj, obs, d_adv_in, d_target_in float32 [T][N] or NULL: zeros) go in GAME-MAJOR: game 0's entries in ascending t, then game
 * 1's, ...; with TETRIS_SELECT_AUGMENT each game's run is followed directly by the same run with d_flags = 1 (augment_data's
 * [x, x2] per trajectory, trajectory.py:102-106; the record and the action are stored unmirrored, the gather makes the
 * image).  Game-major because k_step_view (fcns.py:4-9) takes the next row for a sample's successor; a run selected by `closed`
 * ends in a done, where compute_targets cuts.  A mask whose runs do not end in a done gives k-step views that run on into the
 * next game's entries, as the reference's views across two trajectories do.  d_prio[pos] = d_prio_in ? d_prio_in[t][n] : 2.0f
 * (the reference's "very large prio", trajectory.py:82); d_flags = 0 for the plain copy.  With k entries in all the
 * reference's rule is applied once: if current_idx + k > max_size then current_size = current_idx, current_idx = 0; positions
 * [current_idx, current_idx + k) are written; current_idx += k; current_size = max(current_size, current_idx); d_cursor[2]
 * += k.  Where k > max_size (the reference raises) the first max_size entries are written, current_idx = max_size and
 * d_cursor[3] += k - max_size.  Three launches, none waits for another workgroup.
 * TETRIS_E_ARG: a NULL rp, traj, obs, d_mask or array of either; the rules of the buffer above; capacities of traj and obs
 * that differ; rows outside [1, T]; rows N >= 2^31; an unknown flag.
 *
 * SAMPLE (replaces: get_random_sample in rank mode, experience_replay.py:42-74).  With n = d_cursor[1], read on the device:
 *   rank_i = 1 + n - ordinal_rank(d_prio[i]), i < n  (1 + n - scipy.stats.rankdata(.., 'ordinal'): the highest priority has
 *            rank 1, among equal priorities the later position the smaller rank; -0.0 equals +0.0; NaN priorities rank
 *            somewhere, unspecified, and no access leaves the arrays whatever the bits)
 *   w_i    = powf((float)rank_i, -alpha)
 *   u_i    = ((philox4x32_10(key (seed, 0), counter (i, draw low, draw high, 0))[0] >> 8) + 1) * 2^-24, in (0, 1], exact
 *   key_i  = (-logf(u_i)) / w_i, the division correctly rounded, nothing contracted; a -0.0 key sorts as 0.0
 * The min(M, n) entries of smallest key go to d_index int32 [M] by ascending key, ties by ascending position; entries past
 * that count are -1 with weight 0; d_count[0] = min(M, n).  This is weighted sampling without replacement by exponential keys
 * (Efraimidis & Spirakis 2006): the distribution of successive draws without replacement with probabilities proportional to
 * w, which is what np.random.choice(replace=False, p=p) draws from; the reference's sequence itself hangs on numpy's global
 * generator.  d_weight[j] = powf((float)rank / (float)n, alpha * beta) with the product rounded once in float32: the
 * reference's is_weights, since ((n p)^-beta) / max(..) = (p_min / p)^beta = (rank / n)^(alpha beta) needs no normalising sum
 * (and neither do the keys: they are invariant under scaling of p).  d_rank int32 [max_size] and d_key float32 [max_size] are
 * optional outputs (NULL to skip), entries i < n: the reference's `rank` and what the selection was made on.
 * TETRIS_E_ARG: NULL rp, d_prio, d_cursor, d_index, d_weight or d_count; the rules of the buffer; M < 0.
 *
 * UPDATE_PRIOS (replaces: update_prios, experience_replay.py:140-141): d_prio[d_index[j]] = d_prio_new[j], j < M, for indices
 * in [0, max_size); others, -1 among them, are skipped.  The indices of one sample call are distinct; with repeats which
 * value lands is unspecified (the reference keeps the last).
 * TETRIS_E_ARG: NULL rp, d_prio, d_index or d_prio_new; the rules of the buffer; M < 0.
 *
 * GATHER (replaces: retrieve_samples_by_idx on the k-step views, experience_replay.py:143-150, fcns.py:4-9, with state_fcn
 * and the mirror of augment_data): 1 <= steps <= k_step + 1; out is a tetris_traj_batch sized for M * steps samples.  Sample
 * j * steps + s is ring position d_index[j] + s: the bytes tetris_traj_batch_dev gives for that record and row entry, mirrored
 * (columns reversed, piece_swap, the `next` quirk, t -> 9 - t) when bit 0 of d_flags there is set.  A d_index[j] outside
 * [0, max_size) gives zeros and d_valid = 0 for all of its `steps` samples.  So d_visual is [S][M][steps][H][10], the
 * trainer's visual_states_k; its [:, :, 0] is un_k_step(x, 0).
 * TETRIS_E_ARG: NULL rp, array of it, d_index or out; the rules of the buffer; M < 0; steps outside [1, k_step + 1];
 * M * steps >= 2^31.                                                                                                       */
typedef struct tetris_replay {
    int       capacity;    /* C */
    int       k_step;
    uint32_t *d_obs;       /* [C][S][12], 16-byte aligned */
    uint8_t  *d_action;    /* [C][4] */
    float    *d_prob;      /* [C] */
    float    *d_adv;       /* [C] */
    float    *d_target;    /* [C] */
    float    *d_reward;    /* [C] */
    uint8_t  *d_done;      /* [C] */
    uint8_t  *d_flags;     /* [C]  bit 0: the mirrored sample */
    float    *d_prio;      /* [C - k_step] */
    int32_t  *d_cursor;    /* [4] */
} tetris_replay;
int tetris_replay_add_dev(tetris_batch *b, const tetris_replay *rp, const tetris_traj *traj, const tetris_traj_obs *obs,
                          const float *d_adv_in, const float *d_target_in, const float *d_prio_in, const uint8_t *d_mask,
                          int rows, int flags);
int tetris_replay_sample_dev(tetris_batch *b, const tetris_replay *rp, int M, float alpha, float beta, uint32_t seed,
                             uint64_t draw, int32_t *d_index, float *d_weight, int32_t *d_count, int32_t *d_rank,
                             float *d_key);
int tetris_replay_update_prios_dev(tetris_batch *b, const tetris_replay *rp, const int32_t *d_index, const float *d_prio_new,
                                   int M);
int tetris_replay_gather_dev(tetris_batch *b, const tetris_replay *rp, const int32_t *d_index, int M, int steps,
                             const tetris_traj_batch *out);
/* GATHER of a list of steps (replaces: value_estimator._filter_inputs on the k-step views, agents/networks/value_estimator.py:
 * 47-49, with the steps of _create_steps, :90-99 — the rows the estimator's net is evaluated on, and no others): bit s of
 * step_mask (0 <= s <= k_step) selects ring position d_index[j] + s; n = popcount(step_mask); out is a tetris_traj_batch sized
 * for M * n samples, and sample j * n + i is the row of the i-th set bit in ascending order.  Everything else is GATHER's: the
 * same kernel, the mirror by the entry's flag, zeros and d_valid = 0 for a d_index[j] outside [0, max_size).
 * step_mask == (1 << steps) - 1 gives the bytes of tetris_replay_gather_dev(.., steps, ..).
 * TETRIS_E_ARG: GATHER's rules; step_mask == 0; a bit above k_step; k_step > 63; M * n >= 2^31.                              */
int tetris_replay_gather_steps_dev(tetris_batch *b, const tetris_replay *rp, const int32_t *d_index, int M, uint64_t step_mask,
                                   const tetris_traj_batch *out);

/* ---- loss heads: a trainer's loss, its statistics and the gradient with respect to the network's outputs ------------------
 * replaces: the non-network arithmetic of the two trainers' create_training_ops — agents/networks/ppo_nets.py:141-196 (with
 * N.action_entropy, network_utils.py:114-118) and agents/networks/prio_qnet.py:102-117 — and autograd's backward through it:
 * from the network's outputs for a minibatch of M samples to the loss, the reference's statistics and d loss / d outputs, which
 * the caller hands to the network's backward.  Not included: the regulariser (a function of the network's variables), the
 * compressors (stateful; the caller applies them to d_adv), the optimiser.
 * Both calls take device pointers, enqueue at most three launches on the batch's stream — a count of the valid samples when
 * d_valid or d_weight is given, the head, the reduction of the statistics — and wait for nothing; the batch's games are neither
 * read nor written, every batch shape serves.  The definitions, operation by operation, are in drl-tetris_amd/csrc/tetris_loss.h;
 * float32 arithmetic, no fused multiply-adds, sums in a fixed order without atomics: a call repeated on the same inputs gives
 * the same bits.
 * COMMON.  K = n_pieces (7 or 1).  d_action uint8 [M][3] = (r, t, piece) as tetris_traj_batch_dev writes it; r, t and piece are
 * limited to 3, 9 and K - 1; c = 10 r + t.  d_valid uint8 [M] or NULL: a sample with d_valid[m] == 0 contributes nothing, and
 * its gradient rows and per-sample outputs are zeros.  D = the number of valid samples; D == 0 gives zeros everywhere (the
 * reference's means over nothing are NaN).  The inputs pi / Q [M][4][10][K] are float32, or binary16 with TETRIS_LOSS_F16; the
 * gradients are float32, or binary16 (rounded to nearest even) with TETRIS_LOSS_GRAD_F16; both 16-byte aligned.  Every entry of
 * a gradient array is written: zeros outside the sample's piece.  grad_scale multiplies every gradient (an AMP loss scale).
 * d_stats float32 [TETRIS_LOSS_STATS]; unused slots are zero.
 * PPO (tetris_ppo_loss).  x_j = d_pi[m][j][k], val = d_v[m][min(k, V - 1)] (V = n_values, 1 or K; binary16 with
 * TETRIS_LOSS_VALUE_F16), e = 1e-6:
 *   p = x_c, ratio = max(p, e) / max(prob_old, e), cl = clip(ratio, 1 - clip, 1 + clip), pl = min(ratio adv, cl adv)
 *   H = -sum_j (x_j + e) log(max(e, x_j + e)), bonus0 = H - entropy_floor_loss relu(entropy_floor - H),
 *   bonus = bonus0 + rescaled_entropy (max_entropy - bonus0)
 *   loss = value_loss mean((val - target)^2) - policy_loss mean(pl) - entropy_loss mean(bonus), means over the D valid samples
 *   entropy_floor and max_entropy are the reference's two constants, computed by the caller in float64 (capi.
 *   ppo_entropy_constants); without "entropy_floor_loss" / "rescaled_entropy" in the reference's params pass 0 for them.
 *   d_grad_pi [M][4][10][K], d_grad_v [M][V]; TensorFlow's tie rules for maximum / minimum / clip.
 *   d_terms float32 [6][M] or NULL: p, ratio, pl, H, bonus, val.
 *   d_stats: 0 D, 1 loss, 2 value loss, 3 policy loss, 4 entropy loss, 5 mean H, 6 mean H^2, 7 mean bonus, 8 mean val,
 *   9 mean val^2, 10 mean target, 11 mean target^2, 12 mean [ratio != cl] (clip_saturation), 13 mean ratio.
 * DQN (tetris_dqn_loss).  q = d_Q[m][r][t][k], w = d_weight[m] (NULL: 1):
 *   d_new_prio float32 [M] = |q - target| (+ optimistic_prios relu(that) when optimistic_prios != 0), 0 for invalid samples:
 *   what tetris_replay_update_prios_dev takes.  loss = sum w (q - target)^2 / Dnz, Dnz = the number of valid samples with
 *   w != 0 (tf.losses.mean_squared_error's default reduction), 0 when Dnz == 0.  d_grad_Q [M][4][10][K].  d_q float32 [M] or NULL.
 *   d_stats: 0 D, 1 Dnz, 2 loss, 3 mean q, 4 mean q^2, 5 mean target, 6 mean target^2, 7 mean new_prio (means over D).
 * TETRIS_E_ARG: a NULL argument struct; M < 0; n_pieces not 1 or 7; n_values not 1 or n_pieces; a NULL d_pi, d_v, d_action,
 * d_prob_old, d_adv, d_target, d_grad_pi, d_grad_v or d_stats (PPO), d_Q, d_action, d_target, d_grad_Q, d_new_prio or d_stats
 * (DQN); clip that is not >= 0; an unknown flag; an input or gradient array that is not 16-byte aligned.  M == 0 zeroes
 * d_stats and does nothing else.                                                                                            */
#define TETRIS_LOSS_STATS     16
#define TETRIS_LOSS_F16       1   /* d_pi / d_Q are IEEE binary16 instead of float32 */
#define TETRIS_LOSS_VALUE_F16 2   /* d_v is IEEE binary16 instead of float32 */
#define TETRIS_LOSS_GRAD_F16  4   /* d_grad_pi, d_grad_v / d_grad_Q are IEEE binary16 instead of float32 */
typedef struct tetris_ppo_loss {
    const void    *d_pi;            /* [M][4][10][n_pieces], 16-byte aligned */
    const void    *d_v;             /* [M][n_values] */
    const uint8_t *d_action;        /* [M][3] */
    const float   *d_prob_old;      /* [M] */
    const float   *d_adv;           /* [M] */
    const float   *d_target;        /* [M] */
    const uint8_t *d_valid;         /* [M] or NULL */
    int            M;
    int            n_pieces;        /* K */
    int            n_values;        /* V */
    int            flags;           /* TETRIS_LOSS_* */
    float          clip;            /* clipping_parameter */
    float          value_loss, policy_loss, entropy_loss;      /* c1, c2, c3 */
    float          entropy_floor_loss, rescaled_entropy;       /* 0: the term is absent */
    float          entropy_floor, max_entropy;
    float          grad_scale;
    float          reserved;        /* 0 */
    void          *d_grad_pi;       /* [M][4][10][n_pieces], 16-byte aligned */
    void          *d_grad_v;        /* [M][n_values] */
    float         *d_terms;         /* [6][M] or NULL */
    float         *d_stats;         /* [TETRIS_LOSS_STATS] */
} tetris_ppo_loss;
typedef struct tetris_dqn_loss {
    const void    *d_Q;             /* [M][4][10][n_pieces], 16-byte aligned */
    const uint8_t *d_action;        /* [M][3] */
    const float   *d_target;        /* [M] */
    const float   *d_weight;        /* [M] or NULL */
    const uint8_t *d_valid;         /* [M] or NULL */
    int            M;
    int            n_pieces;        /* K */
    int            flags;           /* TETRIS_LOSS_F16 | TETRIS_LOSS_GRAD_F16 */
    float          optimistic_prios;
    float          grad_scale;
    float          reserved;        /* 0 */
    void          *d_grad_Q;        /* [M][4][10][n_pieces], 16-byte aligned */
    float         *d_new_prio;      /* [M] */
    float         *d_q;             /* [M] or NULL */
    float         *d_stats;         /* [TETRIS_LOSS_STATS] */
} tetris_dqn_loss;
int tetris_ppo_loss_dev(tetris_batch *b, const tetris_ppo_loss *l);
int tetris_dqn_loss_dev(tetris_batch *b, const tetris_dqn_loss *l);

/* ---- planning loss head: the planning agent's PPO loss, statistics and gradients straight from the plan records ------------
 * replaces: the non-network arithmetic of delta_ppo_nets.create_training_ops (agents/networks/delta_ppo_nets.py:150-182) and
 * autograd's backward through it, for a minibatch of M samples of a planning window.  The two [M][H][10] planes delta and
 * delta_sum are never written: the head reads the 448-byte records of `plan` (tetris_traj_record_plan_dev) through d_index, as
 * tetris_traj_plan_batch_dev does, and every value d_t, s_t below is the one that call gives for the same small_fill
 * (small_fill = 0: the reference's numbers).  Not included, as for the PPO head: the regulariser, the advantage compressor, the
 * k-step target estimator, the optimiser.  Device pointers, at most three launches on the batch's stream (the count of the
 * valid samples, the head, the reduction of the statistics), nothing waits; one and two players; the batch's games are neither
 * read nor written.  The definition, operation by operation, and the order of every sum are in
 * drl-tetris_amd/csrc/tetris_loss.h (PLAN); float32, no fused multiply-adds, logf the only library call, no atomics: a call
 * repeated on the same inputs gives the same bits.
 *   d_phi [M][H][10][K]: the network's RAW second output (_phi_tf before the clip), float32 or binary16 (TETRIS_LOSS_F16),
 *   16-byte aligned; K = n_pieces, 7 or 1; H = the batch's height.  d_v [M][V], V = n_values = 1 or K (TETRIS_LOSS_VALUE_F16).
 *   d_index int32 [M]: entries of the window, bit 31 = the mirrored image; an index that names no entry (-1, >= T N) is an
 *   invalid sample, as is one with d_valid[m] == 0 (d_valid uint8 [M] or NULL).  The piece of sample m is the byte
 *   d_piece[m * piece_stride], limited to K - 1: piece_stride = 1 for a uint8 [M] array, 3 with d_piece = d_action + 2 of
 *   tetris_traj_batch_dev's d_action [M][3].  d_prob_old, d_adv, d_target float32 [M].
 * With e = 1e-6, the cells t = 10 y + c of the HW = 10 H, k the piece, x_t = clip(d_phi[m][y][c][k], e, 1):
 *   probability = (sum x_t d_t + e) / (sum x_t s_t + e), ratio = max(probability, e) / max(prob_old, e),
 *   cl = clip(ratio, 1 - clip, 1 + clip), pl = min(ratio adv, cl adv)
 *   imp = sum x_t (1 - min(1, s_t));  S = sum (s_t + e), y_t = x_t s_t / S + e, Hent = -sum y_t log(max(e, y_t))
 *   val = d_v[m][min(k, V - 1)]
 *   loss = value_loss mean((val - target)^2) - policy_loss mean(pl) + impossibility_loss mean(imp) / HW
 *          - entropy_loss mean(Hent), means over the D valid samples; D == 0 gives zeros everywhere
 *   d_grad_phi [M][H][10][K] and d_grad_v [M][V], float32 or binary16 (TETRIS_LOSS_GRAD_F16), times grad_scale; every element
 *   is written, zeros outside the piece's plane and for invalid samples.  Through the clip the gradient passes where
 *   e <= raw <= 1 (tf.clip_by_value sends a tie to its input); the other ties as for the PPO head.
 *   d_terms float32 [6][M] or NULL: probability, ratio, pl, Hent, imp, val (zeros for invalid samples).
 *   d_stats: 0 D, 1 loss, 2 value loss, 3 policy loss, 4 entropy loss, 5 impossibility loss (2-5 signed as they enter the
 *   loss), 6 mean Hent, 7 mean Hent^2, 8 mean val, 9 mean val^2, 10 mean target, 11 mean target^2, 12 clip_saturation,
 *   13 mean ratio, 14 mean probability.
 * TETRIS_E_ARG: a NULL l, plan, d_rec, d_phi, d_v, d_index, d_piece, d_prob_old, d_adv, d_target, d_grad_phi, d_grad_v or
 * d_stats; M < 0; n_pieces not 1 or 7; n_values not 1 or n_pieces; clip that is not >= 0; piece_stride < 1; an unknown flag; a
 * d_phi, d_grad_phi or d_rec that is not 16-byte aligned; a window of no rows or of 2^31 entries or more; three or four
 * players; a split batch.  M == 0 zeroes d_stats and does nothing else.                                                      */
typedef struct tetris_plan_loss {
    const void    *d_phi;           /* [M][H][10][n_pieces], 16-byte aligned */
    const void    *d_v;             /* [M][n_values] */
    const int32_t *d_index;         /* [M] */
    const uint8_t *d_piece;         /* sample m: d_piece[m * piece_stride] */
    const float   *d_prob_old;      /* [M] */
    const float   *d_adv;           /* [M] */
    const float   *d_target;        /* [M] */
    const uint8_t *d_valid;         /* [M] or NULL */
    int            M;
    int            n_pieces;        /* K */
    int            n_values;        /* V */
    int            flags;           /* TETRIS_LOSS_* */
    int            piece_stride;    /* bytes between two samples' pieces, >= 1 */
    float          small_fill;      /* as tetris_traj_plan_batch_dev's; 0: the reference's planes */
    float          clip;            /* clipping_parameter */
    float          value_loss, policy_loss, entropy_loss, impossibility_loss;      /* c1, c2, c3, c4 */
    float          grad_scale;
    void          *d_grad_phi;      /* [M][H][10][n_pieces], 16-byte aligned */
    void          *d_grad_v;        /* [M][n_values] */
    float         *d_terms;         /* [6][M] or NULL */
    float         *d_stats;         /* [TETRIS_LOSS_STATS] */
} tetris_plan_loss;
int tetris_plan_loss_dev(tetris_batch *b, const tetris_traj_plan *plan, const tetris_plan_loss *l);

/* ---- k-step target estimator: the DQN trainer's target from the reference net's outputs for the k-step views ---------------
 * replaces: model.compute_targets (agents/sventon_agent/sventon_agent_dqn_trainer.py:49-59), which is value_estimator
 * (agents/networks/value_estimator.py:51-88: _create_estimator, k_step_estimate, _aggregate) applied to the net's outputs, with
 * q_to_v (agents/networks/network_utils.py:95-98) for the value of a step.  Not included: the net; time_stamps (the reference
 * asserts it None).  The definition, operation by operation and with the order of every sum, is in
 * drl-tetris_amd/csrc/tetris_kstep.h; float32, no fused multiply-adds, a correctly rounded division, no atomics: a call repeated
 * on the same inputs gives the same bits.  Device pointers, two launches on the batch's stream in Q mode (the values of the
 * M n rows, then a lane per sample), one in V mode; nothing waits; the batch's games are neither read nor written, every batch
 * shape serves.
 *   k = k_step, 1..63.  S = the set bits of step_mask, all within [1, k] (capi.kstep_steps / kstep_mask: _create_steps), n = |S|.
 *   d_out: the net's output for the M n rows of tetris_replay_gather_steps_dev(.., step_mask, ..), row j n + i = step s_i of
 *     sample j.  mode TETRIS_KSTEP_Q: Q [M][n][4][10][K], K = n_pieces (7 or 1), 16-byte aligned; the value of a row is the mean
 *     over the pieces of used_pieces (a 7-bit mask) of the maximum over the 40 (r, t): q_to_v.  mode TETRIS_KSTEP_V: v [M][n][V],
 *     V = n_values = 1 or K — the V stream of a (Q, V, A) net or a PPO net's value —, the same mean for V = K, the value itself
 *     for V = 1.  float32, or binary16 with TETRIS_LOSS_F16 in flags.
 *   Ring mode — d_index int32 [M] and max_size >= 1 given: row t of sample j is element d_index[j] + t of d_reward float32 /
 *     d_done uint8, the ring's own arrays (rp->d_reward, rp->d_done, max_size = rp->capacity - rp->k_step; k_step <= rp->k_step):
 *     reward and done are not gathered at all.  A d_index[j] outside [0, max_size): target 0, done_time 0, values 0.
 *   Array mode — d_index NULL and max_size 0: row t is element j (k + 1) + t of d_reward / d_done [M][k + 1], what
 *     tetris_replay_gather_dev(.., k + 1, ..) wrote.  d_index without max_size or max_size without d_index: TETRIS_E_ARG.
 *   dt = the first row of 0..k with a non-zero done byte, k + 1 without one.  With g_t = (float)pow((double)gamma, t) and
 *   l_s = (float)pow((double)lam, s):  P_0 = 0, P_(t+1) = dt >= t ? P_t + r_t g_t : P_t;  E_s = dt >= s ? P_s + V_s g_s : P_s;
 *   w_s = l_s (with TETRIS_KSTEP_TRUNCATE: 0 where dt < s - 1);  target = (sum_S E_s w_s) / (sum_S w_s), 0 where the weights sum
 *   to 0 (the reference: 0 / 0).
 *   d_target float32 [M]; d_values float32 [M][n] (the V_s) and d_done_time uint8 [M] (dt) or NULL.
 * TETRIS_E_ARG, with nothing written: a NULL a, d_out, d_reward, d_done or d_target; M < 0; M n >= 2^31; k_step outside
 * [1, 63]; step_mask without a bit or with a bit outside [1, k_step]; an unknown mode; n_pieces not 1 or 7; n_values not 1 or
 * n_pieces (V mode); used_pieces empty or with a bit at or above n_pieces; an unknown flag; d_index and max_size not both given
 * or both absent; max_size < 1 in ring mode; a d_out that is not 16-byte aligned (Q mode).  M == 0 succeeds and does nothing. */
#define TETRIS_KSTEP_Q        0
#define TETRIS_KSTEP_V        1
#define TETRIS_KSTEP_TRUNCATE 8   /* flags, beside TETRIS_LOSS_F16: truncate_aggregation */
typedef struct tetris_kstep_target {
    const void    *d_out;           /* Q [M][n][4][10][n_pieces] (16-byte aligned) or v [M][n][n_values] */
    const float   *d_reward;        /* the ring's [capacity], or [M][k_step + 1] */
    const uint8_t *d_done;          /* likewise */
    const int32_t *d_index;         /* [M] (ring mode) or NULL */
    int            M;
    int            k_step;
    uint64_t       step_mask;       /* bits 1 .. k_step */
    int            max_size;        /* ring mode: the ring's capacity - k_step; array mode: 0 */
    int            mode;            /* TETRIS_KSTEP_Q / TETRIS_KSTEP_V */
    int            n_pieces;        /* K */
    int            n_values;        /* V (V mode) */
    int            used_pieces;     /* bit p: piece p counts; 0x7F (K = 7) or 1 (K = 1) for all */
    int            flags;           /* TETRIS_LOSS_F16 | TETRIS_KSTEP_TRUNCATE */
    float          gamma, lam;      /* the reference's gamma and _lambda */
    float         *d_target;        /* [M] */
    float         *d_values;        /* [M][n] or NULL */
    uint8_t       *d_done_time;     /* [M] or NULL */
} tetris_kstep_target;
int tetris_kstep_target_dev(tetris_batch *b, const tetris_kstep_target *a);

/* ---- output heads: from a trunk's raw streams to Q / V / A and to pi / v, with their backward -------------------------------
 * replaces: the output-head arithmetic of the reference's networks and autograd's backward through it.  DQN nets:
 * qva_from_raw_streams (agents/networks/network_utils.py:100-104) as base_architecture.py:53-62 calls it — advantage_range * _A
 * through normalize_advantages (network_utils.py:8-35) in mode "mean" or "max" with the used-piece mask, tanh, Q = _V + A,
 * V = q_to_v(Q).  PPO nets (ppo_nets.py:24-33): pi = action_softmax (network_utils.py:120-125) over the 40 (r, t) of each piece,
 * v = normalize_advantages(_V, tanh, axis=3, inplace=True) of the [M, K + 1] value stream.  Not included: the trunk,
 * keyboard_conv's convolution and its slice / concat (the caller hands over [M][4][10][K]), the input side.  The definition,
 * operation by operation and with the order of every sum, is in drl-tetris_amd/csrc/tetris_head.h; float32, no fused
 * multiply-adds, tanhf and expf the only library calls, no atomics: a call repeated on the same inputs gives the same bits.
 * Device pointers, ONE launch per call on the batch's stream, nothing waits; the batch's games are neither read nor written,
 * every batch shape serves.  The output of a forward call is what tetris_select_eval_dev, tetris_ppo_loss_dev,
 * tetris_dqn_loss_dev and tetris_kstep_target_dev take.
 *   Big arrays — d_a, d_Q, d_A, d_grad_Q, d_grad_a; d_x, d_pi, d_grad_pi, d_grad_x — are [M][4][10][K], K = n_pieces = 7 or 1,
 *   float32, or all of them binary16 with TETRIS_HEAD_F16 (what autograd under AMP hands over), 16-byte aligned.  The per-sample
 *   value arrays — d_v, d_grad_v of the Q head; d_w, d_v, d_grad_v, d_grad_w of the policy head — are float32, or all binary16
 *   with TETRIS_HEAD_VALUE_F16.  Outputs are rounded to nearest even.  Every element of every output is written, nothing past M.
 * Q HEAD (tetris_q_head).  a = advantage_range d_a.  d_v [M][n_values], n_values = 1 or K, or NULL: the reference's constant 0
 *   of full_network=False (prio_qnet); n_values is then not read.  mask_k = bit k of used_pieces, U its popcount; K = 1 takes
 *   used_pieces = 1.  mode TETRIS_HEAD_MEAN: d = a - (sum_k mask_k mean_j a_jk) / U, for every piece, used or not.
 *   TETRIS_HEAD_MAX: lo = the minimum of all 40 K elements; mx_k = the maximum over j of a used piece, lo for an unused one;
 *   separate_piece_values != 0: d_jk = a_jk - mx_k; otherwise d = a - (sum_k mask_k mx_k) / U.  TETRIS_HEAD_NONE: d = a.
 *   A = tanh(d), Q_jk = v[min(k, n_values - 1)] + A_jk, V = (sum_k mask_k max_j Q_jk) / U of the Q that was stored.
 *   tetris_q_head_dev reads d_a, d_v; writes d_Q, d_V float32 [M] and, unless NULL, d_A.
 *   tetris_q_head_grad_dev reads d_a, d_grad_Q (and d_v for its presence only: A is recomputed from d_a); writes d_grad_a and,
 *   when d_v is given, d_grad_v [M][n_values]: the gradient of sum grad_Q Q.  V and A are forward-only: no gradient flows through
 *   them (the reference's trainers differentiate Q only).  Ties of a maximum or of the minimum share the gradient equally
 *   (TensorFlow's reduce_max / reduce_min, torch's amax / amin).
 * POLICY HEAD (tetris_policy_head).  d_x: the logits; d_w [M][n_values], n_values = W = 1 or K + 1.
 *   pi_jk = exp(x_jk - max_j x_jk) / sum_j exp(x_jk - max_j x_jk).  W = 1: v_0 = tanh(w_0).  W = K + 1:
 *   v_(k-1) = tanh(w_0 + (w_k - mean_{k=1..K} w_k)), d_v [M][K] — the mean over all K entries, used or not, as in the reference.
 *   tetris_policy_head_dev reads d_x, d_w; writes d_pi, d_v.  tetris_policy_head_grad_dev reads the stored d_pi, d_v and d_grad_pi,
 *   d_grad_v; writes d_grad_x, d_grad_w [M][W].
 * TETRIS_E_ARG, with nothing written: a NULL argument struct or a NULL array the call reads or writes (d_A and, for the Q head,
 * d_v / d_grad_v may be NULL; d_grad_v is required where d_v is given); M < 1; n_pieces not 1 or 7; n_values not 1 or K (Q head,
 * d_v given), not 1 or K + 1 (policy head); an unknown mode; used_pieces empty or with a bit at or above n_pieces; an unknown
 * flag; a big array that is not 16-byte aligned.                                                                             */
#define TETRIS_HEAD_MEAN      0
#define TETRIS_HEAD_MAX       1
#define TETRIS_HEAD_NONE      2
#define TETRIS_HEAD_F16       1   /* the [M][4][10][K] arrays are IEEE binary16 instead of float32 */
#define TETRIS_HEAD_VALUE_F16 2   /* the per-sample value arrays are IEEE binary16 instead of float32 */
typedef struct tetris_q_head {
    const void    *d_a;             /* [M][4][10][n_pieces], 16-byte aligned */
    const void    *d_v;             /* [M][n_values] or NULL */
    const void    *d_grad_Q;        /* backward: [M][4][10][n_pieces], 16-byte aligned */
    int            M;
    int            n_pieces;        /* K */
    int            n_values;        /* Kv */
    int            mode;            /* TETRIS_HEAD_MEAN / _MAX / _NONE */
    int            separate_piece_values;
    int            used_pieces;     /* bit k: piece k is used; 0x7F (K = 7) or 1 (K = 1) for all */
    int            flags;           /* TETRIS_HEAD_F16 | TETRIS_HEAD_VALUE_F16 */
    float          advantage_range;
    void          *d_Q;             /* forward: [M][4][10][n_pieces], 16-byte aligned */
    float         *d_V;             /* forward: [M] */
    void          *d_A;             /* forward: like d_Q, or NULL */
    void          *d_grad_a;        /* backward: like d_a */
    void          *d_grad_v;        /* backward: [M][n_values], with d_v */
} tetris_q_head;
typedef struct tetris_policy_head {
    const void    *d_x;             /* forward: [M][4][10][n_pieces], 16-byte aligned */
    const void    *d_w;             /* forward: [M][n_values] */
    const void    *d_grad_pi;       /* backward: like d_pi */
    const void    *d_grad_v;        /* backward: like d_v */
    int            M;
    int            n_pieces;        /* K */
    int            n_values;        /* W: 1 or K + 1 */
    int            flags;           /* TETRIS_HEAD_F16 | TETRIS_HEAD_VALUE_F16 */
    void          *d_pi;            /* [M][4][10][n_pieces], 16-byte aligned: written forward, read backward */
    void          *d_v;             /* [M][W == 1 ? 1 : K]: written forward, read backward */
    void          *d_grad_x;        /* backward: like d_x */
    void          *d_grad_w;        /* backward: [M][n_values] */
} tetris_policy_head;
int tetris_q_head_dev(tetris_batch *b, const tetris_q_head *h);
int tetris_q_head_grad_dev(tetris_batch *b, const tetris_q_head *h);
int tetris_policy_head_dev(tetris_batch *b, const tetris_policy_head *h);
int tetris_policy_head_grad_dev(tetris_batch *b, const tetris_policy_head *h);

/* ---- network inputs: the padded plane stack and the float vector of a network's first layer, from packed records ------------
 * replaces: the fixed arithmetic every architecture of the reference does between the uint8 planes of a state and its first
 * learned layer (resblock, resblock_kbd: agents/networks/builders/sventon_architectures.py:25-29; the legacy encoder:
 * legacy_build_blocks.py:31) — the cast to float, apply_visual_pad (agents/networks/network_utils.py:71-77) and visual_stack
 * (network_utils.py:79-93) — taken straight from the 48-byte observation records of a window or of the replay ring: the uint8
 * planes tetris_traj_batch_dev / tetris_replay_gather_dev would write are never written.  Not included: conv_shape_vector's
 * tiling of the vector over the image (a broadcast), every learned layer, bfloat16.  The definition, operation by operation, is
 * in drl-tetris_amd/csrc/tetris_input.h.  Device pointers, ONE launch on the batch's stream, nothing waits, the batch's games are
 * neither read nor written; one and two players.
 * SOURCES (struct tetris_net_input): how sample j of the call finds its record — the rules of the calls named, not restated.
 *   a window's index list   obs, d_index int32 [M]: entry d_index[j] & 0x7FFFFFFF of the window, mirrored with bit 31, no sample
 *                           outside [0, T N) (-1 among them): tetris_traj_batch_dev's.  M samples.
 *   a row of a window       obs, d_index NULL, row in [0, T), M == N: sample j is entry row N + j, game order, not mirrored — the
 *                           actor's form: tetris_traj_observe_dev(obs, row, d_player), then this call.
 *   the replay ring         replay (obs NULL), d_index int32 [M], and step_mask != 0 (tetris_replay_gather_steps_dev's rows,
 *                           n = its popcount) or else steps (tetris_replay_gather_dev's, n = steps): sample j n + i is ring
 *                           position d_index[j] + the i-th row, mirrored by bit 0 of d_flags there, no sample for an index
 *                           outside [0, max_size).  M n samples: every output below has M n in the place of M.
 * OUTPUTS, each NULL to skip it; float32, or binary16 with TETRIS_INPUT_F16, aligned to the element:
 *   d_visual  [S][M][C][Hp][Wp], or [S][M][Hp][Wp][C] with TETRIS_INPUT_CHANNELS_LAST (the reference's NHWC; the memory of a torch
 *             channels_last tensor).  C = 1 + n_items; with TETRIS_INPUT_PAD Hp = H + 2, Wp = 12, without Hp = H, Wp = 10.
 *   d_vector  [S][M][12]: the float of each byte tetris_traj_batch_dev writes to d_vector (the mirrored one-hot quirk kept).
 *   d_piece   uint8 [S][M], d_valid uint8 [M]: as tetris_traj_batch_dev writes them.
 * With f[y][c] the byte tetris_traj_batch_dev gives for the sample (bit y of column c, or of column 9 - c when mirrored; bits
 * at and above H of a record word reach no channel), the image P is, with TETRIS_INPUT_PAD,
 *   P[0][x] = 0 for x in 1..10;  P[y][0] = P[y][11] = 1 for every y in 0..H+1;  P[H+1][x] = 1;  P[1+y][1+c] = f[y][c]
 * (a zero row on top, then ones left, right and below: the second pad covers the first pad's row), and P = f without.  Channel
 * 0 is P; channel 1 + i is items[i], in the caller's order (the reference's `items` list):
 *   TETRIS_INPUT_CUMSUM  cumsum[y][x] = sum over y' <= y of P[y'][x]      TETRIS_INPUT_SHADOW  min(cumsum, 1)
 *   TETRIS_INPUT_HEIGHT  y                                                TETRIS_INPUT_HOLES   shadow - P
 * Every value is an integer in [0, 33]: exact in both element types.  A sample that is no sample is zeros in every output —
 * height and the walls included — and d_valid = 0.  16-byte stores are used where the address allows, narrower ones elsewhere.
 * TETRIS_E_ARG, with nothing written: a NULL argument struct; three or four players; a split batch; obs and replay both
 * given or both NULL; obs: d_obs NULL or not 16-byte aligned, T N outside [1, 2^31); d_index NULL: row outside [0, T) or
 * M != N; M < 0; replay: tetris_replay_gather_dev's rules (tetris_replay_gather_steps_dev's with step_mask != 0), a NULL d_index
 * among them; n_items outside [0, 4]; an item code that is unknown or named twice; an unknown flag; d_visual or d_vector not
 * aligned to the element type.                                                                                                */
#define TETRIS_INPUT_CUMSUM 1
#define TETRIS_INPUT_SHADOW 2
#define TETRIS_INPUT_HEIGHT 3
#define TETRIS_INPUT_HOLES  4
#define TETRIS_INPUT_F16           1   /* d_visual / d_vector are IEEE binary16 instead of float32 */
#define TETRIS_INPUT_CHANNELS_LAST 2   /* d_visual is [S][M][Hp][Wp][C] instead of [S][M][C][Hp][Wp] */
#define TETRIS_INPUT_PAD           4   /* apply_visual_pad: Hp = H + 2, Wp = 12 */
typedef struct tetris_net_input {
    const tetris_traj_obs *obs;        /* a window's records, or NULL with replay */
    const tetris_replay   *replay;     /* the ring, or NULL with obs */
    const int32_t         *d_index;    /* [M]; NULL with obs: the row form */
    int                    row;        /* the row form: [0, T) */
    int                    M;
    int                    steps;      /* the ring, step_mask == 0: [1, k_step + 1] */
    int                    n_items;    /* [0, 4] */
    uint64_t               step_mask;  /* the ring: bit s selects row s; 0: the first `steps` rows */
    int                    items[4];   /* TETRIS_INPUT_CUMSUM / _SHADOW / _HEIGHT / _HOLES, channel order */
    int                    flags;      /* TETRIS_INPUT_F16 | _CHANNELS_LAST | _PAD */
    int                    reserved;   /* 0 */
    void                  *d_visual;   /* [S][M][C][Hp][Wp] or [S][M][Hp][Wp][C] */
    void                  *d_vector;   /* [S][M][12] */
    uint8_t               *d_piece;    /* [S][M] */
    uint8_t               *d_valid;    /* [M] */
} tetris_net_input;
int tetris_net_input_dev(tetris_batch *b, const tetris_net_input *in);

/* ---- keyboard convolution: the network's last learned layer, forward and gradients, on the matrix cores --------------------
 * replaces: keyboard_conv (agents/networks/builders/build_blocks.py:68-83) as resblock_kbd ends in it
 * (agents/networks/builders/sventon_architectures.py:71-73) — tf.layers.conv2d with a "valid" kernel as tall as the image and
 * three columns wide (build_blocks.py:69-78), the n_rot = 4 channel slices and their concat along the rotation axis
 * (build_blocks.py:79-80) — and autograd's backward through it.  Not included: kbd_activation (build_blocks.py:81-82; it stays
 * with tetris_q_head_dev / tetris_policy_head_dev), the residual blocks and every other learned layer, conv_shape_vector and the
 * peephole concats, bfloat16, an image width other than 12, the optimiser and the regulariser.  The definition is in
 * drl-tetris_amd/csrc/tetris_kbd.h.  Device pointers, asynchronous on the batch's stream, nothing waits; the batch's games are
 * neither read nor written, every batch shape serves; the batch's scratch holds the repacked kernel and grad_w's partial sums,
 * so calls on one batch are ordered by its stream.
 *   K = n_pieces in 1..7, O = 4 K, o = r K + k; Hp = height in 4..33 (the padded image's rows), C = channels, a multiple of 32
 *   in 32..512.  d_x [M][Hp][12][C] (NHWC: the memory of a torch channels_last tensor [M, C, Hp, 12]); d_w [Hp][3][C][O] (HWIO,
 *   the reference variable's layout); d_bias float32 [O]; d_out, d_grad_out [M][4][10][K]; d_grad_x like d_x; d_grad_w float32
 *   like d_w; d_grad_b float32 [O].  d_x, d_w, d_out, d_grad_out and d_grad_x are float32, or all binary16 with TETRIS_KBD_F16.
 *     out[m][r][t][k]    = bias[o] + sum_h sum_d sum_c x[m][h][t + d][c] w[h][d][c][o]                 d in 0..2, t in 0..9
 *     grad_x[m][h][j][c] = sum over d with 0 <= j - d <= 9, sum_o grad_out[m][r][j - d][k] w[h][d][c][o]
 *     grad_w[h][d][c][o] = sum_m sum_t x[m][h][t + d][c] grad_out[m][r][t][k];   grad_b[o] = sum_m sum_t grad_out[m][r][t][k]
 *   Products and sums in float32, one rounding to nearest even on the way out; the order of the sums is the matrix unit's and is
 *   not specified; no atomics: a call repeated on the same inputs gives the same bytes.  Every element of every output is
 *   written, nothing past it.
 *   tetris_kbd_conv_dev reads d_x, d_w, d_bias; writes d_out.  tetris_kbd_conv_grad_x_dev reads d_grad_out, d_w; writes d_grad_x.
 *   tetris_kbd_conv_grad_w_dev reads d_x, d_grad_out; writes d_grad_w and d_grad_b.  Arrays a call neither reads nor writes may
 *   be NULL.
 * TETRIS_E_ARG, with nothing written: a NULL argument struct or a NULL array the call reads or writes; M < 1; n_pieces outside
 * [1, 7]; height outside [4, 33]; channels no multiple of 32 or outside [32, 512]; an unknown flag; an array of the call that is
 * not 16-byte aligned; an output of the call that overlaps one of its inputs.                                                  */
#define TETRIS_KBD_F16 1   /* d_x, d_w, d_out, d_grad_out and d_grad_x are IEEE binary16 instead of float32 */
typedef struct tetris_kbd_conv {
    const void    *d_x;             /* [M][height][12][channels], 16-byte aligned */
    const void    *d_w;             /* [height][3][channels][4 n_pieces], 16-byte aligned */
    const float   *d_bias;          /* [4 n_pieces], 16-byte aligned */
    const void    *d_grad_out;      /* backward: [M][4][10][n_pieces], 16-byte aligned */
    int            M;
    int            n_pieces;        /* K: 1..7 */
    int            height;          /* Hp: 4..33 */
    int            channels;        /* C: a multiple of 32 in 32..512 */
    int            flags;           /* TETRIS_KBD_F16 */
    int            reserved;        /* 0 */
    void          *d_out;           /* forward: [M][4][10][n_pieces], 16-byte aligned */
    void          *d_grad_x;        /* like d_x */
    float         *d_grad_w;        /* like d_w, float32 */
    float         *d_grad_b;        /* [4 n_pieces] */
} tetris_kbd_conv;
int tetris_kbd_conv_dev(tetris_batch *b, const tetris_kbd_conv *k);
int tetris_kbd_conv_grad_x_dev(tetris_batch *b, const tetris_kbd_conv *k);
int tetris_kbd_conv_grad_w_dev(tetris_batch *b, const tetris_kbd_conv *k);

/* ---- residual layer: one layer of the trunk — 3 x 3 'same' convolution, peephole join, ELU — forward and gradients, on the
 * matrix cores -----------------------------------------------------------------------------------------------------------------
 * replaces: one layer of residual_block (agents/networks/builders/build_blocks.py:8-64) — tf.layers.conv2d(3 x 3, 'same'),
 * peephole_join(x, y, mode = "add" | "truncate_add") (agents/networks/network_utils.py:52-64), elu — and autograd's backward
 * through it.  Not included: normalization = "layer", dropout and pools, strides and filter sizes other than 3 x 3, the 5 x 5
 * pooled value stream, conv_shape_vector and the concat in front of the second block, bfloat16, an image width other than 12,
 * fusing consecutive layers, the optimiser.  The definition is in drl-tetris_amd/csrc/tetris_res.h.  Device pointers, asynchronous
 * on the batch's stream, nothing waits; the batch's games are neither read nor written, every batch shape serves; the batch's
 * scratch holds the repacked kernel and grad_w's partial sums, so calls on one batch are ordered by its stream.
 *   Hp = height in 4..33, 12 columns; Ci = in_channels, a multiple of 8 in 8..512; Co = out_channels, a multiple of 32 in 32..512;
 *   Cout = Co (TETRIS_RES_JOIN_NONE), max(Ci, Co) (_ADD), min(Ci, Co) (_TRUNCATE_ADD).  d_x, d_grad_x [M][Hp][12][Ci] (NHWC: the
 *   memory of a torch channels_last tensor [M, Ci, Hp, 12]); d_w [3][3][Ci][Co] (HWIO, the reference variable's layout); d_bias
 *   float32 [Co]; d_out, d_y, d_grad_out [M][Hp][12][Cout], d_y being d_out as the forward wrote it; d_grad_w float32 like d_w;
 *   d_grad_b float32 [Co].  d_x, d_w, d_out, d_y, d_grad_out and d_grad_x are float32, or all binary16 with TETRIS_RES_F16.
 *     z[m][h][j][o] = bias[o] + sum_(a, b in 0..2) sum_ci x[m][h + a - 1][j + b - 1][ci] w[a][b][ci][o]      x = 0 outside the image
 *     p[c]   = (c < Co ? z[c] : 0) + (join != NONE and c < Ci ? x[m][h][j][c] : 0);   out[c] = ELU ? (p > 0 ? p : expm1f(p)) : p
 *     e[c]   = round(grad_out[c] (ELU and y[c] <= 0 ? y[c] + 1 : 1)) to the element type;   gz[o] = o < min(Co, Cout) ? e[o] : 0
 *     grad_x[m][h][j][ci] = sum_(a, b) sum_o gz[m][h - a + 1][j - b + 1][o] w[a][b][ci][o] + (join != NONE and ci < Cout ? e[ci] : 0)
 *     grad_w[a][b][ci][o] = sum_m sum_h sum_j x[m][h + a - 1][j + b - 1][ci] gz[m][h][j][o];   grad_b[o] = sum_m sum_h sum_j gz[m][h][j][o]
 *   Products and sums in float32, p unrounded into the activation, one rounding to nearest even on the way out; the order of the
 *   sums is the matrix unit's and is not specified; no atomics: a call repeated on the same inputs gives the same bytes.  Every
 *   element of every output is written, nothing past it; the zero border is never a read.
 *   tetris_res_layer_dev reads d_x, d_w, d_bias; writes d_out.  tetris_res_layer_grad_x_dev reads d_grad_out, d_w and, with ELU,
 *   d_y; writes d_grad_x.  tetris_res_layer_grad_w_dev reads d_x, d_grad_out and, with ELU, d_y; writes d_grad_w and d_grad_b.
 *   Arrays a call neither reads nor writes may be NULL.
 * TETRIS_E_ARG, with nothing written: a NULL argument struct or a NULL array the call reads or writes; M < 1; height outside
 * [4, 33]; in_channels no multiple of 8 or outside [8, 512]; out_channels no multiple of 32 or outside [32, 512]; an unknown join,
 * activation or flag; an array of the call that is not 16-byte aligned; an output of the call that overlaps one of its inputs.   */
#define TETRIS_RES_F16 1   /* d_x, d_w, d_out, d_y, d_grad_out and d_grad_x are IEEE binary16 instead of float32 */
#define TETRIS_RES_JOIN_NONE 0
#define TETRIS_RES_JOIN_ADD 1
#define TETRIS_RES_JOIN_TRUNCATE_ADD 2
#define TETRIS_RES_ACT_NONE 0
#define TETRIS_RES_ACT_ELU 1
typedef struct tetris_res_layer {
    const void    *d_x;             /* [M][height][12][in_channels], 16-byte aligned */
    const void    *d_w;             /* [3][3][in_channels][out_channels], 16-byte aligned */
    const float   *d_bias;          /* [out_channels], 16-byte aligned */
    const void    *d_y;             /* backward with ELU: the forward's d_out, 16-byte aligned */
    const void    *d_grad_out;      /* backward: like d_out, 16-byte aligned */
    int            M;
    int            height;          /* Hp: 4..33 */
    int            in_channels;     /* Ci: a multiple of 8 in 8..512 */
    int            out_channels;    /* Co: a multiple of 32 in 32..512 */
    int            join;            /* TETRIS_RES_JOIN_* */
    int            activation;      /* TETRIS_RES_ACT_* */
    int            flags;           /* TETRIS_RES_F16 */
    int            reserved;        /* 0 */
    void          *d_out;           /* forward: [M][height][12][Cout], 16-byte aligned */
    void          *d_grad_x;        /* like d_x */
    float         *d_grad_w;        /* like d_w, float32 */
    float         *d_grad_b;        /* [out_channels] */
} tetris_res_layer;
int tetris_res_layer_dev(tetris_batch *b, const tetris_res_layer *r);
int tetris_res_layer_grad_x_dev(tetris_batch *b, const tetris_res_layer *r);
int tetris_res_layer_grad_w_dev(tetris_batch *b, const tetris_res_layer *r);

/* Built-in synthetic rollout = the worker loop of drl_tetris/worker.py:91-118 with a random policy
 * (SURVEY.md §8d): per env-step  Philox4x32-10(policy_seed; game, step) -> (r = w0 & 3,
 * t = w1 mod 10), acting player = step mod P, perform_action, auto-reset of finished games with
 * seed16 = (12345 + 7919 game + 104729 episode) mod 65536.  Runs `launches` kernel launches of
 * `steps_per_launch` env-steps each on all N games (state stays in registers inside a launch).
 * counters[4] += {env_steps, episodes, lines_cleared, garbage_lines_sent}.  elapsed_ms (optional)
 * = HIP-event time from before the first to after the last launch on the batch's stream.
 * COUNTERS.  Every game keeps four cumulative uint32 words (tetris_rollout_game_totals_dev), which
 * count modulo 2^32.  `counters[k] +=` is exactly what THIS call did, whatever the words held
 * before it: the call keeps a copy of the words, and afterwards sums (after - before) mod 2^32 per
 * game into 64 bits — outside the timed region.  That holds as long as no single game counts
 * 2^32 within the one call.  `step` is 64 bits wide everywhere (policy draw, acting player =
 * step mod P of the 64-bit step); a global game id is 32 bits (tetris_set_game_offset).          */
int tetris_rollout_random(tetris_batch *b, int launches, int steps_per_launch, uint32_t policy_seed,
                          uint64_t first_step, int ms, uint64_t counters[4], float *elapsed_ms);
/* The launches of tetris_rollout_random alone: nothing but the `launches` step kernels lies between the two HIP events
 * and between call and return (plus one final stream synchronisation) — the region bench.py times.  Counters are read
 * with tetris_rollout_totals before and after, outside that region (exact while no per-game word wraps in between: see
 * tetris_rollout_totals).  A chained call numbers its launches with epochs below 0x7FFF0000 and restarts the numbering at a
 * drained point before it would get there; a single chained call of 0x7FFF0000 launches or more cannot be numbered and is
 * refused with TETRIS_E_ARG before anything is enqueued.                                                             */
int tetris_rollout_launch(tetris_batch *b, int launches, int steps_per_launch, uint32_t policy_seed,
                          uint64_t first_step, int ms, float *elapsed_ms);

/* Chained launches of the built-in rollout (default on; single-player batches with one or more steps per launch, two-player
 * batches with one step per launch, on the batch's own stream): a game's step E depends only on the same game's step E - 1,
 * so consecutive launches rotate over three streams and are ordered per WAVE — the games of a wave wait, inside the kernel,
 * for an epoch word that the same wave of the previous launch publishes after its state stores have drained — instead of per
 * launch by the stream (where every launch waits for the slowest wave of the whole previous launch plus the kernel boundary).
 * Results are bit-identical.
 * CHAINING PRESUMES THAT THE DEVICE'S WAVE SLOTS ARE THIS BATCH'S TO USE.  A wave that waits keeps its slot; launches are
 * therefore chained only while three of them — for larger batches two, over two streams — fit on the device together, and that
 * fit is computed as if nothing else ran on the GPU: kernels of the host application (a policy network on another stream), of
 * another process or of a second copy of this library take slots the computation does not know of, and can keep a launch from
 * being resident beside its successor.  No wave waits unboundedly: after `polls` polls of its epoch word (default 2^22, about
 * 2 s; tetris_set_chain_spin_limit, or TETRIS_CHAIN_SPIN_LIMIT in the environment when the batch is created) it gives up and
 * leaves its games untouched, as do the same waves of the launches behind it.  The call then waits for its streams, steps the
 * games that were left behind to the end of the call with the un-chained kernel, and returns TETRIS_OK with the same results;
 * tetris_take_errors reports TETRIS_ERR_CHAIN_FELL_BACK once, and chained launches stay off for the batch until
 * tetris_set_chained(b, 1).  On a GPU that the batch shares with other work, switch chaining off up front:
 * tetris_set_chained(b, 0) — or TETRIS_NO_CHAIN=1 — costs 5.7 us per launch instead of 4.0 and cannot starve anything.
 * The three chain streams belong to the device and are shared by all its batches (their chained calls exclude each other).
 * Side effect a host application may notice: where the device offers three stream priority levels, the three streams are created
 * with three different priorities (that is how the HIP runtime is made to keep them on three hardware queues, where alone they
 * overlap); the batch's own stream has the default priority.
 * on = 0: every launch on the batch's one stream.                                                                       */
int tetris_set_chained(tetris_batch *b, int on);
/* DIRECT DISPATCH of long chained calls.  A chained launch takes the GPU 4 us; hipLaunchKernel costs the calling thread 2.4-4.2 us
 * of it, depending on the process.  Calls of at least `min_launches` launches (default 16) therefore do not go through
 * hipLaunchKernel: the library writes their AQL packets itself, into three HSA user-mode queues of its own per GPU (created on the
 * first such call; shared by the device's batches, whose chained calls exclude each other anyway): 0.2-0.5 us of host time per
 * launch, no helper threads, 1.5-2 % shorter calls.  Same kernels, same machine code (the gfx950 code object is taken from this
 * library's own fat binary and loaded through the HSA loader), same hand-over protocol, same results; a queue's launches are
 * ordered like a stream's (barrier bit), its first packet acquires at system scope.  Such a call first waits for what the batch's
 * stream still holds and returns with its launches retired, like every chained call.  A queue that has been idle takes 10 us to
 * start its first wave, as a stream does: in a 20-launch call the two paths are level (one player) or the queues 5-8 % ahead (two
 * players); calls of a handful of launches stay on the streams (profiles/r03/direct_dispatch.txt).  If the queues cannot be set up (no HSA agent for the HIP device, no host-visible device
 * memory for the kernel arguments, code object not found), the batch keeps launching through its streams.
 * min_launches = 0: never; n > 0: calls of at least n launches; < 0: the default (TETRIS_DIRECT_MIN in the environment, else 16;
 * TETRIS_DIRECT=0: batches are created with 0).  Pre-queued calls (TETRIS_PREQUEUE) go through the streams.              */
int tetris_set_direct_dispatch(tetris_batch *b, int min_launches);
/* 0 if the batch's last tetris_rollout_launch / tetris_rollout_random went through streams, 1 if through those queues, 2 if through
 * them with the XCD-affine kernel (below)                                                                                */
int tetris_rollout_was_direct(tetris_batch *b);
/* XCD-AFFINE chained launches (default on; one-player batches, direct dispatch only).  The MI355X has eight XCDs, each with an L2 of
 * its own that is coherent for its own CUs only; a queue deals a launch's workgroups round-robin over the XCDs, from a start of
 * its own.  With the plain hand-over a game's state therefore crosses the fabric twice per step (written through by one XCD, read
 * by another).  In the affine form the workgroup that finds itself on XCD x (hardware register XCC_ID) takes the game block
 * (b & ~7) | x: a game is stepped on the same XCD in every launch, its state and epoch word stay in that XCD's L2 (plain stores,
 * L1-bypassing loads), and the packets between a queue's first and last carry no cache maintenance; the last one releases at
 * system scope, so memory is current when the call returns.  3.5-3.6 us per launch instead of 4.0 at 64k boards, same results.
 * Relied on: one XCD's L2 is coherent for that XCD's CUs.  Checked, not relied on: that the eight workgroups of a group of eight
 * sit on eight different XCDs — the queues' start XCDs are measured when the queues are made, the form is used only if every
 * queue dealt 1024 workgroups round-robin twice, and in every launch every workgroup compares its XCC_ID with what that
 * measurement predicts; one that is elsewhere touches nothing, its games look abandoned to the next launch, and the call ends
 * like any chained call whose waves gave up (finished un-chained, exact, TETRIS_ERR_CHAIN_FELL_BACK) with this form off for
 * the batch from then on.  on = 0: the plain hand-over.  TETRIS_AFFINE=0 in the environment: batches are created with it off. */
int tetris_set_xcd_affine(tetris_batch *b, int on);
/* TEST AID for the check above: `skew` (0..7) is added to the start XCDs the kernels are told                              */
int tetris_debug_xcd_skew(tetris_batch *b, int skew);
/* TEST AID for the draw limit (TETRIS_ERR_STREAM; nothing in the product calls it): the real limit needs all 64 chunks of the RNG
 * tables, 2.6 GB.  From this call on the kernels of THIS batch are told min(resident chunks, chunks) * 624 draws per episode, and a
 * request to extend the tables is answered only while they have fewer than `chunks` chunks — what happens at 64 without it.
 * chunks = 1..64; 0 restores 64.  The tables themselves (shared by the batches of a device with the same piece map) and
 * tetris_table_chunks are not affected; other batches see all of them.  Synchronises.                                       */
int tetris_debug_table_limit(tetris_batch *b, int chunks);
/* TEST AID (needs no GPU): the gfx950 code objects direct dispatch would load — found in this library's own fat binary —: their
 * number and total size in bytes.  0 objects = direct dispatch cannot work with this build (e.g. a compressed offload bundle).  */
int tetris_debug_code_objects(int *count, uint64_t *bytes);
/* polls of its predecessor's epoch word after which a waiting wave of a chained launch gives up (0 = the default, 2^22);
 * one poll is an agent-scope load and a short sleep, about 0.5 us.                                                     */
int tetris_set_chain_spin_limit(tetris_batch *b, uint32_t polls);
/* MEASUREMENT AID: the GPU's shader clock of the moment in kHz (a 50 us probe kernel on the batch's stream; synchronous).      */
int tetris_debug_clock_khz(tetris_batch *b, int *khz);
/* TEST AID for the give-up path above (nothing in the product calls it): enqueues a kernel that idles for `microseconds` —
 * which = 0..2: on that one of the three chain streams (and of the device's own queues, see tetris_set_direct_dispatch), so the
 * launches the next rollout call puts there start late;
 * which = 3: on the batch's stream; which = -1: on a stream of its own, as workgroups that hold `percent` % of the device's
 * wave slots meanwhile (a co-tenant).  Asynchronous.                                                                   */
int tetris_debug_stall(tetris_batch *b, int which, int microseconds, int percent);
/* TEST AID, nothing in the product calls it: the epoch numbering of chained launches (tetris_set_chained).  A chained call gives
 * its launches consecutive epoch numbers, continuing where the batch's last chained call stopped, and restarts them from 0 (every
 * wave's epoch word cleared on the batch's stream) when the call's last number would reach 0x7FFF0000 — after about two hours of
 * back-to-back launches.  set_epoch >= 0: at a drained point (the batch's stream and the chain streams are synchronised), make
 * the batch look as if `set_epoch` chained launches had already run: every wave's epoch word and the batch's count become
 * `set_epoch`; TETRIS_E_ARG for set_epoch >= 0x7FFF0000.  set_epoch < 0: nothing is changed.  *epoch (optional) = the batch's count
 * afterwards: after a call of L launches that restarted it reads L, after one that did not, the count before the call + L.
 * Synchronises.                                                                                                         */
int tetris_debug_chain_epoch(tetris_batch *b, long long set_epoch, uint32_t *epoch);
/* Environment variables read by the library (measurement aids; none changes a result):
 *   TETRIS_NO_CHAIN=1   batches are created with chained launches off (tetris_set_chained)
 *   TETRIS_NO_DUO=1     two-player single steps through k_game<2> (both players of a game in one lane) instead of k_duo
 *   TETRIS_GRAPH=1      un-chained rollout launches are replayed from HIP graphs of 128 kernel nodes (under rocprofv3 a plain
 *                       launch costs the host more than the kernel takes; from a graph the profiled kernels are back to back)
 *   TETRIS_PREQUEUE=1   (read per call) tetris_rollout_launch of <= 600 chained launches parks its streams behind a blocker kernel
 *                       that runs until the host has queued every launch of the call (it then sets a flag word in pinned memory):
 *                       the GPU-paced launch period, without the host's launch cost
 *   TETRIS_CHAIN_SPIN_LIMIT=<polls>  default of tetris_set_chain_spin_limit for batches created afterwards
 *   TETRIS_CHAIN_DEPTH=1..3  at most that many chained launches in flight; 1 = the chained kernel on one stream, i.e. dispatches
 *                       serialised by the stream (what per-dispatch PMC counters need: profiles/pmc_summary.py)
 *   TETRIS_DIRECT=0     batches are created with direct dispatch off; TETRIS_DIRECT_MIN=<n>: its default threshold
 *                       (tetris_set_direct_dispatch)
 *   TETRIS_AFFINE=0     no XCD-affine launches (tetris_set_xcd_affine)
 *   TETRIS_DIRECT_UNDER_TOOLS=1  direct dispatch also with a profiling tool library in the process (ROCP_TOOL_LIBRARIES, HSA_TOOLS_LIB or
 *                       LD_PRELOAD naming rocprof* / roctracer: by default the launches then stay on the streams)
 *   TETRIS_TIMING=1     tetris_rollout_launch prints its host-side costs (enqueue per launch, gate waits, until drained) to stderr */
/* 1 if tetris_rollout_launch / tetris_rollout_random would chain launches of `steps_per_launch` steps on this batch, 0 if not
 * (switched off — by the caller or by a fall-back —, caller-owned stream, split or colour batch, or not even two launches fit
 * on the device together: a waiting wave keeps its slot, so chaining is only used where it cannot keep the launch it waits
 * for from being dispatched).                                                                                            */
int tetris_rollout_is_chained(tetris_batch *b, int steps_per_launch);

/* Global id of this batch's game 0 (default 0): the built-in rollout keys its policy and its
 * reset-seed schedule by global game id, so that N batches on N GPUs simulate N*n_games distinct
 * games (the reference's equivalent: N worker containers, docker-compose.yaml:27).
 * A global game id is 32 bits: the call keeps the LOW 32 BITS of first_game_id, and the id of
 * game i is (first_game_id + i) mod 2^32 — the ids may wrap inside a batch.                      */
int tetris_set_game_offset(tetris_batch *b, uint64_t first_game_id);

/* ---- split mode: the two players of a game on different GPUs (BASELINE config 5) ------------------------------
 * A split batch holds ONE side (player index `side`, 0 or 1) of n_games two-player games; the batch holding the
 * other side is normally on another GPU and created with the same seeds.  A step is three stages with one 32-bit
 * exchange word per board after each; the caller moves the words (RCCL all-gather in drl-tetris_amd/distributed.py).
 * replaces: PythonHandle::distributeLines + the winner logic across players (PythonHandle.cpp:124-136,151-187).
 *   stage 0: key interpreter for the acting side ([8]*r+[2]+[3]*t+[7]) + loop 1 (side 1 speculatively) -> words A
 *   stage 1: delayCheck of my player.  Side 0 runs it after the A exchange, side 1 after player 0's B words arrived
 *   stage 2: lines arriving after my tick, winner / round_over -> done[n], lines[n], dead[n] (any may be NULL)
 *   stage 3: stage 2 of this step and stage 0 of the NEXT step in one launch (one pass over the state instead of two): for
 *            loops that know the next action when a step ends — d_rot / d_trans / d_acting are the next step's, d_done /
 *            d_lines / d_dead describe the step that ends, d_out receives the next step's A words.  A step of such a loop
 *            is two launches (stage 1, stage 3) and three exchanges.
 * d_words: HOST array of four device pointers to uint32 [n] — my A words, the opponent's A words, player 0's B words,
 * player 1's B words (entries a stage does not read may be NULL): the words a stage wrote (d_out) and the rows an
 * all-gather delivered are read where they lie, nothing is copied in between.  d_out [n]: this stage's words (stages 0, 1, 3).
 * All data pointers are device pointers; everything is enqueued on the batch's stream.  tetris_reset() on a split
 * batch applies the two-player winner rule.  A capacity error (TETRIS_ERR_*) on one side ends the round on BOTH sides in the
 * same step (a bit of the B words); the bit is on the board that has it, and tetris_take_errors of that side's batch reports it.
 * Why three exchanges and not two: within one step the reference's order makes player 0's tick depend on player 1's loop-1
 * words (A), player 1's tick on player 0's tick words (B0), and `done` on player 1's tick words (B1) — three messages that
 * depend on each other.  Folding B1 into the next step's A exchange would need a second speculative shadow state on side 0
 * (it would play the next key list before knowing whether the round had ended) and deliver `done` one step late.      */
int tetris_create_split(tetris_batch **out, int n_games, int side, int height, int width,
                        const uint8_t piece_map[7], int device, const int16_t *seeds);
int tetris_split_stage_dev(tetris_batch *b, int stage, const uint8_t *d_rot, const uint8_t *d_trans,
                           const uint8_t *d_acting, int ms, const uint32_t *const d_words[4], uint32_t *d_out,
                           uint8_t *d_done, uint8_t *d_lines, uint8_t *d_dead);
/* One stage of a split-mode step of the built-in synthetic rollout (same policy and reset-seed schedule as
 * tetris_rollout_random, keyed by global game id and `step`; acting player = step mod 2): stage 0 draws the action on
 * the device, stage 2 counts and auto-resets finished games — identically on both sides, so no host round trip is
 * needed inside a rollout; stage 3 = stage 2 of `step` + stage 0 of `step + 1`.  d_words / d_out as for
 * tetris_split_stage_dev.                                                                                           */
int tetris_split_rollout_stage_dev(tetris_batch *b, int stage, uint32_t policy_seed, uint64_t step, int ms,
                                   const uint32_t *const d_words[4], uint32_t *d_out);
/* cumulative counters of the built-in rollouts of this batch: totals[4] = {env_steps, episodes, lines_cleared,
 * garbage_sent}, each the sum over the games of a per-game word the step kernels keep (env_steps is COUNTED on the
 * device, one increment per game and step, not computed from the launch arguments); synchronous.
 * The per-game words are uint32 and cumulative MODULO 2^32; totals[k] is the sum of those words AS THEY STAND.  The
 * difference of two readings is therefore what happened in between only while no game's word wrapped in between (a
 * wrap takes 2^32 off); tetris_rollout_random / tetris_rollout_policy take the difference per game modulo 2^32 instead. */
int tetris_rollout_totals(tetris_batch *b, uint64_t totals[4]);

/* Run the batch on a caller-owned HIP stream (e.g. torch's current stream) so that its kernels are ordered with the
 * caller's copies and collectives without host synchronisation.  external != 0: use `hip_stream` as given — NULL is
 * then the legacy default stream, which is what torch.cuda.current_stream() usually is; external == 0: back to the
 * batch's own stream (hip_stream ignored).                                                                        */
int tetris_set_stream(tetris_batch *b, void *hip_stream, int external);

/* HIP-event stopwatch on the batch's stream, for timing sequences of _dev calls: start records an event, stop records
 * another, waits for it and returns the milliseconds in between.                                                    */
int tetris_timer_start(tetris_batch *b);
int tetris_timer_stop(tetris_batch *b, float *elapsed_ms);

/* plumbing for zero-copy callers (torch / another HIP library)                                   */
void *tetris_device_state(tetris_batch *b);            /* uint32 [NWORDS][P][N]                  */
void *tetris_stream(tetris_batch *b);                  /* hipStream_t                            */
int   tetris_layout_words(void);                       /* NWORDS                                 */
int   tetris_table_chunks(const tetris_batch *b);      /* RNG-table chunks currently resident    */

#ifdef __cplusplus
}
#endif
#endif
