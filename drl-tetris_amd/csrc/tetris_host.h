// The host-side rules of the C ABI (include/tetris_hip.h) that do not depend on where memory lives or how work is launched: the
// argument checks of the entry points, the filling of the kernels' argument structs, the repacking of host arrays, the mapping
// of flag words to TETRIS_ERR_* bits, and the thread's last error.  No HIP in here.  tetris_hip.hip (hipcc) and
// tests/cpu_harness/harness.cpp (g++, the CPU build of the same kernel bodies) both include it (and tetris_lib_compose.h), so the CPU
// suite runs the lines that ship.  Nothing here needs either side's tetris_batch: a HostShape says what the rules ask of a batch.
//
// The builders fill everything of an argument struct except its embedded KArgs `a`, or take it as `base`: the caller makes it
// with its own base_args, the product after its run-ahead gate (the gate may have extended the RNG tables).
#pragma once
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "tetris_kernels.h"
#include "tetris_plan.h"
#include "tetris_policy.h"
#include "tetris_act.h"
#include "tetris_choose.h"
#include "tetris_traj.h"
#include "tetris_batch.h"
#include "tetris_replay.h"
#include "tetris_plan_traj.h"
#include "tetris_loss.h"
#include "tetris_kstep.h"
#include "tetris_head.h"
#include "tetris_input.h"
#include "tetris_kbd.h"
#include "tetris_res.h"

namespace te {

struct HostShape { int N, P, H, nw, split, tint; };

// ---------------------------------------------------------------- the thread's last error (tetris_last_error)
static thread_local std::string g_err;
static inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
static inline const char* last_error() { return g_err.c_str(); }

static const char* const PACKED_ONE_OR_TWO = "the packed observation is defined for one or two players (own / opponent's board: state_unpack.py:88-137)";
static inline int not_on_split(const HostShape& s, const char* what) {
    if (s.split) return fail(TETRIS_E_ARG, std::string(what) + " is not available on split batches");
    return TETRIS_OK;
}

// Runtime value -> template argument.  with_value<LO, HI>(v, f) calls f(std::integral_constant<int, v>) when LO <= v <= HI and
// returns whether it did; with_flag(v, f) calls f(std::true_type or std::false_type); with_shape<LO, HI>(P, flag, f) calls
// f(P, FLAG) with both.  f is a generic lambda that names its kernel or body with them (k_game<P(), MODE, TINT()>).  In the
// product the bounds decide which instantiations a translation unit holds: player counts 1..2 of k_game, k_plan_* and
// k_policy_step live in tetris_hip.hip, 3..4 in tetris_hip_multi.hip.
template <int LO, int HI, class F>
static bool with_value(int v, F&& f) {
    if constexpr (LO > HI) return false;
    else if (v == LO) { f(std::integral_constant<int, LO>{}); return true; }
    else return with_value<LO + 1, HI>(v, f);
}
template <class F>
static void with_flag(bool v, F&& f) { if (v) f(std::true_type{}); else f(std::false_type{}); }
template <int LO, int HI, class F>
static bool with_shape(int P, bool flag, F&& f) {
    return with_value<LO, HI>(P, [&](auto p) { with_flag(flag, [&](auto t) { f(p, t); }); });
}

// ---------------------------------------------------------------- create, game indices, players
// tetris_create (flags 0, side 0), tetris_create_ex (side 0), tetris_create_split (n_players 1, flags 0); *out = NULL from the
// first check of create_impl on
template <class B>
static inline int create_check(B** out, int n_games, int n_players, int height, int width, const uint8_t piece_map[7], int split, int side, int flags) {
    if (flags & ~TETRIS_FLAG_COLOURS) return fail(TETRIS_E_ARG, "unknown flag");
    if (side != 0 && side != 1) return fail(TETRIS_E_ARG, "side must be 0 or 1");
    if (!out) return fail(TETRIS_E_ARG, "out is NULL");
    *out = nullptr;
    if (n_games < 1) return fail(TETRIS_E_ARG, "n_games must be >= 1");
    if (n_players < 1 || n_players > TETRIS_MAX_PLAYERS) return fail(TETRIS_E_ARG, "n_players must be 1..4");
    if (n_players > 2 && split) return fail(TETRIS_E_ARG, "split batches are two-player games");
    if ((long long)n_games * n_players > (1ll << 23))       // the state allocation stays below 4 GiB (32-bit buffer offsets): 8M boards x 69 words
        return fail(TETRIS_E_ARG, "n_games * n_players must be <= 2^23");
    if (height < 4 || height > MAX_H) return fail(TETRIS_E_ARG, "height must be in [4, 31]");
    if (width != NCOL) return fail(TETRIS_E_ARG, "width must be 10 (the reference hard-codes 10, gamePlay.cpp:202)");
    if (!piece_map) return fail(TETRIS_E_ARG, "piece_map is NULL");
    for (int i = 0; i < 7; i++)
        if (piece_map[i] > 6) return fail(TETRIS_E_ARG, "piece_map entries must be 0..6");
    return TETRIS_OK;
}

// n games, the first n (`indexed` false) or those an index list names
static inline int check_count(const HostShape& s, bool indexed, int n) {
    if (n < 0 || (!indexed && n > s.N)) return fail(TETRIS_E_ARG, "n out of range");
    return TETRIS_OK;
}
static inline int check_idx(const HostShape& s, const int32_t* idx, int n) {
    int rc = check_count(s, idx != nullptr, n);
    if (rc) return rc;
    for (int i = 0; idx && i < n; i++)
        if (idx[i] < 0 || idx[i] >= s.N) return fail(TETRIS_E_ARG, "game index out of range");
    return TETRIS_OK;
}
// every player index < P (player NULL: nothing to check)
static inline int check_players(const HostShape& s, const uint8_t* player, int n) {
    for (int i = 0; player && i < n; i++)
        if (player[i] >= s.P) return fail(TETRIS_E_ARG, "player index out of range");
    return TETRIS_OK;
}

// ---------------------------------------------------------------- key lists in, lines / dead out
static inline int keys_check(const uint8_t* keys, const uint8_t* lens, int max_keys) {
    if (!keys || !lens || max_keys < 1) return fail(TETRIS_E_ARG, "keys/lens/max_keys");
    return TETRIS_OK;
}
// host keys [n][P][K] -> hk [K][P][n]; host lens [n][P] -> hl [P][n]
static inline int keys_pack(const HostShape& s, int n, const uint8_t* keys, const uint8_t* lens, int max_keys, uint8_t* hk, uint8_t* hl) {
    const int P = s.P;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < P; p++) {
            const int len = lens[(size_t)i * P + p];
            if (len > max_keys) return fail(TETRIS_E_ARG, "lens[i][p] > max_keys");
            hl[(size_t)p * n + i] = (uint8_t)len;
        }
    // [n][P][K] -> [K][P][n], blocked over games so that reads stay in L1 and every write run is contiguous
    // (the naive order writes with a stride of n bytes: 52 ms instead of ~2 ms for 64k two-player games)
    const int BLK = 512;
    for (int i0 = 0; i0 < n; i0 += BLK) {
        const int i1 = i0 + BLK < n ? i0 + BLK : n;
        for (int k = 0; k < max_keys; k++)
            for (int p = 0; p < P; p++) {
                uint8_t* dst = hk + ((size_t)k * P + p) * n;
                const uint8_t* src = keys + (size_t)p * max_keys + k;
                for (int i = i0; i < i1; i++) dst[i] = src[(size_t)i * P * max_keys];
            }
    }
    return TETRIS_OK;
}
// a step's lines / dead [P][n] -> the caller's [n][P] (each may be NULL)
static inline void lines_dead_unpack(const HostShape& s, int n, const uint8_t* hl, const uint8_t* hd, uint8_t* lines, uint8_t* dead) {
    const int P = s.P;
    for (int i = 0; i < n; i++)
        for (int p = 0; p < P; p++) {
            if (lines) lines[(size_t)i * P + p] = hl[(size_t)p * n + i];
            if (dead) dead[(size_t)i * P + p] = hd[(size_t)p * n + i];
        }
}

// ---------------------------------------------------------------- tetris_get_actions
static inline int get_actions_check(const HostShape& s, bool indexed, int n, const uint8_t* player, const uint8_t* keys, const uint8_t* lens,
                                    const int32_t* count, int max_lists, int max_keys) {
    if (!keys || !lens || !count || max_lists < 1 || max_keys < 1 || max_keys > 255) return fail(TETRIS_E_ARG, "keys/lens/count/max_*");
    int rc = check_count(s, indexed, n);
    if (rc) return rc;
    return check_players(s, player, n);
}
// The lists of m games as k_actions left them — hc [m * 40] lists per (rotation, x) start, hl their lengths and hk their keys,
// PLAN_LANE_LISTS per start — into the caller's keys [m][max_lists][max_keys], lens [m][max_lists] and count [m]: x-major,
// rotation-minor, as the reference enumerates.  A game with more than max_lists lists: its count is written, then the error.
static inline int get_actions_gather(int m, const uint8_t* hc, const uint8_t* hl, const uint8_t* hk, int max_lists, int max_keys, uint8_t* keys,
                                     uint8_t* lens, int32_t* count) {
    const size_t L = PLAN_LANE_LISTS;
    for (int i = 0; i < m; i++) {
        int total = 0;
        bool over = false;
        for (int xi = 0; xi < 10; xi++)
            for (int r = 0; r < 4; r++) {
                const size_t lane = (size_t)i * 40 + r * 10 + xi;
                for (int k = 0; k < hc[lane]; k++) {
                    if (total >= max_lists) { over = true; break; }
                    const int len = hl[lane * L + k];
                    lens[(size_t)i * max_lists + total] = (uint8_t)len;
                    memcpy(keys + ((size_t)i * max_lists + total) * max_keys, hk + (lane * L + k) * max_keys, (size_t)len);
                    total++;
                }
            }
        count[i] = total;
        if (over) return fail(TETRIS_E_ARG, "more than max_lists key lists for one game");
    }
    return TETRIS_OK;
}

// ---------------------------------------------------------------- steps, resets, observations on the device
// tetris_step_rt_dev_ex (and tetris_step_rt: flags 0)
static inline int step_rt_check(const HostShape& s, const uint8_t* rot, const uint8_t* trans, int flags) {
    if (!rot || !trans) return fail(TETRIS_E_ARG, "rot/trans are NULL");
    if (flags & ~TETRIS_STEP_AUTO_RESET) return fail(TETRIS_E_ARG, "unknown flag");
    if ((flags & TETRIS_STEP_AUTO_RESET) && s.split) return fail(TETRIS_E_ARG, "auto-reset is not available on split batches");
    return TETRIS_OK;
}
static inline int step_rt_observe_check(const HostShape& s, const uint8_t* rot, const uint8_t* trans, int flags, const uint8_t* visual,
                                        const uint8_t* vector, const uint8_t* piece) {
    if (!rot || !trans) return fail(TETRIS_E_ARG, "rot/trans are NULL");
    if (!visual || !vector || !piece) return fail(TETRIS_E_ARG, "visual/vector/piece are NULL");
    if (flags & ~TETRIS_STEP_AUTO_RESET) return fail(TETRIS_E_ARG, "unknown flag");
    if (s.split) return fail(TETRIS_E_ARG, "tetris_step_rt_observe_dev is not available on split batches");
    if (s.P > 2) return fail(TETRIS_E_ARG, PACKED_ONE_OR_TWO);
    return TETRIS_OK;
}
static inline int observe_packed_outputs_check(const uint8_t* visual, const uint8_t* vector, const uint8_t* piece) {
    if (!visual || !vector || !piece) return fail(TETRIS_E_ARG, "visual/vector/piece are NULL");
    return TETRIS_OK;
}
static inline int observe_packed_check(const HostShape& s, bool indexed, int n, const uint8_t* visual, const uint8_t* vector, const uint8_t* piece) {
    int rc = observe_packed_outputs_check(visual, vector, piece);
    if (rc) return rc;
    if (s.P > 2) return fail(TETRIS_E_ARG, PACKED_ONE_OR_TWO);
    return check_count(s, indexed, n);
}
static inline int enumerate_check(const HostShape& s, bool indexed, int n, const void* valid, const void* land_y, const void* cleared, const void* after,
                                  int flags) {
    if (!valid || !land_y || !cleared) return fail(TETRIS_E_ARG, "valid/land_y/cleared are NULL");
    int rc = check_count(s, indexed, n);
    if (rc) return rc;
    if (flags & ~TETRIS_ENUM_PLANAR) return fail(TETRIS_E_ARG, "unknown flag");
    if ((flags & TETRIS_ENUM_PLANAR) && ((((uintptr_t)valid | (uintptr_t)land_y | (uintptr_t)cleared) & 3u) || ((uintptr_t)after & 15u)))
        return fail(TETRIS_E_ARG, "planar outputs: valid / land_y / cleared must be 4-byte aligned, after 16-byte aligned");
    return TETRIS_OK;
}

// ---------------------------------------------------------------- planning (tetris_plan.h)
static inline int action_lists_check(const HostShape& s, const int32_t* count, const uint8_t* lens, const uint8_t* keys, int max_lists, int max_keys,
                                     int flags) {
    int rc = not_on_split(s, "tetris_action_lists_dev");
    if (rc) return rc;
    if (!count || !lens || !keys) return fail(TETRIS_E_ARG, "count/lens/keys are NULL");
    if (max_lists < 1 || max_keys < 1 || max_keys > 254) return fail(TETRIS_E_ARG, "max_lists >= 1, 1 <= max_keys <= 254");
    if (flags & ~TETRIS_LISTS_KEEP_NULL) return fail(TETRIS_E_ARG, "unknown flag");
    return TETRIS_OK;
}
static inline int simulate_lists_check(const HostShape& s, const int32_t* count, const uint8_t* lens, const uint8_t* keys, int max_lists, int max_keys,
                                       int flags, const uint32_t* cols) {
    int rc = not_on_split(s, "tetris_simulate_lists_dev");
    if (rc) return rc;
    if (!count || !lens || !keys || !cols) return fail(TETRIS_E_ARG, "count/lens/keys/cols are NULL");
    if (max_lists < 1 || max_lists > 65535 || max_keys < 1 || max_keys > 255) return fail(TETRIS_E_ARG, "1 <= max_lists <= 65535, 1 <= max_keys <= 255");
    if (flags & ~TETRIS_SIM_FINALIZE) return fail(TETRIS_E_ARG, "unknown flag");
    return TETRIS_OK;
}
static inline int step_lists_check(const HostShape& s, const int32_t* choice, const int32_t* count, const uint8_t* lens, const uint8_t* keys,
                                   int max_lists, int max_keys, int flags) {
    int rc = not_on_split(s, "tetris_step_lists_dev");
    if (rc) return rc;
    if (!choice || !count || !lens || !keys) return fail(TETRIS_E_ARG, "choice/count/lens/keys are NULL");
    if (max_lists < 1 || max_keys < 1 || max_keys > 255) return fail(TETRIS_E_ARG, "max_lists >= 1, 1 <= max_keys <= 255");
    if (flags & ~TETRIS_STEP_AUTO_RESET) return fail(TETRIS_E_ARG, "unknown flag");
    return TETRIS_OK;
}
static inline PlanArgs plan_args(const KArgs& base, const uint8_t* d_player, const int32_t* d_count, const uint8_t* d_lens, const uint8_t* d_keys,
                                 int max_lists, int max_keys, int ms) {
    PlanArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.a = base;
    pa.a.ms = ms;
    pa.player = d_player; pa.count = d_count; pa.lens = d_lens; pa.keys = d_keys;
    pa.max_lists = max_lists; pa.max_keys = max_keys;
    return pa;
}
// tetris_plan_deltas_dev: the checks, then the kernel arguments (a game's lists are the threads of one workgroup of k_plan_deltas)
constexpr int PLAN_DELTAS_MAX_LISTS = 256;
static inline int plan_deltas_args(const HostShape& s, const Geo& geo, const uint8_t* d_player, const int32_t* d_count, const uint32_t* d_cols,
                                   int max_lists, float small_fill, int flags, void* d_deltas, void* d_sums, uint8_t* d_small, PlanDeltaArgs& da) {
    int rc = not_on_split(s, "tetris_plan_deltas_dev");
    if (rc) return rc;
    if (!d_count || !d_cols || !d_deltas) return fail(TETRIS_E_ARG, "count/cols/deltas are NULL");
    if (max_lists < 1 || max_lists > PLAN_DELTAS_MAX_LISTS) return fail(TETRIS_E_ARG, "1 <= max_lists <= 256");
    if (flags & ~(TETRIS_DELTAS_F16 | TETRIS_DELTAS_LIST_MAJOR)) return fail(TETRIS_E_ARG, "unknown flag");
    if ((((uintptr_t)d_deltas) | ((uintptr_t)d_sums)) & 15u) return fail(TETRIS_E_ARG, "deltas / sums must be 16-byte aligned");
    if (((uintptr_t)d_cols) & 3u) return fail(TETRIS_E_ARG, "cols must be 4-byte aligned");
    memset(&da, 0, sizeof da);
    da.geo = geo;
    da.H = s.H; da.n = s.N;
    da.player = d_player; da.count = d_count; da.cols = d_cols;
    da.max_lists = max_lists; da.small_fill = small_fill;
    da.deltas = d_deltas; da.sums = d_sums; da.small = d_small;
    return TETRIS_OK;
}

// ---------------------------------------------------------------- heuristic policy (tetris_policy.h)
// the five calls: not on split batches, `missing` pointers (reported as `missing_text`), flags of the step
static inline int policy_check(const HostShape& s, const char* what, bool missing, const char* missing_text, int flags = 0) {
    int rc = not_on_split(s, what);
    if (rc) return rc;
    if (missing) return fail(TETRIS_E_ARG, missing_text);
    if (flags & ~TETRIS_STEP_AUTO_RESET) return fail(TETRIS_E_ARG, "unknown flag");
    return TETRIS_OK;
}
static inline int rollout_policy_check(const HostShape& s, const int16_t* d_weights, int launches, int steps_per_launch) {
    int rc = policy_check(s, "tetris_rollout_policy", !d_weights, "weights is NULL");
    if (rc) return rc;
    if (launches < 1 || steps_per_launch < 1 || steps_per_launch > 256) return fail(TETRIS_E_ARG, "launches must be >= 1, 1 <= steps_per_launch <= 256");
    return TETRIS_OK;
}
static inline PolicyArgs policy_args(const KArgs& base, const uint8_t* d_player, const int16_t* d_weights, int per_game, int ms, int32_t* d_scores) {
    PolicyArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.a = base;
    pa.a.ms = ms; pa.a.steps = 1;
    pa.player = d_player; pa.weights = d_weights; pa.per_game = per_game ? 1 : 0;
    pa.fixed_player = -1;
    pa.scores = d_scores;
    return pa;
}

// ---------------------------------------------------------------- acting on a network's evaluation (tetris_act.h)
// the argument checks, then the kernel arguments (all but aa.a)
static inline int act_args(const HostShape& s, const tetris_act_eval* e, const char* what, ActArgs& aa) {
    if (!e) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    int rc = not_on_split(s, what);
    if (rc) return rc;
    if (!e->d_action_eval || !e->d_rot || !e->d_trans) return fail(TETRIS_E_ARG, "action_eval/rot/trans are NULL");
    if (e->n_pieces != 1 && e->n_pieces != 7) return fail(TETRIS_E_ARG, "n_pieces must be 1 or 7");
    if (e->d_state_eval && e->n_values != 1 && e->n_values != 7 && e->n_values != 8) return fail(TETRIS_E_ARG, "n_values must be 1, 7 or 8");
    if (e->d_value && !e->d_state_eval) return fail(TETRIS_E_ARG, "value needs state_eval");
    if (e->mode < TETRIS_ACT_ARGMAX || e->mode > TETRIS_ACT_EPSILON) return fail(TETRIS_E_ARG, "unknown mode");
    if (e->flags & ~(TETRIS_ACT_F16 | TETRIS_ACT_VALUE_F16)) return fail(TETRIS_E_ARG, "unknown flag");
    if (e->mode == TETRIS_ACT_RANK && !e->table) return fail(TETRIS_E_ARG, "the RANK mode needs a table");
    if (e->d_entropy && e->mode != TETRIS_ACT_PI) return fail(TETRIS_E_ARG, "entropy is an output of the PI mode");
    if (((uintptr_t)e->d_action_eval) & 15u) return fail(TETRIS_E_ARG, "action_eval must be 16-byte aligned");
    memset(&aa, 0, sizeof aa);
    aa.player = e->d_player;
    aa.action_eval = e->d_action_eval; aa.state_eval = e->d_state_eval;
    aa.K = e->n_pieces; aa.V = e->d_state_eval ? e->n_values : 1;
    aa.eval_f16 = (e->flags & TETRIS_ACT_F16) ? 1 : 0; aa.value_f16 = (e->flags & TETRIS_ACT_VALUE_F16) ? 1 : 0;
    aa.mode = e->mode;
    aa.seed = e->sample_seed; aa.draw_lo = (uint32_t)e->draw; aa.draw_hi = (uint32_t)(e->draw >> 32);
    aa.epsilon = e->epsilon;
    if (e->mode == TETRIS_ACT_RANK) memcpy(aa.table, e->table, sizeof aa.table);
    aa.rot = e->d_rot; aa.trans = e->d_trans; aa.piece = e->d_piece;
    aa.eval = e->d_eval; aa.value = e->d_value; aa.entropy = e->d_entropy;
    return TETRIS_OK;
}
static inline int step_eval_check(int flags) {
    if (flags & ~TETRIS_STEP_AUTO_RESET) return fail(TETRIS_E_ARG, "unknown flag");
    return TETRIS_OK;
}
static inline int step_eval_observe_check(const HostShape& s, int flags, const uint8_t* visual, const uint8_t* vector, const uint8_t* piece) {
    int rc = observe_packed_outputs_check(visual, vector, piece);
    if (rc || (rc = step_eval_check(flags))) return rc;
    if (s.P > 2) return fail(TETRIS_E_ARG, PACKED_ONE_OR_TWO);
    return TETRIS_OK;
}

// ---------------------------------------------------------------- choosing a planning agent's list from phi (tetris_choose.h)
// the argument checks, then the kernel arguments (all but ca.a)
static inline int plan_choose_args(const HostShape& s, const tetris_plan_eval* e, const char* what, PlanChooseArgs& ca) {
    if (!e) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    int rc = not_on_split(s, what);
    if (rc) return rc;
    if (!e->d_phi || !e->d_count || !e->d_cols || !e->d_choice) return fail(TETRIS_E_ARG, "phi/count/cols/choice are NULL");
    if (e->n_pieces != 1 && e->n_pieces != 7) return fail(TETRIS_E_ARG, "n_pieces must be 1 or 7");
    if (e->d_state_eval && e->n_values != 1 && e->n_values != 7 && e->n_values != 8) return fail(TETRIS_E_ARG, "n_values must be 1, 7 or 8");
    if (e->d_value && !e->d_state_eval) return fail(TETRIS_E_ARG, "value needs state_eval");
    if (e->mode != TETRIS_ACT_ARGMAX && e->mode != TETRIS_ACT_PI) return fail(TETRIS_E_ARG, "unknown mode (argmax or pi)");
    if (e->flags & ~(TETRIS_ACT_F16 | TETRIS_ACT_VALUE_F16 | TETRIS_PLAN_OUT_F16)) return fail(TETRIS_E_ARG, "unknown flag");
    if (e->d_entropy && e->mode != TETRIS_ACT_PI) return fail(TETRIS_E_ARG, "entropy is an output of the PI mode");
    if (e->max_lists < 1 || e->max_lists > CHOOSE_MAX_LISTS) return fail(TETRIS_E_ARG, "1 <= max_lists <= 256");
    if ((((uintptr_t)e->d_phi) | ((uintptr_t)e->d_delta) | ((uintptr_t)e->d_sums)) & 15u) return fail(TETRIS_E_ARG, "phi / delta / sums must be 16-byte aligned");
    if (((uintptr_t)e->d_cols) & 3u) return fail(TETRIS_E_ARG, "cols must be 4-byte aligned");
    memset(&ca, 0, sizeof ca);
    ca.player = e->d_player; ca.count = e->d_count; ca.cols = e->d_cols;
    ca.max_lists = e->max_lists; ca.small_fill = e->small_fill;
    ca.phi = e->d_phi; ca.state_eval = e->d_state_eval;
    ca.K = e->n_pieces; ca.V = e->d_state_eval ? e->n_values : 1;
    ca.phi_f16 = (e->flags & TETRIS_ACT_F16) ? 1 : 0; ca.value_f16 = (e->flags & TETRIS_ACT_VALUE_F16) ? 1 : 0;
    ca.out_f16 = (e->flags & TETRIS_PLAN_OUT_F16) ? 1 : 0;
    ca.mode = e->mode;
    ca.seed = e->sample_seed; ca.draw_lo = (uint32_t)e->draw; ca.draw_hi = (uint32_t)(e->draw >> 32);
    ca.choice = e->d_choice; ca.piece = e->d_piece; ca.prob = e->d_prob; ca.probs = e->d_probs;
    ca.value = e->d_value; ca.entropy = e->d_entropy; ca.delta = e->d_delta; ca.sums = e->d_sums;
    return TETRIS_OK;
}
// tetris_step_lists_eval_dev: both halves' rules before the first half runs
static inline int step_lists_eval_check(const HostShape& s, const tetris_plan_eval* e, const uint8_t* d_lens, const uint8_t* d_keys, int max_keys,
                                        int flags) {
    PlanChooseArgs ca;
    int rc = plan_choose_args(s, e, "tetris_step_lists_eval_dev", ca);
    if (rc) return rc;
    return step_lists_check(s, e->d_choice, e->d_count, d_lens, d_keys, e->max_lists, max_keys, flags);
}

// ---------------------------------------------------------------- trajectory windows (tetris_traj.h)
// the argument checks, then the kernel arguments
static inline int traj_record_args(const HostShape& s, const tetris_traj* traj, int row, const tetris_act_eval* e, const uint8_t* d_done,
                                   const uint8_t* d_dead, TrajRecordArgs& ra) {
    if (!traj || !e) return fail(TETRIS_E_ARG, "the window or the argument struct is NULL");
    int rc = not_on_split(s, "tetris_traj_record_dev");
    if (rc) return rc;
    if (s.P > 2) return fail(TETRIS_E_ARG, "the reward is defined for one or two players (tetris_environment.py:135-144)");
    if (!traj->d_action || !traj->d_prob || !traj->d_value || !traj->d_reward || !traj->d_done) return fail(TETRIS_E_ARG, "an array of the window is NULL");
    if (row < 0 || row >= traj->capacity) return fail(TETRIS_E_ARG, "row outside the window");
    if (!e->d_rot || !e->d_trans || !e->d_piece || !e->d_eval) return fail(TETRIS_E_ARG, "rot/trans/piece/eval of the acting call are NULL");
    if (!d_done || !d_dead) return fail(TETRIS_E_ARG, "done/dead are NULL");
    const size_t n = (size_t)s.N, at = (size_t)row * n;
    ra.n = s.N; ra.n_players = s.P;
    ra.rot = e->d_rot; ra.trans = e->d_trans; ra.piece = e->d_piece; ra.player = e->d_player;
    ra.eval = e->d_eval; ra.value = e->d_value;
    ra.done = d_done; ra.dead = d_dead;
    ra.action = traj->d_action + at * 4; ra.prob = traj->d_prob + at;
    ra.value0 = traj->d_value + at; ra.value1 = traj->d_value + (size_t)traj->capacity * n + at;
    ra.reward = traj->d_reward + at; ra.done_out = traj->d_done + at;
    return TETRIS_OK;
}

static inline int traj_adv_args(const HostShape& s, const tetris_traj* traj, int rows, float gamma, float lambda_adv, float lambda_value,
                                const float* d_boot, float* d_adv, float* d_target, uint8_t* d_closed, TrajAdvArgs& aa) {
    if (!traj) return fail(TETRIS_E_ARG, "the window is NULL");
    if (!traj->d_value || !traj->d_reward || !traj->d_done) return fail(TETRIS_E_ARG, "value/reward/done of the window are NULL");
    if (!d_adv || !d_target) return fail(TETRIS_E_ARG, "adv/target are NULL");
    if (rows < 1 || rows > traj->capacity) return fail(TETRIS_E_ARG, "rows outside [1, capacity]");
    aa.n = s.N; aa.rows = rows;
    aa.plane = (size_t)traj->capacity * (size_t)s.N;
    aa.value = traj->d_value; aa.reward = traj->d_reward; aa.done = traj->d_done; aa.boot = d_boot;
    aa.gamma = gamma; aa.lambda_adv = lambda_adv; aa.lambda_value = lambda_value;
    aa.adv = d_adv; aa.target = d_target; aa.closed = d_closed;
    return TETRIS_OK;
}

// ---------------------------------------------------------------- a window's states and sample sets (tetris_batch.h)
// the checks the three calls share: the rules of tetris_traj_record_dev
static inline int traj_batch_rules(const HostShape& s, const char* what) {
    int rc = not_on_split(s, what);
    if (rc) return rc;
    if (s.P > 2) return fail(TETRIS_E_ARG, PACKED_ONE_OR_TWO);
    return TETRIS_OK;
}

static inline int traj_obs_check(const HostShape& s, const tetris_traj_obs* obs) {
    if (!obs || !obs->d_obs) return fail(TETRIS_E_ARG, "the observation records are NULL");
    if (((uintptr_t)obs->d_obs) & 15u) return fail(TETRIS_E_ARG, "d_obs must be 16-byte aligned");
    if (obs->capacity < 1 || (unsigned long long)obs->capacity * (unsigned long long)s.N >= (1ull << 31)) return fail(TETRIS_E_ARG, "the window must hold between 1 and 2^31 - 1 entries");
    return TETRIS_OK;
}

static inline int traj_observe_args(const HostShape& s, const Geo& geo, const tetris_traj_obs* obs, int row, const uint8_t* d_player, TrajObserveArgs& oa) {
    int rc;
    if ((rc = traj_batch_rules(s, "tetris_traj_observe_dev")) || (rc = traj_obs_check(s, obs))) return rc;
    if (row < 0 || row >= obs->capacity) return fail(TETRIS_E_ARG, "row outside the window");
    oa.geo = geo; oa.n = s.N; oa.n_players = s.P; oa.player = d_player;
    oa.obs = obs->d_obs + (size_t)row * (size_t)s.N * (size_t)s.P * OBS_WORDS;
    return TETRIS_OK;
}

// (sa.blocks, the counts per workgroup, is the product's own scratch: NULL here)
static inline int traj_select_args(const HostShape& s, const uint8_t* d_mask, int rows, int flags, int32_t* d_index, long long cap, int32_t* d_count,
                                   TrajSelectArgs& sa) {
    int rc = traj_batch_rules(s, "tetris_traj_select_dev");
    if (rc) return rc;
    if (!d_mask || !d_index || !d_count) return fail(TETRIS_E_ARG, "mask/index/count are NULL");
    if (flags & ~TETRIS_SELECT_AUGMENT) return fail(TETRIS_E_ARG, "unknown flag");
    if (rows < 1 || cap < 0) return fail(TETRIS_E_ARG, "rows < 1 or cap < 0");
    if ((unsigned long long)rows * (unsigned long long)s.N >= (1ull << 31)) return fail(TETRIS_E_ARG, "rows * N must be below 2^31");
    sa.mask = d_mask; sa.total = (uint32_t)rows * (uint32_t)s.N; sa.augment = flags & TETRIS_SELECT_AUGMENT;
    sa.index = d_index; sa.cap = cap; sa.count = d_count;
    sa.nblocks = (int)((sa.total + SELECT_ELEMS - 1) / SELECT_ELEMS);
    sa.blocks = nullptr;
    return TETRIS_OK;
}

static inline int traj_batch_args(const HostShape& s, const tetris_traj* traj, const tetris_traj_obs* obs, const float* d_adv_in, const float* d_target_in,
                                  const int32_t* d_index, int M, const tetris_traj_batch* out, TrajBatchArgs& ba) {
    int rc = traj_batch_rules(s, "tetris_traj_batch_dev");
    if (rc) return rc;
    if (!traj || !out || !d_index) return fail(TETRIS_E_ARG, "the window, the outputs or the index list are NULL");
    if ((rc = traj_obs_check(s, obs))) return rc;
    if (!traj->d_action || !traj->d_prob || !traj->d_reward || !traj->d_done) return fail(TETRIS_E_ARG, "an array of the window is NULL");
    if (traj->capacity != obs->capacity) return fail(TETRIS_E_ARG, "the window and its observation records differ in capacity");
    if (M < 0) return fail(TETRIS_E_ARG, "M < 0");
    ba.m = M; ba.n_slots = s.P; ba.H = s.H;
    ba.total = (uint32_t)traj->capacity * (uint32_t)s.N;
    ba.index = d_index; ba.obs = obs->d_obs;
    ba.action = traj->d_action; ba.prob = traj->d_prob; ba.reward = traj->d_reward; ba.done = traj->d_done;
    ba.adv = d_adv_in; ba.target = d_target_in;
    ba.visual = out->d_visual; ba.vector = out->d_vector; ba.piece = out->d_piece; ba.action_out = out->d_action;
    ba.prob_out = out->d_prob; ba.adv_out = out->d_adv; ba.target_out = out->d_target; ba.reward_out = out->d_reward;
    ba.done_out = out->d_done; ba.valid = out->d_valid;
    ba.steps = 0; ba.limit = 0u; ba.flags = nullptr; ba.step_mask = 0u;
    return TETRIS_OK;
}

// ---------------------------------------------------------------- the planning agent's windows (tetris_plan_traj.h)
// the argument checks, then the kernel arguments
static inline int traj_record_plan_args(const HostShape& s, const tetris_traj* traj, const tetris_traj_plan* plan, const tetris_traj_obs* obs, int row,
                                        const tetris_plan_eval* e, const uint8_t* d_done, const uint8_t* d_dead, PlanRecordArgs& ra) {
    if (!traj || !e) return fail(TETRIS_E_ARG, "the window or the argument struct is NULL");
    int rc = not_on_split(s, "tetris_traj_record_plan_dev");
    if (rc) return rc;
    if (s.P > 2) return fail(TETRIS_E_ARG, "the reward is defined for one or two players (tetris_environment.py:135-144)");
    if (!traj->d_action || !traj->d_prob || !traj->d_value || !traj->d_reward || !traj->d_done) return fail(TETRIS_E_ARG, "an array of the window is NULL");
    if (row < 0 || row >= traj->capacity) return fail(TETRIS_E_ARG, "row outside the window");
    if (!e->d_choice || !e->d_piece || !e->d_prob) return fail(TETRIS_E_ARG, "choice/piece/prob of the choosing call are NULL");
    if (!d_done || !d_dead) return fail(TETRIS_E_ARG, "done/dead are NULL");
    if (plan) {
        if (!plan->d_rec) return fail(TETRIS_E_ARG, "the plan records are NULL");
        if ((rc = traj_obs_check(s, obs))) return rc;
        if (((uintptr_t)plan->d_rec) & 15u) return fail(TETRIS_E_ARG, "d_rec must be 16-byte aligned");
        if (plan->capacity != traj->capacity || obs->capacity != traj->capacity) return fail(TETRIS_E_ARG, "the window, its plan records and its observation records differ in capacity");
        if (!e->d_count || !e->d_cols) return fail(TETRIS_E_ARG, "count/cols of the choosing call are NULL");
        if (e->max_lists < 1 || e->max_lists > PLAN_RECORD_MAX_LISTS) return fail(TETRIS_E_ARG, "1 <= max_lists <= 256");
        if (((uintptr_t)e->d_cols) & 3u) return fail(TETRIS_E_ARG, "cols must be 4-byte aligned");
    }
    const size_t n = (size_t)s.N, at = (size_t)row * n;
    memset(&ra, 0, sizeof ra);
    ra.n = s.N; ra.n_players = s.P; ra.H = s.H; ra.max_lists = e->max_lists;
    ra.player = e->d_player; ra.count = e->d_count; ra.cols = e->d_cols; ra.choice = e->d_choice;
    ra.piece = e->d_piece; ra.prob_in = e->d_prob; ra.value = e->d_value;
    ra.done = d_done; ra.dead = d_dead;
    if (plan) {
        ra.obs = obs->d_obs + at * (size_t)s.P * OBS_WORDS;
        ra.rec = plan->d_rec + at * PLAN_REC_WORDS;
    }
    ra.action = traj->d_action + at * 4; ra.prob = traj->d_prob + at;
    ra.value0 = traj->d_value + at; ra.value1 = traj->d_value + (size_t)traj->capacity * n + at;
    ra.reward = traj->d_reward + at; ra.done_out = traj->d_done + at;
    return TETRIS_OK;
}

static inline int traj_plan_batch_args(const HostShape& s, const tetris_traj_plan* plan, const int32_t* d_index, int M, float small_fill, int flags,
                                       void* d_delta, void* d_sums, PlanBatchArgs& ba) {
    int rc = traj_batch_rules(s, "tetris_traj_plan_batch_dev");
    if (rc) return rc;
    if (!plan || !plan->d_rec || !d_index) return fail(TETRIS_E_ARG, "the plan records or the index list are NULL");
    if (!d_delta && !d_sums) return fail(TETRIS_E_ARG, "delta and sums are both NULL");
    if (M < 0) return fail(TETRIS_E_ARG, "M < 0");
    if (plan->capacity < 1 || (unsigned long long)plan->capacity * (unsigned long long)s.N >= (1ull << 31)) return fail(TETRIS_E_ARG, "the window must hold between 1 and 2^31 - 1 entries");
    if (flags & ~TETRIS_PLAN_BATCH_F16) return fail(TETRIS_E_ARG, "unknown flag");
    if ((((uintptr_t)plan->d_rec) | ((uintptr_t)d_delta) | ((uintptr_t)d_sums)) & 15u) return fail(TETRIS_E_ARG, "d_rec / delta / sums must be 16-byte aligned");
    memset(&ba, 0, sizeof ba);
    ba.m = M; ba.H = s.H;
    ba.total = (uint32_t)plan->capacity * (uint32_t)s.N;
    ba.index = d_index; ba.rec = plan->d_rec;
    ba.small_fill = small_fill; ba.f16 = (flags & TETRIS_PLAN_BATCH_F16) ? 1 : 0;
    ba.delta = d_delta; ba.sums = d_sums;
    return TETRIS_OK;
}

// ---------------------------------------------------------------- experience replay (tetris_replay.h)
// the buffer's rules, shared by the four calls; `arrays`: the call touches the entries' arrays, not the priorities alone
static inline int replay_ring(const HostShape& s, const tetris_replay* rp, const char* what, bool arrays, ReplayRing& r) {
    int rc = traj_batch_rules(s, what);
    if (rc) return rc;
    if (!rp) return fail(TETRIS_E_ARG, "the replay buffer is NULL");
    if (rp->k_step < 0) return fail(TETRIS_E_ARG, "k_step must be >= 0");
    const long long max_size = (long long)rp->capacity - rp->k_step;
    if (max_size < 1 || max_size > REPLAY_MAX_SIZE) return fail(TETRIS_E_ARG, "max_size = capacity - k_step must be in [1, 2^24]");
    if (!rp->d_prio || !rp->d_cursor) return fail(TETRIS_E_ARG, "prio/cursor of the replay buffer are NULL");
    if (arrays) {
        if (!rp->d_obs || !rp->d_action || !rp->d_prob || !rp->d_adv || !rp->d_target || !rp->d_reward || !rp->d_done || !rp->d_flags)
            return fail(TETRIS_E_ARG, "an array of the replay buffer is NULL");
        if (((uintptr_t)rp->d_obs) & 15u) return fail(TETRIS_E_ARG, "d_obs of the replay buffer must be 16-byte aligned");
    }
    r.capacity = rp->capacity; r.k_step = rp->k_step; r.max_size = (int)max_size; r.n_slots = s.P;
    r.obs = rp->d_obs; r.action = rp->d_action; r.prob = rp->d_prob; r.adv = rp->d_adv; r.target = rp->d_target; r.reward = rp->d_reward;
    r.done = rp->d_done; r.flags = rp->d_flags; r.prio = rp->d_prio; r.cursor = rp->d_cursor;
    return TETRIS_OK;
}

// (aa.offsets, the entries per game, is the product's own scratch: NULL here)
static inline int replay_add_args(const HostShape& s, const tetris_replay* rp, const tetris_traj* traj, const tetris_traj_obs* obs, const float* d_adv_in,
                                  const float* d_target_in, const float* d_prio_in, const uint8_t* d_mask, int rows, int flags, ReplayAddArgs& aa) {
    int rc = replay_ring(s, rp, "tetris_replay_add_dev", true, aa.rp);
    if (rc) return rc;
    if (!traj || !d_mask) return fail(TETRIS_E_ARG, "the window or the mask are NULL");
    if ((rc = traj_obs_check(s, obs))) return rc;
    if (!traj->d_action || !traj->d_prob || !traj->d_reward || !traj->d_done) return fail(TETRIS_E_ARG, "an array of the window is NULL");
    if (traj->capacity != obs->capacity) return fail(TETRIS_E_ARG, "the window and its observation records differ in capacity");
    if (flags & ~TETRIS_SELECT_AUGMENT) return fail(TETRIS_E_ARG, "unknown flag");
    if ((unsigned long long)(rows < 0 ? 0 : rows) * (unsigned long long)s.N >= (1ull << 31)) return fail(TETRIS_E_ARG, "rows * N must be below 2^31");
    if (rows < 1 || rows > traj->capacity) return fail(TETRIS_E_ARG, "rows outside [1, capacity]");
    aa.n = s.N; aa.rows = rows; aa.augment = flags & TETRIS_SELECT_AUGMENT;
    aa.mask = d_mask; aa.obs = obs->d_obs; aa.action = traj->d_action; aa.prob = traj->d_prob; aa.reward = traj->d_reward; aa.done = traj->d_done;
    aa.adv = d_adv_in; aa.target = d_target_in; aa.prio = d_prio_in;
    aa.offsets = nullptr;
    return TETRIS_OK;
}

// words of the sort's scratch for max_size entries: two (key, position) pairs, the ranks, the histograms and the digits' totals
static inline int sort_tiles(uint32_t max_size) { return (int)((max_size + SORT_TILE - 1) / SORT_TILE); }
static inline size_t replay_scratch_words(uint32_t max_size) { return 5 * (size_t)max_size + (size_t)SORT_RADIX * sort_tiles(max_size) + SORT_RADIX; }
// (scratch: replay_scratch_words(max_size) words of the caller's own; sorts: the two sorts' arguments, pass and in / out set per pass)
static inline int replay_sample_args(const HostShape& s, const tetris_replay* rp, int M, float alpha, float beta, uint32_t seed, uint64_t draw,
                                     int32_t* d_index, float* d_weight, int32_t* d_count, int32_t* d_rank, float* d_key, ReplaySampleArgs& sa) {
    ReplayRing r;
    int rc = replay_ring(s, rp, "tetris_replay_sample_dev", false, r);
    if (rc) return rc;
    if (!d_index || !d_weight || !d_count) return fail(TETRIS_E_ARG, "index/weight/count are NULL");
    if (M < 0) return fail(TETRIS_E_ARG, "M < 0");
    memset(&sa, 0, sizeof sa);
    sa.max_size = (uint32_t)r.max_size; sa.m = M; sa.prio = r.prio; sa.cursor = r.cursor;
    sa.alpha = alpha; sa.alpha_beta = alpha * beta;
    sa.seed = seed; sa.draw_lo = (uint32_t)draw; sa.draw_hi = (uint32_t)(draw >> 32);
    sa.index = d_index; sa.weight = d_weight; sa.count = d_count; sa.rank_out = d_rank; sa.key_out = d_key;
    return TETRIS_OK;
}
// the scratch's parts: pair a, pair b, the ranks; -> the sort's arguments over the rest (pass, in and out are set per pass)
static inline SortArgs replay_sample_scratch(ReplaySampleArgs& sa, uint32_t* scratch) {
    const size_t m = sa.max_size;
    sa.key_a = scratch; sa.pos_a = scratch + m; sa.key_b = scratch + 2 * m; sa.pos_b = scratch + 3 * m;
    sa.rank = reinterpret_cast<int32_t*>(scratch + 4 * m);
    SortArgs so;
    memset(&so, 0, sizeof so);
    so.total = sa.max_size; so.ntiles = sort_tiles(sa.max_size);
    so.hist = scratch + 5 * m; so.totals = so.hist + (size_t)SORT_RADIX * so.ntiles;
    return so;
}
// pass p of a sort that starts and, after four passes, ends in (key, pos); (okey, opos): the other pair
static inline void sort_pass(SortArgs& so, int pass, uint32_t* key, uint32_t* pos, uint32_t* okey, uint32_t* opos) {
    so.pass = pass;
    so.key_in = (pass & 1) ? okey : key; so.pos_in = (pass & 1) ? opos : pos;
    so.key_out = (pass & 1) ? key : okey; so.pos_out = (pass & 1) ? pos : opos;
}

static inline int replay_update_args(const HostShape& s, const tetris_replay* rp, const int32_t* d_index, const float* d_prio_new, int M, ReplayUpdateArgs& ua) {
    ReplayRing r;
    int rc = replay_ring(s, rp, "tetris_replay_update_prios_dev", false, r);
    if (rc) return rc;
    if (!d_index || !d_prio_new) return fail(TETRIS_E_ARG, "index/prio are NULL");
    if (M < 0) return fail(TETRIS_E_ARG, "M < 0");
    ua.prio = r.prio; ua.max_size = (uint32_t)r.max_size; ua.index = d_index; ua.value = d_prio_new; ua.m = M;
    return TETRIS_OK;
}

// the gather is tetris_traj_batch_dev's kernel over the ring: ba.m = M * steps samples — the first `steps` rows of every view
// (step_mask 0: tetris_replay_gather_dev) or the rows of step_mask's bits (tetris_replay_gather_steps_dev; `steps` is not read)
static inline int replay_gather_mask_args(const HostShape& s, const tetris_replay* rp, const int32_t* d_index, int M, int steps, uint64_t step_mask,
                                          const tetris_traj_batch* out, TrajBatchArgs& ba) {
    ReplayRing r;
    int rc = replay_ring(s, rp, step_mask ? "tetris_replay_gather_steps_dev" : "tetris_replay_gather_dev", true, r);
    if (rc) return rc;
    if (!d_index || !out) return fail(TETRIS_E_ARG, "the index list or the outputs are NULL");
    if (M < 0) return fail(TETRIS_E_ARG, "M < 0");
    if (step_mask) {
        if (r.k_step > 63) return fail(TETRIS_E_ARG, "a step list needs k_step <= 63");
        if (r.k_step < 63 && (step_mask >> (r.k_step + 1))) return fail(TETRIS_E_ARG, "step_mask has a bit above k_step");
        steps = __builtin_popcountll(step_mask);
        if (step_mask == (steps == 64 ? ~0ull : (1ull << steps) - 1ull)) step_mask = 0u;          // the first `steps` rows
    }
    if (steps < 1 || steps > r.k_step + 1) return fail(TETRIS_E_ARG, "steps outside [1, k_step + 1]");
    if ((unsigned long long)M * (unsigned long long)steps >= (1ull << 31)) return fail(TETRIS_E_ARG, "M * steps must be below 2^31");
    ba.m = M * steps; ba.n_slots = s.P; ba.H = s.H;
    ba.total = (uint32_t)r.capacity;
    ba.index = d_index; ba.obs = r.obs;
    ba.action = r.action; ba.prob = r.prob; ba.reward = r.reward; ba.done = r.done;
    ba.adv = r.adv; ba.target = r.target;
    ba.visual = out->d_visual; ba.vector = out->d_vector; ba.piece = out->d_piece; ba.action_out = out->d_action;
    ba.prob_out = out->d_prob; ba.adv_out = out->d_adv; ba.target_out = out->d_target; ba.reward_out = out->d_reward;
    ba.done_out = out->d_done; ba.valid = out->d_valid;
    ba.steps = steps; ba.limit = (uint32_t)r.max_size; ba.flags = r.flags; ba.step_mask = step_mask;
    return TETRIS_OK;
}

static inline int replay_gather_args(const HostShape& s, const tetris_replay* rp, const int32_t* d_index, int M, int steps, const tetris_traj_batch* out,
                                     TrajBatchArgs& ba) {
    return replay_gather_mask_args(s, rp, d_index, M, steps, 0u, out, ba);
}
static inline int replay_gather_steps_args(const HostShape& s, const tetris_replay* rp, const int32_t* d_index, int M, uint64_t step_mask,
                                           const tetris_traj_batch* out, TrajBatchArgs& ba) {
    if (!step_mask) return fail(TETRIS_E_ARG, "step_mask names no step");
    return replay_gather_mask_args(s, rp, d_index, M, 0, step_mask, out, ba);
}
// A gather over host memory (the CPU build of the bodies: tests/cpu_harness), the product's launch as a loop over slots and samples.
// tetris_lib_compose.h says which side runs what.
static inline int traj_batch_run_serial(int n_slots, const TrajBatchArgs& ba) {
    for (int sl = 0; sl < n_slots; sl++)
        for (int j = 0; j < ba.m; j++) batch_sample_slot(ba, j, sl);
    return TETRIS_OK;
}

// ---------------------------------------------------------------- loss heads (tetris_loss.h)
// the rules both heads share, then the kernel arguments (all but count and partial, the caller's scratch)
static inline int loss_common_check(int M, int K, int flags, int known_flags, const void* x, const void* grad_x) {
    if (M < 0) return fail(TETRIS_E_ARG, "M < 0");
    if (K != 1 && K != 7) return fail(TETRIS_E_ARG, "n_pieces must be 1 or 7");
    if (flags & ~known_flags) return fail(TETRIS_E_ARG, "unknown flag");
    if ((((uintptr_t)x) | ((uintptr_t)grad_x)) & 15u) return fail(TETRIS_E_ARG, "the evaluation and its gradient must be 16-byte aligned");
    return TETRIS_OK;
}
static inline int ppo_loss_args(const tetris_ppo_loss* l, LossArgs& la) {
    if (!l) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    if (!l->d_pi || !l->d_v || !l->d_action || !l->d_prob_old || !l->d_adv || !l->d_target)
        return fail(TETRIS_E_ARG, "pi/v/action/prob_old/adv/target are NULL");
    if (!l->d_grad_pi || !l->d_grad_v || !l->d_stats) return fail(TETRIS_E_ARG, "grad_pi/grad_v/stats are NULL");
    int rc = loss_common_check(l->M, l->n_pieces, l->flags, TETRIS_LOSS_F16 | TETRIS_LOSS_VALUE_F16 | TETRIS_LOSS_GRAD_F16, l->d_pi, l->d_grad_pi);
    if (rc) return rc;
    if (l->n_values != 1 && l->n_values != l->n_pieces) return fail(TETRIS_E_ARG, "n_values must be 1 or n_pieces");
    if (!(l->clip >= 0.0f)) return fail(TETRIS_E_ARG, "clip must be >= 0");
    memset(&la, 0, sizeof la);
    la.head = LOSS_PPO;
    la.M = l->M; la.K = l->n_pieces; la.V = l->n_values;
    la.in_f16 = (l->flags & TETRIS_LOSS_F16) ? 1 : 0; la.v_f16 = (l->flags & TETRIS_LOSS_VALUE_F16) ? 1 : 0;
    la.grad_f16 = (l->flags & TETRIS_LOSS_GRAD_F16) ? 1 : 0;
    la.x = l->d_pi; la.v = l->d_v; la.action = l->d_action; la.old = l->d_prob_old; la.adv = l->d_adv; la.target = l->d_target;
    la.valid = l->d_valid;
    la.clip = l->clip; la.c1 = l->value_loss; la.c2 = l->policy_loss; la.c3 = l->entropy_loss;
    la.cf = l->entropy_floor_loss; la.cr = l->rescaled_entropy; la.floor = l->entropy_floor; la.hmax = l->max_entropy;
    la.grad_scale = l->grad_scale;
    la.grad_x = l->d_grad_pi; la.grad_v = l->d_grad_v; la.terms = l->d_terms; la.stats = l->d_stats;
    return TETRIS_OK;
}
static inline int dqn_loss_args(const tetris_dqn_loss* l, LossArgs& la) {
    if (!l) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    if (!l->d_Q || !l->d_action || !l->d_target) return fail(TETRIS_E_ARG, "Q/action/target are NULL");
    if (!l->d_grad_Q || !l->d_new_prio || !l->d_stats) return fail(TETRIS_E_ARG, "grad_Q/new_prio/stats are NULL");
    int rc = loss_common_check(l->M, l->n_pieces, l->flags, TETRIS_LOSS_F16 | TETRIS_LOSS_GRAD_F16, l->d_Q, l->d_grad_Q);
    if (rc) return rc;
    memset(&la, 0, sizeof la);
    la.head = LOSS_DQN;
    la.M = l->M; la.K = l->n_pieces; la.V = 1;
    la.in_f16 = (l->flags & TETRIS_LOSS_F16) ? 1 : 0; la.grad_f16 = (l->flags & TETRIS_LOSS_GRAD_F16) ? 1 : 0;
    la.x = l->d_Q; la.action = l->d_action; la.target = l->d_target; la.weight = l->d_weight; la.valid = l->d_valid;
    la.optimistic = l->optimistic_prios; la.grad_scale = l->grad_scale;
    la.grad_x = l->d_grad_Q; la.new_prio = l->d_new_prio; la.q = l->d_q; la.stats = l->d_stats;
    return TETRIS_OK;
}
// the planning head: the window's own rules (one or two players, no split batch, T N below 2^31), then the head's
static inline int plan_loss_args(const HostShape& s, const tetris_traj_plan* plan, const tetris_plan_loss* l, LossArgs& la) {
    int rc = traj_batch_rules(s, "tetris_plan_loss_dev");
    if (rc) return rc;
    if (!l) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    if (!plan || !plan->d_rec) return fail(TETRIS_E_ARG, "the plan records are NULL");
    if (!l->d_phi || !l->d_v || !l->d_index || !l->d_piece || !l->d_prob_old || !l->d_adv || !l->d_target)
        return fail(TETRIS_E_ARG, "phi/v/index/piece/prob_old/adv/target are NULL");
    if (!l->d_grad_phi || !l->d_grad_v || !l->d_stats) return fail(TETRIS_E_ARG, "grad_phi/grad_v/stats are NULL");
    if ((rc = loss_common_check(l->M, l->n_pieces, l->flags, TETRIS_LOSS_F16 | TETRIS_LOSS_VALUE_F16 | TETRIS_LOSS_GRAD_F16, l->d_phi, l->d_grad_phi))) return rc;
    if (l->n_values != 1 && l->n_values != l->n_pieces) return fail(TETRIS_E_ARG, "n_values must be 1 or n_pieces");
    if (!(l->clip >= 0.0f)) return fail(TETRIS_E_ARG, "clip must be >= 0");
    if (l->piece_stride < 1) return fail(TETRIS_E_ARG, "piece_stride must be >= 1");
    if (plan->capacity < 1 || (unsigned long long)plan->capacity * (unsigned long long)s.N >= (1ull << 31)) return fail(TETRIS_E_ARG, "the window must hold between 1 and 2^31 - 1 entries");
    if (((uintptr_t)plan->d_rec) & 15u) return fail(TETRIS_E_ARG, "d_rec must be 16-byte aligned");
    memset(&la, 0, sizeof la);
    la.head = LOSS_PLAN;
    la.M = l->M; la.K = l->n_pieces; la.V = l->n_values; la.H = s.H;
    la.in_f16 = (l->flags & TETRIS_LOSS_F16) ? 1 : 0; la.v_f16 = (l->flags & TETRIS_LOSS_VALUE_F16) ? 1 : 0;
    la.grad_f16 = (l->flags & TETRIS_LOSS_GRAD_F16) ? 1 : 0;
    la.x = l->d_phi; la.v = l->d_v; la.old = l->d_prob_old; la.adv = l->d_adv; la.target = l->d_target; la.valid = l->d_valid;
    la.total = (uint32_t)plan->capacity * (uint32_t)s.N; la.rec = plan->d_rec; la.index = l->d_index;
    la.piece = l->d_piece; la.piece_stride = l->piece_stride; la.small_fill = l->small_fill;
    la.clip = l->clip; la.c1 = l->value_loss; la.c2 = l->policy_loss; la.c3 = l->entropy_loss; la.c4 = l->impossibility_loss;
    la.grad_scale = l->grad_scale;
    la.grad_x = l->d_grad_phi; la.grad_v = l->d_grad_v; la.terms = l->d_terms; la.stats = l->d_stats;
    return TETRIS_OK;
}
// whether the call counts D / Dnz on the device (otherwise both are M), and the words of scratch it needs: two counts,
// padded to 16 bytes, then the workgroups' partial rows
static inline bool loss_counts(const LossArgs& la) { return la.valid || la.weight || la.index; }
static inline size_t loss_scratch_words(const LossArgs& la) { return 4 + (size_t)loss_blocks_of(la) * LOSS_SUMS; }
// A call over host memory (the CPU build of the bodies: tests/cpu_harness), the product's three launches as three loops: the
// counts, the blocks of LOSS_BLOCK samples, the partial rows.  tetris_lib_compose.h says which side runs what.
static inline int loss_run_serial(LossArgs& la) {
    if (la.M == 0) {
        memset(la.stats, 0, LOSS_STATS * sizeof(float));
        return TETRIS_OK;
    }
    const int blocks = loss_blocks_of(la);
    std::vector<float> partial((size_t)blocks * LOSS_SUMS);
    la.partial = partial.data();
    uint32_t d = (uint32_t)la.M, dnz = (uint32_t)la.M;
    if (loss_counts(la)) {
        d = dnz = 0u;
        for (int m = 0; m < la.M; m++) loss_count_sample(la, (size_t)m, d, dnz);
    }
    for (int blk = 0; blk < blocks; blk++) {
        if (la.head == LOSS_PLAN) plan_loss_block_serial(la, blk, (float)d);
        else loss_block_serial(la, blk, (float)d, (float)dnz);
    }
    loss_reduce_serial(la, blocks, (float)d, (float)dnz);
    return TETRIS_OK;
}

// ---------------------------------------------------------------- k-step target estimator (tetris_kstep.h)
// the argument rules, then the kernel arguments (all but vals, which without d_values is the caller's scratch)
static inline int kstep_target_args(const tetris_kstep_target* t, KstepArgs& a) {
    if (!t) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    if (!t->d_out || !t->d_reward || !t->d_done || !t->d_target) return fail(TETRIS_E_ARG, "out/reward/done/target are NULL");
    if (t->M < 0) return fail(TETRIS_E_ARG, "M < 0");
    if (t->k_step < 1 || t->k_step > KSTEP_MAX) return fail(TETRIS_E_ARG, "k_step must be in [1, 63]");
    if (!t->step_mask) return fail(TETRIS_E_ARG, "step_mask names no step");
    if ((t->step_mask & 1u) || (t->k_step < 63 && (t->step_mask >> (t->k_step + 1)))) return fail(TETRIS_E_ARG, "step_mask has a bit outside [1, k_step]");
    if (t->mode != TETRIS_KSTEP_Q && t->mode != TETRIS_KSTEP_V) return fail(TETRIS_E_ARG, "mode must be TETRIS_KSTEP_Q or TETRIS_KSTEP_V");
    if (t->n_pieces != 1 && t->n_pieces != 7) return fail(TETRIS_E_ARG, "n_pieces must be 1 or 7");
    if (t->mode == TETRIS_KSTEP_V && t->n_values != 1 && t->n_values != t->n_pieces) return fail(TETRIS_E_ARG, "n_values must be 1 or n_pieces");
    if (t->used_pieces <= 0 || (t->used_pieces >> t->n_pieces)) return fail(TETRIS_E_ARG, "used_pieces must name at least one piece and none at or above n_pieces");
    if (t->flags & ~(TETRIS_LOSS_F16 | TETRIS_KSTEP_TRUNCATE)) return fail(TETRIS_E_ARG, "unknown flag");
    if (t->d_index ? t->max_size < 1 : t->max_size != 0) return fail(TETRIS_E_ARG, "d_index and max_size >= 1 (the ring) or neither (arrays [M][k_step + 1])");
    if (t->mode == TETRIS_KSTEP_Q && (((uintptr_t)t->d_out) & 15u)) return fail(TETRIS_E_ARG, "Q must be 16-byte aligned");
    const int n = __builtin_popcountll(t->step_mask);
    if ((unsigned long long)t->M * (unsigned long long)n >= (1ull << 31)) return fail(TETRIS_E_ARG, "M * n must be below 2^31");
    memset(&a, 0, sizeof a);
    a.M = t->M; a.n = n; a.k = t->k_step; a.K = t->n_pieces; a.W = t->mode == TETRIS_KSTEP_V ? t->n_values : t->n_pieces;
    a.mode = t->mode; a.f16 = (t->flags & TETRIS_LOSS_F16) ? 1 : 0; a.truncate = (t->flags & TETRIS_KSTEP_TRUNCATE) ? 1 : 0;
    a.used = (uint32_t)t->used_pieces; a.limit = (uint32_t)t->max_size; a.n_used = (float)__builtin_popcount((unsigned)t->used_pieces);
    a.step_mask = t->step_mask;
    a.x = t->d_out; a.reward = t->d_reward; a.done = t->d_done; a.index = t->d_index;
    a.target = t->d_target; a.values = t->d_values; a.done_time = t->d_done_time;
    for (int i = 0; i <= a.k; i++) { a.g[i] = (float)pow((double)t->gamma, (double)i); a.l[i] = (float)pow((double)t->lam, (double)i); }
    return TETRIS_OK;
}
// A call over host memory (the CPU build of the bodies: tests/cpu_harness), the product's launches as loops: in Q mode the values
// of the M n rows, then the samples.  tetris_lib_compose.h says which side runs what.
static inline int kstep_run_serial(KstepArgs& a) {
    if (a.M == 0) return TETRIS_OK;
    std::vector<float> scratch;
    if (a.mode == KSTEP_Q) {
        if (!a.values) scratch.resize((size_t)a.M * a.n);
        a.vals = a.values ? a.values : scratch.data();
        for (size_t row = 0; row < (size_t)a.M * a.n; row++) kstep_value_row(a, row);
    }
    for (int j = 0; j < a.M; j++) kstep_sample(a, (size_t)j);
    return TETRIS_OK;
}

// ---------------------------------------------------------------- output heads (tetris_head.h)
// the rules both heads share, then the kernel arguments.  `big` are the [M][4][10][K] arrays of the call.
static inline int head_common_check(int M, int K, int flags, const void* const* big, int n_big) {
    if (M < 1) return fail(TETRIS_E_ARG, "M < 1");
    if (K != 1 && K != 7) return fail(TETRIS_E_ARG, "n_pieces must be 1 or 7");
    if (flags & ~(TETRIS_HEAD_F16 | TETRIS_HEAD_VALUE_F16)) return fail(TETRIS_E_ARG, "unknown flag");
    for (int i = 0; i < n_big; i++)
        if (((uintptr_t)big[i]) & 15u) return fail(TETRIS_E_ARG, "the [M][4][10][K] arrays must be 16-byte aligned");
    return TETRIS_OK;
}
static inline int q_head_args(const tetris_q_head* q, int grad, HeadArgs& h) {
    if (!q) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    if (!q->d_a) return fail(TETRIS_E_ARG, "a is NULL");
    if (grad ? !q->d_grad_Q || !q->d_grad_a : !q->d_Q || !q->d_V) return fail(TETRIS_E_ARG, grad ? "grad_Q/grad_a are NULL" : "Q/V are NULL");
    if (grad && q->d_v && !q->d_grad_v) return fail(TETRIS_E_ARG, "grad_v is NULL where v is given");
    const void* const big[3] = {q->d_a, grad ? q->d_grad_Q : q->d_Q, grad ? q->d_grad_a : q->d_A};
    int rc = head_common_check(q->M, q->n_pieces, q->flags, big, 3);
    if (rc) return rc;
    if (q->d_v && q->n_values != 1 && q->n_values != q->n_pieces) return fail(TETRIS_E_ARG, "n_values must be 1 or n_pieces");
    if (q->mode != TETRIS_HEAD_MEAN && q->mode != TETRIS_HEAD_MAX && q->mode != TETRIS_HEAD_NONE) return fail(TETRIS_E_ARG, "mode must be TETRIS_HEAD_MEAN, _MAX or _NONE");
    if (q->used_pieces <= 0) return fail(TETRIS_E_ARG, "used_pieces names no piece");
    if (q->used_pieces >> q->n_pieces) return fail(TETRIS_E_ARG, "used_pieces has a bit at or above n_pieces");
    memset(&h, 0, sizeof h);
    h.head = HEAD_Q; h.grad = grad;
    h.M = q->M; h.K = q->n_pieces; h.W = q->d_v ? q->n_values : 0;
    h.mode = q->mode; h.separate = q->separate_piece_values ? 1 : 0;
    h.f16 = (q->flags & TETRIS_HEAD_F16) ? 1 : 0; h.v_f16 = (q->flags & TETRIS_HEAD_VALUE_F16) ? 1 : 0;
    h.mask = (uint32_t)q->used_pieces; h.U = (float)__builtin_popcount((unsigned)q->used_pieces); h.rho = q->advantage_range;
    h.x = q->d_a; h.v = q->d_v;
    if (grad) { h.g = q->d_grad_Q; h.out = q->d_grad_a; h.out_v = q->d_v ? q->d_grad_v : nullptr; }
    else { h.out = q->d_Q; h.out_A = q->d_A; h.V = q->d_V; }
    return TETRIS_OK;
}
static inline int policy_head_args(const tetris_policy_head* p, int grad, HeadArgs& h) {
    if (!p) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    if (!p->d_pi || !p->d_v) return fail(TETRIS_E_ARG, "pi/v are NULL");
    if (grad ? !p->d_grad_pi || !p->d_grad_v || !p->d_grad_x || !p->d_grad_w : !p->d_x || !p->d_w)
        return fail(TETRIS_E_ARG, grad ? "grad_pi/grad_v/grad_x/grad_w are NULL" : "x/w are NULL");
    const void* const big[3] = {p->d_pi, grad ? p->d_grad_pi : p->d_x, grad ? p->d_grad_x : nullptr};
    int rc = head_common_check(p->M, p->n_pieces, p->flags, big, 3);
    if (rc) return rc;
    if (p->n_values != 1 && p->n_values != p->n_pieces + 1) return fail(TETRIS_E_ARG, "n_values must be 1 or n_pieces + 1");
    memset(&h, 0, sizeof h);
    h.head = HEAD_POLICY; h.grad = grad;
    h.M = p->M; h.K = p->n_pieces; h.W = p->n_values;
    h.f16 = (p->flags & TETRIS_HEAD_F16) ? 1 : 0; h.v_f16 = (p->flags & TETRIS_HEAD_VALUE_F16) ? 1 : 0;
    h.mask = (1u << p->n_pieces) - 1u; h.U = (float)p->n_pieces; h.rho = 1.0f;
    if (grad) { h.x = p->d_pi; h.v = p->d_v; h.g = p->d_grad_pi; h.gv = p->d_grad_v; h.out = p->d_grad_x; h.out_v = p->d_grad_w; }
    else { h.x = p->d_x; h.v = p->d_w; h.out = p->d_pi; h.out_v = p->d_v; }
    return TETRIS_OK;
}
// A call over host memory (the CPU build of the bodies: tests/cpu_harness), the product's one launch as a loop over the samples.
// tetris_lib_compose.h says which side runs what.
static inline int head_run_serial(const HeadArgs& h) {
    for (int m = 0; m < h.M; m++) {
        if (h.head == HEAD_Q) head_q_sample_serial(h, (size_t)m);
        else head_policy_sample_serial(h, (size_t)m);
    }
    return TETRIS_OK;
}

// ---------------------------------------------------------------- network inputs (tetris_input.h)
// the argument rules, then the kernel arguments.  The sample's source goes through the rules of the call it is taken from:
// traj_obs_check for a window, replay_gather_mask_args for the ring (with no output of its own).
static inline int input_args(const HostShape& s, const tetris_net_input* in, InputArgs& ia) {
    if (!in) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    int rc = traj_batch_rules(s, "tetris_net_input_dev");
    if (rc) return rc;
    if (in->obs && in->replay) return fail(TETRIS_E_ARG, "obs and replay are both given");
    memset(&ia, 0, sizeof ia);
    if (in->replay) {
        const tetris_traj_batch none = {};
        if ((rc = replay_gather_mask_args(s, in->replay, in->d_index, in->M, in->steps, in->step_mask, &none, ia.ba))) return rc;
    } else {
        if ((rc = traj_obs_check(s, in->obs))) return rc;
        if (!in->d_index) {
            if (in->row < 0 || in->row >= in->obs->capacity) return fail(TETRIS_E_ARG, "row outside the window");
            if (in->M != s.N) return fail(TETRIS_E_ARG, "the row form takes M = N samples");
        }
        if (in->M < 0) return fail(TETRIS_E_ARG, "M < 0");
        ia.ba.m = in->M; ia.ba.n_slots = s.P; ia.ba.H = s.H;
        ia.ba.total = (uint32_t)in->obs->capacity * (uint32_t)s.N;
        ia.ba.index = in->d_index; ia.ba.obs = in->obs->d_obs;
        ia.row_base = in->d_index ? 0u : (uint32_t)in->row * (uint32_t)s.N;
    }
    if (in->n_items < 0 || in->n_items > INPUT_MAX_ITEMS) return fail(TETRIS_E_ARG, "n_items must be in [0, 4]");
    uint32_t seen = 0u;
    for (int i = 0; i < in->n_items; i++) {
        const int code = in->items[i];
        if (code < TETRIS_INPUT_CUMSUM || code > TETRIS_INPUT_HOLES) return fail(TETRIS_E_ARG, "unknown item code");
        if (seen & (1u << code)) return fail(TETRIS_E_ARG, "an item code is named twice");
        seen |= 1u << code;
        ia.chan |= (uint32_t)code << (4 * (i + 1));
    }
    if (in->flags & ~(TETRIS_INPUT_F16 | TETRIS_INPUT_CHANNELS_LAST | TETRIS_INPUT_PAD)) return fail(TETRIS_E_ARG, "unknown flag");
    ia.f16 = (in->flags & TETRIS_INPUT_F16) ? 1 : 0; ia.last = (in->flags & TETRIS_INPUT_CHANNELS_LAST) ? 1 : 0;
    ia.pad = (in->flags & TETRIS_INPUT_PAD) ? 1 : 0;
    if ((((uintptr_t)in->d_visual) | ((uintptr_t)in->d_vector)) & (ia.f16 ? 1u : 3u)) return fail(TETRIS_E_ARG, "visual / vector must be aligned to their element type");
    ia.C = 1 + in->n_items; ia.Hp = s.H + (ia.pad ? 2 : 0); ia.Wp = NCOL + (ia.pad ? 2 : 0);
    ia.E = ia.C * ia.Hp * ia.Wp;
    ia.dA = (uint32_t)(ia.last ? ia.Wp * ia.C : ia.Hp * ia.Wp); ia.dB = (uint32_t)(ia.last ? ia.C : ia.Wp);
    ia.mE = input_magic((uint32_t)ia.E); ia.mA = input_magic(ia.dA); ia.mB = input_magic(ia.dB);
    ia.visual = in->d_visual; ia.vector = in->d_vector; ia.piece = in->d_piece; ia.valid = in->d_valid;
    return TETRIS_OK;
}
// A call over host memory (the CPU build of the bodies: tests/cpu_harness), the product's one launch as a loop over slots and
// samples.  tetris_lib_compose.h says which side runs what.
static inline int input_run_serial(const InputArgs& ia) {
    for (int sl = 0; sl < ia.ba.n_slots; sl++)
        for (int j = 0; j < ia.ba.m; j++) input_sample_slot(ia, j, sl);
    return TETRIS_OK;
}

// ---------------------------------------------------------------- keyboard convolution (tetris_kbd.h)
// the argument rules of the three entry points, then the kernel arguments (all but the scratch, the launcher's)
static inline bool kbd_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + nq && b < a + np;
}
static inline int kbd_args(const tetris_kbd_conv* k, int op, KbdArgs& a) {
    if (!k) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    if (op == KBD_FWD ? !k->d_x || !k->d_w || !k->d_bias || !k->d_out
        : op == KBD_GRAD_X ? !k->d_grad_out || !k->d_w || !k->d_grad_x
                           : !k->d_x || !k->d_grad_out || !k->d_grad_w || !k->d_grad_b)
        return fail(TETRIS_E_ARG, op == KBD_FWD ? "x/w/bias/out are NULL" : op == KBD_GRAD_X ? "grad_out/w/grad_x are NULL" : "x/grad_out/grad_w/grad_b are NULL");
    if (k->M < 1) return fail(TETRIS_E_ARG, "M < 1");
    if (k->n_pieces < 1 || k->n_pieces > 7) return fail(TETRIS_E_ARG, "n_pieces must be in [1, 7]");
    if (k->height < 4 || k->height > 33) return fail(TETRIS_E_ARG, "height must be in [4, 33]");
    if (k->channels < 32 || k->channels > 512 || k->channels % 32) return fail(TETRIS_E_ARG, "channels must be a multiple of 32 in [32, 512]");
    if (k->flags & ~TETRIS_KBD_F16) return fail(TETRIS_E_ARG, "unknown flag");
    const size_t es = (k->flags & TETRIS_KBD_F16) ? 2 : 4, O = 4 * (size_t)k->n_pieces;
    const size_t nx = (size_t)k->M * k->height * KBD_W * k->channels * es, nw = (size_t)k->height * KBD_D * k->channels * O,
                 no = (size_t)k->M * KBD_T * O * es;
    // the arrays of the call: {pointer, bytes}, inputs first
    const void* in[3] = {nullptr, nullptr, nullptr};
    const void* out[2] = {nullptr, nullptr};
    size_t in_n[3] = {0, 0, 0}, out_n[2] = {0, 0};
    if (op == KBD_FWD) { in[0] = k->d_x; in_n[0] = nx; in[1] = k->d_w; in_n[1] = nw * es; in[2] = k->d_bias; in_n[2] = O * 4; out[0] = k->d_out; out_n[0] = no; }
    else if (op == KBD_GRAD_X) { in[0] = k->d_grad_out; in_n[0] = no; in[1] = k->d_w; in_n[1] = nw * es; out[0] = k->d_grad_x; out_n[0] = nx; }
    else { in[0] = k->d_x; in_n[0] = nx; in[1] = k->d_grad_out; in_n[1] = no; out[0] = k->d_grad_w; out_n[0] = nw * 4; out[1] = k->d_grad_b; out_n[1] = O * 4; }
    for (int i = 0; i < 3; i++)
        if (((uintptr_t)in[i]) & 15u) return fail(TETRIS_E_ARG, "the arrays must be 16-byte aligned");
    for (int i = 0; i < 2; i++)
        if (((uintptr_t)out[i]) & 15u) return fail(TETRIS_E_ARG, "the arrays must be 16-byte aligned");
    for (int o = 0; o < 2; o++) {
        for (int i = 0; i < 3; i++)
            if (kbd_overlap(out[o], out_n[o], in[i], in_n[i])) return fail(TETRIS_E_ARG, "an output overlaps an input");
        if (o == 1 && kbd_overlap(out[0], out_n[0], out[1], out_n[1])) return fail(TETRIS_E_ARG, "the outputs overlap");
    }
    memset(&a, 0, sizeof a);
    a.op = op; a.M = k->M; a.K = k->n_pieces; a.O = 4 * k->n_pieces; a.Hp = k->height; a.C = k->channels;
    a.f16 = (k->flags & TETRIS_KBD_F16) ? 1 : 0;
    if (op == KBD_FWD) { a.x = k->d_x; a.w = k->d_w; a.bias = k->d_bias; a.out = k->d_out; }
    else if (op == KBD_GRAD_X) { a.g = k->d_grad_out; a.w = k->d_w; a.out = k->d_grad_x; }
    else { a.x = k->d_x; a.g = k->d_grad_out; a.grad_w = k->d_grad_w; a.grad_b = k->d_grad_b; }
    return TETRIS_OK;
}
// A call over host memory (the CPU build of the bodies: tests/cpu_harness), the product's launches as loops over samples or over
// the rows of grad_w.  tetris_lib_compose.h says which side runs what.
static inline int kbd_run_serial(const KbdArgs& a) {
    if (a.op == KBD_FWD) {
        for (int m = 0; m < a.M; m++) kbd_forward_sample_serial(a, (size_t)m);
    } else if (a.op == KBD_GRAD_X) {
        for (int m = 0; m < a.M; m++) kbd_grad_x_sample_serial(a, (size_t)m);
    } else {
        for (int h = 0; h < a.Hp; h++)
            for (int d = 0; d < KBD_D; d++)
                for (int c = 0; c < a.C; c++) kbd_grad_w_row_serial(a, h, d, c);
        kbd_grad_b_serial(a);
    }
    return TETRIS_OK;
}

// ---------------------------------------------------------------- residual layer (tetris_res.h)
// the argument rules of the three entry points, then the kernel arguments (all but the scratch, the launcher's)
static inline int res_args(const tetris_res_layer* r, int op, ResArgs& a) {
    if (!r) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    if (r->M < 1) return fail(TETRIS_E_ARG, "M < 1");
    if (r->height < 4 || r->height > 33) return fail(TETRIS_E_ARG, "height must be in [4, 33]");
    if (r->in_channels < 8 || r->in_channels > RES_MAX_C || r->in_channels % 8) return fail(TETRIS_E_ARG, "in_channels must be a multiple of 8 in [8, 512]");
    if (r->out_channels < 32 || r->out_channels > RES_MAX_C || r->out_channels % 32) return fail(TETRIS_E_ARG, "out_channels must be a multiple of 32 in [32, 512]");
    if (r->join != TETRIS_RES_JOIN_NONE && r->join != TETRIS_RES_JOIN_ADD && r->join != TETRIS_RES_JOIN_TRUNCATE_ADD) return fail(TETRIS_E_ARG, "unknown join");
    if (r->activation != TETRIS_RES_ACT_NONE && r->activation != TETRIS_RES_ACT_ELU) return fail(TETRIS_E_ARG, "unknown activation");
    if (r->flags & ~TETRIS_RES_F16) return fail(TETRIS_E_ARG, "unknown flag");
    const bool elu = r->activation == TETRIS_RES_ACT_ELU;
    if (op == RES_FWD ? !r->d_x || !r->d_w || !r->d_bias || !r->d_out
        : op == RES_GRAD_X ? !r->d_grad_out || !r->d_w || !r->d_grad_x || (elu && !r->d_y)
                           : !r->d_x || !r->d_grad_out || !r->d_grad_w || !r->d_grad_b || (elu && !r->d_y))
        return fail(TETRIS_E_ARG, op == RES_FWD ? "x/w/bias/out are NULL" : op == RES_GRAD_X ? "grad_out/w/grad_x (ELU: y) are NULL" : "x/grad_out/grad_w/grad_b (ELU: y) are NULL");
    const size_t es = (r->flags & TETRIS_RES_F16) ? 2 : 4, Ci = (size_t)r->in_channels, Co = (size_t)r->out_channels;
    const size_t Cout = (size_t)res_cout(r->in_channels, r->out_channels, r->join), pos = (size_t)r->M * r->height * RES_W;
    const size_t nx = pos * Ci * es, nw = RES_TAPS * Ci * Co, no = pos * Cout * es;
    // the arrays of the call: {pointer, bytes}, inputs first
    const void* in[3] = {nullptr, nullptr, nullptr};
    const void* out[2] = {nullptr, nullptr};
    size_t in_n[3] = {0, 0, 0}, out_n[2] = {0, 0};
    if (op == RES_FWD) { in[0] = r->d_x; in_n[0] = nx; in[1] = r->d_w; in_n[1] = nw * es; in[2] = r->d_bias; in_n[2] = Co * 4; out[0] = r->d_out; out_n[0] = no; }
    else if (op == RES_GRAD_X) { in[0] = r->d_grad_out; in_n[0] = no; in[1] = r->d_w; in_n[1] = nw * es; if (elu) { in[2] = r->d_y; in_n[2] = no; } out[0] = r->d_grad_x; out_n[0] = nx; }
    else { in[0] = r->d_x; in_n[0] = nx; in[1] = r->d_grad_out; in_n[1] = no; if (elu) { in[2] = r->d_y; in_n[2] = no; } out[0] = r->d_grad_w; out_n[0] = nw * 4; out[1] = r->d_grad_b; out_n[1] = Co * 4; }
    for (int i = 0; i < 3; i++)
        if (((uintptr_t)in[i]) & 15u) return fail(TETRIS_E_ARG, "the arrays must be 16-byte aligned");
    for (int i = 0; i < 2; i++)
        if (((uintptr_t)out[i]) & 15u) return fail(TETRIS_E_ARG, "the arrays must be 16-byte aligned");
    for (int o = 0; o < 2; o++) {
        for (int i = 0; i < 3; i++)
            if (kbd_overlap(out[o], out_n[o], in[i], in_n[i])) return fail(TETRIS_E_ARG, "an output overlaps an input");
        if (o == 1 && kbd_overlap(out[0], out_n[0], out[1], out_n[1])) return fail(TETRIS_E_ARG, "the outputs overlap");
    }
    memset(&a, 0, sizeof a);
    a.op = op; a.M = r->M; a.Hp = r->height; a.Ci = r->in_channels; a.Co = r->out_channels; a.Cout = (int)Cout; a.Cz = imin(a.Co, a.Cout);
    a.join = r->join; a.elu = elu ? 1 : 0; a.f16 = a.f16_in = (r->flags & TETRIS_RES_F16) ? 1 : 0;
    if (op == RES_FWD) { a.x = r->d_x; a.w = r->d_w; a.bias = r->d_bias; a.out = r->d_out; }
    else if (op == RES_GRAD_X) { a.g = r->d_grad_out; a.y = r->d_y; a.w = r->d_w; a.out = r->d_grad_x; }
    else { a.x = r->d_x; a.g = r->d_grad_out; a.y = r->d_y; a.grad_w = r->d_grad_w; a.grad_b = r->d_grad_b; }
    return TETRIS_OK;
}
// A call over host memory (the CPU build of the bodies: tests/cpu_harness), the product's launches as loops over image rows or over
// the rows of grad_w.  The arrays read are widened to float32 once, and e is formed once (res_e of a formed e is that e), so the
// serial forms' inner loops are plain float32.  tetris_lib_compose.h says which side runs what.
static inline int res_run_serial(const ResArgs& in) {
    ResArgs a = in;
    const size_t pos = (size_t)a.M * a.Hp * RES_W;
    std::vector<float> x, w, e;
    auto widen = [&](const void* p, size_t n, std::vector<float>& v) {
        v.resize(n);
        for (size_t i = 0; i < n; i++) v[i] = act_element(p, i, in.f16);
    };
    if (a.op != RES_GRAD_X) { widen(in.x, pos * a.Ci, x); a.x = x.data(); }
    if (a.op != RES_GRAD_W) { widen(in.w, (size_t)RES_TAPS * a.Ci * a.Co, w); a.w = w.data(); }
    if (a.op != RES_FWD) {
        e.resize(pos * a.Cout);
        for (size_t i = 0; i < e.size(); i++) e[i] = res_e_at(in, i);
        a.g = e.data(); a.y = nullptr; a.elu = 0;
    }
    a.f16_in = 0;
    if (a.op == RES_FWD) {
        for (int m = 0; m < a.M; m++)
            for (int h = 0; h < a.Hp; h++) res_forward_row_serial(a, (size_t)m, h);
    } else if (a.op == RES_GRAD_X) {
        for (int m = 0; m < a.M; m++)
            for (int h = 0; h < a.Hp; h++) res_grad_x_row_serial(a, (size_t)m, h);
    } else {
        for (int t = 0; t < RES_TAPS; t++)
            for (int ci = 0; ci < a.Ci; ci++) res_grad_w_row_serial(a, t / 3, t % 3, ci);
        res_grad_b_serial(a);
    }
    return TETRIS_OK;
}

// ---------------------------------------------------------------- rollout, split stages, RNG tables, flag words
static inline int rollout_launch_check(int launches, int steps_per_launch) {
    if (launches < 1 || steps_per_launch < 0) return fail(TETRIS_E_ARG, "launches must be >= 1, steps_per_launch >= 0");
    if (steps_per_launch > 256) return fail(TETRIS_E_ARG, "steps_per_launch must be <= 256");
    return TETRIS_OK;
}
// The low-water margin of the RNG tables for the launches of one call: raised to `need` draws, put back on every return path.
// A step may consume 2 piece draws per player, and the host learns of a board that came close to the end of the tables only
// through the flag words, up to 2 * group + 1 launches late (gate_launch): rollout_margin covers what those launches can consume.
template <class B>          // (either side's tetris_batch)
struct MarginGuard {
    B* b; uint32_t saved;
    MarginGuard(B* b, uint32_t need) : b(b), saved(b->margin) { if (b->margin < need) b->margin = need; }
    ~MarginGuard() { b->margin = saved; }
};
// tetris_split_stage_dev's own rule, then those of both split calls
static inline int split_step_check(int stage, const uint8_t* d_rot, const uint8_t* d_trans) {
    if ((stage == 0 || stage == 3) && (!d_rot || !d_trans)) return fail(TETRIS_E_ARG, "stages 0 and 3 need rot/trans (stage 3: of the NEXT step)");
    return TETRIS_OK;
}
static inline int split_stage_check(const HostShape& s, int side, int stage, const uint32_t* const d_words[4], const uint32_t* d_out) {
    if (!s.split) return fail(TETRIS_E_ARG, "not a split batch (tetris_create_split)");
    if (stage < 0 || stage > 3) return fail(TETRIS_E_ARG, "stage must be 0, 1, 2 or 3 (= 2 of this step + 0 of the next)");
    if (stage != 2 && !d_out) return fail(TETRIS_E_ARG, "stages 0, 1 and 3 need d_out");
    // words a stage reads: stage 1 = both A words (+ player 0's B on side 1); stages 2 and 3 = the opponent's B
    if (stage > 0 && !d_words) return fail(TETRIS_E_ARG, "stages 1, 2 and 3 need d_words");
    if (stage == 1 && (!d_words[0] || !d_words[1] || (side == 1 && !d_words[2]))) return fail(TETRIS_E_ARG, "stage 1 needs both A words (and player 0's B words on side 1)");
    if (stage >= 2 && !d_words[side == 0 ? 3 : 2]) return fail(TETRIS_E_ARG, "stages 2 and 3 need the opponent's B words");
    return TETRIS_OK;
}
static inline int table_limit_check(int chunks) {
    if (chunks < 0 || chunks > MAX_CHUNKS) return fail(TETRIS_E_ARG, "chunks must be 0..64");
    return TETRIS_OK;
}
// draws of the RNG tables a batch's kernels may use (KArgs::n_draws)
static inline uint32_t table_draws(int n_chunks, int table_limit) { return (uint32_t)(n_chunks < table_limit ? n_chunks : table_limit) * CHUNK; }

// F_BADARG, read and cleared at the end of a call
template <class W>
static inline int take_capacity_error(W* f) {
    if (!f[F_BADARG]) return TETRIS_OK;
    f[F_BADARG] = 0;
    return fail(TETRIS_E_ARG, "output capacity exceeded (max_lists / max_keys too small)");
}
// tetris_take_errors: the sticky flag words, read and cleared, as TETRIS_ERR_* bits (W: the product's words are volatile)
static inline int take_errors_check(const uint32_t* bits) {
    if (!bits) return fail(TETRIS_E_ARG, "bits is NULL");
    return TETRIS_OK;
}
template <class W>
static inline uint32_t take_error_bits(W* f) {
    const uint32_t bits = (f[F_FIFO] ? TETRIS_ERR_FIFO : 0u) | (f[F_EXHAUSTED] ? TETRIS_ERR_STREAM : 0u) | (f[F_LISTS] ? TETRIS_ERR_LISTS : 0u);
    f[F_FIFO] = 0; f[F_EXHAUSTED] = 0; f[F_LISTS] = 0;
    return bits;
}

}  // namespace te
