// Kernel bodies of the planning entry points (include/tetris_hip.h: tetris_action_lists_dev, tetris_simulate_lists_dev,
// tetris_step_lists_dev, tetris_plan_deltas_dev): the afterstate loop of a planning agent on the device.  The reference's sherlock agent asks the
// environment, per decision and game, for the ordered key lists of the current piece (get_actions), for the afterstate of
// every list (simulate_all_actions) and then performs the one it picked (perform_action)
// (agents/sherlock_agent/sherlock_agent.py:94-120, sherlock_utils.py:9-20).
//
// `__host__ __device__` like tetris_kernels.h: tetris_hip.hip / tetris_hip_multi.hip wrap these in gfx950 kernels,
// tests/cpu_harness/harness_lib_agent.h in plain host loops.
//
// Lists of one game live at lens[i][L] and keys[i][L][K] (L = max_lists, K = max_keys), count[i] of them (-1: the game's
// lists did not fit).  The per-(game, x, rotation) search is actions_body (k_actions), which writes "slabs": for lane
// t = (game, r * 10 + xi), cnt[t] lists at slab_lens[t][PLAN_LANE_LISTS], slab_keys[t][PLAN_LANE_LISTS][KS].
#pragma once
#include "tetris_kernels.h"

namespace te {

constexpr int PLAN_LANE_LISTS = 16;     // lists one (x, rotation) start can produce (<= H / 2 + 1 for H <= 31; as tetris_get_actions)
constexpr int PLAN_RAW_MAX = 40 * PLAN_LANE_LISTS;

struct PlanArgs {
    KArgs a;                    // state, tables, status words, H, N (a.n = N), ms, done / lines / dead outputs, game offset
    const uint8_t* player;      // [N] acting player (NULL: player 0; clamped)
    const int32_t* count;       // [N] lists per game (as tetris_action_lists_dev wrote them)
    const uint8_t* lens;        // [N][L]
    const uint8_t* keys;        // [N][L][K]
    const int32_t* choice;      // [N] (step)
    uint32_t* cols;             // [L][P][10][N] (simulate)
    int max_lists, max_keys;
};

// ---------------------------------------------------------------- lists: compaction of the slabs of one game
// The reference enumerates x-major, rotation-minor (tetris_get_actions): raw list order j = xi * 4 + r, slab lane r * 10 + xi.
TE_HD int plan_slab_lane(int j) { return (j & 3) * 10 + (j >> 2); }

// key list equality, the test data_types.action_list's `in` makes on two actions
TE_HD bool plan_same_list(const uint8_t* ka, int la, const uint8_t* kb, int lb) {
    if (la != lb) return false;
    for (int j = 0; j < la; j++)
        if (ka[j] != kb[j]) return false;
    return true;
}
TE_HD bool plan_is_null(const uint8_t* k, int len) { return len == 1 && k[0] == 0; }    // data_types.null_action = [0]

// FNV-1a over the keys and the length: the GPU compaction compares hashes before keys
TE_HD uint32_t plan_list_hash(const uint8_t* k, int len) {
    uint32_t h = 2166136261u ^ (uint32_t)len;
    for (int j = 0; j < len; j++) h = (h ^ k[j]) * 16777619u;
    return h;
}

// writes list `o` of game g (lens / keys of the caller's [N][L][K] arrays)
TE_HD void plan_write_list(uint8_t* lens, uint8_t* keys, size_t g, int L, int K, int o, const uint8_t* src, int len) {
    lens[g * (size_t)L + o] = (uint8_t)len;
    uint8_t* dst = keys + (g * (size_t)L + o) * (size_t)K;
    for (int j = 0; j < len; j++) dst[j] = src[j];
}
TE_HD void plan_write_null(uint8_t* lens, uint8_t* keys, size_t g, int L, int K) {
    lens[g * (size_t)L] = 1;
    keys[g * (size_t)L * K] = 0;
}

// A game's lists did not fit the caller's buffers: count -1, TETRIS_ERR_LISTS (plain store to the flag words, as report_status)
TE_HD void plan_report_overflow(uint32_t* status) { ((volatile uint32_t*)status)[F_LISTS] = 1u; }

// Serial form of the compaction of game `g` (CPU harness; the GPU kernel k_plan_lists spreads the same steps over a wave).
// Slabs of the game start at lane t0 = local game * 40; KS = slab key width (max_keys + 1, so that a list longer than
// max_keys shows as one).  data_types.action_list(lists, remove_null) (action_list.py:3-37, data_types.py:27-51):
//   - the null action [0] goes in front unless the lists already hold it; duplicates are dropped, first occurrence kept;
//   - remove_null: every null action is dropped again, unless nothing else is left (then the list is [[0]]).
TE_HD void plan_compact_serial(const uint8_t* cnt, const uint8_t* slab_lens, const uint8_t* slab_keys, int KS, size_t t0, size_t g,
                               int L, int K, bool keep_null, int32_t* count, uint8_t* lens, uint8_t* keys, uint32_t* status) {
    int off[41];
    bool bad = false;
    off[0] = 0;
    for (int j = 0; j < 40; j++) {
        const int c = cnt[t0 + plan_slab_lane(j)];
        bad |= c > PLAN_LANE_LISTS;
        off[j + 1] = off[j] + (c > PLAN_LANE_LISTS ? 0 : c);
    }
    const int M = off[40];
    // raw list m -> its keys and length
    auto raw = [&](int m, int& len) -> const uint8_t* {
        int j = 0;
        while (off[j + 1] <= m) j++;
        const size_t s = (t0 + plan_slab_lane(j)) * PLAN_LANE_LISTS + (m - off[j]);
        len = slab_lens[s];
        return slab_keys + s * KS;
    };
    bool has_null = false;
    int n_out = 0;
    for (int m = 0; m < M; m++) {
        int len;
        const uint8_t* k = raw(m, len);
        bad |= len > K;
        has_null |= plan_is_null(k, len);
    }
    // pass 1 counts, pass 2 writes (nothing is written for a game that does not fit)
    for (int pass = 0; pass < 2; pass++) {
        int o = (!keep_null || has_null) ? 0 : 1;
        for (int m = 0; m < M && !bad; m++) {
            int len;
            const uint8_t* k = raw(m, len);
            if (!keep_null && plan_is_null(k, len)) continue;
            bool first = true;
            for (int e = 0; e < m && first; e++) {
                int le;
                const uint8_t* ke = raw(e, le);
                first = !plan_same_list(k, len, ke, le);
            }
            if (!first) continue;
            if (pass == 1) plan_write_list(lens, keys, g, L, K, o, k, len);
            o++;
        }
        if (o == 0) {                         // nothing but nulls (or nothing): [[0]]
            if (pass == 1) plan_write_null(lens, keys, g, L, K);
            o = 1;
        } else if (pass == 1 && keep_null && !has_null)
            plan_write_null(lens, keys, g, L, K);
        if (pass == 0) {
            n_out = o;
            bad |= n_out > L;
            if (bad) break;
        }
    }
    count[g] = bad ? -1 : n_out;
    if (bad) plan_report_overflow(status);
}

// ---------------------------------------------------------------- simulate / step: the key interpreter on a list
// PythonHandle.cpp:138-147 make_action with `len` keys at `kp` (NULL: the null action [0]) for `player` and [0] for everyone
// else (tetris_environment.py:106-108), as make_keys does for the staged [K][P][n] keys.
template <int P>
TE_HD void plan_make_keys(const Ctx& cx, Game<P>& g, int player, const uint8_t* kp, int len) {
    if (g.round_over) return;
    TE_UNROLL
    for (int p = 0; p < P; p++) {
        Player& q = g.pl[p];
        if (q.dead) continue;
        if (p == player && kp) for (int k = 0; k < len; k++) press_key(cx, q, kp[k]);
        else press_key(cx, q, 0);
    }
}

// list k of game i; its length is clamped to the caller's max_keys
TE_HD const uint8_t* plan_list(const PlanArgs& pa, int i, int k, int& len) {
    len = pa.lens[(size_t)i * pa.max_lists + k];
    if (len > pa.max_keys) len = pa.max_keys;
    return pa.keys + ((size_t)i * pa.max_lists + k) * (size_t)pa.max_keys;
}

// simulate_actions(lists, player, finalize) (tetris_environment.py:87-100) of list k of game i, on a register copy of the
// game: loads as game_load does, runs make_keys (and with `fin`, finish_game as M_STEP_KEYS does), stores the columns of
// every player to cols[k][p][c][i] and, with `fin`, done[k][i] / lines[k][p][i] / dead[k][p][i].  Nothing of the batch's
// state is written.  The trailing bool of the *_lane functions (do the wave's lanes hold consecutive games?) is unused since the
// tiles layout went; it stays because the CPU harness under tests/ passes it.
template <int P, bool TINT>
TE_HD void plan_sim_lane(const PlanArgs& pa, int i, int k, bool fin, const uint32_t* shapes, bool /*consecutive*/) {
    const KArgs& a = pa.a;
    const int c = pa.count[i];
    if (k >= c) return;                                    // (count -1: nothing)
    Game<P> g;
    load_game<P>(geo_of(a), (size_t)i, g, TINT, P > 1, false);
    const Ctx cx = make_ctx(a, shapes, TINT, P > 1);
    const int player = safe_player(pa.player, i, P);
    if (fin) {
        TE_UNROLL
        for (int p = 0; p < P; p++) prefetch_next(cx, g.pl[p], g.seed16, g.status);
    }
    int len;
    const uint8_t* kp = plan_list(pa, i, k, len);
    plan_make_keys<P>(cx, g, player, kp, len);
    const size_t n = (size_t)a.n;
    if (fin) {
        const int done = finish_game<P>(cx, g, a.ms);
        if (a.done) a.done[(size_t)k * n + i] = (uint8_t)done;
        TE_UNROLL
        for (int p = 0; p < P; p++) {
            if (a.lines) a.lines[((size_t)k * P + p) * n + i] = (uint8_t)g.pl[p].reward;
            if (a.dead) a.dead[((size_t)k * P + p) * n + i] = (uint8_t)g.pl[p].dead;
        }
    }
    TE_UNROLL
    for (int p = 0; p < P; p++)
        for (int col = 0; col < NCOL; col++) pa.cols[(((size_t)k * P + p) * NCOL + col) * n + i] = g.pl[p].col[col];
    // a simulated afterstate that runs over a capacity limit says so in its `done`; no game of the batch was ended (nothing is
    // stored), so tetris_take_errors has nothing to report.  The request to extend the tables stands.
    report_status(a, g.status & ~(uint32_t)(ST_STREAM_EXHAUSTED | ST_FIFO_OVERFLOW));
}

// perform_action(lists[choice[i]], player) (tetris_environment.py:102-116): the step of M_STEP_KEYS with the chosen list for
// the acting player and [0] for the others; AUTO: the reset of M_STEP_RT_AUTO in the same pass (seed schedule of
// include/tetris_hip.h); done / lines / dead describe the step before the reset.  choice is clamped into [0, count - 1]; a
// game whose lists did not fit (count < 1) performs the null action.
template <int P, bool TINT, bool AUTO>
TE_HD void plan_step_lane(const PlanArgs& pa, int i, const uint32_t* shapes, bool /*consecutive*/) {
    const KArgs& a = pa.a;
    Game<P> g;
    load_game<P>(geo_of(a), (size_t)i, g, TINT, P > 1, false);
    const Ctx cx = make_ctx(a, shapes, TINT, P > 1);
    TE_UNROLL
    for (int p = 0; p < P; p++) prefetch_next(cx, g.pl[p], g.seed16, g.status);
    ResetPrefetch rpf;
    rpf.ok = 0; rpf.seed16 = 0; rpf.word = 0;
    if (AUTO) prefetch_reset(cx, episode_seed(a.game_offset + (uint32_t)i, g.episode + 1), rpf);
    const int player = safe_player(pa.player, i, P);
    const int c = imin(pa.count[i], pa.max_lists);
    int len = 1;
    const uint8_t* kp = nullptr;
    if (c >= 1) kp = plan_list(pa, i, imax(0, imin(pa.choice[i], c - 1)), len);
    plan_make_keys<P>(cx, g, player, kp, len);
    const int done = finish_game<P>(cx, g, a.ms);
    write_outputs<P>(a, i, g, done);
    if (AUTO && done) {                                    // worker.py:157-166 reset_envs, without the host round trip
        g.episode++;
        reset_game<P>(cx, g, episode_seed(a.game_offset + (uint32_t)i, g.episode), &rpf);
    }
    store_game<P>(geo_of(a), (size_t)i, g, TINT, P > 1, false);
    report_status(a, g.status);
}

// ---------------------------------------------------------------- deltas: simulated columns -> the network input of a planning agent
// sherlock_utils.deltas / generate_deltas (agents/sherlock_agent/sherlock_utils.py:9-20), per game and list: the acting player's
// field after the list minus the field before; a list whose difference adds up to less than 4 is `small_fill` everywhere; lists
// past count are zero; sums = the sum over the lists.  The element logic below is shared by k_plan_deltas (tetris_dev_agent_plan.h) and
// the host loop of tests/cpu_harness/harness_lib_agent.h, so that both give the same bits.
struct PlanDeltaArgs {
    Geo geo;
    int H, n;                   // rows of a board, games
    const uint8_t* player;      // [N] acting player (NULL: player 0; clamped)
    const int32_t* count;       // [N] lists per game (clamped into [0, L])
    const uint32_t* cols;       // [L][P][10][N] (as plan_sim_lane wrote them)
    int max_lists;              // L
    float small_fill;
    void* deltas;               // [N][H][W][L], list-major [N][L][H][W]; float32 or binary16
    void* sums;                 // [N][H][W] (NULL: no sums)
    uint8_t* small;             // [N][L] (NULL: not wanted)
};

enum PlanListKind : int { PLAN_LIST_NORMAL = 0, PLAN_LIST_SMALL = 1, PLAN_LIST_PAST = 2 };

TE_HD uint32_t plan_row_mask(int H) { return H >= 32 ? ~0u : (1u << H) - 1u; }                 // rows 0..H-1 of a column word
// the delta of cell (y, column): bit y of the column after minus bit y of the column before, in {-1, 0, 1}
TE_HD int plan_cell_delta(uint32_t after, uint32_t before, int y) { return (int)((after >> y) & 1u) - (int)((before >> y) & 1u); }
// the integer sum of a list's deltas, from its (masked) columns
TE_HD int plan_list_sum(const uint32_t* after, const uint32_t* before) {
    int s = 0;
    TE_UNROLL
    for (int c = 0; c < NCOL; c++) s += __builtin_popcount(after[c]) - __builtin_popcount(before[c]);
    return s;
}
// the "fewer than 4 cells" rule (sherlock_utils.py:12-14: the piece did not land whole, or the player could not move)
TE_HD int plan_list_kind(int k, int count, int sum) { return k >= count ? PLAN_LIST_PAST : sum < 4 ? PLAN_LIST_SMALL : PLAN_LIST_NORMAL; }
TE_HD int plan_clamp_count(int count, int L) { return imax(0, imin(count, L)); }
// one cell of list `kind`
TE_HD float plan_delta_value(int kind, int delta, float small_fill) {
    return kind == PLAN_LIST_NORMAL ? (float)delta : kind == PLAN_LIST_SMALL ? small_fill : 0.0f;
}
// one cell of the sums: `normal_sum` = the integer sum of the cell's deltas over the normal lists, n_small = the small lists.
// One float32 multiply and one float32 add (the builds use -ffp-contract=off), so no reduction order enters.
TE_HD float plan_sums_value(int normal_sum, int n_small, float small_fill) {
    const float fill = small_fill * (float)n_small;
    return (float)normal_sum + fill;
}
// float32 -> IEEE binary16 bits, round to nearest even, in integer arithmetic (the host compiler of the CPU harness has no
// half type; the kernel uses the same function so that both give the same bits)
TE_HD uint16_t plan_f32_to_f16(float f) {
    uint32_t x = f2u(f);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7FFFFFFFu;
    if (x > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);                  // NaN
    if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                 // >= 65520 rounds to infinity
    if (x >= 0x38800000u) {                                                  // a normal half: rebias, round the 13 dropped bits
        const uint32_t m = x - 0x38000000u;
        return (uint16_t)(sign | ((m + 0xFFFu + ((m >> 13) & 1u)) >> 13));
    }
    const uint32_t shift = 126u - (x >> 23);                                 // a subnormal half: units of 2^-24
    if (shift > 24u) return (uint16_t)sign;                                  // below 2^-25: zero
    const uint32_t mant = (x & 0x7FFFFFu) | 0x800000u;
    uint32_t q = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (q & 1u))) q++;
    return (uint16_t)(sign | q);
}
// an output element of type T (float, or uint16_t = binary16 bits) from the float32 value
TE_HD void plan_encode_to(float v, float& out) { out = v; }
TE_HD void plan_encode_to(float v, uint16_t& out) { out = plan_f32_to_f16(v); }
template <typename T>
TE_HD T plan_encode(float v) {
    T out;
    plan_encode_to(v, out);
    return out;
}

// Serial form of game i (CPU harness; k_plan_deltas spreads the same steps over a workgroup).
template <typename T>
TE_HD void plan_deltas_game(const PlanDeltaArgs& da, int i, bool list_major) {
    const int H = da.H, L = da.max_lists, P = da.geo.P, HW = H * NCOL;
    const size_t n = (size_t)da.n;
    const int p = safe_player(da.player, i, P);
    const int count = plan_clamp_count(da.count[i], L);
    const uint32_t mask = plan_row_mask(H);
    const Ref br = board_ref(da.geo, p, (size_t)i);
    uint32_t before[NCOL], after[NCOL];
    for (int c = 0; c < NCOL; c++) before[c] = word_at(br, W_COL0 + c) & mask;
    T* out = (T*)da.deltas + (size_t)i * HW * L;
    int n_small = 0;
    int acc[MAX_H * NCOL];
    for (int t = 0; t < HW; t++) acc[t] = 0;
    for (int k = 0; k < L; k++) {
        int sum = 0;
        if (k < count) {
            for (int c = 0; c < NCOL; c++) after[c] = da.cols[(((size_t)k * P + p) * NCOL + c) * n + i] & mask;
            sum = plan_list_sum(after, before);
        }
        const int kind = plan_list_kind(k, count, sum);
        n_small += kind == PLAN_LIST_SMALL;
        if (da.small) da.small[(size_t)i * L + k] = (uint8_t)(kind == PLAN_LIST_SMALL);
        for (int t = 0; t < HW; t++) {
            const int d = kind == PLAN_LIST_NORMAL ? plan_cell_delta(after[t % NCOL], before[t % NCOL], t / NCOL) : 0;
            acc[t] += d;
            out[list_major ? (size_t)k * HW + t : (size_t)t * L + k] = plan_encode<T>(plan_delta_value(kind, d, da.small_fill));
        }
    }
    if (da.sums)
        for (int t = 0; t < HW; t++) ((T*)da.sums)[(size_t)i * HW + t] = plan_encode<T>(plan_sums_value(acc[t], n_small, da.small_fill));
}

}  // namespace te
