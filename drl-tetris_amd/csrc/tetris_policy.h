// Kernel bodies of the device-side heuristic policy (include/tetris_hip.h: tetris_rt_features_dev, tetris_policy_rt_dev,
// tetris_step_policy_dev, tetris_rollout_policy, tetris_rollout_game_totals_dev): a one-piece look-ahead over the 40 SVENton
// (rotation, translation) actions, each candidate field reduced to TETRIS_POLICY_FEATURES integer features and scored by a
// dot product with int16 weights — what tests/golden/policies.py:GreedyRT does on the CPU oracle, one game at a time.
//
// `__host__ __device__` like tetris_plan.h: tetris_hip.hip / tetris_hip_multi.hip wrap these in gfx950 kernels,
// tests/cpu_harness/harness_lib_agent.h in plain host loops.
//
// Two mappings over the same bodies (DESIGN.md §4 has the measurements):
//   spread  one lane per (game, candidate), a wave = 64 consecutive games of one candidate (policy_eval_lane: 12 cached loads,
//           play_rt, the reduction; features or a score out), then one lane per game that takes the maximum of its 40 scores
//           (policy_pick_lane) and, in the same lane, steps (policy_step_lane with FROM_SCORES);
//   lane    one lane per game that evaluates its 40 candidates itself on a register copy of the acting board and steps
//           (policy_step_lane without FROM_SCORES): the form of fused rollout launches, where the state stays in registers
//           between the steps of a launch.
// No floating point, no arrays indexed at run time (nothing here needs scratch memory).
#pragma once
#include "tetris_kernels.h"

namespace te {

constexpr int POLICY_FEATURES = TETRIS_POLICY_FEATURES;
constexpr int POLICY_CANDIDATES = 40;            // c = 10 r + t

struct PolicyArgs {
    KArgs a;                    // state, tables, status words, H, N (a.n = N), ms, done / lines / dead outputs, game offset, steps
    const uint8_t* player;      // [N] acting player (NULL: player 0; clamped)
    int fixed_player;           // >= 0: the acting player of every game instead (a rollout step: step mod P); -1: player[]
    const int16_t* weights;     // [8], or [N][8] with per_game
    int per_game;
    int16_t* features;          // [40][8][N] (tetris_rt_features_dev)
    int32_t* scores;            // [40][N]: the spread mapping's hand-over from the evaluation to the choice
    uint8_t* rot;               // [N] the choice (may be NULL in the step kernels)
    uint8_t* trans;             // [N]
    int32_t* score;             // [N] (may be NULL)
};

// What a candidate evaluation needs of the acting player's board: occupancy and the piece's pose.  `can`: the key interpreter
// runs at all (make_rt: the round is not over and the player is alive); otherwise every candidate field is the board as it is.
struct PolicyBoard {
    uint32_t col[NCOL];
    int kind, rot, x, y;
    bool can;
};

template <int P>
TE_HD PolicyBoard policy_board_of(const Game<P>& g, int player) {
    PolicyBoard b;
    for (int c = 0; c < NCOL; c++) b.col[c] = 0;
    b.kind = 0; b.rot = 0; b.x = 0; b.y = 0; b.can = false;
    TE_UNROLL
    for (int p = 0; p < P; p++)
        if (p == player) {
            const Player& q = g.pl[p];
            for (int c = 0; c < NCOL; c++) b.col[c] = q.col[c];
            b.kind = q.kind; b.rot = q.rot; b.x = q.x; b.y = q.y;
            b.can = !g.round_over && !q.dead;
        }
    return b;
}

// the same from memory, for a lane that holds nothing else of the game: plain cached loads (the 40 waves of a block of games
// read the same twelve rows)
TE_HD PolicyBoard policy_board_load(const Geo& geo, size_t slot, int player) {
    PolicyBoard b;
    const Ref br = board_ref(geo, player, slot);
    for (int c = 0; c < NCOL; c++) b.col[c] = word_at(br, W_COL0 + c);
    const uint32_t w = word_at(br, W_PIECE);                          // as load_player unpacks it
    b.kind = w & 7; b.rot = (w >> 3) & 3; b.x = (int)((w >> 5) & 15) - 4; b.y = (w >> 9) & 31;
    const uint32_t meta = word_at(game_ref(geo, slot), G_META);       // as load_game_words
    b.can = !((meta >> 16) & 1u) && !((w >> 17) & 1u);
    return b;
}

// The candidate field of c = 10 r + t: make_action of [8]*r + [2] + [3]*t + [7] without finish_action — play_rt on a copy.
// The piece is stamped, full rows are still present.  `cx.tint` must be false (occupancy only).
TE_HD void policy_candidate(const Ctx& cx, const PolicyBoard& b, int r, int t, uint32_t col[NCOL]) {
    Player q;
    for (int c = 0; c < NCOL; c++) q.col[c] = b.col[c];
    q.kind = b.kind; q.rot = b.rot; q.x = b.x; q.y = b.y;
    q.time_ms = 0; q.drop_time = 0; q.lock_armed = 0;
    if (b.can) play_rt(cx, q, r, t);
    for (int c = 0; c < NCOL; c++) col[c] = q.col[c];
}

TE_HD int policy_popc(uint32_t v) { return __builtin_popcount(v); }

// The eight features of a field given as column words (bit y = row y, row 0 = the top; include/tetris_hip.h has the table).
// Feature 0 is counted on the field as it is; for the others the full rows are removed first: per column a bit compaction
// by the mask of full rows, one full row at a time from the top (the bits above it move down by one).
TE_HD void policy_features(const uint32_t col_in[NCOL], int H, int f[POLICY_FEATURES]) {
    const uint32_t rows = ~(~0u << H);                  // H <= 31
    uint32_t col[NCOL];
    uint32_t full = rows;
    TE_UNROLL
    for (int c = 0; c < NCOL; c++) { col[c] = col_in[c] & rows; full &= col[c]; }
    f[0] = policy_popc(full);
    while (full) {
        const int y = ctz32(full);
        full &= full - 1u;
        const uint32_t above = (1u << y) - 1u;          // rows 0..y-1
        const uint32_t keep = ~((above << 1) | 1u);     // rows y+1..
        TE_UNROLL
        for (int c = 0; c < NCOL; c++) col[c] = (col[c] & keep) | ((col[c] & above) << 1);
    }
    int h[NCOL];
    int holes = 0, agg = 0, mx = 0, coltr = 0;
    TE_UNROLL
    for (int c = 0; c < NCOL; c++) {
        h[c] = col[c] ? H - ctz32(col[c]) : 0;
        holes += h[c] - policy_popc(col[c]);            // the cells from the topmost filled one down to the floor, less the filled ones
        agg += h[c];
        mx = imax(mx, h[c]);
        const uint32_t with_floor = col[c] | (1u << H);
        coltr += policy_popc((with_floor ^ (with_floor >> 1)) & rows);
    }
    int bump = 0, wells = 0;
    int rowtr = policy_popc(~col[0] & rows) + policy_popc(~col[NCOL - 1] & rows);     // the walls count as filled
    TE_UNROLL
    for (int c = 0; c < NCOL; c++) {
        if (c + 1 < NCOL) {
            const int d = h[c + 1] - h[c];
            bump += d < 0 ? -d : d;
            rowtr += policy_popc(col[c] ^ col[c + 1]);
        }
        const int left = c > 0 ? h[c - 1] : H, right = c + 1 < NCOL ? h[c + 1] : H;
        const int d = imax(0, imin(left, right) - h[c]);
        wells += d * (d + 1) / 2;
    }
    f[1] = holes; f[2] = bump; f[3] = agg; f[4] = mx; f[5] = rowtr; f[6] = coltr; f[7] = wells;
}

// weights of game i: one vector for the batch or one per game
TE_HD void policy_weights(const PolicyArgs& pa, int i, int w[POLICY_FEATURES]) {
    const int16_t* p = pa.weights + (pa.per_game ? (size_t)i * POLICY_FEATURES : (size_t)0);
    TE_UNROLL
    for (int k = 0; k < POLICY_FEATURES; k++) w[k] = p[k];
}

// sum of w[k] * f[k] in int32 (no overflow for H <= 31: the largest feature is 4 960)
TE_HD int32_t policy_score(const int w[POLICY_FEATURES], const int f[POLICY_FEATURES]) {
    int32_t s = 0;
    TE_UNROLL
    for (int k = 0; k < POLICY_FEATURES; k++) s += w[k] * f[k];
    return s;
}

TE_HD Ctx policy_probe_ctx(const Ctx& cx) {
    Ctx pc = cx;
    pc.tint = false;                // candidates are stamped into a copy of the occupancy alone
    return pc;
}

// ---------------------------------------------------------------- spread mapping: lane = (game i, candidate c)
// FEAT: the eight features to features[c][k][i]; otherwise the score to scores[c][i].  Nothing of the batch's state is written.
template <bool FEAT>
TE_HD void policy_eval_lane(const PolicyArgs& pa, int i, int c, const uint32_t* shapes) {
    const KArgs& a = pa.a;
    const int player = pa.fixed_player >= 0 ? safe_player_value(pa.fixed_player, a.n_players) : safe_player(pa.player, i, a.n_players);
    const PolicyBoard b = policy_board_load(geo_of(a), (size_t)i, player);
    const Ctx cx = make_ctx(a, shapes, false, true);
    uint32_t col[NCOL];
    policy_candidate(cx, b, c / 10, c % 10, col);
    int f[POLICY_FEATURES];
    policy_features(col, a.H, f);
    const size_t n = (size_t)a.n;
    if (FEAT) {
        TE_UNROLL
        for (int k = 0; k < POLICY_FEATURES; k++) pa.features[((size_t)c * POLICY_FEATURES + k) * n + i] = (int16_t)f[k];
    } else {
        int w[POLICY_FEATURES];
        policy_weights(pa, i, w);
        pa.scores[(size_t)c * n + i] = policy_score(w, f);
    }
}

// the highest of game i's 40 scores, among equals the lowest c
TE_HD int policy_pick_scores(const PolicyArgs& pa, int i, int32_t& best) {
    const size_t n = (size_t)pa.a.n;
    int bc = 0;
    best = pa.scores[i];
    for (int c = 1; c < POLICY_CANDIDATES; c++) {
        const int32_t s = pa.scores[(size_t)c * n + i];
        if (s > best) { best = s; bc = c; }
    }
    return bc;
}

// ---------------------------------------------------------------- lane mapping: the 40 candidates of one game in its own lane
TE_HD int policy_pick_board(const Ctx& cx, const PolicyBoard& b, const int w[POLICY_FEATURES], int H, int32_t& best) {
    const Ctx pc = policy_probe_ctx(cx);
    int bc = 0;
    best = 0;
    for (int c = 0; c < POLICY_CANDIDATES; c++) {
        uint32_t col[NCOL];
        policy_candidate(pc, b, c / 10, c % 10, col);
        int f[POLICY_FEATURES];
        policy_features(col, H, f);
        const int32_t s = policy_score(w, f);
        if (c == 0 || s > best) { best = s; bc = c; }
    }
    return bc;
}

TE_HD void policy_write_choice(const PolicyArgs& pa, int i, int c, int32_t score) {
    if (pa.rot) pa.rot[i] = (uint8_t)(c / 10);
    if (pa.trans) pa.trans[i] = (uint8_t)(c % 10);
    if (pa.score) pa.score[i] = score;
}

// tetris_policy_rt_dev, second kernel of the spread mapping
TE_HD void policy_pick_lane(const PolicyArgs& pa, int i) {
    int32_t best;
    const int c = policy_pick_scores(pa, i, best);
    policy_write_choice(pa, i, c, best);
}

// ---------------------------------------------------------------- the step with (r, t) taken from the choice
// ROLL = false: the body of M_STEP_RT / M_STEP_RT_AUTO (prefetches, make_rt, finish_game, outputs before the reset) for
// pa.player[i].  ROLL = true: a.steps steps of the body of M_ROLLOUT (acting player = step mod P, per-game counter words,
// auto-reset) with the policy's choice in place of the Philox draw.  FROM_SCORES: the choice is the maximum of scores[..][i]
// (spread mapping; one step per launch); otherwise the lane evaluates its candidates itself.
template <int P, bool TINT, bool ROLL, bool AUTO, bool FROM_SCORES>
TE_HD void policy_step_lane(const PolicyArgs& pa, int i, const uint32_t* shapes, bool /*consecutive: unused, see plan_sim_lane*/) {
    const KArgs& a = pa.a;
    Game<P> g;
    load_game<P>(geo_of(a), (size_t)i, g, TINT, P > 1, ROLL);
    const Ctx cx = make_ctx(a, shapes, TINT, P > 1);
    int w[POLICY_FEATURES];
    if (!FROM_SCORES) policy_weights(pa, i, w);
    const int steps = ROLL ? a.steps : 1;
    uint32_t earlier = 0;            // the status bits of the launch's earlier steps (g.status is one step's: see game_run)
    for (int s = 0; s < steps; s++) {
        if (ROLL) { earlier |= g.status; g.status = 0; }
        const unsigned long long step = a.first_step + (unsigned long long)s;
        const int player = ROLL ? (P > 1 ? (int)(step % (unsigned long long)P) : 0) : safe_player(pa.player, i, P);
        int32_t best;
        const int c = FROM_SCORES ? policy_pick_scores(pa, i, best) : policy_pick_board(cx, policy_board_of<P>(g, player), w, a.H, best);
        if (!ROLL) policy_write_choice(pa, i, c, best);
        TE_UNROLL
        for (int p = 0; p < P; p++) prefetch_next(cx, g.pl[p], g.seed16, g.status);
        ResetPrefetch rpf;
        rpf.ok = 0; rpf.seed16 = 0; rpf.word = 0;
        if (AUTO) prefetch_reset(cx, episode_seed(a.game_offset + (uint32_t)i, g.episode + 1), rpf);
        uint32_t sent_before = 0;
        TE_UNROLL
        for (int p = 0; p < P; p++) sent_before += g.pl[p].lines_sent;
        make_rt<P>(cx, g, player, c / 10, c % 10);
        const int done = finish_game<P>(cx, g, a.ms);
        if (!ROLL) write_outputs<P>(a, i, g, done);          // done / lines / dead as they stand BEFORE the reset
        if (ROLL) {
            g.steps++;
            uint32_t sent_after = 0;
            TE_UNROLL
            for (int p = 0; p < P; p++) {
                sent_after += g.pl[p].lines_sent;
                if (!g.pl[p].dead) g.add_lines += (unsigned)g.pl[p].reward;
            }
            g.add_sent += (sent_after - sent_before) & 0xFFFFu;
        }
        if (AUTO && done) {                                  // worker.py:157-166 reset_envs, without the host round trip
            g.episode++;
            reset_game<P>(cx, g, episode_seed(a.game_offset + (uint32_t)i, g.episode), &rpf);
        }
    }
    store_game<P>(geo_of(a), (size_t)i, g, TINT, P > 1, ROLL);
    report_status(a, g.status | earlier);
}

// tetris_rollout_game_totals_dev: totals[k][i] = the per-game word tetris_rollout_totals sums
TE_HD void policy_game_totals_lane(const Geo& geo, int i, uint32_t* totals) {
    unsigned long long t[4];
    totals_of_game(geo, i, t);
    for (int k = 0; k < 4; k++) totals[(size_t)k * geo.n_games + i] = (uint32_t)t[k];
}

}  // namespace te
