// Host side of the CPU harness, part 3 (as tetris_lib_core.h): the core entry points: create / destroy, settings and test aids (most
// of them no-ops here), split stages, reset, steps, observations, snapshots, drop enumeration, key lists; at the end, the exports only
// the harness has.  Needs harness_lib_batch.h.  "Device" pointers are host pointers here.

extern "C" {

int tetris_device_count(void) { return 0; }
int tetris_device_name(int, char* buf, int len) { if (buf && len > 0) snprintf(buf, (size_t)len, "cpu test harness (g++ build of the kernel bodies, no GPU)"); return TETRIS_OK; }
int tetris_table_chunks(const tetris_batch* b) { return b ? b->tab->n_chunks : 0; }
void* tetris_device_state(tetris_batch* b) { return b ? b->state.data() : nullptr; }
void* tetris_stream(tetris_batch*) { return nullptr; }

static int create_impl(tetris_batch** out, int n_games, int n_players, int height, int width, const uint8_t piece_map[7],
                       int /*device*/, const int16_t* seeds, int split, int side, int flags = 0) {
    int rc = create_check(out, n_games, n_players, height, width, piece_map, split, side, flags);
    if (rc) return rc;
    tetris_batch* b = new tetris_batch();
    b->N = n_games; b->P = n_players; b->H = height;
    b->tint = (flags & TETRIS_FLAG_COLOURS) ? 1 : 0; b->nw = b->tint ? NWORDS_TINT : NWORDS;
    b->state.assign(state_words((size_t)n_games, n_players, b->nw), 0);
    b->gstate.assign(gstate_words((size_t)n_games), 0);
    b->tab = tables_for(piece_map);
    b->split = split; b->side = side;
    if (split && side == 1) b->shadow.assign((size_t)(UNDO_WORDS + b->nw) * (size_t)n_games, 0);
    KArgs a = base_args(b, n_games, nullptr);
    a.seeds = seeds; a.steps = side;
    if (split) run<M_SPLIT_INIT>(b, a); else run<M_INIT>(b, a);
    if ((rc = finish_call(b))) { delete b; return rc; }
    *out = b;
    return TETRIS_OK;
}

int tetris_set_stream(tetris_batch*, void*, int) { return TETRIS_OK; }
static int split_stage_run(tetris_batch* b, int stage, KArgs& a, const uint32_t* const words[4], uint32_t* outw) {
    int rc = split_stage_check(shape_of(b), b->side, stage, words, outw);
    if (rc) return rc;
    for (int k = 0; k < 4; k++) a.xw[k] = words ? words[k] : nullptr;
    a.shadow = b->shadow.data(); a.xout = outw; a.split_side = b->side;
    for (int i = 0; i < b->N; i++) with_value<0, 3>(stage, [&](auto STAGE) { split_body<STAGE()>(a, i, SHAPES.s); });
    return TETRIS_OK;
}
int tetris_split_stage_dev(tetris_batch* b, int stage, const uint8_t* rot, const uint8_t* trans, const uint8_t* acting, int ms,
                           const uint32_t* const words[4], uint32_t* outw, uint8_t* done, uint8_t* lines, uint8_t* dead) {
    int rc = split_step_check(stage, rot, trans);
    if (rc) return rc;
    KArgs a = base_args(b, b->N, nullptr);
    a.rot = rot; a.trans = trans; a.player = acting; a.ms = ms; a.done = done; a.lines = lines; a.dead = dead;
    return split_stage_run(b, stage, a, words, outw);
}
int tetris_split_rollout_stage_dev(tetris_batch* b, int stage, uint32_t policy_seed, uint64_t step, int ms, const uint32_t* const words[4],
                                   uint32_t* outw) {
    KArgs a = base_args(b, b->N, nullptr);
    a.ms = ms; a.policy_seed = policy_seed; a.first_step = step; a.steps = 1;
    return split_stage_run(b, stage, a, words, outw);
}
int tetris_rollout_totals(tetris_batch* b, uint64_t totals[4]) {
    totals[0] = totals[1] = totals[2] = totals[3] = 0;
    for (int i = 0; i < b->N; i++) {
        unsigned long long t[4];
        totals_of_game(geo_of_batch(b), i, t);
        for (int k = 0; k < 4; k++) totals[k] += t[k];
    }
    return TETRIS_OK;
}
int tetris_destroy(tetris_batch* b) { delete b; return TETRIS_OK; }
int tetris_sync(tetris_batch* b) { return finish_call(b); }
int tetris_take_errors(tetris_batch* b, uint32_t* bits) {
    int rc = take_errors_check(bits);
    if (rc) return rc;
    *bits = take_error_bits(b->flags);
    return TETRIS_OK;
}
int tetris_set_chained(tetris_batch*, int) { return TETRIS_OK; }
int tetris_set_chain_spin_limit(tetris_batch*, uint32_t) { return TETRIS_OK; }
int tetris_set_direct_dispatch(tetris_batch*, int) { return TETRIS_OK; }
int tetris_rollout_was_direct(tetris_batch*) { return 0; }
int tetris_set_xcd_affine(tetris_batch*, int) { return TETRIS_OK; }
int tetris_debug_xcd_skew(tetris_batch*, int) { return TETRIS_OK; }
int tetris_debug_table_limit(tetris_batch* b, int chunks) {
    int rc = table_limit_check(chunks);
    if (rc) return rc;
    b->table_limit = chunks ? chunks : MAX_CHUNKS;
    return TETRIS_OK;
}
int tetris_debug_code_objects(int* count, uint64_t* bytes) { if (count) *count = 0; if (bytes) *bytes = 0; return TETRIS_OK; }
int tetris_debug_stall(tetris_batch*, int, int, int) { return TETRIS_OK; }
int tetris_debug_chain_epoch(tetris_batch*, long long, uint32_t*) { return fail(TETRIS_E_ARG, "chained launches exist on the GPU only"); }
int tetris_debug_clock_khz(tetris_batch*, int* khz) { if (khz) *khz = 0; return TETRIS_OK; }
int tetris_rollout_is_chained(tetris_batch*, int) { return 0; }
int tetris_set_game_offset(tetris_batch* b, uint64_t first) { b->game_offset = (uint32_t)first; return TETRIS_OK; }

static int check_idx(tetris_batch* b, const int32_t* idx, int n) { return check_idx(shape_of(b), idx, n); }

int tetris_reset(tetris_batch* b, const int32_t* idx, int n, const int16_t* seeds) {
    int rc = check_idx(b, idx, n); if (rc) return rc;
    KArgs a = base_args(b, n, idx); a.seeds = seeds;
    if (b->split) run<M_SPLIT_RESET>(b, a); else run<M_RESET>(b, a);
    return finish_call(b);
}

int tetris_make_actions(tetris_batch* b, const int32_t* idx, int n, const uint8_t* keys, const uint8_t* lens, int max_keys) {
    int rc = check_idx(b, idx, n); if (rc) return rc;
    KArgs a = base_args(b, n, idx); KeyStage s;
    if ((rc = stage_keys(b, n, keys, lens, max_keys, a, s))) return rc;
    run<M_MAKE>(b, a);
    return finish_call(b);
}

int tetris_finish_actions(tetris_batch* b, const int32_t* idx, int n, int ms, uint8_t* done, uint8_t* lines, uint8_t* dead) {
    int rc = check_idx(b, idx, n); if (rc) return rc;
    KArgs a = base_args(b, n, idx); a.ms = ms; OutStage o; stage_out(b, n, a, o);
    run<M_FINISH>(b, a);
    fetch_out(b, n, o, done, lines, dead);
    return finish_call(b);
}

int tetris_step_keys(tetris_batch* b, const int32_t* idx, int n, const uint8_t* keys, const uint8_t* lens, int max_keys, int ms,
                     uint8_t* done, uint8_t* lines, uint8_t* dead) {
    int rc = check_idx(b, idx, n); if (rc) return rc;
    KArgs a = base_args(b, n, idx); a.ms = ms; KeyStage s; OutStage o;
    if ((rc = stage_keys(b, n, keys, lens, max_keys, a, s))) return rc;
    stage_out(b, n, a, o);
    run<M_STEP_KEYS>(b, a);
    fetch_out(b, n, o, done, lines, dead);
    return finish_call(b);
}

int tetris_step_rt(tetris_batch* b, const uint8_t* rot, const uint8_t* trans, const uint8_t* player, int ms, uint8_t* done,
                   uint8_t* lines, uint8_t* dead) {
    int rc = step_rt_check(shape_of(b), rot, trans, 0);
    if (rc || (rc = check_players(shape_of(b), player, b->N))) return rc;
    KArgs a = base_args(b, b->N, nullptr); a.ms = ms; a.rot = rot; a.trans = trans; a.player = player;
    OutStage o; stage_out(b, b->N, a, o);
    run<M_STEP_RT>(b, a);
    fetch_out(b, b->N, o, done, lines, dead);
    return finish_call(b);
}

int tetris_step_rt_dev_ex(tetris_batch* b, const uint8_t* rot, const uint8_t* trans, const uint8_t* player, int ms, uint8_t* done,
                          uint8_t* lines, uint8_t* dead, int flags) {
    int rc = step_rt_check(shape_of(b), rot, trans, flags);
    if (rc || (rc = finish_call(b))) return rc;          // (the product polls its flag words here instead)
    KArgs a = base_args(b, b->N, nullptr); a.ms = ms; a.rot = rot; a.trans = trans; a.player = player;
    a.done = done; a.lines = lines; a.dead = dead;
    if (flags & TETRIS_STEP_AUTO_RESET) run<M_STEP_RT_AUTO>(b, a); else run<M_STEP_RT>(b, a);
    return TETRIS_OK;
}
int tetris_reset_dev(tetris_batch* b, const uint8_t* mask, const int16_t* seeds) {
    int rc = not_on_split(shape_of(b), "tetris_reset_dev");
    if (rc || (rc = finish_call(b))) return rc;
    KArgs a = base_args(b, b->N, nullptr); a.mask = mask; a.seeds = seeds;
    if (seeds) run<M_RESET>(b, a); else run<M_RESET_SCHED>(b, a);
    return TETRIS_OK;
}

int tetris_observe_records(tetris_batch* b, const int32_t* idx, int n, tetris_record* records, uint8_t* round_over,
                           int8_t* last_winner) {
    int rc = check_idx(b, idx, n); if (rc) return rc;
    for (int i = 0; i < n; i++) {
        const Geo geo = geo_of_batch(b);
        with_shape<1, 4>(b->P, b->tint != 0, [&](auto P, auto TINT) {
            observe_body<P(), TINT()>(geo, i, idx, b->H, SHAPES.s, records, round_over, last_winner);
        });
    }
    return TETRIS_OK;
}

int tetris_snapshot(tetris_batch* b, const int32_t* idx, int n, uint32_t* blob) {
    int rc = check_idx(b, idx, n); if (rc) return rc;
    size_t total = (size_t)n * (NGWORDS + b->P * b->nw);
    for (size_t t = 0; t < total; t++) snapshot_body(geo_of_batch(b), t, idx, blob, 0);
    return TETRIS_OK;
}
int tetris_restore(tetris_batch* b, const int32_t* idx, int n, const uint32_t* blob) {
    int rc = check_idx(b, idx, n); if (rc) return rc;
    size_t total = (size_t)n * (NGWORDS + b->P * b->nw);
    for (size_t t = 0; t < total; t++) snapshot_body(geo_of_batch(b), t, idx, (uint32_t*)blob, 1);
    return TETRIS_OK;
}
int tetris_set_dead(tetris_batch* b, const int32_t* idx, int n, const uint8_t* dead) {
    int rc = check_idx(b, idx, n); if (rc) return rc;
    for (int t = 0; t < n * b->P; t++) set_dead_body(geo_of_batch(b), t, idx, dead);
    return TETRIS_OK;
}

int tetris_enumerate_drops_dev_ex(tetris_batch* b, const int32_t* idx, int n, const uint8_t* player, uint8_t* valid, int8_t* land_y,
                                  uint8_t* cleared, uint32_t* after, int flags) {
    int rc = enumerate_check(shape_of(b), idx != nullptr, n, valid, land_y, cleared, after, flags);
    if (rc || (rc = check_idx(b, idx, n))) return rc;        // (the indices are host memory here)
    for (int i = 0; i < n; i++)
        with_value<1, 4>(b->P, [&](auto P) {
            enumerate_body<P()>(geo_of_batch(b), i, n, idx, player, b->H, SHAPES.s, valid, land_y, cleared, after, flags & TETRIS_ENUM_PLANAR);
        });
    return TETRIS_OK;
}
int tetris_enumerate_drops(tetris_batch* b, const int32_t* idx, int n, const uint8_t* player, uint8_t* valid, int8_t* land_y,
                           uint8_t* cleared, uint32_t* after) {
    int rc = enumerate_check(shape_of(b), idx != nullptr, n, valid, land_y, cleared, after, 0);
    if (rc || (rc = check_idx(b, idx, n)) || (rc = check_players(shape_of(b), player, n))) return rc;
    return tetris_enumerate_drops_dev_ex(b, idx, n, player, valid, land_y, cleared, after, 0);
}
int tetris_timer_start(tetris_batch*) { return TETRIS_OK; }
int tetris_timer_stop(tetris_batch*, float* ms) { if (ms) *ms = 0.0f; return TETRIS_OK; }

int tetris_get_actions(tetris_batch* b, const int32_t* idx, int n, const uint8_t* player, uint8_t* keys, uint8_t* lens, int32_t* count,
                       int max_lists, int max_keys) {
    int rc = get_actions_check(shape_of(b), idx != nullptr, n, player, keys, lens, count, max_lists, max_keys);
    if (rc || (rc = check_idx(b, idx, n))) return rc;
    const size_t lanes = (size_t)n * 40;
    std::vector<uint8_t> hc(lanes), hl(lanes * PLAN_LANE_LISTS), hk(lanes * PLAN_LANE_LISTS * max_keys);
    for (size_t t = 0; t < lanes; t++)
        with_value<1, 4>(b->P, [&](auto P) {
            actions_body<P()>(geo_of_batch(b), t, idx, player, b->H, SHAPES.s, hc.data(), hl.data(), hk.data(), PLAN_LANE_LISTS, max_keys, b->flags);
        });
    if ((rc = take_capacity_error(b->flags))) return rc;
    return get_actions_gather(n, hc.data(), hl.data(), hk.data(), max_lists, max_keys, keys, lens, count);
}

int tetris_observe_packed_dev(tetris_batch* b, const int32_t* idx, int n, const uint8_t* player, uint8_t* visual, uint8_t* vector,
                              uint8_t* piece) {
    int rc = observe_packed_check(shape_of(b), idx != nullptr, n, visual, vector, piece);
    if (rc || (rc = check_idx(b, idx, n))) return rc;        // (the indices are host memory here)
    const int cells = b->H * NCOL;
    for (int sl = 0; sl < b->P; sl++)
        for (int i = 0; i < n; i++) {
            size_t slot = idx ? (size_t)idx[i] : (size_t)i;
            int me = player ? player[i] : 0;
            int p = sl == 0 ? me : b->P - 1 - me;
            piece[(size_t)sl * n + i] = (uint8_t)observe_board(geo_of_batch(b), slot, p, b->H,
                                                               visual + ((size_t)sl * n + i) * cells, vector + ((size_t)sl * n + i) * 12);
        }
    return TETRIS_OK;
}
int tetris_observe_packed(tetris_batch* b, const int32_t* idx, int n, const uint8_t* player, uint8_t* visual, uint8_t* vector,
                          uint8_t* piece) {
    int rc = observe_packed_outputs_check(visual, vector, piece);
    if (rc || (rc = check_idx(b, idx, n)) || (rc = check_players(shape_of(b), player, n))) return rc;
    return tetris_observe_packed_dev(b, idx, n, player, visual, vector, piece);
}

int tetris_step_rt_observe_dev(tetris_batch* b, const uint8_t* rot, const uint8_t* trans, const uint8_t* player, int ms, uint8_t* done,
                               uint8_t* lines, uint8_t* dead, int flags, const uint8_t* next_player, uint8_t* visual, uint8_t* vector,
                               uint8_t* piece) {
    int rc = step_rt_observe_check(shape_of(b), rot, trans, flags, visual, vector, piece);
    if (rc) return rc;
    rc = tetris_step_rt_dev_ex(b, rot, trans, player, ms, done, lines, dead, flags);       // (the product fuses the two kernels)
    if (rc) return rc;
    return tetris_observe_packed_dev(b, nullptr, b->N, next_player, visual, vector, piece);
}

// ---------------------------------------------------------------- exports only the harness has
// test-only: reads (and clears) the key-interpreter path counters of tetris_engine.h
void harness_path_counts(unsigned long long* out) {
    for (int i = 0; i < PC_NCOUNTERS; i++) { out[i] = te_path_count[i]; te_path_count[i] = 0; }
}

// mask bytes per workgroup of the product's selection kernels: the sizes around which tests/test_traj_batch.py puts its shapes
extern const int tetris_harness_select_elems = SELECT_ELEMS;

// entries per workgroup of the product's sort, and the number of tiles past which its scan carries: the sizes around which
// tests/test_prio_replay.py puts its shapes
extern const int tetris_harness_sort_tile = SORT_TILE;
extern const int tetris_harness_sort_scan_span = SORT_SCAN_SPAN;

}  // extern "C"
