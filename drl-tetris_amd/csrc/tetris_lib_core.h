// Host side of libtetris_hip.so, part 3: the core entry points: create / destroy, settings and test aids, split stages, reset, steps,
// observations, snapshots, drop enumeration, key lists.  Needs tetris_lib_batch.h and tetris_lib_rollout.h.

extern "C" {

int tetris_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(TETRIS_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return n;
}

int tetris_device_name(int device, char* buf, int len) {
    if (!buf || len < 1) return fail(TETRIS_E_ARG, "buf/len");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    snprintf(buf, (size_t)len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return TETRIS_OK;
}

int tetris_table_chunks(const tetris_batch* b) { return b && b->tab ? b->tab->n_chunks : 0; }
void* tetris_device_state(tetris_batch* b) { return b ? b->d_state : nullptr; }
void* tetris_stream(tetris_batch* b) { return b ? (void*)b->stream : nullptr; }

int tetris_destroy(tetris_batch* b) {
    if (!b) return TETRIS_OK;
    (void)hipSetDevice(b->device);
    for (hipStream_t st : b->chain_stream) if (st) (void)hipStreamSynchronize(st);      // (a call that failed half-way may have left launches there)
    chain_release(b);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->tab) tables_release(b->tab);
    (void)hipFree(b->d_shadow); (void)hipFree(b->d_state); (void)hipFree(b->d_gstate); (void)hipFree(b->d_counters);
    if (b->flags) (void)hipHostFree(b->flags);
    if (b->h_counters) (void)hipHostFree(b->h_counters);
    for (hipEvent_t e : b->gate_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : b->chain_ev) if (e) (void)hipEventDestroy(e);
    for (auto& pair : b->worker_gate_ev) for (hipEvent_t e : pair) if (e) (void)hipEventDestroy(e);
    (void)hipFree(b->d_chain);
    free(b->h_chain);
    if (b->stall_stream) { (void)hipStreamSynchronize(b->stall_stream); (void)hipStreamDestroy(b->stall_stream); }
    if (b->direct_used) { aql::Device* dev = aql::device_for(b->device); if (dev->ok) aql::quiesce(dev->qs); }      // (a test's idle kernel may still sit there)
    b->release_scratch();
    for (Stage& s : b->stage) s.release();
    b->recover_idx.release();
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
    delete b;
    return TETRIS_OK;
}

static int default_direct_min() {
    const char* off = getenv("TETRIS_DIRECT");
    if (off && off[0] == '0') return 0;
    const char* e = getenv("TETRIS_DIRECT_MIN");
    const int v = e ? atoi(e) : 16;
    return v < 1 ? 16 : v;
}

static int create_impl(tetris_batch** out, int n_games, int n_players, int height, int width, const uint8_t piece_map[7],
                       int device, const int16_t* seeds, int split, int side, int flags = 0) {
    int rc = create_check(out, n_games, n_players, height, width, piece_map, split, side, flags);
    if (rc) return rc;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(TETRIS_E_HIP, std::string("no HIP device available (this library has no CPU path): ") +
                                      (e != hipSuccess ? hipGetErrorString(e) : "device count 0"));
    if (device < 0 || device >= ndev) return fail(TETRIS_E_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    tetris_batch* b = new (std::nothrow) tetris_batch();
    if (!b) return fail(TETRIS_E_HIP, "out of host memory");
    b->device = device; b->N = n_games; b->P = n_players; b->H = height;
    b->stride = n_games;
    b->tint = (flags & TETRIS_FLAG_COLOURS) ? 1 : 0;
    { const char* e = getenv("TETRIS_NO_DUO"); b->use_duo = !(e && e[0] == '1'); }
    { const char* e = getenv("TETRIS_NO_CHAIN"); b->use_chain = !(e && e[0] == '1'); }
    b->direct_min = default_direct_min();
    { const char* e = getenv("TETRIS_AFFINE"); b->use_affine = !(e && e[0] == '0'); }
    { const char* e = getenv("TETRIS_GRAPH"); b->use_graph = (e && e[0] == '1'); }
    { const char* e = getenv("TETRIS_CHAIN_SPIN_LIMIT"); if (e && atoll(e) > 0) b->chain_spin_limit = (uint32_t)atoll(e); }
    b->nw = b->tint ? NWORDS_TINT : NWORDS;
#define CREATE_TRY(expr)                                                                    \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            tetris_destroy(b);                                                              \
            return fail(TETRIS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
        }                                                                                   \
    } while (0)
    CREATE_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    b->own_stream = b->stream;
    CREATE_TRY(hipEventCreate(&b->ev0));
    CREATE_TRY(hipEventCreate(&b->ev1));
    {   // the chain streams belong to the DEVICE (device_chain_streams below): every batch of a device uses the same three
        hipError_t ce = device_chain_streams(device, b->chain_stream);
        CREATE_TRY(ce);
    }
    for (int k = 0; k < CHAIN_STREAMS + 1; k++) CREATE_TRY(hipEventCreateWithFlags(&b->chain_ev[k], hipEventDisableTiming));
    for (int k = 0; k < CHAIN_STREAMS; k++) for (int j = 0; j < 2; j++) CREATE_TRY(hipEventCreateWithFlags(&b->worker_gate_ev[k][j], hipEventDisableTiming));
    {
        const size_t chain_bytes = (((size_t)n_games + 15) / 16) * sizeof(uint32_t) * CHAIN_STRIDE;       // (one word per wave; at least 16 games per wave)
        CREATE_TRY(hipMalloc((void**)&b->d_chain, chain_bytes));
        CREATE_TRY(hipMemsetAsync(b->d_chain, 0, chain_bytes, b->stream));
    }
    CREATE_TRY(hipEventCreateWithFlags(&b->gate_ev[0], hipEventDisableTiming));
    CREATE_TRY(hipEventCreateWithFlags(&b->gate_ev[1], hipEventDisableTiming));
    const size_t state_bytes = state_words((size_t)b->stride, n_players, b->nw) * 4, gstate_bytes = gstate_words((size_t)b->stride) * 4;
    CREATE_TRY(hipMalloc((void**)&b->d_state, state_bytes));
    CREATE_TRY(hipMalloc((void**)&b->d_gstate, gstate_bytes));
    CREATE_TRY(hipMalloc((void**)&b->d_counters, 8 * sizeof(unsigned long long)));
    CREATE_TRY(hipHostMalloc((void**)&b->h_counters, 8 * sizeof(unsigned long long), hipHostMallocDefault));
    // flag words: host memory the GPU can write (fine-grained, so a store is visible to the host while the kernel runs)
    CREATE_TRY(hipHostMalloc((void**)&b->flags, NFLAGS * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
    memset(b->flags, 0, NFLAGS * sizeof(uint32_t));
    CREATE_TRY(hipMemsetAsync(b->d_gstate, 0, gstate_bytes, b->stream));
    CREATE_TRY(hipMemsetAsync(b->d_state, 0, state_bytes, b->stream));
    rc = tables_acquire(&b->tab, device, piece_map, b->stream);
    if (rc) { std::string keep = g_err; tetris_destroy(b); return fail(rc, keep); }
    HostCall io{b};
    const int16_t* d_seeds;
    if ((rc = io.in(seeds, (size_t)n_games, &d_seeds))) { std::string keep = g_err; tetris_destroy(b); return fail(rc, keep); }
    b->split = split; b->side = side;
    if (split && side == 1) CREATE_TRY(hipMalloc((void**)&b->d_shadow, (size_t)(UNDO_WORDS + b->nw) * (size_t)b->stride * 4));
    KArgs a = base_args(b, n_games, nullptr);
    a.seeds = d_seeds;
    a.steps = side;
    rc = split ? launch_game<M_SPLIT_INIT>(b, a) : launch_game<M_INIT>(b, a);
    if (!rc) rc = io.finish();
    if (rc) { std::string keep = g_err; tetris_destroy(b); return fail(rc, keep); }
    *out = b;
    return TETRIS_OK;
}

int tetris_set_chained(tetris_batch* b, int on) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = finish_call(b))) return rc;
    b->use_chain = on ? 1 : 0;
    return TETRIS_OK;
}

int tetris_set_direct_dispatch(tetris_batch* b, int min_launches) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = finish_call(b))) return rc;
    b->direct_min = min_launches < 0 ? default_direct_min() : min_launches;
    return TETRIS_OK;
}

int tetris_set_xcd_affine(tetris_batch* b, int on) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = finish_call(b))) return rc;
    b->use_affine = on ? 1 : 0;
    return TETRIS_OK;
}

int tetris_debug_xcd_skew(tetris_batch* b, int skew) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = finish_call(b))) return rc;
    b->xcd_skew = (uint32_t)skew & 7u;
    return TETRIS_OK;
}

int tetris_debug_table_limit(tetris_batch* b, int chunks) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = table_limit_check(chunks)) || (rc = finish_call(b))) return rc;
    b->table_limit = chunks ? chunks : MAX_CHUNKS;
    return TETRIS_OK;
}

int tetris_debug_code_objects(int* count, uint64_t* bytes) {
    if (!count || !bytes) return fail(TETRIS_E_ARG, "count / bytes is NULL");
    std::vector<std::vector<char>> images;
    std::string why;
    *count = 0; *bytes = 0;
    if (!aql::own_code_objects(images, why)) return TETRIS_OK;      // (none: the caller sees count == 0)
    *count = (int)images.size();
    for (auto& img : images) *bytes += img.size();
    return TETRIS_OK;
}

int tetris_rollout_was_direct(tetris_batch* b) {
    int rc = check_batch(b, false);
    if (rc) return rc;
    return b->last_direct ? (b->last_affine ? 2 : 1) : 0;
}

int tetris_set_chain_spin_limit(tetris_batch* b, uint32_t polls) {
    int rc = check_batch(b, false);
    if (rc) return rc;
    if ((rc = finish_call(b))) return rc;
    b->chain_spin_limit = polls ? polls : CHAIN_SPIN_LIMIT;
    return TETRIS_OK;
}

// Test aid (tests of the give-up path of chained launches; nothing in the product calls it): enqueues a kernel that does nothing for
// `microseconds` — which = 0..2: on that chain stream (the launches the next rollout puts there start late); 3: on the batch's
// stream; -1: on a stream of its own, as 1024-thread workgroups that take `percent` % of the device's wave slots meanwhile.
int tetris_debug_stall(tetris_batch* b, int which, int microseconds, int percent) {
    int rc = check_batch(b);
    if (rc) return rc;
    if (which < -1 || which > 3 || microseconds < 0 || microseconds > 2000000 || percent < 0 || percent > 100) return fail(TETRIS_E_ARG, "which / microseconds / percent");
    const unsigned long long ticks = (unsigned long long)microseconds * 100ull;
    if (which >= 0 && which < 3 && b->direct_min > 0) {
        // the device's own queues (tetris_aql.h), if they exist: the idle kernel goes to the one that stands for that stream as well —
        // whichever way the next call's launches go, the ones with that number start late
        aql::Device* dev = aql::device_for(b->device);
        std::string why;
        if (dev->ok && aql::make_queues(dev, why) && dev->blocker.ok) {
            struct { const uint32_t* go; unsigned long long ticks; } args = {nullptr, ticks};
            aql::Pending pd;
            aql::write_dispatch(dev->qs, pd, which, dev->blocker, &args, sizeof args, 1, HSA_FENCE_SCOPE_AGENT, HSA_FENCE_SCOPE_AGENT, hsa_signal_t{});
            aql::ring(dev->qs, pd);
            b->direct_used = true;
        }
    }
    if (which >= 0) {
        hipStream_t st = which == 3 ? b->stream : b->chain_stream[which % CHAIN_STREAMS];
        if (which < 3) b->chain_pending = true;
        return launch_on(st, k_blocker, dim3(1), dim3(64), 0, (const uint32_t*)nullptr, ticks);
    }
    if (!b->stall_stream) HIP_TRY(hipStreamCreateWithFlags(&b->stall_stream, hipStreamNonBlocking));
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
    const int blocks = (int)((long long)cus * 2 * percent / 100);        // 2 x 1024 threads = the 32 wave slots of a CU
    return blocks > 0 ? launch_on(b->stall_stream, k_blocker, dim3((unsigned)blocks), dim3(1024), 0, (const uint32_t*)nullptr, ticks) : launched();
}

// Test aid (tests of the restart of the epoch numbering, tetris_rollout_launch; nothing in the product calls it): at a drained point
// every wave's epoch word and the batch's count of chained launches become `set_epoch`, the way chain_recover leaves them.
int tetris_debug_chain_epoch(tetris_batch* b, long long set_epoch, uint32_t* epoch) {
    int rc = check_batch(b);
    if (rc) return rc;
    if (set_epoch >= (long long)CHAIN_EPOCH_MAX) return fail(TETRIS_E_ARG, "set_epoch must be below 0x7FFF0000");
    if ((rc = finish_call(b))) return rc;
    if (set_epoch >= 0) {
        hipStream_t const home = b->own_stream;
        HIP_TRY(hipStreamSynchronize(b->stream));
        for (int k = 0; k < CHAIN_STREAMS; k++) HIP_TRY(hipStreamSynchronize(b->chain_stream[k]));
        HIP_TRY(hipStreamSynchronize(home));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)b->d_chain, (int)set_epoch, (((size_t)b->N + 15) / 16) * CHAIN_STRIDE, home));
        HIP_TRY(hipStreamSynchronize(home));
        b->chain_epoch = (uint32_t)set_epoch;
    }
    if (epoch) *epoch = b->chain_epoch;
    return TETRIS_OK;
}

// Measurement aid: the GPU's shader clock right now, in kHz (a 50 us probe kernel on the batch's stream; synchronous).  The
// chained period follows it: DESIGN.md, section 6.
int tetris_debug_clock_khz(tetris_batch* b, int* khz) {
    int rc = check_batch(b);
    if (rc) return rc;
    if (!khz) return fail(TETRIS_E_ARG, "khz is NULL");
    HIP_TRY(hipMemsetAsync(b->d_counters + 4, 0, 2 * sizeof(unsigned long long), b->stream));
    if ((rc = launch(b, k_clock_probe, dim3(1), dim3(64), 0, 5000ull, b->d_counters + 4))) return rc;
    HIP_TRY(hipMemcpyAsync(b->h_counters + 4, b->d_counters + 4, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
    if ((rc = finish_call(b))) return rc;
    *khz = b->h_counters[5] ? (int)(b->h_counters[4] * 100000ull / b->h_counters[5]) : 0;
    return TETRIS_OK;
}

int tetris_set_game_offset(tetris_batch* b, uint64_t first_game_id) {
    if (!b) return fail(TETRIS_E_ARG, "null batch");
    b->game_offset = (uint32_t)first_game_id;
    return TETRIS_OK;
}

int tetris_set_stream(tetris_batch* b, void* hip_stream, int external) {
    int rc = check_batch(b);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->stream = external ? (hipStream_t)hip_stream : b->own_stream;      // NULL + external = the legacy default stream
    return TETRIS_OK;
}

static int split_stage_launch(tetris_batch* b, int stage, KArgs& a, const uint32_t* const d_words[4], uint32_t* d_out) {
    int rc = split_stage_check(shape_of(b), b->side, stage, d_words, d_out);
    if (rc) return rc;
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;
    for (int k = 0; k < 4; k++) a.xw[k] = d_words ? d_words[k] : nullptr;
    a.shadow = b->d_shadow; a.xout = d_out; a.split_side = b->side;
    dim3 grid(blocks_for(b->N)), block(256);
    with_value<0, 3>(stage, [&](auto STAGE) { hipLaunchKernelGGL((k_split<STAGE(), false>), grid, block, 0, b->stream, a); });
    return launched();
}

// the arguments of a step of all games by (rot, trans) actions in device arrays
static KArgs step_args(tetris_batch* b, const uint8_t* d_rot, const uint8_t* d_trans, const uint8_t* d_player, int ms, uint8_t* d_done,
                       uint8_t* d_lines, uint8_t* d_dead) {
    KArgs a = base_args(b, b->N, nullptr);
    a.rot = d_rot; a.trans = d_trans; a.player = d_player; a.ms = ms;
    a.done = d_done; a.lines = d_lines; a.dead = d_dead;
    return a;
}

int tetris_split_stage_dev(tetris_batch* b, int stage, const uint8_t* d_rot, const uint8_t* d_trans, const uint8_t* d_acting, int ms,
                           const uint32_t* const d_words[4], uint32_t* d_out, uint8_t* d_done, uint8_t* d_lines, uint8_t* d_dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = split_step_check(stage, d_rot, d_trans))) return rc;
    KArgs a = step_args(b, d_rot, d_trans, d_acting, ms, d_done, d_lines, d_dead);
    return split_stage_launch(b, stage, a, d_words, d_out);
}

int tetris_split_rollout_stage_dev(tetris_batch* b, int stage, uint32_t policy_seed, uint64_t step, int ms, const uint32_t* const d_words[4],
                                   uint32_t* d_out) {
    int rc = check_batch(b);
    if (rc) return rc;
    KArgs a = base_args(b, b->N, nullptr);
    a.ms = ms; a.policy_seed = policy_seed; a.first_step = step; a.steps = 1;
    return split_stage_launch(b, stage, a, d_words, d_out);
}

int tetris_rollout_totals(tetris_batch* b, uint64_t totals[4]) {
    int rc = check_batch(b);
    if (rc) return rc;
    if (!totals) return fail(TETRIS_E_ARG, "totals is NULL");
    if ((rc = read_totals(b, nullptr))) return rc;
    for (int k = 0; k < 4; k++) totals[k] = b->h_counters[k];
    return TETRIS_OK;
}

int tetris_take_errors(tetris_batch* b, uint32_t* bits) {
    int rc = check_batch(b, false);
    if (rc) return rc;
    if ((rc = take_errors_check(bits)) || (rc = finish_call(b))) return rc;
    volatile uint32_t* f = b->flags;
    *bits = take_error_bits(f) | (b->chain_fell_back ? TETRIS_ERR_CHAIN_FELL_BACK : 0u);
    b->chain_fell_back = false;
    return TETRIS_OK;
}

int tetris_sync(tetris_batch* b) {
    int rc = check_batch(b, false);
    if (rc) return rc;
    return finish_call(b);
}

int tetris_reset(tetris_batch* b, const int32_t* idx, int n, const int16_t* seeds) {
    int rc = check_batch(b);
    if (rc) return rc;
    HostCall io{b};
    if ((rc = io.idx(idx, n))) return rc;
    if (n == 0) return io.finish();             // still a synchronisation point: sticky errors surface, tables get extended
    KArgs a = base_args(b, n, io.d_idx);
    if ((rc = io.in(seeds, (size_t)n, &a.seeds))) return rc;
    if ((rc = b->split ? launch_game<M_SPLIT_RESET>(b, a) : launch_game<M_RESET>(b, a))) return rc;
    return io.finish();
}

// host keys [n][P][K] -> device [K][P][n]; host lens [n][P] -> device [P][n]
static int stage_keys(HostCall& io, int n, const uint8_t* keys, const uint8_t* lens, int max_keys, KArgs& a) {
    int rc = keys_check(keys, lens, max_keys);
    if (rc) return rc;
    const int P = io.b->P;
    Stage *sk, *sl;
    if ((rc = io.take((size_t)n * P * max_keys, &sk)) || (rc = io.take((size_t)n * P, &sl))) return rc;
    if ((rc = keys_pack(shape_of(io.b), n, keys, lens, max_keys, (uint8_t*)sk->h, (uint8_t*)sl->h))) return rc;
    if ((rc = io.send(sk, (size_t)n * P * max_keys)) || (rc = io.send(sl, (size_t)n * P))) return rc;
    a.keys = (const uint8_t*)sk->d; a.lens = (const uint8_t*)sl->d; a.max_keys = max_keys;
    return TETRIS_OK;
}

int tetris_make_actions(tetris_batch* b, const int32_t* idx, int n, const uint8_t* keys, const uint8_t* lens, int max_keys) {
    int rc = check_batch(b);
    if (rc) return rc;
    HostCall io{b};
    if ((rc = io.idx(idx, n))) return rc;
    if (n == 0) return TETRIS_OK;
    KArgs a = base_args(b, n, io.d_idx);
    if ((rc = stage_keys(io, n, keys, lens, max_keys, a))) return rc;
    if ((rc = launch_game<M_MAKE>(b, a))) return rc;
    return io.finish();
}

int tetris_finish_actions(tetris_batch* b, const int32_t* idx, int n, int ms, uint8_t* done, uint8_t* lines, uint8_t* dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    HostCall io{b};
    if ((rc = io.idx(idx, n))) return rc;
    if (n == 0) return TETRIS_OK;
    KArgs a = base_args(b, n, io.d_idx);
    a.ms = ms;
    return finish_step<M_FINISH>(io, a, n, done, lines, dead);
}

int tetris_step_keys(tetris_batch* b, const int32_t* idx, int n, const uint8_t* keys, const uint8_t* lens, int max_keys,
                     int ms, uint8_t* done, uint8_t* lines, uint8_t* dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    HostCall io{b};
    if ((rc = io.idx(idx, n))) return rc;
    if (n == 0) return TETRIS_OK;
    KArgs a = base_args(b, n, io.d_idx);
    a.ms = ms;
    if ((rc = stage_keys(io, n, keys, lens, max_keys, a))) return rc;
    return finish_step<M_STEP_KEYS>(io, a, n, done, lines, dead);
}

int tetris_step_rt_dev_ex(tetris_batch* b, const uint8_t* d_rot, const uint8_t* d_trans, const uint8_t* d_player, int ms,
                          uint8_t* d_done, uint8_t* d_lines, uint8_t* d_dead, int flags) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = step_rt_check(shape_of(b), d_rot, d_trans, flags)) || (rc = enqueue(b, Enqueue::STEPS))) return rc;
    const KArgs a = step_args(b, d_rot, d_trans, d_player, ms, d_done, d_lines, d_dead);
    return (flags & TETRIS_STEP_AUTO_RESET) ? launch_game<M_STEP_RT_AUTO>(b, a) : launch_game<M_STEP_RT>(b, a);
}

int tetris_step_rt_observe_dev(tetris_batch* b, const uint8_t* d_rot, const uint8_t* d_trans, const uint8_t* d_player, int ms,
                               uint8_t* d_done, uint8_t* d_lines, uint8_t* d_dead, int flags, const uint8_t* d_next_player,
                               uint8_t* d_visual, uint8_t* d_vector, uint8_t* d_piece) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = step_rt_observe_check(shape_of(b), d_rot, d_trans, flags, d_visual, d_vector, d_piece))) return rc;
    const bool fused = !b->tint && b->H % 2 == 0 && ((uintptr_t)d_visual & 3u) == 0 && ((uintptr_t)d_vector & 3u) == 0;
    if (!fused) {             // colour batches, odd heights, unaligned outputs: the same two kernels back to back
        if ((rc = tetris_step_rt_dev_ex(b, d_rot, d_trans, d_player, ms, d_done, d_lines, d_dead, flags))) return rc;
        return tetris_observe_packed_dev(b, nullptr, b->N, d_next_player, d_visual, d_vector, d_piece);
    }
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    KArgs a = step_args(b, d_rot, d_trans, d_player, ms, d_done, d_lines, d_dead);
    a.next_player = d_next_player; a.obs_visual = d_visual; a.obs_vector = d_vector; a.obs_piece = d_piece;
    const int nw = b->H * NCOL / 4;
    const size_t lds = ((size_t)SHAPE_WORDS + (size_t)64 * nw) * 4;
    const dim3 grid(blocks_for(b->N, 64)), block(64);
    const bool autoreset = (flags & TETRIS_STEP_AUTO_RESET) != 0;
    if (b->P == 2 && b->use_duo) {
        // two players: one player per lane (k_duo) — every lane builds the one board it holds
        const size_t lds2 = ((size_t)4 * 64 * nw + 16) * 4;
        if (lds2 > 48 * 1024) {
            const void* fn = autoreset ? (const void*)k_duo<M_STEP_RT_AUTO, false, true> : (const void*)k_duo<M_STEP_RT, false, true>;
            HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
        }
        const dim3 grid2(blocks_for(b->N, 128)), block2(256);
        return autoreset ? launch(b, k_duo<M_STEP_RT_AUTO, false, true>, grid2, block2, lds2, a) : launch(b, k_duo<M_STEP_RT, false, true>, grid2, block2, lds2, a);
    }
    with_shape<1, 2>(b->P, autoreset, [&](auto P, auto AUTO) {
        hipLaunchKernelGGL((k_step_observe<P(), AUTO() ? M_STEP_RT_AUTO : M_STEP_RT>), grid, block, lds, b->stream, a);
    });
    return launched();
}

int tetris_reset_dev(tetris_batch* b, const uint8_t* d_mask, const int16_t* d_seeds) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = not_on_split(shape_of(b), "tetris_reset_dev")) || (rc = enqueue(b, Enqueue::STEPS))) return rc;
    KArgs a = base_args(b, b->N, nullptr);
    a.mask = d_mask; a.seeds = d_seeds;
    return d_seeds ? launch_game<M_RESET>(b, a) : launch_game<M_RESET_SCHED>(b, a);
}

int tetris_step_rt(tetris_batch* b, const uint8_t* rot, const uint8_t* trans, const uint8_t* player, int ms, uint8_t* done,
                   uint8_t* lines, uint8_t* dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    const int n = b->N;
    if ((rc = step_rt_check(shape_of(b), rot, trans, 0)) || (rc = check_players(shape_of(b), player, n))) return rc;
    KArgs a = base_args(b, n, nullptr);
    a.ms = ms;
    HostCall io{b};
    if ((rc = io.in(rot, (size_t)n, &a.rot)) || (rc = io.in(trans, (size_t)n, &a.trans)) || (rc = io.in(player, (size_t)n, &a.player))) return rc;
    return finish_step<M_STEP_RT>(io, a, n, done, lines, dead);
}

int tetris_observe_records(tetris_batch* b, const int32_t* idx, int n, tetris_record* records, uint8_t* round_over,
                           int8_t* last_winner) {
    int rc = check_batch(b);
    if (rc) return rc;
    HostCall io{b};
    if ((rc = io.idx(idx, n))) return rc;
    if (n == 0) return TETRIS_OK;
    const size_t rec_bytes = (size_t)n * b->P * sizeof(tetris_record);
    tetris_record* d_rec;
    uint8_t* d_round_over;
    int8_t* d_last_winner;
    Stage* rec;                         // (records NULL: the kernel writes them all the same, nothing copies them back)
    if ((rc = records ? io.out(records, (size_t)n * b->P, &d_rec) : io.take(rec_bytes, &rec))) return rc;
    if (!records) d_rec = (tetris_record*)rec->d;
    if ((rc = io.out(round_over, (size_t)n, &d_round_over)) || (rc = io.out(last_winner, (size_t)n, &d_last_winner))) return rc;
    dim3 grid(blocks_for(n)), block(256);
    HIP_TRY(hipMemsetAsync(d_rec, 0, rec_bytes, b->stream));      // struct padding stays deterministic
    with_shape<1, 4>(b->P, b->tint != 0, [&](auto P, auto TINT) {
        hipLaunchKernelGGL((k_observe<P(), TINT()>), grid, block, 0, b->stream, geo_of_batch(b), n, io.d_idx, b->H, d_rec, d_round_over, d_last_winner);
    });
    return (rc = launched()) ? rc : io.finish();
}

int tetris_observe_packed_dev(tetris_batch* b, const int32_t* d_idx, int n, const uint8_t* d_player, uint8_t* d_visual,
                              uint8_t* d_vector, uint8_t* d_piece) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = observe_packed_check(shape_of(b), d_idx != nullptr, n, d_visual, d_vector, d_piece))) return rc;
    if (n == 0) return TETRIS_OK;
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;
    dim3 grid(blocks_for(n)), block(256);
    if (b->H % 2 == 0&& ((uintptr_t)d_visual & 3u) == 0 && ((uintptr_t)d_vector & 3u) == 0) {
        // one wave per workgroup (<= 20 KB of LDS): several workgroups per CU overlap their load / build / store phases
        constexpr int OB = 64;
        const int nw = b->H * NCOL / 4;
        const size_t lds = (size_t)OB * nw * 4;
        dim3 ogrid(blocks_for(n, OB), (unsigned)b->P), oblock(OB);
        with_value<1, 2>(b->P, [&](auto P) {
            hipLaunchKernelGGL((k_observe_packed<P(), OB>), ogrid, oblock, lds, b->stream, geo_of_batch(b), n, d_idx, d_player, b->H,
                               d_visual, d_vector, d_piece);
        });
        return launched();
    }
    const size_t lds = (size_t)256 * b->H * NCOL;             // odd heights (boards are not word-aligned in `visual`): byte tile
    if (lds > 48 * 1024) {      // up to 79 KB of the CU's 160 KB for 31-row boards
        const void* fn = nullptr;
        with_value<1, 2>(b->P, [&](auto P) { fn = (const void*)k_observe_packed_bytes<P()>; });
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    with_value<1, 2>(b->P, [&](auto P) {
        hipLaunchKernelGGL(k_observe_packed_bytes<P()>, grid, block, lds, b->stream, geo_of_batch(b), n, d_idx, d_player, b->H, d_visual,
                           d_vector, d_piece);
    });
    return launched();
}

int tetris_observe_packed(tetris_batch* b, const int32_t* idx, int n, const uint8_t* player, uint8_t* visual, uint8_t* vector,
                          uint8_t* piece) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = observe_packed_outputs_check(visual, vector, piece))) return rc;
    HostCall io{b};
    if ((rc = io.idx(idx, n))) return rc;
    if (n == 0) return TETRIS_OK;
    const uint8_t* d_player;
    if ((rc = check_players(shape_of(b), player, n)) || (rc = io.in(player, (size_t)n, &d_player))) return rc;
    const size_t pn = (size_t)b->P * n;
    uint8_t *d_visual, *d_vector, *d_piece;
    if ((rc = io.out(visual, pn * b->H * NCOL, &d_visual)) || (rc = io.out(vector, pn * 12, &d_vector)) || (rc = io.out(piece, pn, &d_piece))) return rc;
    if ((rc = tetris_observe_packed_dev(b, io.d_idx, n, d_player, d_visual, d_vector, d_piece))) return rc;
    return io.finish();
}

static int snapshot_impl(tetris_batch* b, const int32_t* idx, int n, uint32_t* blob, int restore) {
    int rc = check_batch(b);
    if (rc) return rc;
    if (!blob) return fail(TETRIS_E_ARG, "blob is NULL");
    HostCall io{b};
    if ((rc = io.idx(idx, n))) return rc;
    if (n == 0) return TETRIS_OK;
    const size_t total = (size_t)n * (NGWORDS + b->P * b->nw);
    const uint32_t* d_in;
    uint32_t* d_out;
    if ((rc = restore ? io.in((const uint32_t*)blob, total, &d_in) : io.out(blob, total, &d_out))) return rc;
    rc = launch(b, k_snapshot, dim3(blocks_for(total)), dim3(256), 0, geo_of_batch(b), n, io.d_idx, restore ? (uint32_t*)d_in : d_out, restore);
    return rc ? rc : io.finish();
}

int tetris_snapshot(tetris_batch* b, const int32_t* idx, int n, uint32_t* blob) { return snapshot_impl(b, idx, n, blob, 0); }
int tetris_restore(tetris_batch* b, const int32_t* idx, int n, const uint32_t* blob) {
    return snapshot_impl(b, idx, n, (uint32_t*)blob, 1);
}

int tetris_set_dead(tetris_batch* b, const int32_t* idx, int n, const uint8_t* dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    if (!dead) return fail(TETRIS_E_ARG, "dead is NULL");
    HostCall io{b};
    const uint8_t* d_dead;
    if ((rc = io.idx(idx, n))) return rc;
    if (n == 0) return TETRIS_OK;
    if ((rc = io.in(dead, (size_t)n * b->P, &d_dead))) return rc;
    rc = launch(b, k_set_dead, dim3(blocks_for(n * b->P)), dim3(256), 0, geo_of_batch(b), n, io.d_idx, d_dead);
    return rc ? rc : io.finish();
}

int tetris_enumerate_drops_dev_ex(tetris_batch* b, const int32_t* d_idx, int n, const uint8_t* d_player, uint8_t* d_valid,
                                  int8_t* d_land_y, uint8_t* d_cleared, uint32_t* d_after, int flags) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = enumerate_check(shape_of(b), d_idx != nullptr, n, d_valid, d_land_y, d_cleared, d_after, flags))) return rc;
    if (n == 0) return TETRIS_OK;
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;
    dim3 grid(blocks_for(n, ENUM_BOARDS)), block(ENUM_BLOCK);
    const Geo geo = geo_of_batch(b);
    const bool planar = (flags & TETRIS_ENUM_PLANAR) != 0;
    with_shape<1, 4>(b->P, planar, [&](auto P, auto PLANAR) {
        hipLaunchKernelGGL((k_enumerate<P(), PLANAR()>), grid, block, 0, b->stream, geo, n, d_idx, d_player, b->H, d_valid, d_land_y, d_cleared, d_after);
    });
    return launched();
}

int tetris_enumerate_drops(tetris_batch* b, const int32_t* idx, int n, const uint8_t* player, uint8_t* valid, int8_t* land_y,
                           uint8_t* cleared, uint32_t* after) {
    int rc = check_batch(b);
    if (rc) return rc;
    if (!valid || !land_y || !cleared) return fail(TETRIS_E_ARG, "valid/land_y/cleared are NULL");
    HostCall io{b};
    if ((rc = io.idx(idx, n))) return rc;
    if (n == 0) return TETRIS_OK;
    const uint8_t* d_player;
    if ((rc = check_players(shape_of(b), player, n)) || (rc = io.in(player, (size_t)n, &d_player))) return rc;
    const size_t lanes = (size_t)n * 40;
    uint8_t *d_valid, *d_cleared;
    int8_t* d_land_y;
    uint32_t* d_after = nullptr;
    if ((rc = io.out(valid, lanes, &d_valid)) || (rc = io.out(land_y, lanes, &d_land_y)) || (rc = io.out(cleared, lanes, &d_cleared)) ||
        (after && (rc = io.out(after, lanes * NCOL, &d_after)))) return rc;
    if ((rc = tetris_enumerate_drops_dev_ex(b, io.d_idx, n, d_player, d_valid, d_land_y, d_cleared, d_after, 0))) return rc;
    return io.finish();
}

int tetris_timer_start(tetris_batch* b) {
    int rc = check_batch(b);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(b->ev0, b->stream));
    return TETRIS_OK;
}

int tetris_timer_stop(tetris_batch* b, float* elapsed_ms) {
    int rc = check_batch(b);
    if (rc) return rc;
    if (!elapsed_ms) return fail(TETRIS_E_ARG, "elapsed_ms is NULL");
    HIP_TRY(hipEventRecord(b->ev1, b->stream));
    HIP_TRY(hipEventSynchronize(b->ev1));
    HIP_TRY(hipEventElapsedTime(elapsed_ms, b->ev0, b->ev1));
    return TETRIS_OK;
}

int tetris_get_actions(tetris_batch* b, const int32_t* idx, int n, const uint8_t* player, uint8_t* keys, uint8_t* lens,
                       int32_t* count, int max_lists, int max_keys) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = get_actions_check(shape_of(b), idx != nullptr, n, player, keys, lens, count, max_lists, max_keys))) return rc;
    const int CHUNK_GAMES = 1024;                    // bounds the staging buffers
    const size_t L = PLAN_LANE_LISTS;                // lists one (x, rotation) start can produce
    std::vector<int32_t> ident;
    for (int g0 = 0; g0 < n; g0 += CHUNK_GAMES) {    // (each chunk drains before its lists are read: HostCall::finish)
        const int m = (n - g0 < CHUNK_GAMES) ? n - g0 : CHUNK_GAMES;
        const size_t lanes = (size_t)m * 40;
        const int32_t* h_idx = idx ? idx + g0 : nullptr;
        if (!h_idx && g0 > 0) { ident.resize(m); for (int i = 0; i < m; i++) ident[i] = g0 + i; h_idx = ident.data(); }
        HostCall io{b};
        const uint8_t *d_player, *hc, *hl, *hk;
        uint8_t *d_cnt, *d_len, *d_key;
        if ((rc = io.idx(h_idx, m)) || (rc = io.in(player ? player + g0 : nullptr, (size_t)m, &d_player)) ||
            (rc = io.out(nullptr, lanes, &d_cnt, &hc)) || (rc = io.out(nullptr, lanes * L, &d_len, &hl)) ||
            (rc = io.out(nullptr, lanes * L * max_keys, &d_key, &hk))) return rc;
        dim3 grid(blocks_for(lanes, 64)), block(64);
        with_value<1, 4>(b->P, [&](auto P) {
            hipLaunchKernelGGL(k_actions<P()>, grid, block, 0, b->stream, geo_of_batch(b), m, io.d_idx, d_player, b->H, d_cnt, d_len, d_key,
                               PLAN_LANE_LISTS, max_keys, b->flags);
        });
        if ((rc = launched()) || (rc = io.finish())) return rc;
        if ((rc = get_actions_gather(m, hc, hl, hk, max_lists, max_keys, keys + (size_t)g0 * max_lists * max_keys, lens + (size_t)g0 * max_lists, count + g0))) return rc;
    }
    return TETRIS_OK;
}

}  // extern "C"
