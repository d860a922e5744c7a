// Host side of libtetris_hip.so, part 1: the batch object with its RNG tables and staging, the launch / enqueue / scratch helpers,
// the flag service, the run-ahead gate, finish_call and HostCall.  Included by tetris_hip.hip behind the kernel headers (tetris_dev_*.h); no host header before it.

struct tetris_batch;
static int chain_recover(tetris_batch* b);           // (tetris_lib_rollout.h; finish_call needs it)
#define HIP_TRY(expr)                                                                                            \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess)                                                                                    \
            return fail(TETRIS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                        \
    } while (0)

// What the launches made since the last look left behind, as the library's code.  On its own it follows a with_shape / with_value
// dispatcher, whose lambda launches and returns nothing.
static int launched() {
    HIP_TRY(hipGetLastError());
    return TETRIS_OK;
}
// One kernel on `stream` (launch, below: on the batch's own)
template <class... P, class... A>
static int launch_on(hipStream_t stream, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return launched();
}
// workgroups of `per` items for n items
static unsigned blocks_for(size_t n, size_t per = 256) { return (unsigned)((n + per - 1) / per); }

// RNG tables, shared by every batch on the same device with the same piece map
struct Tables {
    int device = -1;
    uint8_t map[8] = {0};
    int only_sz = 0;
    int refs = 0;
    uint32_t* d_mt = nullptr;        // [624][65536]
    float* d_w = nullptr;            // [7][65536]
    uint64_t* d_start = nullptr;     // [65536] per-seed start entries
    double* d_pow = nullptr;         // [256]
    uint8_t* d_table = nullptr;      // [(chunk * 65536 + seed) * 624 + r], capacity `cap_chunks`
    int n_chunks = 0, cap_chunks = 0;
    std::vector<uint8_t*> retired;   // outgrown tables: other streams may still be reading them
};
static const size_t CHUNK_BYTES = (size_t)65536 * CHUNK;
static std::mutex g_tab_mutex;
static std::vector<Tables*> g_tables;

static int tables_extend(Tables* t, hipStream_t stream) {
    if (t->n_chunks >= MAX_CHUNKS) return fail(TETRIS_E_STREAM, "RNG tables: MAX_CHUNKS reached");
    if (t->n_chunks == t->cap_chunks) {            // grow: new allocation, copy, retire the old one
        int cap = t->cap_chunks ? t->cap_chunks * 2 : 2;
        if (cap > MAX_CHUNKS) cap = MAX_CHUNKS;
        uint8_t* d = nullptr;
        HIP_TRY(hipMalloc((void**)&d, CHUNK_BYTES * cap));
        if (t->n_chunks) HIP_TRY(hipMemcpyAsync(d, t->d_table, CHUNK_BYTES * t->n_chunks, hipMemcpyDeviceToDevice, stream));
        if (t->d_table) t->retired.push_back(t->d_table);
        t->d_table = d;
        t->cap_chunks = cap;
    }
    MapArg m;
    memcpy(m.m, t->map, 8);
    const int rc = launch_on(stream, k_gen_chunk, dim3(256), dim3(256), 0, t->d_mt, t->d_w, t->d_table + CHUNK_BYTES * t->n_chunks,
                             t->d_start, t->n_chunks, m, t->only_sz);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    t->n_chunks++;
    return TETRIS_OK;
}

static void tables_free(Tables* t) {
    (void)hipFree(t->d_mt); (void)hipFree(t->d_w); (void)hipFree(t->d_start); (void)hipFree(t->d_pow);
    (void)hipFree(t->d_table);
    for (uint8_t* c : t->retired) (void)hipFree(c);
    delete t;
}

static int tables_build(Tables* t, hipStream_t stream);

static int tables_acquire(Tables** out, int device, const uint8_t map[7], hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_tab_mutex);
    for (Tables* t : g_tables)
        if (t->device == device && memcmp(t->map, map, 7) == 0) { t->refs++; *out = t; return TETRIS_OK; }
    Tables* t = new (std::nothrow) Tables();
    if (!t) return fail(TETRIS_E_HIP, "out of host memory");
    t->device = device;
    memcpy(t->map, map, 7);
    t->only_sz = 1;                                             // PythonHandle.h:116-121 set_pieces
    for (int i = 0; i < 7; i++) if (map[i] != 2 && map[i] != 3) t->only_sz = 0;
    int rc = tables_build(t, stream);
    if (rc) { std::string keep = g_err; tables_free(t); return fail(rc, keep); }
    t->refs = 1;
    g_tables.push_back(t);
    *out = t;
    return TETRIS_OK;
}

static int tables_build(Tables* t, hipStream_t stream) {
    HIP_TRY(hipMalloc((void**)&t->d_mt, (size_t)624 * 65536 * 4));
    HIP_TRY(hipMalloc((void**)&t->d_w, (size_t)7 * 65536 * 4));
    HIP_TRY(hipMalloc((void**)&t->d_start, 65536 * sizeof(uint64_t)));
    HIP_TRY(hipMalloc((void**)&t->d_pow, 256 * sizeof(double)));
    double powtab[256];
    for (int c = 0; c < 256; c++) powtab[c] = pow((double)c, 1.4 + (double)c * 0.01);   // Combo.cpp:41, host libm
    HIP_TRY(hipMemcpyAsync(t->d_pow, powtab, sizeof powtab, hipMemcpyHostToDevice, stream));
    int rc = launch_on(stream, k_gen_seed, dim3(256), dim3(256), 0, t->d_mt);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    for (int c = 0; c < 2 && !rc; c++) rc = tables_extend(t, stream);
    return rc;
}

static void tables_release(Tables* t) {
    std::lock_guard<std::mutex> lock(g_tab_mutex);
    if (--t->refs > 0) return;
    for (size_t i = 0; i < g_tables.size(); i++)
        if (g_tables[i] == t) { g_tables.erase(g_tables.begin() + i); break; }
    tables_free(t);
}

// grow-on-demand device + pinned-host staging pair
struct Stage {
    void* h = nullptr;
    void* d = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return TETRIS_OK;
        size_t want = bytes < 4096 ? 4096 : bytes + bytes / 2;
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        h = d = nullptr; cap = 0;
        HIP_TRY(hipHostMalloc(&h, want, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&d, want));
        cap = want;
        return TETRIS_OK;
    }
    void release() {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        h = d = nullptr; cap = 0;
    }
};
// grow-on-demand device scratch of a batch, `count` T exactly (an array asked for at one size only is allocated once)
template <class T>
struct Scratch {
    T* d = nullptr;
    size_t cap = 0;
    // `stream`: the batch's — drained before an array that work on it may still use is freed
    int ensure(size_t count, hipStream_t stream) {
        if (count <= cap) return TETRIS_OK;
        if (d) { HIP_TRY(hipStreamSynchronize(stream)); (void)hipFree(d); }
        d = nullptr; cap = 0;
        HIP_TRY(hipMalloc((void**)&d, count * sizeof(T)));
        cap = count;
        return TETRIS_OK;
    }
    void release() {
        (void)hipFree(d);
        d = nullptr; cap = 0;
    }
};
constexpr int STAGES = 6;               // most pairs one synchronous call stages through (HostCall): step_keys, step_rt, enumerate_drops

// 120: the host may be 241 launches (~1 ms of GPU work at 64k boards) ahead of what it has seen finish.  With 32 (round 2: 65
// launches, 0.26 ms) a host thread that loses its core for a fraction of a millisecond — other tenants' jobs share the box's CPUs —
// starves the GPU: 8192-launch runs measured 4.2-5.1 us per launch in bad minutes against 4.02-4.21 with 120, and 4.02 either way in
// good ones (profiles/r03/gate_depth_ab.txt).  The low-water margin of the RNG tables is sized from it (< one chunk of 624 draws).
constexpr int GATE_GROUP = 120;
#include "tetris_aql.h"

// One call of tetris_rollout_launch: what every launch path needs to build its launches (rollout_args), and, kept in
// tetris_batch::chain_call for the last chained call, what chain_recover needs to finish abandoned games un-chained.
struct RolloutCall {
    uint32_t epoch0 = 0;                 // chained: the epoch before the call's first launch (launch l publishes epoch0 + l + 1)
    uint64_t first_step = 0;
    int steps_per_launch = 0;
    uint32_t policy_seed = 0;
    int ms = 0;
    int launches = 0;
    bool chained = false;
};

struct tetris_batch {
    int device = 0, N = 0, P = 0, H = 0;
    int stride = 0;                      // games per row of the state arrays: N + padding (see create_impl)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t* d_state = nullptr;
    uint32_t* d_gstate = nullptr;
    uint32_t* flags = nullptr;           // te::Flag words: pinned, host-coherent, written by kernels with plain stores
    unsigned long long* d_counters = nullptr;
    unsigned long long* h_counters = nullptr;   // pinned [8]
    Tables* tab = nullptr;
    uint32_t margin = 2 * (2 * GATE_GROUP + 2) + 16;         // low-water mark of the RNG tables (draws); covers the launches in flight (gate below)
    uint32_t game_offset = 0;
    int split = 0, side = 0;
    int tint = 0, nw = NWORDS;           // colour planes tracked; words per player-board
    int use_duo = 1;                     // two-player rollout / step_rt through k_duo (TETRIS_NO_DUO=1 in the environment: k_game<2>)
    uint32_t* d_shadow = nullptr;        // split mode, side 1
    hipStream_t own_stream = nullptr;
    // chained launches (k_chain): two extra streams, one epoch word per wave, the number of the last chained launch
    hipStream_t chain_stream[CHAIN_STREAMS] = {};     // the device's (device_chain_streams): shared with its other batches, never destroyed
    hipEvent_t chain_ev[CHAIN_STREAMS + 1] = {};      // [k]: end of chain stream k's last launch (join); [CHAIN_STREAMS]: fork from the batch's stream
    hipEvent_t worker_gate_ev[CHAIN_STREAMS][2] = {}; // run-ahead gates of the per-stream enqueue threads (tetris_rollout_launch)
    uint32_t* d_chain = nullptr;
    Scratch<uint32_t> words_before;      // the per-game counter words [4][N] as a rollout call found them (rollout_counters_begin)
    uint32_t chain_epoch = 0;
    int use_chain = 1;                   // TETRIS_NO_CHAIN=1 in the environment: every rollout launch on the batch's one stream
    int use_graph = 0;                   // TETRIS_GRAPH=1: un-chained rollout launches replayed from HIP graphs (profiling aid)
    long long chain_capacity[2] = {-1, -1};   // wave slots of the device for the chained kernel, [fused] (computed on first use)
    int chain_depth = 0;                 // launches in flight = streams rotated over (3, or 2 where only two launches fit; 0: not chained)
    bool chain_pending = false;          // chained launches were enqueued since the last drain
    uint32_t chain_spin_limit = CHAIN_SPIN_LIMIT;     // polls before a waiting wave gives up (tetris_set_chain_spin_limit)
    RolloutCall chain_call;              // the chained call in progress (or the last one)
    bool chain_fell_back = false;        // a chained call was finished un-chained since the last tetris_take_errors (TETRIS_ERR_CHAIN_FELL_BACK)
    uint32_t* h_chain = nullptr;         // host copy of the epoch words (chain_recover)
    hipStream_t stall_stream = nullptr;  // tetris_debug_stall(.., -1, ..)
    // direct dispatch of the chained launches (tetris_aql.h): queues of the batch's own; off when anything about it failed
    int direct_min = 16;                 // calls of at least this many launches go through the device's own queues; 0: never (TETRIS_DIRECT=0 / TETRIS_DIRECT_MIN, tetris_set_direct_dispatch)
    bool last_direct = false;            // the last rollout call went through those queues
    bool direct_used = false;            // ... and so did some call of this batch (its destruction waits for the queues)
    int use_affine = 1;                  // XCD-affine launches (k_chain_affine) where the device's queues allow them; TETRIS_AFFINE=0 / tetris_set_xcd_affine
    bool last_affine = false;            // the last rollout call ran them
    uint32_t xcd_skew = 0;               // test aid (tetris_debug_xcd_skew): added to the queues' measured start XCDs
    int table_limit = MAX_CHUNKS;        // test aid (tetris_debug_table_limit): this batch's kernels see at most that many chunks of the tables
    int affine_failures = 0;             // calls in which a workgroup found itself misplaced (three: the affine form is switched off)
    bool home_async = false;             // asynchronous (_dev) work was enqueued on the batch's stream since the last drain
    // something was enqueued on one of the batch's streams since the last drain.  Whatever enqueues sets it (check_batch, HostCall,
    // service_flags): on the batch's own stream finish_call skips the drain without it, also in a call's second drain (get_actions)
    bool busy = true;
    // Run-ahead gate of the asynchronous entry points: every GATE_GROUP launches an event is recorded; before a new group is
    // enqueued the host waits for the event of the group before the previous one.  At most 2 * GATE_GROUP + 1 launches are
    // therefore in flight whose flag words the host has not seen; `margin` is sized for that many steps.
    hipEvent_t gate_ev[2] = {nullptr, nullptr};
    int gate_count = 0;                  // launches since the last recorded event
    int gate_slot = 0;                   // event to record next
    int gate_pending[2] = {0, 0};        // event has been recorded and not waited for
    Stage stage[STAGES];                 // the synchronous calls' staging pairs (HostCall hands them out in order)
    Stage recover_idx;                   // chain_recover's game lists: it runs inside finish_call, while a call's outputs still wait in `stage`
    // tetris_action_lists_dev: device scratch for the slabs of one chunk of games (grown on demand), the identity index the
    // chunks' k_actions launches read their game numbers from, and the status words k_actions writes its own overflow flag to
    // (the compaction finds every overflow itself, per game, and reports it as F_LISTS instead)
    Scratch<uint8_t> plan_slabs;
    Scratch<int32_t> iota;
    Scratch<uint32_t> plan_status;
    // the heuristic policy's spread mapping: the 40 scores of every game, [40][N], from k_policy_eval to the kernel that chooses
    Scratch<int32_t> policy_scores;
    // tetris_traj_select_dev: the counts per workgroup and their scan (grown on demand)
    Scratch<int32_t> select_blocks;
    // tetris_replay_add_dev: the entries per game and their scan; tetris_replay_sample_dev: the sort's pairs, ranks and
    // histograms (both grown on demand)
    Scratch<uint32_t> replay_offsets, replay_sort;
    // the loss heads: the words D and Dnz and the workgroups' partial rows of the statistics (grown on demand)
    Scratch<uint32_t> loss_scratch;
    // tetris_kstep_target_dev in Q mode without d_values: the values of the M n rows (grown on demand)
    Scratch<float> kstep_values;
    // the keyboard convolution: w repacked for the matrix unit (forward, grad_x) or grad_w's partial sums (grown on demand)
    Scratch<uint32_t> kbd_scratch;
    // the residual layer: likewise
    Scratch<uint32_t> res_scratch;
    void release_scratch() {
        kbd_scratch.release(); res_scratch.release();
        plan_slabs.release(); iota.release(); plan_status.release(); policy_scores.release(); words_before.release();
        select_blocks.release(); replay_offsets.release(); replay_sort.release(); loss_scratch.release(); kstep_values.release();
    }
};

// One kernel on the batch's stream
template <class... P, class... A>
static int launch(tetris_batch* b, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, const A&... args) {
    return launch_on(b->stream, kernel, grid, block, lds, args...);
}

static HostShape shape_of(const tetris_batch* b) { return {b->N, b->P, b->H, b->nw, b->split, b->tint}; }

static Geo geo_of_batch(tetris_batch* b) {
    Geo g = {b->d_state, b->d_gstate, (size_t)b->N, b->P, b->nw, (size_t)b->stride};
    return g;
}

static KArgs base_args(tetris_batch* b, int n, const int32_t* d_idx) {
    KArgs a;
    memset(&a, 0, sizeof a);
    a.state = b->d_state; a.gstate = b->d_gstate; a.status = b->flags;
    {   // tables are shared between batches: take pointer and size together (another batch may be growing them)
        std::lock_guard<std::mutex> lock(g_tab_mutex);
        a.table = b->tab->d_table;
        a.n_draws = table_draws(b->tab->n_chunks, b->table_limit);
    }
    a.start = b->tab->d_start; a.combo_pow = b->tab->d_pow; a.margin = b->margin;
    a.H = b->H; a.n_games = b->N; a.n_stride = b->stride; a.n_players = b->P; a.nw = b->nw; a.n = n; a.idx = d_idx; a.game_offset = b->game_offset;
    return a;
}

template <int MODE>
static int launch_game(tetris_batch* b, const KArgs& a) {
    dim3 grid(blocks_for(a.n)), block(256);
    if constexpr (MODE == M_ROLLOUT || MODE == M_STEP_RT || MODE == M_STEP_RT_AUTO) {
        // two-player full-batch single steps: players in adjacent half-waves (k_duo), 32 games per wave.  Measured on
        // MI355X at 64k games: 9.37 us vs 9.73 us for k_game<2> at one step per launch, but 4.4 vs 3.9 us per step when
        // 16 steps are fused, so fused rollouts stay on k_game<2>.
        if (b->P == 2 && !b->tint && !a.idx && b->use_duo && (MODE != M_ROLLOUT || a.steps == 1))
            return launch(b, k_duo<MODE>, dim3(blocks_for(a.n, 128)), block, 0, a);
    }
    // (three and four players per game: the same kernel with all players of a game in one lane; it spills, and nothing is tuned for it)
    const bool here = with_shape<1, 2>(b->P, b->tint != 0, [&](auto P, auto TINT) {
        hipLaunchKernelGGL((k_game<P(), MODE, TINT()>), grid, block, 0, b->stream, a);
    });
    if (!here && tetris_launch_game_multi(b->P, b->tint, MODE, grid, block, b->stream, a)) return fail(TETRIS_E_ARG, "no kernel for this player count / mode");
    return launched();
}

// Looks at the flag words WITHOUT enqueuing or waiting for anything: answers a pending "extend the RNG tables" request
// (the generation kernel goes on the batch's stream, i.e. before every launch made after this call).
static int service_flags(tetris_batch* b) {
    volatile uint32_t* f = b->flags;
    const uint32_t want = f[F_EXTEND];
    if (want) {
        std::lock_guard<std::mutex> lock(g_tab_mutex);
        // not yet answered (requests carry the size their kernel saw); at MAX_CHUNKS (the batch's table_limit) the tables stay as
        // they are and a game that outruns them is ended with ERR_STREAM
        if (want >= (uint32_t)b->tab->n_chunks * CHUNK && b->tab->n_chunks < b->table_limit) {
            int rc = tables_extend(b->tab, b->stream);
            if (rc) return rc;
            b->busy = true;
        }
        f[F_EXTEND] = 0;
    }
    return TETRIS_OK;
}

// Waits for an event by polling it `spins` times before the blocking wait: a thread blocked in hipEventSynchronize is woken
// through an interrupt — 10-20 us late at best, milliseconds when the scheduler has given its core away meanwhile.
static hipError_t poll_event(hipEvent_t e, int spins) {
    hipError_t qe = hipErrorNotReady;
    for (int spin = 0; spin < spins && qe == hipErrorNotReady; spin++) qe = hipEventQuery(e);
    return qe == hipErrorNotReady ? hipEventSynchronize(e) : qe;
}

// One more asynchronous launch is about to be enqueued: bound the run-ahead (see tetris_batch) and service the flags.
static int gate_launch(tetris_batch* b, int group) {
    if (b->gate_count >= group) {
        const int k = b->gate_slot;
        if (b->gate_pending[k]) {                               // the group before the previous one must have finished
            // polled (the GPU has only the launches of two groups, ~0.26 ms, to live on)
            HIP_TRY(poll_event(b->gate_ev[k], 2000000));
            b->gate_pending[k] = 0;
        }
        HIP_TRY(hipEventRecord(b->gate_ev[k], b->stream));
        b->gate_pending[k] = 1;
        b->gate_slot = k ^ 1;
        b->gate_count = 0;
    }
    b->gate_count++;
    {
        bool on_chain = false;
        for (hipStream_t st : b->chain_stream) on_chain |= b->stream == st;
        if (!on_chain) b->home_async = true;
    }
    return service_flags(b);
}

// What an asynchronous (_dev) entry point is about to put on the batch's stream.  Every such entry point passes through enqueue()
// once: behind check_batch, the argument rules (a refused call has neither gated nor marked) and the growth of its scratch, in
// front of base_args (the gate may extend the RNG tables) and of its launches.  A new entry point picks the first class that fits.
enum class Enqueue {
    STEPS,      // moves games on, or is enqueued once per step of a loop the host never waits in: run-ahead gate, flag service
                // (table extensions) and the mark below — gate_launch(b, GATE_GROUP)
    STATE,      // reads or writes the games' state, the batch's scratch or the epoch words: marked (home_async), so that a later
                // chained rollout — on other streams, or in the library's own queues, which HIP does not order — goes behind it
    CALLER,     // touches nothing but the caller's buffers (a window included): nothing.  A chained rollout neither reads nor
                // writes those, and whatever the caller does with them next is ordered by the stream it shares with this call
};
static int enqueue(tetris_batch* b, Enqueue what) {
    if (what == Enqueue::STEPS) return gate_launch(b, GATE_GROUP);
    if (what == Enqueue::STATE) b->home_async = true;
    return TETRIS_OK;
}

// Waits for a stream by polling it for a while before falling back to the blocking wait: a blocked host thread is woken
// through an interrupt, 10-20 us after the GPU is done — as long as a whole 20-launch rollout of 64k boards.
static hipError_t drain_stream(hipStream_t st) {
    for (int spin = 0; spin < 20000; spin++) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
    }
    return hipStreamSynchronize(st);
}

// drain the batch's stream(s), then the flag words: sticky errors surface, the RNG tables are extended when a board came close to their end
// `drained`: the caller has already seen an event complete that is ordered behind everything the batch's streams held (a stream
// query makes the runtime push a marker through the queue and wait for it: ~6 us per stream even when the stream is idle)
static int finish_call(tetris_batch* b, bool drained = false) {
    if (!b->busy && !b->chain_pending && b->stream == b->own_stream) {      // drained already and nothing enqueued since: only the flag words
        int rc0 = service_flags(b);
        if (rc0) return rc0;
        if (!b->busy) return TETRIS_OK;           // (an extension would have enqueued work)
    }
    if (b->chain_pending && !drained)
        for (int k = 0; k < CHAIN_STREAMS; k++) HIP_TRY(drain_stream(b->chain_stream[k]));
    b->chain_pending = false;
    if (!drained) HIP_TRY(drain_stream(b->stream));
    b->home_async = false;
    b->busy = false;
    b->gate_count = 0; b->gate_pending[0] = b->gate_pending[1] = 0;
    volatile uint32_t* f = b->flags;
    // (F_EXHAUSTED / F_FIFO: capacity errors are confined to the games they happened in — tetris_take_errors)
    int rc = TETRIS_OK;
    // a workgroup of an affine launch was not where its queue's calibration put it (it left its games alone): that form stays off,
    // and the games it — and whoever waited for it — left behind are finished like abandoned ones
    const bool misplaced = f[F_PLACE] != 0;
    if (misplaced) {
        // The games such workgroups — and whoever waited for them — left behind are finished like abandoned ones.  A queue's start XCD
        // moves when the driver re-maps hardware queues (many queues in the process); the next call expects what this one saw.
        // Not the caller's business unless it keeps happening: chaining stays as it was, the affine form goes after three such calls.
        const int keep_chain = b->use_chain;
        const bool keep_fell_back = b->chain_fell_back;
        f[F_PLACE] = 0;
        if ((rc = chain_recover(b))) return rc;
        b->use_chain = keep_chain; b->chain_fell_back = keep_fell_back;
        if (++b->affine_failures >= 3) b->use_affine = 0;
    }
    if (f[F_CHAIN] && (rc = chain_recover(b))) return rc;       // waves of a chained launch gave up: their games are finished un-chained
    if ((rc = service_flags(b))) return rc;                     // before the argument error below: an extend request is never dropped
    return take_capacity_error(f);
}

// every entry point starts here; `enqueues`: the call may put work on one of the batch's streams (all but the pure waits)
static int check_batch(tetris_batch* b, bool enqueues = true) {
    if (!b) return fail(TETRIS_E_ARG, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    if (enqueues) b->busy = true;
    return TETRIS_OK;
}

// The host traffic of one synchronous call (the entry points that take and return host arrays), on the batch's stream.  An input
// goes from the caller's array to a pinned half, then to the device; an output gets a device half for the kernel, and finish()
// copies it back to its pinned half, drains (finish_call) and only then copies it on to the caller's array.  The k-th input or
// output of a call takes b->stage[k] (a NULL input keeps its place), so one call's buffers never alias, and every copy queued
// here sets b->busy.
struct HostCall {
    tetris_batch* const b;
    const int32_t* d_idx = nullptr;      // idx(): the call's game indices on the device (NULL: the first n games)
    int used = 0, n_out = 0;
    struct Out { const Stage* s; size_t bytes; void* dst; } outs[STAGES];

    // the next pair, `bytes` long at least (the caller fills its pinned half, or the kernel its device half)
    int take(size_t bytes, Stage** s) {
        if (used >= STAGES) return fail(TETRIS_E_ARG, "internal: a call takes more than STAGES staging buffers");
        *s = &b->stage[used++];
        return (*s)->ensure(bytes + 16);
    }
    // pinned half -> device half
    int send(const Stage* s, size_t bytes) {
        b->busy = true;
        HIP_TRY(hipMemcpyAsync(s->d, s->h, bytes, hipMemcpyHostToDevice, b->stream));
        return TETRIS_OK;
    }
    // `count` T of the caller's -> the device (*d; src NULL: *d = NULL)
    template <class T> int in(const T* src, size_t count, const T** d) {
        *d = nullptr;
        if (!src) { used++; return TETRIS_OK; }
        Stage* s;
        int rc = take(count * sizeof(T), &s);
        if (rc) return rc;
        memcpy(s->h, src, count * sizeof(T));
        *d = (const T*)s->d;
        return send(s, count * sizeof(T));
    }
    // game indices: validated, then staged (-> d_idx)
    int idx(const int32_t* idx, int n) {
        int rc = check_idx(shape_of(b), idx, n);
        return rc ? rc : in(idx, (size_t)n, &d_idx);
    }
    // `count` T on the device for the kernel (*d); finish() copies them to `dst`, or leaves them in the pinned half for the caller
    // to read (*h) when dst is NULL
    template <class T> int out(void* dst, size_t count, T** d, const T** h = nullptr) {
        Stage* s;
        int rc = take(count * sizeof(T), &s);
        if (rc) return rc;
        outs[n_out++] = {s, count * sizeof(T), dst};
        *d = (T*)s->d;
        if (h) *h = (const T*)s->h;
        return TETRIS_OK;
    }
    int finish() {
        for (int k = 0; k < n_out; k++) {
            b->busy = true;
            HIP_TRY(hipMemcpyAsync(outs[k].s->h, outs[k].s->d, outs[k].bytes, hipMemcpyDeviceToHost, b->stream));
        }
        int rc = finish_call(b);
        if (rc) return rc;
        for (int k = 0; k < n_out; k++)
            if (outs[k].dst) memcpy(outs[k].dst, outs[k].s->h, outs[k].bytes);
        return TETRIS_OK;
    }
};

// The rest of a synchronous step: done [n] and lines / dead [P][n] on the device, the launch, io.finish(), then lines / dead to the
// caller as [n][P]
template <int MODE>
static int finish_step(HostCall& io, KArgs& a, int n, uint8_t* done, uint8_t* lines, uint8_t* dead) {
    const int P = io.b->P;
    const uint8_t *hl, *hd;
    int rc = io.out(done, (size_t)n, &a.done);
    if (rc || (rc = io.out(nullptr, (size_t)n * P, &a.lines, &hl)) || (rc = io.out(nullptr, (size_t)n * P, &a.dead, &hd))) return rc;
    if ((rc = launch_game<MODE>(io.b, a)) || (rc = io.finish())) return rc;
    lines_dead_unpack(shape_of(io.b), n, hl, hd, lines, dead);
    return TETRIS_OK;
}
