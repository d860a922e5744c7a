// Host side of the CPU harness, part 1 (as tetris_lib_batch.h): the RNG tables, the batch, base_args, run<MODE> (a launch of
// the game kernel as a loop over lanes), finish_call, check_batch, the staging of keys and outputs.  Needs tetris_host.h.
// "Device" pointers are host pointers here.

unsigned long long te::te_path_count[te::PC_NCOUNTERS];

using namespace te;

struct Tables {
    uint8_t map[8] = {0};
    int only_sz = 0;
    std::vector<uint32_t> mt;        // [624][65536]
    std::vector<float> w;            // [7][65536]
    std::vector<uint64_t> start;     // [65536] per-seed start entries
    double powtab[256];
    std::vector<uint8_t> table;      // [(chunk * 65536 + seed) * 624 + r]
    int n_chunks = 0;
    void extend() {
        int c = n_chunks;
        table.resize((size_t)65536 * CHUNK * (c + 1));
        uint8_t* out = table.data() + (size_t)65536 * CHUNK * c;
#pragma omp parallel for schedule(static)
        for (int seed = 0; seed < 65536; seed++) {
            uint64_t word = 0;
            gen_chunk_for_seed(mt.data() + seed, 65536, w.data() + seed, 65536, out + (size_t)seed * CHUNK, &word, c, map, only_sz != 0);
            if (c == 0) start[seed] = word;
        }
        n_chunks++;
    }
};
static std::map<std::string, Tables*> g_tables;

static Tables* tables_for(const uint8_t map[7]) {
    std::string key((const char*)map, 7);
    auto it = g_tables.find(key);
    if (it != g_tables.end()) return it->second;
    Tables* t = new Tables();
    memcpy(t->map, map, 7);
    t->only_sz = 1;
    for (int i = 0; i < 7; i++) if (map[i] != 2 && map[i] != 3) t->only_sz = 0;
    t->mt.resize((size_t)624 * 65536);
    t->w.resize((size_t)7 * 65536);
    t->start.resize(65536);
    for (int c = 0; c < 256; c++) t->powtab[c] = pow((double)c, 1.4 + (double)c * 0.01);
#pragma omp parallel for schedule(static)
    for (int seed = 0; seed < 65536; seed++) mt_seed(t->mt.data() + seed, 65536, (uint32_t)(int32_t)(int16_t)(uint16_t)seed);
    t->extend();
    t->extend();
    g_tables[key] = t;
    return t;
}

struct tetris_batch {
    int N, P, H;
    std::vector<uint32_t> state, gstate;
    uint32_t flags[NFLAGS] = {0};
    uint32_t margin = 64;
    uint32_t game_offset = 0;
    int split = 0, side = 0;
    int tint = 0, nw = NWORDS;
    int table_limit = MAX_CHUNKS;    // tetris_debug_table_limit
    std::vector<uint32_t> shadow;
    std::vector<uint32_t> words_before;      // the per-game counter words [4][N] as a rollout call found them (rollout_counters_begin)
    Tables* tab;
};

static HostShape shape_of(const tetris_batch* b) { return {b->N, b->P, b->H, b->nw, b->split, b->tint}; }

static KArgs base_args(tetris_batch* b, int n, const int32_t* idx) {
    KArgs a;
    memset(&a, 0, sizeof a);
    a.state = b->state.data(); a.gstate = b->gstate.empty() ? b->state.data() : b->gstate.data(); a.status = b->flags;
    a.table = b->tab->table.data(); a.start = b->tab->start.data(); a.combo_pow = b->tab->powtab;
    a.n_draws = table_draws(b->tab->n_chunks, b->table_limit); a.margin = b->margin;
    a.H = b->H; a.n_games = b->N; a.n_stride = b->N; a.n_players = b->P; a.nw = b->nw; a.n = n; a.idx = idx; a.game_offset = b->game_offset;
    return a;
}
static Geo geo_of_batch(tetris_batch* b) {
    Geo g = {b->state.data(), b->gstate.empty() ? b->state.data() : b->gstate.data(), (size_t)b->N, b->P, b->nw, (size_t)b->N};
    return g;
}

template <int MODE>
static void run(tetris_batch* b, const KArgs& a, LaneCounters* total = nullptr) {
    LaneCounters sum = {0, 0, 0, 0};
    for (int i = 0; i < a.n; i++) {
        LaneCounters c = {0, 0, 0, 0};
        if (!lane_active(a, i)) continue;
        with_shape<1, 4>(b->P, b->tint != 0, [&](auto P, auto TINT) { game_body<P(), MODE, TINT()>(a, i, SHAPES.s, c); });
        sum.steps += c.steps; sum.episodes += c.episodes; sum.lines += c.lines; sum.sent += c.sent;
    }
    if (total) *total = sum;
}

static int finish_call(tetris_batch* b) {
    if (b->flags[F_EXTEND]) {
        if (b->flags[F_EXTEND] >= (uint32_t)b->tab->n_chunks * CHUNK && b->tab->n_chunks < b->table_limit) b->tab->extend();
        b->flags[F_EXTEND] = 0;
    }
    return take_capacity_error(b->flags);
}

// what the shared entry points (tetris_lib_compose.h) ask first: the product's refusal of a NULL batch (there is no device to set here)
static int check_batch(tetris_batch* b, bool /*enqueues*/ = true) {
    if (!b) return fail(TETRIS_E_ARG, "null batch");
    return TETRIS_OK;
}

// host [n][P][K] -> [K][P][n], [n][P] -> [P][n]
struct KeyStage { std::vector<uint8_t> k, l; };
static int stage_keys(tetris_batch* b, int n, const uint8_t* keys, const uint8_t* lens, int max_keys, KArgs& a, KeyStage& s) {
    int rc = keys_check(keys, lens, max_keys);
    if (rc) return rc;
    s.k.assign((size_t)n * b->P * max_keys, 0); s.l.assign((size_t)n * b->P, 0);
    if ((rc = keys_pack(shape_of(b), n, keys, lens, max_keys, s.k.data(), s.l.data()))) return rc;
    a.keys = s.k.data(); a.lens = s.l.data(); a.max_keys = max_keys;
    return TETRIS_OK;
}

struct OutStage { std::vector<uint8_t> done, lines, dead; };
static void stage_out(tetris_batch* b, int n, KArgs& a, OutStage& o) {
    o.done.assign(n, 0); o.lines.assign((size_t)n * b->P, 0); o.dead.assign((size_t)n * b->P, 0);
    a.done = o.done.data(); a.lines = o.lines.data(); a.dead = o.dead.data();
}
static void fetch_out(tetris_batch* b, int n, const OutStage& o, uint8_t* done, uint8_t* lines, uint8_t* dead) {
    if (done) memcpy(done, o.done.data(), n);
    lines_dead_unpack(shape_of(b), n, o.lines.data(), o.dead.data(), lines, dead);
}
