// Kernels of libtetris_hip.so, part 2: what tetris_lib_rollout.h launches.  The chained rollout kernels (k_chain and its three
// siblings; k_duo for two players), the XCD probe, the blocker and the clock probe of the measurement aids, and the counter
// totals.  Needs tetris_dev_observe.h (k_duo with OBS).

// Chained launches of the built-in rollout (one env-step per launch).  A game's step E depends on nothing but the same game's
// step E - 1, yet launches on one stream are separated by a full barrier: launch E waits for the SLOWEST wave of launch E - 1
// plus the kernel boundary (~1.4 us of a ~5.7 us launch period, profiles/).  Here consecutive launches rotate over CHAIN_STREAMS (3)
// streams, so launch E is dispatched while E - 1 and E - 2 still run, and the dependence is enforced per WAVE (one workgroup = one
// wave = 64 games): wave w of launch E polls an epoch word until wave w of launch E - 1 has published E - 1.  Every state
// load / store is agent-scope (`sc1`: written through, read past the per-XCD L2), the storing wave drains its stores
// (`s_waitcnt vmcnt(0)`) before it publishes — the measured-valid hand-off of MI355X_MICROARCH.md.  Spins are bounded: a wave
// that gives up marks its epoch word (CHAIN_ABANDONED), raises F_CHAIN and leaves its games untouched; so does the same wave of
// every later launch, and the host finishes those games un-chained once the streams have drained (chain_recover).
constexpr int CHAIN_LANES = 64;      // games per wave of k_chain
constexpr int CHAIN_STREAMS = 3;     // streams the chained launches rotate over = launches in flight.  3 x 1024 waves of 64k single-player
                                     // boards fit in the 15 x 256 wave slots chain_fits counts; GPU-paced 4.02 us per launch against 4.14 with 2
                                     // (with the epoch words still packed 32 to a line it had been 4.9-5.06 against 4.71-4.80)
// XCD-AFFINE form (k_chain_affine; direct dispatch only, tetris_aql.h).  The write-through hand-off above crosses the fabric twice per
// step because block b of consecutive launches never meets its own XCD again (a queue deals its blocks round-robin over the eight XCDs
// from a start of its own: profiles/r03/handoff_experiments.txt).  Here the GAMES follow the XCD instead: the workgroup that finds
// itself on XCD x takes the game block (b & ~7) | x, so a block is stepped on the same XCD in every launch and its state and epoch
// word can stay in that XCD's L2 — plain stores, `sc1` loads (past the CU's L1, served by the L2).  One L2 is coherent for all CUs
// of its XCD; nothing else is relied on.  That the eight workgroups of a group of eight really sit on eight different XCDs is
// CHECKED, by every workgroup for itself: the queue's start XCD is measured when the queue is made (a.xcd_base), and a
// workgroup that is not on XCD (xcd_base + b) mod 8 touches nothing, raises F_PLACE and leaves — its games then look abandoned to the
// next launch, whose waves give up, and the host finishes the call un-chained (chain_recover) and switches the affine form off.
// What makes this FASTER only with direct dispatch: the packets between a queue's first and last carry no cache maintenance
// (a kernel boundary's L2 write-back + invalidate, three times per 12 us, cost more than the fabric: +0.1 us per launch through
// streams); the queue's last packet releases, so memory is current when the call returns.
// FUSED says which launches a kernel serves.  false: one env-step per launch, the case that is timed (k_chain, k_chain_affine) —
// rollout_step once, straight-line.  With game_run's loop over a.steps around the step the compiler hoists the loop's constants
// and the next step's policy draw into a preheader BEHIND the state loads, where every instruction is on the wave's dependent
// chain, and keeps a second copy of Philox in the body; a one-step launch uses none of it.  true: any other step count (k_chain_fused,
// k_chain_fused_affine: S > 1, and S = 0 of the counter calibration), game_run with its loop.
template <int P, bool AFFINE, bool FUSED>
__device__ __forceinline__ void chain_body(const KArgs& a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_shapes[SHAPE_WORDS];
    const int lane = threadIdx.x;
    if (a.steps < 0) { chain_census(a, lane == 0); return; }
    constexpr int CMEM = AFFINE ? MEM_AFFINE : MEM_AGENT;
    int wave = blockIdx.x;
    uint32_t xcc = 0;
    // AFFINE: block 0 reports where this queue starts dealing (F_XCC0 + queue: the host's expectation for the next call) on its way
    // out, so that the store's trip to host memory never holds up the step (a wave waits for ALL its outstanding vector memory
    // accesses at the first poll)
    const auto report_xcc = [&]() { if (AFFINE && blockIdx.x == 0 && lane == 0) st_flag(a.status + F_XCC0 + (a.xcd_slot & 3u), 0x100u | xcc); };
    if (AFFINE) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 0xFu;
        if (xcc != ((a.xcd_base + blockIdx.x) & 7u)) {          // not where the host expects this block to run: hands off
            if (lane == 0) st_flag(a.status + F_PLACE, 1u);
            report_xcc();
            return;
        }
        wave = (int)((blockIdx.x & ~7u) | xcc);
        if (wave * CHAIN_LANES >= a.n) { report_xcc(); return; }   // (padding of the last group of eight: no games, no epoch word)
    }
    const int i = wave * CHAIN_LANES + lane;
    const bool active = lane < CHAIN_LANES && i < a.n;
    LaneCounters cnt = {0, 0, 0, 0};
    const uint32_t shape_word = d_shape_table.s[lane];     // (issued at the top; it has long arrived when the LDS table is written)
    Game<P> g;
    // Work that does not depend on the predecessor happens before the poll: the policy draw of this step (kernel arguments only:
    // its 40 dependent multiplies run while the wave waits), and the row stride of the state arrays (pinned into an SGPR here;
    // the compiler would load it after the poll, with a wait for the scalar load in front of the first state load).  The LDS
    // shape table is written after the state loads are issued: written before the poll it would need a wait for its global load
    // in front of the first poll.
    // (Issuing the first poll of the epoch word BEFORE the draw — most waves find their predecessor done at that poll — measured
    // +0.06 us per launch, GPU-paced: profiles/r02/chain_ab_gpu_paced.txt.)
    if (active) policy_draw(a, (uint32_t)i, a.first_step, g.draw0, g.draw1);
    const uint32_t d0 = g.draw0, d1 = g.draw1;
    int stride = a.n_stride;
    asm volatile("" : "+s"(stride));
    // The single-step kernels also multiply out, here, the byte offsets of the state rows the step touches (tetris_engine.h: RowTable)
    // and pin them into SGPRs: the loads behind the poll and the stores behind the step then find their offsets ready.  Left to itself
    // the compiler multiplies them out where they are used, twice, between the loads and among the stores: on the chain.
    RowTable<NWORDS> rows = {};
    RowTable<NGWORDS> grows = {};
    if (!FUSED) {
        TE_UNROLL
        for (int w = 0; w < NWORDS; w++)
            if (P > 1 || (w < NWORDS_HOT && w != W_INCOMING && w != W_HOLE_DRAWS)) {      // (one player: no queue, these are never touched)
                uint32_t bytes = (uint32_t)(w * P) * (uint32_t)stride * 4u;
                asm volatile("" : "+s"(bytes));
                rows.bytes[w] = bytes;
            }
        TE_UNROLL
        for (int w = 0; w < NGWORDS; w++) {            // (G_LINES, G_SENT: the rare counter atomics)
            uint32_t bytes = (uint32_t)w * (uint32_t)stride * 4u;
            asm volatile("" : "+s"(bytes));
            grows.bytes[w] = bytes;
        }
    }
    const uint32_t seen = chain_poll(a, (uint32_t)wave);
    if (seen == a.epoch - 1u) {                 // (a uniform branch: the state loads follow the poll's exit)
        Geo geo = geo_of(a);
        geo.stride = (size_t)stride;
        if (active) {
            if (FUSED) load_game<P>(geo, (size_t)i, g, false, P > 1, true, CMEM);
            else load_game_rows<P>(geo, (size_t)i, rows, grows, g, false, P > 1, true, CMEM);
            g.draw0 = d0; g.draw1 = d1;
        }
        s_shapes[lane] = shape_word;
        __builtin_amdgcn_wave_barrier();
        if (FUSED) {
            if (active) game_run<P, M_ROLLOUT, false, CMEM>(a, i, s_shapes, g, cnt);
        } else if (active) {
            const Ctx cx = make_ctx(a, s_shapes, false, P > 1);
            rollout_step<P>(cx, a, (size_t)i, a.first_step, g, cnt);
            store_game_rows<P>(geo, (size_t)i, rows, grows, g, false, P > 1, true, CMEM);
            report_status(a, g.status);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every store (and counter atomic) of this wave has been acknowledged
        if (lane == 0) {
            // AFFINE: a plain store, the line stays in this XCD's L2 where the next launch's wave polls it; otherwise written through
            // (`sc1`).  Neither waits for its acknowledgement: the wave ends here.
            if (AFFINE) st_xcd(a.chain + (size_t)wave * CHAIN_STRIDE, a.epoch);
            else st_agent(a.chain + (size_t)wave * CHAIN_STRIDE, a.epoch);
        }
    } else if (!(seen & CHAIN_ABANDONED)) {     // (with the bit set an earlier launch's wave gave up and recorded it)
        chain_give_up(a, (uint32_t)wave, lane == 0);          // the games stay as launch E - 1 (or an earlier one) left them
    }
    report_xcc();
}
template <int P>
__global__ __launch_bounds__(64) void k_chain(KArgs a) { chain_body<P, false, false>(a); }
template <int P>
__global__ __launch_bounds__(64) void k_chain_affine(KArgs a) { chain_body<P, true, false>(a); }
template <int P>
__global__ __launch_bounds__(64) void k_chain_fused(KArgs a) { chain_body<P, false, true>(a); }
template <int P>
__global__ __launch_bounds__(64) void k_chain_fused_affine(KArgs a) { chain_body<P, true, true>(a); }
template __global__ void k_chain_affine<1>(KArgs);
template __global__ void k_chain_fused_affine<1>(KArgs);
// the XCD every workgroup of a launch lands on (calibration of the affine form: aql::make_queues)
extern "C" __global__ void tetris_k_xcc_probe(uint32_t* out) {
    if (threadIdx.x == 0) {
        uint32_t xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        out[blockIdx.x] = xcc & 0xFu;
    }
}

// "Duo" mapping for two-player games (BASELINE config 3): the two players of a game sit in lanes l and l ^ 32 of ONE wave,
// so 64k games are 2 waves per SIMD instead of 1 and the second player's clear/spawn, timers and state traffic overlap with
// the first's.  The in-step order dependence between the players is the split-mode stage protocol (tetris_engine.h) with
// the exchange words moved by __shfl_xor(.., 32): A = key interpreter + loop 1 (player 1 speculatively, with a register
// backup for the rollback when player 0 died), B0 / B1 = delayCheck of player 0, then player 1, C = winner logic.
// CHAIN (rollout only, 64-thread workgroups): chained launches as in k_chain — a wave's 32 games wait for the epoch word the same
// wave of the previous launch published, and all state traffic is agent-scope.
// OBS (tetris_step_rt_observe_dev): after the step every lane turns its own board into the packed observation — slot 0 if its
// player is the one the game's next decision is for, slot 1 otherwise; rows 0..31 / 32..63 of the wave's LDS tile.
// AFFINE (with CHAIN; k_duo_affine, direct dispatch only): the XCD-affine hand-over of k_chain_affine — a wave's 32 games follow the XCD.
template <int MODE, bool CHAIN, bool OBS, bool AFFINE>
__device__ __forceinline__ void duo_body(const KArgs& a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_shapes_all[4][SHAPE_WORDS];      // per-wave copy, no block barrier (see k_game)
    extern __shared__ __attribute__((aligned(16))) uint32_t s_duo_tile[];               // OBS: 4 waves x 64 rows x nw words
    uint32_t* s_shapes = s_shapes_all[threadIdx.x >> 6];
    const uint32_t shape_word = d_shape_table.s[threadIdx.x & 63];
    const int lane = threadIdx.x & 63, side = lane >> 5;
    int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    constexpr bool ROLL = MODE == M_ROLLOUT, AUTO = MODE == M_STEP_RT_AUTO;
    constexpr int MEM = CHAIN ? (AFFINE ? MEM_AFFINE : MEM_AGENT) : MEM_STREAM;
    if (CHAIN && a.steps < 0) { chain_census(a, lane == 0); return; }
    uint32_t xcc = 0;
    const auto report_xcc = [&]() { if (AFFINE && blockIdx.x == 0 && lane == 0) st_flag(a.status + F_XCC0 + (a.xcd_slot & 3u), 0x100u | xcc); };
    if (AFFINE) {                        // (64-thread workgroups: one wave each; see chain_body, also for report_xcc)
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 0xFu;
        if (xcc != ((a.xcd_base + blockIdx.x) & 7u)) {
            if (lane == 0) st_flag(a.status + F_PLACE, 1u);
            report_xcc();
            return;
        }
        wave = (int)((blockIdx.x & ~7u) | xcc);
        if (wave * 32 >= a.n) { report_xcc(); return; }
    }
    const int gi = wave * 32 + (lane & 31);
    const bool active = gi < a.n;
    Geo geo = geo_of(a);
    geo.P = 2;                           // compile-time stride factor for the hot loads
    const Ref gr = game_ref(geo, (size_t)gi);
    // one UNIFORM row base for both half-waves (it becomes a buffer resource): the player's offset goes into the lane offset
    const Ref br = {geo.state, (uint32_t)((size_t)side * geo.stride + (size_t)gi) * 4u, 2 * geo.stride};
    Game<1> g;
    Player& q = g.pl[0];
    uint32_t pd0 = 0, pd1 = 0;
    if (CHAIN) {
        if (active) policy_draw(a, (uint32_t)gi, a.first_step, pd0, pd1);        // while the wave waits for its predecessor
        if (!chain_wait(a, (uint32_t)wave, lane == 0)) { report_xcc(); return; }
    }
    if (active) {
        load_game_words<1>(gr, g, ROLL, MEM);
        load_player(br.s, br.o, br.ws, q, false, true, MEM);
        if (CHAIN) { g.draw0 = pd0; g.draw1 = pd1; }
        else if (ROLL) policy_draw(a, (uint32_t)gi, a.first_step, g.draw0, g.draw1);   // under the loads (see game_load)
        else { g.draw0 = a.rot[gi]; g.draw1 = (uint32_t)a.trans[gi] | ((a.player ? (uint32_t)a.player[gi] : 0u) << 8); }
    }
    s_shapes[lane] = shape_word;
    __builtin_amdgcn_wave_barrier();
    Ctx cx = make_ctx(a, s_shapes, false);
    uint32_t my_lines = 0, my_sent = 0;
    int done = 0, out_reward = 0, out_dead = 0;
    // ONE env-step per launch (launch_game sends fused rollouts to k_game<2>): as a loop over a.steps this kernel needed 199
    // registers per lane instead of ~130 — everything stayed live around the loop's back edge.
    {
        int r = 0, t = 0, acting = 0;
        ResetPrefetch rpf;
        rpf.ok = 0; rpf.seed16 = 0; rpf.word = 0;
        uint32_t sent_start = 0;
        uint32_t wa = 0;
        uint32_t undo_pose = 0, undo_group = 0, undo_draws = 0, undo_cleared = 0;
        bool undo_ran = false;
        Player pre;                                                    // un-chained kernels only: player 1's board before its speculative pass
        if (active) {
            if (ROLL) {
                r = (int)(g.draw0 & 3u); t = (int)(g.draw1 % 10u); acting = (int)(a.first_step % 2ull);
            } else {
                r = (int)(g.draw0 & 3u); t = (int)(g.draw1 & 0xFFu); acting = (int)(g.draw1 >> 8);
            }
            if (ROLL || AUTO) prefetch_reset(cx, episode_seed(a.game_offset + (uint32_t)gi, g.episode + 1), rpf);
            prefetch_next(cx, q, g.seed16, g.status);
            sent_start = q.lines_sent;
            // stage A
            if (!g.round_over && !q.dead && acting == side) play_rt(cx, q, r, t);
            // Player 1's loop-1 pass is speculative (the reference skips it when player 0 died in loop 1, PythonHandle.cpp:153-156,
            // which this lane learns from the shuffle below).  What the pass changes when it clears no row and the new piece
            // fits — nearly always — is the piece (kind, rotation, position, next), the draw counter, now and then the piece
            // group, and 200 ms of combo time: an undo record of three registers.  (A full copy of the board in registers cost
            // ~80 of them in every lane of every step; loading the state again and replaying the keys on EVERY rollback made the
            // slowest wave of most launches ~2 us longer.)  The chained kernel — which has to stay within 128 registers for two
            // launches of 64k games to fit on the device — falls back to that reload where the record does not do; a wave that
            // takes it (1-2 % of them per launch) delays only its own chain.  The un-chained kernels keep the copy in registers
            // instead (they have room): there a launch ends with its SLOWEST wave, and one reload per launch cost every launch
            // 1.4 us (10.0 against 8.6 us, same box: profiles/r03/ab_r02.txt).
            if (!CHAIN && side == 1) pre = q;
            undo_pose = pose_pack(q);
            undo_group = q.pgroup; undo_draws = q.piece_draws;
            undo_cleared = q.lines_cleared; undo_ran = !g.round_over && !q.dead;
            wa = split_settle(cx, g);
        }
        const uint32_t opp_a = __shfl_xor(wa, 32);
        uint32_t wb0 = 0, wb1 = 0;
        if (active) {
            if (side == 1 && (opp_a & XW_DIED)) {
                if (!CHAIN) {
                    q = pre;
                } else if (undo_ran && q.lines_cleared == undo_cleared && !q.dead) {
                    undo_simple_settle(q, undo_pose, undo_group, undo_draws);
                } else if (undo_ran) {
                    // rows were cleared or the new piece did not fit (rare together with a rollback): nothing has been stored by
                    // this launch yet, so the state before this step is still in memory — load it again and replay the keys
                    load_player(br.s, br.o, br.ws, q, false, true, MEM);
                    prefetch_next(cx, q, g.seed16, g.status);
                    if (!g.round_over && !q.dead && acting == side) play_rt(cx, q, r, t);
                    sent_start = q.lines_sent;
                }
                wa = 0;
            }
            if (side == 0) {                                           // stage B0
                const int in = (!(wa & XW_DIED) && (opp_a & XW_RAN) && !(opp_a & XW_DIED)) ? xw_sent(opp_a) : 0;
                wb0 = split_tick(cx, g, a.ms, in);
            }
        }
        const uint32_t x0 = __shfl_xor(wb0, 32);
        if (active && side == 1) {                                     // stage B1
            const int in1 = ((opp_a & XW_RAN) && !(opp_a & XW_DIED)) ? xw_sent(opp_a) : 0;
            if (!g.round_over && in1 > 0) q.incoming = q.incoming + (float)in1 / 1.0f;
            wb1 = split_tick(cx, g, a.ms, (x0 & XW_DIED) ? 0 : xw_sent(x0));
        }
        const uint32_t x1 = __shfl_xor(wb1, 32);
        if (active) {                                                  // stage C
            const uint32_t opp_b = side == 0 ? x1 : x0;
            const int in = (side == 0 && !(opp_b & XW_DIED)) ? xw_sent(opp_b) : 0;
            g.flags = (uint32_t)side;
            done = split_finish(g, in, (opp_b & XW_DEAD_NOW) != 0, (opp_b & XW_ERR) != 0);
            out_reward = q.reward; out_dead = q.dead;                  // what the step reports: the state BEFORE an auto-reset
            if (ROLL) {
                g.steps++;
                if (!q.dead) my_lines += (unsigned)q.reward;
                my_sent += (q.lines_sent - sent_start) & 0xFFFFu;
            }
            if ((ROLL || AUTO) && done) {
                g.episode++;
                reset_split(cx, g, episode_seed(a.game_offset + (uint32_t)gi, g.episode));
            }
        }
    }
    const uint32_t opp_lines = __shfl_xor(my_lines, 32), opp_sent = __shfl_xor(my_sent, 32);
    if (active) {
        store_player(br.s, br.o, br.ws, q, false, true, MEM);
        if (!ROLL) {
            if (a.lines) a.lines[(size_t)side * a.n + gi] = (uint8_t)out_reward;
            if (a.dead) a.dead[(size_t)side * a.n + gi] = (uint8_t)out_dead;
        }
        const uint32_t st = g.status | __shfl_xor(g.status, 32);
        if (side == 0) {
            if (!ROLL && a.done) a.done[gi] = (uint8_t)done;
            g.flags = 0;
            g.add_lines = my_lines + opp_lines;
            g.add_sent = my_sent + opp_sent;
            store_game_words<1>(gr, g, ROLL, MEM);
            report_status(a, st);
        }
    }
    if (CHAIN) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every store (and counter atomic) of this wave has been acknowledged
        if (lane == 0) {                // (as in chain_body: no wait for the acknowledgement)
            if (AFFINE) st_xcd(a.chain + (size_t)wave * CHAIN_STRIDE, a.epoch);
            else st_agent(a.chain + (size_t)wave * CHAIN_STRIDE, a.epoch);
        }
        report_xcc();
    }
    if (OBS) {
        const int pitch = a.H * NCOL / 4, first = wave * 32;
        uint32_t* tile = s_duo_tile + ((size_t)(threadIdx.x >> 6) * 64 * pitch + 3) / 4 * 4;       // (16-byte aligned per wave)
        if (active) {
            const int sl = side == safe_player(a.next_player, gi, 2) ? 0 : 1;
            obs_build(a, tile + (size_t)(sl * 32 + (lane & 31)) * pitch, sl, gi, q.col[0], q.col[1], q.col[2], q.col[3], q.col[4], q.col[5], q.col[6],
                      q.col[7], q.col[8], q.col[9], q.x, q.y, q.next, q.kind, q.inc_count, q.combo_count, q.combo_remaining);
        }
        __syncthreads();
        const int nb = (a.n - first < 32) ? a.n - first : 32;
        if (nb > 0) {
            obs_stream(a, tile, 0, first, nb, lane);
            obs_stream(a, tile + (size_t)32 * pitch, 1, first, nb, lane);
        }
    }
}
template <int MODE, bool CHAIN = false, bool OBS = false>
__global__ __launch_bounds__(CHAIN ? 64 : 256) void k_duo(KArgs a) { duo_body<MODE, CHAIN, OBS, false>(a); }
__global__ __launch_bounds__(64) void k_duo_affine(KArgs a) { duo_body<M_ROLLOUT, true, false, true>(a); }

// Measurement / test aid: keeps a stream busy until the HOST sets `*go` (a word in pinned host memory; NULL: no such word) or
// `ticks` of the 100 MHz real-time clock have passed, whichever comes first.  TETRIS_PREQUEUE=1 parks the chain streams behind it
// while the host enqueues, so that every launch of the call is queued before the first one starts — the GPU-paced launch period
// without any host pacing; tetris_debug_stall uses it to hold a stream or the device's wave slots (tests of the give-up path).
__global__ void k_blocker(const uint32_t* go, unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) {
        if (go && __hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) break;
        __builtin_amdgcn_s_sleep(32);
    }
}

// Measurement aid (tetris_debug_clock_khz): shader clock of the moment, from the ratio of the shader cycle counter to the constant
// 100 MHz real-time counter over ~`ticks` of the latter, by one wave
__global__ void k_clock_probe(unsigned long long ticks, unsigned long long* out) {
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) { __builtin_amdgcn_s_sleep(4); r1 = __builtin_amdgcn_s_memrealtime(); }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}

// Sums the per-game cumulative rollout counters (G_STEPS, G_EPISODE, G_LINES, G_SENT): run once before and once
// after a rollout, outside its timed region, instead of any cross-lane reduction inside the step
// kernel (4096 same-address atomics per launch cost ~28 us; a shuffle + LDS + read-modify-write tail
// still ~1.2 us of a 8 us launch).
__global__ __launch_bounds__(256) void k_totals(Geo geo, unsigned long long* out /*[4]*/) {
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (int)geo.n_games; i += gridDim.x * blockDim.x) {
        unsigned long long t[4];
        totals_of_game(geo, i, t);
        v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
    }
    for (int k = 0; k < 4; k++) {
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
        if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd(&out[k], v[k]);
    }
}

// The per-game words as they stand, totals[k][i] (tetris_rollout_game_totals_dev; kept by a rollout call that reports counters), and
// what the games counted since such a copy: (now - before) mod 2^32 per game, summed in 64 bits.  The words are cumulative modulo
// 2^32, so the difference of two k_totals sums is off by 2^32 for every word that wrapped in between; this one is exact as long as
// no single game counts 2^32 between the two readings.
__global__ __launch_bounds__(256) void k_policy_totals(Geo geo, uint32_t* totals /*[4][N]*/) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int)geo.n_games) policy_game_totals_lane(geo, i, totals);
}
__global__ __launch_bounds__(256) void k_totals_since(Geo geo, const uint32_t* before /*[4][N]*/, unsigned long long* out /*[4]*/) {
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (int)geo.n_games; i += gridDim.x * blockDim.x) {
        unsigned long long t[4];
        totals_of_game(geo, i, t);
        for (int k = 0; k < 4; k++) v[k] += (uint32_t)((uint32_t)t[k] - before[(size_t)k * geo.n_games + i]);
    }
    for (int k = 0; k < 4; k++) {
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
        if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd(&out[k], v[k]);
    }
}
