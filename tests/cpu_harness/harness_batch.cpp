// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// The CPU test harness with every entry point of harness_traj.cpp (included whole) plus tetris_traj_observe_dev,
// tetris_traj_select_dev and tetris_traj_batch_dev of include/tetris_hip.h as plain host loops over the same bodies
// (drl-tetris_amd/csrc/tetris_batch.h: traj_observe_slot, select_bits / select_emit, batch_sample_slot).  "Device" pointers are
// host pointers here.  __graft_entry__.build_harness compiles this file into libtetris_cpu_harness.so.
#include "harness_traj.cpp"

#include "../../drl-tetris_amd/csrc/tetris_batch.h"

// the argument checks of the product (tetris_hip.hip: traj_batch_rules, traj_obs_check, traj_select_args, traj_batch_args)
static int traj_batch_rules(tetris_batch* b, const char* what) {
    if (b->split) return fail(TETRIS_E_ARG, what);
    if (b->P > 2) return fail(TETRIS_E_ARG, "the packed observation is defined for one or two players (own / opponent's board: state_unpack.py:88-137)");
    return TETRIS_OK;
}

static int traj_obs_check(tetris_batch* b, const tetris_traj_obs* obs) {
    if (!obs || !obs->d_obs) return fail(TETRIS_E_ARG, "the observation records are NULL");
    if (((uintptr_t)obs->d_obs) & 15u) return fail(TETRIS_E_ARG, "d_obs must be 16-byte aligned");
    if (obs->capacity < 1 || (unsigned long long)obs->capacity * (unsigned long long)b->N >= (1ull << 31)) return fail(TETRIS_E_ARG, "the window must hold between 1 and 2^31 - 1 entries");
    return TETRIS_OK;
}

static int traj_select_args(tetris_batch* b, const uint8_t* d_mask, int rows, int flags, int32_t* d_index, long long cap, int32_t* d_count,
                            TrajSelectArgs& sa) {
    int rc = traj_batch_rules(b, "tetris_traj_select_dev is not available on split batches");
    if (rc) return rc;
    if (!d_mask || !d_index || !d_count) return fail(TETRIS_E_ARG, "mask/index/count are NULL");
    if (flags & ~TETRIS_SELECT_AUGMENT) return fail(TETRIS_E_ARG, "unknown flag");
    if (rows < 1 || cap < 0) return fail(TETRIS_E_ARG, "rows < 1 or cap < 0");
    if ((unsigned long long)rows * (unsigned long long)b->N >= (1ull << 31)) return fail(TETRIS_E_ARG, "rows * N must be below 2^31");
    sa.mask = d_mask; sa.total = (uint32_t)rows * (uint32_t)b->N; sa.augment = flags & TETRIS_SELECT_AUGMENT;
    sa.index = d_index; sa.cap = cap; sa.count = d_count;
    sa.nblocks = (int)((sa.total + SELECT_ELEMS - 1) / SELECT_ELEMS);
    sa.blocks = nullptr;
    return TETRIS_OK;
}

static int traj_batch_args(tetris_batch* b, const tetris_traj* traj, const tetris_traj_obs* obs, const float* d_adv_in, const float* d_target_in,
                           const int32_t* d_index, int M, const tetris_traj_batch* out, TrajBatchArgs& ba) {
    int rc = traj_batch_rules(b, "tetris_traj_batch_dev is not available on split batches");
    if (rc) return rc;
    if (!traj || !out || !d_index) return fail(TETRIS_E_ARG, "the window, the outputs or the index list are NULL");
    if ((rc = traj_obs_check(b, obs))) return rc;
    if (!traj->d_action || !traj->d_prob || !traj->d_reward || !traj->d_done) return fail(TETRIS_E_ARG, "an array of the window is NULL");
    if (traj->capacity != obs->capacity) return fail(TETRIS_E_ARG, "the window and its observation records differ in capacity");
    if (M < 0) return fail(TETRIS_E_ARG, "M < 0");
    ba.m = M; ba.n_slots = b->P; ba.H = b->H;
    ba.total = (uint32_t)traj->capacity * (uint32_t)b->N;
    ba.index = d_index; ba.obs = obs->d_obs;
    ba.action = traj->d_action; ba.prob = traj->d_prob; ba.reward = traj->d_reward; ba.done = traj->d_done;
    ba.adv = d_adv_in; ba.target = d_target_in;
    ba.visual = out->d_visual; ba.vector = out->d_vector; ba.piece = out->d_piece; ba.action_out = out->d_action;
    ba.prob_out = out->d_prob; ba.adv_out = out->d_adv; ba.target_out = out->d_target; ba.reward_out = out->d_reward;
    ba.done_out = out->d_done; ba.valid = out->d_valid;
    return TETRIS_OK;
}

extern "C" {

// mask bytes per workgroup of the product's selection kernels: the sizes around which tests/test_traj_batch.py puts its shapes
extern const int tetris_harness_select_elems = SELECT_ELEMS;

int tetris_traj_observe_dev(tetris_batch* b, const tetris_traj_obs* obs, int row, const uint8_t* d_player) {
    int rc;
    if ((rc = traj_batch_rules(b, "tetris_traj_observe_dev is not available on split batches")) || (rc = traj_obs_check(b, obs))) return rc;
    if (row < 0 || row >= obs->capacity) return fail(TETRIS_E_ARG, "row outside the window");
    TrajObserveArgs oa;
    oa.geo = geo_of_batch(b); oa.n = b->N; oa.n_players = b->P; oa.player = d_player;
    oa.obs = obs->d_obs + (size_t)row * (size_t)b->N * (size_t)b->P * OBS_WORDS;
    for (int sl = 0; sl < b->P; sl++)
        for (int i = 0; i < b->N; i++) traj_observe_slot(oa, i, sl);
    return TETRIS_OK;
}

int tetris_traj_select_dev(tetris_batch* b, const uint8_t* d_mask, int rows, int flags, int32_t* d_index, long long cap,
                           int32_t* d_count) {
    TrajSelectArgs sa;
    int rc = traj_select_args(b, d_mask, rows, flags, d_index, cap, d_count, sa); if (rc) return rc;
    long long k = 0;
    for (uint32_t base = 0; base < sa.total; base += 16u) k += __builtin_popcount(select_bits(sa, base));
    long long pos = 0;
    for (uint32_t base = 0; base < sa.total; base += 16u) {
        const uint32_t bits = select_bits(sa, base);
        select_emit(sa, base, bits, pos, k);
        pos += __builtin_popcount(bits);
    }
    for (long long p = sa.augment ? 2 * k : k; p < sa.cap; p++) sa.index[p] = -1;
    *sa.count = (int32_t)(sa.augment ? 2 * k : k);
    return TETRIS_OK;
}

int tetris_traj_batch_dev(tetris_batch* b, const tetris_traj* traj, const tetris_traj_obs* obs, const float* d_adv_in,
                          const float* d_target_in, const int32_t* d_index, int M, const tetris_traj_batch* out) {
    TrajBatchArgs ba;
    int rc = traj_batch_args(b, traj, obs, d_adv_in, d_target_in, d_index, M, out, ba); if (rc) return rc;
    for (int sl = 0; sl < b->P; sl++)
        for (int j = 0; j < M; j++) batch_sample_slot(ba, j, sl);
    return TETRIS_OK;
}

}  // extern "C"
