// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// The CPU test harness with every entry point of harness_traj.cpp (included whole) plus tetris_traj_observe_dev,
// tetris_traj_select_dev and tetris_traj_batch_dev of include/tetris_hip.h as plain host loops over the same bodies
// (drl-tetris_amd/csrc/tetris_batch.h: traj_observe_slot, select_bits / select_emit, batch_sample_slot).  "Device" pointers are
// host pointers here.  __graft_entry__.build_harness compiles this file into libtetris_cpu_harness.so.  The checks and the
// argument structs' fills are the product's (tetris_host.h: traj_observe_args, traj_select_args, traj_batch_args).
#include "harness_traj.cpp"

extern "C" {

// mask bytes per workgroup of the product's selection kernels: the sizes around which tests/test_traj_batch.py puts its shapes
extern const int tetris_harness_select_elems = SELECT_ELEMS;

int tetris_traj_observe_dev(tetris_batch* b, const tetris_traj_obs* obs, int row, const uint8_t* d_player) {
    TrajObserveArgs oa;
    int rc = traj_observe_args(shape_of(b), geo_of_batch(b), obs, row, d_player, oa);
    if (rc) return rc;
    for (int sl = 0; sl < b->P; sl++)
        for (int i = 0; i < b->N; i++) traj_observe_slot(oa, i, sl);
    return TETRIS_OK;
}

int tetris_traj_select_dev(tetris_batch* b, const uint8_t* d_mask, int rows, int flags, int32_t* d_index, long long cap,
                           int32_t* d_count) {
    TrajSelectArgs sa;
    int rc = traj_select_args(shape_of(b), d_mask, rows, flags, d_index, cap, d_count, sa); if (rc) return rc;
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
    int rc = traj_batch_args(shape_of(b), traj, obs, d_adv_in, d_target_in, d_index, M, out, ba); if (rc) return rc;
    for (int sl = 0; sl < b->P; sl++)
        for (int j = 0; j < M; j++) batch_sample_slot(ba, j, sl);
    return TETRIS_OK;
}

}  // extern "C"
