// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// libtetris_cpu_harness.so, its one translation unit: an include list and no function, laid out like tetris_hip.hip.
//
// Compiles the product's kernel bodies (drl-tetris_amd/csrc/tetris_kernels.h, tetris_engine.h,
// tetris_tables.h — the exact sources hipcc builds for gfx950) with g++ and wraps them in plain
// loops over host memory, behind the same C symbols as include/tetris_hip.h.  Purpose: let the
// `-m "not gpu"` suite check the bitboard step logic, the RNG tables and the SoA load/store
// against the oracle in a container that has no GPU.  Only tests/ loads this library, always by
// explicit path; the product binding (drl-tetris_amd/capi.py) loads libtetris_hip.so and nothing else.
//
// The host rules of an entry point — its argument checks, the filling of its kernel-argument struct, the repacking of keys,
// lens, lines and dead, the gathering of tetris_get_actions, the flag words' TETRIS_ERR_* bits, the last error — are the
// product's own: drl-tetris_amd/csrc/tetris_host.h, which tetris_hip.hip includes too; so are the entry points that only call
// other entry points (tetris_lib_compose.h).  What is written in the harness_lib_*.h headers is what differs: the tables, host
// vectors for device memory, loops over lanes for launches.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#define TE_PATH_COUNTERS 1
#include "../../drl-tetris_amd/csrc/tetris_host.h"

// ============================================================================ host side (loops over the kernel bodies above)
#include "harness_lib_batch.h"
#include "harness_lib_rollout.h"
#include "harness_lib_core.h"            // the harness-only exports are at its end
#include "harness_lib_agent.h"
#include "../../drl-tetris_amd/csrc/tetris_lib_compose.h"
