// libtetris_hip.so — kernels and C ABI of the MI355X batched Tetris environment (gfx950 only), first translation unit: an include
// list and no function.  Every header below is part of this one translation unit, in dependency order; a kernel is
// defined in exactly one tetris_dev_*.h, or in tetris_game_kernel.h, which tetris_hip_multi.hip compiles too.
//
// One lane = one game (all its players), state SoA in HBM (tetris_layout.h), step logic in
// tetris_engine.h.  Launch geometry: 256-thread workgroups (one wave per SIMD of a CU); 64k games
// = 256 workgroups = one per CU, so the kernel is latency/issue bound, not occupancy bound.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <new>
#include <chrono>
#include <string>
#include <vector>

// ============================================================================ device side
#include "tetris_game_kernel.h"          // the step kernels of both translation units; `using namespace te;` for all that follows
#include "tetris_dev_vec.h"              // no kernel: the 16-byte vector helpers of the headers below
#include "tetris_dev_observe.h"
#include "tetris_dev_rollout.h"
#include "tetris_dev_core.h"
#include "tetris_dev_agent_plan.h"
#include "tetris_dev_act.h"
#include "tetris_dev_loss.h"             // (act_gather of tetris_dev_act.h)
#include "tetris_dev_kstep.h"
#include "tetris_dev_head.h"
#include "tetris_dev_kbd.h"
#include "tetris_dev_res.h"             // (the fragments of tetris_dev_kbd.h)
#include "tetris_dev_traj.h"
#include "tetris_dev_replay.h"           // (select_block_scan of tetris_dev_traj.h)
#include "tetris_dev_input.h"

// ============================================================================ host side (they launch the kernels above)
#include "tetris_lib_batch.h"
#include "tetris_lib_rollout.h"
#include "tetris_lib_core.h"
#include "tetris_lib_agent.h"
#include "tetris_lib_compose.h"          // entry points that only call other entry points: the CPU harness includes it too
