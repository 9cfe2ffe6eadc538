// Host-side helpers shared by the row-kernel translation units: the launch status macros and the grid sizes of the element-wise
// sweeps.
#pragma once
#include "common.h"

namespace rl {

#define RL_LAUNCH_CHECK() (hipGetLastError() == hipSuccess ? RL_OK : RL_ERR_LAUNCH)
#define RL_TRY(expr) do { const int _rc = (expr); if (_rc != RL_OK) return _rc; } while (0)

// log2 of a power of two, -1 for anything else
static inline int pow2_shift(int C) { int s = 0; while (s < 31 && (1 << s) < C) ++s; return (1 << s) == C ? s : -1; }
// workgroups of a grid-stride sweep: 256 threads over n4 items, 4096 at most; the 16-byte form walks four items per thread, 2048 at most
static inline int ew_blocks(int64_t n4) { int64_t b = (n4 + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }
static inline int ew16_blocks(int64_t n8) { int64_t b = (n8 + 255) / 256; b = (b + 3) / 4; return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b)); }

}  // namespace rl
