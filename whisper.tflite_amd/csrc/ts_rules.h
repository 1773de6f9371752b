// The interval form of Whisper's timestamp rules 1 .. 4, shared by the kernels that choose under them
// (k_timestamps.hip) and the kernels that score the choice (k_scores.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace wt {
namespace {

struct Allowed {
  int t_lo, t_hi, s_lo, s_hi;  // inclusive id intervals; lo > hi: empty
};

// rules 1 .. 4 for a clip that has generated n_gen ids
__device__ __forceinline__ Allowed allowed_of(const TsState st, int n_gen, int V, int eot, int beg, int mit) {
  const bool last_ts = n_gen >= 1 && st.last_is_ts != 0;
  const bool pen_ts = n_gen < 2 || st.prev_is_ts != 0;
  Allowed a;
  a.t_lo = 0, a.t_hi = eot;      // rule 1: (eot, beg) is never allowed
  a.s_lo = beg, a.s_hi = V - 1;
  if (last_ts && pen_ts) a.s_lo = V;   // rule 2: a pair is complete, text (or EOT) follows
  if (last_ts && !pen_ts) a.t_lo = eot;  //         a segment was closed: its pair (or EOT) follows
  const int tick = min(max(st.tick, -1), V - 1 - beg);  // (the state is data: bounded)
  if (tick >= 0) a.s_lo = max(a.s_lo, beg + tick + (last_ts && !pen_ts ? 0 : 1));  // rule 3
  if (n_gen == 0) {                                                                 // rule 4
    a.t_lo = 1, a.t_hi = 0;
    if (mit >= 0) a.s_hi = min(a.s_hi, beg + mit);
  }
  return a;
}

}  // namespace
}  // namespace wt
