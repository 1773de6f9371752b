// Logit suppression (wt_engine_set_suppress): Whisper's SuppressTokens and SuppressBlank filters, in
// front of every other decoding rule of a full-length chain.
//   suppress_logits   per row: -inf into the cells of the always-list, and of the first-list when `first` is set
// The lists are one device buffer, the always-ids then the first-ids; only the counts and the flag are launch
// constants, so a captured launch reads whatever the buffer holds when it is replayed.  A logit of -inf is outside every
// allowed set behind it (ts_partial, sample_partial, score_partial, beam_full_partial: its exp adds an exact 0 and its
// key never wins against a finite one).  Stores only: no logit is read, duplicates write the same value twice, and an id
// outside [0, V) — the buffer is data — is skipped, so nothing beyond column V - 1 is touched.
#include <hip/hip_runtime.h>

#include <cmath>

#include "error.h"
#include "kernels.h"

namespace wt {
namespace {

constexpr int kThreads = 256;

// grid = rows
__global__ __launch_bounds__(kThreads) void suppress_logits(float* __restrict__ logits, int ldl, int V,
                                                            const int* __restrict__ ids, int n, int n_first, int first) {
  float* const z = logits + (long)blockIdx.x * ldl;
  const int total = n + (first ? n_first : 0);
  for (int i = threadIdx.x; i < total; i += kThreads) {
    const int id = ids[i];
    if (id >= 0 && id < V) z[id] = -INFINITY;
  }
}

}  // namespace

void launch_suppress_logits(const SuppressArgs& a, hipStream_t s) {
  if (!a.logits || !a.ids || a.rows < 1 || a.rows > kSuppressRowsMax || a.V < 1 || a.ldl < a.V || a.n < 0 ||
      a.n > kSuppressIdsMax || a.n_first < 0 || a.n_first > kSuppressIdsMax) {
    throw Error(kErrInvalidArg, "suppress_logits: needs 1 .. 128 rows, V <= ldl, non-null pointers and at most 1024 ids per list");
  }
  hipLaunchKernelGGL(suppress_logits, dim3(a.rows), dim3(kThreads), 0, s, a.logits, a.ldl, a.V, a.ids, a.n, a.n_first,
                     a.first ? 1 : 0);
}

}  // namespace wt
