// Several samples per clip (option best_of): the start and the end of a chain that decodes N samples
// of each of its clips on rows r = j * clips + c (sample j of clip c).
//   best_of_begin  per row: the clip's prompt ids, n_ids, finished, the score sum and count, and the row's FIXED
//                  ancestor table for the gathered self_attention_long: the prompt's K / V below n_prompt - 1 are read
//                  from the clip's row c, everything behind them from the row itself
//   best_of_pick   per clip: the first sample with the largest sum / count in float64 (EOT counted, section 15's
//                  avg_logprob; a NaN never wins), its row copied to the clip's output row
// Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <cmath>

#include "error.h"
#include "kernels.h"

namespace wt {
namespace {

// grid (N * clips), 256 threads
__global__ __launch_bounds__(256) void best_of_begin(BestOfArgs a) {
  const int r = blockIdx.x, rows = a.N * a.clips, tid = threadIdx.x;
  if (r >= rows) return;
  const int c = r % a.clips;
  if (r != c) {  // rows c hold the prompts already
    const long long* const src = a.ids + (long)c * a.stride;
    long long* const dst = a.ids + (long)r * a.stride;
    for (int i = tid; i < a.stride; i += 256) dst[i] = i < a.n_prompt ? src[i] : 0ll;
  }
  unsigned char* const anc = a.anc + (long)r * a.cap;
  for (int k = tid; k < a.cap; k += 256) anc[k] = (unsigned char)(k < a.n_prompt - 1 ? c : r);
  if (tid == 0) {
    a.n_ids[r] = a.n_prompt;
    a.finished[r] = a.frozen && a.frozen[c] ? 1 : 0;
    a.sum[r] = 0.0;
    a.count[r] = 0;
  }
}

// grid (clips), one wavefront
__global__ __launch_bounds__(64) void best_of_pick(BestOfArgs a) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (c >= a.clips) return;
  const int o = a.c0 + c;
  int best = -1;  // (every lane ranks the N <= 8 samples: the same result, no exchange)
  double best_avg = 0.0;
  for (int j = 0; j < a.N; ++j) {
    const int r = j * a.clips + c, n = a.count[r];
    const double avg = n >= 1 ? a.sum[r] / (double)n : NAN;
    if (!(avg != avg) && (best < 0 || avg > best_avg)) best = j, best_avg = avg;
  }
  if (best < 0) best = 0;
  const int r = best * a.clips + c;
  const int n = min(max(a.n_ids[r], 0), a.stride);
  const long long* const ids = a.ids + (long)r * a.stride;
  const float* const lp = a.lp + (long)r * a.stride;
  for (int i = lane; i < a.stride; i += 64) {
    a.out_ids[(long)o * a.stride + i] = i < n ? ids[i] : 0ll;
    a.out_lp[(long)o * a.stride + i] = i < n ? lp[i] : 0.0f;
  }
  if (lane < kSampleGroupMax) {
    const bool in = lane < a.N;
    a.all_sum[o * kSampleGroupMax + lane] = in ? a.sum[lane * a.clips + c] : 0.0;
    a.all_count[o * kSampleGroupMax + lane] = in ? a.count[lane * a.clips + c] : 0;
  }
  if (lane == 0) {
    a.out_n[o] = n;
    a.out_sum[o] = a.sum[r];
    a.out_count[o] = a.count[r];
    a.picked[o] = best;
  }
}

void check_shape(const BestOfArgs& a, const char* who) {
  if (a.N < 1 || a.N > kSampleGroupMax || a.clips < 1 || a.N * a.clips > kSampleRowsMax || a.c0 < 0 ||
      a.c0 + a.clips > kSampleClipsMax || a.n_prompt < 1 || a.n_prompt > a.cap || a.cap > kSelfLongCap || a.cap >= a.stride) {
    throw Error(kErrInvalidArg, std::string(who) + ": needs 1 .. 8 samples per clip, at most 128 rows and 64 clips, 1 <= n_prompt <= cap < stride, cap <= 448");
  }
}

}  // namespace

void launch_best_of_begin(const BestOfArgs& a, hipStream_t s) {
  check_shape(a, "best_of_begin");
  if (!a.ids || !a.n_ids || !a.finished || !a.sum || !a.count || !a.anc) throw Error(kErrInvalidArg, "best_of_begin: null array");
  hipLaunchKernelGGL(best_of_begin, dim3(a.N * a.clips), dim3(256), 0, s, a);
}

void launch_best_of_pick(const BestOfArgs& a, hipStream_t s) {
  check_shape(a, "best_of_pick");
  if (!a.ids || !a.lp || !a.n_ids || !a.sum || !a.count || !a.out_ids || !a.out_lp || !a.out_n || !a.out_count || !a.picked ||
      !a.out_sum || !a.all_sum || !a.all_count) {
    throw Error(kErrInvalidArg, "best_of_pick: null array");
  }
  hipLaunchKernelGGL(best_of_pick, dim3(a.clips), dim3(64), 0, s, a);
}

}  // namespace wt
