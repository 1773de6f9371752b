// Decode confidence (option scores): the log-probability of the id a greedy step chose and the
// no-speech probability of a clip, between the selection kernel of a step and the next decoder pass of a full-length chain.
//   score_partial    per (clip, 4096-entry vocabulary chunk): max and sum of exp of the allowed text ids and of the
//                    allowed timestamps
//   score_finish     per clip: merges its records in chunk order in float64, decides rule 5 as ts_select does, writes
//                    lp = z[tok] - logsumexp(allowed) and carries the clip's sum and count
//   no_speech_finish per clip: exp(z0[nosp] - logsumexp(z0)) from the records of the position-0 row
// A step's allowed set is two inclusive id intervals, text and timestamps (ts_rules.h); without timestamps the text
// interval is the whole vocabulary and the other one empty.  Every result is a function of the row's logits, its
// intervals and its carried sum alone: the chunking is fixed (kTsChunk), a chunk's reductions have a fixed shape — a
// thread's values in index order, lanes by butterfly, wavefronts left to right, the shape of ts_partial, so the
// timestamp sums are ts_partial's bit for bit — and the chunks are merged in index order by one lane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "error.h"
#include "kernels.h"
#include "ts_rules.h"

namespace wt {
namespace {

constexpr int kThreads = 256;
constexpr int kQuads = kTsChunk / (4 * kThreads);  // 16-byte loads per thread

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// grid (chunks, clips): thread t holds the 4 consecutive entries chunk * 4096 + j * 1024 + 4 t .. + 3, j = 0 .. 3.
// state == nullptr: plain mode, text = [0, V - 1] and no timestamps; else the intervals of allowed_of(state[row]).
__global__ __launch_bounds__(kThreads) void score_partial(const float* __restrict__ logits, int ldl, int V,
                                                          const TsState* __restrict__ state, int n_gen, int eot, int beg,
                                                          int mit, ScorePart* __restrict__ part) {
  __shared__ float red[2][4];
  const int chunk = blockIdx.x, row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  Allowed a;
  a.t_lo = 0, a.t_hi = V - 1, a.s_lo = V, a.s_hi = V - 1;
  if (state) a = allowed_of(state[row], n_gen, V, eot, beg, mit);
  const float* z = logits + (long)row * ldl;  // ldl % 4 == 0 and a 16-byte base: every quad below is aligned
  float v[4 * kQuads];
  float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
  for (int j = 0; j < kQuads; ++j) {
    const int i0 = chunk * kTsChunk + j * 4 * kThreads + 4 * tid;
    float4 q = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (i0 < V) q = *reinterpret_cast<const float4*>(z + i0);  // (i0 + 3 < ldl: the row's padding is readable)
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + c;
      v[4 * j + c] = e[c];
      if (i >= a.t_lo && i <= a.t_hi) mt = fmaxf(mt, e[c]);  // (t_hi, s_hi < V: the padding is in neither interval)
      if (i >= a.s_lo && i <= a.s_hi) ms = fmaxf(ms, e[c]);
    }
  }
  mt = wave_max_f(mt);
  ms = wave_max_f(ms);
  if (lane == 0) red[0][wid] = mt, red[1][wid] = ms;
  __syncthreads();
  mt = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));  // a maximum: exact in any order
  ms = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  __syncthreads();
  float st = 0.0f, ss = 0.0f;
  if (mt != -INFINITY) {  // (block-uniform; an entry outside the interval adds exp(-inf) = 0, as in ts_partial)
#pragma unroll
    for (int j = 0; j < 4 * kQuads; ++j) {
      const int i = chunk * kTsChunk + (j >> 2) * 4 * kThreads + 4 * tid + (j & 3);
      st += expf((i >= a.t_lo && i <= a.t_hi ? v[j] : -INFINITY) - mt);
    }
  }
  if (ms != -INFINITY) {
#pragma unroll
    for (int j = 0; j < 4 * kQuads; ++j) {
      const int i = chunk * kTsChunk + (j >> 2) * 4 * kThreads + 4 * tid + (j & 3);
      ss += expf((i >= a.s_lo && i <= a.s_hi ? v[j] : -INFINITY) - ms);
    }
  }
  st = wave_sum_f(st);
  ss = wave_sum_f(ss);
  if (lane == 0) red[0][wid] = st, red[1][wid] = ss;
  __syncthreads();
  if (tid == 0) {
    ScorePart* const out = part + ((long)row * gridDim.x + chunk);
    out->mt = mt;
    out->st = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    out->ms = ms;
    out->ss = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    out->has_t = a.t_lo <= a.t_hi;  // (the same in every chunk of the clip)
    out->has_s = a.s_lo <= a.s_hi;
  }
}

struct Merged {
  float mt, ms;     // maxima of the two intervals over the chunks
  double St, Ss;    // sum_c s_c exp(m_c - m), chunks in index order (Ss: ts_select's S)
  bool has_t, has_s;
};

__device__ __forceinline__ Merged merge_parts(const ScorePart* sp, int n_chunks) {
  Merged g;
  g.mt = g.ms = -INFINITY;
  g.St = g.Ss = 0.0;
  g.has_t = sp[0].has_t != 0, g.has_s = sp[0].has_s != 0;
  for (int c = 0; c < n_chunks; ++c) g.mt = fmaxf(g.mt, sp[c].mt), g.ms = fmaxf(g.ms, sp[c].ms);
  for (int c = 0; c < n_chunks; ++c) {
    if (sp[c].mt != -INFINITY) g.St += (double)sp[c].st * exp((double)sp[c].mt - (double)g.mt);
    if (sp[c].ms != -INFINITY) g.Ss += (double)sp[c].ss * exp((double)sp[c].ms - (double)g.ms);
  }
  return g;
}

// logsumexp over both intervals (or over the timestamps alone); -inf when nothing finite is in them
__device__ __forceinline__ double denominator_of(const Merged& g, bool ts_only) {
  const double Lt = g.mt != -INFINITY ? (double)g.mt + log(g.St) : -INFINITY;
  const double Ls = g.ms != -INFINITY ? (double)g.ms + log(g.Ss) : -INFINITY;
  if (ts_only || Lt == -INFINITY) return Ls;
  if (Ls == -INFINITY) return Lt;
  const double hi = fmax(Lt, Ls), lo = fmin(Lt, Ls);
  return hi + log1p(exp(lo - hi));
}

// one wavefront per clip, after the selection kernel of the step wrote ids[b][pos + 1] and n_ids[b]
__global__ __launch_bounds__(64) void score_finish(const ScorePart* __restrict__ part, int n_chunks,
                                                   const float* __restrict__ logits, int ldl, int V,
                                                   const long long* __restrict__ ids, int ids_stride, int pos,
                                                   const int* __restrict__ n_ids, float* __restrict__ token_logprob,
                                                   int lp_stride, double* __restrict__ sum, int* __restrict__ count,
                                                   double* dbg_den) {
  __shared__ ScorePart sp[kTsMaxChunks];
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < n_chunks; c += 64) sp[c] = part[(long)b * n_chunks + c];
  __syncthreads();
  if (threadIdx.x != 0) return;
  const Merged g = merge_parts(sp, n_chunks);
  // rule 5 exactly as ts_select decides it: both intervals non-empty and L > M, M the text interval's maximum
  const double L = (g.has_s && g.ms != -INFINITY) ? (double)g.ms + log(g.Ss) : -INFINITY;
  const bool ts_only = g.has_t && g.has_s && L > (double)g.mt;
  const double D = denominator_of(g, ts_only);
  long long tok = ids[(long)b * ids_stride + pos + 1];
  tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);  // (the id is data: bounded before it indexes the row)
  const float zt = logits[(long)b * ldl + tok];
  const float lp = D == -INFINITY ? -INFINITY : (float)((double)zt - D);
  token_logprob[(long)b * lp_stride + pos + 1] = lp;
  if (dbg_den) dbg_den[b] = D;
  if (n_ids[b] == pos + 2) {  // the clip was live at this step (select_token / ts_select count only then)
    sum[b] += (double)lp;
    count[b] += 1;
  }
}

// the records of the position-0 row over the whole vocabulary -> p(nosp)
__global__ __launch_bounds__(64) void no_speech_finish(const ScorePart* __restrict__ part, int n_chunks,
                                                       const float* __restrict__ logits, int ldl, int nosp,
                                                       float* __restrict__ prob) {
  __shared__ ScorePart sp[kTsMaxChunks];
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < n_chunks; c += 64) sp[c] = part[(long)b * n_chunks + c];
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double D = denominator_of(merge_parts(sp, n_chunks), false);
  const float z = logits[(long)b * ldl + nosp];
  prob[b] = D == -INFINITY ? 0.0f : (float)exp((double)z - D);
}

void check_rows(const ScoreArgs& a, const char* who) {
  if (a.batch < 1 || a.V < 2 || ts_chunks(a.V) > kTsMaxChunks || a.ldl < a.V || a.ldl % 4 != 0 ||
      (reinterpret_cast<uintptr_t>(a.logits) & 15) != 0 || !a.logits || !a.part) {
    throw Error(kErrInvalidArg, std::string(who) + ": needs 2 <= V <= 4096 * 64 and 16-byte aligned logits rows (ldl % 4 == 0)");
  }
}

}  // namespace

void launch_score_partial(const ScoreArgs& a, hipStream_t s) {
  check_rows(a, "score_partial");
  if (a.state && (a.eot < 0 || a.eot >= a.beg || a.beg >= a.V || a.n_gen < 0 || a.max_initial < -1)) {
    throw Error(kErrInvalidArg, "score_partial: the timestamp rules need 0 <= eot < beg < V");
  }
  hipLaunchKernelGGL(score_partial, dim3(ts_chunks(a.V), a.batch), dim3(kThreads), 0, s, a.logits, a.ldl, a.V, a.state,
                     a.n_gen, a.eot, a.beg, a.max_initial, a.part);
}

void launch_score_finish(const ScoreArgs& a, hipStream_t s) {
  check_rows(a, "score_finish");
  if (!a.ids || !a.n_ids || !a.token_logprob || !a.sum || !a.count || a.pos < 0 || a.pos + 1 >= a.ids_stride ||
      a.pos + 1 >= a.lp_stride) {
    throw Error(kErrInvalidArg, "score_finish: needs pos + 1 < ids_stride and pos + 1 < lp_stride");
  }
  hipLaunchKernelGGL(score_finish, dim3(a.batch), dim3(64), 0, s, a.part, ts_chunks(a.V), a.logits, a.ldl, a.V, a.ids,
                     a.ids_stride, a.pos, a.n_ids, a.token_logprob, a.lp_stride, a.sum, a.count, a.dbg_den);
}

void launch_no_speech_prob(const ScoreArgs& a, int nosp, float* prob, hipStream_t s) {
  check_rows(a, "no_speech_prob");
  if (nosp < 0 || nosp >= a.V || !prob) throw Error(kErrInvalidArg, "no_speech_prob: the no-speech id must lie in [0, V)");
  hipLaunchKernelGGL(score_partial, dim3(ts_chunks(a.V), a.batch), dim3(kThreads), 0, s, a.logits, a.ldl, a.V,
                     static_cast<const TsState*>(nullptr), 0, 0, 0, -1, a.part);
  hipLaunchKernelGGL(no_speech_finish, dim3(a.batch), dim3(64), 0, s, a.part, ts_chunks(a.V), a.logits, a.ldl, nosp, prob);
}

}  // namespace wt
