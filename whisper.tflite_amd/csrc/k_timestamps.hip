// Timestamp decoding (option timestamps): Whisper's decoding-time logit filter and the greedy step
// behind it, between the logits GEMM and the next decoder pass of a full-length chain.
//   ts_state_init   per clip: the carried state from the ids generated so far (chain start, debug tap)
//   ts_partial      per (clip, 4096-entry vocabulary chunk): best allowed key below `beg`, best allowed timestamp key,
//                   max and sum of exp of the allowed timestamps
//   ts_select       per clip: merges its records in chunk order, decides logsumexp(timestamps) against the best text
//                   logit, writes the token, n_ids, finished and the clip's state
// The rules mask RANGES of ids (kernels.h), so a clip's step is two intervals: text [t_lo, t_hi] and timestamps
// [s_lo, s_hi].  Every result is a function of the row's logits and its state alone: the chunking is fixed (kTsChunk),
// a chunk's reductions have a fixed shape, and the chunks are merged in index order by one lane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "error.h"
#include "kernels.h"
#include "ts_rules.h"

namespace wt {
namespace {

constexpr int kThreads = 256;
constexpr int kQuads = kTsChunk / (4 * kThreads);  // 16-byte loads per thread

// float -> unsigned with the same order, -0 and +0 one value (as k_beam.hip); key = ord << 32 | id, 0 = none
__device__ __forceinline__ unsigned ord_of(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? (u == 0x80000000u ? 0x80000000u : ~u) : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}
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

// grid (chunks, clips): thread t holds the 4 consecutive entries chunk * 4096 + j * 1024 + 4 t .. + 3, j = 0 .. 3
__global__ __launch_bounds__(kThreads) void ts_partial(const float* __restrict__ logits, int ldl, int V,
                                                       const TsState* __restrict__ state, int n_gen, int eot, int beg,
                                                       int mit, TsPart* __restrict__ part) {
  __shared__ float red[4];
  __shared__ unsigned long long kred[2][4];
  const int chunk = blockIdx.x, row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const Allowed a = allowed_of(state[row], n_gen, V, eot, beg, mit);
  const float* z = logits + (long)row * ldl;  // ldl % 4 == 0 and a 16-byte base: every quad below is aligned
  float v[4 * kQuads];
  unsigned long long kt = 0ull, ks = 0ull;
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < kQuads; ++j) {
    const int i0 = chunk * kTsChunk + j * 4 * kThreads + 4 * tid;
    float4 q = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (i0 < V) q = *reinterpret_cast<const float4*>(z + i0);  // (i0 + 3 < ldl: the row's padding is readable)
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + c;
      const unsigned long long key = ((unsigned long long)ord_of(e[c]) << 32) | (unsigned)i;
      const bool is_t = i >= a.t_lo && i <= a.t_hi, is_s = i >= a.s_lo && i <= a.s_hi;  // (s_hi < V)
      if (is_t && key > kt) kt = key;
      if (is_s && key > ks) ks = key;
      v[4 * j + c] = is_s ? e[c] : -INFINITY;
      m = fmaxf(m, v[4 * j + c]);
    }
  }
  m = wave_max_f(m);
  kt = wave_max_u64(kt);
  ks = wave_max_u64(ks);
  if (lane == 0) red[wid] = m, kred[0][wid] = kt, kred[1][wid] = ks;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));  // a maximum: exact in any order
  __syncthreads();
  float s = 0.0f;
  if (m != -INFINITY) {  // (block-uniform; exp(-inf - m) = 0 for the masked entries)
#pragma unroll
    for (int j = 0; j < 4 * kQuads; ++j) s += expf(v[j] - m);
  }
  s = wave_sum_f(s);
  if (lane == 0) red[wid] = s;
  __syncthreads();
  if (tid == 0) {
    TsPart* const out = part + ((long)row * gridDim.x + chunk);
    for (int w = 1; w < 4; ++w) {
      kt = kred[0][w] > kt ? kred[0][w] : kt;
      ks = kred[1][w] > ks ? kred[1][w] : ks;
    }
    out->key_text = kt;
    out->key_ts = ks;
    out->m = m;
    out->s = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

// one wavefront per clip
__global__ __launch_bounds__(64) void ts_select(const TsPart* __restrict__ part, int n_chunks, long long* ids,
                                                int ids_stride, int pos, int* n_ids, int* finished,
                                                TsState* __restrict__ state, int beg, long long eot, int stop_at_eot,
                                                double* dbg_L, float* dbg_M) {
  __shared__ TsPart sp[kTsMaxChunks];
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < n_chunks; c += 64) sp[c] = part[(long)b * n_chunks + c];
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned long long kt = 0ull, ks = 0ull;
  float m = -INFINITY;
  for (int c = 0; c < n_chunks; ++c) {
    kt = sp[c].key_text > kt ? sp[c].key_text : kt;
    ks = sp[c].key_ts > ks ? sp[c].key_ts : ks;
    m = fmaxf(m, sp[c].m);
  }
  // rule 5 in double: L = m + log(sum_c s_c exp(m_c - m)), chunks in index order
  double S = 0.0;
  for (int c = 0; c < n_chunks; ++c) {
    if (sp[c].m != -INFINITY) S += (double)sp[c].s * exp((double)sp[c].m - (double)m);
  }
  const double L = (ks != 0ull && m != -INFINITY) ? (double)m + log(S) : -INFINITY;
  const float M = kt != 0ull ? float_of((unsigned)(kt >> 32)) : -INFINITY;
  if (dbg_L) dbg_L[b] = ks != 0ull ? L : NAN;  // NaN: no such id is allowed
  if (dbg_M) dbg_M[b] = kt != 0ull ? M : NAN;
  if (kt != 0ull && ks != 0ull && L > (double)M) kt = 0ull;
  // rule 6: the allowed set is never empty, so one of the keys exists
  const unsigned long long p = kt > ks ? kt : ks;
  const long long tok = (long long)(unsigned)(p & 0xffffffffull);
  ids[(long)b * ids_stride + pos + 1] = tok;
  if (!finished[b]) {  // as select_token
    n_ids[b] = pos + 2;
    if (stop_at_eot && tok == eot) finished[b] = 1;
  }
  TsState st = state[b];
  st.prev_is_ts = st.last_is_ts;
  st.last_is_ts = tok >= beg;
  if (tok >= beg) st.tick = (int)(tok - beg);
  state[b] = st;
}

// the state of a clip whose row holds n ids, the first sample_begin of them the prompt
__global__ void ts_state_init(const long long* __restrict__ ids, int ids_stride, const int* __restrict__ n_ids,
                              int n_fixed, int sample_begin, int V, int beg, TsState* __restrict__ state, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const int n = min(n_ids ? n_ids[b] : n_fixed, ids_stride);
  TsState st{-1, 0, 0};
  for (int i = sample_begin; i < n; ++i) {
    const long long id = ids[(long)b * ids_stride + i];
    const bool ts = id >= beg && id < V;
    st.prev_is_ts = st.last_is_ts;
    st.last_is_ts = ts;
    if (ts) st.tick = (int)(id - beg);
  }
  state[b] = st;
}

}  // namespace

int ts_chunks(int n_vocab) { return (n_vocab + kTsChunk - 1) / kTsChunk; }

void launch_ts_state_init(const long long* ids, int ids_stride, const int* n_ids, int n_fixed, int sample_begin, int V,
                          int beg, TsState* state, int batch, hipStream_t s) {
  if (batch < 1 || ids_stride < 1 || sample_begin < 0) throw Error(kErrInvalidArg, "ts_state_init: bad arguments");
  hipLaunchKernelGGL(ts_state_init, dim3((batch + 63) / 64), dim3(64), 0, s, ids, ids_stride, n_ids, n_fixed, sample_begin,
                     V, beg, state, batch);
}

void launch_ts_select(const TsSelectArgs& a, hipStream_t s) {
  const int n_chunks = ts_chunks(a.V);
  if (a.batch < 1 || a.V < 2 || n_chunks > kTsMaxChunks || a.eot < 0 || a.eot >= a.beg || a.beg >= a.V || a.ldl < a.V ||
      a.ldl % 4 != 0 || (reinterpret_cast<uintptr_t>(a.logits) & 15) != 0 || a.pos < 0 || a.pos + 1 >= a.ids_stride ||
      a.n_gen < 0 || a.max_initial < -1) {
    throw Error(kErrInvalidArg, "ts_select: needs 0 <= eot < beg < V <= 4096 * 64, 16-byte aligned logits rows and pos + 1 < ids_stride");
  }
  hipLaunchKernelGGL(ts_partial, dim3(n_chunks, a.batch), dim3(kThreads), 0, s, a.logits, a.ldl, a.V, a.state, a.n_gen,
                     a.eot, a.beg, a.max_initial, a.part);
  hipLaunchKernelGGL(ts_select, dim3(a.batch), dim3(64), 0, s, a.part, n_chunks, a.ids, a.ids_stride, a.pos, a.n_ids,
                     a.finished, a.state, a.beg, (long long)a.eot, a.stop_at_eot, a.dbg_L, a.dbg_M);
}

}  // namespace wt
