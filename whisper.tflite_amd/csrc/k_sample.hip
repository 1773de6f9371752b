// Temperature sampling (option temperature): a sample from softmax(z[A] / T) over the set A a step may
// choose from, drawn as the Gumbel maximum: token = argmax over i in A of k_i = z_i / T + g_i, g_i = -log(-log u_i), u_i
// from Philox4x32-10 under the counter (i >> 2, pos, clip, attempt) and the key (seed low, seed high).  T = 0: k_i = z_i,
// no random number, the greedy step of select_token / ts_select.
//   sample_partial  per (clip, 4096-entry vocabulary chunk): best perturbed key over the allowed text ids, best over the
//                   allowed timestamps, and the unperturbed record ts_partial forms (rule 5 is decided on the logits)
//   sample_select   per clip: merges its records in chunk order, decides rule 5 as ts_select does, takes the larger
//                   perturbed key of what is left, writes the token, n_ids, finished and the clip's state
// A is the whole vocabulary (state == nullptr) or what the timestamp rules leave (ts_rules.h).  Everything that varies
// from attempt to attempt (1 / T per clip, seed, attempt, the first clip's index) is read from a SampleParams block in
// device memory, so one captured launch sequence serves them all.
// Several samples per clip (SampleArgs::group = N > 1): the launch's rows are N samples of
// ceil(rows / N) clips, row r = sample j = r / clips of clip r % clips (the rows of a beam chain, which the absorbed
// cross-attention groups per clip).  The parameter block is indexed by the clip; the counter's fourth word is
// attempt + (j << 16), so sample 0 is the ungrouped draw.  sample_partial<true, int> is that form, sample_partial<false>
// the launch of group = 1.  sample_select reads nothing of the block and serves both.
#include <hip/hip_runtime.h>

#include <cmath>

#include "error.h"
#include "kernels.h"
#include "ts_rules.h"

namespace wt {
namespace {

constexpr int kThreads = 256;
constexpr int kQuads = kTsChunk / (4 * kThreads);  // 16-byte loads per thread

// float -> unsigned with the same order, -0 and +0 one value (as k_timestamps.hip); key = ord << 32 | id, 0 = none
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

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between them
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}
// u = ((x >> 9) + 0.5) 2^-23: exact in fp32, inside (0, 1); g = -log(-log u) in [-2.82, 16.64]
__device__ __forceinline__ float gumbel_of(unsigned x) {
  const float u = ((float)(x >> 9) + 0.5f) * 0x1p-23f;
  return -logf(-logf(u));
}

// grid (chunks, clips): thread t holds the 4 consecutive entries chunk * 4096 + j * 1024 + 4 t .. + 3, j = 0 .. 3 (the
// load shape of ts_partial, and its reductions for key_text, m and s: the same bits)
// (kGroup = true takes one more argument, the clips of the launch; without it the argument list, and with it every
// instruction, is the ungrouped kernel's)
template <bool kGroup, typename... Clips>
__global__ __launch_bounds__(kThreads) void sample_partial(const float* __restrict__ logits, int ldl, int V,
                                                           const TsState* __restrict__ state, int n_gen, int eot, int beg,
                                                           int mit, const SampleParams* __restrict__ prm, int row0,
                                                           int rng_pos, SamplePart* __restrict__ part, Clips... n_clips) {
  static_assert(sizeof...(Clips) == (kGroup ? 1 : 0), "the grouped kernel takes the number of clips");
  const int clips = (n_clips + ... + 0);
  __shared__ float red[4];
  __shared__ unsigned long long kred[4][4];
  const int chunk = blockIdx.x, row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  Allowed a;
  if (state) {
    a = allowed_of(state[row], n_gen, V, eot, beg, mit);
  } else {  // plain mode: every id is "text"
    a.t_lo = 0, a.t_hi = V - 1, a.s_lo = V, a.s_hi = V - 1;
  }
  // the row's entry of the parameter block, and its sample index on top of the attempt
  const int crow = kGroup ? row % clips : row;
  const float inv_t = prm->inv_t[row0 + crow];  // 0: greedy
  const unsigned k0 = prm->seed_lo, k1 = prm->seed_hi, attempt = prm->attempt + (kGroup ? (unsigned)(row / clips) << 16 : 0u);
  const unsigned clip = prm->clip_base + (unsigned)(row0 + crow) + (unsigned)prm->clip_off[row0 + crow];
  rng_pos -= prm->pos_off[row0 + crow];
  const float* z = logits + (long)row * ldl;  // ldl % 4 == 0 and a 16-byte base: every quad below is aligned
  float v[4 * kQuads];
  unsigned long long kt = 0ull, ks = 0ull, pt = 0ull, ps = 0ull;
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < kQuads; ++j) {
    const int i0 = chunk * kTsChunk + j * 4 * kThreads + 4 * tid;
    float4 q = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (i0 < V) q = *reinterpret_cast<const float4*>(z + i0);  // (i0 + 3 < ldl: the row's padding is readable)
    const float e[4] = {q.x, q.y, q.z, q.w};
    unsigned x[4] = {0u, 0u, 0u, 0u};
    if (inv_t != 0.0f) philox4x32_10((unsigned)(i0 >> 2), (unsigned)rng_pos, clip, attempt, k0, k1, x);  // (block-uniform)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + c;
      const unsigned long long key = ((unsigned long long)ord_of(e[c]) << 32) | (unsigned)i;
      const float k = inv_t != 0.0f ? fmaf(e[c], inv_t, gumbel_of(x[c])) : e[c];
      const unsigned long long pkey = ((unsigned long long)ord_of(k) << 32) | (unsigned)i;
      const bool is_t = i >= a.t_lo && i <= a.t_hi, is_s = i >= a.s_lo && i <= a.s_hi;  // (t_hi, s_hi < V)
      if (is_t && key > kt) kt = key;
      if (is_s && key > ks) ks = key;
      if (is_t && pkey > pt) pt = pkey;
      if (is_s && pkey > ps) ps = pkey;
      v[4 * j + c] = is_s ? e[c] : -INFINITY;
      m = fmaxf(m, v[4 * j + c]);
    }
  }
  m = wave_max_f(m);
  kt = wave_max_u64(kt);
  ks = wave_max_u64(ks);
  pt = wave_max_u64(pt);
  ps = wave_max_u64(ps);
  if (lane == 0) red[wid] = m, kred[0][wid] = kt, kred[1][wid] = ks, kred[2][wid] = pt, kred[3][wid] = ps;
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
    SamplePart* const out = part + ((long)row * gridDim.x + chunk);
    for (int w = 1; w < 4; ++w) {
      kt = kred[0][w] > kt ? kred[0][w] : kt;
      ks = kred[1][w] > ks ? kred[1][w] : ks;
      pt = kred[2][w] > pt ? kred[2][w] : pt;
      ps = kred[3][w] > ps ? kred[3][w] : ps;
    }
    out->pkey_text = pt;
    out->pkey_ts = ps;
    out->key_text = kt;
    out->key_ts = ks;
    out->m = m;
    out->s = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

// one wavefront per clip
__global__ __launch_bounds__(64) void sample_select(const SamplePart* __restrict__ part, int n_chunks, long long* ids,
                                                    int ids_stride, int pos, int* n_ids, int* finished,
                                                    TsState* __restrict__ state, int beg, long long eot, int stop_at_eot,
                                                    double* dbg_L, float* dbg_M, float* dbg_key) {
  __shared__ SamplePart sp[kTsMaxChunks];
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < n_chunks; c += 64) sp[c] = part[(long)b * n_chunks + c];
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned long long kt = 0ull, ks = 0ull, pt = 0ull, ps = 0ull;
  float m = -INFINITY;
  for (int c = 0; c < n_chunks; ++c) {
    kt = sp[c].key_text > kt ? sp[c].key_text : kt;
    ks = sp[c].key_ts > ks ? sp[c].key_ts : ks;
    pt = sp[c].pkey_text > pt ? sp[c].pkey_text : pt;
    ps = sp[c].pkey_ts > ps ? sp[c].pkey_ts : ps;
    m = fmaxf(m, sp[c].m);
  }
  // rule 5 on the untempered logits, as ts_select: L = m + log(sum_c s_c exp(m_c - m)) in double, chunks in index order
  double S = 0.0;
  for (int c = 0; c < n_chunks; ++c) {
    if (sp[c].m != -INFINITY) S += (double)sp[c].s * exp((double)sp[c].m - (double)m);
  }
  const double L = (ks != 0ull && m != -INFINITY) ? (double)m + log(S) : -INFINITY;
  const float M = kt != 0ull ? float_of((unsigned)(kt >> 32)) : -INFINITY;
  if (dbg_L) dbg_L[b] = ks != 0ull ? L : NAN;  // NaN: no such id is allowed
  if (dbg_M) dbg_M[b] = kt != 0ull ? M : NAN;
  if (kt != 0ull && ks != 0ull && L > (double)M) pt = 0ull;
  // the allowed set is never empty, so one of the keys exists
  const unsigned long long p = pt > ps ? pt : ps;
  if (dbg_key) dbg_key[b] = float_of((unsigned)(p >> 32));
  const long long tok = (long long)(unsigned)(p & 0xffffffffull);
  ids[(long)b * ids_stride + pos + 1] = tok;
  if (!finished[b]) {  // as select_token
    n_ids[b] = pos + 2;
    if (stop_at_eot && tok == eot) finished[b] = 1;
  }
  if (state) {
    TsState st = state[b];
    st.prev_is_ts = st.last_is_ts;
    st.last_is_ts = tok >= beg;
    if (tok >= beg) st.tick = (int)(tok - beg);
    state[b] = st;
  }
}

}  // namespace

void launch_sample_select(const SampleArgs& a, hipStream_t s) {
  const int n_chunks = ts_chunks(a.V);
  const bool ts = a.state != nullptr;
  if (a.batch < 1 || a.V < 2 || n_chunks > kTsMaxChunks || a.eot < 0 || a.eot >= a.V || (ts && (a.eot >= a.beg || a.beg >= a.V)) ||
      a.ldl < a.V || a.ldl % 4 != 0 || (reinterpret_cast<uintptr_t>(a.logits) & 15) != 0 || a.pos < 0 ||
      a.pos + 1 >= a.ids_stride || a.n_gen < 0 || a.max_initial < -1 || !a.params || a.row0 < 0 ||
      (a.group == 1 && a.row0 + a.batch > kSampleClipsMax)) {
    throw Error(kErrInvalidArg, "sample_select: needs 0 <= eot (< beg) < V <= 4096 * 64, 16-byte aligned logits rows, pos + 1 < ids_stride and at most 64 clips");
  }
  const int clips = a.group > 0 ? (a.batch + a.group - 1) / a.group : 0;
  if (a.group < 1 || a.group > kSampleGroupMax || (a.group > 1 && (a.batch > kSampleRowsMax || a.row0 + clips > kSampleClipsMax))) {
    throw Error(kErrInvalidArg, "sample_select: a group is 1 .. 8 samples per clip, at most 128 rows and 64 clips");
  }
  if (a.group > 1) {
    hipLaunchKernelGGL((sample_partial<true, int>), dim3(n_chunks, a.batch), dim3(kThreads), 0, s, a.logits, a.ldl, a.V, a.state,
                       a.n_gen, a.eot, a.beg, a.max_initial, a.params, a.row0, a.rng_pos >= 0 ? a.rng_pos : a.pos, a.part, clips);
  } else {
    hipLaunchKernelGGL(sample_partial<false>, dim3(n_chunks, a.batch), dim3(kThreads), 0, s, a.logits, a.ldl, a.V, a.state, a.n_gen,
                       a.eot, a.beg, a.max_initial, a.params, a.row0, a.rng_pos >= 0 ? a.rng_pos : a.pos, a.part);
  }
  hipLaunchKernelGGL(sample_select, dim3(a.batch), dim3(64), 0, s, a.part, n_chunks, a.ids, a.ids_stride, a.pos, a.n_ids,
                     a.finished, a.state, ts ? a.beg : a.V, (long long)a.eot, a.stop_at_eot, a.dbg_L, a.dbg_M, a.dbg_key);
}

}  // namespace wt
