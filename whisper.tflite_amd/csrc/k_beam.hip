// Beam-search decoding (option beam_size 2..8): the per-step kernels that sit between the logits
// GEMM and the next decoder pass.  A step of K beams over `clips` clips:
//   beam_topk_partial   per (row, 4096-entry vocabulary chunk): max, sum of exp against it, top K+1 (logit, id)
//   beam_select         per clip: merges the chunks of its live rows in chunk order (logsumexp, top K+1 log-probs),
//                       orders the candidates, walks them (EOT -> finished list, others -> next live rows)
//   beam_reorder        per new row: its parent's self-attention K / V rows and id history, into the other buffer
//   beam_finalize       per clip: fills an unfinished list from the live rows, ranks by sum / length, writes ids
// Every result is a function of the row's logits alone: the chunking of the vocabulary is fixed (kBeamChunk), a
// chunk's thread and wavefront reductions have a fixed shape, and the chunks are merged in index order by one lane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.h"

namespace wt {
namespace {

constexpr int kTopThreads = 256, kTopPer = kBeamChunk / kTopThreads;  // 16 entries per thread
constexpr int kKK = kBeamMax + 1;                                     // candidates per hypothesis, at most

// float -> unsigned with the same order (larger float, larger key); the low 32 bits of a key hold the id, so the
// maximum key is the larger logit and, on equal logits, the larger id: the reference argmax's last-index rule.  -0 and
// +0 are one logit, so they share the key of +0 (every other value keeps its bits)
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

// grid (chunks, rows), 256 threads: thread t holds entries chunk * 4096 + j * 256 + t, j = 0..15
__global__ __launch_bounds__(kTopThreads) void beam_topk_partial(const float* __restrict__ logits, int ldl, int V, int kk,
                                                                 BeamPart* __restrict__ part) {
  __shared__ float red[4];
  __shared__ unsigned long long kred[2][4];
  const int chunk = blockIdx.x, row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* z = logits + (long)row * ldl;
  const int base = chunk * kBeamChunk + tid;
  float v[kTopPer];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < kTopPer; ++j) {
    const int i = base + j * kTopThreads;
    v[j] = i < V ? z[i] : -INFINITY;
    m = fmaxf(m, v[j]);
  }
  m = wave_max_f(m);
  if (lane == 0) red[wid] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));  // a maximum: exact in any order
  __syncthreads();
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < kTopPer; ++j) s += (base + j * kTopThreads < V) ? expf(v[j] - m) : 0.0f;
  s = wave_sum_f(s);
  if (lane == 0) red[wid] = s;
  __syncthreads();
  BeamPart* const out = part + ((long)row * gridDim.x + chunk);
  if (tid == 0) {
    out->m = m;
    out->s = m == -INFINITY ? 0.0f : ((red[0] + red[1]) + red[2]) + red[3];  // (a masked chunk: exp(-inf - -inf) is NaN)
  }
  // top kk keys: round r takes the largest key below the previous round's winner (keys are distinct: the id is in them)
  unsigned long long prev = ~0ull;
  for (int r = 0; r < kk; ++r) {
    unsigned long long best = 0ull;
#pragma unroll
    for (int j = 0; j < kTopPer; ++j) {
      const int i = base + j * kTopThreads;
      const unsigned long long key = i < V ? ((unsigned long long)ord_of(v[j]) << 32) | (unsigned)i : 0ull;
      if (key < prev && key > best) best = key;
    }
    best = wave_max_u64(best);
    if (lane == 0) kred[r & 1][wid] = best;
    __syncthreads();
    unsigned long long w = kred[r & 1][0];
    for (int q = 1; q < 4; ++q) w = kred[r & 1][q] > w ? kred[r & 1][q] : w;
    if (tid == 0) out->key[r] = w;  // 0: the chunk holds fewer than kk entries
    prev = w;
  }
}

struct Cand {
  float score;
  int s, r, tok, valid;
};

__device__ __forceinline__ bool cand_before(const Cand& a, const Cand& b) {
  if (a.valid != b.valid) return a.valid > b.valid;
  if (a.score != b.score) return a.score > b.score;
  if (a.s != b.s) return a.s < b.s;
  return a.r < b.r;
}

// one block (8 wavefronts) per clip of the chain
__global__ __launch_bounds__(512) void beam_select(BeamStepArgs a) {
  __shared__ Cand cand[kBeamMax * kKK];
  __shared__ int order[kBeamMax * kKK];
  __shared__ int app_cand[kBeamMax], app_at[kBeamMax], live_cand[kBeamMax];
  __shared__ int n_app_s, n_live_s;
  const int c = blockIdx.x, g = a.c0 + c, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int K = a.K, kk = K + 1, rows_next = K * a.clips;
  const int t = a.pos + 1 - a.n_prompt;  // tokens each live hypothesis has generated before this step
  if (a.done[g]) {
    // a finished clip: its rows keep computing behind themselves, nothing else changes
    if (tid < K) {
      const int row = tid * a.clips + c;
      a.parent[row] = row;
      a.token[row] = a.eot;
    }
    return;
  }
  // merge of the chunk records of live row `wid` (one wavefront per hypothesis)
  if (wid < a.n_live) {
    const int row = wid * a.clips + c;
    const BeamPart* p = a.part + (long)row * a.n_chunks;
    float lse = 0.0f;
    if (lane == 0) {
      float M = -INFINITY;
      for (int q = 0; q < a.n_chunks; ++q) M = fmaxf(M, p[q].m);
      float S = 0.0f;
      for (int q = 0; q < a.n_chunks; ++q) S += p[q].s * expf(p[q].m - M);
      lse = M + logf(S);
    }
    lse = __shfl(lse, 0, 64);
    const float sum = t == 0 ? 0.0f : a.live_sum[g * kBeamMax + wid];  // the prompt: one hypothesis, sum 0
    const int n_rec = a.n_chunks * kk;  // <= 16 chunks x 9 keys: three per lane
    unsigned long long prev = ~0ull;
    for (int r = 0; r < kk; ++r) {
      unsigned long long best = 0ull;
      for (int i = lane; i < n_rec; i += 64) {
        const unsigned long long key = p[i / kk].key[i % kk];
        if (key < prev && key > best) best = key;
      }
      best = wave_max_u64(best);
      prev = best;
      if (lane == 0) {
        Cand& x = cand[wid * kk + r];
        const int tok = (int)(unsigned)(best & 0xffffffffull);
        const float lp = float_of((unsigned)(best >> 32)) - lse;
        x.valid = best != 0ull && tok >= 0 && tok < a.V && lp == lp;
        x.score = x.valid ? sum + lp : -INFINITY;
        x.s = wid, x.r = r, x.tok = x.valid ? tok : 0;
      }
    }
  }
  __syncthreads();
  const int n_c = a.n_live * kk;
  if (tid < n_c) order[tid] = -1;
  __syncthreads();
  if (tid < n_c) {
    int rank = 0;
    for (int j = 0; j < n_c; ++j) rank += cand_before(cand[j], cand[tid]) ? 1 : 0;
    if (rank < n_c) order[rank] = tid;  // (s, r) are distinct: the ranks are a permutation
  }
  __syncthreads();
  if (tid == 0) {
    int nf = a.n_fin[g], na = 0, nl = 0;
    for (int q = 0; q < n_c && nl < K; ++q) {
      const int i = order[q];
      if (i < 0 || i >= n_c || !cand[i].valid) continue;
      if (cand[i].tok == a.eot) {
        if (nf < K) {
          app_cand[na] = i, app_at[na] = nf;
          ++na, ++nf;
        }
      } else {
        live_cand[nl++] = i;
      }
    }
    for (int k = nl; k < K; ++k) live_cand[k] = nl > 0 ? live_cand[0] : 0;  // (cannot happen: >= K non-EOT candidates)
    n_app_s = na;
    n_live_s = nl;
    a.n_fin[g] = nf;
    a.done[g] = nf >= K ? 1 : 0;
  }
  __syncthreads();
  // finished entries: the hypothesis's generated ids, then EOT
  if (wid < n_app_s) {
    const Cand& x = cand[app_cand[wid]];
    const int at = app_at[wid], src = x.s * a.clips + c;
    int* ft = a.fin_tok + ((long)g * kBeamMax + at) * 32;
    if (lane < t && a.n_prompt + lane < 32) ft[lane] = (int)a.ids[(long)src * 32 + a.n_prompt + lane];
    if (lane == t && t < 32) ft[lane] = (int)a.eot;
    if (lane == 0) {
      a.fin_sum[g * kBeamMax + at] = x.score;
      a.fin_len[g * kBeamMax + at] = t + 1;
    }
  }
  if (tid < K) {
    const Cand& x = cand[live_cand[tid]];
    const int row = tid * a.clips + c;
    if (row < rows_next) {
      a.parent[row] = x.s * a.clips + c;
      a.token[row] = n_live_s > 0 ? x.tok : a.eot;
      a.live_sum[g * kBeamMax + tid] = x.score;
    }
  }
}

// grid (rows, layers * 2 + 1): y < layers * 2 copies one (layer, k|v) cache row of positions 0..pos from the parent
// row; y = layers * 2 writes the id row (parent's history + the selected token at pos + 1)
__global__ __launch_bounds__(256) void beam_reorder(BeamReorderArgs a) {
  const int r = blockIdx.x, y = blockIdx.y;
  int p = a.parent[r];
  p = p < 0 ? 0 : (p >= a.src_rows ? a.src_rows - 1 : p);
  if (y < a.slabs) {
    const long row_elems = (long)a.cap * a.d;
    const float4* src = reinterpret_cast<const float4*>(a.kv_src + (long)y * a.src_rows * row_elems + (long)p * row_elems);
    float4* dst = reinterpret_cast<float4*>(a.kv_dst + (long)y * a.dst_rows * row_elems + (long)r * row_elems);
    const int n4 = (a.pos + 1) * a.d / 4;
    for (int i = threadIdx.x; i < n4; i += 256) dst[i] = src[i];
    return;
  }
  const int i = threadIdx.x;
  if (i < 32) {
    long long v = 0;
    if (i <= a.pos) v = a.ids_src[(long)p * 32 + i];
    if (i == a.pos + 1) {
      v = a.token[r];
      v = v < 0 || v >= a.V ? 0 : v;  // an id the embedding reads: inside the vocabulary whatever happened
    }
    a.ids_dst[(long)r * 32 + i] = v;
  }
}

// one block per clip of the chain (64 threads)
__global__ __launch_bounds__(64) void beam_finalize(BeamFinalArgs a) {
  __shared__ int best_s;
  const int c = blockIdx.x, g = a.c0 + c, lane = threadIdx.x, K = a.K;
  const int t = a.pos + 1 - a.n_prompt;  // the last step's index: live rows hold t + 1 generated ids
  if (lane == 0) {
    int nf = a.n_fin[g];
    if (!a.done[g]) {
      for (int k = 0; nf < K && k < K; ++k, ++nf) {
        const long row = (long)k * a.clips + c;
        int* ft = a.fin_tok + ((long)g * kBeamMax + nf) * 32;
        for (int j = 0; j <= t && a.n_prompt + j < 32; ++j) ft[j] = (int)a.ids[row * 32 + a.n_prompt + j];
        a.fin_sum[g * kBeamMax + nf] = a.live_sum[g * kBeamMax + k];
        a.fin_len[g * kBeamMax + nf] = t + 1;
      }
      a.n_fin[g] = nf;
    }
    int b = 0;
    float bv = -INFINITY;
    for (int i = 0; i < nf && i < K; ++i) {
      const int len = a.fin_len[g * kBeamMax + i];
      const float v = a.fin_sum[g * kBeamMax + i] / (float)(len > 0 ? len : 1);
      if (i == 0 || v > bv) b = i, bv = v;  // strictly better: the earlier entry wins a tie
    }
    best_s = b;
    a.out_sum[g] = a.fin_sum[g * kBeamMax + b];
    a.out_len[g] = a.fin_len[g * kBeamMax + b];
    int n = a.n_prompt + a.fin_len[g * kBeamMax + b];
    a.out_n[g] = n < 32 ? n : 32;
  }
  __syncthreads();
  const int b = best_s, len = a.fin_len[g * kBeamMax + b];
  if (lane < 32) {
    long long v = 0;
    if (lane < a.n_prompt) v = a.ids[(long)c * 32 + lane];  // every row starts with the prompt
    else if (lane - a.n_prompt < len) v = a.fin_tok[((long)g * kBeamMax + b) * 32 + lane - a.n_prompt];
    a.out_ids[(long)g * 32 + lane] = v;
  }
}

}  // namespace

int beam_chunks(int n_vocab) { return (n_vocab + kBeamChunk - 1) / kBeamChunk; }

void launch_beam_topk(const float* logits, int ldl, int V, int rows, int kk, BeamPart* part, hipStream_t s) {
  if (!logits || !part || V < 1 || beam_chunks(V) > kBeamMaxChunks || rows < 1 || rows > 128 || kk < 2 || kk > kBeamMax + 1 ||
      ldl < V) {
    throw Error(kErrInvalidArg, "beam_topk: bad shape");
  }
  hipLaunchKernelGGL(beam_topk_partial, dim3(beam_chunks(V), rows), dim3(kTopThreads), 0, s, logits, ldl, V, kk, part);
}

void launch_beam_select(const BeamStepArgs& a, hipStream_t s) {
  if (a.K < 2 || a.K > kBeamMax || a.clips < 1 || a.K * a.clips > 128 || (a.n_live != 1 && a.n_live != a.K) || a.c0 < 0 ||
      a.c0 + a.clips > kBeamClipsMax || a.n_chunks != beam_chunks(a.V) || a.n_prompt < 1 || a.pos + 1 < a.n_prompt ||
      a.pos + 1 > 31) {
    throw Error(kErrInvalidArg, "beam_select: bad shape");
  }
  hipLaunchKernelGGL(beam_select, dim3(a.clips), dim3(512), 0, s, a);
}

void launch_beam_reorder(const BeamReorderArgs& a, hipStream_t s) {
  if (a.dst_rows < 1 || a.dst_rows > 128 || a.src_rows < 1 || a.src_rows > 128 || a.pos < 0 || a.pos + 1 >= 32 ||
      a.pos + 1 > a.cap || a.d % 4 != 0 || a.slabs < 0 || (a.slabs > 0 && (!a.kv_src || !a.kv_dst))) {
    throw Error(kErrInvalidArg, "beam_reorder: bad shape");
  }
  hipLaunchKernelGGL(beam_reorder, dim3(a.dst_rows, a.slabs + 1), dim3(256), 0, s, a);
}

void launch_beam_finalize(const BeamFinalArgs& a, hipStream_t s) {
  if (a.K < 2 || a.K > kBeamMax || a.clips < 1 || a.K * a.clips > 128 || a.c0 < 0 || a.c0 + a.clips > kBeamClipsMax ||
      a.n_prompt < 1 || a.pos + 1 < a.n_prompt || a.pos + 1 > 31) {
    throw Error(kErrInvalidArg, "beam_finalize: bad shape");
  }
  hipLaunchKernelGGL(beam_finalize, dim3(a.clips), dim3(64), 0, s, a);
}

}  // namespace wt
