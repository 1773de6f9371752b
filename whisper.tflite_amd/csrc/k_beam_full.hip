// Full-length beam search (option full_beam): the per-step kernels between the logits GEMM and the
// next decoder pass of a beam chain that runs to max_positions behind the timestamp rules.
//   beam_full_begin     per clip: nothing finished, one live hypothesis with sum 0 and no timestamp yet, the prompt's
//                       ancestor entries (its K / V sit in the clip's slot-0 row)
//   beam_full_partial   per (row, 4096-entry vocabulary chunk) and class — allowed text ids, allowed timestamps —:
//                       max, sum of exp against it, top K+1 keys
//   beam_full_select    per clip: merges the chunks of its live rows in chunk order in float64, decides rule 5, forms
//                       logsumexp_A and the top K+1 keys of A, orders and walks the candidates as beam_select does
//   beam_full_advance   per new row: the parent's id, log-probability and ancestor rows into the other half of the
//                       double buffer, the token appended, anc[r][pos] = parent.  No K / V moves.
//   beam_full_finalize  per clip: fills an unfinished list from the live rows, ranks by sum / length, writes ids and lps
// Every result is a function of the row's logits and state alone: the chunking of the vocabulary is fixed (kBeamChunk), a
// chunk's reductions have a fixed shape (a masked entry adds an exact 0), and the chunks are merged in index order by one
// lane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "error.h"
#include "kernels.h"
#include "ts_rules.h"

namespace wt {
namespace {

constexpr int kThreads = 256, kPer = kBeamChunk / kThreads;  // 16 entries per thread
constexpr int kKK = kBeamMax + 1;                            // candidates per hypothesis, at most

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

__device__ __forceinline__ int step_of(const BeamFullArgs& a) { return a.pos + 1 - a.n_prompt; }
__device__ __forceinline__ int live_rows_of(const BeamFullArgs& a) { return step_of(a) == 0 ? a.clips : a.K * a.clips; }

// one block per clip (64 threads)
__global__ __launch_bounds__(64) void beam_full_begin(BeamFullArgs a) {
  const int c = blockIdx.x, g = a.c0 + c;
  if (threadIdx.x == 0) {
    a.n_fin[g] = 0;
    a.done[g] = 0;
    a.n_live[g] = 1;
    for (int k = 0; k < kBeamMax; ++k) a.live_sum[g * kBeamMax + k] = k == 0 ? 0.0 : -INFINITY;
    a.ts[c] = TsState{-1, 0, 0};
  }
  for (int i = threadIdx.x; i < a.n_prompt && i < a.cap; i += 64) a.anc_dst[(long)c * a.cap + i] = (unsigned char)c;
}

// grid (chunks, live rows), 256 threads: thread t holds entries chunk * 4096 + j * 256 + t, j = 0..15
__global__ __launch_bounds__(kThreads) void beam_full_partial(BeamFullArgs a) {
  __shared__ float red[2][4];
  __shared__ unsigned long long kred[2][2][4];
  const int chunk = blockIdx.x, row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kk = a.K + 1;
  Allowed al;
  if (a.timestamps) {
    al = allowed_of(a.ts[row], step_of(a), a.V, a.eot, a.beg, a.max_initial);
  } else {
    al.t_lo = 0, al.t_hi = a.V - 1, al.s_lo = 1, al.s_hi = 0;
  }
  const float* z = a.logits + (long)row * a.ldl;
  const int base = chunk * kBeamChunk + tid;
  float v[kPer];
  unsigned cls = 0u;  // two bits per entry: 1 = an allowed text id, 2 = an allowed timestamp
  float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = base + j * kThreads;
    v[j] = i < a.V ? z[i] : -INFINITY;
    const bool in = v[j] > -INFINITY;  // a logit of -inf (or NaN) is a masked id
    const bool is_t = in && i >= al.t_lo && i <= al.t_hi, is_s = in && i >= al.s_lo && i <= al.s_hi;
    cls |= ((is_t ? 1u : 0u) | (is_s ? 2u : 0u)) << (2 * j);
    if (is_t) mt = fmaxf(mt, v[j]);
    if (is_s) ms = fmaxf(ms, v[j]);
  }
  mt = wave_max_f(mt);
  ms = wave_max_f(ms);
  if (lane == 0) red[0][wid] = mt, red[1][wid] = ms;
  __syncthreads();
  mt = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));  // a maximum: exact in any order
  ms = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  __syncthreads();
  float st = 0.0f, ss = 0.0f;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    st += ((cls >> (2 * j)) & 1u) ? expf(v[j] - mt) : 0.0f;
    ss += ((cls >> (2 * j)) & 2u) ? expf(v[j] - ms) : 0.0f;
  }
  st = wave_sum_f(st);
  ss = wave_sum_f(ss);
  if (lane == 0) red[0][wid] = st, red[1][wid] = ss;
  __syncthreads();
  BeamFullPart* const out = a.part + ((long)row * gridDim.x + chunk);
  if (tid == 0) {
    out->mt = mt;
    out->st = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    out->ms = ms;
    out->ss = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
  // top kk keys of either class: round r takes the largest key below the previous round's winner (keys are distinct)
  unsigned long long prev_t = ~0ull, prev_s = ~0ull;
  for (int r = 0; r < kk; ++r) {
    unsigned long long bt = 0ull, bs = 0ull;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const unsigned long long key = ((unsigned long long)ord_of(v[j]) << 32) | (unsigned)(base + j * kThreads);
      const unsigned c2 = cls >> (2 * j);
      if ((c2 & 1u) && key < prev_t && key > bt) bt = key;
      if ((c2 & 2u) && key < prev_s && key > bs) bs = key;
    }
    bt = wave_max_u64(bt);
    bs = wave_max_u64(bs);
    if (lane == 0) kred[r & 1][0][wid] = bt, kred[r & 1][1][wid] = bs;
    __syncthreads();
    unsigned long long wt_ = kred[r & 1][0][0], ws_ = kred[r & 1][1][0];
    for (int q = 1; q < 4; ++q) {
      wt_ = kred[r & 1][0][q] > wt_ ? kred[r & 1][0][q] : wt_;
      ws_ = kred[r & 1][1][q] > ws_ ? kred[r & 1][1][q] : ws_;
    }
    if (tid == 0) out->kt[r] = wt_, out->ks[r] = ws_;  // 0: the chunk holds fewer than kk such entries
    prev_t = wt_;  // (0: nothing is below it, the later rounds find nothing either)
    prev_s = ws_;
  }
}

struct Cand {
  double score;
  float lp;
  int s, r, tok, valid;
};

__device__ __forceinline__ bool cand_before(const Cand& a, const Cand& b) {
  if (a.valid != b.valid) return a.valid > b.valid;
  if (a.score != b.score) return a.score > b.score;
  if (a.s != b.s) return a.s < b.s;
  return a.r < b.r;
}

// one block (8 wavefronts) per clip of the chain
__global__ __launch_bounds__(512) void beam_full_select(BeamFullArgs a) {
  __shared__ Cand cand[kBeamMax * kKK];
  __shared__ int order[kBeamMax * kKK];
  __shared__ int app_cand[kBeamMax], app_at[kBeamMax], live_cand[kBeamMax];
  __shared__ TsState pst[kBeamMax];
  __shared__ int n_app_s, n_live_s;
  const int c = blockIdx.x, g = a.c0 + c, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int K = a.K, kk = K + 1, n_chunks = (a.V + kBeamChunk - 1) / kBeamChunk;
  const int t = step_of(a);  // ids each live hypothesis has generated before this step
  if (a.done[g]) {
    // a finished clip: its rows keep computing behind themselves, nothing else changes
    if (tid < K) {
      const int row = tid * a.clips + c;
      a.parent[row] = row;
      a.token[row] = a.eot;
      a.tok_lp[row] = 0.0f;
    }
    return;
  }
  const int n_in = t == 0 ? 1 : min(max(a.n_live[g], 0), K);  // (the count is data: bounded)
  if (wid < n_in) {  // one wavefront per live hypothesis: the merge of its chunk records
    const int row = wid * a.clips + c;
    const BeamFullPart* p = a.part + (long)row * n_chunks;
    double lse = 0.0;
    int use_t = 0, use_s = 0;
    if (lane == 0) {
      if (a.timestamps) pst[wid] = a.ts[row];
      float Mt = -INFINITY, Ms = -INFINITY;
      unsigned long long bt = 0ull, bs = 0ull;
      for (int q = 0; q < n_chunks; ++q) {
        Mt = fmaxf(Mt, p[q].mt);
        Ms = fmaxf(Ms, p[q].ms);
        bt = p[q].kt[0] > bt ? p[q].kt[0] : bt;
        bs = p[q].ks[0] > bs ? p[q].ks[0] : bs;
      }
      double St = 0.0, Ss = 0.0;
      for (int q = 0; q < n_chunks; ++q) {
        if (p[q].mt != -INFINITY) St += (double)p[q].st * exp((double)p[q].mt - (double)Mt);
        if (p[q].ms != -INFINITY) Ss += (double)p[q].ss * exp((double)p[q].ms - (double)Ms);
      }
      use_t = bt != 0ull, use_s = bs != 0ull;
      const double Lt = use_t ? (double)Mt + log(St) : -INFINITY, Ls = use_s ? (double)Ms + log(Ss) : -INFINITY;
      // rule 5: the summed probability of the timestamps against the best text logit
      if (a.timestamps && use_t && use_s && Ls > (double)float_of((unsigned)(bt >> 32))) use_t = 0;
      if (use_t && use_s) {
        const double mx = fmax((double)Mt, (double)Ms);
        lse = mx + log(St * exp((double)Mt - mx) + Ss * exp((double)Ms - mx));
      } else {
        lse = use_t ? Lt : Ls;
      }
      if (a.dbg_lse) a.dbg_lse[row] = (use_t || use_s) ? lse : NAN;
    }
    lse = __shfl(lse, 0, 64);
    use_t = __shfl(use_t, 0, 64);
    use_s = __shfl(use_s, 0, 64);
    const double sum = t == 0 ? 0.0 : a.live_sum[g * kBeamMax + wid];  // the prompt: one hypothesis, sum 0
    const int n_rec = n_chunks * kk;  // per class, <= 16 chunks x 9 keys
    unsigned long long prev = ~0ull;
    for (int r = 0; r < kk; ++r) {
      unsigned long long best = 0ull;
      for (int i = lane; i < 2 * n_rec; i += 64) {
        const int cl = i >= n_rec, j = cl ? i - n_rec : i;
        if (cl ? !use_s : !use_t) continue;
        const unsigned long long key = cl ? p[j / kk].ks[j % kk] : p[j / kk].kt[j % kk];
        if (key < prev && key > best) best = key;
      }
      best = wave_max_u64(best);
      prev = best;  // (0: nothing is below it, the later rounds find nothing either)
      if (lane == 0) {
        Cand& x = cand[wid * kk + r];
        const int tok = (int)(unsigned)(best & 0xffffffffull);
        const double lp = (double)float_of((unsigned)(best >> 32)) - lse;
        x.valid = best != 0ull && tok >= 0 && tok < a.V && lp == lp;
        x.score = x.valid ? sum + lp : -INFINITY;
        x.lp = x.valid ? (float)lp : 0.0f;
        x.s = wid, x.r = r, x.tok = x.valid ? tok : 0;
      }
    }
  }
  __syncthreads();
  const int n_c = n_in * kk;
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
    n_app_s = na;
    n_live_s = nl;
    a.n_fin[g] = nf;
    a.n_live[g] = nl;
    a.done[g] = (nf >= K || nl == 0) ? 1 : 0;
  }
  __syncthreads();
  // finished entries: the hypothesis's generated ids and their log-probabilities, then EOT and its own
  for (int e = 0; e < n_app_s; ++e) {
    const Cand& x = cand[app_cand[e]];
    const long at = ((long)g * kBeamMax + app_at[e]), src = (long)(x.s * a.clips + c) * a.stride + a.n_prompt;
    for (int i = tid; i <= t && i < a.stride; i += 512) {
      a.fin_tok[at * a.stride + i] = i < t ? (int)a.ids_src[src + i] : a.eot;
      a.fin_lp[at * a.stride + i] = i < t ? a.lp_src[src + i] : x.lp;
    }
    if (tid == 0) {
      a.fin_sum[at] = x.score;
      a.fin_len[at] = t + 1;
    }
  }
  if (tid < K) {
    // the rows of the missing slots keep computing behind the clip's slot 0: sum -inf, nothing offered
    const int nl = n_live_s, row = tid * a.clips + c;
    if (nl == 0) {
      a.parent[row] = c;
      a.token[row] = a.eot;
      a.tok_lp[row] = 0.0f;
      a.live_sum[g * kBeamMax + tid] = -INFINITY;
    } else {
      const Cand& x = cand[live_cand[tid < nl ? tid : 0]];
      a.parent[row] = x.s * a.clips + c;
      a.token[row] = x.tok;
      a.tok_lp[row] = x.lp;
      a.live_sum[g * kBeamMax + tid] = tid < nl ? x.score : -INFINITY;
      if (a.timestamps) {  // the child's state: the parent's, advanced by the token
        TsState s2 = pst[x.s];
        s2.prev_is_ts = s2.last_is_ts;
        s2.last_is_ts = x.tok >= a.beg;
        if (x.tok >= a.beg) s2.tick = x.tok - a.beg;
        a.ts[row] = s2;
      }
    }
  }
}

// one block per new row
__global__ __launch_bounds__(256) void beam_full_advance(BeamFullArgs a) {
  const int r = blockIdx.x, src_rows = live_rows_of(a);
  int p = a.parent[r];
  p = p < 0 ? 0 : (p >= src_rows ? src_rows - 1 : p);  // parents and tokens are data: clamped
  const long so = (long)p * a.stride, dst = (long)r * a.stride;
  for (int i = threadIdx.x; i <= a.pos; i += 256) {
    a.ids_dst[dst + i] = a.ids_src[so + i];
    a.lp_dst[dst + i] = a.lp_src[so + i];
  }
  for (int i = threadIdx.x; i < a.pos; i += 256) a.anc_dst[(long)r * a.cap + i] = a.anc_src[(long)p * a.cap + i];
  if (threadIdx.x == 0) {
    long long v = a.token[r];
    v = v < 0 || v >= a.V ? 0 : v;  // an id the embedding reads: inside the vocabulary whatever happened
    a.ids_dst[dst + a.pos + 1] = v;
    a.lp_dst[dst + a.pos + 1] = a.tok_lp[r];
    a.anc_dst[(long)r * a.cap + a.pos] = (unsigned char)p;  // position pos was written by the parent's row
  }
}

// one block per clip of the chain
__global__ __launch_bounds__(256) void beam_full_finalize(BeamFullArgs a) {
  __shared__ int nf0_s, n_add_s, best_s, len_s;
  const int c = blockIdx.x, g = a.c0 + c, tid = threadIdx.x, K = a.K;
  const int t = step_of(a);  // the last step's index: live rows hold t + 1 generated ids
  if (tid == 0) {
    const int nf = min(max(a.n_fin[g], 0), K);
    nf0_s = nf;
    n_add_s = a.done[g] ? 0 : min(min(max(a.n_live[g], 0), K), K - nf);
  }
  __syncthreads();
  const int nf0 = nf0_s, n_add = n_add_s;
  for (int e = 0; e < n_add; ++e) {  // the live hypotheses fill the list in slot order
    const long at = (long)g * kBeamMax + nf0 + e, src = (long)(e * a.clips + c) * a.stride + a.n_prompt;
    for (int j = tid; j <= t && a.n_prompt + j < a.stride; j += 256) {
      a.fin_tok[at * a.stride + j] = (int)a.ids_src[src + j];
      a.fin_lp[at * a.stride + j] = a.lp_src[src + j];
    }
    if (tid == 0) {
      a.fin_sum[at] = a.live_sum[g * kBeamMax + e];
      a.fin_len[at] = t + 1;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int nf = nf0 + n_add;
    a.n_fin[g] = nf;
    int b = 0;
    double bv = -INFINITY;
    for (int i = 0; i < nf; ++i) {
      const int len = a.fin_len[g * kBeamMax + i];
      const double v = a.fin_sum[g * kBeamMax + i] / (double)(len > 0 ? len : 1);
      if (i == 0 || v > bv) b = i, bv = v;  // strictly better: the earlier entry wins a tie
    }
    best_s = b;
    const int len = nf > 0 ? min(max(a.fin_len[g * kBeamMax + b], 0), a.stride - a.n_prompt) : 0;
    len_s = len;
    a.out_sum[g] = nf > 0 ? a.fin_sum[g * kBeamMax + b] : 0.0;
    a.out_len[g] = len;
    a.out_n[g] = a.n_prompt + len;
  }
  __syncthreads();
  const int b = best_s, len = len_s;
  for (int i = tid; i < a.stride; i += 256) {
    long long v = 0;
    float lp = 0.0f;
    if (i < a.n_prompt) {
      v = a.ids_src[(long)c * a.stride + i];  // every row starts with the prompt
    } else if (i - a.n_prompt < len) {
      v = a.fin_tok[((long)g * kBeamMax + b) * a.stride + i - a.n_prompt];
      lp = a.fin_lp[((long)g * kBeamMax + b) * a.stride + i - a.n_prompt];
    }
    a.out_ids[(long)g * a.stride + i] = v;
    a.out_lp[(long)g * a.stride + i] = lp;
  }
}

void check_shape(const BeamFullArgs& a, const char* what) {
  const bool ok = a.K >= 2 && a.K <= kBeamMax && a.clips >= 1 && a.K * a.clips <= 128 && a.c0 >= 0 &&
                  a.c0 + a.clips <= kBeamClipsMax && a.n_prompt >= 1 && a.pos + 1 >= a.n_prompt && a.pos >= 0 &&
                  a.pos < a.cap && a.cap <= kSelfLongCap && a.cap < a.stride && a.V >= 1 && a.ldl >= a.V &&
                  beam_chunks(a.V) <= kBeamMaxChunks && (!a.timestamps || (a.eot >= 0 && a.eot < a.beg && a.beg < a.V));
  if (!ok) throw Error(kErrInvalidArg, std::string(what) + ": bad shape");
}

}  // namespace

void launch_beam_full_begin(const BeamFullArgs& a, hipStream_t s) {
  check_shape(a, "beam_full_begin");
  if (!a.n_fin || !a.done || !a.n_live || !a.live_sum || !a.ts || !a.anc_dst) throw Error(kErrInvalidArg, "beam_full_begin: null array");
  hipLaunchKernelGGL(beam_full_begin, dim3(a.clips), dim3(64), 0, s, a);
}

void launch_beam_full_partial(const BeamFullArgs& a, hipStream_t s) {
  check_shape(a, "beam_full_partial");
  if (!a.logits || !a.part || (a.timestamps && !a.ts)) throw Error(kErrInvalidArg, "beam_full_partial: null array");
  const int rows = a.pos + 1 == a.n_prompt ? a.clips : a.K * a.clips;
  hipLaunchKernelGGL(beam_full_partial, dim3(beam_chunks(a.V), rows), dim3(kThreads), 0, s, a);
}

void launch_beam_full_select(const BeamFullArgs& a, hipStream_t s) {
  check_shape(a, "beam_full_select");
  if (!a.part || !a.ids_src || !a.lp_src || !a.n_live || !a.live_sum || !a.fin_tok || !a.fin_lp || !a.fin_sum || !a.fin_len ||
      !a.n_fin || !a.done || !a.parent || !a.token || !a.tok_lp || (a.timestamps && !a.ts)) {
    throw Error(kErrInvalidArg, "beam_full_select: null array");
  }
  hipLaunchKernelGGL(beam_full_select, dim3(a.clips), dim3(512), 0, s, a);
}

void launch_beam_full_advance(const BeamFullArgs& a, hipStream_t s) {
  check_shape(a, "beam_full_advance");
  if (!a.ids_src || !a.ids_dst || !a.lp_src || !a.lp_dst || !a.anc_src || !a.anc_dst || !a.parent || !a.token || !a.tok_lp) {
    throw Error(kErrInvalidArg, "beam_full_advance: null array");
  }
  hipLaunchKernelGGL(beam_full_advance, dim3(a.K * a.clips), dim3(256), 0, s, a);
}

void launch_beam_full_finalize(const BeamFullArgs& a, hipStream_t s) {
  check_shape(a, "beam_full_finalize");
  if (!a.ids_src || !a.lp_src || !a.n_live || !a.live_sum || !a.fin_tok || !a.fin_lp || !a.fin_sum || !a.fin_len || !a.n_fin ||
      !a.done || !a.out_ids || !a.out_lp || !a.out_n || !a.out_len || !a.out_sum) {
    throw Error(kErrInvalidArg, "beam_full_finalize: null array");
  }
  hipLaunchKernelGGL(beam_full_finalize, dim3(a.clips), dim3(256), 0, s, a);
}

}  // namespace wt
