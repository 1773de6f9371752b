// Truncated sampling (options top_k, top_p): the cut of a row of logits, in front of sample_partial.
// With the allowed ids A of the row ordered by the record key ord(z_i) << 32 | i, descending (the larger logit first, the
// larger id among equal logits), K is the first min(top_k, |A|) of them and N the shortest prefix of K whose mass reaches
// top_p times the mass of K, p_i = exp((z_i - m) / T).  nucleus_cut writes the key of N's last id; the sampler then
// draws its Gumbel maximum over key >= cut.
//   one block of 1024 threads per row.  V <= 65536: the row is read once, as the aligned float4 quads of sample_partial,
//   into 64 registers per thread (the ordered logit, 0 outside A) and every pass below runs from them; larger V (up to
//   2^20): the same code re-reads the row on each pass (kReg = false).
//   mass is fixed point: q_i = floor(p_i 2^40) in 64 bits, p_i = exp2 of one fma.  Every sum of q is an integer sum, so
//   histograms filled by LDS atomics, and with them the cut, do not depend on the order of arrival.
//   the search is a radix select on the 52-bit key ord << 20 | id in five levels of 11 / 11 / 10 / 10 / 10 bits: the
//   three levels of the logit, then two of the id, which rank equal logits by id with the very same code.  A level
//   adds 1 (top-k) or q (top-p) per entry under the prefix found so far into a 2048-bin LDS histogram; wavefront 0
//   takes a suffix sum over the bins from the top, finds the bin where the running sum (with what lies above the
//   prefix) reaches the target, and the search descends into it.  The other wavefronts clear the second histogram for
//   the next level meanwhile.  After the fifth level the prefix is the key itself.
//   top-k runs first; top-p runs over the entries at or above the k-cut with the target ceil(top_p * their mass).
#include <hip/hip_runtime.h>

#include <cmath>

#include "error.h"
#include "kernels.h"
#include "ts_rules.h"

namespace wt {
namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kRegQuads = 16;                      // quads a thread keeps: 4 * 16 * 1024 = 65536 entries
constexpr int kRegV = 4 * kRegQuads * kThreads;
constexpr int kBins = 2048;
constexpr int kLevels = 5, kIdBits = 20;           // key52 = ord << 20 | id, V <= 2^20
typedef unsigned long long u64;

// float -> unsigned with the same order (k_sample.hip's)
__device__ __forceinline__ unsigned ord_of(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? (u == 0x80000000u ? 0x80000000u : ~u) : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// the sum over the block, in every thread (integers: any order); red [kWaves] is free again behind it
__device__ __forceinline__ u64 block_sum(u64 v, u64* red, int tid) {
  v = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  u64 s = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += red[w];
  return s;
}
__device__ __forceinline__ unsigned ord_in(const Allowed& a, float e, int i) {
  const bool in = (i >= a.t_lo && i <= a.t_hi) || (i >= a.s_lo && i <= a.s_hi);  // (t_hi, s_hi < V)
  return in ? ord_of(e) : 0u;
}

// f(ordered logit or 0, id) over the row's entries: from the registers, or from memory again
template <bool kReg, class F>
__device__ __forceinline__ void for_entries(const unsigned* o, const float* z, int V, const Allowed& a, int tid, F&& f) {
  if constexpr (kReg) {
#pragma unroll
    for (int j = 0; j < kRegQuads; ++j) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        // (an opaque copy: nothing computed from an entry is hoisted out of the level loop, where 64 keys and masses
        // held at once would push the row itself out of the 128 registers; one quad at a time for the same reason)
        unsigned x = o[4 * j + c];
        asm volatile("" : "+v"(x));
        f(x, j * 4 * kThreads + 4 * tid + c);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    for (int i0 = 4 * tid; i0 < V; i0 += 4 * kThreads) {
      const float4 q = *reinterpret_cast<const float4*>(z + i0);  // (i0 + 3 < ldl)
      const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) f(ord_in(a, e[c], i0 + c), i0 + c);
    }
  }
}

template <bool kReg>
__global__ __launch_bounds__(kThreads) void nucleus_cut(const float* __restrict__ logits, int ldl, int V,
                                                        const TsState* __restrict__ state, int n_gen, int eot, int beg,
                                                        int mit, const SampleParams* __restrict__ prm, int row0, int clips,
                                                        NucleusCut* __restrict__ out) {
  __shared__ u64 hist[2][kBins];
  __shared__ u64 red[kWaves];
  __shared__ u64 sel[2];  // the level's result: the prefix with its bin, and the sum above that bin
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  Allowed a;
  if (state) {
    a = allowed_of(state[row], n_gen, V, eot, beg, mit);
  } else {
    a.t_lo = 0, a.t_hi = V - 1, a.s_lo = V, a.s_hi = V - 1;
  }
  const float inv_t = prm->inv_t[row0 + (clips > 0 ? row % clips : row)];
  const int top_k = prm->top_k;
  const float top_p = prm->top_p;
  const float* z = logits + (long)row * ldl;
  unsigned o[kReg ? 4 * kRegQuads : 1];
  if constexpr (kReg) {
#pragma unroll
    for (int j = 0; j < kRegQuads; ++j) {
      const int i0 = j * 4 * kThreads + 4 * tid;
      float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (i0 < V) q = *reinterpret_cast<const float4*>(z + i0);  // (ids from V on lie outside A)
      const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) o[4 * j + c] = ord_in(a, e[c], i0 + c);
      if (j % 4 == 3) __builtin_amdgcn_sched_barrier(0);  // four loads in flight, not sixteen beside their results
    }
  }
  // pass 0: the maximum and |A|
  unsigned omax = 0u;
  u64 n_a = 0;
  for_entries<kReg>(o, z, V, a, tid, [&](unsigned oi, int) {
    omax = oi > omax ? oi : omax;
    n_a += oi != 0u;
  });
  n_a = block_sum(n_a, red, tid);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned t = __shfl_xor(omax, off, 64);
    omax = t > omax ? t : omax;
  }
  __syncthreads();
  if (lane == 0) red[wid] = omax;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) omax = (unsigned)red[w] > omax ? (unsigned)red[w] : omax;
  const float m = float_of(omax);
  const float c1 = inv_t * 1.44269504088896341f, c0 = -(m * c1);  // p = exp2(z c1 + c0)
  NucleusCut r;
  r.cut = 0ull, r.kept_q = r.total_q = 0ull, r.kept = (int)n_a, r.pad = 0;
  // (block-uniform) nothing to cut: an empty set, a greedy row, no finite scale
  if (n_a == 0 || !(inv_t > 0.0f) || omax == 0u || isinf(m) || isnan(m) || isinf(c0) || isnan(c0)) {
    if (tid == 0) out[row] = r;
    return;
  }
  auto q_of = [&](unsigned oi) { return (u64)(exp2f(fmaf(float_of(oi), c1, c0)) * 0x1p40f); };
  // count and mass of the entries at or above a 52-bit key
  auto tally = [&](u64 floor52, u64& count, u64& mass) {
    u64 n = 0, q = 0;
    for_entries<kReg>(o, z, V, a, tid, [&](unsigned oi, int i) {
      if (oi != 0u && (((u64)oi << kIdBits) | (unsigned)i) >= floor52) n += 1, q += q_of(oi);
    });
    count = block_sum(n, red, tid);
    mass = block_sum(q, red, tid);
  };
  u64 kept = 0, kept_q = 0;
  tally(0ull, kept, kept_q);
  r.total_q = kept_q;
  u64 cut52 = 0ull;
#pragma unroll 1
  for (int phase = 0; phase < 2; ++phase) {
    const bool by_mass = phase == 1;
    u64 target;
    if (!by_mass) {
      if (top_k <= 0) continue;
      target = (u64)top_k < kept ? (u64)top_k : kept;  // (top_k >= |A|: the smallest key of A)
    } else {
      if (!(top_p > 0.0f && top_p < 1.0f) || kept_q == 0) continue;
      const double t = ceil((double)top_p * (double)kept_q);
      target = t < 1.0 ? 1ull : (u64)t;
      target = target > kept_q ? kept_q : target;
    }
    // (1 <= target <= the sum over the entries at or above cut52: every level finds its bin)
    const u64 floor52 = cut52;
    u64 prefix = 0ull, above = 0ull;
    for (int b = tid; b < kBins; b += kThreads) hist[0][b] = 0ull;
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < kLevels; ++l) {
      const int w = l < 2 ? 11 : 10, sh = l < 2 ? 41 - 11 * l : 20 - 10 * (l - 2), nb = 1 << w;
      u64* const h = hist[l & 1];
      for_entries<kReg>(o, z, V, a, tid, [&](unsigned oi, int i) {
        const u64 key = ((u64)oi << kIdBits) | (unsigned)i;
        if (oi == 0u || key < floor52 || (key >> (sh + w)) != prefix) return;
        atomicAdd(&h[(int)(key >> sh) & (nb - 1)], by_mass ? q_of(oi) : 1ull);
      });
      __syncthreads();
      if (wid == 0) {
        const int per = nb / 64;  // bins per lane, the higher bins in the higher lanes
        u64 tot = 0ull;
        for (int k = 0; k < per; ++k) tot += h[lane * per + k];
        u64 inc = tot;  // -> the sum over this lane and those above it
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const u64 t = __shfl_down(inc, off, 64);
          if (lane + off < 64) inc += t;
        }
        const u64 over = above + inc - tot;
        if (lane == 0) sel[0] = prefix << w, sel[1] = above;  // (never kept: one lane below holds the crossing)
        if (over < target && over + tot >= target) {
          u64 run = over;
          int b = lane * per + per - 1;
          for (; b > lane * per; --b) {
            if (run + h[b] >= target) break;
            run += h[b];
          }
          sel[0] = (prefix << w) | (u64)b, sel[1] = run;
        }
      } else {
        u64* const next = hist[(l + 1) & 1];
        for (int b = tid - 64; b < kBins; b += kThreads - 64) next[b] = 0ull;
      }
      __syncthreads();
      prefix = sel[0], above = sel[1];
    }
    cut52 = prefix;
    tally(cut52, kept, kept_q);  // top-k: the mass top-p works on
  }
  if (tid == 0) {
    r.cut = ((cut52 >> kIdBits) << 32) | (cut52 & ((1ull << kIdBits) - 1));
    r.kept = (int)kept, r.kept_q = kept_q;
    out[row] = r;
  }
}

}  // namespace

void launch_nucleus_cut(const NucleusArgs& a, hipStream_t s) {
  const bool ts = a.state != nullptr;
  if (a.rows < 1 || a.V < 2 || a.V > (1 << kIdBits) || a.eot < 0 || a.eot >= a.V || (ts && (a.eot >= a.beg || a.beg >= a.V)) ||
      a.ldl < a.V || a.ldl % 4 != 0 || (reinterpret_cast<uintptr_t>(a.logits) & 15) != 0 || a.n_gen < 0 || a.max_initial < -1 ||
      !a.params || !a.out || a.row0 < 0 || a.clips < 0 || a.row0 + (a.clips > 0 ? a.clips : a.rows) > kSampleClipsMax) {
    throw Error(kErrInvalidArg, "nucleus_cut: needs 0 <= eot (< beg) < V <= 2^20, 16-byte aligned logits rows and at most 64 clips");
  }
  if (a.V <= kRegV) {
    hipLaunchKernelGGL(nucleus_cut<true>, dim3(a.rows), dim3(kThreads), 0, s, a.logits, a.ldl, a.V, a.state, a.n_gen, a.eot, a.beg,
                       a.max_initial, a.params, a.row0, a.clips, a.out);
  } else {
    hipLaunchKernelGGL(nucleus_cut<false>, dim3(a.rows), dim3(kThreads), 0, s, a.logits, a.ldl, a.V, a.state, a.n_gen, a.eot, a.beg,
                       a.max_initial, a.params, a.row0, a.clips, a.out);
  }
}

}  // namespace wt
