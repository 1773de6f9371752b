// Word-level timestamps on the device: what Whisper's find_alignment does to the cross-attention
// weights W [clip][alignment head][fed position][encoder frame] of a teacher-forced pass.
//   align_scores        W = softmax over the clip's valid frames of q' . e_t, on the matrix cores (mode 0: softmax in
//                       the same kernel; mode 1, the default: blocks per frame chunk, then align_softmax_rows)
//   align_column_stats  mean and 1 / std of W[clip][head][.][t] over the clip's own positions
//   align_filter_mean   Z = (W - mean) / std, median of 7 along t with reflect padding, mean over the heads, negated:
//                       the cost C [clip][N][F] of the rows <|notimestamps|> .. last text id
//   align_dtw           dynamic time warping over C and the back-trace: jump[clip][row] = first frame of the row
// Every clip of a launch has its own position count, row count and frame count, read from device memory, so that no
// kernel argument depends on what a decode produced.
#include <hip/hip_runtime.h>

#include "bf16_split.h"
#include "kernels.h"

namespace wt {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using half8 = __attribute__((ext_vector_type(8))) _Float16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

struct AlignScoresDev {
  const float* qp;
  const _Float16* e;
  long e_plane;
  float e_scale;
  float* W;
  int B, H, T, np, pos0, n_heads, heads_total, L_max, ldw, tiles_per_chunk;
  int head[kAlignLayerHeadsMax], slot[kAlignLayerHeadsMax];
  int F[kAlignClipsMax];
};

// The attention weights themselves: W[b][slot][pos0 + p][t] = softmax over t < F_b of q'_head(row p B + b) . e_t, the
// score product of k_cross_absorbed.hip (E as its two fp16 planes, q' split in registers, three
// v_mfma_f32_16x16x32_f16 per 32 columns, fp32 accumulation) without its context product.  A wavefront owns 16 query
// columns (column c = head index x np + position) and sweeps every 16-frame tile of the clip: the E fragment (16 frames x
// 32 columns per step) is read straight from global memory, 16 bytes per lane and plane; the four wavefronts of a block
// sweep the same frames at the same time, so three of four reads hit the CU's cache.  The sweep stores the scaled scores
// and carries the column's running maximum and sum; a second sweep over the wavefront's own output turns them into
// weights and writes zero at the frames t >= F_b.  Every column is computed from its own query and the clip's E alone
// (its operand scale comes from its own largest element), so its bits do not depend on its neighbours, on the batch or
// on how the positions were cut into launches.
// FUSED = false (AlignScoresArgs::mode 1): the frames are cut into chunks of tiles_per_chunk tiles, one block each
// (blockIdx.z), so that a launch fills the chip whatever the number of columns; the kernel stores the scaled scores only
// and align_softmax_rows, one wavefront per row, turns them into weights.
// BF (bf16 storage mode, option full_bf16_all): E is the ONE bf16 plane the bf16 encoder leaves for
// the absorbed cross-attention (a.e points at it, e_plane and e_scale are not read), q' is rounded to bf16 in registers
// and a 32-column step is one v_mfma_f32_16x16x32_bf16, the score product of cross_absorbed_attention<DM, 3, true>: no
// operand scale, bf16 has the fp32 range.  Columns, tiles, chunks, maxima, sums and the zeros are as above.
template <int DM, bool FUSED, bool BF = false>
__global__ __launch_bounds__(256) void align_scores(AlignScoresDev a) {
  constexpr int KS = DM / 32;
  const int b = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int qc = lane & 15, lq = lane >> 4;
  const int n_cols = a.n_heads * a.np;
  const int c0 = (blockIdx.x * 4 + wid) * 16;
  if (c0 >= n_cols) return;  // (wavefront-uniform; the kernel has no barrier)
  const int col = c0 + qc;
  const bool q_ok = col < n_cols;
  const int hi = q_ok ? col / a.np : 0, p = q_ok ? col % a.np : 0;
  const int F = a.F[b];

  // ---- Q' planes of this lane's column: power-of-two scale from the column's largest element (k_cross_absorbed.hip)
  u32x4 qh[KS], ql[BF ? 1 : KS];  // (BF: one plane of q', no lo plane)
  (void)ql;
  float s_inv;
  if constexpr (BF) {
    const float* src = a.qp + ((long)p * a.B + b) * (long)(a.H * DM) + a.head[hi] * DM + 8 * lq;
    const float keep = q_ok ? 1.0f : 0.0f;
    s_inv = 1.0f;
#pragma unroll
    for (int c = 0; c < KS; ++c) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + 32 * c), v1 = *reinterpret_cast<const f32x4*>(src + 32 * c + 4);
      qh[c] = u32x4{pack_bf16x2(v0[0] * keep, v0[1] * keep), pack_bf16x2(v0[2] * keep, v0[3] * keep),
                    pack_bf16x2(v1[0] * keep, v1[1] * keep), pack_bf16x2(v1[2] * keep, v1[3] * keep)};
    }
  } else {
    const float* src = a.qp + ((long)p * a.B + b) * (long)(a.H * DM) + a.head[hi] * DM + 8 * lq;
    const float keep = q_ok ? 1.0f : 0.0f;
    float mx = 0.0f;
#pragma unroll
    for (int c = 0; c < KS; ++c) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + 32 * c), v1 = *reinterpret_cast<const f32x4*>(src + 32 * c + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fmaxf(fabsf(v0[e]), fabsf(v1[e])));
    }
    mx = xor32_max(xor16_max(mx * keep));
    const unsigned ex = (__float_as_uint(mx) >> 23) & 0xFFu;
    const float sc = ex < 32u ? 1.0f : __uint_as_float((268u - ex) << 23);  // largest element -> [2^14, 2^15)
    const float inv = ex < 32u ? 1.0f : __uint_as_float((ex - 14u) << 23);
    s_inv = inv / a.e_scale;
#pragma unroll
    for (int c = 0; c < KS; ++c) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + 32 * c), v1 = *reinterpret_cast<const f32x4*>(src + 32 * c + 4);
      const float own[8] = {v0[0] * keep, v0[1] * keep, v0[2] * keep, v0[3] * keep, v1[0] * keep, v1[1] * keep, v1[2] * keep, v1[3] * keep};
      u32x4_t pl[3];
      split8_f16x2(own, sc, pl);
      qh[c] = pl[0];
      ql[c] = pl[1];
    }
  }

  float* const out = a.W + (((long)b * a.heads_total + a.slot[hi]) * a.L_max + a.pos0 + p) * (long)a.ldw + 4 * lq;
  const _Float16* const eclip = a.e + (long)b * a.T * DM + 8 * lq;
  const int n_tiles = (a.T + 15) / 16;
  const int kt_lo = FUSED ? 0 : (int)blockIdx.z * a.tiles_per_chunk;
  const int kt_hi = FUSED ? n_tiles : (kt_lo + a.tiles_per_chunk < n_tiles ? kt_lo + a.tiles_per_chunk : n_tiles);
  float m_run = -__builtin_inff(), l_run = 0.0f;
  for (int kt = kt_lo; kt < kt_hi; ++kt) {
    int key = 16 * kt + qc;  // the A fragment's row of this lane: frames past T re-read the last one and are not stored
    key = key < a.T ? key : a.T - 1;
    const _Float16* const er = eclip + (long)key * DM;
    f32x4 sp = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < KS; ++c) {
      if constexpr (BF) {  // eight bf16 of the one plane: 16 bytes, as a lane's share of an fp16 plane
        const u32x4 eb = *reinterpret_cast<const u32x4*>(er + 32 * c);
        sp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, eb), __builtin_bit_cast(bf16x8, qh[c]), sp, 0, 0, 0);
      } else {
        const half8 eh = *reinterpret_cast<const half8*>(er + 32 * c);
        const half8 el = *reinterpret_cast<const half8*>(er + a.e_plane + 32 * c);
        sp = __builtin_amdgcn_mfma_f32_16x16x32_f16(eh, __builtin_bit_cast(half8, ql[c]), sp, 0, 0, 0);
        sp = __builtin_amdgcn_mfma_f32_16x16x32_f16(el, __builtin_bit_cast(half8, qh[c]), sp, 0, 0, 0);
        sp = __builtin_amdgcn_mfma_f32_16x16x32_f16(eh, __builtin_bit_cast(half8, qh[c]), sp, 0, 0, 0);
      }
    }
    // register r of this lane: frame 16 kt + 4 lq + r, column qc
    const int t0 = 16 * kt + 4 * lq;
    f32x4 sv;
    float tmax = -__builtin_inff();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sv[r] = sp[r] * s_inv;
      if (t0 + r < F) tmax = fmaxf(tmax, sv[r]);
    }
    if constexpr (!FUSED) {
      if (q_ok && t0 < a.T) *reinterpret_cast<f32x4*>(out + 16 * kt) = sv;
      continue;
    }
    tmax = xor32_max(xor16_max(tmax));  // the column's lanes qc, qc + 16, qc + 32, qc + 48
    if (tmax > m_run) {                 // (equal in the four lanes of a column)
      l_run *= __builtin_amdgcn_exp2f(m_run - tmax);
      m_run = tmax;
    }
    float psum = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (t0 + r < F) psum += __builtin_amdgcn_exp2f(sv[r] - m_run);
    l_run += xor32_sum(xor16_sum(psum));
    if (q_ok && t0 < a.T) *reinterpret_cast<f32x4*>(out + 16 * kt) = sv;
  }
  if (!FUSED || !q_ok) return;
  const float rl = 1.0f / l_run;
  for (int kt = 0; kt < n_tiles; ++kt) {
    const int t0 = 16 * kt + 4 * lq;
    if (t0 >= a.T) continue;
    f32x4 sv = *reinterpret_cast<const f32x4*>(out + 16 * kt);
#pragma unroll
    for (int r = 0; r < 4; ++r) sv[r] = t0 + r < F ? __builtin_amdgcn_exp2f(sv[r] - m_run) * rl : 0.0f;
    *reinterpret_cast<f32x4*>(out + 16 * kt) = sv;
  }
}

// mode 1: one wavefront per row W[b][slot][pos0 + p][.] of scaled scores: the maximum and the sum of exp2 over t < F_b,
// lane l taking the float4 groups l, l + 64, ... and the lanes combined in one fixed order, then the weights in place
// and zero at F_b <= t < T.
__global__ __launch_bounds__(64) void align_softmax_rows(AlignScoresDev a) {
  const int p = blockIdx.x, hi = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const int F = a.F[b], n4 = a.T / 4;
  float* const row = a.W + (((long)b * a.heads_total + a.slot[hi]) * a.L_max + a.pos0 + p) * (long)a.ldw;
  float m = -__builtin_inff();
  for (int g = lane; g < n4; g += 64) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g + r < F) m = fmaxf(m, v[r]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float l = 0.0f;
  for (int g = lane; g < n4; g += 64) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g + r < F) l += __builtin_amdgcn_exp2f(v[r] - m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o);
  const float rl = 1.0f / l;
  for (int g = lane; g < n4; g += 64) {
    f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = 4 * g + r < F ? __builtin_amdgcn_exp2f(v[r] - m) * rl : 0.0f;
    *reinterpret_cast<f32x4*>(row + 4 * g) = v;
  }
}

template <int DM, bool BF = false>
void launch_scores(const AlignScoresDev& g, bool fused, hipStream_t s) {
  const unsigned cols = unsigned((g.n_heads * g.np + 63) / 64);
  if (fused) {
    hipLaunchKernelGGL((align_scores<DM, true, BF>), dim3(cols, g.B), dim3(256), 0, s, g);
  } else {
    const int n_tiles = (g.T + 15) / 16;
    hipLaunchKernelGGL((align_scores<DM, false, BF>), dim3(cols, g.B, (n_tiles + g.tiles_per_chunk - 1) / g.tiles_per_chunk), dim3(256), 0, s, g);
    hipLaunchKernelGGL(align_softmax_rows, dim3(g.np, g.n_heads, g.B), dim3(64), 0, s, g);
  }
}

struct AlignMatDev {
  const float* W;
  const int *L, *F;
  float *stats, *C;
  int heads, L_max, ldw, n_a, N_max, ldc;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// One thread per (clip, head, frame): the column is read top to bottom, a wavefront 256 contiguous bytes per row.  The
// sums run in float64 (as k_scores.hip's), so the mean is the float64 one rounded once.  A column of equal values has
// std = 0 whatever its mean rounds to: it is recognised by min == max and gets rstd = 0 (Z = 0 instead of Whisper's NaN).
__global__ __launch_bounds__(256) void align_column_stats(AlignMatDev a) {
  const int b = blockIdx.z, h = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  const int L = clampi(a.L[b], 0, a.L_max), F = clampi(a.F[b], 0, a.ldw);
  if (t >= F || L < 1) return;
  const float* w = a.W + ((long)b * a.heads + h) * a.L_max * (long)a.ldw + t;
  double sum = 0.0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int i = 0; i < L; ++i) {
    const float x = w[(long)i * a.ldw];
    sum += (double)x;
    mn = fminf(mn, x), mx = fmaxf(mx, x);
  }
  const double mean = sum / (double)L;
  double var = 0.0;
  for (int i = 0; i < L; ++i) {
    const double d = (double)w[(long)i * a.ldw] - mean;
    var += d * d;
  }
  float* st = a.stats + ((long)b * a.heads + h) * 2 * (long)a.ldw + t;
  st[0] = (float)mean;
  st[a.ldw] = mn == mx ? 0.0f : (float)(1.0 / sqrt(var / (double)L));
}

__device__ __forceinline__ void order(float& x, float& y) {
  const float lo = fminf(x, y), hi = fmaxf(x, y);
  x = lo, y = hi;
}

// One thread per (clip, cost row, frame).  The seven neighbours are normalised again by every thread that needs them:
// they come from the same few cache lines the wavefront reads anyway.  Heads are added in ascending order.
__global__ __launch_bounds__(256) void align_filter_mean(AlignMatDev a) {
  const int b = blockIdx.z, r = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  const int L = clampi(a.L[b], 0, a.L_max), F = clampi(a.F[b], 0, a.ldw < a.ldc ? a.ldw : a.ldc);
  const int N = clampi(L - a.n_a - 1, 0, a.N_max);
  if (t >= F || r >= N) return;
  int idx[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    int j = t + k - 3;
    j = j < 0 ? -j : j;
    j = j > F - 1 ? 2 * (F - 1) - j : j;
    idx[k] = F > 3 ? j : t;  // the filter is skipped when F <= 3, as in Whisper
  }
  float acc = 0.0f;
  for (int h = 0; h < a.heads; ++h) {
    const long bh = (long)b * a.heads + h;
    const float* row = a.W + (bh * a.L_max + a.n_a + r) * (long)a.ldw;
    const float* mean = a.stats + bh * 2 * (long)a.ldw;
    const float* rstd = mean + a.ldw;
    float v[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = (row[idx[k]] - mean[idx[k]]) * rstd[idx[k]];
#pragma unroll
    for (int pass = 0; pass < 6; ++pass)  // bubble sort, unrolled: 21 min / max pairs
#pragma unroll
      for (int k = 0; k < 6 - pass; ++k) order(v[k], v[k + 1]);
    acc += v[3];
  }
  a.C[((long)b * a.N_max + r) * a.ldc + t] = -(acc / (float)a.heads);
}

struct AlignDtwDev {
  const float* C;
  const int *N, *F;
  unsigned char* trace;
  int* jump;
  int N_max, ldc;
};

// One block per clip, thread i - 1 owns row i of D (1-based, as in wt::dtw_path).  The cells of anti-diagonal k = i + j
// need diagonal k - 1 at rows i and i - 1 and diagonal k - 2 at row i - 1: three diagonals rotate through LDS, one
// barrier per diagonal (the diagonal written now was read last two diagonals ago, behind the previous barrier).  The
// border of D is not stored: it is 0 at (0, 0) and +inf elsewhere.  The cost of the next diagonal's cell is loaded
// before the barrier.  Each cell is one fp32 add of a minimum, so the order of evaluation does not show in the bits.
// The trace codes go to global memory; then wavefront 0 walks back, 64 codes of a row at a time: the path leaves row i
// at the first code that is not 2, and the frame of that cell is jump[i - 1].
template <int NT>
__global__ __launch_bounds__(NT) void align_dtw(AlignDtwDev a) {
  __shared__ float diag[3][kAlignRowsMax + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = clampi(a.N[b], 0, a.N_max < NT ? a.N_max : NT), F = clampi(a.F[b], 0, a.ldc);
  const float* const C = a.C + (long)b * a.N_max * a.ldc;
  unsigned char* const tr = a.trace + (long)b * a.N_max * a.ldc;
  int* const jump = a.jump + (long)b * a.N_max;
  for (int r = tid; r < a.N_max; r += NT) jump[r] = 0;
  if (N < 1 || F < 1) return;  // (block-uniform)
  const float inf = __builtin_inff();
  const int i = tid + 1;
  const bool mine = i <= N;
  const float* const crow = C + (long)(i - 1) * a.ldc;
  unsigned char* const trow = tr + (long)(i - 1) * a.ldc;
  float cnext = (mine && i == 1) ? crow[0] : 0.0f;  // diagonal 2 is the cell (1, 1)
  for (int k = 2; k <= N + F; ++k) {
    const int j = k - i;
    const bool on = mine && j >= 1 && j <= F;
    const float cost = cnext;
    if (mine && j + 1 >= 1 && j + 1 <= F) cnext = crow[j];  // the cell (i, j + 1) of diagonal k + 1
    if (on) {
      const float* const d1 = diag[(k + 2) % 3];  // diagonal k - 1
      const float* const d2 = diag[(k + 1) % 3];  // diagonal k - 2
      const float c0 = (i == 1 && j == 1) ? 0.0f : (i == 1 || j == 1) ? inf : d2[i - 1];
      const float c1 = i == 1 ? inf : d1[i - 1];
      const float c2 = j == 1 ? inf : d1[i];
      diag[k % 3][i] = cost + fminf(fminf(c0, c1), c2);
      trow[j - 1] = (c0 < c1 && c0 < c2) ? 0 : (c1 < c0 && c1 < c2) ? 1 : 2;  // 2 on c0 == c1 < c2 as well, as in dtw_path
    }
    __syncthreads();
  }
  // (the barrier of the last diagonal: every trace code of the block is visible to the block)
  if (tid >= 64) return;
  int ri = N, rj = F;
  while (ri > 0 && rj > 0) {
    const int jj = rj - tid;  // this lane's column, 1-based; columns left of the matrix act as the border's code 1
    const unsigned code = jj >= 1 ? tr[(long)(ri - 1) * a.ldc + (jj - 1)] : 1u;
    const unsigned long long stop = __ballot(code != 2u);
    if (stop == 0ull) {
      rj -= 64;
      continue;
    }
    const int l = __ffsll((long long)stop) - 1;
    const unsigned code_l = (unsigned)__shfl((int)code, l);
    const int jl = rj - l;
    if (jl < 1) break;  // the border: only a cost that is not finite leads here; the rows above keep jump = 0
    if (tid == 0) jump[ri - 1] = jl - 1;
    rj = code_l == 0u ? jl - 1 : jl;
    ri -= 1;
  }
}

}  // namespace

void launch_align_scores(const AlignScoresArgs& a, hipStream_t s) {
  const int dm = a.d_model;
  bool ok = a.qp && a.e && a.W && a.batch >= 1 && a.batch <= kAlignClipsMax && a.H >= 1 && a.H * 64 == dm && a.T >= 4 &&
            a.T <= kAlignFramesMax && a.T % 4 == 0 && a.np >= 1 && (long)a.np * a.batch <= 128 && a.pos0 >= 0 && a.L_max >= 1 &&
            a.pos0 + a.np <= a.L_max && a.n_heads >= 1 && a.n_heads <= kAlignLayerHeadsMax && a.n_heads <= a.H &&
            a.heads_total >= 1 && a.heads_total <= kAlignHeadsMax && a.ldw >= a.T && a.ldw % 4 == 0;
  // (bf16: one plane, no operand scale: e_plane and e_scale are not read)
  ok = ok && (a.bf16 || (a.e_scale > 0.0f && a.e_plane >= (long)a.batch * a.T * dm && a.e_plane % 8 == 0));
  ok = ok && (a.mode == 0 || a.mode == 1);
  for (int i = 0; ok && i < a.n_heads; ++i) {
    ok = a.head[i] >= 0 && a.head[i] < a.H && a.slot[i] >= 0 && a.slot[i] < a.heads_total;
    for (int j = 0; ok && j < i; ++j) ok = a.head[j] != a.head[i] && a.slot[j] != a.slot[i];  // two columns would share rows of W
  }
  for (int b = 0; ok && b < a.batch; ++b) ok = a.F[b] >= 1 && a.F[b] <= a.T;
  if (!ok) throw Error(kErrInvalidArg, "alignment scores: shape outside the kernel contract");
  AlignScoresDev g{};
  g.qp = a.qp, g.e = reinterpret_cast<const _Float16*>(a.e), g.W = a.W;
  g.e_plane = a.bf16 ? 0 : a.e_plane, g.e_scale = a.bf16 ? 1.0f : a.e_scale;
  g.B = a.batch, g.H = a.H, g.T = a.T, g.np = a.np, g.pos0 = a.pos0, g.n_heads = a.n_heads, g.heads_total = a.heads_total;
  g.L_max = a.L_max, g.ldw = a.ldw, g.tiles_per_chunk = kAlignChunkTiles;
  for (int i = 0; i < a.n_heads; ++i) g.head[i] = a.head[i], g.slot[i] = a.slot[i];
  for (int b = 0; b < a.batch; ++b) g.F[b] = a.F[b];
  switch (dm) {
    case 128: a.bf16 ? launch_scores<128, true>(g, a.mode == 0, s) : launch_scores<128>(g, a.mode == 0, s); break;
    case 384: a.bf16 ? launch_scores<384, true>(g, a.mode == 0, s) : launch_scores<384>(g, a.mode == 0, s); break;
    case 512: a.bf16 ? launch_scores<512, true>(g, a.mode == 0, s) : launch_scores<512>(g, a.mode == 0, s); break;
    default: throw Error(kErrInvalidArg, "alignment scores: d_model 128, 384 or 512");
  }
}

void launch_align_matrix(const AlignMatrixArgs& a, hipStream_t s) {
  if (!a.W || !a.L || !a.F || !a.stats || !a.C || a.clips < 1 || a.clips > 65535 || a.heads < 1 || a.heads > kAlignHeadsMax ||
      a.L_max < 1 || a.ldw < 1 || a.ldw > kAlignFramesMax || a.n_a < 0 || a.N_max < 1 || a.N_max > kAlignRowsMax || a.ldc < 1 ||
      a.ldc > kAlignFramesMax) {
    throw Error(kErrInvalidArg, "alignment matrix: shape outside the kernel contract");
  }
  const AlignMatDev g{a.W, a.L, a.F, a.stats, a.C, a.heads, a.L_max, a.ldw, a.n_a, a.N_max, a.ldc};
  hipLaunchKernelGGL(align_column_stats, dim3((a.ldw + 255) / 256, a.heads, a.clips), dim3(256), 0, s, g);
  hipLaunchKernelGGL(align_filter_mean, dim3((a.ldc + 255) / 256, a.N_max, a.clips), dim3(256), 0, s, g);
}

void launch_align_dtw(const AlignDtwArgs& a, hipStream_t s) {
  if (!a.C || !a.N || !a.F || !a.trace || !a.jump || a.clips < 1 || a.N_max < 1 || a.N_max > kAlignRowsMax || a.ldc < 1 ||
      a.ldc > kAlignFramesMax) {
    throw Error(kErrInvalidArg, "alignment DTW: at most 447 rows and 1500 frames per clip");
  }
  const AlignDtwDev g{a.C, a.N, a.F, a.trace, a.jump, a.N_max, a.ldc};
  if (a.N_max <= 64) {
    hipLaunchKernelGGL(align_dtw<64>, dim3(a.clips), dim3(64), 0, s, g);
  } else if (a.N_max <= 256) {
    hipLaunchKernelGGL(align_dtw<256>, dim3(a.clips), dim3(256), 0, s, g);
  } else {
    hipLaunchKernelGGL(align_dtw<512>, dim3(a.clips), dim3(512), 0, s, g);
  }
}

}  // namespace wt
