// The int8 dynamic-range encoder conv stem for gfx950 (option "encoder_int8" = 2): the two width-3
// convolutions in front of the encoder blocks as TFLite's hybrid convolution computes them.  W is conv_gemm_order's
// [co][tap * C_in + ci] as int8 rows + one fp32 scale per output channel (quantize_rows_i8, K padded with zero columns
// to a multiple of 32, tile_rows_i8); the input is quantised with ONE scale per clip, sx[b] = amax[b] / 127 (row_scale_i8's
// rule on the clip's largest |x|), element by element with dec_rows.h's quant_i8; int32 sums on v_mfma_i32_32x32x32_i8;
//   t = ((float)acc * sx[b]) * sw[n];  0: t + bias;  1: gelu_erf(t + bias);  2: gelu_erf(t + bias) + pos[t_out][n]
// every product and sum rounded on its own (-ffp-contract=fast-honor-pragmas, the epilogue under contract(off)).
//
// The clip's scale is known before the contraction starts, so there is no quantise launch and no qx buffer: a block
// reads fp32 input rows and quantises them on their way into LDS, each element once, and all three taps of an output row
// are MFMA A-fragments of the same LDS rows.  Kernels:
//   * clip_absmax_f32: amax[b] = max |x| over a clip's contiguous floats.  16-byte loads, one value per block, merged by
//     one atomicMax on the value's bits (non-negative floats order as their bit patterns: no dependence on block order).
//   * enc_conv1_i8<CIN, EPI> (stride 1, C_in = n_mels = 80 or 128): the 130 input rows of a 128-row tile are ONE flat
//     run of 130 * C_in floats and land in LDS at a pitch of exactly C_in bytes.  Output row r's K vector (taps 0, 1, 2 =
//     rows r, r + 1, r + 2) is then the contiguous bytes [r C_in, r C_in + 3 C_in): K runs straight through the taps, and
//     on into the next row's bytes for the zero-weight padding columns (K = 240 -> 256), which integer arithmetic ignores.
//   * enc_conv2_i8<CIN, EPI> (stride 2, C_in = 128, 384 or 512): channels are streamed in chunks of 64 through two LDS
//     buffers.  A chunk's 257 input rows (2 * 127 + 3) are split by parity: even rows in one region, odd rows in another,
//     each at a pitch of 80 bytes.  Tap j of output row r is input row 2 r + j = even[r], odd[r], even[r + 1], so the 32
//     rows of a fragment read are CONSECUTIVE rows of one region and the read is as conflict-free as enc_gemm_i8's (one
//     region at a pitch P would put them 2 P apart: an even number of 16-byte slots, every second bank group unused).  The
//     next chunk's global loads are issued before the current chunk's 24 MFMAs and quantised and stored behind them, one
//     barrier per chunk.
// Both: 256 threads = 2 x 2 wavefronts on a tile of 128 output rows x 128 output channels of ONE clip (grid N / 128,
// ceil(T_out / 128), B: no tile straddles two clips, a block reads one scale), each wavefront 64 x 64 as 2 x 2
// accumulators.  W fragments come straight from global memory in tile_rows_i8's order, one group of k-steps ahead in
// registers.  Loads are clamped into the clip's padded rows, stores guarded by row < T_out, every trip count is a
// template constant, stores use a wave-uniform row base plus a 32-bit lane offset.  On request the epilogue reduces
// |output| over the tile's valid elements into amax_out[b] with one atomicMax per block: conv1 so leaves conv2's scale.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dec_rows.h"
#include "kernels.h"

namespace wt {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

constexpr int kTile = 128;  // output rows and output channels of a block's tile

// max over the block's 256 threads; `red` holds 4 floats.  Thread 0 returns the block's value.
__device__ __forceinline__ float block_max(float m, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ------------------------------------------------------------------------------------------ the clip maximum ---
__global__ __launch_bounds__(64) void zero_words(unsigned* p, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) p[i] = 0u;
}

// x [B][n4 pieces of 4 floats]; grid (blocks per clip, B)
__global__ __launch_bounds__(256) void clip_absmax_f32(const f32x4* __restrict__ x, unsigned n4, float* __restrict__ amax) {
  __shared__ float red[4];
  const f32x4* xc = x + (size_t)blockIdx.y * n4;
  float m = 0.0f;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
    const f32x4 v = xc[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));  // fmaxf drops a NaN
  }
  m = block_max(m, red);
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(amax) + blockIdx.y, __float_as_uint(m));
}

// ------------------------------------------------------------------------------------------- the convolutions ---
struct EncConvDev {
  const float* X;     // [B][T_in + 2][C_in], the pad rows zero
  const float* amax;  // [B]
  const i32x4* Wq;    // [N / 32][KP / 32][64]
  const float* sw;    // [N]
  const float* bias;
  const float* pos;  // [T_out][N] (epilogue 2)
  float* Y;          // clip b's row t at Y + b * y_bs + t * N
  long y_bs;
  float* amax_out;  // [B] or null
  int T_in, T_out, N;
};

// the block's clip: its scales by row_scale_i8's rule (IEEE divisions, both 0 at amax == 0)
__device__ __forceinline__ void clip_scale(const EncConvDev& g, int b, float* sx, float* inv) {
  const float mx = g.amax[b];
  *sx = mx > 0.0f ? __fdiv_rn(mx, 127.0f) : 0.0f;
  *inv = mx > 0.0f ? __fdiv_rn(127.0f, mx) : 0.0f;
}

// the wavefront's two 32-column W tiles, k-step s of the launch at [s * 64]
template <int KS>
__device__ __forceinline__ void w_tiles(const EncConvDev& g, int n0, int wn, int lane, const i32x4* (&wp)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) wp[j] = g.Wq + (long)((n0 + wn * 64 + j * 32) >> 5) * KS * 64 + lane;
}

template <int EPI>
__device__ __forceinline__ void conv_epilogue(const EncConvDev& g, const i32x16 (&acc)[2][2], int b, int t0, int n0, float sx,
                                              float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1, l31 = lane & 31, lh = lane >> 5;
  const int N = g.N;
  int n[2];
  float swn[2], bn[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    n[j] = n0 + wn * 64 + j * 32 + l31;  // < N: N is a multiple of the tile
    swn[j] = g.sw[n[j]], bn[j] = g.bias[n[j]];
  }
  float* const yb = g.Y + (long)b * g.y_bs;
  float mx = 0.0f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma clang fp contract(off)
      const int tr = t0 + wm * 64 + i * 32 + crow(r, 0);  // the row is tr + 4 lh
      if (tr + 4 * lh < g.T_out) {
        float* const yp = yb + (long)tr * N;
        const float* const pp = g.pos + (long)tr * N;  // (never read without epilogue 2)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const unsigned off = (unsigned)(4 * lh * N + n[j]);
          // plain operators: the pragma is lexical
          const float t = ((float)acc[i][j][r] * sx) * swn[j];  // this order: (acc * sx) * sw
          float v = t + bn[j];
          if (EPI >= 1) v = gelu_erf(v);
          if (EPI == 2) v = v + pp[off];
          yp[off] = v;
          mx = fmaxf(mx, fabsf(v));
        }
      }
    }
  }
  if (g.amax_out) {  // (uniform over the launch)
    mx = block_max(mx, red);
    if (tid == 0) atomicMax(reinterpret_cast<unsigned*>(g.amax_out) + b, __float_as_uint(mx));
  }
}

// Stride 1.  KP = 3 CIN rounded up to 32 (256 or 384), in groups of 4 k-steps.
template <int CIN, int EPI>
__global__ __launch_bounds__(256) void enc_conv1_i8(EncConvDev g) {
  constexpr int KS = (3 * CIN + 31) / 32, NG = KS / 4;
  static_assert(KS % 4 == 0 && CIN % 16 == 0, "whole groups of 4 k-steps, 16-byte rows");
  constexpr int NP = (kTile + 2) * CIN / 4;  // 4-float pieces of the tile's input rows
  constexpr int PASS = (NP + 255) / 256;
  // + 16: row 127's K runs KP - 3 CIN bytes past row 129 (zero weights; the bytes are zeroed all the same)
  __shared__ __attribute__((aligned(16))) signed char as[(kTile + 2) * CIN + 16];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1, l31 = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * kTile, t0 = blockIdx.y * kTile, b = blockIdx.z;
  float sx, inv;
  clip_scale(g, b, &sx, &inv);
  // the tile's padded rows t0 .. t0 + 129 are one flat run of the clip; pieces past the clip's last row re-read its
  // last piece (a pad row's zeros) and feed only rows >= T_out, which are never stored
  const f32x4* const xc = reinterpret_cast<const f32x4*>(g.X + ((long)b * (g.T_in + 2) + t0) * CIN);
  const int last = (g.T_in + 2 - t0) * (CIN / 4) - 1;
  f32x4 xr[PASS];
#pragma unroll
  for (int p = 0; p < PASS; ++p) {
    const int i = tid + 256 * p;
    xr[p] = xc[i < last ? i : last];
  }
  const i32x4* wp[2];
  w_tiles<KS>(g, n0, wn, lane, wp);
  i32x4 w[2][2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s) w[0][j][s] = wp[j][s * 64];
#pragma unroll
  for (int p = 0; p < PASS; ++p) {
    const int i = tid + 256 * p;
    if (i < NP) *reinterpret_cast<unsigned*>(&as[4 * i]) = quant4_i8(xr[p], inv);
  }
  if (tid < 4) *reinterpret_cast<unsigned*>(&as[(kTile + 2) * CIN + 4 * tid]) = 0u;
  __syncthreads();

  i32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
  const signed char* const a = as + (wm * 64 + l31) * CIN + 16 * lh;
#pragma unroll
  for (int c = 0; c < NG; ++c) {
    if (c + 1 < NG) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) w[(c + 1) & 1][j][s] = wp[j][((c + 1) * 4 + s) * 64];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const i32x4 a0 = *reinterpret_cast<const i32x4*>(a + (c * 4 + s) * 32);
      const i32x4 a1 = *reinterpret_cast<const i32x4*>(a + 32 * CIN + (c * 4 + s) * 32);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc[0][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, w[c & 1][j][s], acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, w[c & 1][j][s], acc[1][j], 0, 0, 0);
      }
    }
  }
  conv_epilogue<EPI>(g, acc, b, t0, n0, sx, red);
}

// Stride 2.  Channel chunks of 64: per chunk 3 taps x 2 k-steps; W one tap ahead.
constexpr int kCC = 64;                 // channels per chunk
constexpr int kPitch2 = kCC + 16;       // an odd multiple of 16 bytes
constexpr int kRows2 = 2 * kTile + 1;   // input rows 0 .. 2 * 127 + 2 of a tile
constexpr int kOdd2 = (kTile + 1) * kPitch2;  // the odd rows' region behind the 129 even rows
constexpr int kBuf2 = kRows2 * kPitch2;

template <int CIN, int EPI>
__global__ __launch_bounds__(256) void enc_conv2_i8(EncConvDev g) {
  static_assert(CIN % kCC == 0, "whole chunks");
  constexpr int NCH = CIN / kCC, KS = 3 * CIN / 32, NQ = 3 * NCH;
  constexpr int PASS = (kRows2 + 15) / 16;  // 16 rows of 16 pieces per pass: 17, the last one row
  __shared__ __attribute__((aligned(16))) signed char as[2][kBuf2];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1, l31 = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * kTile, t0 = blockIdx.y * kTile, b = blockIdx.z;
  float sx, inv;
  clip_scale(g, b, &sx, &inv);
  // staging: thread (row tid >> 4 (+ 16 p), piece tid & 15) of every chunk; rows past the clip's last padded row re-read
  // it (zeros) and feed only rows >= T_out
  const int sr = tid >> 4, sc = tid & 15, rmax = g.T_in + 1 - 2 * t0;
  const float* const xc = g.X + ((long)b * (g.T_in + 2) + 2 * t0) * CIN + sc * 4;
  unsigned xo[PASS];
#pragma unroll
  for (int p = 0; p < PASS; ++p) {
    const int r = sr + 16 * p;
    xo[p] = (unsigned)((r < rmax ? r : rmax) * CIN);
  }
  // row r lands in region r & 1 at row r >> 1: sr's parity is the thread's
  signed char* const sdst = &as[0][0] + (sr & 1) * kOdd2 + (sr >> 1) * kPitch2 + sc * 4;
  const i32x4* wp[2];
  w_tiles<KS>(g, n0, wn, lane, wp);

  f32x4 xr[PASS];
  i32x4 w[2][2][2];
#pragma unroll
  for (int p = 0; p < PASS; ++p) xr[p] = *reinterpret_cast<const f32x4*>(xc + xo[p]);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int s = 0; s < 2; ++s) w[0][j][s] = wp[j][s * 64];
#pragma unroll
  for (int p = 0; p < PASS; ++p)
    if (p + 1 < PASS || sr == 0) *reinterpret_cast<unsigned*>(sdst + 8 * p * kPitch2) = quant4_i8(xr[p], inv);
  __syncthreads();

  i32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c + 1 < NCH) {  // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
      for (int p = 0; p < PASS; ++p) xr[p] = *reinterpret_cast<const f32x4*>(xc + (c + 1) * kCC + xo[p]);
    }
#pragma unroll
    for (int tap = 0; tap < 3; ++tap) {
      const int q = 3 * c + tap;
      if (q + 1 < NQ) {  // W of the next tap (or of the next chunk's first): k-step (tap CIN + c kCC) / 32 + s
        const int c1 = (q + 1) / 3, tap1 = (q + 1) % 3, ks1 = (tap1 * CIN + c1 * kCC) / 32;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int s = 0; s < 2; ++s) w[(q + 1) & 1][j][s] = wp[j][(ks1 + s) * 64];
      }
      // input row 2 r + tap: even[r], odd[r], even[r + 1]
      const signed char* a = as[c & 1] + (tap == 1 ? kOdd2 : 0) + (wm * 64 + l31 + (tap == 2 ? 1 : 0)) * kPitch2 + 16 * lh;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const i32x4 a0 = *reinterpret_cast<const i32x4*>(a + s * 32);
        const i32x4 a1 = *reinterpret_cast<const i32x4*>(a + 32 * kPitch2 + s * 32);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[0][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, w[q & 1][j][s], acc[0][j], 0, 0, 0);
          acc[1][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, w[q & 1][j][s], acc[1][j], 0, 0, 0);
        }
      }
    }
    if (c + 1 < NCH) {
      // buffer (c + 1) & 1 was last read in chunk c - 1, in front of the barrier that ended it
      signed char* const d = sdst + ((c + 1) & 1) * kBuf2;
#pragma unroll
      for (int p = 0; p < PASS; ++p)
        if (p + 1 < PASS || sr == 0) *reinterpret_cast<unsigned*>(d + 8 * p * kPitch2) = quant4_i8(xr[p], inv);
      __syncthreads();
    }
  }
  conv_epilogue<EPI>(g, acc, b, t0, n0, sx, red);
}

template <int EPI>
void launch_conv(const EncConvDev& g, int stride, int C_in, int B, hipStream_t s) {
  const dim3 grid(g.N / kTile, (g.T_out + kTile - 1) / kTile, B);  // column tiles fastest: they share the input rows in L2
#define WT_CONV(KERNEL, CIN) hipLaunchKernelGGL((KERNEL<CIN, EPI>), grid, dim3(256), 0, s, g)
  if (stride == 1) {
    if (C_in == 80) WT_CONV(enc_conv1_i8, 80);
    else WT_CONV(enc_conv1_i8, 128);
  } else {
    if (C_in == 128) WT_CONV(enc_conv2_i8, 128);
    else if (C_in == 384) WT_CONV(enc_conv2_i8, 384);
    else WT_CONV(enc_conv2_i8, 512);
  }
#undef WT_CONV
}

}  // namespace

void launch_clip_absmax_f32(const float* x, int B, long n, float* amax, int n_zero, hipStream_t s) {
  if (!x || !amax || B < 1 || B > 65535 || n_zero < B || n < 4 || n % 4 != 0 || n / 4 >= (1ll << 32)) {
    throw Error(kErrInvalidArg, "clip maximum: x and amax, 1 <= B <= 65535, n_zero >= B, n a positive multiple of 4 below 2^34");
  }
  hipLaunchKernelGGL(zero_words, dim3((n_zero + 63) / 64), dim3(64), 0, s, reinterpret_cast<unsigned*>(amax), n_zero);
  const long per_block = 256 * 4 * 8;  // eight 16-byte loads per lane
  const unsigned blocks = (unsigned)std::min<long>((n + per_block - 1) / per_block, 64);
  hipLaunchKernelGGL(clip_absmax_f32, dim3(blocks, B), dim3(256), 0, s, reinterpret_cast<const f32x4*>(x), (unsigned)(n / 4), amax);
}

void check_enc_conv_i8(const EncConvI8Args& a, int epi) {
  if (a.stride == 1) {
    if (a.C_in != 80 && a.C_in != 128) throw Error(kErrInvalidArg, "int8 encoder conv: stride 1 takes C_in 80 or 128");
  } else if (a.stride == 2) {
    if (a.C_in != 128 && a.C_in != 384 && a.C_in != 512) throw Error(kErrInvalidArg, "int8 encoder conv: stride 2 takes C_in 128, 384 or 512");
  } else {
    throw Error(kErrInvalidArg, "int8 encoder conv: stride 1 or 2");
  }
  if (a.N < kTile || a.N % kTile != 0) throw Error(kErrInvalidArg, "int8 encoder conv: N must be a positive multiple of 128");
  if (a.B < 1 || a.T_out < 1) throw Error(kErrInvalidArg, "int8 encoder conv: B >= 1 and T_out >= 1");
  if (a.T_in != a.stride * a.T_out) throw Error(kErrInvalidArg, "int8 encoder conv: T_in must be stride x T_out");
  if (!a.X || !a.amax || !a.Wq || !a.sw || !a.bias || !a.Y) throw Error(kErrInvalidArg, "int8 encoder conv: null operand");
  if (epi != kConvBias && epi != kConvGelu && epi != kConvGeluPos) throw Error(kErrInvalidArg, "int8 encoder conv: unknown epilogue");
  if (epi == kConvGeluPos && !a.pos) throw Error(kErrInvalidArg, "int8 encoder conv: the positional epilogue needs pos");
  if (a.y_bs < (long long)a.T_out * a.N) throw Error(kErrInvalidArg, "int8 encoder conv: a clip's output stride below T_out x N");
  // the padded row counts: the grid's last tile forms its row bases before it masks them
  const long long rows = (long long)(a.T_out + kTile - 1) / kTile * kTile, lim = 1ll << 32;
  if (rows * a.N * 4 >= lim || (a.stride * rows + 2) * a.C_in * 4 >= lim || (long long)a.N * 3 * a.C_in >= lim || rows / kTile > 65535 ||
      a.B > 65535) {
    throw Error(kErrInvalidArg, "int8 encoder conv: an operand's byte offsets leave 32 bits");
  }
}

void launch_enc_conv_i8(const EncConvI8Args& a, int epi, hipStream_t s) {
  check_enc_conv_i8(a, epi);
  const EncConvDev g{a.X, a.amax, reinterpret_cast<const i32x4*>(a.Wq), a.sw, a.bias, epi == kConvGeluPos ? a.pos : a.Y, a.Y,
                     (long)a.y_bs, a.amax_out, a.T_in, a.T_out, a.N};
  if (epi == kConvBias) {
    launch_conv<kConvBias>(g, a.stride, a.C_in, a.B, s);
  } else if (epi == kConvGelu) {
    launch_conv<kConvGelu>(g, a.stride, a.C_in, a.B, s);
  } else {
    launch_conv<kConvGeluPos>(g, a.stride, a.C_in, a.B, s);
  }
}

}  // namespace wt
