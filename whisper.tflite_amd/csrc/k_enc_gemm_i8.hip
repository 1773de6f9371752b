// The int8 dynamic-range encoder-block GEMM for gfx950 (option "encoder_int8"): the four Linear
// matrices of an encoder layer (q|k|v, attention out, fc1, fc2) over M = 1500 x clips rows, in the arithmetic of
// DESIGN sections 37 / 38: W as int8 rows + one fp32 scale per output (quantize_rows_i8, tile_rows_i8), every A row
// quantised over the WHOLE K by TFLite's SymmetricQuantizeFloats (dec_rows.h: row_scale_i8 / quant_i8), int32 sums on
// v_mfma_i32_32x32x32_i8, and
//   t = ((float)acc * sx[m]) * sw[n];  bias: t + b;  GELU: gelu_erf(t + b);  residual: R + (t + b)
// every product and sum rounded on its own (-ffp-contract=fast-honor-pragmas, the epilogue under contract(off)).
//
// Two kernels, because a row's scale needs the whole row and the GEMM that produces the row only ever sees one column
// tile of it:
//   * enc_quant_rows_i8 / enc_quant_ln_rows_i8: activation rows -> qx int8 [M][K] row-major + sx fp32 [M], one launch
//     per contraction.  Sources: fp32 rows, two fp16 planes with their power-of-two scale (what
//     encoder_attention_planes writes), or the LayerNorm of fp32 rows.  A row is read ONCE and lives in registers
//     between the max pass and the quantise pass: 8 lanes per row up to K = 512 (at most 64 floats per lane), 32 lanes
//     per row above (K = 2048: 64 floats per lane; 8 lanes would need 256 registers).  A lane owns whole 16-element
//     pieces sub, sub + LPR, ..: 64 source bytes in 16-byte loads, one 16-byte store of qx.  The LayerNorm source keeps
//     the decoder kernels' mapping and code (dec_rows.h load_row / row_stats / ln_apply_max: 4-element columns per
//     lane) and turns its 4-byte words into 16-byte pieces through LDS.
//   * enc_gemm_i8<KS, EPI>: 256 threads = 2 x 2 wavefronts on a 128 x 128 tile, each wavefront 64 x 64 as 2 x 2
//     accumulators of the 32x32x32 MFMA (64 accumulator registers).  K is streamed in chunks of 128 bytes: the A
//     chunk [128 rows][128] goes global -> registers -> LDS (row pitch 144: the fragment read of row l & 31 at byte
//     16 (l >> 5) is conflict-free), two buffers, the next chunk's global loads issued before the current chunk's 16
//     MFMAs and stored behind them, one barrier per chunk.  W fragments come straight from global memory in
//     tile_rows_i8's order (1 KiB contiguous per wave-instruction, the same lines for the two wavefronts of a column
//     half and for every row tile: L2), one chunk ahead in registers.  Column tiles run fastest in the grid, so the
//     blocks that share a row panel of qx run together.  sx of the tile's rows is parked in LDS once, sw and bias of
//     a lane's two columns in registers.
// Every index that guards a load is clamped (rows past M re-read row M - 1 and are never stored), every trip count is
// a template constant, stores use a wave-uniform row base plus a 32-bit lane offset.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dec_rows.h"
#include "kernels.h"

namespace wt {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

// ------------------------------------------------------------------------------------------------ the quantiser ---
struct EncQuantDev {
  const float* X;  // fp32 rows [M][ld] (kEncSrcF32, kEncSrcLn: ld == K)
  int ld;
  const f16x8* hi;  // kEncSrcPlanes: [M][K] each
  const f16x8* lo;
  float inv_scale;
  const float* ln_g;
  const float* ln_b;
  int M, K;
  signed char* qx;
  float* sx;
};

// LPR lanes per row, NP 16-element pieces per lane (piece sub + LPR j; K / 16 pieces in the row, the rest masked)
template <int SRC, int LPR, int NP>
__global__ __launch_bounds__(256) void enc_quant_rows_i8(EncQuantDev g) {
  constexpr int RPB = 256 / LPR;
  const int tid = threadIdx.x, sub = tid % LPR, row = blockIdx.x * RPB + tid / LPR;
  const int rowc = row < g.M ? row : g.M - 1, np = g.K >> 4;
  f32x4 v[NP][4];
  float mx = 0.0f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = sub + LPR * j, pc = p < np ? p : np - 1;
    if (SRC == kEncSrcF32) {
      const f32x4* s = reinterpret_cast<const f32x4*>(g.X + (long)rowc * g.ld + pc * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[j][e] = s[e];
    } else {
      const long o = ((long)rowc * g.K + pc * 16) >> 3;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f16x8 a = g.hi[o + h], b = g.lo[o + h];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][2 * h + (e >> 2)][e & 3] = ((float)a[e] + (float)b[e]) * g.inv_scale;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    float m = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) m = fmaxf(m, fabsf(v[j][e >> 2][e & 3]));
    if (sub + LPR * j < np) mx = fmaxf(mx, m);
  }
  if (LPR == 32) {  // (row_scale_i8 joins the lanes of a group of 8)
    mx = fmaxf(mx, __shfl_xor(mx, 8, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  }
  float sx, inv;
  row_scale_i8(mx, &sx, &inv);
  if (row >= g.M) return;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = sub + LPR * j;
    const u32x4 q = {quant4_i8(v[j][0], inv), quant4_i8(v[j][1], inv), quant4_i8(v[j][2], inv), quant4_i8(v[j][3], inv)};
    if (p < np) *reinterpret_cast<u32x4*>(g.qx + (long)row * g.K + p * 16) = q;
  }
  if (sub == 0) g.sx[row] = sx;
}

// The LayerNorm source: the decoder kernels' row code, 8 lanes per row and 8 rows per wavefront, 32 rows per block
template <int KS>
__global__ __launch_bounds__(256) void enc_quant_ln_rows_i8(EncQuantDev g) {
  constexpr int K = KS * 32;
  __shared__ __attribute__((aligned(16))) float lnp[2 * K];
  __shared__ __attribute__((aligned(16))) signed char qs[32 * K];
  const int tid = threadIdx.x, lane = tid & 63, sub = lane & 7, lrow = (tid >> 6) * 8 + (lane >> 3);
  const int row = blockIdx.x * 32 + lrow, rowc = row < g.M ? row : g.M - 1;
  if (tid < K / 2) {
    *reinterpret_cast<f32x4*>(&lnp[tid * 4]) = *reinterpret_cast<const f32x4*>((tid < K / 4 ? g.ln_g : g.ln_b - K) + tid * 4);
  }
  const RowSrc src{g.X, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 0, nullptr, 0};
  f32x4 v[KS];
  load_row<KS, 0>(v, src, rowc, sub, K);
  __syncthreads();
  float mean, rstd, sx, inv;
  row_stats<KS>(v, K, &mean, &rstd);
  row_scale_i8(ln_apply_max<KS>(v, lnp, K, sub, mean, rstd), &sx, &inv);
#pragma unroll
  for (int j = 0; j < KS; ++j) *reinterpret_cast<unsigned*>(&qs[lrow * K + (sub + 8 * j) * 4]) = quant4_i8(v[j], inv);
  __syncthreads();
  if (row >= g.M) return;
#pragma unroll
  for (int j = 0; j < KS / 4; ++j) {  // K / 16 pieces per row
    const int c = (sub + 8 * j) * 16;
    *reinterpret_cast<u32x4*>(g.qx + (long)row * K + c) = *reinterpret_cast<const u32x4*>(&qs[lrow * K + c]);
  }
  if (sub == 0) g.sx[row] = sx;
}

template <int SRC>
void launch_quant(const EncQuantDev& g, hipStream_t s) {
  const int K = g.K;
#define WT_ENC_QUANT(LPR, NP) \
  hipLaunchKernelGGL((enc_quant_rows_i8<SRC, LPR, NP>), dim3((g.M + 256 / LPR - 1) / (256 / LPR)), dim3(256), 0, s, g)
  if (K <= 128) WT_ENC_QUANT(8, 1);
  else if (K <= 256) WT_ENC_QUANT(8, 2);
  else if (K <= 384) WT_ENC_QUANT(8, 3);
  else if (K <= 512) WT_ENC_QUANT(8, 4);
  else if (K <= 1024) WT_ENC_QUANT(32, 2);
  else if (K <= 1536) WT_ENC_QUANT(32, 3);
  else WT_ENC_QUANT(32, 4);
#undef WT_ENC_QUANT
}

// ------------------------------------------------------------------------------------------------------ the GEMM ---
struct EncGemmI8Dev {
  const signed char* qx;  // [M][K]
  const float* sx;        // [M]
  const i32x4* Wq;        // [N / 32][K / 32][64]
  const float* sw;        // [N]
  const float* bias;
  const float* R;
  float* Y;
  int M, ldc;
};

constexpr int kTile = 128;           // rows and columns of a block's tile
constexpr int kChunk = 128;          // bytes of K per LDS buffer: 4 k-steps
constexpr int kPitch = kChunk + 16;  // an odd multiple of 16 bytes

// KS = K / 32
template <int KS, int EPI>
__global__ __launch_bounds__(256) void enc_gemm_i8(EncGemmI8Dev g) {
  static_assert(KS % 4 == 0, "whole chunks of 4 k-steps");
  constexpr int K = KS * 32, NCH = KS / 4;
  __shared__ __attribute__((aligned(16))) signed char as[2][kTile * kPitch];
  __shared__ float sxs[kTile];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * kTile, m0 = blockIdx.y * kTile, M = g.M;
  // A: thread (row tid >> 3 (+ 32 p), 16-byte column tid & 7) of every chunk
  const int ar = tid >> 3, ac = (tid & 7) * 16;
  const signed char* ap[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int m = m0 + ar + 32 * p;
    ap[p] = g.qx + (long)(m < M ? m : M - 1) * K + ac;
  }
  // W: the wavefront's two 32-column tiles, k-step s of the launch at [s * 64]
  const i32x4* wp[2];
  int n[2];
  float swn[2], bn[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    n[j] = n0 + wn * 64 + j * 32 + l31;  // < N: N is a multiple of the tile
    wp[j] = g.Wq + (long)((n0 + wn * 64 + j * 32) >> 5) * KS * 64 + lane;
  }
  i32x4 areg[4], w[2][2][4];
#pragma unroll
  for (int p = 0; p < 4; ++p) areg[p] = *reinterpret_cast<const i32x4*>(ap[p]);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s) w[0][j][s] = wp[j][s * 64];
  if (tid < kTile) sxs[tid] = g.sx[m0 + tid < M ? m0 + tid : M - 1];
#pragma unroll
  for (int j = 0; j < 2; ++j) swn[j] = g.sw[n[j]], bn[j] = g.bias[n[j]];
#pragma unroll
  for (int p = 0; p < 4; ++p) *reinterpret_cast<i32x4*>(&as[0][(ar + 32 * p) * kPitch + ac]) = areg[p];
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
      for (int p = 0; p < 4; ++p) areg[p] = *reinterpret_cast<const i32x4*>(ap[p] + (c + 1) * kChunk);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) w[(c + 1) & 1][j][s] = wp[j][((c + 1) * 4 + s) * 64];
    }
    const signed char* a = as[c & 1] + (wm * 64 + l31) * kPitch + 16 * lh;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const i32x4 a0 = *reinterpret_cast<const i32x4*>(a + s * 32);
      const i32x4 a1 = *reinterpret_cast<const i32x4*>(a + 32 * kPitch + s * 32);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc[0][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, w[c & 1][j][s], acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, w[c & 1][j][s], acc[1][j], 0, 0, 0);
      }
    }
    if (c + 1 < NCH) {
      // buffer (c + 1) & 1 was last read in chunk c - 1, in front of the barrier that ended it
#pragma unroll
      for (int p = 0; p < 4; ++p) *reinterpret_cast<i32x4*>(&as[(c + 1) & 1][(ar + 32 * p) * kPitch + ac]) = areg[p];
      __syncthreads();
    }
  }

#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma clang fp contract(off)
      const int lr = wm * 64 + i * 32 + crow(r, 0), mr = m0 + lr;  // the row is mr + 4 lh = m0 + .. crow(r, lh)
      const float sxm = sxs[lr + 4 * lh];
      if (mr + 4 * lh < M) {
        float* const yp = g.Y + (long)mr * g.ldc;
        const float* const rp = g.R + (long)mr * g.ldc;  // (never read without kDecResid)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const unsigned off = (unsigned)(4 * lh * g.ldc + n[j]);
          // plain operators: the pragma is lexical
          const float t = ((float)acc[i][j][r] * sxm) * swn[j];  // this order: (acc * sx) * sw
          float v = t + bn[j];
          if (EPI == kDecBiasGelu) v = gelu_erf(v);
          if (EPI == kDecResid) v = rp[off] + v;  // R + (t + bias); R may alias Y: read and written by the same lane
          yp[off] = v;
        }
      }
    }
  }
}

template <int EPI>
void launch_gemm(const EncGemmI8Dev& g, int N, int K, hipStream_t s) {
  const dim3 grid(N / kTile, (g.M + kTile - 1) / kTile);  // column tiles fastest: a row panel of qx is shared through L2
  switch (K) {
    case 128: hipLaunchKernelGGL((enc_gemm_i8<4, EPI>), grid, dim3(256), 0, s, g); break;
    case 384: hipLaunchKernelGGL((enc_gemm_i8<12, EPI>), grid, dim3(256), 0, s, g); break;
    case 512: hipLaunchKernelGGL((enc_gemm_i8<16, EPI>), grid, dim3(256), 0, s, g); break;
    case 1536: hipLaunchKernelGGL((enc_gemm_i8<48, EPI>), grid, dim3(256), 0, s, g); break;
    default: hipLaunchKernelGGL((enc_gemm_i8<64, EPI>), grid, dim3(256), 0, s, g); break;
  }
}

}  // namespace

void check_enc_gemm_i8(const EncGemmI8Args& a, int epi) {
  const bool k_ok = a.K == 128 || a.K == 384 || a.K == 512 || a.K == 1536 || a.K == 2048;
  if (!k_ok) throw Error(kErrInvalidArg, "int8 encoder GEMM: K must be 128, 384, 512, 1536 or 2048");
  if (a.M < 1) throw Error(kErrInvalidArg, "int8 encoder GEMM: M >= 1");
  if (a.N < kTile || a.N % kTile != 0) throw Error(kErrInvalidArg, "int8 encoder GEMM: N must be a positive multiple of 128");
  if (a.ldc < a.N) throw Error(kErrInvalidArg, "int8 encoder GEMM: ldc >= N");
  if (!a.qx || !a.sx || !a.Wq || !a.sw || !a.bias || !a.Y) throw Error(kErrInvalidArg, "int8 encoder GEMM: null operand");
  if (epi != kDecResid && epi != kDecBias && epi != kDecBiasGelu) throw Error(kErrInvalidArg, "int8 encoder GEMM: unknown epilogue");
  if (epi == kDecResid && !a.R) throw Error(kErrInvalidArg, "int8 encoder GEMM: the residual epilogue needs R");
  // the padded row count: the grid's last tile forms its row bases before it masks them
  const long long rows = (long long)(a.M + kTile - 1) / kTile * kTile, lim = 1ll << 32;
  if (rows * a.ldc * 4 >= lim || rows * a.K >= lim || (long long)a.N * a.K >= lim || rows / kTile > 65535) {
    throw Error(kErrInvalidArg, "int8 encoder GEMM: an operand's byte offsets leave 32 bits");
  }
}

void launch_enc_gemm_i8(const EncGemmI8Args& a, int epi, hipStream_t s) {
  check_enc_gemm_i8(a, epi);
  const EncGemmI8Dev g{reinterpret_cast<const signed char*>(a.qx), a.sx, reinterpret_cast<const i32x4*>(a.Wq), a.sw, a.bias,
                       epi == kDecResid ? a.R : a.Y, a.Y, a.M, a.ldc};
  if (epi == kDecResid) {
    launch_gemm<kDecResid>(g, a.N, a.K, s);
  } else if (epi == kDecBias) {
    launch_gemm<kDecBias>(g, a.N, a.K, s);
  } else {
    launch_gemm<kDecBiasGelu>(g, a.N, a.K, s);
  }
}

void launch_enc_quant_rows_i8(const EncQuantI8Args& a, int src, hipStream_t s) {
  if (a.K < 16 || a.K % 16 != 0 || a.K > 2048) throw Error(kErrInvalidArg, "int8 row quantiser: K a multiple of 16 up to 2048");
  if (a.M < 1 || !a.qx || !a.sx) throw Error(kErrInvalidArg, "int8 row quantiser: M >= 1, qx and sx");
  EncQuantDev g{a.X, a.ld, reinterpret_cast<const f16x8*>(a.hi), reinterpret_cast<const f16x8*>(a.lo),
                a.scale != 0.0f ? 1.0f / a.scale : 0.0f, a.ln_g, a.ln_b, a.M, a.K, reinterpret_cast<signed char*>(a.qx), a.sx};
  if (src == kEncSrcF32) {
    if (!a.X || a.ld < a.K || a.ld % 4 != 0) throw Error(kErrInvalidArg, "int8 row quantiser: X [M][ld >= K], ld a multiple of 4");
    launch_quant<kEncSrcF32>(g, s);
  } else if (src == kEncSrcPlanes) {
    if (!a.hi || !a.lo || !(a.scale > 0.0f)) throw Error(kErrInvalidArg, "int8 row quantiser: both planes and their scale");
    launch_quant<kEncSrcPlanes>(g, s);
  } else if (src == kEncSrcLn) {
    if (a.K > 512) throw Error(kErrInvalidArg, "int8 row quantiser: the LayerNorm source takes K up to 512");
    if (!a.X || !a.ln_g || !a.ln_b) throw Error(kErrInvalidArg, "int8 row quantiser: X, gain and shift");
    const dim3 grid((a.M + 31) / 32);
    switch (a.K) {
      case 128: hipLaunchKernelGGL((enc_quant_ln_rows_i8<4>), grid, dim3(256), 0, s, g); break;
      case 384: hipLaunchKernelGGL((enc_quant_ln_rows_i8<12>), grid, dim3(256), 0, s, g); break;
      case 512: hipLaunchKernelGGL((enc_quant_ln_rows_i8<16>), grid, dim3(256), 0, s, g); break;
      default: throw Error(kErrInvalidArg, "int8 row quantiser: the LayerNorm source takes d_model 128, 384 or 512");
    }
  } else {
    throw Error(kErrInvalidArg, "int8 row quantiser: unknown source");
  }
}

}  // namespace wt
