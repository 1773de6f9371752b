// The int8 dynamic-range decoder-block GEMM for gfx950 (option "decoder_int8"):
//   out[M][N] = epi( q(pro(x))[M][K] . Wq[N][K]^T )
// in the arithmetic of a dynamic-range quantised TFLite graph: W as int8 rows + one fp32 scale per output column
// (wt_quantize_rows_i8, wt_tile_rows_i8, made once on the host), every A row quantised at every launch by TFLite's
// SymmetricQuantizeFloats over the WHOLE K (dec_rows.h: row_scale_i8 / quant_i8), int32 accumulation on
// v_mfma_i32_32x32x32_i8, and
//   t = ((float)acc * sx[m]) * sw[n];  bias: t + b;  GELU: gelu_erf(t + b);  residual: R + (t + b)
// with every product and sum rounded on its own (this file is compiled with -ffp-contract=fast-honor-pragmas and the
// epilogue sits under contract(off)).
//
// A row's scale needs the whole row before its first product, so dec_gemm's per-(row, k-slice) scales and its "split K
// first, think later" shape (k_decoder.hip) do not carry over.  One block = one 32-column tile, 4 wavefronts, two phases:
//   * the block's weight stream goes in flight first: wavefront w owns the k-steps [w K/128, (w + 1) K/128) of the tile
//     (K / 128 x 16 bytes per lane: 1 register quad at K = 128, 16 at K = 2048), loaded ONCE per launch and kept over
//     all row groups; with it the column's bias and scale, and the LayerNorm gain | shift (parked in LDS);
//   * PHASE 1, per group of 32 rows: the four wavefronts form and quantise the rows once, 8 lanes per row and 8 rows per
//     wavefront (the mapping of dec_rows.h).  kProLn: load_row / row_stats / ln_apply_max, the row lives in registers
//     (K <= 512).  kProNone: K up to 2048 does not fit registers beside the weights, so the row is read in chunks of
//     16 x 16 bytes per lane: a max pass, then a quantise pass that re-reads X (at most 1 MB, written by the launch
//     before: L2) — at K <= 512 one chunk, read once.  The int8 panel [32][K + 16] and the 32 scales go to LDS;
//   * PHASE 2: the wavefronts split K; each reads its A fragments from the panel (16 bytes per lane per k-step, row
//     pitch K + 16: an odd multiple of 16 bytes, conflict-free) and runs one MFMA chain.  The int32 partials meet in
//     LDS and every wavefront finishes 4 of the 16 accumulator registers (8 rows).  The sum is exact, so no bit
//     depends on the split or the order;
//   * two barriers per group: the partials have their own LDS (16 KB) instead of aliasing the panel, and the scales of
//     the rows a wavefront finishes are taken to registers before the second one, so a wavefront may start the next
//     group's phase 1 while the others still reduce;
//   * every load index is clamped (rows past M re-read row M - 1 and are never stored) and every trip count that
//     guards a load is a template constant (k_decoder.hip's header); stores use a wave-uniform row base plus a 32-bit
//     lane offset (DESIGN section 37's spill finding).
// No K split over blocks (ksplit): at 1 byte per element a K = 1536 launch on 12 tiles streams 48 KB per block, less
// than the split fp16-plane form's 96 KB.  kProCombine stays on dec_gemm.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dec_rows.h"
#include "kernels.h"

namespace wt {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

struct DecGemmI8Dev {
  const i32x4* Wq;  // [N / 32][K / 32][64]
  const float* sw;  // [N]
  int N, M;
  const float* X;
  int ldx;
  RowSrc src;  // kProLn
  float* xout;
  const float* ln_g;
  const float* ln_b;
  const float* bias;
  int gelu;
  const float* R;
  float* Y;
  int ldy;
  signed char* qx_out;
  float* sx_out;
};

constexpr int kRedInts = 4 * 16 * 64;  // split-K partials [wavefront][register][lane]
constexpr size_t dec_i8_smem(int K, bool ln) {
  return size_t(32) * (K + 16) + kRedInts * sizeof(int) + 32 * sizeof(float) + (ln ? size_t(2) * K * sizeof(float) : 0);
}

// KS = K / 32 (k-steps of the tile, and 16-byte columns a lane owns of its row); LNMODE as load_row's (kProLn only)
template <int KS, int PRO, int LNMODE, int EPI>
__global__ __launch_bounds__(256) void dec_gemm_i8(DecGemmI8Dev g) {
  static_assert(KS % 4 == 0 && (PRO == kProNone || KS <= 16), "K = 128 steps per wavefront; LayerNorm rows live in registers");
  constexpr int K = KS * 32, QLD = K + 16, KW = KS / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_i8[];
  signed char* const qs = reinterpret_cast<signed char*>(smem_i8);  // [32][QLD]
  int* const red = reinterpret_cast<int*>(smem_i8 + 32 * QLD);      // [4][16][64]
  float* const sxs = reinterpret_cast<float*>(red + kRedInts);      // [32]
  float* const lnp = sxs + 32;                                      // [2][K] (kProLn)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int tile = blockIdx.x, M = g.M, m_tiles = (M + 31) >> 5;
  // this wavefront's weights for all row groups, in flight over the first group's phase 1
  i32x4 w[KW];
  {
    const i32x4* wp = g.Wq + ((long)tile * KS + wid * KW) * 64 + lane;
#pragma unroll
    for (int s = 0; s < KW; ++s) w[s] = wp[s * 64];
  }
  f32x4 lnreg = {0, 0, 0, 0};
  if (PRO == kProLn && tid < K / 2) lnreg = *reinterpret_cast<const f32x4*>((tid < K / 4 ? g.ln_g : g.ln_b - K) + tid * 4);
  const int n = tile * 32 + l31;  // < N: N is a multiple of 32
  const float bias = g.bias[n], swn = g.sw[n];
  const int r8 = lane >> 3, sub = lane & 7, lrow = wid * 8 + r8;

  for (int g0 = 0; g0 < m_tiles; ++g0) {
    const int m0 = g0 * 32, row = m0 + lrow, rowc = row < M ? row : M - 1;
    const bool tap = tile == 0 && row < M;
    // the residual elements this lane will finish do not depend on the product either
    float r_pre[4] = {0, 0, 0, 0};
    if (EPI == kDecResid) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int m = m0 + crow(wid * 4 + rr, lh);
        r_pre[rr] = g.R[(long)(m < M ? m : M - 1) * g.ldy + n];
      }
    }
    // ---- phase 1: the group's 32 rows, formed and quantised once ----
    float sx, inv;
    if (PRO == kProLn) {
      f32x4 v[KS];
      load_row<KS, LNMODE>(v, g.src, rowc, sub, K);
      if (g0 == 0) {
        if (tid < K / 2) *reinterpret_cast<f32x4*>(&lnp[tid * 4]) = lnreg;
        __syncthreads();
      }
      if ((LNMODE == 2 || LNMODE == 3) && tile == 0 && g.xout != nullptr && row < M) {  // block 0 materialises the rows
#pragma unroll
        for (int j = 0; j < KS; ++j) *reinterpret_cast<f32x4*>(g.xout + (long)row * K + (sub + 8 * j) * 4) = v[j];
      }
      float mean, rstd;
      row_stats<KS>(v, K, &mean, &rstd);
      row_scale_i8(ln_apply_max<KS>(v, lnp, K, sub, mean, rstd), &sx, &inv);
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        const int c = (sub + 8 * j) * 4;
        const unsigned q4 = quant4_i8(v[j], inv);
        *reinterpret_cast<unsigned*>(&qs[lrow * QLD + c]) = q4;
        if (tap && g.qx_out) *reinterpret_cast<unsigned*>(g.qx_out + (long)row * K + c) = q4;
      }
    } else {
      constexpr int CH = KS < 16 ? KS : 16, NCH = KS / CH;  // chunks of CH x 16 bytes per lane = CH * 32 columns
      const float* xr = g.X + (long)rowc * g.ldx + sub * 4;
      f32x4 v[CH];
      float mx = 0.0f;
#pragma unroll 1
      for (int c0 = 0; c0 < NCH; ++c0) {
#pragma unroll
        for (int j = 0; j < CH; ++j) v[j] = *reinterpret_cast<const f32x4*>(xr + (c0 * CH + j) * 32);
#pragma unroll
        for (int j = 0; j < CH; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fabsf(v[j][e]));
      }
      row_scale_i8(mx, &sx, &inv);
#pragma unroll 1
      for (int c0 = 0; c0 < NCH; ++c0) {
        if (NCH > 1) {  // (one chunk: the row is still in registers)
#pragma unroll
          for (int j = 0; j < CH; ++j) v[j] = *reinterpret_cast<const f32x4*>(xr + (c0 * CH + j) * 32);
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int c = (c0 * CH + j) * 32 + sub * 4;
          const unsigned q4 = quant4_i8(v[j], inv);
          *reinterpret_cast<unsigned*>(&qs[lrow * QLD + c]) = q4;
          if (tap && g.qx_out) *reinterpret_cast<unsigned*>(g.qx_out + (long)row * K + c) = q4;
        }
      }
    }
    if (sub == 0) {
      sxs[lrow] = sx;
      if (tap && g.sx_out) g.sx_out[row] = sx;
    }
    __syncthreads();  // the panel and its scales are complete (and the previous group's partials are consumed)

    // ---- phase 2: K over the wavefronts; lane (row l31, half lh) of k-step s holds qx[row][32 s + 16 lh .. + 15] ----
    float rsx[4];  // accumulator register r belongs to row crow(r, lh); this wavefront finishes registers 4 wid .. + 3
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) rsx[rr] = sxs[crow(wid * 4 + rr, lh)];
    i32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
    for (int s = 0; s < KW; ++s) {
      const i32x4 a = *reinterpret_cast<const i32x4*>(&qs[l31 * QLD + 32 * (wid * KW + s) + 16 * lh]);
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, w[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(wid * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();  // every wavefront is done with the panel and the scales: the next group's phase 1 may overwrite them
    const unsigned yoff = (unsigned)(4 * lh * g.ldy + n);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
#pragma clang fp contract(off)
      const int r = wid * 4 + rr, mr = m0 + crow(r, 0);  // the row is mr + 4 lh = m0 + crow(r, lh)
      const int sum = (red[r * 64 + lane] + red[(16 + r) * 64 + lane]) + (red[(32 + r) * 64 + lane] + red[(48 + r) * 64 + lane]);
      // plain operators: the pragma is lexical (an operator inside an inlined __fadd_rn would keep its contract flag)
      const float t = ((float)sum * rsx[rr]) * swn;  // this order: (acc * sx) * sw
      float v = t + bias;
      if (EPI == kDecBias && g.gelu) v = gelu_erf(v);
      if (EPI == kDecResid) v = r_pre[rr] + v;  // R + (t + bias); R may alias Y: read and written by the same lane
      if (mr + 4 * lh < M) (g.Y + (long)mr * g.ldy)[yoff] = v;
    }
  }
}

template <int KS, int PRO, int LNMODE, int EPI>
void launch_one(const DecGemmI8Dev& g, hipStream_t s) {
  constexpr size_t smem = dec_i8_smem(KS * 32, PRO == kProLn);
  // dynamic LDS beyond the 64 KiB default (K = 2048: 81 KB) needs an opt-in, once per kernel
  static const bool raised = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_gemm_i8<KS, PRO, LNMODE, EPI>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL((dec_gemm_i8<KS, PRO, LNMODE, EPI>), dim3(g.N / 32), dim3(256), smem, s, g);
}

template <int LNMODE>
void launch_ln(const DecGemmI8Dev& g, int K, hipStream_t s) {
  switch (K) {
    case 128: launch_one<4, kProLn, LNMODE, kDecBias>(g, s); break;
    case 384: launch_one<12, kProLn, LNMODE, kDecBias>(g, s); break;
    case 512: launch_one<16, kProLn, LNMODE, kDecBias>(g, s); break;
    default: throw Error(kErrInvalidArg, "int8 decoder GEMM: the LayerNorm prologue takes d_model 128, 384 or 512");
  }
}

template <int EPI>
void launch_none(const DecGemmI8Dev& g, int K, hipStream_t s) {
  switch (K) {
    case 128: launch_one<4, kProNone, 0, EPI>(g, s); break;
    case 384: launch_one<12, kProNone, 0, EPI>(g, s); break;
    case 512: launch_one<16, kProNone, 0, EPI>(g, s); break;
    case 1536: launch_one<48, kProNone, 0, EPI>(g, s); break;
    default: launch_one<64, kProNone, 0, EPI>(g, s); break;
  }
}

}  // namespace

void launch_dec_gemm_i8(const DecGemmI8Args& a, int pro, int epi, hipStream_t s) {
  const bool k_ok = a.K == 128 || a.K == 384 || a.K == 512 || a.K == 1536 || a.K == 2048;
  if (!k_ok || a.M < 1 || a.M > 128 || a.N < 32 || a.N % 32 != 0 || a.ldy < a.N || a.ldy > (1 << 24) || a.ksplit != 1 ||
      pro == kProCombine || epi == kDecLogits || !a.Wq || !a.sw || !a.bias || !a.Y) {
    throw Error(kErrInvalidArg, "int8 decoder GEMM: shape, prologue / epilogue or operands outside the kernel contract");
  }
  if (epi != kDecResid && epi != kDecBias && epi != kDecBiasGelu) throw Error(kErrInvalidArg, "int8 decoder GEMM: unknown epilogue");
  if (epi == kDecResid && !a.R) throw Error(kErrInvalidArg, "int8 decoder GEMM: the residual epilogue needs R");
  const int B = a.B > 0 ? a.B : a.M;
  DecGemmI8Dev g{reinterpret_cast<const i32x4*>(a.Wq), a.sw, a.N, a.M, a.X, a.ldx,
                 RowSrc{a.xin, a.xpart, a.ids, a.ids_stride, a.pos, B, a.tok_emb, a.pos_emb, a.n_vocab, a.pos_start, a.n_ctx},
                 a.xout, a.ln_g, a.ln_b, a.bias, epi == kDecBiasGelu ? 1 : 0, a.R, a.Y, a.ldy,
                 reinterpret_cast<signed char*>(a.qx_out), a.sx_out};
  if (pro == kProNone) {
    if (!a.X || a.ldx < a.K || a.ldx % 4 != 0) throw Error(kErrInvalidArg, "int8 decoder GEMM: X [M][ldx >= K]");
    if (epi == kDecResid) {
      launch_none<kDecResid>(g, a.K, s);
    } else {
      launch_none<kDecBias>(g, a.K, s);
    }
    return;
  }
  if (pro != kProLn) throw Error(kErrInvalidArg, "int8 decoder GEMM: unknown prologue");
  if (epi == kDecResid || !a.ln_g || !a.ln_b || a.M % B != 0) {
    throw Error(kErrInvalidArg, "int8 decoder GEMM: the LayerNorm prologue pairs with the bias epilogues, M = positions x B");
  }
  if (a.ids) {  // the layer-0 token + positional embedding
    if (a.xpart || !a.tok_emb || !a.pos_emb || a.n_vocab < 1 || a.ids_stride < 1 || a.pos < 0 || (a.pos_start && a.n_ctx < 1)) {
      throw Error(kErrInvalidArg, "int8 decoder GEMM: embedding rows take ids and both tables, and have no pending partial");
    }
    launch_ln<2>(g, a.K, s);
  } else {
    if (!a.xin) throw Error(kErrInvalidArg, "int8 decoder GEMM: the LayerNorm prologue needs xin or ids");
    if (a.xpart) {
      launch_ln<3>(g, a.K, s);
    } else {
      launch_ln<0>(g, a.K, s);
    }
  }
}

}  // namespace wt
