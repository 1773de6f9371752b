// The int8 dynamic-range logits head for gfx950 (option "logits_int8"): logits[m][n] of the final
// LayerNorm rows against the tied embedding, with the embedding as int8 rows + one fp32 scale per vocabulary row
// (quantised once on the host, wt_quantize_rows_i8), the LayerNorm rows quantised per row at every launch, and int32
// accumulation on v_mfma_i32_32x32x32_i8:
//   y[m][n] = ((float)(sum_k qx[m][k] * qw[n][k]) * sx[m]) * sw[n]
// The sum is exact (|acc| <= 127 * 127 * 512 < 2^24), so the kernel has no order to keep and its work split is not the
// fp16-plane kernel's (dec_logits_persistent, k_decoder.hip):
//   * ONE WAVEFRONT PER COLUMN TILE over the whole K: a 32-column tile is K / 32 MFMAs (12 at K = 384) on one
//     accumulator — no split-K, no LDS reduction, no barrier inside the tile loop;
//   * the block (4 wavefronts) normalises and quantises its 32 rows ONCE, 8 lanes per row as the LayerNorm prologue of
//     dec_logits_persistent does (load_row / row_stats, the same fp32 code), the row maximum by shuffles; the int8 rows
//     and their scales go through LDS once, and every wavefront then keeps the A fragments of the full K in registers
//     (K / 32 x 4 VGPRs);
//   * the wavefronts of the grid walk the column tiles (tile = 4 blockIdx.x + wavefront, stride 4 gridDim.x); the next
//     tile's weights (K / 32 x 4 VGPRs, and its 32 column scales) are requested before the current tile's MFMAs, in
//     two register sets that swap roles (the loop is written out twice: no register copies);
//   * the table is in fragment order [tile][K / 32][64 lanes][16 bytes] (wt_tile_rows_i8): lane (l & 31, l >> 5) of
//     step s holds qw[32 tile + (l & 31)][32 s + 16 (l >> 5) .. + 15], one wave-instruction reads 1 KiB contiguous;
//   * every trip count that guards a load is a template constant or a clamped index (k_decoder.hip's header);
//   * the epilogue is the wavefront's own: scale back, the optional Y store, and the (value, column) record by the
//     ballot / __clz rule of dec_logits_persistent (largest ordered key, then the LARGEST column among equals).
// Up to four 32-row tiles go through blockIdx.y (M <= 128); each streams the table.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dec_rows.h"
#include "kernels.h"

namespace wt {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

struct LogitsI8Dev {
  const i32x4* Wq;  // [n_tiles][K / 32][64]
  const float* sw;  // [n_tiles * 32]
  int V, M;
  const float* xin;
  const float* xpart;
  const float* ln_g;
  const float* ln_b;
  float* Y;
  int ldy;
  unsigned long long* best;
  int best_stride;
  signed char* qx_out;
  float* sx_out;
};

template <int KS>
__device__ __forceinline__ void load_tile(i32x4 (&w)[KS], float* sw, const LogitsI8Dev& g, int tile, int lane) {
  const i32x4* p = g.Wq + (long)tile * (KS * 64) + lane;
#pragma unroll
  for (int s = 0; s < KS; ++s) w[s] = p[s * 64];
  *sw = g.sw[tile * 32 + (lane & 31)];
}

// one column tile of one wavefront: K / 32 MFMAs, then 16 accumulator registers = 32 rows x this lane's column
template <int KS>
__device__ __forceinline__ void finish_tile(const i32x4 (&a)[KS], const i32x4 (&w)[KS], float sw, const float (&rsx)[16],
                                            const LogitsI8Dev& g, int tile, int m0, int lane) {
  const int l31 = lane & 31, lh = lane >> 5;
  i32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
  for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], w[s], acc, 0, 0, 0);
  const int n = tile * 32 + l31;
  const bool n_ok = n < g.V;
  // addresses = a wave-uniform row base (scalar registers) + one 32-bit lane offset per tile: sixteen 64-bit lane
  // addresses per buffer, which do not change from tile to tile, would be kept in (and spilled from) vector registers
  const unsigned yoff = (unsigned)(4 * lh * g.ldy + n), boff = (unsigned)(4 * lh * g.best_stride + tile);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int mr = m0 + crow(r, 0), m = mr + 4 * lh;  // crow(r, lh)
    const float y = __fmul_rn(__fmul_rn((float)acc[r], rsx[r]), sw);  // this order: (acc * sx) * sw
    const bool ok = n_ok && m < g.M;
    if (ok && g.Y) (g.Y + (long)mr * g.ldy)[yoff] = y;
    const unsigned key = ok ? ordered_bits(y) : 0u;
    unsigned kmax = key;
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
      const unsigned o2 = __shfl_xor(kmax, off, 64);
      kmax = o2 > kmax ? o2 : kmax;
    }
    const unsigned long long hit = __ballot(ok && key == kmax);
    const unsigned half_hits = (unsigned)(hit >> (32 * lh));
    if (l31 == 0 && m < g.M) {
      const unsigned col = half_hits ? (unsigned)(tile * 32 + 31 - __clz(half_hits)) : 0u;
      (g.best + (long)mr * g.best_stride)[boff] = half_hits ? (((unsigned long long)kmax << 32) | col) : 0ull;
    }
  }
}

template <int KS, int LNMODE>  // KS = K / 32: 32-deep k-steps = MFMAs per tile = 16-byte chunks a lane owns of its row
__global__ __launch_bounds__(256, 2) void dec_logits_i8(LogitsI8Dev g) {
  constexpr int K = KS * 32, QLD = K + 16;  // LDS row pitch in bytes (16-byte aligned, off the 256-byte bank period)
  __shared__ __attribute__((aligned(16))) signed char qs[32 * QLD];
  __shared__ float sxs[32];
  __shared__ __attribute__((aligned(16))) float lnp[2 * K];  // the LayerNorm gain | shift
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int n_tiles = (g.V + 31) / 32, M = g.M;
  const int stride = 4 * (int)gridDim.x;
  int tile = 4 * (int)blockIdx.x + wid;
  // the first tile's weights do not depend on the rows: in flight over the whole prologue (a wavefront with no tile
  // re-reads the last one and never uses it)
  i32x4 w0[KS], w1[KS];
  float sw0, sw1;
  load_tile<KS>(w0, &sw0, g, tile < n_tiles ? tile : n_tiles - 1, lane);

  const int m0 = blockIdx.y * 32;
  {
    const int r8 = lane >> 3, sub = lane & 7, lrow = wid * 8 + r8, row = m0 + lrow;
    const RowSrc src{g.xin, g.xpart, nullptr, 0, 0, M, nullptr, nullptr, 0, nullptr, 0};
    // gain / shift are row-independent: one 16-byte load per thread, requested with the rows and parked in LDS while
    // those are in flight (holding them per lane beside the first tile's weights does not fit the register file)
    f32x4 lnreg = {0, 0, 0, 0};
    if (tid < K / 2) lnreg = *reinterpret_cast<const f32x4*>((tid < K / 4 ? g.ln_g : g.ln_b - K) + tid * 4);
    f32x4 v[KS];
    load_row<KS, LNMODE>(v, src, row < M ? row : M - 1, sub, K);
    if (tid < K / 2) *reinterpret_cast<f32x4*>(&lnp[tid * 4]) = lnreg;
    __syncthreads();
    float mean, rstd;
    row_stats<KS>(v, K, &mean, &rstd);
    float sx, inv;  // TFLite's SymmetricQuantizeFloats of the row (dec_rows.h)
    row_scale_i8(ln_apply_max<KS>(v, lnp, K, sub, mean, rstd), &sx, &inv);
    const bool tap = blockIdx.x == 0 && row < M;
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int c = (sub + 8 * j) * 4;
      const unsigned q4 = quant4_i8(v[j], inv);
      *reinterpret_cast<unsigned*>(&qs[lrow * QLD + c]) = q4;
      if (tap && g.qx_out) *reinterpret_cast<unsigned*>(g.qx_out + (long)row * K + c) = q4;
    }
    if (sub == 0) {
      sxs[lrow] = sx;
      if (tap && g.sx_out) g.sx_out[row] = sx;
    }
    __syncthreads();
  }
  // A fragments of the full K: lane (row l31, half lh) holds qx[row][32 s + 16 lh .. + 15]; accumulator register r
  // belongs to row crow(r, lh)
  i32x4 a[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) a[s] = *reinterpret_cast<const i32x4*>(&qs[l31 * QLD + 32 * s + 16 * lh]);
  float rsx[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) rsx[r] = sxs[crow(r, lh)];

  while (tile < n_tiles) {
    // the next tile's weights first (a tile past the end re-reads this one: no branch around a load)
    load_tile<KS>(w1, &sw1, g, tile + stride < n_tiles ? tile + stride : tile, lane);
    finish_tile<KS>(a, w0, sw0, rsx, g, tile, m0, lane);
    tile += stride;
    if (tile >= n_tiles) break;
    load_tile<KS>(w0, &sw0, g, tile + stride < n_tiles ? tile + stride : tile, lane);
    finish_tile<KS>(a, w1, sw1, rsx, g, tile, m0, lane);
    tile += stride;
  }
}

template <int LNMODE>
void launch_mode(const LogitsI8Dev& g, int K, dim3 grid, hipStream_t s) {
  switch (K) {
    case 128: hipLaunchKernelGGL((dec_logits_i8<4, LNMODE>), grid, dim3(256), 0, s, g); break;
    case 384: hipLaunchKernelGGL((dec_logits_i8<12, LNMODE>), grid, dim3(256), 0, s, g); break;
    default: hipLaunchKernelGGL((dec_logits_i8<16, LNMODE>), grid, dim3(256), 0, s, g); break;
  }
}

}  // namespace

void launch_dec_logits_i8(const DecLogitsI8Args& a, hipStream_t s) {
  const int n_tiles = (a.V + 31) / 32, m_tiles = (a.M + 31) / 32;
  const int best_stride = a.best_stride > 0 ? a.best_stride : n_tiles;
  if ((a.K != 128 && a.K != 384 && a.K != 512) || a.M < 1 || a.M > 128 || a.V < 1 || !a.Wq || !a.sw || !a.xin || !a.ln_g ||
      !a.ln_b || !a.best || best_stride < n_tiles || a.ldy < a.V || a.V > (1 << 24) || a.ldy > (1 << 24) || best_stride > (1 << 24)) {
    throw Error(kErrInvalidArg, "int8 logits head: shape or operands outside the kernel contract");
  }
  // `blocks` resident blocks in all, as the fp16-plane kernel counts them (0 = 512); a block's four wavefronts take
  // four column tiles at a time
  const int total = a.blocks >= 32 && a.blocks <= 1024 ? a.blocks : 512;
  const int per = total / m_tiles, want = (n_tiles + 3) / 4;
  const dim3 grid(want < per ? want : per, m_tiles);
  const LogitsI8Dev g{reinterpret_cast<const i32x4*>(a.Wq), a.sw, a.V, a.M, a.xin, a.xpart, a.ln_g, a.ln_b, a.Y, a.ldy,
                      a.best, best_stride, reinterpret_cast<signed char*>(a.qx_out), a.sx_out};
  if (a.xpart) {
    launch_mode<3>(g, a.K, grid, s);
  } else {
    launch_mode<0>(g, a.K, grid, s);
  }
}

}  // namespace wt
