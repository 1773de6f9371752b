// Row helpers shared by the decoder kernels (k_decoder.hip, k_logits_i8.hip, k_dec_gemm_i8.hip): the row sources of the
// residual stream, the LayerNorm statistics of a row spread over 8 lanes, the per-row int8 quantiser of the two int8
// kernels, and the ordering rules of the argmax records.
#pragma once
#include <hip/hip_runtime.h>

namespace wt {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ unsigned ordered_bits(float v) {
  v = v + 0.0f;  // -0.0 -> +0.0 so that equal values compare equal
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Row sources of the residual stream.  LNMODE 0: x = xin;  2: x = tok_emb[id] + pos_emb (row = p * B + b reads
// ids[b][pos + p] and positional row pos + p);  3: x = xin + xpart (the second K-half of the previous residual
// GEMM is still pending in xpart).
// pos_start (LNMODE 2, optional): `pos` counts slots and clip b's positional row is pos + p - pos_start[b], clamped into
// the table for the rows in front of a clip's position 0 and behind its cap (void rows: nothing reads what they make).
struct RowSrc {
  const float* xin;
  const float* xpart;
  const long long* ids;
  int ids_stride, pos, B;
  const float* tok_emb;
  const float* pos_emb;
  int n_vocab;
  const int* pos_start;
  int n_ctx;
};

// 8 lanes own one row (16-byte columns sub, sub + 8, ...); the NF4 loads of the row are
// independent and issued before the first use.
template <int NF4, int LNMODE>
__device__ __forceinline__ void load_row(f32x4 (&v)[NF4], const RowSrc& r, int row, int sub, int K) {
  const float* src = r.xin + (long)row * K;
  int p = 0;
  if (LNMODE == 2) {
    p = row / r.B;
    const int b = row - p * r.B;
    long long id = r.ids[(long)b * r.ids_stride + r.pos + p];
    id = id < 0 ? 0 : (id >= r.n_vocab ? r.n_vocab - 1 : id);  // never index outside the table
    src = r.tok_emb + id * K;
  }
#pragma unroll
  for (int j = 0; j < NF4; ++j) v[j] = *reinterpret_cast<const f32x4*>(src + (sub + 8 * j) * 4);
  if (LNMODE == 2) {
    int pr = r.pos + p;
    if (r.pos_start) {  // (uniform over the launch)
      const int st = min(max(r.pos_start[row - p * r.B], -(1 << 20)), 1 << 20);
      pr = min(max(pr - st, 0), r.n_ctx - 1);
    }
    const float* pe = r.pos_emb + (long)pr * K;
#pragma unroll
    for (int j = 0; j < NF4; ++j) v[j] += *reinterpret_cast<const f32x4*>(pe + (sub + 8 * j) * 4);
  }
  if (LNMODE == 3) {
    const float* pp = r.xpart + (long)row * K;
#pragma unroll
    for (int j = 0; j < NF4; ++j) v[j] += *reinterpret_cast<const f32x4*>(pp + (sub + 8 * j) * 4);
  }
}

// LayerNorm statistics of a row spread over 8 lanes (two-pass, eps 1e-5).
template <int NF4>
__device__ __forceinline__ void row_stats(const f32x4 (&v)[NF4], int K, float* mean, float* rstd) {
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < NF4; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  const float m = s / (float)K;
  float q = 0.0f;
#pragma unroll
  for (int j = 0; j < NF4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = v[j][e] - m;
      q += t * t;
    }
  q += __shfl_xor(q, 1, 64);
  q += __shfl_xor(q, 2, 64);
  q += __shfl_xor(q, 4, 64);
  *mean = m;
  *rstd = rsqrtf(q / (float)K + 1e-5f);
}

// The LayerNorm of a row held by 8 lanes, in place, from the gain | shift parked in LDS (lnp [2][K]); returns this lane's
// share of max |.| of the normalised row.
template <int NF4>
__device__ __forceinline__ float ln_apply_max(f32x4 (&v)[NF4], const float* lnp, int K, int sub, float mean, float rstd) {
  float mx = 0.0f;
#pragma unroll
  for (int j = 0; j < NF4; ++j) {
    const int c = (sub + 8 * j) * 4;
    const f32x4 gg = *reinterpret_cast<const f32x4*>(&lnp[c]);
    const f32x4 bb = *reinterpret_cast<const f32x4*>(&lnp[K + c]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[j][e] = (v[j][e] - mean) * rstd * gg[e] + bb[e];
      mx = fmaxf(mx, fabsf(v[j][e]));
    }
  }
  return mx;
}

// TFLite's SymmetricQuantizeFloats, the scales of a row whose 8 lanes each hold their share of max |a_k|: IEEE
// divisions, both results 0 for an all-zero row
__device__ __forceinline__ void row_scale_i8(float mx, float* sx, float* inv) {
  mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
  *sx = mx > 0.0f ? __fdiv_rn(mx, 127.0f) : 0.0f;
  *inv = mx > 0.0f ? __fdiv_rn(127.0f, mx) : 0.0f;
}
// ... and one element: the product is rounded once (never contracted into roundf's own arithmetic), half away from
// zero, then clamped to [-127, 127]
__device__ __forceinline__ unsigned quant_i8(float a, float inv) {
  const float r = fminf(fmaxf(roundf(__fmul_rn(a, inv)), -127.0f), 127.0f);
  return (unsigned)(int)r & 0xFFu;
}
__device__ __forceinline__ unsigned quant4_i8(const f32x4& v, float inv) {
  return quant_i8(v[0], inv) | (quant_i8(v[1], inv) << 8) | (quant_i8(v[2], inv) << 16) | (quant_i8(v[3], inv) << 24);
}

__device__ __forceinline__ float gelu_erf(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

}  // namespace
}  // namespace wt
