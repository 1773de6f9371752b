// Absorbed cross-attention on an int8 image of the encoder output (gfx950; option "cross_int8").
//
// k_cross_absorbed.hip sweeps the encoder output E once per decoder layer and position as two fp16 planes, 4 bytes per
// element (2 in the bf16 storage mode), and is bound by that stream.  Here E is stored once per encoded batch as int8
// rows with one fp32 scale per key row (quantize_e_rows_i8 below: section 37's per-row quantiser on the values the
// default kernel reconstructs from its planes), 1 byte per element, and the two products become
//   S^T[key][qc]  = (qe_tile . qq^T) sq[qc] se[key]     v_mfma_i32_16x16x64_i8, exact (127 . 127 . 512 < 2^24)
//   C^T[d][qc]   += qe_tile^T . W^T,  W = P . se          v_mfma_f32_16x16x32_f16: qe -> fp16 in registers (exact),
//                                                         W as two fp16 planes under a power-of-two launch scale
// with qq, sq the absorbed query column (position, head) quantised over its d_model elements in registers.
//
// Block = (clip, key chunk), four computing wavefronts and a loader.  The loader streams tiles of 32 keys global -> LDS
// by LDS-DMA into a ring of NST = 4 stages (a tile is 32 d bytes: 12 KB at d = 384, so three blocks share a CU's LDS).
// ONE image serves both products: [panel of 128 columns][32 keys][128 B], the 16-byte units of a row XORed with
//   sw(key) = ((key >> 1) & 7) ^ ((key >> 2) & 4),
// applied to the DMA's per-lane SOURCE address.  The score product's ds_read_b128 of 16 consecutive keys at one unit then
// covers all 16 units of a 256-byte bank row, and so do the 8 keys x 16 B x two lane groups of a ds_read_b64_tr_b8.
// With an int8 tile the whole score product is 2 d / 64 MFMAs, so EVERY computing wavefront forms all 32 x 16 scores
// itself: no partial scores through LDS and ONE barrier per tile (the parent kernel has two).  The wavefronts differ
// only in the quarter of the d range whose context they accumulate.  The transposed read hands lane i of a 16-lane group
// column i of the 8 key rows its lanes address — rows 4 lq .. 4 lq + 3 and 16 + 4 lq .. + 3, the keys whose scores the
// lane group holds in its accumulator registers, so P never moves between lanes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bf16_split.h"
#include "dec_rows.h"
#include "kernels.h"

namespace wt {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using half8 = __attribute__((ext_vector_type(8))) _Float16;
using half2 = __attribute__((ext_vector_type(2))) _Float16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

struct CrossAbsI8Dev {
  const float* qp;           // [rows][heads * DM] absorbed queries (log2 domain)
  const signed char* qe[4];  // clip b reads qe[b / split] at clip b % split: int8 rows [clips * T][DM]
  const float* se[4];        // ... and their scales [clips * T]
  int split;
  float w_scale;             // power of two on the planes of W = P . se
  float* ws;                 // [rows][heads][chunks][DM + 4]: c[DM], m (natural log units), l, pad
  int B, H, T, chunks, nq, p0, tiles_per_chunk;
};

constexpr float kDeferA = 3.0f;  // as in k_cross_absorbed.hip: the running maximum moves only past this margin

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)p;
}
__device__ __forceinline__ int sw_of(int key) { return ((key >> 1) & 7) ^ ((key >> 2) & 4); }

// Transposed 8-bit reads of TWO 16-column blocks and the wait for them in ONE asm statement (as a builtin the read
// would wait for the wavefront's global loads; as separate statements the results would count as landed at once).
// The results feed vector ALU conversions, never an MFMA directly.
__device__ __forceinline__ void ds_read_tr8_x2(unsigned a0, unsigned a1, u32x2& x, u32x2& y) {
  asm volatile(
      "ds_read_b64_tr_b8 %0, %2\n\t"
      "ds_read_b64_tr_b8 %1, %3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(x), "=&v"(y)
      : "v"(a0), "v"(a1)
      : "memory");
}

// dec_rows.h's quant4_i8 with every product pinned to ONE fp32 value first: this file is compiled with -ffp-contract=fast,
// under which hipcc fuses a * inv into roundf's own v - trunc(v), and a tie then rounds by the exact product instead of the
// fp32 one (x = max / 2 gives 63.5: one element in a thousand among bf16 values, measured against the numpy quantiser).
__device__ __forceinline__ unsigned quant4_pinned_i8(const f32x4& x, float inv) {
  f32x4 v = {x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv};
  asm volatile("" : "+v"(v));
  return quant4_i8(v, 1.0f);
}

// 8 int8 (two dwords) -> 8 fp16, exact: byte b ^ 0x80 under the exponent of 1024 is the fp16 value 1152 + q
__device__ __forceinline__ half8 i8x8_to_f16(u32x2 raw) {
  const unsigned lo = raw[0] ^ 0x80808080u, hi = raw[1] ^ 0x80808080u;
  const half2 bias = {(_Float16)1152.0f, (_Float16)1152.0f};
  const half2 h0 = __builtin_bit_cast(half2, __builtin_amdgcn_perm(0x64646464u, lo, 0x04010400u)) - bias;
  const half2 h1 = __builtin_bit_cast(half2, __builtin_amdgcn_perm(0x64646464u, lo, 0x04030402u)) - bias;
  const half2 h2 = __builtin_bit_cast(half2, __builtin_amdgcn_perm(0x64646464u, hi, 0x04010400u)) - bias;
  const half2 h3 = __builtin_bit_cast(half2, __builtin_amdgcn_perm(0x64646464u, hi, 0x04030402u)) - bias;
  return half8{h0[0], h0[1], h1[0], h1[1], h2[0], h2[1], h3[0], h3[1]};
}

template <int DM, int NST>
__global__ __launch_bounds__(320) void cross_absorbed_attention_i8(CrossAbsI8Dev a) {
  constexpr int kTile = 32 * DM;  // bytes of a 32-key tile: DM / 128 panels of 4 KiB
  constexpr int KS = DM / 64;     // 64-deep k-steps of the score product
  constexpr int DT = DM / 64;     // 16-wide d tiles per wavefront (context product)
  constexpr int IPT = DM / 32;    // LDS-DMA instructions per tile (1 KiB each: 8 keys x 128 B of one panel)
  static_assert(NST >= 2 && NST <= 4 && (NST - 2) * IPT <= 63, "the counted wait leaves NST - 2 whole tiles in flight");
  static_assert(DT % 2 == 0, "d tiles are read in pairs");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  const int b = blockIdx.x / a.chunks, ck = blockIdx.x % a.chunks;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qc = lane & 15, lq = lane >> 4;
  const int n_qc = a.nq * a.H;
  const bool q_ok = qc < n_qc;
  const int qpos = q_ok ? qc / a.H : 0, qh_i = q_ok ? qc % a.H : 0;
  const long row = (long)(a.p0 + qpos) * a.B + b;

  // ---- key range of this chunk, in tiles of 32
  const int key_lo = ck * a.tiles_per_chunk * 32;
  int key_hi = key_lo + a.tiles_per_chunk * 32;
  key_hi = key_hi < a.T ? key_hi : a.T;
  const int n_tiles = key_hi > key_lo ? (key_hi - key_lo + 31) / 32 : 0;

  const int eb = b / a.split;  // (block-uniform)
  const long clip_row0 = (long)(b - eb * a.split) * a.T;
  const signed char* const ebase = (eb == 0 ? a.qe[0] : eb == 1 ? a.qe[1] : eb == 2 ? a.qe[2] : a.qe[3]) + clip_row0 * DM;
  const float* const sbase = (eb == 0 ? a.se[0] : eb == 1 ? a.se[1] : eb == 2 ? a.se[2] : a.se[3]) + clip_row0;

  if (wid == 4) {
    // ---- the loader.  Instruction i of a tile copies 8 keys x 128 B: panel i / 4, key group kg = i % 4; LDS slot (key
    // row lane >> 3, unit lane & 7) takes the global unit (lane & 7) ^ sw(key) of that key row, and with key = 8 kg + r
    // sw is (r >> 1) + 4 ((kg & 1) ^ (kg >> 1)): two constant per-lane offsets, everything else a scalar base.  A tile
    // that reaches past the clip's last key row takes the per-lane form with the row index clamped.
    const int r8 = lane >> 3, u = lane & 7;
    const unsigned long long ebytes = reinterpret_cast<unsigned long long>(ebase);
    const unsigned lds_ring = lds_addr(lds);
    const unsigned voff0 = (unsigned)(r8 * DM + ((u ^ (r8 >> 1)) << 4));
    const unsigned voff1 = (unsigned)(r8 * DM + ((u ^ ((r8 >> 1) + 4)) << 4));
    auto dma_tile = [&](int t) {
      if (t >= n_tiles) return;
      const int stage = t % NST;
      if (key_lo + t * 32 + 32 <= a.T) {
        const unsigned long long tb = ebytes + (unsigned long long)(key_lo + t * 32) * DM;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
          const int panel = i / 4, kg = i % 4;
          lds_dma16_sgpr(((kg & 1) ^ (kg >> 1)) ? voff1 : voff0, tb + (unsigned)(8 * kg * DM + panel * 128),
                         lds_ring + (unsigned)(stage * kTile + panel * 4096 + kg * 1024));
        }
      } else {
        unsigned char* const sb = lds + stage * kTile;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
          const int panel = i / 4, kg = i % 4;
          const int key = 8 * kg + r8;
          int gk = key_lo + t * 32 + key;
          gk = gk < a.T ? gk : a.T - 1;  // keys past T re-read the last row; their scores are masked
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ebase + (long)gk * DM + panel * 128 + ((u ^ sw_of(key)) << 4)),
                                           (__attribute__((address_space(3))) void*)(sb + panel * 4096 + kg * 1024), 16, 0, 0);
        }
      }
    };
#pragma unroll
    for (int st0 = 0; st0 < NST - 1; ++st0) dma_tile(st0);
    for (int t = 0; t < n_tiles; ++t) {
      // "tile t has landed": the tiles issued behind it (at most NST - 2) stay in flight
      const int ahead = n_tiles - 1 - t < NST - 2 ? n_tiles - 1 - t : NST - 2;
      if (ahead >= 2) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * IPT) : "memory");
      } else if (ahead == 1) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();  // ... and every computing wavefront has finished tile t - 1, whose stage is refilled now
      dma_tile(t + NST - 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return;
  }

  // ---- the query column of this lane, quantised over its d_model elements (section 37's quantiser): the lane holds
  // elements 64 c + 16 lq .. + 15 of every k-step c, the column's four lanes share max |q'|.  Two passes over the same
  // addresses (the second from the cache) instead of d / 4 live registers per lane.
  i32x4 qq[KS];
  float sq;
  {
    const float* src = a.qp + row * (long)(a.H * DM) + qh_i * DM + 16 * lq;
    float mx = 0.0f;
#pragma unroll
    for (int c = 0; c < KS; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(src + 64 * c + 4 * v);
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3]))));
      }
    mx = q_ok ? mx : 0.0f;  // columns past nq * heads contribute zeros
    mx = xor32_max(xor16_max(mx));
    sq = mx > 0.0f ? __fdiv_rn(mx, 127.0f) : 0.0f;
    const float inv = mx > 0.0f ? __fdiv_rn(127.0f, mx) : 0.0f;
    asm volatile("" ::: "memory");  // the second pass loads again
#pragma unroll
    for (int c = 0; c < KS; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        f32x4 x = *reinterpret_cast<const f32x4*>(src + 64 * c + 4 * v);
        if (!q_ok) x = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        qq[c][v] = (int)quant4_pinned_i8(x, inv);
      }
  }

  f32x4 cacc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) cacc[t] = f32x4{0, 0, 0, 0};
  float m_run = -1e30f, l_run = 0.0f;

  // fragment address parts that do not depend on the tile
  const int sw0 = sw_of(qc), sw1 = sw_of(16 + qc);           // score A fragments: key rows qc and 16 + qc of the tile
  const int tr_r = (lane & 15) >> 1;                         // transposed read: this lane addresses row tr_r of 8 ...
  const int tr_key = tr_r < 4 ? 4 * lq + tr_r : 12 + 4 * lq + tr_r;  // ... = the keys of accumulator registers s0[0..3], s1[0..3]
  const int tr_sw = sw_of(tr_key);
  const unsigned tr_base = lds_addr(lds) + (unsigned)(tr_key * 128 + 8 * (lane & 1));

  // the scales of this lane's eight keys of a tile, loaded one tile ahead (indices clamped into the clip)
  auto load_se = [&](int t, float (&s)[8]) {
    const int k0 = key_lo + t * 32 + 4 * lq;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i0 = k0 + r, i1 = k0 + 16 + r;
      s[r] = sbase[i0 < a.T ? i0 : a.T - 1];
      s[4 + r] = sbase[i1 < a.T ? i1 : a.T - 1];
    }
  };
  float se_next[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (n_tiles > 0) load_se(0, se_next);

  for (int t = 0; t < n_tiles; ++t) {
    float se_cur[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) se_cur[r] = se_next[r];
    load_se(t + 1, se_next);
    // tile t has landed (the loader's counted wait, then this barrier)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    const unsigned char* const st = lds + (t % NST) * kTile;

    // -- all 32 x 16 scores of the tile, exact in int32
    i32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < KS; ++c) {
      const int unit = 4 * (c & 1) + lq;
      const i32x4 e0 = *reinterpret_cast<const i32x4*>(st + (c >> 1) * 4096 + qc * 128 + ((unit ^ sw0) << 4));
      const i32x4 e1 = *reinterpret_cast<const i32x4*>(st + (c >> 1) * 4096 + (16 + qc) * 128 + ((unit ^ sw1) << 4));
      a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(e0, qq[c], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(e1, qq[c], a1, 0, 0, 0);
    }
    // accumulator register r of this lane: keys 4 lq + r and 16 + 4 lq + r of the tile, query column qc
    float s0[4], s1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s0[r] = (float)a0[r] * (sq * se_cur[r]);
      s1[r] = (float)a1[r] * (sq * se_cur[4 + r]);
    }
    const int kbase = key_lo + t * 32 + 4 * lq;
    if (kbase + 32 > key_hi) {  // the chunk's last tile: keys past its end do not exist (-inf whatever their scale is)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (kbase + r >= key_hi) s0[r] = -__builtin_inff();
        if (kbase + 16 + r >= key_hi) s1[r] = -__builtin_inff();
      }
    }
    // -- online softmax per query column (lanes qc, qc + 16, qc + 32, qc + 48), deferred maximum
    float tmax = fmaxf(fmaxf(fmaxf(s0[0], s0[1]), fmaxf(s0[2], s0[3])), fmaxf(fmaxf(s1[0], s1[1]), fmaxf(s1[2], s1[3])));
    tmax = xor32_max(xor16_max(tmax));
    if (__any(tmax > m_run + kDeferA)) {
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int d = 0; d < DT; ++d) cacc[d] *= alpha;
      m_run = m_new;
    }
    float psum = 0.0f;
    float w8[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p0 = __builtin_amdgcn_exp2f(s0[r] - m_run), p1 = __builtin_amdgcn_exp2f(s1[r] - m_run);
      psum += p0 + p1;
      w8[r] = p0 * (se_cur[r] * a.w_scale);  // W = P . se: the context runs on the int8 values themselves
      w8[4 + r] = p1 * (se_cur[4 + r] * a.w_scale);
    }
    psum = xor32_sum(xor16_sum(psum));
    l_run += psum;
    u32x4 wh, wl;
    split_f16x8_mfma(w8, wh, wl);  // the form whose outputs an MFMA may read at once (bf16_split.h)
    const half8 wH = __builtin_bit_cast(half8, wh);
    const half8 wL = __builtin_bit_cast(half8, wl);

    // -- context: this wavefront's DT d tiles; qe^T fragments by transposed reads, keys in the order of W^T
    const unsigned sa = tr_base + (unsigned)((t % NST) * kTile);
#pragma unroll
    for (int d = 0; d < DT; d += 2) {
      const int g0 = wid * DT + d, g1 = g0 + 1;  // 16-column blocks of the row
      u32x2 r0, r1;
      ds_read_tr8_x2(sa + (unsigned)((g0 >> 3) * 4096 + (((g0 & 7) ^ tr_sw) << 4)),
                     sa + (unsigned)((g1 >> 3) * 4096 + (((g1 & 7) ^ tr_sw) << 4)), r0, r1);
      const half8 e0 = i8x8_to_f16(r0), e1 = i8x8_to_f16(r1);
      cacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(e0, wL, cacc[d], 0, 0, 0);
      cacc[d + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(e1, wL, cacc[d + 1], 0, 0, 0);
      cacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(e0, wH, cacc[d], 0, 0, 0);
      cacc[d + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(e1, wH, cacc[d + 1], 0, 0, 0);
    }
  }

  // ---- record of this (row, head, chunk): c = sum p e (relative to the chunk's maximum), m, l
  if (q_ok) {
    const float cs = 1.0f / a.w_scale;
    float* rec = a.ws + ((row * a.H + qh_i) * a.chunks + ck) * (long)(DM + 4);
#pragma unroll
    for (int d = 0; d < DT; ++d) *reinterpret_cast<f32x4*>(rec + 16 * (wid * DT + d) + 4 * lq) = cacc[d] * cs;
    if (wid == 0 && lq == 0) {
      rec[DM] = m_run * 0.69314718055994530942f;  // natural-log units, like the parent's records
      rec[DM + 1] = l_run;
    }
  }
}

// E rows -> int8 rows + scales.  8 lanes own a row (16-byte units sub, sub + 8, ...): x = (hi + lo) / e_scale from the two
// fp16 planes (the value the default kernel reconstructs), or the bf16 value; then row_scale_i8 / quant_i8.
template <int DM, bool BF>
__global__ __launch_bounds__(256) void quantize_e_rows_i8(const unsigned short* __restrict__ e, long e_plane, float e_inv,
                                                          long rows, signed char* __restrict__ qe, float* __restrict__ se) {
  constexpr int NU = DM / 64;  // units of 8 elements per lane
  const int sub = threadIdx.x & 7;
  const long r = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const long rr = r < rows ? r : rows - 1;  // (all 8 lanes of a row alike: they stay together for the shuffles)
  float x[NU][8];
  float mx = 0.0f;
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    const long at = rr * DM + (sub + 8 * j) * 8;
    const u32x4 h = *reinterpret_cast<const u32x4*>(e + at);
    if constexpr (BF) {
#pragma unroll
      for (int k = 0; k < 4; ++k) x[j][2 * k] = bf16_lo(h[k]), x[j][2 * k + 1] = bf16_hi(h[k]);
    } else {
      const half8 hi = __builtin_bit_cast(half8, h);
      const half8 lo = __builtin_bit_cast(half8, *reinterpret_cast<const u32x4*>(e + e_plane + at));
#pragma unroll
      for (int k = 0; k < 8; ++k) x[j][k] = __fmul_rn(__fadd_rn((float)hi[k], (float)lo[k]), e_inv);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) mx = fmaxf(mx, fabsf(x[j][k]));
  }
  float sx, inv;
  row_scale_i8(mx, &sx, &inv);
  if (r >= rows) return;
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    const f32x4 lo4 = {x[j][0], x[j][1], x[j][2], x[j][3]}, hi4 = {x[j][4], x[j][5], x[j][6], x[j][7]};
    *reinterpret_cast<u32x2*>(qe + r * DM + (sub + 8 * j) * 8) = u32x2{quant4_pinned_i8(lo4, inv), quant4_pinned_i8(hi4, inv)};
  }
  if (sub == 0) se[r] = sx;
}

template <int DM, int NST>
void launch_abs_i8(const CrossAbsI8Dev& g, hipStream_t s) {
  constexpr size_t smem = (size_t)NST * 32 * DM;
  static_assert(smem <= 160 * 1024, "the ring fits the CU's LDS");
  static const bool raised = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cross_absorbed_attention_i8<DM, NST>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL((cross_absorbed_attention_i8<DM, NST>), dim3(g.B * g.chunks), dim3(320), smem, s, g);
}

template <int DM>
void launch_quant_e(const unsigned short* e, long e_plane, float e_scale, bool bf16, long rows, int8_t* qe, float* se,
                    hipStream_t s) {
  const dim3 grid((unsigned)((rows + 31) / 32));
  signed char* q = reinterpret_cast<signed char*>(qe);
  if (bf16) {
    hipLaunchKernelGGL((quantize_e_rows_i8<DM, true>), grid, dim3(256), 0, s, e, 0L, 1.0f, rows, q, se);
  } else {
    hipLaunchKernelGGL((quantize_e_rows_i8<DM, false>), grid, dim3(256), 0, s, e, e_plane, 1.0f / e_scale, rows, q, se);
  }
}

}  // namespace

void launch_quantize_e_rows_i8(const unsigned short* e, long e_plane, float e_scale, bool bf16, long rows, int d_model,
                               int8_t* qe, float* se, hipStream_t s) {
  if (!e || !qe || !se || rows < 1 || rows > (1L << 31) / 512 || (!bf16 && (!(e_scale > 0.0f) || e_plane < rows * d_model))) {
    throw Error(kErrInvalidArg, "int8 encoder-output rows: bad arguments");
  }
  switch (d_model) {
    case 128: launch_quant_e<128>(e, e_plane, e_scale, bf16, rows, qe, se, s); break;
    case 384: launch_quant_e<384>(e, e_plane, e_scale, bf16, rows, qe, se, s); break;
    case 512: launch_quant_e<512>(e, e_plane, e_scale, bf16, rows, qe, se, s); break;
    default: throw Error(kErrFormat, "int8 encoder-output rows: d_model 128, 384 or 512");
  }
}

void launch_cross_absorbed_i8(const CrossAbsorbedI8Args& a, hipStream_t s) {
  const int dm = a.d_model;
  if (!a.qp || !a.qe || !a.se || !a.ws || a.batch < 1 || a.heads < 1 || a.heads * 64 != dm || a.T < 1 || a.chunks < 1 ||
      a.chunks > 16 || a.nq < 1 || a.nq * a.heads > 16 || a.p0 < 0 || !(a.e_scale > 0.0f)) {
    throw Error(kErrInvalidArg, "int8 absorbed cross-attention: shape outside the kernel contract");
  }
  const int tiles = (a.T + 31) / 32;
  const int split = a.qe2 ? a.split : a.batch;
  if (split < 1 || split > a.batch) throw Error(kErrInvalidArg, "int8 absorbed cross-attention: bad batch split");
  const int groups = (a.batch + split - 1) / split;
  const int8_t* q[4] = {a.qe, a.qe2, a.qe3, a.qe4};
  const float* sc[4] = {a.se, a.se2, a.se3, a.se4};
  if (groups > 4) throw Error(kErrInvalidArg, "int8 absorbed cross-attention: at most four encoder batches per chain");
  for (int i = 0; i < groups; ++i)
    if (!q[i] || !sc[i]) throw Error(kErrInvalidArg, "int8 absorbed cross-attention: an encoder batch of the chain has no int8 image");
  CrossAbsI8Dev g{};
  g.qp = a.qp;
  for (int i = 0; i < 4; ++i) {
    g.qe[i] = reinterpret_cast<const signed char*>(q[i] && i < groups ? q[i] : a.qe);
    g.se[i] = sc[i] && i < groups ? sc[i] : a.se;
  }
  // |E| e_scale <= 2^14 (f16_scale_for), so se <= 2^14 / (127 e_scale) and, with p <= 2^kDeferA, W . 16 e_scale < 2^15
  g.split = split; g.w_scale = 16.0f * a.e_scale; g.ws = a.ws;
  g.B = a.batch; g.H = a.heads; g.T = a.T; g.chunks = a.chunks; g.nq = a.nq; g.p0 = a.p0;
  g.tiles_per_chunk = (tiles + a.chunks - 1) / a.chunks;
  switch (dm) {
    case 128: launch_abs_i8<128, 4>(g, s); break;
    case 384: launch_abs_i8<384, 4>(g, s); break;
    case 512: launch_abs_i8<512, 4>(g, s); break;
    default: throw Error(kErrFormat, "int8 absorbed cross-attention supports d_model 128, 384 or 512");
  }
}

}  // namespace wt
