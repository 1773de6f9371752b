// Encoder GEMM of the bf16 STORAGE mode (BASELINE configs[3]: whisper-base, bf16 weights / activations / KV with
// fp32 accumulation; option "bf16").  C = epilogue(A . W^T): A [M][K] and W [N][K] are bf16 in HBM — weights rounded
// once at load time, activations written as bf16 by the kernel that produces them (LayerNorm, this kernel's GELU /
// plain epilogues, encoder attention) — one v_mfma_f32_16x16x32_bf16 product per k-step, fp32 accumulators, fp32
// bias / GELU / positional add / residual in the epilogue.  The residual stream itself stays fp32 (it is only ever an
// epilogue operand); everything a matrix unit reads is bf16.
//
// Same skeleton as k_gemm_planes.hip (LDS-DMA straight into swizzled LDS stages, no VALU work in the loop, per-wave
// transposing epilogue), re-balanced for a third of the MFMA work per byte: k-tiles of 64 (128-byte LDS rows, the
// eight 16-byte chunks XOR-swizzled by (row >> 1) & 7 on the SOURCE address of the LDS-DMA) so that a stage holds
// twice the k-depth in the same bytes and a barrier covers 4 k-steps.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "bf16_split.h"
#include "kernels.h"

namespace wt {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int BK = 64;

// diagnostic build (tools/gemm_bf16_probe.hip): WT_BF16_ABL 1 = no LDS-DMA after the first k-tile, 2 = no MFMAs,
// 3 = no epilogue; s_memtime per phase of wave 0 into g_bf16_stamps.  The product build compiles none of it.
#ifndef WT_BF16_ABL
#define WT_BF16_ABL 0
#endif
#ifdef WT_BF16_STAMPS
__device__ long long g_bf16_stamps[4096 * 8];
#define BF_STAMP(i) do { if (tid == 0 && blockIdx.x < 4096) g_bf16_stamps[blockIdx.x * 8 + (i)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#define BF_STAMP_RT(i) do { if (tid == 0 && blockIdx.x < 4096) g_bf16_stamps[blockIdx.x * 8 + (i)] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define BF_STAMP(i) do {} while (0)
#define BF_STAMP_RT(i) do {} while (0)
#endif

struct Bf16GemmDev {
  const unsigned short* A;
  const unsigned short* W;
  float* C;            // fp32 output
  unsigned short* P;   // bf16 output (row-major like C, or the cross-KV cache layout)
  const float* bias;
  const float* R;
  const float* pos;
  int M, N, K;
  int a_rpb;
  long a_bs;
  int lda;
  int c_rpb;
  long c_bs;
  int ldc;
  int pos_period;
  int kv_batch, kv_heads, kv_dmodel;
  // LN (round 4): LayerNorm of the finished rows (N == BN: a block owns whole rows), written as the bf16 plane the next
  // GEMM reads, optionally also as fp32 (the encoder's enc_out) with the non-finite flag of the LayerNorm kernel
  const float* ln_g;
  const float* ln_b;
  unsigned short* ln_P;
  float* ln_y32;
  int* nonfinite;
};

// Epilogue shared by the two tile kernels: each wavefront transposes one 32 x 32 MFMA tile at a time through a private
// 4 KB LDS stage (conflict-free image of k_gemm_planes.hip) and moves 16 bytes per lane.  `smem` is the block's dynamic
// LDS, dead as operand staging by the time this runs; (mw0, nw0) is the wave tile's origin.
template <int EPI, bool BF_OUT, int MI_, int NI, bool LN = false, int WN = 4>
__device__ __forceinline__ void bf16_epilogue(const Bf16GemmDev& g, f32x4 (&acc)[2 * MI_][2 * NI], unsigned char* smem, int wid, int lane,
                                              int mw0, int nw0) {
  static_assert(!LN || !BF_OUT, "LayerNorm fusion: fp32 output");
  const int lc = lane & 15, lq = lane >> 4;  // accumulator tile (16 x 16): column lc, rows 4 lq + r
  // LN: the accumulator registers of a finished 32 x 32 block are dead and keep its row-major values: item i = 4 p + e
  // (row p * 8 + prow, columns c0 + e) of block (mi, ni) lives in acc[2 mi + (i >> 3)][2 ni + ((i >> 2) & 1)][i & 3]
  auto keep = [&](int mi, int ni, int i, float v) { acc[2 * mi + (i >> 3)][2 * ni + ((i >> 2) & 1)][i & 3] = v; };
  auto kept = [&](int mi, int ni, int i) -> float { return acc[2 * mi + (i >> 3)][2 * ni + ((i >> 2) & 1)][i & 3]; };
  constexpr int SLD = 32;
  float* const stage = reinterpret_cast<float*>(smem) + wid * (32 * SLD);
  constexpr int CPL = BF_OUT ? 8 : 4;
  constexpr int LPR = 32 / CPL;
  constexpr int RPS = 64 / LPR;
  const int prow = lane / LPR, c0 = (lane % LPR) * CPL;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int n = nw0 + ni * 32 + c0;
    float bias_v[CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) bias_v[e] = (EPI & kEpiBias) ? g.bias[n + e] : 0.0f;
    const int slab = (EPI & kEpiKvLayout) ? n / g.kv_dmodel : 0, rem = (EPI & kEpiKvLayout) ? n % g.kv_dmodel : 0;
    const int head = rem >> 6, dd = rem & 63;
#pragma unroll
    for (int mi = 0; mi < MI_; ++mi) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r)  // row 16 a + 4 lq + r (its bit 2 is lq & 1), columns XORed by 20 on rows with bit 2 set
            stage[(16 * a + 4 * lq + r) * SLD + ((16 * b + lc) ^ ((lq & 1) * 20))] = acc[2 * mi + a][2 * ni + b][r];
      const int mbase = mw0 + mi * 32;
      const int mb0 = mbase / g.c_rpb, mt0 = mbase % g.c_rpb;
      const int mp0 = (EPI & kEpiPos) ? mbase % g.pos_period : 0;
#pragma unroll
      for (int p = 0; p < 32 / RPS; ++p) {
        const int row = p * RPS + prow;
        float v[CPL];
#pragma unroll
        for (int e = 0; e < CPL; e += 4) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(&stage[row * SLD + ((c0 + e) ^ (((row >> 2) & 1) * 20))]);
          v[e] = t[0], v[e + 1] = t[1], v[e + 2] = t[2], v[e + 3] = t[3];
        }
        if (mbase + row < g.M) {
          int mb = mb0, mt = mt0 + row;
          if (mt >= g.c_rpb) mt -= g.c_rpb, mb += 1;
#pragma unroll
          for (int e = 0; e < CPL; e += 2) {
            v[e] += bias_v[e];
            v[e + 1] += bias_v[e + 1];
            if (EPI & kEpiGelu) {
              const f32x2_t gl = gelu_erf2(f32x2_t{v[e], v[e + 1]});
              v[e] = gl[0];
              v[e + 1] = gl[1];
            }
          }
          if (EPI & kEpiPos) {
            int mp = mp0 + row;
            if (mp >= g.pos_period) mp -= g.pos_period;
#pragma unroll
            for (int e = 0; e < CPL; e += 4) {
              const f32x4 t = *reinterpret_cast<const f32x4*>(g.pos + (long)mp * g.N + n + e);
              v[e] += t[0], v[e + 1] += t[1], v[e + 2] += t[2], v[e + 3] += t[3];
            }
          }
          if (BF_OUT) {
            const long o = (EPI & kEpiKvLayout)
                               ? (((long)slab * g.kv_batch + mb) * g.kv_heads + head) * (long)g.c_rpb * 64 + (long)mt * 64 + dd
                               : (long)mb * g.c_bs + (long)mt * g.ldc + n;
            u32x4 pk;
#pragma unroll
            for (int e = 0; e < CPL; e += 2) pk[e / 2] = pack_bf16x2(v[e], v[e + 1]);
            if (EPI & kEpiKvLayout) {  // read next by the decoder, after the caches have turned over: streaming store
              __builtin_nontemporal_store(pk, reinterpret_cast<u32x4*>(g.P + o));
            } else {
              *reinterpret_cast<u32x4*>(g.P + o) = pk;
            }
          } else {
            const long o = (long)mb * g.c_bs + (long)mt * g.ldc + n;
            f32x4 out = {v[0], v[1], v[2], v[3]};
            if (EPI & kEpiResidual) out += *reinterpret_cast<const f32x4*>(g.R + o);
            *reinterpret_cast<f32x4*>(g.C + o) = out;
            if constexpr (LN) {
#pragma unroll
              for (int e = 0; e < 4; ++e) keep(mi, ni, 4 * p + e, out[e]);
            }
          }
        } else if constexpr (LN) {
#pragma unroll
          for (int e = 0; e < 4; ++e) keep(mi, ni, 4 * p + e, 0.0f);  // rows past M: no part in anything
        }
      }
    }
  }
  if constexpr (LN) {
    // LayerNorm of the rows this block has just finished (N == BN: whole rows), as in k_gemm_planes.hip: two-pass
    // statistics, the WN wavefront columns of a block row exchange their partial sums through LDS (behind the stage
    // area), first of the values, then of the squared deviations.  The separate LayerNorm launch re-read the fp32
    // residual stream and wrote this plane: 295 MB per launch at 64 clips of whisper-base, 13 launches per pass.
    constexpr int BN = WN * NI * 32, NW = 2 * WN, BMr = 64 * MI_;
    float* const part = reinterpret_cast<float*>(smem) + NW * (32 * SLD);  // [BMr][4] partial sums, twice
    const int wm = wid / WN, wn = wid % WN;
    const int rbase = wm * (32 * MI_) + prow;
    const int m0 = mw0 - wm * (32 * MI_), n0 = nw0 - wn * (NI * 32);
    float mean[MI_][4], rstd[MI_][4];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int mi = 0; mi < MI_; ++mi)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          float t = 0.0f;
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float x = kept(mi, ni, 4 * p + e) - (pass ? mean[mi][p] : 0.0f);
              t += pass ? x * x : x;
            }
          t += __shfl_xor(t, 1, 64);
          t += __shfl_xor(t, 2, 64);
          t += __shfl_xor(t, 4, 64);
          if ((lane & 7) == 0) part[pass * (BMr * 4) + (rbase + mi * 32 + p * 8) * 4 + wn] = t;
        }
      __syncthreads();
#pragma unroll
      for (int mi = 0; mi < MI_; ++mi)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(&part[pass * (BMr * 4) + (rbase + mi * 32 + p * 8) * 4]);
          float tot = q[0];
          if (WN > 1) tot += q[1];
          if (WN > 2) tot += q[2] + q[3];
          tot *= 1.0f / (float)BN;
          if (pass == 0) {
            mean[mi][p] = tot;
          } else {
            if (g.nonfinite != nullptr && (lane & 7) == 0 && wn == 0 && !(fabsf(mean[mi][p]) <= 3.0e38f && tot <= 3.0e38f)) atomicOr(g.nonfinite, 1);
            rstd[mi][p] = rsqrtf(tot + 1e-5f);
          }
        }
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int n = n0 + (wn * NI + ni) * 32 + c0;
      const f32x4 gg = *reinterpret_cast<const f32x4*>(g.ln_g + n), bb = *reinterpret_cast<const f32x4*>(g.ln_b + n);
#pragma unroll
      for (int mi = 0; mi < MI_; ++mi)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int m = m0 + rbase + mi * 32 + p * 8;
          if (m >= g.M) continue;
          f32x4 y;
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = (kept(mi, ni, 4 * p + e) - mean[mi][p]) * rstd[mi][p] * gg[e] + bb[e];
          const long o = (long)m * BN + n;
          if (g.ln_y32 != nullptr) __builtin_nontemporal_store(y, reinterpret_cast<f32x4*>(g.ln_y32 + o));
          using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
          *reinterpret_cast<u32x2*>(g.ln_P + o) = u32x2{pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3])};
        }
    }
  }
}

// Block tile 192 x BN, BN = WN * NI * 32, 2 x WN wavefronts of 3 x NI MFMA tiles:
//   (2, 2) 192 x 128, 4 wavefronts, 40 KB per stage, two blocks per CU;  (4, 2) 192 x 256 and (4, 3) 192 x 384,
//   8 wavefronts, 56 / 72 KB per stage, one block per CU.
template <int EPI, bool BF_OUT, int WN, int NI, int MI_ = 3, bool LN = false>
__global__ __launch_bounds__(128 * WN, 2) void gemm_bf16_planes(Bf16GemmDev g) {
  // MI_ = 32-row blocks per wavefront (two wavefront rows): 3 -> 192 block rows; 2 -> 128 rows, for the 512-column
  // LayerNorm-fused tile (N == BN: the block owns whole rows) whose accumulators would not fit at 3
  constexpr int BM = 64 * MI_, MI = MI_;
  constexpr int BN = WN * NI * 32, NW = 2 * WN;
  constexpr int kABytes = BM * BK * 2, kWBytes = BN * BK * 2;
  constexpr int kStage = kABytes + kWBytes;
  constexpr int QA = BM / 8, QW = BN / 8;  // LDS-DMA instructions per operand tile (8 rows of 128 B each)
  constexpr int QT = QA + QW, QPW = QT / NW;
  static_assert(QT % NW == 0, "whole instructions per wavefront");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int logical = xcd_logical_block(gridDim.x, blockIdx.x);
  const int n_tiles = g.N / BN;
  const int m0 = (logical / n_tiles) * BM;
  const int n0 = (logical % n_tiles) * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;

  // LDS-DMA: instruction q copies rows 8 q .. 8 q + 7 of the A tile (q < QA) or of the W tile; lane i fills slot
  // (row i >> 3, chunk i & 7) with the global chunk (i & 7) ^ ((row >> 1) & 7) of that row
  const int srow = lane >> 3;
  // (uniform base) + (32-bit per-lane byte offset), issued in the SGPR-base form of global_load_lds_dwordx4 written out:
  // no vector instruction in front of a load (k_gemm_planes.hip explains why that matters on this part)
  unsigned voff[QPW];
  const unsigned char* ubase[QPW];
  const unsigned lds_base = (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)smem;
#pragma unroll
  for (int j = 0; j < QPW; ++j) {
    const int q = wid + NW * j;
    const bool is_a = q < QA;
    const int row = 8 * (is_a ? q : q - QA) + srow;
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    if (is_a) {
      int m = m0 + row;
      m = m < g.M ? m : g.M - 1;
      voff[j] = (unsigned)(2 * ((long)(m / g.a_rpb) * g.a_bs + (long)(m % g.a_rpb) * g.lda + chunk * 8));
      ubase[j] = reinterpret_cast<const unsigned char*>(g.A);
    } else {
      voff[j] = (unsigned)(2 * ((long)(n0 + row) * g.K + chunk * 8));
      ubase[j] = reinterpret_cast<const unsigned char*>(g.W);
    }
  }
  auto issue_stage = [&](int kt, int buf) {
    const size_t ko = (size_t)kt * (BK * 2);  // bytes
#pragma unroll
    for (int j = 0; j < QPW; ++j) {
      const unsigned long long sb = reinterpret_cast<unsigned long long>(ubase[j]) + ko;
      const unsigned dst = lds_base + (unsigned)(buf * kStage + (wid + NW * j) * 1024);
      lds_dma16_sgpr(voff[j], sb, dst);
    }
  };

  // (round 4) v_mfma_f32_16x16x32_bf16: the matrix pipe is power-bound and this shape does the same arithmetic on less
  // energy; lane (row lc of a 16-row fragment, 16-byte chunk lq of the 32-deep k-step)
  f32x4 acc[2 * MI][2 * NI];
#pragma unroll
  for (int i = 0; i < 2 * MI; ++i)
#pragma unroll
    for (int j = 0; j < 2 * NI; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  const int lc = lane & 15, lq = lane >> 4;
  const int swz = (lc >> 1) & 7;  // fragment bases are multiples of 16 rows: the swizzle term depends on the lane only
  const int a_off = (wm * (32 * MI) + lc) * 128, b_off = kABytes + (wn * NI * 32 + lc) * 128;
  auto compute = [&](int buf) {
    const unsigned char* base = smem + buf * kStage;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int slot = ((ks * 4 + lq) ^ swz) * 16;
      bf16x8 af[2 * MI], bf[2 * NI];
#pragma unroll
      for (int i = 0; i < 2 * MI; ++i) af[i] = *reinterpret_cast<const bf16x8*>(base + a_off + i * 16 * 128 + slot);
#pragma unroll
      for (int j = 0; j < 2 * NI; ++j) bf[j] = *reinterpret_cast<const bf16x8*>(base + b_off + j * 16 * 128 + slot);
#pragma unroll
      for (int i = 0; i < 2 * MI; ++i)
#pragma unroll
        for (int j = 0; j < 2 * NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };

  const int nkt = g.K / BK;
  BF_STAMP(0);
  BF_STAMP_RT(4);
  issue_stage(0, 0);
  for (int kt = 0; kt < nkt; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt == 0) BF_STAMP(1);
    if (kt + 1 < nkt && WT_BF16_ABL != 1) issue_stage(kt + 1, (kt + 1) & 1);
    if (WT_BF16_ABL != 2) compute(kt & 1);
  }
  __syncthreads();
  BF_STAMP(2);
  if (WT_BF16_ABL == 3 && acc[0][0][0] != 12345.678f) return;

  bf16_epilogue<EPI, BF_OUT, MI, NI, LN, WN>(g, acc, smem, wid, lane, m0 + wm * (MI * 32), n0 + wn * (NI * 32));
  BF_STAMP(3);
  BF_STAMP_RT(5);
}

template <int EPI, bool BF_OUT, int WN, int NI, int MI_ = 3, bool LN = false>
void launch_shape(const Bf16GemmDev& g, hipStream_t s) {
  constexpr int BN = WN * NI * 32, BMs = 64 * MI_;
  const int blocks = ((g.M + BMs - 1) / BMs) * (g.N / BN);
  constexpr size_t smem = 2 * (BMs * BK * 2 + BN * BK * 2);
  static_assert(!LN || smem >= (size_t)(2 * WN) * 4096 + (size_t)BMs * 4 * 2 * 4, "the LayerNorm partial sums sit behind the epilogue stages");
  static const bool raised = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_bf16_planes<EPI, BF_OUT, WN, NI, MI_, LN>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return true;
  }();
  (void)raised;
  WT_LAUNCH_TIMED((gemm_bf16_planes<EPI, BF_OUT, WN, NI, MI_, LN>), dim3(blocks), dim3(128 * WN), smem, s, g);
}

// LayerNorm fusion: the tile whose columns are the whole row (d_model 512 / 384 / 128)
template <int EPI>
void launch_bf16_ln(const Bf16GemmDev& g, hipStream_t s, const Bf16GemmPlan& plan) {
  switch (plan.bn) {
    case 512: launch_shape<EPI, false, 4, 4, 2, true>(g, s); return;
    case 384: launch_shape<EPI, false, 4, 3, 3, true>(g, s); return;
    case 128: launch_shape<EPI, false, 2, 2, 3, true>(g, s); return;
    default: throw Error(kErrUnsupported, "bf16 GEMM: the plan names a whole-row tile there is none of");
  }
}

// the tile bf16_gemm_plan (below) names
template <int EPI, bool BF_OUT>
void launch_bf16_planes(const Bf16GemmDev& g, hipStream_t s, const Bf16GemmPlan& plan) {
  if (plan.bn == 384) {
    launch_shape<EPI, BF_OUT, 4, 3>(g, s);
  } else if (plan.bn == 256) {
    launch_shape<EPI, BF_OUT, 4, 2>(g, s);
  } else {
    launch_shape<EPI, BF_OUT, 2, 2>(g, s);
  }
}

}  // namespace

Bf16GemmPlan bf16_gemm_plan(int M, int N, int epi, bool bf16_out, bool ln, int c_rpb, int ldc) {
  static const int forced = [] {
    const char* v = getenv("WT_BF16_TILE");  // measurement knob: 128 / 256 / 384 = that tile where N allows it
    return v ? atoi(v) : 0;
  }();
  // LayerNorm fusion: fp32 output in contiguous [M][N] rows, N one of the whole-row tiles; WT_BF16_LN_FUSE=0
  // keeps the separate LayerNorm launch (A/B runs)
  static const bool fuse = [] {
    const char* v = getenv("WT_BF16_LN_FUSE");
    return !v || atoi(v) != 0;
  }();
  Bf16GemmPlan p;
  if (ln && fuse && !bf16_out && ldc == N && c_rpb >= M && (N == 512 || N == 384 || N == 128) &&
      (epi == (kEpiBias | kEpiResidual) || epi == (kEpiBias | kEpiGelu | kEpiPos))) {
    p.whole_row = true;
    p.bn = N;
    p.bm = N == 512 ? 128 : 192;
    return p;
  }
  p.bn = N % 384 == 0 ? 384 : N % 256 == 0 ? 256 : 128;
  if (forced && N % forced == 0) p.bn = forced;
  if (p.bn != 384 && p.bn != 256) p.bn = 128;
  return p;
}

bool launch_gemm_bf16_planes(const PlaneGemmArgs& a, int epi, hipStream_t s) {
  Bf16GemmDev g{};
  g.A = a.A; g.W = a.W; g.C = a.C; g.P = a.P;
  g.bias = a.bias; g.R = a.R; g.pos = a.pos;
  g.M = a.M; g.N = a.N; g.K = a.K;
  g.a_rpb = a.a_rpb; g.a_bs = a.a_bs; g.lda = a.lda;
  g.c_rpb = a.c_rpb; g.c_bs = a.c_bs; g.ldc = a.ldc;
  g.pos_period = a.pos_period;
  g.kv_batch = a.kv_batch; g.kv_heads = a.kv_heads; g.kv_dmodel = a.kv_dmodel;
  const bool bf_out = a.P != nullptr;
  if (a.N % 128 != 0 || a.K % BK != 0 || a.M < 1 || a.c_rpb < 32 || a.pos_period < (epi & kEpiPos ? 32 : 1) || a.lda % 8 != 0 ||
      a.a_bs % 8 != 0 || a.ldc % 8 != 0 || a.c_bs % 8 != 0 || (!bf_out && !a.C) ||
      ((epi & kEpiKvLayout) && (!bf_out || a.kv_dmodel % 64 != 0))) {
    throw Error(kErrInvalidArg, "bf16 GEMM shape outside the kernel contract");
  }
  {  // both operands are addressed as a uniform base + 32-bit per-lane byte offset
    const long a_span = (long)((a.M - 1) / a.a_rpb) * a.a_bs + (long)(a.a_rpb < a.M ? a.a_rpb : a.M) * a.lda + a.K + 64;
    const long w_span = (long)a.N * a.K + 64;
    if (a.a_bs < 0 || 2 * a_span >= (1L << 32) || 2 * w_span >= (1L << 32)) {
      throw Error(kErrInvalidArg, "bf16 GEMM operand spans more than the 4 GiB its 32-bit offsets reach");
    }
  }
  // LayerNorm fusion (ln_g, ln_b, ln_P set; the conditions are bf16_gemm_plan's).  Returns whether the LayerNorm was done here.
  const Bf16GemmPlan plan =
      bf16_gemm_plan(a.M, a.N, epi, bf_out, a.ln_g != nullptr && a.ln_b != nullptr && a.ln_P != nullptr, a.c_rpb, a.ldc);
  if (plan.whole_row) {
    g.ln_g = a.ln_g; g.ln_b = a.ln_b; g.ln_P = a.ln_P; g.ln_y32 = a.ln_y32; g.nonfinite = a.nonfinite;
    if (epi == (kEpiBias | kEpiResidual)) {
      launch_bf16_ln<kEpiBias | kEpiResidual>(g, s, plan);
    } else {
      launch_bf16_ln<kEpiBias | kEpiGelu | kEpiPos>(g, s, plan);
    }
    return true;
  }
  switch (epi | (bf_out ? 256 : 0)) {
    case kEpiBias: launch_bf16_planes<kEpiBias, false>(g, s, plan); break;
    case kEpiBias | kEpiGelu: launch_bf16_planes<kEpiBias | kEpiGelu, false>(g, s, plan); break;  // fp32 copy of a GELU output (kernel-level taps)
    case kEpiBias | kEpiResidual: launch_bf16_planes<kEpiBias | kEpiResidual, false>(g, s, plan); break;
    case kEpiBias | kEpiGelu | kEpiPos: launch_bf16_planes<kEpiBias | kEpiGelu | kEpiPos, false>(g, s, plan); break;
    case kEpiBias | 256: launch_bf16_planes<kEpiBias, true>(g, s, plan); break;
    case kEpiBias | kEpiGelu | 256: launch_bf16_planes<kEpiBias | kEpiGelu, true>(g, s, plan); break;
    case kEpiBias | kEpiKvLayout | 256: launch_bf16_planes<kEpiBias | kEpiKvLayout, true>(g, s, plan); break;
    default: throw Error(kErrInvalidArg, "unsupported bf16 GEMM epilogue combination");
  }
  return false;
}

}  // namespace wt
