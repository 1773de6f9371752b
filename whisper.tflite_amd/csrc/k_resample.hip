// Input resampler for gfx950: interleaved PCM at R Hz -> 16 kHz mono fp32, the Hann-windowed sinc
// polyphase filter written as a banded Toeplitz GEMM on the matrix cores.
//
//   y[(m G + g) new + p] = sum_k h[p][k] x[(m G + g) orig + k - w]
//                        = sum_kk band[kk][c] X[m][kk],   X[m][kk] = x[m S - w + kk], S = G orig, c = g new + p,
//
// band[kk][c] = h[p][kk - g orig] inside the band and exactly 0 outside it.  Every operand is two fp16 planes (hi | lo of
// value x power of two, bf16_split.h), the product three v_mfma_f32_16x16x32_f16 (hi.hi, hi.lo, lo.hi) into one fp32
// accumulator: the scheme of the plane GEMM.
//
// X is never built.  A block owns TM rows of one clip and reads their contiguous span of (TM - 1) S + Kp frames once:
// each thread converts a pair of frames (int16 -> v / 32768), takes the channel mean, clamps, splits and stores one
// dword per plane into the LDS image; frames outside [0, n) of the clip are zeros there.  Row m's window is the image at
// half-word offset m S, so the MFMA fragment of (row, k .. k + 7) starts at an offset of any parity: a lane reads the
// five dwords that cover its eight halves and funnel-shifts by 0 or 16 bits (v_alignbit_b32, an instruction the
// compiler emits and pads itself: DESIGN section 25).  The band is the "A" operand and the windows the "B" operand of the
// MFMA (Y^T = band^T X^T), so that a lane ends up with four CONSECUTIVE outputs of one row and stores them as one float4.
//
// The band planes arrive in fragment order (ResamplePlan::band): one 16-byte load per lane, plane and (k-tile, column
// tile), 1 KiB contiguous per wavefront, kept in registers for the RB row tiles of an item.  The block's work is split
// into items of RB row tiles x CB column tiles, dealt round robin to the four wavefronts; an item sweeps only the
// k-tiles its columns' band crosses (a column tile of a G = 1 plan: all of them; of a grouped plan: K + orig of Kp).
#include <hip/hip_runtime.h>

#include "bf16_split.h"
#include "kernels.h"

namespace wt {

namespace {

using half8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct ResampleK {
  const void* in;
  float* out;
  const u32x4_t* band;
  long n_frames, in_stride, n_out, out_stride, tile0;
  int format, channels;
  int orig, nnew, w, K, S, Kp, TM, cols, nct;
  int pd;        // dwords per plane of the LDS image
  int vec_ok;    // rows start 16-byte aligned: float4 stores
  float inv_ch, pcm_scale, pcm_limit, unscale;
};

// channel mean of frame f of the clip at `base` (frames outside [0, n) read as zero)
__device__ __forceinline__ float load_frame(const ResampleK& a, const void* base, long f) {
  if (f < 0 || f >= a.n_frames) return 0.0f;
  float sum = 0.0f;
  if (a.format == 1) {
    const short* p = static_cast<const short*>(base) + f * a.channels;
    for (int c = 0; c < a.channels; ++c) sum += float(p[c]) * (1.0f / 32768.0f);
  } else {
    const float* p = static_cast<const float*>(base) + f * a.channels;
    for (int c = 0; c < a.channels; ++c) sum += p[c];
  }
  return sum * a.inv_ch;
}

// No packed fp32 instructions in this kernel: hipcc would make 72 v_pk_mul_f32 of the epilogues' unscale, and an item's
// epilogue runs beside the other wavefronts' MFMAs (items end at different times), where packed fp32 costs more than the
// scalar forms it replaces (the Makefile's note on k_attention_planes; not measured here).  The attribute means something
// to the device pass only.
#if defined(__HIP_DEVICE_COMPILE__)
#define WT_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define WT_NO_PACKED_F32
#endif

template <int RB, int CB>
WT_NO_PACKED_F32 __global__ __launch_bounds__(256) void resample_band(const ResampleK a) {
  extern __shared__ unsigned image[];  // hi plane [pd] dwords (two frames each), then lo plane [pd]
  const int clip = blockIdx.y;
  const long m0 = (a.tile0 + blockIdx.x) * long(a.TM);
  const long f0 = m0 * a.S - a.w;
  const void* src = a.format == 1 ? static_cast<const void*>(static_cast<const short*>(a.in) + long(clip) * a.in_stride * a.channels)
                                  : static_cast<const void*>(static_cast<const float*>(a.in) + long(clip) * a.in_stride * a.channels);
  for (int i = threadIdx.x; i < a.pd; i += 256) {
    float v0 = load_frame(a, src, f0 + 2 * i), v1 = load_frame(a, src, f0 + 2 * i + 1);
    v0 = fminf(fmaxf(v0, -a.pcm_limit), a.pcm_limit) * a.pcm_scale;
    v1 = fminf(fmaxf(v1, -a.pcm_limit), a.pcm_limit) * a.pcm_scale;
    unsigned hi, lo;
    split_f16x2(v0, v1, &hi, &lo);
    image[i] = hi;
    image[a.pd + i] = lo;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int ncg = a.nct / CB, nrg = a.TM / (16 * RB);
  float* const dst = a.out + long(clip) * a.out_stride;
  for (int item = wv; item < nrg * ncg; item += 4) {
    const int rg = item / ncg, cg = item - rg * ncg;
    // the k-tiles the band of columns [16 CB cg, 16 CB (cg + 1)) crosses
    const int c_lo = 16 * CB * cg, c_hi = min(c_lo + 16 * CB, a.cols) - 1;
    const int kt0 = ((c_lo / a.nnew) * a.orig) >> 5;
    const int kt1 = min(a.Kp >> 5, ((c_hi / a.nnew) * a.orig + a.K + 31) >> 5);
    int xoff[RB], sh[RB];  // image offset (dwords) of this lane's fragment at k-tile 0, and its funnel shift
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int at = ((rg * RB + rb) * 16 + li) * a.S + 8 * q;  // half-words
      xoff[rb] = at >> 1;
      sh[rb] = (at & 1) * 16;
    }
    f32x4 acc[RB][CB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) acc[rb][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kt = kt0; kt < kt1; ++kt) {
      u32x4_t bh[CB], bl[CB];
      const u32x4_t* bp = a.band + (long(kt) * a.nct + cg * CB) * 128 + lane;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        bh[cb] = bp[cb * 128];
        bl[cb] = bp[cb * 128 + 64];
      }
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const unsigned* ph = image + xoff[rb] + 16 * kt;
        const unsigned* pl = ph + a.pd;
        unsigned dh[5], dl[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          dh[j] = ph[j];
          dl[j] = pl[j];
        }
        u32x4_t xh, xl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xh[j] = __builtin_amdgcn_alignbit(dh[j + 1], dh[j], sh[rb]);
          xl[j] = __builtin_amdgcn_alignbit(dl[j + 1], dl[j], sh[rb]);
        }
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, bh[cb]), __builtin_bit_cast(half8, xl), acc[rb][cb], 0, 0, 0);
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, bl[cb]), __builtin_bit_cast(half8, xh), acc[rb][cb], 0, 0, 0);
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, bh[cb]), __builtin_bit_cast(half8, xh), acc[rb][cb], 0, 0, 0);
        }
      }
    }
    // register i of this lane: column 16 ct + 4 q + i of row li, i.e. four consecutive outputs
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const long m = m0 + (rg * RB + rb) * 16 + li;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int c = 16 * (cg * CB + cb) + 4 * q;
        const long j = m * a.cols + c;
        const f32x4 v = acc[rb][cb] * a.unscale;
        if (a.vec_ok && c + 3 < a.cols && j + 3 < a.n_out) {
          *reinterpret_cast<f32x4*>(dst + j) = v;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c + i < a.cols && j + i < a.n_out) dst[j + i] = v[i];
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void pcm_downmix(const void* in, int format, int channels, float inv_ch, long n_frames,
                                                   long in_stride, float* out, long out_stride) {
  const int clip = blockIdx.y;
  for (long f = long(blockIdx.x) * 256 + threadIdx.x; f < n_frames; f += long(gridDim.x) * 256) {
    const long at = (long(clip) * in_stride + f) * channels;
    float sum = 0.0f;
    if (format == 1) {
      for (int c = 0; c < channels; ++c) sum += float(static_cast<const short*>(in)[at + c]) * (1.0f / 32768.0f);
    } else {
      for (int c = 0; c < channels; ++c) sum += static_cast<const float*>(in)[at + c];
    }
    out[long(clip) * out_stride + f] = sum * inv_ch;
  }
}

using KernelFn = void (*)(const ResampleK);
template <int RB>
KernelFn kernel_for_cb(int cb) {
  switch (cb) {
    case 1: return resample_band<RB, 1>;
    case 2: return resample_band<RB, 2>;
    case 4: return resample_band<RB, 4>;
    case 5: return resample_band<RB, 5>;
  }
  return nullptr;
}

void check_pcm(const void* in, int format, int channels, long n_frames, int batch, long in_stride, const float* out,
               long n_out, long out_stride) {
  if (!in || !out || (format != 0 && format != 1) || channels < 1 || channels > 8 || n_frames < 0 || batch < 1 ||
      batch > 65535 || (batch > 1 && (in_stride < n_frames || out_stride < n_out))) {
    throw Error(kErrInvalidArg, "resample: bad buffers, format, channels (1..8), batch (1..65535) or strides");
  }
}

}  // namespace

void launch_resample(const ResampleArgs& r, hipStream_t s) {
  check_pcm(r.in, r.format, r.channels, r.n_frames, r.batch, r.in_stride, r.out, r.n_out, r.out_stride);
  const long S = long(r.G) * r.orig, cols = long(r.G) * r.nnew;
  const long frames = long(r.TM - 1) * S + r.Kp;
  KernelFn fn = r.RB == 1 ? kernel_for_cb<1>(r.CB) : r.RB == 2 ? kernel_for_cb<2>(r.CB) : nullptr;
  if (!fn || !r.band || r.orig < 1 || r.nnew < 1 || r.G < 1 || r.w < 0 || r.K != 2 * r.w + r.orig || r.Kp % 32 != 0 ||
      r.Kp < r.K + (r.G - 1) * r.orig || r.TM < 16 || r.TM % (16 * r.RB) != 0 || ((cols + 15) / 16) % r.CB != 0 ||
      frames > 36864 || r.tiles < 1 || r.tile0 < 0 || r.n_out < 1 || (r.tile0 + r.tiles - 1) * r.TM * cols >= r.n_out) {
    throw Error(kErrInvalidArg, "resample: plan outside the kernel's contract (RB 1..2, CB 1, 2, 4, 5, Kp % 32, image <= 36864 frames) or "
                                "row tiles past the output");
  }
  ResampleK k{};
  k.in = r.in;
  k.out = r.out;
  k.band = reinterpret_cast<const u32x4_t*>(r.band);
  k.n_frames = r.n_frames;
  k.in_stride = r.in_stride;
  k.n_out = r.n_out;
  k.out_stride = r.out_stride;
  k.tile0 = r.tile0;
  k.format = r.format;
  k.channels = r.channels;
  k.orig = r.orig;
  k.nnew = r.nnew;
  k.w = r.w;
  k.K = r.K;
  k.S = int(S);
  k.Kp = r.Kp;
  k.TM = r.TM;
  k.cols = int(cols);
  k.nct = int((cols + 15) / 16);
  k.pd = int(frames / 2 + 2);
  k.vec_ok = cols % 4 == 0 && r.out_stride % 4 == 0 && reinterpret_cast<uintptr_t>(r.out) % 16 == 0;
  k.inv_ch = 1.0f / float(r.channels);
  k.pcm_scale = r.pcm_scale;
  k.pcm_limit = r.pcm_limit;
  k.unscale = 1.0f / (r.pcm_scale * r.band_scale);
  const size_t lds = size_t(k.pd) * 8;
  if (lds > 65536 &&  // above 64 KiB a kernel has to ask (per device, so at every such launch)
      hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess) {
    throw Error(kErrDevice, "resample: hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
  }
  hipLaunchKernelGGL(fn, dim3(unsigned(r.tiles), unsigned(r.batch)), dim3(256), lds, s, k);
}

void launch_pcm_downmix(const void* in, int format, int channels, long n_frames, int batch, long in_stride, float* out,
                        long out_stride, hipStream_t s) {
  check_pcm(in, format, channels, n_frames, batch, in_stride, out, n_frames, out_stride);
  if (n_frames == 0) return;
  const unsigned blocks = unsigned(std::min<long>((n_frames + 255) / 256, 4096));
  hipLaunchKernelGGL(pcm_downmix, dim3(blocks, unsigned(batch)), dim3(256), 0, s, in, format, channels, 1.0f / float(channels),
                     n_frames, in_stride, out, out_stride);
}

}  // namespace wt
