// Host side of the input resampler: any WAV rate -> 16 kHz with the Hann-windowed sinc filter of
// wt_capi.h's specification, as a banded Toeplitz GEMM on k_resample.hip.  Nothing here touches a device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace wt {

constexpr int kResampleRateOut = 16000;   // WT_SAMPLE_RATE
constexpr int kResampleRatioMax = 1024;   // orig and new of an accepted rate
constexpr int kResampleChannelsMax = 8;
constexpr int kResampleImageFrames = 36864;  // frames of one block's LDS image (4 bytes each: hi | lo fp16), 144 KiB
constexpr int kResampleImageTarget = 16384;  // what TM aims for: 64 KiB, two blocks per CU

// R : 16000 = orig : nnew in lowest terms.  Phase p, tap k of the filter weighs x[i orig + k - w] in y[i nnew + p].
// The kernel's GEMM: row m = G consecutive input blocks, its window x[m S - w .. + Kp) with S = G orig, against the band
// [Kp][cols], cols = G nnew, column c = g nnew + p holding h[p][kk - g orig] at window index kk and exact zeros elsewhere.
struct ResamplePlan {
  int rate = 0, orig = 0, nnew = 0, w = 0, K = 0;
  int G = 1;     // input blocks per row: 16 / gcd(nnew, 16), halved while 16 rows of it do not fit the LDS image (then
                 // cols is no multiple of 16 and the last column tile ends in zero columns)
  int Kp = 0;    // K + (G - 1) orig, padded to a multiple of 32
  int TM = 16;   // rows per block (a multiple of 16 RB)
  int RB = 1, CB = 1;  // 16-row tiles and 16-column tiles per wavefront item (k_resample.hip)
  int cols = 0, nct = 0;  // G nnew, ceil(cols / 16)
  float band_scale = 1.0f;  // power of two the band planes carry: max |h| * band_scale <= 16384
  std::vector<double> h;    // [nnew][K]
  // both fp16 planes of the band in MFMA-fragment order, [Kp / 32][nct][hi | lo][64 lanes][8]: lane l of (t, ct) holds
  // band[32 t + 8 (l >> 4) + e][16 ct + (l & 15)], e < 8
  std::vector<unsigned short> band;
};
// Throws kErrInvalidArg for rate < 1 or orig, nnew above kResampleRatioMax.  with_band = false leaves `band` empty.
ResamplePlan make_resample_plan(int rate, bool with_band = true);
// ceil(nnew n / orig); throws as make_resample_plan
size_t resample_len(int rate, size_t n_frames);

// A plain RIFF / WAVE reader: walks the chunks to "fmt " and "data"; PCM16 (format 0 = WT_PCM_F32, 1 = WT_PCM_S16 of
// wt_capi.h) and IEEE float32, WAVE_FORMAT_EXTENSIBLE with either sub-format included.  The interleaved samples come
// back as the file holds them.  Throws kErrIo (cannot open) or kErrFormat.
struct WavData {
  int format = 0, channels = 0, rate = 0;
  size_t n_frames = 0;
  std::vector<unsigned char> bytes;
};
WavData wav_read(const std::string& path);

}  // namespace wt
