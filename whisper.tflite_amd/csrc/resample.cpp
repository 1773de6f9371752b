// The resampler's plan (filter, GEMM geometry, band planes) and the RIFF reader: DESIGN section 35.
#include "resample.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <numeric>

#include "error.h"
#include "kernels.h"

namespace wt {

namespace {
constexpr int kLpw = 6;           // lowpass_filter_width
constexpr double kRolloff = 0.99;

void ratio_of(int rate, int* orig, int* nnew) {
  if (rate < 1) throw Error(kErrInvalidArg, "resample: the sample rate must be positive");
  const int g = std::gcd(rate, kResampleRateOut);
  *orig = rate / g;
  *nnew = kResampleRateOut / g;
  if (*orig > kResampleRatioMax || *nnew > kResampleRatioMax) {
    throw Error(kErrInvalidArg, "resample: " + std::to_string(rate) + " Hz : 16000 Hz = " + std::to_string(*orig) + " : " +
                                    std::to_string(*nnew) + ", both must be at most " + std::to_string(kResampleRatioMax));
  }
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }
}  // namespace

size_t resample_len(int rate, size_t n_frames) {
  int orig = 0, nnew = 0;
  ratio_of(rate, &orig, &nnew);
  return size_t((static_cast<unsigned __int128>(n_frames) * unsigned(nnew) + unsigned(orig) - 1) / unsigned(orig));
}

ResamplePlan make_resample_plan(int rate, bool with_band) {
  ResamplePlan p;
  p.rate = rate;
  ratio_of(rate, &p.orig, &p.nnew);
  const double base = std::min(p.orig, p.nnew) * kRolloff;
  p.w = int(std::ceil(kLpw * p.orig / base));
  p.K = 2 * p.w + p.orig;
  p.h.resize(size_t(p.nnew) * p.K);
  double hmax = 0.0;
  for (int ph = 0; ph < p.nnew; ++ph) {
    for (int k = 0; k < p.K; ++k) {
      double t = (double(k - p.w) / p.orig - double(ph) / p.nnew) * base;
      t = std::min(double(kLpw), std::max(-double(kLpw), t));
      const double a = M_PI * t;
      const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
      const double c = std::cos(a / (2.0 * kLpw));
      const double v = sinc * (c * c) * (base / p.orig);
      p.h[size_t(ph) * p.K + k] = v;
      hmax = std::max(hmax, std::fabs(v));
    }
  }
  // geometry: G fills the 16 MFMA columns where nnew alone cannot; rows are S = G orig frames apart, and a block's 16 RB
  // rows must fit the LDS image, so a wide row (an odd nnew under a large orig) takes a smaller G and zero columns
  auto kp_of = [&](int G) { return round_up(p.K + (G - 1) * p.orig, 32); };
  auto frames_of = [&](int G, int TM) { return long(TM - 1) * G * p.orig + kp_of(G); };
  p.G = 16 / std::gcd(p.nnew, 16);
  while (p.G > 1 && frames_of(p.G, 16) > kResampleImageFrames) p.G /= 2;
  p.Kp = kp_of(p.G);
  p.cols = p.G * p.nnew;
  p.nct = (p.cols + 15) / 16;
  if (frames_of(p.G, 32) <= kResampleImageFrames) {
    p.RB = 2;
    p.TM = 32;
    while (p.TM + 32 <= 256 && frames_of(p.G, p.TM + 32) <= kResampleImageTarget) p.TM += 32;
  } else {
    p.RB = 1;
    p.TM = 16;
  }
  // column tiles per item: the widest of 5, 4, 2, 1 that divides nct and still leaves the block's four wavefronts an item each
  const int row_groups = p.TM / (16 * p.RB);
  p.CB = 1;
  for (int cb : {5, 4, 2}) {
    if (p.nct % cb == 0 && row_groups * (p.nct / cb) >= 4) {
      p.CB = cb;
      break;
    }
  }
  p.band_scale = f16_scale_for(float(hmax));
  if (!with_band) return p;
  p.band.assign(size_t(p.Kp / 32) * p.nct * 2 * 64 * 8, 0);
  for (int c = 0; c < p.cols; ++c) {
    const int g = c / p.nnew, ph = c % p.nnew;
    for (int k = 0; k < p.K; ++k) {
      const int kk = g * p.orig + k;
      const double v = p.h[size_t(ph) * p.K + k] * double(p.band_scale);
      const _Float16 hi = static_cast<_Float16>(v);
      const _Float16 lo = static_cast<_Float16>(v - double(hi));
      const int lane = (c & 15) | (((kk & 31) >> 3) << 4);
      const size_t at = ((size_t(kk / 32) * p.nct + c / 16) * 2 * 64 + lane) * 8 + (kk & 7);
      std::memcpy(&p.band[at], &hi, 2);
      std::memcpy(&p.band[at + 64 * 8], &lo, 2);
    }
  }
  return p;
}

// ------------------------------------------------------------------ WAV ---
WavData wav_read(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f.is_open()) throw Error(kErrIo, "Failed to open file: " + path);
  unsigned char h[12];
  if (!f.read(reinterpret_cast<char*>(h), 12) || std::memcmp(h, "RIFF", 4) != 0 || std::memcmp(h + 8, "WAVE", 4) != 0) {
    throw Error(kErrFormat, "not a RIFF / WAVE file: " + path);
  }
  auto u16 = [](const unsigned char* p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8); };
  auto u32 = [](const unsigned char* p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24); };
  WavData wv;
  uint32_t tag = 0, bits = 0, align = 0;
  bool have_fmt = false;
  unsigned char ch[8];
  while (f.read(reinterpret_cast<char*>(ch), 8)) {
    const uint32_t size = u32(ch + 4);
    if (std::memcmp(ch, "fmt ", 4) == 0) {
      unsigned char fm[40] = {};
      if (size < 16 || !f.read(reinterpret_cast<char*>(fm), std::min<uint32_t>(size, 40))) throw Error(kErrFormat, "short fmt chunk: " + path);
      tag = u16(fm);
      wv.channels = int(u16(fm + 2));
      wv.rate = int(u32(fm + 4));
      align = u16(fm + 12);
      bits = u16(fm + 14);
      if (tag == 0xFFFE && size >= 26) tag = u16(fm + 24);  // WAVE_FORMAT_EXTENSIBLE: the sub-format's first two bytes
      have_fmt = true;
      f.seekg(std::streamoff(size > 40 ? size - 40 : 0) + (size & 1), std::ios::cur);
    } else if (std::memcmp(ch, "data", 4) == 0) {
      if (!have_fmt) throw Error(kErrFormat, "data chunk in front of the fmt chunk: " + path);
      if (tag == 1 && bits == 16) wv.format = 1;
      else if (tag == 3 && bits == 32) wv.format = 0;
      else throw Error(kErrFormat, "only PCM16 and IEEE float32 are read (format tag " + std::to_string(tag) + ", " + std::to_string(bits) + " bits): " + path);
      const uint32_t frame = uint32_t(wv.channels) * (bits / 8);
      if (wv.channels < 1 || wv.rate < 1 || align != frame) throw Error(kErrFormat, "inconsistent fmt chunk: " + path);
      // a data size that runs past the end of the file (a truncated copy, a streamed header of 0xFFFFFFFF): what is there
      const std::streamoff at = f.tellg();
      f.seekg(0, std::ios::end);
      const std::streamoff left = f.tellg() - at;
      f.seekg(at);
      wv.bytes.resize(size_t(std::min<std::streamoff>(size, std::max<std::streamoff>(left, 0))));
      f.read(reinterpret_cast<char*>(wv.bytes.data()), std::streamsize(wv.bytes.size()));
      wv.n_frames = size_t(f.gcount()) / frame;
      wv.bytes.resize(wv.n_frames * frame);
      return wv;
    } else {
      f.seekg(std::streamoff(size) + (size & 1), std::ios::cur);
    }
  }
  throw Error(kErrFormat, "no data chunk: " + path);
}

}  // namespace wt
