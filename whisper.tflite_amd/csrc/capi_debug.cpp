// Kernel-level debug taps (include/wt_debug.h): host in / host out wrappers around single kernels so that a parity
// failure can be localised (tests/test_gpu_kernels.py).  Not part of the drop-in boundary.
#include "wt_debug.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "capi_internal.h"
#include "kernels.h"

namespace {
// ------------------------------------------------------------ device memory ---
// Device copy of a host array of n elements of T, and the only owner of device memory in this file (n = 0 or host =
// nullptr: uninitialised, at least one element).
template <class T>
struct DevArr {
  T* p = nullptr;
  size_t n = 0;
  explicit DevArr(size_t n_, const T* host = nullptr) : n(n_) {
    hipchk(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)), "hipMalloc");
    if (host && n) hipchk(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice), "H2D");
  }
  explicit DevArr(const std::vector<T>& host) : DevArr(host.size(), host.data()) {}
  DevArr(const DevArr&) = delete;
  DevArr& operator=(const DevArr&) = delete;
  ~DevArr() { (void)hipFree(p); }
  void to_host(T* host, size_t count) const {
    if (count) hipchk(hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost), "D2H");
  }
  void to_host(T* host) const {  // the whole array; an optional output (host = nullptr) is skipped
    if (host) to_host(host, n);
  }
  // Clears the array on the stream the kernel is launched on: that stream does not wait for the null stream, on which a
  // hipMemset may still be pending when the kernel runs.
  void zero(hipStream_t st) {
    if (n) hipchk(hipMemsetAsync(p, 0, n * sizeof(T), st), "memset");
  }
};

// ---------------------------------------------------------- operand formats ---
// fp32 [n] -> halfs hi [n + pad] then lo [n + pad] of x * scale; the pads (and all of it when x is nullptr) hold `fill`
std::vector<unsigned short> to_f16_planes(const float* x, size_t n, float scale, size_t pad, unsigned short fill = 0) {
  std::vector<unsigned short> host(2 * (n + pad), fill);
  for (size_t i = 0; x && i < n; ++i) {
    const float v = x[i] * scale;
    const _Float16 hi = static_cast<_Float16>(v), lo = static_cast<_Float16>(v - static_cast<float>(hi));
    std::memcpy(&host[i], &hi, 2);
    std::memcpy(&host[n + pad + i], &lo, 2);
  }
  return host;
}
// planes of `plane` halfs each -> fp32 [n]: (hi + lo) / scale
void from_f16_planes(const unsigned short* host, size_t plane, size_t n, float scale, float* out) {
  for (size_t i = 0; i < n; ++i) {
    _Float16 hi, lo;
    std::memcpy(&hi, &host[i], 2);
    std::memcpy(&lo, &host[plane + i], 2);
    out[i] = (static_cast<float>(hi) + static_cast<float>(lo)) / scale;
  }
}
// fp32 [n] -> bf16 [n + pad], round to nearest even; the pad (and all of it when x is nullptr) holds `fill`
std::vector<unsigned short> to_bf16(const float* x, size_t n, size_t pad, unsigned short fill = 0) {
  std::vector<unsigned short> host(n + pad, fill);
  for (size_t i = 0; x && i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, &x[i], 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) {
      host[i] = static_cast<unsigned short>((u >> 16) | 0x40u);
    } else {
      u += 0x7FFFu + ((u >> 16) & 1u);
      host[i] = static_cast<unsigned short>(u >> 16);
    }
  }
  return host;
}
void from_bf16(const unsigned short* host, size_t n, float* out) {
  for (size_t i = 0; i < n; ++i) {
    const uint32_t u = uint32_t(host[i]) << 16;
    std::memcpy(&out[i], &u, 4);
  }
}

// fp32 [n] as device planes: hi [n + pad] then lo [n + pad] halfs of x * scale (the kernels' 16-byte reads may run
// into the pad)
struct DevPlanes {
  long plane;
  DevArr<unsigned short> d;
  DevPlanes(const float* x, size_t n, float scale, size_t pad = 64) : plane(long(n + pad)), d(to_f16_planes(x, n, scale, pad)) {}
  unsigned short* ptr() const { return d.p; }
  void to_host(float* out, size_t n, float scale) const {
    std::vector<unsigned short> host(d.n);
    d.to_host(host.data());
    from_f16_planes(host.data(), size_t(plane), n, scale, out);
  }
};
// fp32 [n] as device bf16 [n + pad]
struct DevBf16 {
  DevArr<unsigned short> d;
  DevBf16(const float* x, size_t n, size_t pad = 256) : d(to_bf16(x, n, pad)) {}
  unsigned short* ptr() const { return d.p; }
  void to_host(float* out, size_t count) const {
    std::vector<unsigned short> host(count);
    d.to_host(host.data(), count);
    from_bf16(host.data(), count, out);
  }
};
// W [N][K] as device-resident fp16 planes (or bf16) in the decoder GEMM's fragment order
struct DevTiled {
  float scale = 1.0f;
  DevArr<unsigned short> d;
  DevTiled(const float* W, int N, int K, bool bf16 = false)
      : d(bf16 ? wt::tile_weights_bf16(W, N, K) : wt::tile_weights_f16(W, N, K, &scale)) {}
  const unsigned short* w() const { return d.p; }
};
// W [N][K] as the plane GEMM takes it: split_weight_planes()'s blocked layout, with 256 bytes behind it for the
// kernel's 16-byte tail reads
std::vector<unsigned short> weight_planes(const float* W, int N, int K, float scale) {
  const std::vector<unsigned short> w = wt::split_weight_planes(W, N, K, K, scale);
  std::vector<unsigned short> host(w.size() + 128, 0);
  std::copy(w.begin(), w.end(), host.begin());
  return host;
}

// ------------------------------------------------------------------ helpers ---
float max_abs(const float* x, size_t n) {
  float m = 0.0f;
  for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(x[i]));
  return m;
}

// ms per launch of f on st, after `warmup` untimed launches
template <class F>
float time_launches(hipStream_t st, int warmup, int iters, F&& f) {
  struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } ev;
  hipchk(hipEventCreate(&ev.e0), "event");
  hipchk(hipEventCreate(&ev.e1), "event");
  for (int i = 0; i < warmup; ++i) f();
  hipchk(hipEventRecord(ev.e0, st), "record");
  for (int i = 0; i < iters; ++i) f();
  hipchk(hipEventRecord(ev.e1, st), "record");
  hipchk(hipEventSynchronize(ev.e1), "sync");
  float ms = 0;
  hipchk(hipEventElapsedTime(&ms, ev.e0, ev.e1), "elapsed");
  return ms / iters;
}

// the bench taps' operands: random values in [-1, 1] (zero-filled ones would run at a higher clock and flatter the kernel)
struct Xorshift {
  uint64_t x = 88172645463325252ull;
  float operator()() {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return float(int64_t(x % 2000001) - 1000000) * 1e-6f;
  }
};

// what every dense GEMM tap sets: row-major A [M][K], C [M][N] accumulating in place, bias and positional rows
template <class G>
void dense_gemm_args(G& g, int M, int N, int K, const float* bias, float* C, const float* pos, int pos_period) {
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N;
  g.bias = bias; g.C = C; g.R = C; g.pos = pos; g.pos_period = pos_period > 0 ? pos_period : 1;
}

// max |q|, |k|, |v| over `rows` rows of [q | k | v], d columns each
struct QkvMax { float q = 0.0f, k = 0.0f, v = 0.0f; };
QkvMax qkv_maxima(const float* qkv, size_t rows, size_t d) {
  QkvMax m;
  for (size_t r = 0; r < rows; ++r) {
    const float* row = qkv + r * 3 * d;
    for (size_t c = 0; c < d; ++c) {
      m.q = std::max(m.q, std::fabs(row[c]));
      m.k = std::max(m.k, std::fabs(row[d + c]));
      m.v = std::max(m.v, std::fabs(row[2 * d + c]));
    }
  }
  return m;
}
// the softmax scale and log2(e) that the qkv GEMM's epilogue folds into q
constexpr float kQ = 0.125f * 1.44269504088896340736f;
// rows of [q | k | v] as the qkv GEMM's epilogue scales them before the plane split: q * sq (kQ included) | k * sk | v * sv
std::vector<float> scale_qkv(const float* qkv, size_t rows, size_t d, float sq, float sk, float sv) {
  std::vector<float> scaled(rows * 3 * d);
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < 3 * d; ++c) scaled[r * 3 * d + c] = qkv[r * 3 * d + c] * (c < d ? sq : c < 2 * d ? sk : sv);
  return scaled;
}

// launch_cross_attention's own refusals for a shape, before a tap sizes or allocates anything from it
void check_cross_shape(int batch, int heads, int T, int chunks, int nq) {
  wt::CrossAttnArgs ca;
  ca.batch = batch; ca.heads = heads; ca.T = T; ca.chunks = chunks; ca.nq = nq;
  wt::check_cross_attention(ca);
}

// --- what the timestamp, sample and score taps share ---
// logits [B][V] -> rows of ldl floats (V rounded up to a multiple of 4), zero padded
std::vector<float> pad_logits(const float* logits, int B, int V, int ldl) {
  std::vector<float> padded(size_t(B) * ldl, 0.0f);
  for (int b = 0; b < B; ++b) std::memcpy(&padded[size_t(b) * ldl], logits + size_t(b) * V, size_t(V) * sizeof(float));
  return padded;
}
// id rows [B][ids_stride] -> [B][ids_stride + 1]: row b's first n_ids[b] ids from column col0 on, zeros around them
std::vector<long long> widen_ids(const int64_t* ids, int B, int ids_stride, const int32_t* n_ids, int col0) {
  const int stride = ids_stride + 1;
  std::vector<long long> rows(size_t(B) * stride, 0);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < n_ids[b]; ++i) rows[size_t(b) * stride + col0 + i] = ids[size_t(b) * ids_stride + i];
  return rows;
}
// Every row decides the step behind ITS n_ids[b] ids, and the kernels take one step count per launch: f(b0, count) is
// called for each run of consecutive rows with equal n_ids (a run's launch sees only its own rows: same
// grid-independent arithmetic).
template <class F>
void for_equal_runs(const int32_t* n_ids, int B, F&& f) {
  for (int b0 = 0, b1 = 0; b0 < B; b0 = b1) {
    b1 = b0 + 1;
    while (b1 < B && n_ids[b1] == n_ids[b0]) ++b1;
    f(b0, b1 - b0);
  }
}
}  // namespace

extern "C" {

int wt_dbg_gemm(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias,
                const float* R, const float* pos, int pos_period, int epi, float* C) {
  if (!h || N % 128 || K % 32) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    DevArr<float> dA(size_t(M) * K, A), dW(size_t(N) * K, W), dB(N, bias), dC(size_t(M) * N, R),
        dP(pos ? size_t(pos_period) * N : 0, pos);
    wt::GemmArgs g;
    dense_gemm_args(g, M, N, K, dB.p, dC.p, dP.p, pos_period);
    g.A = dA.p; g.W = dW.p; g.variant = int(h->impl->gemm_variant);
    wt::launch_gemm(g, epi, h->impl->stream());
    h->impl->sync();
    dC.to_host(C, size_t(M) * N);
  });
}

int wt_dbg_gemm_planes(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias,
                       const float* R, const float* pos, int pos_period, int epi, int planes_out, int iters, float* C,
                       float* avg_ms, int n_cu) {
  if (!h || !A || !W || !C || N % 128 || K % 32 || M < 1 || n_cu < 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const float sa = wt::f16_scale_for(max_abs(A, size_t(M) * K)), sw = wt::f16_scale_for(max_abs(W, size_t(N) * K));
    const DevPlanes dA(A, size_t(M) * K, sa);
    const DevArr<unsigned short> dW(weight_planes(W, N, K, sw));
    DevArr<float> dB(N, bias), dC(size_t(M) * N, R), dP(pos ? size_t(pos_period) * N : 0, pos);
    // plane output: scale from the fp64-free bound sum |a||w| is overkill for a test tap; 2^10 / max |bias| + ... is not
    // known here, so the caller's outputs are assumed O(max|A| max|W| K): use a conservative power of two
    const float out_bound = max_abs(A, size_t(M) * K) * max_abs(W, size_t(N) * K) * float(K) + (bias ? max_abs(bias, N) : 0.0f);
    const float so = wt::f16_scale_for(out_bound);
    DevPlanes dO(nullptr, size_t(M) * N, 1.0f);
    wt::PlaneGemmArgs g;
    dense_gemm_args(g, M, N, K, dB.p, dC.p, dP.p, pos_period);
    g.A = dA.ptr(); g.a_plane = dA.plane; g.W = dW.p; g.a_scale = sa; g.w_scale = sw; g.n_cu = n_cu;
    if (planes_out) { g.P = dO.ptr(); g.p_plane = dO.plane; g.out_scale[0] = so; }
    hipStream_t st = h->impl->stream();
    wt::launch_gemm_planes(g, epi, st);
    h->impl->sync();
    if (planes_out) dO.to_host(C, size_t(M) * N, so); else dC.to_host(C, size_t(M) * N);
    // (C has been copied out: a residual epilogue may keep accumulating in place)
    if (avg_ms && iters > 0) *avg_ms = time_launches(st, 3, iters, [&] { wt::launch_gemm_planes(g, epi, st); });
  });
}

int wt_dbg_set_forced_ids(wt_engine* h, const int64_t* ids, int clips) {
  if (!h || clips < 0 || clips > 4096 || (clips && !ids)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    h->impl->forced_ids.assign(ids, ids + size_t(clips) * 32);
    for (long long v : h->impl->forced_ids)
      if (v < 0) throw wt::Error(wt::kErrInvalidArg, "forced ids must be token ids");
  });
}

int wt_dbg_set_plane_gemm_mode(int mode) {
  if (mode < 0 || mode > 4) return WT_ERR_INVALID_ARG;
  wt::set_plane_gemm_mode(mode);
  return WT_OK;
}

int wt_dbg_gemm_planes_ln(wt_engine* h, int M, int K, const float* A, const float* W, const float* bias, const float* R,
                          const float* pos, int pos_period, int epi, const float* ln_g, const float* ln_b, int n_cu,
                          float* C, float* ln_out, float* ln_y32, int* fused) {
  const int N = 384;
  if (!h || !A || !W || !C || !ln_g || !ln_b || !ln_out || !fused || K % 32 || M < 1 || n_cu < 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const float sa = wt::f16_scale_for(max_abs(A, size_t(M) * K)), sw = wt::f16_scale_for(max_abs(W, size_t(N) * K));
    const DevPlanes dA(A, size_t(M) * K, sa);
    const DevArr<unsigned short> dW(weight_planes(W, N, K, sw));
    DevArr<float> dB(N, bias), dC(size_t(M) * N, R), dP(pos ? size_t(pos_period) * N : 0, pos), dG(N, ln_g), dS(N, ln_b),
        dY(size_t(M) * N);
    DevArr<int> dF(1);
    hipStream_t st = h->impl->stream();
    dF.zero(st);
    const float so = 64.0f;  // LayerNorm output is O(|g| sqrt(N))
    DevPlanes dO(nullptr, size_t(M) * N, 1.0f);
    wt::PlaneGemmArgs g;
    dense_gemm_args(g, M, N, K, dB.p, dC.p, dP.p, pos_period);
    g.A = dA.ptr(); g.a_plane = dA.plane; g.W = dW.p; g.a_scale = sa; g.w_scale = sw; g.n_cu = n_cu;
    g.ln_g = dG.p; g.ln_b = dS.p; g.ln_P = dO.ptr(); g.ln_plane = dO.plane; g.ln_scale = so;
    g.ln_y32 = ln_y32 ? dY.p : nullptr; g.nonfinite = dF.p;
    *fused = wt::launch_gemm_planes(g, epi, st) ? 1 : 0;
    h->impl->sync();
    dC.to_host(C, size_t(M) * N);
    if (*fused) {
      dO.to_host(ln_out, size_t(M) * N, so);
      if (ln_y32) dY.to_host(ln_y32, size_t(M) * N);
    }
  });
}

int wt_dbg_encoder_attention_planes(wt_engine* h, int batch, int T, int heads, const float* qkv, int iters, float* out,
                                    float* avg_ms) {
  if (!h || !qkv || !out) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(batch) * T;
    const QkvMax m = qkv_maxima(qkv, rows, d);
    const float sq = wt::f16_scale_for(m.q * kQ), sk = wt::f16_scale_for(m.k), sv = wt::f16_scale_for(m.v), so = wt::f16_scale_for(m.v);
    const std::vector<float> scaled = scale_qkv(qkv, rows, d, kQ * sq, sk, sv);
    const DevPlanes dQ(scaled.data(), scaled.size(), 1.0f);
    DevPlanes dO(nullptr, rows * d, 1.0f);
    hipStream_t st = h->impl->stream();
    const auto launch = [&] {
      wt::launch_encoder_attention_planes(dQ.ptr(), dQ.plane, dO.ptr(), dO.plane, batch, T, heads, sq, sk, sv, so, st);
    };
    launch();
    h->impl->sync();
    dO.to_host(out, rows * d, so);
    if (avg_ms && iters > 0) *avg_ms = time_launches(st, 0, iters, launch);
  });
}

int wt_dbg_gemm_bf16(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias,
                     const float* R, const float* pos, int pos_period, int epi, int bf16_out, int iters, float* C,
                     float* avg_ms) {
  if (!h || !A || !W || !C || N % 128 || K % 64 || M < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevBf16 dA(A, size_t(M) * K), dW(W, size_t(N) * K);
    DevArr<float> dB(N, bias), dC(size_t(M) * N, R), dP(pos ? size_t(pos_period) * N : 0, pos);
    const DevBf16 dO(nullptr, size_t(M) * N);
    wt::PlaneGemmArgs g;
    dense_gemm_args(g, M, N, K, dB.p, dC.p, dP.p, pos_period);
    g.A = dA.ptr(); g.W = dW.ptr();
    if (bf16_out) g.P = dO.ptr();
    hipStream_t st = h->impl->stream();
    wt::launch_gemm_bf16_planes(g, epi, st);
    h->impl->sync();
    if (bf16_out) dO.to_host(C, size_t(M) * N); else dC.to_host(C, size_t(M) * N);
    // (C has been copied out: a residual epilogue may keep accumulating in place)
    if (avg_ms && iters > 0) *avg_ms = time_launches(st, 3, iters, [&] { wt::launch_gemm_bf16_planes(g, epi, st); });
  });
}

int wt_dbg_gemm_bf16_ln(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias, const float* R,
                        const float* ln_g, const float* ln_b, float* C, float* ln_out, float* ln_y32, int* fused) {
  if (!h || !A || !W || !bias || !R || !ln_g || !ln_b || !C || !ln_out || !ln_y32 || !fused || N % 128 || K % 64 || M < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevBf16 dA(A, size_t(M) * K), dW(W, size_t(N) * K);
    DevArr<float> dB(N, bias), dC(size_t(M) * N, R), dG(N, ln_g), dS(N, ln_b), dY(size_t(M) * N);
    const DevBf16 dL(nullptr, size_t(M) * N);
    wt::PlaneGemmArgs g;  // x += A . W^T + bias, LayerNorm(x) as a bf16 plane and as fp32
    dense_gemm_args(g, M, N, K, dB.p, dC.p, nullptr, 1);
    g.A = dA.ptr(); g.W = dW.ptr();
    g.ln_g = dG.p; g.ln_b = dS.p; g.ln_P = dL.ptr(); g.ln_y32 = dY.p;
    *fused = wt::launch_gemm_bf16_planes(g, wt::kEpiBias | wt::kEpiResidual, h->impl->stream()) ? 1 : 0;
    h->impl->sync();
    dC.to_host(C, size_t(M) * N);
    dL.to_host(ln_out, size_t(M) * N);
    dY.to_host(ln_y32, size_t(M) * N);
  });
}

int wt_dbg_encoder_attention_bf16(wt_engine* h, int batch, int T, int heads, const float* qkv, int iters, float* out,
                                  float* avg_ms) {
  if (!h || !qkv || !out) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(batch) * T;
    const DevBf16 dQ(qkv, rows * 3 * d), dO(nullptr, rows * d);
    hipStream_t st = h->impl->stream();
    const auto launch = [&] { wt::launch_encoder_attention_bf16(dQ.ptr(), dO.ptr(), batch, T, heads, st); };
    launch();
    h->impl->sync();
    dO.to_host(out, rows * d);
    if (avg_ms && iters > 0) *avg_ms = time_launches(st, 3, iters, launch);
  });
}

int wt_dbg_gemm_bench(wt_engine* h, int M, int N, int K, int epi, int variant, int iters, float* avg_ms) {
  if (!h || N % 128 || K % 32 || iters < 1 || !avg_ms) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    std::vector<float> hostA(size_t(M) * K), hostW(size_t(N) * K), hostB(N);
    Xorshift rnd;
    for (auto& v : hostA) v = rnd();
    for (auto& v : hostW) v = rnd() * 0.05f;
    for (auto& v : hostB) v = rnd();
    DevArr<float> dA(hostA), dW(hostW), dB(hostB), dC(size_t(M) * N);
    hipStream_t st = h->impl->stream();
    dC.zero(st);
    wt::GemmArgs g;
    dense_gemm_args(g, M, N, K, dB.p, dC.p, nullptr, 1);
    g.A = dA.p; g.W = dW.p; g.variant = variant;
    g.a_scale = wt::f16_scale_for(1.0f);
    g.w_scale = wt::f16_scale_for(0.05f);
    *avg_ms = time_launches(st, 3, iters, [&] { wt::launch_gemm(g, epi, st); });
    if (getenv("WT_VERBOSE_OCCUPANCY")) fprintf(stderr, "[wt] gemm variant %d: %d blocks per CU\n", g.variant, wt::gemm_occupancy(g.variant));
  });
}

int wt_dbg_interference(wt_engine* h, const float* d_mel, int batch, int n_enc, int chain_len, int blocks,
                        float* enc_ms, float* chain_ms) {
  if (!h || !d_mel || !enc_ms || !chain_ms || batch < 1 || batch > 64 || n_enc < 0 || n_enc > 8 ||
      chain_len < 0 || blocks < 1 || blocks > 4096)
    return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.sync();
    DevArr<float> buf(4096);
    hipStream_t es = e.stream(), ds = e.decoder_stream(0);
    hipEvent_t ev[4];
    for (auto& x : ev) hipchk(hipEventCreate(&x), "event");
    hipchk(hipEventRecord(ev[0], es), "record");
    for (int i = 0; i < n_enc; ++i) e.encode(d_mel, batch);
    hipchk(hipEventRecord(ev[1], es), "record");
    hipchk(hipEventRecord(ev[2], ds), "record");
    for (int i = 0; i < chain_len; ++i) wt::launch_chain_probe(buf.p, blocks, ds);
    hipchk(hipEventRecord(ev[3], ds), "record");
    hipchk(hipEventSynchronize(ev[1]), "sync");
    hipchk(hipEventSynchronize(ev[3]), "sync");
    hipchk(hipEventElapsedTime(enc_ms, ev[0], ev[1]), "elapsed");
    hipchk(hipEventElapsedTime(chain_ms, ev[2], ev[3]), "elapsed");
    for (auto& x : ev) (void)hipEventDestroy(x);
  });
}

int wt_dbg_concurrency(wt_engine* h, const float* d_mel, int batch, int n_dec, int n_enc, float* dec_ms,
                       float* enc_ms) {
  if (!h || !d_mel || !dec_ms || !enc_ms || batch < 1 || batch > 64) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] { h->impl->debug_concurrency(d_mel, batch, n_dec, n_enc, dec_ms, enc_ms); });
}

int wt_dbg_dec_gemm_bench(wt_engine* h, int kind, int B, int N, int K, int rows, int iters, float* avg_us) {
  if (!h || !avg_us || B < 1 || B > 64 || iters < 1 || rows < B || rows % B != 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    // kind 0: residual GEMM, 1: LayerNorm-fused GEMM (+bias), 2: combine + residual GEMM, 3: LayerNorm + logits + argmax records
    const int heads = K / 64, chunks = 2;
    std::vector<float> hostW(size_t(N) * K), hostX(size_t(rows) * std::max(K, N)), ws(size_t(rows) * heads * chunks * 68);
    Xorshift rnd;
    for (auto& v : hostW) v = rnd() * 0.05f;
    for (auto& v : hostX) v = rnd();
    for (auto& v : ws) v = rnd();
    const DevTiled dW(hostW.data(), N, K);
    DevArr<float> dX(size_t(rows) * K, hostX.data()), dB(N, hostX.data()), dG(K, hostX.data());
    DevArr<float> dY(size_t(rows) * N, hostX.data()), dWs(ws);
    wt::DecGemmArgs g;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = B; g.M = rows; g.bias = dB.p; g.Y = dY.p; g.ldy = N;
    int pro = wt::kProNone, epi = wt::kDecResid;
    DevArr<float> dPart(size_t(rows) * N), dR(size_t(rows) * N, hostX.data());
    if (kind == 0) { g.X = dX.p; g.ldx = K; g.R = dY.p; }
    if (kind == 0 && K > 1024) { g.ksplit = 2; g.part = dPart.p; g.R = dR.p; }  // fc2: K split over twice the blocks
    if (kind == 1) { pro = wt::kProLn; epi = wt::kDecBias; g.xin = dX.p; g.ln_g = dG.p; g.ln_b = dG.p; }
    if (kind == 2) { pro = wt::kProCombine; g.cross_ws = dWs.p; g.heads = heads; g.chunks = chunks; g.R = dY.p; }
    DevArr<unsigned long long> dBest(kind == 3 ? size_t(rows) * size_t((N + 31) / 32) : 0);
    if (kind == 3) {  // final LayerNorm + logits + argmax records (the persistent kernel; no logits written)
      pro = wt::kProLn; epi = wt::kDecLogits; g.xin = dX.p; g.ln_g = dG.p; g.ln_b = dG.p; g.Y = nullptr; g.bias = nullptr;
      g.best = dBest.p;
    }
    hipStream_t st = h->impl->stream();
    *avg_us = 1e3f * time_launches(st, 5, iters, [&] { wt::launch_dec_gemm(g, pro, epi, st); });
  });
}

static int dbg_dec_gemm_impl(wt_engine* h, int mode, int B, int N, int K, const float* X, const float* W, const float* bias,
                             const float* R, float* Y, int64_t* argmax_out, bool bf) {
  if (!h || mode < 0 || mode > 3 || B < 1 || B > 128 || (mode == 2 && !R)) {
    return WT_ERR_INVALID_ARG;
  }
  // B rows in all; more than 64 rows are presented as positions x clips (the kernels' row = p * B + b)
  const int rows_per = B > 64 ? (B % 4 == 0 ? B / 4 : (B % 2 == 0 ? B / 2 : 0)) : B;
  if (rows_per == 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevTiled dW(W, N, K, bf);
    const int n_tiles = (N + 31) / 32;
    DevArr<float> dX(size_t(B) * K, X), dB(N, bias), dY(size_t(B) * N, mode == 2 ? R : nullptr);
    DevArr<unsigned long long> dBest(size_t(B) * n_tiles);
    dBest.zero(h->impl->stream());
    wt::DecGemmArgs g;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = rows_per; g.M = B; g.X = dX.p; g.ldx = K;
    g.bf16 = bf;
    g.bias = dB.p; g.R = dY.p; g.Y = dY.p; g.ldy = N;  // residual in place, as the engine does
    g.best = dBest.p;
    const int epi = mode == 0 ? wt::kDecBias : mode == 1 ? wt::kDecBiasGelu : mode == 2 ? wt::kDecResid : wt::kDecLogits;
    wt::launch_dec_gemm(g, wt::kProNone, epi, h->impl->stream());
    h->impl->sync();
    dY.to_host(Y, size_t(B) * N);
    if (argmax_out && mode == 3) {
      // reduce the per-tile records exactly as select_token does (max of the packed keys)
      std::vector<unsigned long long> best(dBest.n);
      dBest.to_host(best.data());
      for (int b = 0; b < B; ++b) {
        unsigned long long m = 0;
        for (int t = 0; t < n_tiles; ++t) m = std::max(m, best[size_t(b) * n_tiles + t]);
        argmax_out[b] = int64_t(m & 0xffffffffull);
      }
    }
  });
}

int wt_dbg_dec_gemm(wt_engine* h, int mode, int B, int N, int K, const float* X, const float* W,
                    const float* bias, const float* R, float* Y, int64_t* argmax_out) {
  return dbg_dec_gemm_impl(h, mode, B, N, K, X, W, bias, R, Y, argmax_out, false);
}
int wt_dbg_dec_gemm_bf16(wt_engine* h, int mode, int B, int N, int K, const float* X, const float* W,
                         const float* bias, const float* R, float* Y, int64_t* argmax_out) {
  return dbg_dec_gemm_impl(h, mode, B, N, K, X, W, bias, R, Y, argmax_out, true);
}

static int dbg_dec_ln_gemm_impl(wt_engine* h, int B, int N, int K, const float* xin, const int64_t* ids, int pos,
                                const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos, const float* ln_g,
                                const float* ln_b, const float* W, const float* bias, int gelu, float* Y, float* xout, bool bf,
                                const int32_t* pos_start = nullptr) {
  // (pos_start: pos counts slots and may lie past the table; the kernel clamps the row it reads)
  if (!h || B < 1 || B > 64 || (K != 128 && K != 384 && K != 512) || (!xin && !ids) || pos < 0 ||
      (ids && pos >= (pos_start ? 4096 : n_pos)) || (pos_start && (!ids || n_pos < 1))) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevTiled dW(W, N, K, bf);
    DevArr<float> dxin(xin ? size_t(B) * K : 0, xin);
    DevArr<float> dtok(ids ? size_t(n_vocab) * K : 0, tok_emb), dpos(ids ? size_t(n_pos) * K : 0, pos_emb);
    DevArr<float> dg(K, ln_g), db(K, ln_b), dB(N, bias), dY(size_t(B) * N), dxo(size_t(B) * K);
    // the kernel reads ids[b][pos]: one row of pos + 1 ids per clip, the given id in its last column
    std::vector<long long> idrows(size_t(B) * (pos + 1), 0);
    if (ids)
      for (int b = 0; b < B; ++b) idrows[size_t(b) * (pos + 1) + pos] = ids[b];
    DevArr<long long> dids(idrows);
    dxo.zero(h->impl->stream());
    wt::DecGemmArgs g;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = B; g.bf16 = bf;
    g.xin = dxin.p; g.xout = dxo.p; g.ln_g = dg.p; g.ln_b = db.p;
    if (ids) {
      g.ids = dids.p; g.ids_stride = pos + 1; g.pos = pos;
      g.tok_emb = dtok.p; g.pos_emb = dpos.p; g.n_vocab = n_vocab;
    }
    const DevArr<int> dstart(pos_start ? size_t(B) : 0, pos_start);
    if (pos_start) g.pos_start = dstart.p, g.n_ctx = n_pos;
    g.bias = dB.p; g.Y = dY.p; g.ldy = N;
    wt::launch_dec_gemm(g, wt::kProLn, gelu ? wt::kDecBiasGelu : wt::kDecBias, h->impl->stream());
    h->impl->sync();
    dY.to_host(Y, size_t(B) * N);
    if (xout) dxo.to_host(xout, size_t(B) * K);
  });
}

int wt_dbg_dec_ln_gemm(wt_engine* h, int B, int N, int K, const float* xin, const int64_t* ids, int pos,
                       const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos,
                       const float* ln_g, const float* ln_b, const float* W, const float* bias,
                       int gelu, float* Y, float* xout) {
  return dbg_dec_ln_gemm_impl(h, B, N, K, xin, ids, pos, tok_emb, pos_emb, n_vocab, n_pos, ln_g, ln_b, W, bias, gelu, Y, xout, false);
}
int wt_dbg_dec_ln_gemm_bf16(wt_engine* h, int B, int N, int K, const float* xin, const int64_t* ids, int pos,
                            const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos,
                            const float* ln_g, const float* ln_b, const float* W, const float* bias,
                            int gelu, float* Y, float* xout) {
  return dbg_dec_ln_gemm_impl(h, B, N, K, xin, ids, pos, tok_emb, pos_emb, n_vocab, n_pos, ln_g, ln_b, W, bias, gelu, Y, xout, true);
}

int wt_dbg_dec_ln_gemm_ragged(wt_engine* h, int B, int N, int K, const int64_t* ids, int pos, const int32_t* pos_start,
                              const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos,
                              const float* ln_g, const float* ln_b, const float* W, const float* bias,
                              int gelu, float* Y, float* xout) {
  return dbg_dec_ln_gemm_impl(h, B, N, K, nullptr, ids, pos, tok_emb, pos_emb, n_vocab, n_pos, ln_g, ln_b, W, bias, gelu, Y, xout, false, pos_start);
}

int wt_dbg_layernorm(wt_engine* h, int M, int d, const float* x, const float* g, const float* b, float* y) {
  if (!h || d > 512) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    DevArr<float> dx(size_t(M) * d, x), dg(d, g), db(d, b), dy(size_t(M) * d);
    wt::launch_layernorm(dx.p, dy.p, dg.p, db.p, M, d, h->impl->stream());
    h->impl->sync();
    dy.to_host(y, size_t(M) * d);
  });
}

int wt_dbg_encoder_attention(wt_engine* h, int batch, int T, int heads, const float* qkv, float* out) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64;
    DevArr<float> dq(size_t(batch) * T * 3 * d, qkv), dout(size_t(batch) * T * d);
    // fp32-storage forms only (0, 1); the default plane kernel has its own tap (wt_dbg_encoder_attention_planes)
    wt::launch_encoder_attention(dq.p, dout.p, batch, T, heads, h->impl->attn_variant == 4 ? 1 : int(h->impl->attn_variant),
                                 h->impl->stream());
    h->impl->sync();
    dout.to_host(out, size_t(batch) * T * d);
  });
}

static int dbg_cross_attention_impl(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                    const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                    const float* vc, float* out, bool bf) {
  if (!h || (chunks != 1 && chunks != 2 && chunks != 4 && chunks != 8) || batch < 1 || nq < 1 || nq * batch > 128 ||
      !x || !ln_g || !ln_b || !wq || !bq || !kc || !vc || !out)
    return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    check_cross_shape(batch, heads, T, chunks, nq);
    const size_t d = size_t(heads) * 64, rows = size_t(nq) * batch, nc = size_t(batch) * T * d;
    DevArr<float> dx(rows * d, x), dg(d, ln_g), db(d, ln_b), dbq(d, bq), dk(bf ? 0 : nc, kc), dv(bf ? 0 : nc, vc);
    const DevBf16 dkb(kc, bf ? nc : 0), dvb(vc, bf ? nc : 0);
    DevArr<float> dwq(wt::cross_q_layout(wq, int(d)));
    DevArr<float> dws(rows * heads * chunks * 68), dout(rows * d), dzero(d);
    hipStream_t st = h->impl->stream();
    dout.zero(st);
    dzero.zero(st);
    // the product combines the chunk partials in the out-projection's prologue; an identity
    // projection onto a zero residual exposes exactly that combined row
    std::vector<float> eye(d * d, 0.0f);
    for (size_t i = 0; i < d; ++i) eye[i * d + i] = 1.0f;
    const DevTiled dW(eye.data(), int(d), int(d));
    wt::CrossAttnArgs ca;
    ca.x = dx.p; ca.ln_g = dg.p; ca.ln_b = db.p; ca.wq_t = dwq.p; ca.bq = dbq.p;
    ca.kc = bf ? static_cast<const void*>(dkb.ptr()) : dk.p; ca.vc = bf ? static_cast<const void*>(dvb.ptr()) : dv.p; ca.bf16 = bf;
    ca.ws = dws.p; ca.batch = batch; ca.heads = heads; ca.T = T; ca.chunks = chunks; ca.nq = nq;
    wt::launch_cross_attention(ca, st);
    wt::DecGemmArgs g;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = int(d); g.K = int(d); g.B = batch; g.M = int(rows);
    g.cross_ws = dws.p; g.heads = heads; g.chunks = chunks;
    g.bias = dzero.p; g.R = dout.p; g.Y = dout.p; g.ldy = int(d);
    wt::launch_dec_gemm(g, wt::kProCombine, wt::kDecResid, st);
    h->impl->sync();
    dout.to_host(out, rows * d);
  });
}

int wt_dbg_cross_attention(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                           const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                           const float* vc, float* out) {
  return dbg_cross_attention_impl(h, batch, heads, T, chunks, nq, x, ln_g, ln_b, wq, bq, kc, vc, out, false);
}
int wt_dbg_cross_attention_bf16(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                const float* vc, float* out) {
  return dbg_cross_attention_impl(h, batch, heads, T, chunks, nq, x, ln_g, ln_b, wq, bq, kc, vc, out, true);
}

static int dbg_cross_records_impl(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                  const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                  const float* vc, int row0, int n_rows, float* ws, bool bf) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    check_cross_shape(batch, heads, T, chunks, n_rows);  // the launcher's own refusals, before anything is allocated
    if (!x || !ln_g || !ln_b || !wq || !bq || !kc || !vc || !ws || row0 < 0 || nq < 1 || nq > 128 / batch || row0 > nq - n_rows)
      throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_cross_attention_records: NULL array or positions outside the buffer");
    const size_t d = size_t(heads) * 64, rows = size_t(nq) * batch, nc = size_t(batch) * T * d;
    const size_t rec = size_t(heads) * chunks * 68;  // floats per row of ws
    DevArr<float> dx(rows * d, x), dg(d, ln_g), db(d, ln_b), dbq(d, bq), dk(bf ? 0 : nc, kc), dv(bf ? 0 : nc, vc);
    const DevBf16 dkb(kc, bf ? nc : 0), dvb(vc, bf ? nc : 0);
    DevArr<float> dwq(wt::cross_q_layout(wq, int(d)));
    DevArr<float> dws(rows * rec, ws);  // the caller's guard pattern
    wt::CrossAttnArgs ca;
    ca.ln_g = dg.p; ca.ln_b = db.p; ca.wq_t = dwq.p; ca.bq = dbq.p;
    ca.kc = bf ? static_cast<const void*>(dkb.ptr()) : dk.p; ca.vc = bf ? static_cast<const void*>(dvb.ptr()) : dv.p; ca.bf16 = bf;
    ca.batch = batch; ca.heads = heads; ca.T = T; ca.chunks = chunks;
    // positions row0 .. row0 + n_rows - 1 of the buffer, addressed as Engine::decoder_pass's p0 loop addresses them
    ca.x = dx.p + size_t(row0) * batch * d; ca.ws = dws.p + size_t(row0) * batch * rec; ca.nq = n_rows;
    wt::launch_cross_attention(ca, h->impl->stream());
    h->impl->sync();
    dws.to_host(ws);
  });
}

int wt_dbg_cross_attention_records(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                   const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                   const float* vc, int row0, int n_rows, float* ws) {
  return dbg_cross_records_impl(h, batch, heads, T, chunks, nq, x, ln_g, ln_b, wq, bq, kc, vc, row0, n_rows, ws, false);
}
int wt_dbg_cross_attention_records_bf16(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                        const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                        const float* vc, int row0, int n_rows, float* ws) {
  return dbg_cross_records_impl(h, batch, heads, T, chunks, nq, x, ln_g, ln_b, wq, bq, kc, vc, row0, n_rows, ws, true);
}

static int dbg_cross_combine_impl(wt_engine* h, int M, int B, int heads, int chunks, const float* records, const float* W,
                                  const float* bias, const float* R, int guard_rows, float* Y, bool bf) {
  if (!h || !records || !W || !bias || !R || !Y || M < 1 || M > 128 || B < 1 || heads < 1 || heads > 8 || chunks < 1 ||
      chunks > 8 || guard_rows < 0 || guard_rows > 128)
    return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64;
    const DevTiled dW(W, int(d), int(d), bf);
    DevArr<float> dws(size_t(M) * heads * chunks * 68, records), db(d, bias);
    std::vector<float> y0(Y, Y + (size_t(M) + guard_rows) * d);  // rows >= M: the caller's guard pattern
    std::copy(R, R + size_t(M) * d, y0.begin());
    DevArr<float> dY(y0);
    wt::DecGemmArgs g;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = int(d); g.K = int(d); g.B = B; g.M = M; g.bf16 = bf;
    g.cross_ws = dws.p; g.heads = heads; g.chunks = chunks;
    g.bias = db.p; g.R = dY.p; g.Y = dY.p; g.ldy = int(d);  // residual in place, as the engine does
    wt::launch_dec_gemm(g, wt::kProCombine, wt::kDecResid, h->impl->stream());
    h->impl->sync();
    dY.to_host(Y);
  });
}

int wt_dbg_cross_combine(wt_engine* h, int M, int B, int heads, int chunks, const float* records, const float* W,
                         const float* bias, const float* R, int guard_rows, float* Y) {
  return dbg_cross_combine_impl(h, M, B, heads, chunks, records, W, bias, R, guard_rows, Y, false);
}
int wt_dbg_cross_combine_bf16(wt_engine* h, int M, int B, int heads, int chunks, const float* records, const float* W,
                              const float* bias, const float* R, int guard_rows, float* Y) {
  return dbg_cross_combine_impl(h, M, B, heads, chunks, records, W, bias, R, guard_rows, Y, true);
}

static int dbg_cross_absorbed_impl(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* qp, const float* E,
                                   const float* wv, const float* bv, float* out, int iters, float* avg_us, bool bf) {
  if (!h || !qp || !E || !wv || !bv || !out || batch < 1 || heads < 1 || T < 1 || nq < 1 || chunks < 1 || chunks > 16) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(nq) * batch, ne = size_t(batch) * T * d;
    const float se = bf ? 1.0f : wt::f16_scale_for(max_abs(E, ne));
    const DevArr<unsigned short> dE(bf ? to_bf16(E, ne, 256) : to_f16_planes(E, ne, se, 64));
    DevArr<float> dq(rows * heads * d, qp), dws(rows * heads * chunks * (d + 4)), dout(rows * d), dwv(wt::cross_q_layout(wv, int(d))),
        dbv(d, bv);
    const int nq_max = wt::cross_absorbed_max_nq(heads);
    hipStream_t st = h->impl->stream();
    const auto launch = [&](int p0, int n) {
      wt::CrossAbsorbedArgs a;
      a.qp = dq.p; a.e = dE.p; a.e_plane = bf ? 0 : long(ne + 64); a.e_scale = se; a.ws = dws.p; a.bf16 = bf;
      a.batch = batch; a.heads = heads; a.d_model = int(d); a.T = T; a.chunks = chunks; a.nq = n; a.p0 = p0;
      wt::launch_cross_absorbed(a, st);
    };
    for (int p0 = 0; p0 < nq; p0 += nq_max) launch(p0, std::min(nq_max, nq - p0));
    wt::launch_cross_absorbed_combine(dws.p, dwv.p, dbv.p, dout.p, int(rows), heads, chunks, int(d), st);
    h->impl->sync();
    dout.to_host(out, rows * d);
    if (iters > 0 && avg_us) *avg_us = 1e3f * time_launches(st, 3, iters, [&] { launch(0, std::min(nq_max, nq)); });
  });
}

int wt_dbg_cross_absorbed(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* qp, const float* E,
                          const float* wv, const float* bv, float* out, int iters, float* avg_us) {
  return dbg_cross_absorbed_impl(h, batch, heads, T, chunks, nq, qp, E, wv, bv, out, iters, avg_us, false);
}

int wt_dbg_cross_absorbed_bf16(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* qp, const float* E,
                               const float* wv, const float* bv, float* out, int iters, float* avg_us) {
  return dbg_cross_absorbed_impl(h, batch, heads, T, chunks, nq, qp, E, wv, bv, out, iters, avg_us, true);
}

static int dbg_self_attention_impl(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                   float* kcache, float* vcache, float* out, bool bf) {
  if (!h || cap > wt::kSelfLongCap) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::check_self_attention(cap, pos, npos, batch, heads);  // the launcher's own refusals, before anything is allocated
    if (!qkv || !kcache || !vcache || !out) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_self_attention: NULL array");
    const size_t d = size_t(heads) * 64, rows = size_t(npos) * batch, nc = size_t(batch) * cap * d;
    DevArr<float> dq(rows * 3 * d, qkv), dk(bf ? 0 : nc, kcache), dv(bf ? 0 : nc, vcache), dout(rows * d);
    const DevBf16 dkb(kcache, bf ? nc : 0), dvb(vcache, bf ? nc : 0);  // bf16 caches (storage mode)
    wt::launch_self_attention(dq.p, bf ? static_cast<void*>(dkb.ptr()) : dk.p, bf ? static_cast<void*>(dvb.ptr()) : dv.p, cap, pos,
                              npos, dout.p, batch, heads, h->impl->stream(), bf);
    h->impl->sync();
    dout.to_host(out, rows * d);
    if (bf) {
      dkb.to_host(kcache, nc);
      dvb.to_host(vcache, nc);
    } else {
      dk.to_host(kcache, nc);
      dv.to_host(vcache, nc);
    }
  });
}
int wt_dbg_self_attention(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                          float* kcache, float* vcache, float* out) {
  return dbg_self_attention_impl(h, batch, heads, cap, pos, npos, qkv, kcache, vcache, out, false);
}
int wt_dbg_self_attention_bf16(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                               float* kcache, float* vcache, float* out) {
  return dbg_self_attention_impl(h, batch, heads, cap, pos, npos, qkv, kcache, vcache, out, true);
}
// The fp32 or the bf16 pair of self-attention caches of a tap (bf16 storage mode: the host arrays are float32 holding
// bf16-representable values, as wt_dbg_self_attention_bf16 takes them)
struct DbgSelfCaches {
  DevArr<float> dk, dv;
  const DevBf16 dkb, dvb;
  const bool bf;
  DbgSelfCaches(float* kcache, float* vcache, size_t nc, bool bf_)
      : dk(bf_ ? 0 : nc, kcache), dv(bf_ ? 0 : nc, vcache), dkb(kcache, bf_ ? nc : 0), dvb(vcache, bf_ ? nc : 0), bf(bf_) {}
  void* k() const { return bf ? static_cast<void*>(dkb.ptr()) : dk.p; }
  void* v() const { return bf ? static_cast<void*>(dvb.ptr()) : dv.p; }
  void to_host(float* kcache, float* vcache, size_t nc) const {
    if (bf) {
      dkb.to_host(kcache, nc);
      dvb.to_host(vcache, nc);
    } else {
      dk.to_host(kcache, nc);
      dv.to_host(vcache, nc);
    }
  }
};
static int dbg_self_attention_long_impl(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                                        float* vcache, float* out, bool bf) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    // the launcher's own refusals, before anything is allocated
    if (bf) wt::check_self_attention_long_bf16(cap, pos, batch, heads);
    else wt::check_self_attention_long(cap, pos, batch, heads);
    if (!qkv || !kcache || !vcache || !out) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_self_attention_long: NULL array");
    const size_t d = size_t(heads) * 64, nc = size_t(batch) * cap * d;
    DevArr<float> dq(size_t(batch) * 3 * d, qkv), dout(size_t(batch) * d);
    const DbgSelfCaches c(kcache, vcache, nc, bf);
    wt::launch_self_attention_long(dq.p, c.k(), c.v(), cap, pos, dout.p, batch, heads, h->impl->stream(), bf);
    h->impl->sync();
    dout.to_host(out, size_t(batch) * d);
    c.to_host(kcache, vcache, nc);
  });
}
int wt_dbg_self_attention_long(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                               float* vcache, float* out) {
  return dbg_self_attention_long_impl(h, batch, heads, cap, pos, qkv, kcache, vcache, out, false);
}
int wt_dbg_self_attention_long_bf16(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                                    float* vcache, float* out) {
  return dbg_self_attention_long_impl(h, batch, heads, cap, pos, qkv, kcache, vcache, out, true);
}
static int dbg_self_attention_prefill_impl(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                           float* kcache, float* vcache, float* out, bool bf) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    // the launcher's own refusals, before anything is allocated
    if (bf) wt::check_self_attention_prefill_bf16(cap, pos, npos, batch, heads);
    else wt::check_self_attention_prefill(cap, pos, npos, batch, heads);
    if (!qkv || !kcache || !vcache || !out) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_self_attention_prefill: NULL array");
    const size_t d = size_t(heads) * 64, rows = size_t(npos) * batch, nc = size_t(batch) * cap * d;
    DevArr<float> dq(rows * 3 * d, qkv), dout(rows * d);
    const DbgSelfCaches c(kcache, vcache, nc, bf);
    wt::launch_self_attention_prefill(dq.p, c.k(), c.v(), cap, pos, npos, dout.p, batch, heads, h->impl->stream(), bf);
    h->impl->sync();
    dout.to_host(out, rows * d);
    c.to_host(kcache, vcache, nc);
  });
}
int wt_dbg_self_attention_prefill(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                  float* kcache, float* vcache, float* out) {
  return dbg_self_attention_prefill_impl(h, batch, heads, cap, pos, npos, qkv, kcache, vcache, out, false);
}
int wt_dbg_self_attention_prefill_bf16(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                       float* kcache, float* vcache, float* out) {
  return dbg_self_attention_prefill_impl(h, batch, heads, cap, pos, npos, qkv, kcache, vcache, out, true);
}
static int dbg_self_attention_long_ragged_impl(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv,
                                               float* kcache, float* vcache, float* out, const int32_t* start, int P, bool bf) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    // the launcher's own refusals, before anything is allocated
    if (bf) wt::check_self_attention_long_ragged_bf16(cap, pos, P, batch, heads);
    else wt::check_self_attention_long_ragged(cap, pos, P, batch, heads);
    if (!qkv || !kcache || !vcache || !out || !start) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_self_attention_long_ragged: NULL array");
    const size_t d = size_t(heads) * 64, nc = size_t(batch) * cap * d;
    DevArr<float> dq(size_t(batch) * 3 * d, qkv), dout(size_t(batch) * d);
    const DbgSelfCaches c(kcache, vcache, nc, bf);
    const DevArr<int> ds(size_t(batch), start);
    wt::launch_self_attention_long_ragged(dq.p, c.k(), c.v(), cap, pos, ds.p, P, dout.p, batch, heads, h->impl->stream(), bf);
    h->impl->sync();
    dout.to_host(out, size_t(batch) * d);
    c.to_host(kcache, vcache, nc);
  });
}
int wt_dbg_self_attention_long_ragged(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                                      float* vcache, float* out, const int32_t* start, int P) {
  return dbg_self_attention_long_ragged_impl(h, batch, heads, cap, pos, qkv, kcache, vcache, out, start, P, false);
}
int wt_dbg_self_attention_long_ragged_bf16(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                                           float* vcache, float* out, const int32_t* start, int P) {
  return dbg_self_attention_long_ragged_impl(h, batch, heads, cap, pos, qkv, kcache, vcache, out, start, P, true);
}
static int dbg_self_attention_long_gather_impl(wt_engine* h, int rows, int heads, int cap, int pos, const float* qkv,
                                               float* kcache, float* vcache, float* out, const uint8_t* anc, bool bf) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    // the launcher's own refusals, before anything is allocated
    if (bf) wt::check_self_attention_long_gather_bf16(cap, pos, rows, heads);
    else wt::check_self_attention_long_gather(cap, pos, rows, heads);
    if (!qkv || !kcache || !vcache || !out || !anc) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_self_attention_long_gather: NULL array");
    const size_t d = size_t(heads) * 64, nc = size_t(rows) * cap * d;
    DevArr<float> dq(size_t(rows) * 3 * d, qkv), dout(size_t(rows) * d);
    const DbgSelfCaches c(kcache, vcache, nc, bf);
    const DevArr<unsigned char> da(size_t(rows) * cap, anc);
    wt::launch_self_attention_long_gather(dq.p, c.k(), c.v(), cap, pos, da.p, dout.p, rows, heads, h->impl->stream(), bf);
    h->impl->sync();
    dout.to_host(out, size_t(rows) * d);
    c.to_host(kcache, vcache, nc);
  });
}
int wt_dbg_self_attention_long_gather(wt_engine* h, int rows, int heads, int cap, int pos, const float* qkv, float* kcache,
                                      float* vcache, float* out, const uint8_t* anc) {
  return dbg_self_attention_long_gather_impl(h, rows, heads, cap, pos, qkv, kcache, vcache, out, anc, false);
}
int wt_dbg_self_attention_long_gather_bf16(wt_engine* h, int rows, int heads, int cap, int pos, const float* qkv, float* kcache,
                                           float* vcache, float* out, const uint8_t* anc) {
  return dbg_self_attention_long_gather_impl(h, rows, heads, cap, pos, qkv, kcache, vcache, out, anc, true);
}
static int dbg_self_attention_prefill_ragged_impl(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                                  float* kcache, float* vcache, float* out, const int32_t* start, int P, bool bf) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    // the launcher's own refusals, before anything is allocated
    if (bf) wt::check_self_attention_prefill_ragged_bf16(cap, pos, npos, P, batch, heads);
    else wt::check_self_attention_prefill_ragged(cap, pos, npos, P, batch, heads);
    if (!qkv || !kcache || !vcache || !out || !start) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_self_attention_prefill_ragged: NULL array");
    const size_t d = size_t(heads) * 64, rows = size_t(npos) * batch, nc = size_t(batch) * cap * d;
    DevArr<float> dq(rows * 3 * d, qkv), dout(rows * d);
    const DbgSelfCaches c(kcache, vcache, nc, bf);
    const DevArr<int> ds(size_t(batch), start);
    wt::launch_self_attention_prefill_ragged(dq.p, c.k(), c.v(), cap, pos, npos, ds.p, P, dout.p, batch, heads,
                                             h->impl->stream(), bf);
    h->impl->sync();
    dout.to_host(out, rows * d);
    c.to_host(kcache, vcache, nc);
  });
}
int wt_dbg_self_attention_prefill_ragged(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                         float* kcache, float* vcache, float* out, const int32_t* start, int P) {
  return dbg_self_attention_prefill_ragged_impl(h, batch, heads, cap, pos, npos, qkv, kcache, vcache, out, start, P, false);
}
int wt_dbg_self_attention_prefill_ragged_bf16(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                              float* kcache, float* vcache, float* out, const int32_t* start, int P) {
  return dbg_self_attention_prefill_ragged_impl(h, batch, heads, cap, pos, npos, qkv, kcache, vcache, out, start, P, true);
}
int wt_dbg_ragged_cap(wt_engine* h, int batch, int pos, int P, const int32_t* start, int32_t* finished) {
  if (!h || batch < 1 || batch > 64 || !start || !finished) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevArr<int> ds(size_t(batch), start);
    DevArr<int> df(size_t(batch), finished);
    wt::launch_ragged_cap(ds.p, pos, P, df.p, batch, h->impl->stream());
    h->impl->sync();
    df.to_host(finished, size_t(batch));
  });
}

}  // extern "C"

namespace {
// the engine's per-clip beam state (ensure_beam_workspace), host in / host out
struct DevBeamState {
  static constexpr size_t C = wt::kBeamClipsMax, S = wt::kBeamMax;
  DevArr<float> live_sum, fin_sum;
  DevArr<int> fin_tok, fin_len, n_fin, done;
  DevBeamState(const float* ls, const int32_t* ft, const float* fs, const int32_t* fl, const int32_t* nf, const int32_t* dn)
      : live_sum(C * S, ls), fin_sum(C * S, fs), fin_tok(C * S * 32, ft), fin_len(C * S, fl), n_fin(C, nf), done(C, dn) {}
};
}  // namespace

extern "C" {

int wt_dbg_beam_topk(wt_engine* h, int rows, int V, int ldl, int kk, const float* logits, float* m, float* s,
                     uint64_t* keys) {
  if (!h || !logits || !m || !s || !keys || rows < 1 || V < 1 || ldl < V || kk < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const int chunks = wt::beam_chunks(V);
    DevArr<float> dz(size_t(rows) * ldl, logits);
    DevArr<wt::BeamPart> dp(size_t(rows) * chunks);
    dp.zero(h->impl->stream());
    wt::launch_beam_topk(dz.p, ldl, V, rows, kk, dp.p, h->impl->stream());
    h->impl->sync();
    std::vector<wt::BeamPart> part(dp.n);
    dp.to_host(part.data());
    for (size_t i = 0; i < part.size(); ++i) {
      m[i] = part[i].m;
      s[i] = part[i].s;
      for (int r = 0; r < kk; ++r) keys[i * kk + r] = part[i].key[r];
    }
  });
}

int wt_dbg_beam_step(wt_engine* h, int K, int clips, int c0, int n_live, int pos, int n_prompt, int V, int64_t eot,
                     const float* logits, const int64_t* ids, float* live_sum, int32_t* fin_tok, float* fin_sum,
                     int32_t* fin_len, int32_t* n_fin, int32_t* done, int32_t* parent, int64_t* token, int64_t* ids_next) {
  if (!h || !logits || !ids || !live_sum || !fin_tok || !fin_sum || !fin_len || !n_fin || !done || !parent || !token ||
      !ids_next || K < 1 || clips < 1 || n_live < 1 || V < 1 || size_t(K) * clips > 128 || size_t(n_live) * clips > 128) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    hipStream_t st = h->impl->stream();
    const int src_rows = n_live * clips, dst_rows = K * clips;
    DevArr<float> dz(size_t(src_rows) * V, logits);
    DevArr<wt::BeamPart> dp(size_t(src_rows) * wt::beam_chunks(V));
    DevArr<long long> dids(size_t(src_rows) * 32, reinterpret_cast<const long long*>(ids)), dnext(size_t(dst_rows) * 32);
    DevArr<int> dparent(dst_rows);
    DevArr<long long> dtoken(dst_rows);
    DevBeamState bs(live_sum, fin_tok, fin_sum, fin_len, n_fin, done);
    wt::launch_beam_topk(dz.p, V, V, src_rows, K + 1, dp.p, st);
    wt::BeamStepArgs sa;
    sa.part = dp.p; sa.n_chunks = wt::beam_chunks(V); sa.ids = dids.p;
    sa.clips = clips; sa.K = K; sa.n_live = n_live; sa.pos = pos; sa.n_prompt = n_prompt; sa.V = V; sa.c0 = c0;
    sa.eot = eot;
    sa.live_sum = bs.live_sum.p; sa.fin_tok = bs.fin_tok.p; sa.fin_sum = bs.fin_sum.p; sa.fin_len = bs.fin_len.p;
    sa.n_fin = bs.n_fin.p; sa.done = bs.done.p; sa.parent = dparent.p; sa.token = dtoken.p;
    wt::launch_beam_select(sa, st);
    wt::BeamReorderArgs ra;  // the id rows only, as after decode_beam's last step
    ra.src_rows = src_rows; ra.dst_rows = dst_rows; ra.cap = 32; ra.d = 4; ra.slabs = 0; ra.pos = pos; ra.V = V;
    ra.ids_src = dids.p; ra.ids_dst = dnext.p; ra.parent = dparent.p; ra.token = dtoken.p;
    wt::launch_beam_reorder(ra, st);
    h->impl->sync();
    bs.live_sum.to_host(live_sum);
    bs.fin_tok.to_host(fin_tok);
    bs.fin_sum.to_host(fin_sum);
    bs.fin_len.to_host(fin_len);
    bs.n_fin.to_host(n_fin);
    bs.done.to_host(done);
    dparent.to_host(parent);
    dtoken.to_host(reinterpret_cast<long long*>(token));
    dnext.to_host(reinterpret_cast<long long*>(ids_next));
  });
}

namespace {
// device mirror of a wt_dbg_beam_full_args
struct DevBeamFull {
  static constexpr size_t C = wt::kBeamClipsMax, S = wt::kBeamMax;
  const wt_dbg_beam_full_args& a;
  size_t live, rows, chunks, stride, cap;
  DevArr<float> logits;
  DevArr<wt::BeamFullPart> part;
  DevArr<long long> ids, ids_next;
  DevArr<float> lp, lp_next;
  DevArr<unsigned char> anc, anc_next;
  DevArr<wt::TsState> ts;
  DevArr<int> n_live, fin_tok, fin_len, n_fin, done, parent, out_n, out_len;
  DevArr<double> live_sum, fin_sum, lse, out_sum;
  DevArr<float> fin_lp, tok_lp, out_lp;
  DevArr<long long> token, out_ids;
  static size_t live_rows(const wt_dbg_beam_full_args& a) { return size_t(a.pos + 1 == a.n_prompt ? a.clips : a.K * a.clips); }
  explicit DevBeamFull(const wt_dbg_beam_full_args& a_)
      : a(a_), live(live_rows(a_)), rows(size_t(a_.K) * a_.clips), chunks(size_t(wt::beam_chunks(a_.V))), stride(size_t(a_.stride)),
        cap(size_t(a_.cap)),
        logits(live * a_.ldl, a_.logits), part(live * chunks),
        ids(live * stride, reinterpret_cast<const long long*>(a_.ids)), ids_next(rows * stride, reinterpret_cast<const long long*>(a_.ids_next)),
        lp(live * stride, a_.lp), lp_next(rows * stride, a_.lp_next), anc(live * cap, a_.anc), anc_next(rows * cap, a_.anc_next),
        ts(128, reinterpret_cast<const wt::TsState*>(a_.ts_state)), n_live(C, a_.n_live), fin_tok(C * S * stride, a_.fin_tok),
        fin_len(C * S, a_.fin_len), n_fin(C, a_.n_fin), done(C, a_.done), parent(rows), out_n(C, a_.out_n), out_len(C, a_.out_len),
        live_sum(C * S, a_.live_sum), fin_sum(C * S, a_.fin_sum), lse(live, a_.lse), out_sum(C, a_.out_sum),
        fin_lp(C * S * stride, a_.fin_lp), tok_lp(rows), out_lp(C * stride, a_.out_lp), token(rows),
        out_ids(C * stride, reinterpret_cast<const long long*>(a_.out_ids)) {}
  wt::BeamFullArgs args() const {
    wt::BeamFullArgs x;
    x.clips = a.clips; x.K = a.K; x.c0 = a.c0; x.pos = a.pos; x.n_prompt = a.n_prompt; x.V = a.V; x.ldl = a.ldl;
    x.stride = a.stride; x.cap = a.cap; x.eot = a.eot; x.beg = a.beg; x.max_initial = a.max_initial; x.timestamps = a.timestamps;
    x.logits = logits.p; x.part = part.p; x.ids_src = ids.p; x.ids_dst = ids_next.p; x.lp_src = lp.p; x.lp_dst = lp_next.p;
    x.anc_src = anc.p; x.anc_dst = anc_next.p; x.ts = ts.p; x.n_live = n_live.p; x.live_sum = live_sum.p;
    x.fin_tok = fin_tok.p; x.fin_lp = fin_lp.p; x.fin_sum = fin_sum.p; x.fin_len = fin_len.p; x.n_fin = n_fin.p; x.done = done.p;
    x.parent = parent.p; x.token = token.p; x.tok_lp = tok_lp.p; x.dbg_lse = a.lse ? lse.p : nullptr;
    x.out_ids = out_ids.p; x.out_lp = out_lp.p; x.out_n = out_n.p; x.out_len = out_len.p; x.out_sum = out_sum.p;
    return x;
  }
  void state_to_host() const {
    ts.to_host(reinterpret_cast<wt::TsState*>(a.ts_state));
    n_live.to_host(a.n_live);
    live_sum.to_host(a.live_sum);
    fin_tok.to_host(a.fin_tok);
    fin_lp.to_host(a.fin_lp);
    fin_sum.to_host(a.fin_sum);
    fin_len.to_host(a.fin_len);
    n_fin.to_host(a.n_fin);
    done.to_host(a.done);
  }
};
bool beam_full_args_ok(const wt_dbg_beam_full_args* a) {
  return a && a->K >= 1 && a->clips >= 1 && size_t(a->K) * a->clips <= 128 && a->V >= 1 && a->ldl >= a->V && a->stride >= 1 &&
         a->cap >= 1 && a->stride <= 4096 && a->cap <= 4096 && a->ids && a->lp && a->ts_state && a->n_live && a->live_sum &&
         a->fin_tok && a->fin_lp && a->fin_sum && a->fin_len && a->n_fin && a->done;
}
}  // namespace

int wt_dbg_beam_full_step(wt_engine* h, const wt_dbg_beam_full_args* a) {
  if (!h || !beam_full_args_ok(a) || !a->logits || !a->anc || !a->parent || !a->token || !a->tok_lp || !a->ids_next ||
      !a->lp_next || !a->anc_next) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    hipStream_t st = h->impl->stream();
    DevBeamFull dv(*a);
    wt::BeamFullArgs x = dv.args();
    if (a->begin) {  // the chain's start writes the prompt's ancestor entries into the rows the first step reads
      wt::BeamFullArgs b = x;
      b.anc_dst = dv.anc.p;
      wt::launch_beam_full_begin(b, st);
    }
    wt::launch_beam_full_partial(x, st);
    wt::launch_beam_full_select(x, st);
    wt::launch_beam_full_advance(x, st);
    h->impl->sync();
    dv.state_to_host();
    dv.parent.to_host(a->parent);
    dv.token.to_host(reinterpret_cast<long long*>(a->token));
    dv.tok_lp.to_host(a->tok_lp);
    dv.ids_next.to_host(reinterpret_cast<long long*>(a->ids_next));
    dv.lp_next.to_host(a->lp_next);
    dv.anc_next.to_host(a->anc_next);
    dv.lse.to_host(a->lse);
    if (a->part_stats || a->part_keys) {
      std::vector<wt::BeamFullPart> hp(dv.part.n);
      dv.part.to_host(hp.data());
      const size_t kk = size_t(a->K) + 1;
      for (size_t i = 0; i < hp.size(); ++i) {
        if (a->part_stats) {
          float* o = a->part_stats + i * 4;
          o[0] = hp[i].mt, o[1] = hp[i].st, o[2] = hp[i].ms, o[3] = hp[i].ss;
        }
        for (size_t r = 0; a->part_keys && r < kk; ++r) {
          a->part_keys[(i * 2 + 0) * kk + r] = hp[i].kt[r];
          a->part_keys[(i * 2 + 1) * kk + r] = hp[i].ks[r];
        }
      }
    }
  });
}

int wt_dbg_beam_full_finalize(wt_engine* h, const wt_dbg_beam_full_args* a) {
  if (!h || !beam_full_args_ok(a) || !a->out_ids || !a->out_lp || !a->out_n || !a->out_len || !a->out_sum) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    // (the rows handed in are the K * clips rows after the last advance, whatever the step)
    wt_dbg_beam_full_args b = *a;
    b.logits = nullptr, b.anc = nullptr, b.ids_next = nullptr, b.lp_next = nullptr, b.anc_next = nullptr, b.lse = nullptr;
    const size_t rows = size_t(a->K) * a->clips, stride = size_t(a->stride);
    DevBeamFull dv(b);
    DevArr<long long> ids(rows * stride, reinterpret_cast<const long long*>(a->ids));
    DevArr<float> lp(rows * stride, a->lp);
    wt::BeamFullArgs x = dv.args();
    x.ids_src = ids.p, x.lp_src = lp.p;
    wt::launch_beam_full_finalize(x, h->impl->stream());
    h->impl->sync();
    dv.state_to_host();
    dv.out_ids.to_host(reinterpret_cast<long long*>(a->out_ids));
    dv.out_lp.to_host(a->out_lp);
    dv.out_n.to_host(a->out_n);
    dv.out_len.to_host(a->out_len);
    dv.out_sum.to_host(a->out_sum);
  });
}

int wt_dbg_beam_reorder(wt_engine* h, int src_rows, int dst_rows, int cap, int d, int slabs, int pos, int V,
                        const float* kv_src, float* kv_dst, const int64_t* ids_src, int64_t* ids_dst,
                        const int32_t* parent, const int64_t* token) {
  if (!h || !ids_src || !ids_dst || !parent || !token || src_rows < 1 || dst_rows < 1 || cap < 1 || d < 1 || slabs < 0 ||
      src_rows > 128 || dst_rows > 128 || (slabs > 0 && (!kv_src || !kv_dst))) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t row = size_t(cap) * d;
    DevArr<float> dsrc(slabs > 0 ? size_t(slabs) * src_rows * row : 0, kv_src);
    DevArr<float> ddst(slabs > 0 ? (size_t(slabs) * dst_rows + 1) * row : 0, kv_dst);
    DevArr<long long> dids_src(size_t(src_rows) * 32, reinterpret_cast<const long long*>(ids_src));
    DevArr<long long> dids_dst(size_t(128) * 32, reinterpret_cast<const long long*>(ids_dst));
    DevArr<int> dparent(dst_rows, parent);
    DevArr<long long> dtoken(dst_rows, reinterpret_cast<const long long*>(token));
    wt::BeamReorderArgs ra;
    ra.kv_src = slabs > 0 ? dsrc.p : nullptr; ra.kv_dst = slabs > 0 ? ddst.p : nullptr;
    ra.src_rows = src_rows; ra.dst_rows = dst_rows; ra.cap = cap; ra.d = d; ra.slabs = slabs; ra.pos = pos; ra.V = V;
    ra.ids_src = dids_src.p; ra.ids_dst = dids_dst.p; ra.parent = dparent.p; ra.token = dtoken.p;
    wt::launch_beam_reorder(ra, h->impl->stream());
    h->impl->sync();
    if (slabs > 0) ddst.to_host(kv_dst);
    dids_dst.to_host(reinterpret_cast<long long*>(ids_dst));
  });
}

int wt_dbg_beam_finalize(wt_engine* h, int K, int clips, int c0, int pos, int n_prompt, const int64_t* ids,
                         const float* live_sum, int32_t* fin_tok, float* fin_sum, int32_t* fin_len, int32_t* n_fin,
                         const int32_t* done, int64_t* out_ids, int32_t* out_n, float* out_sum, int32_t* out_len) {
  if (!h || !ids || !live_sum || !fin_tok || !fin_sum || !fin_len || !n_fin || !done || !out_ids || !out_n || !out_sum ||
      !out_len || K < 1 || clips < 1 || size_t(K) * clips > 128) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    constexpr size_t C = wt::kBeamClipsMax;
    DevArr<long long> dids(size_t(K) * clips * 32, reinterpret_cast<const long long*>(ids));
    DevBeamState bs(live_sum, fin_tok, fin_sum, fin_len, n_fin, done);
    DevArr<long long> dout(C * 32, reinterpret_cast<const long long*>(out_ids));
    DevArr<int> dn(C, out_n), dlen(C, out_len);
    DevArr<float> dsum(C, out_sum);
    wt::BeamFinalArgs fa;
    fa.ids = dids.p; fa.clips = clips; fa.K = K; fa.c0 = c0; fa.pos = pos; fa.n_prompt = n_prompt;
    fa.live_sum = bs.live_sum.p; fa.fin_tok = bs.fin_tok.p; fa.fin_sum = bs.fin_sum.p; fa.fin_len = bs.fin_len.p;
    fa.n_fin = bs.n_fin.p; fa.done = bs.done.p;
    fa.out_ids = dout.p; fa.out_n = dn.p; fa.out_sum = dsum.p; fa.out_len = dlen.p;
    wt::launch_beam_finalize(fa, h->impl->stream());
    h->impl->sync();
    bs.fin_tok.to_host(fin_tok);
    bs.fin_sum.to_host(fin_sum);
    bs.fin_len.to_host(fin_len);
    bs.n_fin.to_host(n_fin);
    dout.to_host(reinterpret_cast<long long*>(out_ids));
    dn.to_host(out_n);
    dsum.to_host(out_sum);
    dlen.to_host(out_len);
  });
}

// ------------------------------------------- the greedy step's tail, kernel by kernel ---
int wt_dbg_dec_gemm_ksplit(wt_engine* h, int bf16, int M, int B, int N, int K, const float* X, const float* W,
                           const float* bias, float* R, float* Y, float* part) {
  if (!h || !X || !W || !bias || !R || !Y || !part || B < 1 || M < B || M > 128 || M % B != 0 || N < 1 || K < 1) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const bool bf = bf16 != 0;
    const DevTiled dW(W, N, K, bf);
    const size_t mn = size_t(M) * N;
    DevArr<float> dX(size_t(M) * K, X), dB(N, bias), dR(mn, R), dY(mn, Y), dP(mn, part);
    wt::DecGemmArgs g;  // the engine's fc2 with fc2_ksplit = 2: out of place, second K-half into `part`
    g.bf16 = bf;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = B; g.M = M; g.X = dX.p; g.ldx = K;
    g.bias = dB.p; g.R = dR.p; g.Y = dY.p; g.ldy = N; g.ksplit = 2; g.part = dP.p;
    wt::launch_dec_gemm(g, wt::kProNone, wt::kDecResid, h->impl->stream());
    h->impl->sync();
    dR.to_host(R);
    dY.to_host(Y);
    dP.to_host(part);
  });
}

int wt_dbg_dec_ln_gemm_rows(wt_engine* h, int bf16, int M, int B, int N, int K, const float* xin, const float* xpart,
                            const int64_t* ids, int ids_stride, int pos, const float* tok_emb, const float* pos_emb,
                            int n_vocab, int n_pos, const float* ln_g, const float* ln_b, const float* W, const float* bias,
                            int gelu, float* Y, float* xout) {
  if (!h || !ln_g || !ln_b || !W || !bias || !Y || !xout || B < 1 || M < B || M > 128 || M % B != 0 || N < 1 ||
      (K != 128 && K != 384 && K != 512) || (ids ? (xin || xpart) : !xin)) {
    return WT_ERR_INVALID_ARG;
  }
  const int np = M / B;
  if (ids && (!tok_emb || !pos_emb || n_vocab < 1 || pos < 0 || pos + np > ids_stride || pos + np > n_pos)) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const bool bf = bf16 != 0;
    const DevTiled dW(W, N, K, bf);
    const size_t mk = size_t(M) * K;
    DevArr<float> dxin(xin ? mk : 0, xin), dxp(xpart ? mk : 0, xpart);
    DevArr<long long> dids(ids ? size_t(B) * ids_stride : 0, reinterpret_cast<const long long*>(ids));
    DevArr<float> dtok(ids ? size_t(n_vocab) * K : 0, tok_emb), dpos(ids ? size_t(n_pos) * K : 0, pos_emb);
    DevArr<float> dg(K, ln_g), db(K, ln_b), dB(N, bias), dY(size_t(M) * N);
    DevArr<float> dxo(mk + K, xout);  // [M + 1][K]: the last row is a guard the kernel must not write
    wt::DecGemmArgs g;
    g.bf16 = bf;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = B; g.M = M;
    g.ln_g = dg.p; g.ln_b = db.p; g.xout = dxo.p;
    if (ids) {  // LNMODE 2: row p * B + b = tok_emb[ids[b][pos + p]] + pos_emb[pos + p]
      g.ids = dids.p; g.ids_stride = ids_stride; g.pos = pos; g.tok_emb = dtok.p; g.pos_emb = dpos.p; g.n_vocab = n_vocab;
    } else {    // LNMODE 0 (xin) or 3 (xin + xpart)
      g.xin = dxin.p; g.xpart = xpart ? dxp.p : nullptr;
    }
    g.bias = dB.p; g.Y = dY.p; g.ldy = N;
    wt::launch_dec_gemm(g, wt::kProLn, gelu ? wt::kDecBiasGelu : wt::kDecBias, h->impl->stream());
    h->impl->sync();
    dY.to_host(Y);
    dxo.to_host(xout);
  });
}

int wt_dbg_dec_logits(wt_engine* h, int bf16, int M, int V, int K, const float* xin, const float* xpart, const float* ln_g,
                      const float* ln_b, const float* E, int blocks, float* logits, uint64_t* records) {
  if (!h || !xin || !ln_g || !ln_b || !E || !records || M < 1 || M > 128 || V < 1 || blocks < 0 ||
      (K != 128 && K != 384 && K != 512)) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const bool bf = bf16 != 0;
    const int n_tiles = (V + 31) / 32;
    const DevTiled dE(E, V, K, bf);
    const size_t mk = size_t(M) * K;
    DevArr<float> dxin(mk, xin), dxp(xpart ? mk : 0, xpart), dg(K, ln_g), db(K, ln_b);
    // [M + 1][V] and [M + 1][n_tiles]: the last row of each is a guard the kernel must not write
    DevArr<float> dY(logits ? (size_t(M) + 1) * V : 0, logits);
    DevArr<unsigned long long> dBest((size_t(M) + 1) * n_tiles, reinterpret_cast<const unsigned long long*>(records));
    wt::DecGemmArgs g;  // the engine's final LayerNorm + logits + argmax records
    g.bf16 = bf;
    g.logits_blocks = blocks;
    g.Wt = dE.w(); g.w_scale = dE.scale; g.N = V; g.K = K; g.B = M; g.M = M;
    g.xin = dxin.p; g.xpart = xpart ? dxp.p : nullptr; g.ln_g = dg.p; g.ln_b = db.p;
    g.Y = logits ? dY.p : nullptr; g.ldy = V; g.best = dBest.p;
    wt::launch_dec_gemm(g, wt::kProLn, wt::kDecLogits, h->impl->stream());
    h->impl->sync();
    if (logits) dY.to_host(logits);
    dBest.to_host(reinterpret_cast<unsigned long long*>(records));
  });
}

int wt_dbg_select_token(wt_engine* h, int B, int n_tiles, const uint64_t* records, int64_t* ids, int stride, int pos,
                        int32_t* n_ids, int32_t* finished, int64_t eot, int stop_at_eot, int keep_ids) {
  if (!h || !records || !ids || !n_ids || !finished || B < 1 || n_tiles < 1 || pos < 0 || pos + 1 >= stride) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    DevArr<unsigned long long> dRec(size_t(B) * n_tiles, reinterpret_cast<const unsigned long long*>(records));
    DevArr<long long> dids(size_t(B) * stride, reinterpret_cast<const long long*>(ids));
    DevArr<int> dn(B, n_ids), dfin(B, finished);
    wt::launch_select_token(dRec.p, n_tiles, dids.p, stride, pos, dn.p, dfin.p, eot, stop_at_eot, B, h->impl->stream(),
                            keep_ids != 0);
    h->impl->sync();
    dids.to_host(reinterpret_cast<long long*>(ids));
    dn.to_host(n_ids);
    dfin.to_host(finished);
  });
}

int wt_dbg_timestamp_select(wt_engine* h, int B, int V, const float* logits, const int64_t* ids, int ids_stride,
                            const int32_t* n_ids, int sample_begin, int eot, int beg, int max_initial_timestamp,
                            int64_t* token, double* L, float* M) {
  if (!h || !logits || !ids || !n_ids || !token || B < 1 || B > 64 || V < 2 || ids_stride < 1 || sample_begin < 0) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    for (int b = 0; b < B; ++b) {
      if (n_ids[b] < sample_begin || n_ids[b] > ids_stride) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_timestamp_select: n_ids outside [sample_begin, ids_stride]");
    }
    const int ldl = (V + 3) & ~3, stride = ids_stride + 1;  // the kernel writes the token at ids[b][n_ids[b]]
    std::vector<long long> rows = widen_ids(ids, B, ids_stride, n_ids, 0);
    DevArr<float> dlog(pad_logits(logits, B, V, ldl));
    DevArr<long long> dids(rows);
    DevArr<int> dn(B, n_ids), dfin(B);
    DevArr<wt::TsPart> dpart(size_t(B) * wt::ts_chunks(V));
    DevArr<wt::TsState> dstate(B);
    DevArr<double> dL(B);
    DevArr<float> dM(B);
    dfin.zero(h->impl->stream());
    wt::launch_ts_state_init(dids.p, stride, dn.p, 0, sample_begin, V, beg, dstate.p, B, h->impl->stream());
    for_equal_runs(n_ids, B, [&](int b0, int count) {
      wt::TsSelectArgs t;
      t.logits = dlog.p + size_t(b0) * ldl; t.ldl = ldl; t.V = V; t.batch = count;
      t.eot = eot; t.beg = beg; t.max_initial = max_initial_timestamp;
      t.n_gen = n_ids[b0] - sample_begin; t.part = dpart.p + size_t(b0) * wt::ts_chunks(V); t.state = dstate.p + b0;
      t.ids = dids.p + size_t(b0) * stride; t.ids_stride = stride; t.pos = n_ids[b0] - 1; t.stop_at_eot = 1;
      t.n_ids = dn.p + b0; t.finished = dfin.p + b0;
      t.dbg_L = dL.p + b0; t.dbg_M = dM.p + b0;
      wt::launch_ts_select(t, h->impl->stream());
    });
    h->impl->sync();
    dids.to_host(rows.data());
    for (int b = 0; b < B; ++b) token[b] = rows[size_t(b) * stride + n_ids[b]];
    if (L) dL.to_host(L);
    if (M) dM.to_host(M);
  });
}

int wt_dbg_sample_select(wt_engine* h, int B, int V, const float* logits, const int64_t* ids, int ids_stride,
                         const int32_t* n_ids, int sample_begin, int timestamps, int eot, int beg, int max_initial_timestamp,
                         const float* temperature, uint64_t seed, int attempt, int clip_base, int pos, int64_t* token,
                         double* L, float* M, float* key) {
  if (!h || !logits || !ids || !n_ids || !token || !temperature || B < 1 || B > wt::kSampleClipsMax || V < 2 ||
      ids_stride < 1 || sample_begin < 1 || attempt < 0 || clip_base < 0) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    wt::SampleParams prm{};
    prm.seed_lo = unsigned(seed & 0xffffffffull), prm.seed_hi = unsigned(seed >> 32);
    prm.attempt = unsigned(attempt), prm.clip_base = unsigned(clip_base);
    for (int b = 0; b < B; ++b) {
      if (n_ids[b] < sample_begin || n_ids[b] > ids_stride) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_sample_select: n_ids outside [sample_begin, ids_stride]");
      if (!(temperature[b] >= 0.0f) || std::isinf(temperature[b])) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_sample_select: a temperature is negative or not finite");
      prm.inv_t[b] = temperature[b] > 0.0f ? 1.0f / temperature[b] : 0.0f;
    }
    const int ldl = (V + 3) & ~3, stride = ids_stride + 1;  // the kernel writes the token at ids[b][n_ids[b]]
    std::vector<long long> rows = widen_ids(ids, B, ids_stride, n_ids, 0);
    DevArr<float> dlog(pad_logits(logits, B, V, ldl));
    DevArr<long long> dids(rows);
    DevArr<int> dn(B, n_ids), dfin(B);
    DevArr<wt::SamplePart> dpart(size_t(B) * wt::ts_chunks(V));
    DevArr<wt::TsState> dstate(B);
    DevArr<wt::SampleParams> dprm(1, &prm);
    DevArr<double> dL(B);
    DevArr<float> dM(B), dK(B);
    dfin.zero(h->impl->stream());
    if (timestamps) wt::launch_ts_state_init(dids.p, stride, dn.p, 0, sample_begin, V, beg, dstate.p, B, h->impl->stream());
    for_equal_runs(n_ids, B, [&](int b0, int count) {
      wt::SampleArgs t;
      t.logits = dlog.p + size_t(b0) * ldl; t.ldl = ldl; t.V = V; t.batch = count;
      t.eot = eot; t.beg = beg; t.max_initial = max_initial_timestamp;
      t.n_gen = n_ids[b0] - sample_begin; t.part = dpart.p + size_t(b0) * wt::ts_chunks(V);
      t.state = timestamps ? dstate.p + b0 : nullptr;
      t.params = dprm.p; t.row0 = b0; t.rng_pos = pos;
      t.ids = dids.p + size_t(b0) * stride; t.ids_stride = stride; t.pos = n_ids[b0] - 1; t.stop_at_eot = 1;
      t.n_ids = dn.p + b0; t.finished = dfin.p + b0;
      t.dbg_L = dL.p + b0; t.dbg_M = dM.p + b0; t.dbg_key = dK.p + b0;
      wt::launch_sample_select(t, h->impl->stream());
    });
    h->impl->sync();
    dids.to_host(rows.data());
    for (int b = 0; b < B; ++b) token[b] = rows[size_t(b) * stride + n_ids[b]];
    if (L) dL.to_host(L);
    if (M) dM.to_host(M);
    if (key) dK.to_host(key);
  });
}

int wt_dbg_sample_select_group(wt_engine* h, int B, int group, int V, const float* logits, const int64_t* ids, int ids_stride,
                               int n_ids, int sample_begin, int timestamps, int eot, int beg, int max_initial_timestamp,
                               const float* temperature, uint64_t seed, int attempt, int clip_base, int row0, int pos,
                               int64_t* token, double* L, float* M, float* key) {
  if (!h || !logits || !ids || !token || !temperature || B < 1 || group < 1 || V < 2 || ids_stride < 1 || sample_begin < 1 ||
      attempt < 0 || clip_base < 0 || row0 < 0 || n_ids < sample_begin || n_ids > ids_stride) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const int clips = (B + group - 1) / group;
    // (the launcher refuses what the parameter block cannot hold; the block is filled for the clips it can)
    wt::SampleParams prm{};
    prm.seed_lo = unsigned(seed & 0xffffffffull), prm.seed_hi = unsigned(seed >> 32);
    prm.attempt = unsigned(attempt), prm.clip_base = unsigned(clip_base);
    for (int c = 0; c < clips && row0 + c < wt::kSampleClipsMax; ++c) {
      if (!(temperature[c] >= 0.0f) || std::isinf(temperature[c])) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_sample_select_group: a temperature is negative or not finite");
      prm.inv_t[row0 + c] = temperature[c] > 0.0f ? 1.0f / temperature[c] : 0.0f;
    }
    if (B > 4 * wt::kSampleRowsMax) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_sample_select_group: too many rows");
    const int ldl = (V + 3) & ~3, stride = ids_stride + 1;  // the kernel writes the token at ids[b][n_ids]
    std::vector<int32_t> n(size_t(B), n_ids);
    std::vector<long long> rows = widen_ids(ids, B, ids_stride, n.data(), 0);
    DevArr<float> dlog(pad_logits(logits, B, V, ldl));
    DevArr<long long> dids(rows);
    DevArr<int> dn(B, n.data()), dfin(B);
    DevArr<wt::SamplePart> dpart(size_t(B) * wt::ts_chunks(V));
    DevArr<wt::TsState> dstate(B);
    DevArr<wt::SampleParams> dprm(1, &prm);
    DevArr<double> dL(B);
    DevArr<float> dM(B), dK(B);
    dfin.zero(h->impl->stream());
    if (timestamps) wt::launch_ts_state_init(dids.p, stride, dn.p, 0, sample_begin, V, beg, dstate.p, B, h->impl->stream());
    wt::SampleArgs t;
    t.logits = dlog.p; t.ldl = ldl; t.V = V; t.batch = B; t.group = group;
    t.eot = eot; t.beg = beg; t.max_initial = max_initial_timestamp;
    t.n_gen = n_ids - sample_begin; t.part = dpart.p;
    t.state = timestamps ? dstate.p : nullptr;
    t.params = dprm.p; t.row0 = row0; t.rng_pos = pos;
    t.ids = dids.p; t.ids_stride = stride; t.pos = n_ids - 1; t.stop_at_eot = 1;
    t.n_ids = dn.p; t.finished = dfin.p;
    t.dbg_L = dL.p; t.dbg_M = dM.p; t.dbg_key = dK.p;
    wt::launch_sample_select(t, h->impl->stream());
    h->impl->sync();
    dids.to_host(rows.data());
    for (int b = 0; b < B; ++b) token[b] = rows[size_t(b) * stride + n_ids];
    if (L) dL.to_host(L);
    if (M) dM.to_host(M);
    if (key) dK.to_host(key);
  });
}

int wt_dbg_best_of_begin(wt_engine* h, int clips, int N, int n_prompt, int stride, int cap, const int32_t* frozen,
                         int64_t* ids, int32_t* n_ids, int32_t* finished, double* sum, int32_t* count, uint8_t* anc) {
  if (!h || !ids || !n_ids || !finished || !sum || !count || !anc || clips < 1 || N < 1 || stride < 1 || cap < 1 ||
      clips > 4 * wt::kSampleRowsMax || N > 4 * wt::kSampleRowsMax) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t R = size_t(N) * clips;
    static_assert(sizeof(long long) == sizeof(int64_t), "id rows");
    DevArr<long long> dids(R * stride, reinterpret_cast<const long long*>(ids));
    DevArr<int> dn(R, n_ids), dfin(R, finished), dcount(R, count), dfrozen(size_t(clips), frozen);
    DevArr<double> dsum(R, sum);
    DevArr<unsigned char> danc(R * cap, anc);
    wt::BestOfArgs a;
    a.clips = clips; a.N = N; a.n_prompt = n_prompt; a.stride = stride; a.cap = cap;
    a.ids = dids.p; a.n_ids = dn.p; a.finished = dfin.p; a.sum = dsum.p; a.count = dcount.p;
    a.frozen = frozen ? dfrozen.p : nullptr; a.anc = danc.p;
    wt::launch_best_of_begin(a, h->impl->stream());
    h->impl->sync();
    dids.to_host(reinterpret_cast<long long*>(ids));
    dn.to_host(n_ids), dfin.to_host(finished), dcount.to_host(count), dsum.to_host(sum), danc.to_host(anc);
  });
}

int wt_dbg_best_of_pick(wt_engine* h, int clips, int N, int c0, int n_out, int stride, const int64_t* ids, const float* lp,
                        const int32_t* n_ids, const double* sum, const int32_t* count, int64_t* out_ids, float* out_lp,
                        int32_t* out_n, double* out_sum, int32_t* out_count, int32_t* picked, double* all_sum,
                        int32_t* all_count) {
  if (!h || !ids || !lp || !n_ids || !sum || !count || !out_ids || !out_lp || !out_n || !out_sum || !out_count || !picked ||
      !all_sum || !all_count || clips < 1 || N < 1 || stride < 2 || c0 < 0 || n_out < 1 || n_out > wt::kSampleClipsMax ||
      clips > 4 * wt::kSampleRowsMax || N > 4 * wt::kSampleRowsMax) {
    return WT_ERR_INVALID_ARG;
  }
  if (c0 + clips > n_out) return WT_ERR_INVALID_ARG;  // (the output rows the kernel may write are the caller's arrays)
  return guarded(h, [&] {
    const size_t R = size_t(N) * clips, O = size_t(n_out), G = wt::kSampleGroupMax;
    DevArr<long long> dids(R * stride, reinterpret_cast<const long long*>(ids)), doids(O * stride, reinterpret_cast<const long long*>(out_ids));
    DevArr<float> dlp(R * stride, lp), dolp(O * stride, out_lp);
    DevArr<int> dn(R, n_ids), dcount(R, count), don(O, out_n), docount(O, out_count), dpicked(O, picked), dacount(O * G, all_count);
    DevArr<double> dsum(R, sum), dosum(O, out_sum), dasum(O * G, all_sum);
    wt::BestOfArgs a;
    a.clips = clips; a.N = N; a.c0 = c0; a.n_prompt = 1; a.stride = stride; a.cap = stride - 1;
    a.ids = dids.p; a.lp = dlp.p; a.n_ids = dn.p; a.sum = dsum.p; a.count = dcount.p;
    a.out_ids = doids.p; a.out_lp = dolp.p; a.out_n = don.p; a.out_count = docount.p; a.picked = dpicked.p;
    a.out_sum = dosum.p; a.all_sum = dasum.p; a.all_count = dacount.p;
    wt::launch_best_of_pick(a, h->impl->stream());
    h->impl->sync();
    doids.to_host(reinterpret_cast<long long*>(out_ids));
    dolp.to_host(out_lp), don.to_host(out_n), docount.to_host(out_count), dpicked.to_host(picked);
    dosum.to_host(out_sum), dasum.to_host(all_sum), dacount.to_host(all_count);
  });
}

int wt_dbg_token_scores(wt_engine* h, int B, int V, const float* logits, const int64_t* ids, int ids_stride,
                        const int32_t* n_ids, int sample_begin, int timestamps, int eot, int beg, int max_initial_timestamp,
                        const int32_t* live, float* lp, double* sum, int32_t* count, double* den) {
  if (!h || !logits || !ids || !n_ids || !live || !lp || !sum || !count || B < 1 || B > 64 || V < 2 || ids_stride < 1 ||
      sample_begin < 0) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    for (int b = 0; b < B; ++b) {
      if (n_ids[b] < sample_begin + 1 || n_ids[b] > ids_stride) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_token_scores: n_ids outside [sample_begin + 1, ids_stride]");
    }
    // device rows are the caller's behind one more leading column, so that the chosen id (the last of the row) sits at
    // pos + 1 with pos = n_ids[b] - 1 >= 0 even when it is the only id
    const int ldl = (V + 3) & ~3, stride = ids_stride + 1, sb = sample_begin + 1;
    std::vector<int> n_after(B);  // what the selection kernel leaves where the clip was live: pos + 2
    for (int b = 0; b < B; ++b) n_after[b] = live[b] ? n_ids[b] + 1 : 0;
    DevArr<float> dlog(pad_logits(logits, B, V, ldl)), dlp(size_t(B) * stride);
    DevArr<long long> dids(widen_ids(ids, B, ids_stride, n_ids, 1));
    DevArr<int> dn0(B, n_ids), dn1(n_after), dcount(B, count);  // dn0: the device row's ids before the chosen one
    DevArr<double> dsum(B, sum), dden(B);
    DevArr<wt::ScorePart> dpart(size_t(B) * wt::ts_chunks(V));
    DevArr<wt::TsState> dstate(B);
    hipStream_t st = h->impl->stream();
    dlp.zero(st);
    if (timestamps) wt::launch_ts_state_init(dids.p, stride, dn0.p, 0, sb, V, beg, dstate.p, B, st);
    for_equal_runs(n_ids, B, [&](int b0, int rows) {
      wt::ScoreArgs a;
      a.logits = dlog.p + size_t(b0) * ldl; a.ldl = ldl; a.V = V; a.batch = rows;
      a.state = timestamps ? dstate.p + b0 : nullptr; a.eot = eot; a.beg = beg; a.max_initial = max_initial_timestamp;
      a.n_gen = n_ids[b0] - 1 - sample_begin; a.part = dpart.p + size_t(b0) * wt::ts_chunks(V);
      a.ids = dids.p + size_t(b0) * stride; a.ids_stride = stride; a.pos = n_ids[b0] - 1; a.n_ids = dn1.p + b0;
      a.token_logprob = dlp.p + size_t(b0) * stride; a.lp_stride = stride; a.sum = dsum.p + b0; a.count = dcount.p + b0;
      a.dbg_den = dden.p + b0;
      wt::launch_score_partial(a, st);
      wt::launch_score_finish(a, st);
    });
    h->impl->sync();
    std::vector<float> hlp(size_t(B) * stride);
    dlp.to_host(hlp.data());
    for (int b = 0; b < B; ++b) lp[b] = hlp[size_t(b) * stride + n_ids[b]];
    dsum.to_host(sum);
    dcount.to_host(count);
    if (den) dden.to_host(den);
  });
}

int wt_dbg_language_head(wt_engine* h, int rows, int d, int n_vocab, int lang_lo, int n_lang, int forced_lang, const float* x,
                         const float* xpart, const float* ln_g, const float* ln_b, const float* tok_emb, float* probs,
                         int32_t* lang, float* lang_prob, int64_t* ids, int ids_stride) {
  if (!h || !x || !ln_g || !ln_b || !tok_emb || !probs || !lang || !lang_prob || rows < 1 || rows > 128 || d < 1 ||
      d > wt::kLangMaxD || n_vocab < 1 || n_vocab > 4096 || lang_lo < 0 || n_lang < 1 || n_lang > wt::kLangMax ||
      lang_lo + n_lang > n_vocab || forced_lang >= n_lang || (ids && ids_stride < 2)) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t rd = size_t(rows) * d;
    DevArr<float> dx(rd, x), dxp(xpart ? rd : 0, xpart), dg(d, ln_g), db(d, ln_b), demb(size_t(n_vocab) * d, tok_emb);
    DevArr<float> dprobs(size_t(rows) * n_lang), dprob(rows);
    DevArr<int> dlang(rows);
    DevArr<long long> dids(ids ? size_t(rows) * ids_stride : 0, reinterpret_cast<const long long*>(ids));
    wt::LanguageHeadArgs a;
    a.x = dx.p; a.xpart = xpart ? dxp.p : nullptr; a.ln_g = dg.p; a.ln_b = db.p; a.tok_emb = demb.p;
    a.rows = rows; a.d = d; a.n_vocab = n_vocab; a.lang_lo = lang_lo; a.n_lang = n_lang;
    a.probs = dprobs.p; a.lang = dlang.p; a.lang_prob = dprob.p; a.forced_lang = forced_lang;
    if (ids) a.ids = dids.p, a.ids_stride = ids_stride, a.id_pos = 1;
    wt::launch_language_head(a, h->impl->stream());
    h->impl->sync();
    dprobs.to_host(probs);
    dprob.to_host(lang_prob);
    dlang.to_host(lang);
    if (ids) dids.to_host(reinterpret_cast<long long*>(ids));
  });
}

int wt_dbg_language_head_rows(wt_engine* h, int clips, int x_rows, int x_rows_per_clip, int d, int n_vocab, int lang_lo,
                              int n_lang, const float* x, const float* xpart, const float* ln_g, const float* ln_b,
                              const float* tok_emb, const uint32_t* allow, const int32_t* hold, float* probs, int32_t* lang,
                              float* lang_prob, int64_t* ids0, int64_t* ids1, int ids_rows, int ids_stride, int id_pos,
                              int fan) {
  // what the copies below need; shapes, ranges and the id rows are the launcher's to refuse
  if (!h || !x || !ln_g || !ln_b || !tok_emb || !probs || !lang || !lang_prob || clips < 1 || clips > 128 || x_rows < 1 ||
      x_rows > 1024 || d < 1 || d > 4096 || n_vocab < 1 || n_vocab > 4096 || n_lang < 1 || n_lang > 1024 ||
      ((ids0 || ids1) && (ids_rows < 1 || ids_rows > 4096 || ids_stride < 1 || ids_stride > 4096))) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t rd = size_t(x_rows) * d, ni = size_t(ids_rows) * ids_stride;
    DevArr<float> dx(rd, x), dxp(xpart ? rd : 0, xpart), dg(d, ln_g), db(d, ln_b), demb(size_t(n_vocab) * d, tok_emb);
    DevArr<float> dprobs(size_t(clips) * n_lang, probs), dprob(clips, lang_prob);
    DevArr<int> dlang(clips, lang), dhold(hold ? clips : 0, hold);
    DevArr<unsigned> dallow(allow ? 4 : 0, allow);
    DevArr<long long> di0(ids0 ? ni : 0, reinterpret_cast<const long long*>(ids0));
    DevArr<long long> di1(ids1 ? ni : 0, reinterpret_cast<const long long*>(ids1));
    wt::LanguageRowsArgs a;
    a.x = dx.p; a.xpart = xpart ? dxp.p : nullptr; a.ln_g = dg.p; a.ln_b = db.p; a.tok_emb = demb.p;
    a.clips = clips; a.x_rows = x_rows; a.x_rows_per_clip = x_rows_per_clip; a.d = d; a.n_vocab = n_vocab;
    a.lang_lo = lang_lo; a.n_lang = n_lang; a.allow = allow ? dallow.p : nullptr; a.hold = hold ? dhold.p : nullptr;
    a.probs = dprobs.p; a.lang = dlang.p; a.lang_prob = dprob.p;
    if (ids0) a.ids[0] = di0.p, a.ids_rows[0] = ids_rows, a.ids_stride[0] = ids_stride;
    if (ids1) a.ids[1] = di1.p, a.ids_rows[1] = ids_rows, a.ids_stride[1] = ids_stride;
    a.id_pos = id_pos; a.fan = fan;
    wt::launch_language_head_rows(a, h->impl->stream());
    h->impl->sync();
    dprobs.to_host(probs);
    dprob.to_host(lang_prob);
    dlang.to_host(lang);
    if (ids0) di0.to_host(reinterpret_cast<long long*>(ids0));
    if (ids1) di1.to_host(reinterpret_cast<long long*>(ids1));
  });
}

int wt_dbg_cross_absorbed_chain(wt_engine* h, int bf16, int batch, int heads, int T, int chunks, int nq, int split, int n_src,
                                const float* const* E_src, const float* qp, const float* wv, const float* bv, int mode,
                                int p0_only, int nq_only, float* out, float* ws) {
  if (!h || !wv || !bv || !out || !ws || batch < 1 || heads < 1 || heads > 8 || T < 1 || nq < 1 || chunks < 1 || chunks > 16 ||
      size_t(nq) * batch > 128 || mode < 0 || mode > 2) {
    return WT_ERR_INVALID_ARG;
  }
  if (mode != 2) {
    if (!qp || !E_src || n_src < 1 || n_src > 4 || split < 1 || split > batch || (n_src == 1 && split != batch)) return WT_ERR_INVALID_ARG;
    for (int i = 0; i < n_src; ++i)
      if (!E_src[i]) return WT_ERR_INVALID_ARG;
    // a single launch must stay inside the nq positions ws and qp were sized for
    if (mode == 1 && (p0_only < 0 || nq_only < 1 || p0_only + nq_only > nq)) return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const bool bf = bf16 != 0;
    const size_t d = size_t(heads) * 64, rows = size_t(nq) * batch, clip = size_t(T) * d;
    const std::vector<float> wvt = wt::cross_q_layout(wv, int(d));
    DevArr<float> dwv(wvt), dbv(d, bv), dq(mode != 2 ? rows * heads * d : 0, qp);
    // [rows + 1][...]: the last row of each is a guard the kernels must not write
    DevArr<float> dws((rows + 1) * heads * chunks * (d + 4), ws), dout((rows + 1) * d, out);
    hipStream_t st = h->impl->stream();
    // Every source is an allocation of its own with room for `batch` clips at ONE plane stride; the clips a group does
    // not have hold NaN halfs, so a wrong source or clip offset reads poison instead of some other clip's bytes.
    const size_t plane = size_t(batch) * clip + 64;
    std::vector<std::unique_ptr<DevArr<unsigned short>>> src;
    float se = 1.0f;
    if (mode != 2) {
      const auto clips_of = [&](int i) { return std::max(0, std::min(split, batch - i * split)); };
      float mx = 0.0f;
      for (int i = 0; i < n_src; ++i) mx = std::max(mx, max_abs(E_src[i], size_t(clips_of(i)) * clip));
      se = bf ? 1.0f : wt::f16_scale_for(mx);  // one scale for all sources, as the engine's sc_cross_kv_
      for (int i = 0; i < n_src; ++i) {
        const size_t n = size_t(clips_of(i)) * clip;
        src.push_back(std::make_unique<DevArr<unsigned short>>(bf ? to_bf16(E_src[i], n, plane - n, 0x7FC0)
                                                                  : to_f16_planes(E_src[i], n, se, plane - n, 0x7E00)));
      }
      const int nq_max = wt::cross_absorbed_max_nq(heads);
      const auto launch = [&](int p0, int n) {
        wt::CrossAbsorbedArgs a;
        a.qp = dq.p; a.e = src[0]->p; a.e_plane = long(plane); a.e_scale = se; a.ws = dws.p; a.bf16 = bf;
        if (n_src > 1) {
          a.split = split;
          a.e2 = src[1]->p;
          if (n_src > 2) a.e3 = src[2]->p;
          if (n_src > 3) a.e4 = src[3]->p;
        }
        a.batch = batch; a.heads = heads; a.d_model = int(d); a.T = T; a.chunks = chunks; a.nq = n; a.p0 = p0;
        wt::launch_cross_absorbed(a, st);
      };
      if (mode == 1) {
        launch(p0_only, nq_only);
      } else {
        for (int p0 = 0; p0 < nq; p0 += nq_max) launch(p0, std::min(nq_max, nq - p0));  // Engine::decode's loop
      }
    }
    wt::launch_cross_absorbed_combine(dws.p, dwv.p, dbv.p, dout.p, int(rows), heads, chunks, int(d), st);
    h->impl->sync();
    dout.to_host(out);
    dws.to_host(ws);
  });
}

int wt_dbg_absorbed_query_matrix(int heads, int d, const float* wq, const float* bq, const float* wk, float* A, float* av) {
  if (heads < 1 || d != heads * 64 || !wq || !bq || !wk || !A || !av) return WT_ERR_INVALID_ARG;
  return guarded(nullptr, [&] {
    std::vector<float> Am, am;
    wt::absorbed_query_matrix(wq, bq, wk, heads, d, &Am, &am);
    std::memcpy(A, Am.data(), Am.size() * sizeof(float));
    std::memcpy(av, am.data(), am.size() * sizeof(float));
  });
}

// --- the log-mel front end, kernel by kernel (tests/test_gpu_frontend_kernels.py) ---

}  // extern "C"

namespace {
// a partial-maximum word of log_clipmax (order-preserving bits of a float; 0 = no block wrote it) -> the float
float clip_max_word_value(unsigned o) {
  if (o == 0u) return -std::numeric_limits<float>::infinity();
  const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// device words [(b * kClipMaxWays + w) * kClipMaxStride] -> words [B][kClipMaxWays] (+ their values)
void clip_max_to_host(const unsigned* d_words, int B, uint32_t* words, float* maxima) {
  std::vector<unsigned> host(size_t(B) * wt::kClipMaxWays * wt::kClipMaxStride);
  hipchk(hipMemcpy(host.data(), d_words, host.size() * sizeof(unsigned), hipMemcpyDeviceToHost), "D2H clip_max");
  for (size_t i = 0; i < size_t(B) * wt::kClipMaxWays; ++i) {
    if (words) words[i] = host[i * wt::kClipMaxStride];
    if (maxima) maxima[i] = clip_max_word_value(host[i * wt::kClipMaxStride]);
  }
}
}  // namespace

extern "C" {

int wt_dbg_frontend_dims(wt_engine* h, int32_t out[8]) {
  if (!h || !out) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const wt::Engine& e = *h->impl;
    const wt::Engine::FrontendView v = e.frontend_view();
    if (v.dft_n == 0) throw wt::Error(WT_ERR_FORMAT, "vocab file carries no 80x201 mel filter bank");
    const int32_t d[8] = {e.mel_frames(), int32_t(e.pcm_elems()), int32_t(v.pcm_stride), v.pw_ld, v.mel_n, v.mel_k, v.dft_n, v.dft_k};
    std::memcpy(out, d, sizeof(d));
  });
}

int wt_dbg_frontend_stages(wt_engine* h, int batch, const float* pcm, int valid_frames, float* mel, float* planes,
                           uint16_t* hi, uint16_t* lo, float* pw, float* melacc, float* raw, uint32_t* words, float* maxima,
                           float* basis, float* mel_matrix) {
  if (!h || !pcm || !mel || batch < 1 || valid_frames < -1 || valid_frames > h->impl->mel_frames()) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    const size_t nb = size_t(batch), T0 = size_t(e.mel_frames());
    float* d_mel = e.staging_mel(batch);
    DevArr<float> d_raw(nb * e.mel_elems());
    e.logmel(e.upload_pcm(pcm, batch), batch, d_mel, valid_frames, d_raw.p);
    e.sync();
    const wt::Engine::FrontendView v = e.frontend_view();
    hipchk(hipMemcpy(mel, d_mel, nb * e.mel_elems() * sizeof(float), hipMemcpyDeviceToHost), "D2H mel");
    if (raw) d_raw.to_host(raw, nb * e.mel_elems());
    if (planes || hi || lo) {
      const size_t n = nb * size_t(v.pcm_stride);
      std::vector<unsigned short> hl(2 * n);  // hi [n] then lo [n]
      hipchk(hipMemcpy(hl.data(), v.pcm_planes, n * 2, hipMemcpyDeviceToHost), "D2H pcm hi");
      hipchk(hipMemcpy(hl.data() + n, v.pcm_planes + v.pcm_plane, n * 2, hipMemcpyDeviceToHost), "D2H pcm lo");
      if (hi) std::memcpy(hi, hl.data(), n * 2);
      if (lo) std::memcpy(lo, hl.data() + n, n * 2);
      if (planes) from_f16_planes(hl.data(), n, n, v.pcm_scale, planes);
    }
    if (pw) hipchk(hipMemcpy(pw, v.pw, nb * T0 * size_t(v.pw_ld) * sizeof(float), hipMemcpyDeviceToHost), "D2H pw");
    if (melacc) hipchk(hipMemcpy(melacc, v.melacc, nb * T0 * size_t(v.mel_n) * sizeof(float), hipMemcpyDeviceToHost), "D2H melacc");
    if (words || maxima) clip_max_to_host(v.clip_max, batch, words, maxima);
    if (basis) std::memcpy(basis, v.basis, size_t(v.dft_n) * v.dft_k * sizeof(float));
    if (mel_matrix) std::memcpy(mel_matrix, v.mel_matrix, size_t(v.mel_n) * v.mel_k * sizeof(float));
  });
}

int wt_dbg_log_clipmax(wt_engine* h, int B, int T, int n_mel, int ld, int t_valid, const float* melacc, float* raw,
                       uint32_t* words, float* maxima) {
  if (!h || !melacc || !raw || B < 1 || T < 1 || n_mel < 1 || ld < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    DevArr<float> din(size_t(B) * T * ld, melacc), dout(size_t(B) * n_mel * T);
    DevArr<unsigned> dmax(size_t(B) * wt::kClipMaxWays * wt::kClipMaxStride);
    dmax.zero(h->impl->stream());  // as Engine::logmel clears them
    wt::launch_log_clipmax(din.p, ld, dout.p, dmax.p, B, n_mel, T, h->impl->stream(), t_valid);
    h->impl->sync();
    dout.to_host(raw);
    clip_max_to_host(dmax.p, B, words, maxima);
  });
}

int wt_dbg_mel_normalize(wt_engine* h, int B, int T, int n_mel, const uint32_t* words, float* logmel) {
  if (!h || !words || !logmel || B < 1 || T < 1 || n_mel < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    DevArr<float> dx(size_t(B) * n_mel * T, logmel);
    std::vector<unsigned> host(size_t(B) * wt::kClipMaxWays * wt::kClipMaxStride, 0u);
    for (size_t i = 0; i < size_t(B) * wt::kClipMaxWays; ++i) host[i * wt::kClipMaxStride] = words[i];
    DevArr<unsigned> dmax(host.size(), host.data());
    wt::launch_mel_normalize(dx.p, dmax.p, B, n_mel, T, h->impl->stream());
    h->impl->sync();
    dx.to_host(logmel);
  });
}

int wt_dbg_mel_transpose(wt_engine* h, int planes, int B, int C, int T, int ld, float scale, const float* mel, void* out) {
  if (!h || !mel || !out || planes < 0 || planes > 2 || B < 1 || C < 1 || T < 1 || ld < 1 || (planes == 0 && ld != C)) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t n = size_t(B) * (size_t(T) + 2) * ld;
    DevArr<float> din(size_t(B) * C * T, mel);
    if (planes == 0) {
      DevArr<float> dout(n, static_cast<const float*>(out));
      wt::launch_mel_transpose(din.p, dout.p, B, C, T, h->impl->stream());
      h->impl->sync();
      dout.to_host(static_cast<float*>(out));
    } else {
      DevArr<unsigned short> dout(planes == 1 ? 2 * n : n, static_cast<const unsigned short*>(out));
      wt::launch_mel_transpose_planes(din.p, dout.p, planes == 1 ? long(n) : 0, planes == 1 ? scale : 1.0f, B, C, T, ld,
                                      h->impl->stream(), planes == 2);
      h->impl->sync();
      dout.to_host(static_cast<unsigned short*>(out));
    }
  });
}

int wt_dbg_pcm_to_planes(wt_engine* h, int batch, int n, int out_stride, int guard, float scale, float limit, const float* pcm,
                         uint16_t* planes) {
  if (!h || !pcm || !planes || batch < 1 || n < 1 || out_stride < 1 || guard < 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t plane = size_t(batch) * out_stride + guard;
    DevArr<float> din(size_t(batch) * n, pcm);
    DevArr<unsigned short> dout(2 * plane, planes);
    wt::launch_pcm_to_planes(din.p, dout.p, long(plane), scale, limit, batch, long(n), long(out_stride), h->impl->stream());
    h->impl->sync();
    dout.to_host(planes);
  });
}

}  // extern "C"

namespace {
// one past the last element that rows 0 .. M - 1 of `width` elements reach when row m starts at
// (m / rpb) * bs + (m % rpb) * ld: the last row, or the last row of the last whole group of rpb rows
long rows_extent(int M, int rpb, long bs, long ld, long width) {
  const long last = long((M - 1) / rpb) * bs + long((M - 1) % rpb) * ld;
  const long whole = M >= rpb ? long(M / rpb - 1) * bs + long(rpb - 1) * ld : 0;
  return std::max(last, whole) + width;
}
}  // namespace

extern "C" {

int wt_dbg_gemm_addressed(wt_engine* h, int kind, int epi, int M, int N, int K, const float* A, long a_len, int a_rpb,
                          long a_bs, int lda, const float* W, const float* bias, const float* pos, int pos_period,
                          int out_format, void* out, long c_len, long c_off, int c_rpb, long c_bs, int ldc,
                          const float* out_scale, int seg, int kv_batch, int kv_heads, int kv_dmodel, int n_cu) {
  if (!h || !A || !W || !out || kind < 0 || kind > 2 || M < 1 || N < 1 || K < 1 || a_rpb < 1 || a_bs < 0 || lda < 0 ||
      c_rpb < 1 || c_bs < 0 || ldc < 0 || c_off < 0 || c_len < 1 || n_cu < 0 || seg < 0 || ((epi & wt::kEpiBias) && !bias) ||
      ((epi & wt::kEpiPos) && (!pos || pos_period < 1)) || (out_format != 0 && out_format != kind) ||
      (out_format == 1 && !out_scale)) {
    return WT_ERR_INVALID_ARG;
  }
  // nothing is launched over operands or an output the buffers do not hold, or at an address the 16-byte accesses of
  // the kernels cannot take; what the launchers check themselves (rows per clip, multiples of 8, segments) is left to them
  if (a_len < rows_extent(M, a_rpb, a_bs, lda, K)) return WT_ERR_INVALID_ARG;
  const bool kv = (epi & wt::kEpiKvLayout) != 0;
  if (kv) {
    if (kv_batch < 1 || kv_heads < 1 || kv_dmodel != 64 * kv_heads || N % kv_dmodel != 0 || long(kv_batch) * c_rpb < M ||
        c_off + long(N / kv_dmodel) * kv_batch * kv_heads * c_rpb * 64 > c_len) {
      return WT_ERR_INVALID_ARG;
    }
  } else if (c_off + rows_extent(M, c_rpb, c_bs, ldc, N) > c_len) {
    return WT_ERR_INVALID_ARG;
  }
  const int align = out_format == 0 ? 4 : 8;
  if (c_off % align != 0 || (out_format == 1 && c_len % 8 != 0) ||
      (kind == 0 && (lda % 4 != 0 || a_bs % 4 != 0 || ldc % 4 != 0 || c_bs % 4 != 0))) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    DevArr<float> dB(N, bias), dP(pos ? size_t(pos_period) * N : 0, pos);
    hipStream_t st = h->impl->stream();
    if (kind == 0) {
      DevArr<float> dA(size_t(a_len) + 64), dC(size_t(c_len), static_cast<const float*>(out));
      // (cleared on the launch's own stream: it does not wait for the null stream, and hipMemset may return early)
      hipchk(hipMemsetAsync(dA.p + a_len, 0, 64 * sizeof(float), st), "memset");
      hipchk(hipMemcpy(dA.p, A, size_t(a_len) * sizeof(float), hipMemcpyHostToDevice), "H2D");
      DevArr<float> dW(size_t(N) * K, W);
      wt::GemmArgs g;
      g.A = dA.p; g.a_rpb = a_rpb; g.a_bs = a_bs; g.lda = lda; g.W = dW.p; g.bias = dB.p;
      g.C = dC.p + c_off; g.R = g.C; g.c_rpb = c_rpb; g.c_bs = c_bs; g.ldc = ldc;
      g.pos = dP.p; g.pos_period = pos_period > 0 ? pos_period : 1;
      g.kv_batch = kv_batch; g.kv_heads = kv_heads; g.kv_dmodel = kv_dmodel;
      g.M = M; g.N = N; g.K = K; g.variant = int(h->impl->gemm_variant);
      wt::launch_gemm(g, epi, st);
      h->impl->sync();
      dC.to_host(static_cast<float*>(out));
      return;
    }
    wt::PlaneGemmArgs g;
    g.a_rpb = a_rpb; g.a_bs = a_bs; g.lda = lda; g.bias = dB.p;
    g.c_rpb = c_rpb; g.c_bs = c_bs; g.ldc = ldc; g.pos = dP.p; g.pos_period = pos_period > 0 ? pos_period : 1;
    g.kv_batch = kv_batch; g.kv_heads = kv_heads; g.kv_dmodel = kv_dmodel;
    g.M = M; g.N = N; g.K = K; g.n_cu = n_cu;
    DevArr<float> dC(out_format == 0 ? size_t(c_len) : 0, static_cast<const float*>(out));
    DevArr<unsigned short> dO(out_format == 1 ? 2 * size_t(c_len) : out_format == 2 ? size_t(c_len) : 0,
                              static_cast<const unsigned short*>(out));
    if (out_format == 0) {
      g.C = dC.p + c_off; g.R = g.C;
    } else {
      g.P = dO.p + c_off; g.p_plane = c_len; g.seg = seg;
      if (out_format == 1) g.out_scale[0] = out_scale[0], g.out_scale[1] = out_scale[1], g.out_scale[2] = out_scale[2];
    }
    if (kind == 1) {
      const float sa = wt::f16_scale_for(max_abs(A, size_t(a_len))), sw = wt::f16_scale_for(max_abs(W, size_t(N) * K));
      const DevPlanes dA(A, size_t(a_len), sa);
      const DevArr<unsigned short> dW(weight_planes(W, N, K, sw));
      g.A = dA.ptr(); g.a_plane = dA.plane; g.W = dW.p; g.a_scale = sa; g.w_scale = sw;
      wt::launch_gemm_planes(g, epi, st);
      h->impl->sync();
    } else {
      const DevBf16 dA(A, size_t(a_len)), dW(W, size_t(N) * K);
      g.A = dA.ptr(); g.W = dW.ptr();
      wt::launch_gemm_bf16_planes(g, epi, st);
      h->impl->sync();
    }
    if (out_format == 0) dC.to_host(static_cast<float*>(out)); else dO.to_host(static_cast<unsigned short*>(out));
  });
}

int wt_dbg_plane_gemm_plan(int family, int M, int N, int K, int epi, int planes_out, int ln, int n_cu, int c_rpb, int ldc,
                           int32_t plan[4]) {
  if (!plan || family < 0 || family > 1 || M < 1 || N < 1 || K < 1 || n_cu < 0) return WT_ERR_INVALID_ARG;
  if (family == 0) {
    const int mode = wt::plane_gemm_mode();
    const wt::PlaneGemmPlan p = wt::plane_gemm_plan(M, N, K, epi, planes_out != 0, ln != 0, n_cu, mode);
    plan[0] = p.tile; plan[1] = p.schedule; plan[2] = p.fused ? 1 : 0; plan[3] = mode;
  } else {
    const wt::Bf16GemmPlan p = wt::bf16_gemm_plan(M, N, epi, planes_out != 0, ln != 0, c_rpb, ldc);
    plan[0] = p.bn; plan[1] = p.bm; plan[2] = p.whole_row ? 1 : 0; plan[3] = 0;
  }
  return WT_OK;
}

int wt_dbg_gemm_ln_fused(wt_engine* h, int family, int epi, int M, int N, int K, const float* A, long a_len, int a_rpb, long a_bs,
                         int lda, const float* W, const float* bias, const float* pos, int pos_period, const float* ln_g,
                         const float* ln_b, float ln_scale, int n_cu, int guard_rows, int c_rpb, long c_bs, int ldc, float* C,
                         uint16_t* planes, float* ln_y32, uint16_t* p_out, int32_t* flag, int32_t* fused) {
  const int kmul = family == 0 ? 32 : 64;
  if (!h || !A || !W || !C || !planes || !flag || !fused || family < 0 || family > 1 || M < 1 || N < 128 || N % 128 != 0 || K < kmul ||
      K % kmul != 0 || guard_rows < 256 || a_rpb < 1 || a_bs < 0 || lda < 0 || c_rpb < 1 || c_bs < 0 || ldc < 0 || n_cu < 0 ||
      (epi != (wt::kEpiBias | wt::kEpiResidual) && epi != (wt::kEpiBias | wt::kEpiGelu | wt::kEpiPos)) || !bias ||
      ((epi & wt::kEpiPos) && (!pos || pos_period < 1))) {
    return WT_ERR_INVALID_ARG;
  }
  // nothing is launched over an operand or an output the buffers do not hold; every output has M + guard_rows rows, a
  // whole tile more than the launch owns, so that a store to any row of the last tile still lands inside it
  const size_t cells = size_t(M + guard_rows) * N;
  if (a_len < rows_extent(M, a_rpb, a_bs, lda, K) || rows_extent(M, c_rpb, c_bs, ldc, N) > long(cells)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    DevArr<float> dB(N, bias), dP(pos ? size_t(pos_period) * N : 0, pos), dG(ln_g ? N : 0, ln_g), dS(ln_b ? N : 0, ln_b),
        dC(cells, C), dY(ln_y32 ? cells : 0, ln_y32);
    DevArr<unsigned short> dL((family == 0 ? 2 : 1) * cells, planes), dO(p_out ? (family == 0 ? 2 : 1) * cells : 0, p_out);
    DevArr<int> dF(1);
    hipStream_t st = h->impl->stream();
    dF.zero(st);  // as the engine clears its flag
    wt::PlaneGemmArgs g;
    g.a_rpb = a_rpb; g.a_bs = a_bs; g.lda = lda; g.bias = dB.p;
    g.C = dC.p; g.R = dC.p; g.c_rpb = c_rpb; g.c_bs = c_bs; g.ldc = ldc;  // the residual in place, as the engine runs it
    g.pos = dP.p; g.pos_period = pos_period > 0 ? pos_period : 1;
    g.M = M; g.N = N; g.K = K; g.n_cu = n_cu;
    g.ln_g = ln_g ? dG.p : nullptr; g.ln_b = ln_b ? dS.p : nullptr; g.ln_P = dL.p; g.ln_plane = long(cells); g.ln_scale = ln_scale;
    g.ln_y32 = ln_y32 ? dY.p : nullptr; g.nonfinite = dF.p;
    if (p_out) { g.P = dO.p; g.p_plane = long(cells); }
    bool did = false;
    if (family == 0) {
      const float sa = wt::f16_scale_for(max_abs(A, size_t(a_len))), sw = wt::f16_scale_for(max_abs(W, size_t(N) * K));
      const DevPlanes dA(A, size_t(a_len), sa);
      const DevArr<unsigned short> dW(weight_planes(W, N, K, sw));
      g.A = dA.ptr(); g.a_plane = dA.plane; g.W = dW.p; g.a_scale = sa; g.w_scale = sw;
      did = wt::launch_gemm_planes(g, epi, st);
      h->impl->sync();
    } else {
      const DevBf16 dA(A, size_t(a_len)), dW(W, size_t(N) * K);
      g.A = dA.ptr(); g.W = dW.ptr();
      did = wt::launch_gemm_bf16_planes(g, epi, st);
      h->impl->sync();
    }
    dC.to_host(C);
    dL.to_host(planes);
    dY.to_host(ln_y32);
    if (p_out) dO.to_host(p_out);
    dF.to_host(flag);
    *fused = did ? 1 : 0;
  });
}

int wt_dbg_layernorm_planes(wt_engine* h, int M, int d, const float* x, const float* g, const float* b, float scale, int bf16,
                            int guard, uint16_t* planes, float* y32, int32_t* nonfinite) {
  if (!h || !x || !g || !b || !planes || M < 1 || d < 1 || guard < 0 || guard % 4 != 0 || !(scale > 0.0f)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t plane = size_t(M) * d + guard;
    DevArr<float> dx(size_t(M) * d, x), dg(size_t(d), g), db(size_t(d), b), dy(y32 ? plane : 0, y32);
    DevArr<unsigned short> dout(bf16 ? plane : 2 * plane, planes);
    DevArr<int> dflag(1);
    dflag.zero(h->impl->stream());  // as the engine clears its flag
    wt::launch_layernorm_planes(dx.p, dout.p, bf16 ? 0 : long(plane), scale, y32 ? dy.p : nullptr, dg.p, db.p, M, d,
                                h->impl->stream(), nonfinite ? dflag.p : nullptr, bf16 != 0);
    h->impl->sync();
    dout.to_host(planes);
    dy.to_host(y32);
    if (nonfinite) dflag.to_host(nonfinite);
  });
}

int wt_dbg_f32_to_planes(wt_engine* h, int M, int ld, const float* x, const float* scales, int seg, int guard,
                         uint16_t* planes) {
  if (!h || !x || !scales || !planes || M < 0 || ld < 1 || seg < 0 || guard < 0 || guard % 4 != 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t plane = size_t(M) * ld + guard;
    DevArr<float> dx(size_t(M) * ld, x);
    DevArr<unsigned short> dout(2 * plane, planes);
    wt::launch_f32_to_planes(dx.p, dout.p, long(plane), M, ld, scales, seg, h->impl->stream());
    h->impl->sync();
    dout.to_host(planes);
  });
}

int wt_dbg_encoder_scales(wt_engine* h, float* rec, int cap, int* n) {
  if (!h || !n || cap < 0 || (cap && !rec)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const std::vector<std::array<float, 10>> r = h->impl->encoder_scales();
    *n = int(r.size());
    for (size_t i = 0; i < r.size() && i < size_t(cap); ++i) std::copy(r[i].begin(), r[i].end(), rec + 10 * i);
  });
}

float wt_dbg_f16_scale_for(float bound) { return wt::f16_scale_for(bound); }

int wt_dbg_gemm_planes_scaled(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias, int epi,
                              float a_scale, float w_scale, const float out_scale[3], int seg, int n_cu, int planes_out,
                              int guard_rows, void* out) {
  const bool epi_ok = planes_out ? (epi == wt::kEpiBias || epi == (wt::kEpiBias | wt::kEpiGelu))
                                 : (epi == wt::kEpiBias || epi == (wt::kEpiBias | wt::kEpiGelu) || epi == (wt::kEpiBias | wt::kEpiResidual));
  if (!h || !A || !W || !bias || !out || !out_scale || !epi_ok || M < 1 || N < 128 || N % 128 || K < 32 || K % 32 || n_cu < 0 ||
      guard_rows < 0 || seg < 0) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t cells = size_t(M + guard_rows) * N;
    const DevPlanes dA(A, size_t(M) * K, a_scale);  // no clamping: an element past fp16's range uploads as hi = inf, lo = -inf
    const DevArr<unsigned short> dW(weight_planes(W, N, K, w_scale));
    DevArr<float> dB(N, bias), dC(planes_out ? 0 : cells, static_cast<const float*>(out));
    DevArr<unsigned short> dO(planes_out ? 2 * cells : 0, static_cast<const unsigned short*>(out));
    wt::PlaneGemmArgs g;
    dense_gemm_args(g, M, N, K, dB.p, planes_out ? nullptr : dC.p, nullptr, 0);
    g.A = dA.ptr(); g.a_plane = dA.plane; g.W = dW.p; g.a_scale = a_scale; g.w_scale = w_scale; g.n_cu = n_cu;
    if (planes_out) {
      g.P = dO.p; g.p_plane = long(cells); g.seg = seg;
      g.out_scale[0] = out_scale[0]; g.out_scale[1] = out_scale[1]; g.out_scale[2] = out_scale[2];
    }
    wt::launch_gemm_planes(g, epi, h->impl->stream());
    h->impl->sync();
    if (planes_out) dO.to_host(static_cast<unsigned short*>(out)); else dC.to_host(static_cast<float*>(out));
  });
}

int wt_dbg_encoder_attention_at(wt_engine* h, int kind, int variant, int batch, int T, int heads, int guard_rows,
                                const float* qkv, const float scales[4], void* out) {
  if (!h || !qkv || !out || kind < 0 || kind > 2 || guard_rows < 0 || batch < 0 || T < 0 || heads < 0 || (kind == 1 && !scales)) {
    return WT_ERR_INVALID_ARG;
  }
  if (kind == 1) {
    for (int i = 0; i < 4; ++i) {
      int e = 0;
      if (!(scales[i] > 0.0f) || !std::isfinite(scales[i]) || std::frexp(scales[i], &e) != 0.5f) return WT_ERR_INVALID_ARG;
    }
  }
  // batch, T or heads of zero, and a variant it does not have, are the launcher's to refuse: it throws before it launches,
  // and nothing is downloaded behind a throw
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(batch) * T + guard_rows, n_in = rows * 3 * d, n_out = rows * d;
    hipStream_t st = h->impl->stream();
    if (kind == 0) {
      const DevArr<float> dQ(n_in, qkv), dO(n_out, static_cast<const float*>(out));
      wt::launch_encoder_attention(dQ.p, dO.p, batch, T, heads, variant, st);
      h->impl->sync();
      dO.to_host(static_cast<float*>(out));
    } else if (kind == 1) {
      const std::vector<float> scaled = scale_qkv(qkv, rows, d, kQ * scales[0], scales[1], scales[2]);
      const DevPlanes dQ(scaled.data(), n_in, 1.0f);
      const DevArr<unsigned short> dO(2 * n_out, static_cast<const unsigned short*>(out));
      wt::launch_encoder_attention_planes(dQ.ptr(), dQ.plane, dO.p, long(n_out), batch, T, heads, scales[0], scales[1],
                                          scales[2], scales[3], st);
      h->impl->sync();
      dO.to_host(static_cast<unsigned short*>(out));
    } else {
      const DevBf16 dQ(qkv, n_in);
      const DevArr<unsigned short> dO(n_out, static_cast<const unsigned short*>(out));
      wt::launch_encoder_attention_bf16(dQ.ptr(), dO.p, batch, T, heads, st);
      h->impl->sync();
      dO.to_host(static_cast<unsigned short*>(out));
    }
  });
}

int wt_dbg_f32_to_bf16(wt_engine* h, int n, int guard, const float* x, float* out) {
  if (!h || !x || !out || n < 1 || guard < 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevArr<float> dx(size_t(n), x);
    const DevBf16 dy(out, size_t(n) + size_t(guard), 0);  // as given: the guard cells must come back untouched
    wt::launch_f32_to_bf16(dx.p, dy.ptr(), long(n), h->impl->stream());
    h->impl->sync();
    dy.to_host(out, size_t(n) + size_t(guard));
  });
}

static int dbg_align_scores_impl(wt_engine* h, int batch, int H, int T, int np, int pos0, const float* qp, const float* E,
                                 int n_heads, const int32_t* head, const int32_t* slot, int heads_total, const int32_t* F,
                                 int L_max, int ld, float* W, int mode, bool bf) {
  if (!h || !qp || !E || !head || !slot || !F || !W || batch < 1 || batch > wt::kAlignClipsMax || H < 1 || T < 1 || np < 1 ||
      n_heads < 0 || n_heads > wt::kAlignLayerHeadsMax || heads_total < 1 || L_max < 1 || ld < 1) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t d = size_t(H) * 64, ne = size_t(batch) * T * d;
    const float se = bf ? 1.0f : wt::f16_scale_for(max_abs(E, ne));
    const DevArr<unsigned short> dE(bf ? to_bf16(E, ne, 64) : to_f16_planes(E, ne, se, 64));  // (bf16: ONE plane)
    DevArr<float> dq(size_t(np) * batch * H * d, qp), dW(size_t(batch) * heads_total * L_max * ld, W);
    wt::AlignScoresArgs a;
    a.qp = dq.p; a.e = dE.p; a.bf16 = bf;
    if (!bf) a.e_plane = long(ne + 64), a.e_scale = se;
    a.batch = batch; a.H = H; a.d_model = int(d); a.T = T; a.np = np; a.pos0 = pos0; a.n_heads = n_heads;
    for (int i = 0; i < n_heads; ++i) a.head[i] = head[i], a.slot[i] = slot[i];
    for (int b = 0; b < batch; ++b) a.F[b] = F[b];
    a.W = dW.p; a.heads_total = heads_total; a.L_max = L_max; a.ldw = ld; a.mode = mode;
    wt::launch_align_scores(a, h->impl->stream());
    h->impl->sync();
    dW.to_host(W);
  });
}
int wt_dbg_align_scores(wt_engine* h, int batch, int H, int T, int np, int pos0, const float* qp, const float* E, int n_heads,
                        const int32_t* head, const int32_t* slot, int heads_total, const int32_t* F, int L_max, int ld, float* W,
                        int mode) {
  return dbg_align_scores_impl(h, batch, H, T, np, pos0, qp, E, n_heads, head, slot, heads_total, F, L_max, ld, W, mode, false);
}
int wt_dbg_align_scores_bf16(wt_engine* h, int batch, int H, int T, int np, int pos0, const float* qp, const float* E, int n_heads,
                             const int32_t* head, const int32_t* slot, int heads_total, const int32_t* F, int L_max, int ld,
                             float* W, int mode) {
  return dbg_align_scores_impl(h, batch, H, T, np, pos0, qp, E, n_heads, head, slot, heads_total, F, L_max, ld, W, mode, true);
}

int wt_dbg_align_matrix(wt_engine* h, int clips, int heads, int L_max, int ld, int n_a, int N_max, const float* W,
                        const int32_t* L, const int32_t* F, float* C, float* stats) {
  if (!h || !W || !L || !F || !C || clips < 1 || heads < 1 || L_max < 1 || ld < 1 || n_a < 0 || N_max < 1) return WT_ERR_INVALID_ARG;
  for (int b = 0; b < clips; ++b) {
    if (L[b] < n_a + 2 || L[b] > L_max || F[b] < 1 || F[b] > ld || L[b] - n_a - 1 > N_max) return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t bh = size_t(clips) * heads;
    DevArr<float> dW(bh * L_max * ld, W), dC(size_t(clips) * N_max * ld, C), dS(bh * 2 * ld, stats);
    DevArr<int> dL(clips, L), dF(clips, F);
    wt::AlignMatrixArgs a;
    a.W = dW.p; a.clips = clips; a.heads = heads; a.L_max = L_max; a.ldw = ld;
    a.L = dL.p; a.F = dF.p; a.n_a = n_a; a.stats = dS.p; a.C = dC.p; a.N_max = N_max; a.ldc = ld;
    wt::launch_align_matrix(a, h->impl->stream());
    h->impl->sync();
    dC.to_host(C);
    dS.to_host(stats);
  });
}

int wt_dbg_align_dtw(wt_engine* h, int clips, int N_max, int ld, const float* C, const int32_t* N, const int32_t* F,
                     int32_t* jump, uint8_t* trace) {
  if (!h || !C || !N || !F || !jump || clips < 1 || N_max < 1 || ld < 1) return WT_ERR_INVALID_ARG;
  for (int b = 0; b < clips; ++b) {
    if (N[b] < 0 || N[b] > N_max || F[b] < 1 || F[b] > ld) return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t cells = size_t(clips) * N_max * ld;
    DevArr<float> dC(cells, C);
    DevArr<unsigned char> dT(cells, trace);
    DevArr<int> dN(clips, N), dF(clips, F), dJ(size_t(clips) * N_max, jump);
    wt::AlignDtwArgs a;
    a.C = dC.p; a.clips = clips; a.N_max = N_max; a.ldc = ld; a.N = dN.p; a.F = dF.p; a.trace = dT.p; a.jump = dJ.p;
    wt::launch_align_dtw(a, h->impl->stream());
    h->impl->sync();
    dJ.to_host(jump);
    dT.to_host(trace);
  });
}

int wt_dbg_suppress_logits(wt_engine* h, int rows, int V, int ldl, const float* logits, float* out, const int64_t* ids, int n,
                           const int64_t* first_ids, int n_first, int first) {
  if (!h || !logits || !out || (n > 0 && !ids) || (n_first > 0 && !first_ids)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    h->impl->bind_device();
    // a shape the launcher refuses allocates nothing of its size: the launcher itself is asked, and throws
    const bool ok = rows >= 1 && rows <= wt::kSuppressRowsMax && V >= 1 && ldl >= V && n >= 0 && n <= wt::kSuppressIdsMax &&
                    n_first >= 0 && n_first <= wt::kSuppressIdsMax;
    std::vector<int> list;  // the engine's buffer layout: the always-ids, then the first-ids; an id no int holds: none
    for (int i = 0; ok && i < n + n_first; ++i) {
      const int64_t id = i < n ? ids[i] : first_ids[i - n];
      list.push_back(id >= 0 && id <= std::numeric_limits<int>::max() ? int(id) : -1);
    }
    DevArr<float> dlog(ok ? size_t(rows) * size_t(ldl) : 0, ok ? logits : nullptr);
    DevArr<int> dids(list);
    wt::SuppressArgs u;
    u.logits = dlog.p; u.ldl = ldl; u.V = V; u.rows = rows; u.ids = dids.p; u.n = n; u.n_first = n_first; u.first = first;
    wt::launch_suppress_logits(u, h->impl->stream());
    h->impl->sync();
    dlog.to_host(out);
  });
}

int wt_dbg_set_alignment(wt_engine* h, int keep, int mode, int sub) {
  if (!h || keep > 1 || mode > 1 || sub > wt::kAlignClipsMax) return WT_ERR_INVALID_ARG;
  wt::Engine& e = *h->impl;
  if (keep >= 0) e.keep_alignment = keep;
  if (mode >= 0) e.align_mode = mode;
  if (sub >= 0) e.align_sub = sub;
  return WT_OK;
}

int wt_dbg_last_alignment(const wt_engine* h, int clip, int32_t dims[6], int64_t* row, float* W, float* C, int32_t* jump) {
  if (!h || clip < 0 || size_t(clip) >= h->impl->last.alignment.size()) return WT_ERR_INVALID_ARG;
  const wt::ClipAlignment& a = h->impl->last.alignment[size_t(clip)];
  if (dims) {
    const int32_t v[6] = {a.n_a, a.L, a.N, a.F, a.heads, a.T};
    std::memcpy(dims, v, sizeof(v));
  }
  if (row) std::copy(a.row.begin(), a.row.end(), row);
  if (W) std::copy(a.W.begin(), a.W.end(), W);
  if (C) std::copy(a.C.begin(), a.C.end(), C);
  if (jump) std::copy(a.jump.begin(), a.jump.end(), jump);
  return WT_OK;
}

}  // extern "C"
