#include "engine_internal.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "kernels.h"

namespace wt {

namespace {
size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }
}  // namespace

// ------------------------------------------------------------ weights ---

// W [N][K] -> two fp16 planes in MFMA-fragment order [ceil(N/32)][K/16][plane][64 lanes][8] (rows past N zero):
// lane (l & 31, l >> 5) of tile t, k-step s holds W[32t + (l & 31)][16s + 8(l >> 5) .. +7], so one wave-instruction
// of the decoder GEMM reads 1 KiB contiguous.  The planes are hi = fp16(w * scale), lo = fp16(w * scale - hi) with
// scale the power of two that puts max |W| into (8192, 16384]: 22 significand bits, same bytes as fp32.
std::vector<unsigned short> tile_weights_f16(const float* W, int N, int K, float* scale) {
  float mx = 0.0f;
  for (size_t i = 0; i < size_t(N) * K; ++i) mx = std::max(mx, std::fabs(W[i]));
  const float sc = f16_scale_for(mx);
  *scale = sc;
  const int n_tiles = (N + 31) / 32, steps = K / 16;
  std::vector<unsigned short> out(size_t(n_tiles) * steps * 1024, 0);
  for (int t = 0; t < n_tiles; ++t)
    for (int s = 0; s < steps; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int n = t * 32 + (lane & 31);
        if (n >= N) continue;
        const float* src = W + size_t(n) * K + 16 * s + 8 * (lane >> 5);
        unsigned short* hi = out.data() + (size_t(t) * steps + s) * 1024 + lane * 8;
        unsigned short* lo = hi + 512;
        for (int e = 0; e < 8; ++e) {
          const float v = src[e] * sc;
          const _Float16 h = static_cast<_Float16>(v);
          const _Float16 l = static_cast<_Float16>(v - static_cast<float>(h));
          std::memcpy(hi + e, &h, 2);
          std::memcpy(lo + e, &l, 2);
        }
      }
  return out;
}

namespace {
inline unsigned short bf16_rne(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return static_cast<unsigned short>((u >> 16) | 0x40u);  // NaN stays NaN
  u += 0x7FFFu + ((u >> 16) & 1u);
  return static_cast<unsigned short>(u >> 16);
}
}  // namespace

// bf16 storage mode: one bf16 plane in the decoder GEMM's fragment order [ceil(N/32)][K/16][64 lanes][8]
std::vector<unsigned short> tile_weights_bf16(const float* W, int N, int K) {
  const int n_tiles = (N + 31) / 32, steps = K / 16;
  std::vector<unsigned short> out(size_t(n_tiles) * steps * 512, 0);
  for (int t = 0; t < n_tiles; ++t)
    for (int s = 0; s < steps; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int n = t * 32 + (lane & 31);
        if (n >= N) continue;
        const float* src = W + size_t(n) * K + 16 * s + 8 * (lane >> 5);
        unsigned short* dst = out.data() + (size_t(t) * steps + s) * 512 + lane * 8;
        for (int e = 0; e < 8; ++e) dst[e] = bf16_rne(src[e]);
      }
  return out;
}

// bf16 storage mode: W [N][K] fp32 -> bf16 [N][Kpad], zero filled
std::vector<unsigned short> round_weights_bf16(const float* W, int N, int K, int Kpad) {
  std::vector<unsigned short> out(size_t(N) * Kpad, 0);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) out[size_t(n) * Kpad + k] = bf16_rne(W[size_t(n) * K + k]);
  return out;
}

// Wq [d][d] (row = output) -> [head][d / 4][64 outputs of the head][4 k]: thread (output j, k-quarter) of
// cross_attention_step reads 16 contiguous bytes per step and a wavefront 1 KiB
std::vector<float> cross_q_layout(const float* Wq, int d) {
  const int heads = d / 64, c4 = d / 4;
  std::vector<float> out(size_t(d) * d);
  for (int h = 0; h < heads; ++h)
    for (int c = 0; c < c4; ++c)
      for (int j = 0; j < 64; ++j)
        for (int e = 0; e < 4; ++e)
          out[((size_t(h) * c4 + c) * 64 + j) * 4 + e] = Wq[size_t(h * 64 + j) * d + 4 * c + e];
  return out;
}

const unsigned short* Engine::upload_planes(const float* W, int N, int K, int Kpad, float scale) {
  const std::vector<unsigned short> planes = split_weight_planes(W, N, K, Kpad, scale);
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, planes.size() * sizeof(unsigned short) + 256));
  allocations_.push_back(p);
  HIPCHK(hipMemcpy(p, planes.data(), planes.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  return static_cast<const unsigned short*>(p);
}

TiledW Engine::upload_tiled(const float* W, int N, int K) {
  TiledW t;
  const std::vector<unsigned short> planes = tile_weights_f16(W, N, K, &t.scale);
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, std::max<size_t>(planes.size(), 1) * sizeof(unsigned short)));
  allocations_.push_back(p);
  HIPCHK(hipMemcpy(p, planes.data(), planes.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  t.w = static_cast<const unsigned short*>(p);
  return t;
}

float* Engine::upload(const std::vector<float>& host) {
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, std::max<size_t>(host.size(), 1) * sizeof(float)));
  allocations_.push_back(p);
  if (!host.empty()) HIPCHK(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  return static_cast<float*>(p);
}

float* Engine::dalloc(size_t n_floats) {
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, std::max<size_t>(n_floats, 1) * sizeof(float)));
  return static_cast<float*>(p);
}

void* Engine::dev_zeroed_bytes(size_t bytes) {
  bytes = std::max<size_t>(bytes, 4);
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, bytes));
  allocations_.push_back(p);
  HIPCHK(hipMemset(p, 0, bytes));
  return p;
}

void* Engine::pinned_bytes(size_t bytes) {
  void* p = nullptr;
  HIPCHK(hipHostMalloc(&p, bytes, 0));
  pinned_.push_back(p);
  return p;
}

const float* Engine::dev(const std::string& name) const {
  auto it = tensors_.find(name);
  if (it == tensors_.end()) throw Error(3, "weight file: missing tensor " + name);
  return it->second;
}

namespace {
// A .wtw file mapped read-only: header checked, tensor table parsed into name -> (fp32 payload, element count).
struct WtwFile {
  void* map = MAP_FAILED;
  size_t bytes = 0;
  wtw::WtwHeader hdr{};
  std::map<std::string, std::pair<const float*, size_t>> host;

  explicit WtwFile(const std::string& path) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) throw Error(2, "Failed to open file: " + path);
    struct stat st;
    if (fstat(fd, &st) != 0 || size_t(st.st_size) < sizeof(wtw::WtwHeader)) {
      ::close(fd);
      throw Error(3, "weight file too small: " + path);
    }
    bytes = size_t(st.st_size);
    map = mmap(nullptr, bytes, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (map == MAP_FAILED) throw Error(2, "Failed to mmap file: " + path);
    try {
      const char* base = static_cast<const char*>(map);
      std::memcpy(&hdr, base, sizeof(hdr));
      if (hdr.magic != wtw::kMagic || hdr.version != wtw::kVersion || hdr.n_tensors > (1u << 20) ||
          size_t(hdr.table_offset) + size_t(hdr.n_tensors) * sizeof(wtw::WtwTensor) > bytes) {
        throw Error(3, "not a .wtw weight file: " + path);
      }
      const uint64_t file_bytes = uint64_t(bytes);
      for (uint32_t i = 0; i < hdr.n_tensors; ++i) {
        wtw::WtwTensor t;
        std::memcpy(&t, base + hdr.table_offset + size_t(i) * sizeof(t), sizeof(t));
        // overflow-safe range check; fp32 payloads are read in place, so they must be 4-byte aligned
        if (t.dtype != 0 || t.offset > file_bytes || t.nbytes > file_bytes - t.offset || t.offset % 4 != 0 || t.nbytes % 4 != 0) {
          throw Error(kErrFormat, "corrupt tensor table in " + path);
        }
        t.name[sizeof(t.name) - 1] = 0;
        host[t.name] = {reinterpret_cast<const float*>(base + t.offset), t.nbytes / sizeof(float)};
      }
    } catch (...) {
      munmap(map, bytes);
      throw;
    }
  }
  ~WtwFile() {
    if (map != MAP_FAILED) munmap(map, bytes);
  }
  WtwFile(const WtwFile&) = delete;
  WtwFile& operator=(const WtwFile&) = delete;
  const float* get(const std::string& n, size_t expect) const {
    auto it = host.find(n);
    if (it == host.end()) throw Error(3, "weight file: missing tensor " + n);
    if (it->second.second != expect) throw Error(3, "weight file: bad shape for " + n);
    return it->second.first;
  }
};

// A convolution weight [co][ci][3] in the implicit GEMM's order [co][kk * n_ci + ci]: the three taps of output frame t
// are three consecutive rows of the time-major padded input
std::vector<float> conv_gemm_order(const float* w, int n_co, int n_ci) {
  std::vector<float> r(size_t(n_co) * 3 * n_ci);
  for (int co = 0; co < n_co; ++co)
    for (int ci = 0; ci < n_ci; ++ci)
      for (int kk = 0; kk < 3; ++kk) r[size_t(co) * 3 * n_ci + kk * n_ci + ci] = w[(size_t(co) * n_ci + ci) * 3 + kk];
  return r;
}

// query | key | value of the self-attention `p` as one matrix [3d][d]
std::vector<float> fused_qkv_weight(const WtwFile& f, const std::string& p, int d) {
  const size_t dd = size_t(d) * d;
  std::vector<float> w(3 * dd);
  std::memcpy(w.data(), f.get(p + ".query.weight", dd), dd * 4);
  std::memcpy(w.data() + dd, f.get(p + ".key.weight", dd), dd * 4);
  std::memcpy(w.data() + 2 * dd, f.get(p + ".value.weight", dd), dd * 4);
  return w;
}

// all decoder layers' cross K/V projections act on the same encoder output: one matrix [layer][k|v][d][d]
std::vector<float> cross_kv_weight(const WtwFile& f, const wtw::Dims& c) {
  const size_t dd = size_t(c.n_text_state) * c.n_text_state;
  std::vector<float> w(size_t(c.n_text_layer) * 2 * dd);
  for (int l = 0; l < c.n_text_layer; ++l) {
    const std::string blk = "decoder.blocks." + std::to_string(l);
    std::memcpy(w.data() + (size_t(l) * 2 + 0) * dd, f.get(blk + ".cross_attn.key.weight", dd), dd * 4);
    std::memcpy(w.data() + (size_t(l) * 2 + 1) * dd, f.get(blk + ".cross_attn.value.weight", dd), dd * 4);
  }
  return w;
}

// Which tensors of the file make up which encoder contraction: fn(record, W, N, K) for each of them, W [N][K] fp32 on
// the host as the GEMMs contract with it.  upload_weights and ensure_bf16_weights fill the records' forms through it.
template <class Fn>
void fill_enc_linears(const WtwFile& f, const wtw::Dims& c, EncLinear& conv1, EncLinear& conv2, std::vector<EncLayer>& layers,
                      EncLinear& cross_kv, Fn&& fn) {
  const int d = c.n_audio_state, nm = c.n_mels;
  const size_t dd = size_t(d) * d;
  fn(conv1, conv_gemm_order(f.get("encoder.conv1.weight", size_t(d) * nm * 3), d, nm).data(), d, 3 * nm);
  fn(conv2, conv_gemm_order(f.get("encoder.conv2.weight", dd * 3), d, d).data(), d, 3 * d);
  for (size_t l = 0; l < layers.size(); ++l) {
    const std::string blk = "encoder.blocks." + std::to_string(l);
    fn(layers[l].qkv, fused_qkv_weight(f, blk + ".attn", d).data(), 3 * d, d);
    fn(layers[l].out, f.get(blk + ".attn.out.weight", dd), d, d);
    fn(layers[l].fc1, f.get(blk + ".mlp.0.weight", 4 * dd), 4 * d, d);
    fn(layers[l].fc2, f.get(blk + ".mlp.2.weight", 4 * dd), d, 4 * d);
  }
  fn(cross_kv, cross_kv_weight(f, c).data(), c.n_text_layer * 2 * d, d);
}
}  // namespace

void check_wtw_file(const std::string& path) {
  const WtwFile file(path);  // throws kErrIo / kErrFormat
  if (file.hdr.file_bytes != 0 && file.hdr.file_bytes != file.bytes) {
    throw Error(kErrFormat, "truncated or padded .wtw weight file (header says " + std::to_string(file.hdr.file_bytes) +
                                " bytes, file has " + std::to_string(file.bytes) + "): " + path);
  }
}

// The fused query matrix of the absorbed cross-attention, folded once, in double: A_h = c0 Wk_h^T Wq_h stacked over the
// heads ([heads * d][d]: row (h, c) gives column c of head h's d-wide query) and a_h = c0 Wk_h^T bq_h, with
// c0 = d_head^-1/2 log2 e (the kernel's softmax is an exp2).
void absorbed_query_matrix(const float* wq, const float* bq, const float* wk, int heads, int d, std::vector<float>* A,
                           std::vector<float>* av) {
  const double c0 = 0.125 * 1.44269504088896340736;
  A->assign(size_t(heads) * d * d, 0.0f);
  av->assign(size_t(heads) * d, 0.0f);
  std::vector<double> acc(d);
  for (int h = 0; h < heads; ++h) {
    for (int cc = 0; cc < d; ++cc) {
      std::fill(acc.begin(), acc.end(), 0.0);
      double ab = 0.0;
      for (int i = 0; i < 64; ++i) {
        const double kv = wk[size_t(h * 64 + i) * d + cc];
        const float* qrow = wq + size_t(h * 64 + i) * d;
        for (int j = 0; j < d; ++j) acc[j] += kv * qrow[j];
        ab += kv * bq[h * 64 + i];
      }
      float* arow = A->data() + (size_t(h) * d + cc) * d;
      for (int j = 0; j < d; ++j) arow[j] = float(c0 * acc[j]);
      (*av)[size_t(h) * d + cc] = float(c0 * ab);
    }
  }
}

void Engine::upload_weights(const std::string& path) {
  // Replaces Atom::Atom (whisper.cpp:261-271): instead of mmapping a .tflite FlatBuffer and
  // building an interpreter, the flat .wtw payload is mapped, re-laid-out for the kernels
  // and copied to HBM once.
  const WtwFile file(path);
  weights_path_ = path;
  const wtw::WtwHeader& hdr = file.hdr;
  dims_ = hdr.dims;
  const wtw::Dims& c = dims_;
  // Everything the kernels index with comes from this header: reject what they do not support here, as a
  // format error, instead of faulting (or dividing by zero) later.
  const auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
  const int dm = c.n_audio_state;
  if (!(dm == 128 || dm == 384 || dm == 512) || c.n_text_state != dm) {
    throw Error(kErrFormat, "unsupported model dims: d_model must be 128, 384 or 512 (encoder == decoder)");
  }
  if (!in(c.n_audio_head, 1, 64) || !in(c.n_text_head, 1, 64) || dm != 64 * c.n_audio_head || dm != 64 * c.n_text_head) {
    throw Error(kErrFormat, "unsupported model dims: heads must be d_model / 64");
  }
  if (!in(c.n_mels, 1, 128) || !in(c.n_audio_ctx, 32, 4096) || !in(c.n_text_ctx, 32, 4096) ||
      !in(c.n_audio_layer, 1, 64) || !in(c.n_text_layer, 1, 64) || !in(c.n_vocab, 1, 1 << 20)) {
    throw Error(kErrFormat, "unsupported model dims: n_mels 1..128, n_audio_ctx / n_text_ctx 32..4096, layers 1..64, n_vocab 1..2^20");
  }
  auto H = [&](const std::string& n, size_t expect) -> const float* { return file.get(n, expect); };
  auto up = [&](const std::string& n, size_t expect) -> const float* {
    const float* p = H(n, expect);
    const float* d = upload(std::vector<float>(p, p + expect));
    tensors_[n] = d;
    return d;
  };

  const int d = c.n_audio_state, nm = c.n_mels;
  // The encoder's vectors.  Its matrices follow the scales below: one of their forms is made with them (fill_enc_linears).
  auto fused_qkv_bias = [&](const std::string& p) {
    std::vector<float> b(3 * size_t(d), 0.0f);  // key has no bias
    std::memcpy(b.data(), H(p + ".query.bias", d), size_t(d) * 4);
    std::memcpy(b.data() + 2 * size_t(d), H(p + ".value.bias", d), size_t(d) * 4);
    return b;
  };
  conv1_.bias = up("encoder.conv1.bias", d);
  conv2_.bias = up("encoder.conv2.bias", d);
  enc_pos = up("encoder.positional_embedding", size_t(c.n_audio_ctx) * d);
  enc_layers_.assign(c.n_audio_layer, EncLayer{});
  for (int l = 0; l < c.n_audio_layer; ++l) {
    const std::string blk = "encoder.blocks." + std::to_string(l);
    EncLayer& el = enc_layers_[l];
    el.attn_ln_g = up(blk + ".attn_ln.weight", d);
    el.attn_ln_b = up(blk + ".attn_ln.bias", d);
    el.qkv.bias = upload(fused_qkv_bias(blk + ".attn"));
    el.out.bias = up(blk + ".attn.out.bias", d);
    el.mlp_ln_g = up(blk + ".mlp_ln.weight", d);
    el.mlp_ln_b = up(blk + ".mlp_ln.bias", d);
    el.fc1.bias = up(blk + ".mlp.0.bias", size_t(4) * d);
    el.fc2.bias = up(blk + ".mlp.2.bias", d);
  }
  enc_ln_post_g = up("encoder.ln_post.weight", d);
  enc_ln_post_b = up("encoder.ln_post.bias", d);

  tok_emb = up("decoder.token_embedding.weight", size_t(c.n_vocab) * d);  // row lookup
  tok_emb_tiled = upload_tiled(H("decoder.token_embedding.weight", size_t(c.n_vocab) * d), c.n_vocab, d);  // logits GEMM
  dec_pos = up("decoder.positional_embedding", size_t(c.n_text_ctx) * d);
  dec_blocks_.resize(c.n_text_layer);
  const size_t dd = size_t(d) * d;
  std::vector<float> ckv_b(size_t(c.n_text_layer) * 2 * d, 0.0f);
  for (int l = 0; l < c.n_text_layer; ++l) {
    const std::string blk = "decoder.blocks." + std::to_string(l);
    DecBlockWeights& bw = dec_blocks_[l];
    bw.attn_ln_g = up(blk + ".attn_ln.weight", d);
    bw.attn_ln_b = up(blk + ".attn_ln.bias", d);
    bw.wqkv = upload_tiled(fused_qkv_weight(file, blk + ".attn", d).data(), 3 * d, d);  // decoder Linears: fp16 planes in MFMA-fragment order
    bw.bqkv = upload(fused_qkv_bias(blk + ".attn"));
    bw.wo = upload_tiled(H(blk + ".attn.out.weight", dd), d, d);
    bw.bo = up(blk + ".attn.out.bias", d);
    bw.cross_ln_g = up(blk + ".cross_attn_ln.weight", d);
    bw.cross_ln_b = up(blk + ".cross_attn_ln.bias", d);
    bw.cross_wq_t = upload(cross_q_layout(H(blk + ".cross_attn.query.weight", dd), d));
    bw.cross_bq = up(blk + ".cross_attn.query.bias", d);
    bw.cross_wo = upload_tiled(H(blk + ".cross_attn.out.weight", dd), d, d);
    bw.cross_bo = up(blk + ".cross_attn.out.bias", d);
    {
      // Absorbed cross-attention (k_cross_absorbed.hip): scores q_h . (Wk_h e) = (Wk_h^T q_h) . e and contexts
      // sum_j p_j (Wv_h e_j + bv_h) = Wv_h (sum_j p_j e_j) + bv_h, so the decoder works on the encoder output e itself.
      // Wv_h and bv_h are applied to each head's combined context (cross_absorbed_combine).
      const int Hh = c.n_text_head;
      const float* wv = H(blk + ".cross_attn.value.weight", dd);
      const float* bv = H(blk + ".cross_attn.value.bias", d);
      std::vector<float> A, av;
      absorbed_query_matrix(H(blk + ".cross_attn.query.weight", dd), H(blk + ".cross_attn.query.bias", d),
                            H(blk + ".cross_attn.key.weight", dd), Hh, d, &A, &av);
      bw.wq_abs = upload_tiled(A.data(), Hh * d, d);
      bw.bq_abs = upload(av);
      bw.cross_wv_t = upload(cross_q_layout(wv, d));
      bw.cross_bv = upload(std::vector<float>(bv, bv + d));
    }
    // all layers' cross K/V projections act on the same encoder output: one GEMM (cross_kv_weight; the key has no bias)
    std::memcpy(ckv_b.data() + (size_t(l) * 2 + 1) * d, H(blk + ".cross_attn.value.bias", d), size_t(d) * 4);
    bw.mlp_ln_g = up(blk + ".mlp_ln.weight", d);
    bw.mlp_ln_b = up(blk + ".mlp_ln.bias", d);
    bw.w1 = upload_tiled(H(blk + ".mlp.0.weight", 4 * dd), 4 * d, d);
    bw.b1 = up(blk + ".mlp.0.bias", size_t(4) * d);
    bw.w2 = upload_tiled(H(blk + ".mlp.2.weight", 4 * dd), d, 4 * d);
    bw.b2 = up(blk + ".mlp.2.bias", d);
  }
  cross_kv_.bias = upload(ckv_b);
  dec_ln_g = up("decoder.ln.weight", d);
  dec_ln_b = up("decoder.ln.bias", d);
  // ---- operand bounds -> fp16 plane scales (engine.h, GemmScale) ----
  // Next to every bound a TYPICAL magnitude of the same operand is propagated (rms under unit-variance inputs:
  // LayerNorm sqrt(mean g^2 + mean b^2), Linear sqrt(mean_n sum_k W^2) * typical input).  The two-plane fp16
  // form keeps 22 significand bits only while the second plane stays a normal fp16 number, i.e. while
  // |x| * scale >= 2^-3; with scale = 2^14 / bound that needs typical / bound >= 2^-17.  A contraction whose
  // operand has bound / typical above kF16Slack (2^12: a factor 32 of margin for elements below the typical
  // magnitude) is given the full-range bf16 three-plane kernels instead — decided here, once, from the
  // weights alone (LayerNorm gains with outliers, heavy-tailed rows: tests/test_gpu_boundary.py).
  {
    auto maxabs = [](const float* w, size_t n) {
      float m = 0.0f;
      for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(w[i]));
      return m;
    };
    auto vmax = [](const std::vector<float>& v) {
      float m = 0.0f;
      for (float x : v) m = std::max(m, x);
      return m;
    };
    struct Op {  // one contraction operand: per-channel bound, typical magnitude
      std::vector<float> bound;
      float typ;
    };
    auto ln_op = [&](const std::string& gname, const std::string& bname) {
      const float* gg = H(gname, d);
      const float* bb = H(bname, d);
      Op o{std::vector<float>(d), 0.0f};
      const float r = std::sqrt(float(d - 1));
      double acc = 0.0;
      for (int i = 0; i < d; ++i) {
        o.bound[i] = std::fabs(gg[i]) * r + std::fabs(bb[i]);
        acc += double(gg[i]) * gg[i] + double(bb[i]) * bb[i];
      }
      o.typ = float(std::sqrt(acc / d));
      return o;
    };
    // out[n] = sum_k |W[n][k]| in[k % in.size()] + |bias[n]|.  Column k of a Linear is input channel k.  Column k of a
    // conv tensor [co][ci][3] is channel k / 3, so k % in.size() pairs it with the right channel only for a one-element
    // input bound: that is conv1 (the mel bound), the only conv whose output bound is formed — conv2's never is.
    auto linear_op = [&](const float* w, const float* bias, int N, int K, const Op& in) {
      Op o{std::vector<float>(N), 0.0f};
      double sq = 0.0;
      for (int n = 0; n < N; ++n) {
        double acc = bias ? std::fabs(bias[n]) : 0.0;
        for (int k = 0; k < K; ++k) {
          const double wv = w[size_t(n) * K + k];
          acc += std::fabs(wv) * in.bound[size_t(k) % in.bound.size()];
          sq += wv * wv;
        }
        o.bound[n] = float(acc);
      }
      o.typ = float(std::sqrt(sq / N)) * in.typ;
      return o;
    };
    auto gelu_op = [](Op o) {
      for (float& x : o.bound) x = std::max(x, 0.17f);  // gelu(x) in [-0.17, max(x, 0)]
      o.typ *= 0.5f;
      return o;
    };
    n_f16_fallbacks_ = 0;
    // slack of an operand in bits: log2(kF16Slack * typical / bound) — negative: the contraction leaves the plane kernels
    f16_min_slack_bits_ = 1.0e9f;
    auto slack_ok = [&](const Op& o) {
      const float b = vmax(o.bound);
      if (b > 0.0f && o.typ > 0.0f) f16_min_slack_bits_ = std::min(f16_min_slack_bits_, std::log2(kF16Slack * o.typ / b));
      return !(b > kF16Slack * o.typ);
    };
    // the operands' {largest bound, typical} beside each verdict (encoder_scales): up to three per contraction
    load_ops_.clear();
    auto note = [&](const Op& a, const Op* b = nullptr, const Op* c = nullptr, float a_factor = 1.0f) {
      std::array<float, 6> r{vmax(a.bound) * a_factor, a.typ * a_factor, 0.0f, 0.0f, 0.0f, 0.0f};
      if (b) r[2] = vmax(b->bound), r[3] = b->typ;
      if (c) r[4] = vmax(c->bound), r[5] = c->typ;
      load_ops_.push_back(r);
    };
    auto scale_of = [&](const Op& in, const float* w, size_t n) {
      note(in);
      GemmScale g{f16_scale_for(vmax(in.bound)), f16_scale_for(maxabs(w, n)), slack_ok(in)};
      if (!g.f16_ok) ++n_f16_fallbacks_;
      return g;
    };
    // conv1: host copy in the kernel's [co][kpad] order is gone; bounds use the original [co][ci][3] tensor,
    // which has the same absolute values
    const Op mel_op{std::vector<float>(1, kMelBound), 1.0f};
    const float* c1w = H("encoder.conv1.weight", size_t(d) * nm * 3);
    conv1_.sc = scale_of(mel_op, c1w, size_t(d) * nm * 3);
    const Op h1 = gelu_op(linear_op(c1w, H("encoder.conv1.bias", d), d, nm * 3, mel_op));
    const float* c2w = H("encoder.conv2.weight", size_t(d) * d * 3);
    conv2_.sc = scale_of(h1, c2w, size_t(d) * d * 3);
    const size_t dd2 = size_t(d) * d;
    for (int l = 0; l < c.n_audio_layer; ++l) {
      const std::string blk = "encoder.blocks." + std::to_string(l);
      EncLayer& sl = enc_layers_[l];
      const Op ln1 = ln_op(blk + ".attn_ln.weight", blk + ".attn_ln.bias");
      const float* wq = H(blk + ".attn.query.weight", dd2);
      const float* wk = H(blk + ".attn.key.weight", dd2);
      const float* wv = H(blk + ".attn.value.weight", dd2);
      const float wmax = std::max(maxabs(wq, dd2), std::max(maxabs(wk, dd2), maxabs(wv, dd2)));
      sl.qkv.sc = GemmScale{f16_scale_for(vmax(ln1.bound)), f16_scale_for(wmax), slack_ok(ln1)};
      if (!sl.qkv.sc.f16_ok) ++n_f16_fallbacks_;
      note(ln1);
      const Op qo = linear_op(wq, H(blk + ".attn.query.bias", d), d, d, ln1);
      const Op ko = linear_op(wk, nullptr, d, d, ln1);
      const Op vo = linear_op(wv, H(blk + ".attn.value.bias", d), d, d, ln1);
      sl.q = f16_scale_for(vmax(qo.bound) * 0.125f * 1.44269504f);  // the kernel splits q * d_head^-1/2 * log2(e)
      sl.k = f16_scale_for(vmax(ko.bound));
      sl.v = f16_scale_for(vmax(vo.bound));
      sl.attn_f16_ok = slack_ok(qo) && slack_ok(ko) && slack_ok(vo);
      if (!sl.attn_f16_ok) ++n_f16_fallbacks_;
      note(qo, &ko, &vo, 0.125f * 1.44269504f);  // q as the kernel splits it
      sl.out.sc = scale_of(vo, H(blk + ".attn.out.weight", dd2), dd2);  // a convex combination of V rows
      const Op ln2 = ln_op(blk + ".mlp_ln.weight", blk + ".mlp_ln.bias");
      const float* w1 = H(blk + ".mlp.0.weight", 4 * dd2);
      sl.fc1.sc = scale_of(ln2, w1, 4 * dd2);
      const Op hb = gelu_op(linear_op(w1, H(blk + ".mlp.0.bias", size_t(4) * d), 4 * d, d, ln2));
      sl.fc2.sc = scale_of(hb, H(blk + ".mlp.2.weight", 4 * dd2), 4 * dd2);
    }
    const Op lnp = ln_op("encoder.ln_post.weight", "encoder.ln_post.bias");
    const std::vector<float> ckv_w = cross_kv_weight(file, c);
    cross_kv_.sc = GemmScale{f16_scale_for(vmax(lnp.bound)), f16_scale_for(maxabs(ckv_w.data(), ckv_w.size())), slack_ok(lnp)};
    if (!cross_kv_.sc.f16_ok) ++n_f16_fallbacks_;
    note(lnp);
    load_ok_.clear();
    for (bool* f : ok_flags()) load_ok_.push_back(*f);
  }
  // ---- the encoder's matrices: fp32 for the fall-back kernels (k_gemm.hip) and the two fp16 planes of W * sc.w for the
  // plane GEMM (k_gemm_planes.hip), split once, here ----
  fill_enc_linears(file, c, conv1_, conv2_, enc_layers_, cross_kv_, [&](EncLinear& L, const float* W, int N, int K) {
    L.N = N; L.k = K;
    L.k32 = L.kp = int(round_up(size_t(K), 32));
    L.kbf = int(round_up(size_t(K), 64));
    std::vector<float> w32(size_t(N) * L.k32, 0.0f);
    for (int n = 0; n < N; ++n) std::memcpy(w32.data() + size_t(n) * L.k32, W + size_t(n) * K, size_t(K) * 4);
    L.w32 = upload(w32);
    L.wp = upload_planes(W, N, K, L.kp, L.sc.w);
  });
}

// The f16_ok / attn_f16_ok verdicts of the records in launch order: the bit numbering of force_fallback
std::vector<bool*> Engine::ok_flags() {
  std::vector<bool*> f{&conv1_.sc.f16_ok, &conv2_.sc.f16_ok};
  for (EncLayer& el : enc_layers_) {
    for (bool* p : {&el.qkv.sc.f16_ok, &el.attn_f16_ok, &el.out.sc.f16_ok, &el.fc1.sc.f16_ok, &el.fc2.sc.f16_ok}) f.push_back(p);
  }
  f.push_back(&cross_kv_.sc.f16_ok);
  return f;
}

// One record per contraction in the order of ok_flags(): the scales the launches take, the load-time verdict (load_ok_,
// not what force_fallback made of it) and the operands' largest bound and typical magnitude.  GEMM: {a_scale, w_scale,
// ok, bound, typical}; attention: {q, k, v scales, ok, then bound and typical of q (times d_head^-1/2 log2 e), k and v}.
std::vector<std::array<float, 10>> Engine::encoder_scales() const {
  std::vector<std::array<float, 10>> r;
  auto gemm = [&](const EncLinear& L) {
    const size_t i = r.size();
    r.push_back({L.sc.a, L.sc.w, load_ok_[i] ? 1.0f : 0.0f, load_ops_[i][0], load_ops_[i][1], 0.0f, 0.0f, 0.0f, 0.0f, 0.0f});
  };
  gemm(conv1_);
  gemm(conv2_);
  for (const EncLayer& el : enc_layers_) {
    gemm(el.qkv);
    const size_t i = r.size();
    const std::array<float, 6>& o = load_ops_[i];
    r.push_back({el.q, el.k, el.v, load_ok_[i] ? 1.0f : 0.0f, o[0], o[1], o[2], o[3], o[4], o[5]});
    gemm(el.out);
    gemm(el.fc1);
    gemm(el.fc2);
  }
  gemm(cross_kv_);
  return r;
}

void Engine::set_force_fallback(long mask) {
  require_idle();
  const std::vector<bool*> f = ok_flags();
  if (mask < 0 || (f.size() < 63 && (mask >> f.size()) != 0)) throw Error(kErrInvalidArg, "force_fallback: bit beyond the last contraction");
  n_f16_fallbacks_ = 0;
  for (size_t i = 0; i < f.size(); ++i) {
    *f[i] = load_ok_[i] && !((mask >> i) & 1);
    if (!*f[i]) ++n_f16_fallbacks_;
  }
  force_fallback_ = mask;
}

// bf16 storage mode (option "bf16", BASELINE configs[3]): bf16 copies of every matrix a kernel contracts with, made
// from the weight file the first time the mode is switched on.  Biases, LayerNorm gains / shifts, positional tables
// and the embedding rows the decoder looks up stay fp32 (epilogue / prologue operands, never MFMA operands), and so
// does the cross-attention query projection, which runs as an fp32 matrix-vector product inside cross_attention_step.
void Engine::ensure_bf16_weights() {
  if (bf16_ready_) return;
  if (dims_.n_audio_state == 0) throw Error(kErrUnsupported, "front-end-only engine: no model weights loaded");
  const WtwFile file(weights_path_);
  const wtw::Dims& c = dims_;
  const int d = c.n_audio_state;
  auto H = [&](const std::string& n, size_t expect) -> const float* { return file.get(n, expect); };
  auto up16 = [&](const std::vector<unsigned short>& v) -> const unsigned short* {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(unsigned short) + 256));
    allocations_.push_back(p);
    HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    return static_cast<const unsigned short*>(p);
  };
  const size_t dd = size_t(d) * d;
  fill_enc_linears(file, c, conv1_, conv2_, enc_layers_, cross_kv_, [&](EncLinear& L, const float* W, int N, int K) {
    L.wbf = up16(round_weights_bf16(W, N, K, L.kbf));
  });
  dec_blocks_bf_ = dec_blocks_;  // fp32 vectors shared; the tiled matrices are replaced below
  for (int l = 0; l < c.n_text_layer; ++l) {
    const std::string blk = "decoder.blocks." + std::to_string(l);
    DecBlockWeights& bw = dec_blocks_bf_[l];
    bw.wqkv = TiledW{up16(tile_weights_bf16(fused_qkv_weight(file, blk + ".attn", d).data(), 3 * d, d)), 1.0f};
    bw.wo = TiledW{up16(tile_weights_bf16(H(blk + ".attn.out.weight", dd), d, d)), 1.0f};
    bw.cross_wo = TiledW{up16(tile_weights_bf16(H(blk + ".cross_attn.out.weight", dd), d, d)), 1.0f};
    bw.w1 = TiledW{up16(tile_weights_bf16(H(blk + ".mlp.0.weight", 4 * dd), 4 * d, d)), 1.0f};
    bw.w2 = TiledW{up16(tile_weights_bf16(H(blk + ".mlp.2.weight", 4 * dd), d, 4 * d)), 1.0f};
    std::vector<float> A, av;  // absorbed cross-attention: the fused query matrix as bf16 (bq_abs, Wv, bv stay fp32: shared)
    absorbed_query_matrix(H(blk + ".cross_attn.query.weight", dd), H(blk + ".cross_attn.query.bias", d),
                          H(blk + ".cross_attn.key.weight", dd), c.n_text_head, d, &A, &av);
    bw.wq_abs = TiledW{up16(tile_weights_bf16(A.data(), c.n_text_head * d, d)), 1.0f};
  }
  tok_emb_tiled_bf_ = TiledW{up16(tile_weights_bf16(H("decoder.token_embedding.weight", size_t(c.n_vocab) * d), c.n_vocab, d)), 1.0f};
  bf16_ready_ = true;
}

namespace {
// The linear map the reference's transform actually applies.  whisper.cpp:58-106 is a
// radix-2 recursion (400 -> 200 -> 100 -> 50 -> 25) over a naive 25-point DFT (:37-54) whose
// twiddles are cosf/sinf of an angle already rounded to float (:46, :92): at the leaf the
// angle reaches 2*pi*24*24/25 = 145 rad, so the rounded argument is off by up to ~1e-5 rad.
// That systematic deviation from the ideal DFT is 100x above fp32 rounding noise and shows in
// every bin that sits 40 dB below a frame's peak, so the device transform is built from the
// SAME twiddle values: the recursion is evaluated here in double on unit impulses, giving
// the effective 400x400 complex matrix, which the GPU then applies as one fp32 MFMA GEMM.
using cd = std::complex<double>;
void effective_fft(const std::vector<cd>& in, std::vector<cd>& out) {
  const int N = int(in.size());
  out.assign(N, cd(0, 0));
  if (N == 1) {
    out[0] = in[0];
    return;
  }
  if (N % 2 == 1) {
    for (int k = 0; k < N; ++k) {
      cd acc(0, 0);
      for (int n = 0; n < N; ++n) {
        double a = 2 * M_PI;
        a = a * k;
        a = a * n;
        a = a / N;
        const float angle = static_cast<float>(a);
        acc += in[n] * cd(double(cosf(angle)), -double(sinf(angle)));
      }
      out[k] = acc;
    }
    return;
  }
  std::vector<cd> even(N / 2), odd(N / 2), fe, fo;
  for (int i = 0; i < N / 2; ++i) {
    even[i] = in[2 * i];
    odd[i] = in[2 * i + 1];
  }
  effective_fft(even, fe);
  effective_fft(odd, fo);
  for (int k = 0; k < N / 2; ++k) {
    double a = 2 * M_PI;
    a = a * k;
    a = a / N;
    const float theta = static_cast<float>(a);
    const cd w(double(cosf(theta)), -double(sinf(theta)));
    out[k] = fe[k] + w * fo[k];
    out[k + N / 2] = fe[k] - w * fo[k];
  }
}
}  // namespace

void Engine::build_frontend_tables() {
  // STFT as a GEMM: rows of the basis are the reference's effective transform with the Hann
  // window (whisper.cpp:117-120: double cos, float store) folded in.  All 400 output bins are
  // kept because the reference adds the mirror bin's power computed by the same inexact
  // transform (:164-166).
  const int n_fft = 400, n_bins = 201;
  if (filters_.n_fft != n_bins || filters_.n_mel != dims_.n_mels) {
    have_logmel_ = false;  // front end needs the 80x201 bank; encoder/decoder still work
    return;
  }
  // Round 4: the STFT runs on the fp16-plane GEMM (PCM is bounded, the windowed basis is bounded: the two-plane form is
  // admissible) and writes the POWER spectrum from its epilogue (kEpiPower).  Rows (2 k, 2 k + 1) of the basis are the
  // real and imaginary parts of bin k for k = 0 .. 200 only: the input is real, so the mirror bin the reference adds
  // (P[j] += P[400 - j], whisper.cpp:164-166) is folded into the row of bin j (below).  402 rows, padded to 512;
  // round 3 contracted all 800 rows (896 padded) on six bf16 products and squared / folded in a kernel of its own.
  dft_k = int(round_up(n_fft, 32));  // 416: samples 400..415 meet zero basis entries
  dft_n = int(round_up(2 * n_bins, 128));  // 512
  std::vector<float> basis(size_t(dft_n) * dft_k, 0.0f);
  std::vector<cd> impulse(n_fft), col;
  const double r2 = std::sqrt(2.0);
  float bmax = 0.0f;
  for (int n = 0; n < n_fft; ++n) {
    const float hann = static_cast<float>(0.5 * (1.0 - std::cos((2.0 * M_PI * n) / n_fft)));
    std::fill(impulse.begin(), impulse.end(), cd(0, 0));
    impulse[n] = cd(double(hann), 0);
    effective_fft(impulse, col);
    for (int k = 0; k < n_bins; ++k) {
      // bins 1 .. 199: sqrt(2) * (X_k + conj(X_{400-k})) / 2 — twice its squared magnitude is |X_k|^2 + |X_{400-k}|^2 up to
      // the SQUARE of the two bins' difference (the reference's inexact twiddles make them differ by ~1e-7 of the
      // largest amplitude, which shows at the 2e-4 level in bins eight decades below the maximum: a sweep's far bins)
      const bool folded = k >= 1 && k < n_fft / 2;
      const cd y = folded ? r2 * 0.5 * (col[k] + std::conj(col[n_fft - k])) : col[k];
      const float re = static_cast<float>(y.real()), im = static_cast<float>(y.imag());
      basis[size_t(2 * k) * dft_k + n] = re;
      basis[size_t(2 * k + 1) * dft_k + n] = im;
      bmax = std::max(bmax, std::max(std::fabs(re), std::fabs(im)));
    }
  }
  dft_w_scale_ = f16_scale_for(bmax);
  dft_basis_p_ = upload_planes(basis.data(), dft_n, dft_k, dft_k, dft_w_scale_);
  dft_basis_host_ = std::move(basis);
  dft_zero_bias_ = upload(std::vector<float>(size_t(dft_n), 0.0f));
  pw_ld_ = dft_n / 2;  // 256 powers per frame row (201 used)
  mel_k = int(round_up(n_bins, 32));  // 224 (the mel GEMM reads rows of pw_ld_ = 256 powers)
  mel_n = int(round_up(size_t(dims_.n_mels), 128));
  std::vector<float> mw(size_t(mel_n) * mel_k, 0.0f);
  for (int j = 0; j < dims_.n_mels; ++j)
    for (int k = 0; k < n_bins; ++k) mw[size_t(j) * mel_k + k] = filters_.data[size_t(j) * n_bins + k];
  mel_w = upload(mw);
  mel_w_host_ = std::move(mw);
  have_logmel_ = true;
}

// ---------------------------------------------------------- lifecycle ---

void Engine::open_device() {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    throw Error(5, "no HIP device available: this engine has no CPU fallback");
  }
  if (device_ < 0 || device_ >= n_dev) throw Error(5, "device_id out of range");
  HIPCHK(hipSetDevice(device_));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device_));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
    throw Error(5, std::string("device is ") + prop.gcnArchName +
                            ", kernels are built for gfx950 only");
  }
  n_cu_ = prop.multiProcessorCount;
}

void Engine::create_streams() {
  int prio_lo = 0, prio_hi = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  HIPCHK(hipStreamCreateWithPriority(&stream_full_, hipStreamNonBlocking, prio_lo));
  // Pipelined batches run the encoder on a stream that leaves `reserve` CUs of every XCD to the
  // decoders (mask bit i = CU i/8 of XCD i%8): measured on MI355X, three decoder chains next
  // to an encoder that owns every CU stretch it by 2.5 ms per batch, next to one that owns
  // 224 of 256 CUs by 0.9 ms; with the faster encoder kernels 4..8 CUs per XCD measure
  // within 2 % of each other. Synchronous calls keep the whole chip.
  // (round 4: the absorbed cross-attention needs a third less CU time — 4 per XCD = 224 CUs for the encoder measured
  // 148.6 k against 146.8 k audio-sec/s with 8, 5 / 6 in between, 3: 139.5 k; tools/ab_r4_pipeline.sh)
  int reserve = 4;  // 224 CUs for the pipelined encoder: 188 row tiles of 256 fill one round
  if (const char* v = getenv("WT_ENC_CU_RESERVE")) reserve = std::min(std::max(atoi(v), 0), 16);
  reserve_ = reserve;
  const int n_cu = n_cu_;
  if (reserve > 0 && n_cu >= 64 && n_cu % 8 == 0) {
    int keep = n_cu - 8 * reserve;
    if (const char* v = getenv("WT_ENC_CU_KEEP")) keep = std::min(std::max(atoi(v), 64), n_cu);  // CUs of the masked stream
    enc_cus_masked_ = keep;
    std::vector<uint32_t> mask((n_cu + 31) / 32, 0u);
    for (int i = 0; i < keep; ++i) mask[i / 32] |= 1u << (i % 32);
    HIPCHK(hipExtStreamCreateWithCUMask(&stream_masked_, uint32_t(mask.size()), mask.data()));
  }
  stream_ = stream_full_;
  HIPCHK(hipEventCreate(&ev_switch_));
  if (const char* v = getenv("WT_DEC_STREAMS")) n_dec_streams_ = std::min(std::max(atoi(v), 1), kDecStreams);
  // WT_DEC_PARTITION=1 (measurement knob): the decoder streams are confined to the CUs the pipelined encoder stream
  // leaves free — a strict partition instead of "decoders may run anywhere"
  const char* part = getenv("WT_DEC_PARTITION");
  if (part && atoi(part) >= 1 && enc_cus_masked_ > 0 && enc_cus_masked_ < n_cu) {
    // 1 = the reserved CUs only; N > 1 = the reserved CUs and the N CUs of the encoder's share next to them (soft partition)
    const int shared = atoi(part) > 1 ? std::min(atoi(part), enc_cus_masked_) : 0;
    std::vector<uint32_t> dmask((n_cu + 31) / 32, 0u);
    for (int i = enc_cus_masked_ - shared; i < n_cu; ++i) dmask[i / 32] |= 1u << (i % 32);
    for (auto& ds : dstream_) HIPCHK(hipExtStreamCreateWithCUMask(&ds, uint32_t(dmask.size()), dmask.data()));
  } else {
    const char* dp = getenv("WT_DEC_PRIO");  // measurement knob: "lo" = decoder streams at the encoder's priority
    const int prio = dp && dp[0] == 'l' ? prio_lo : prio_hi;
    // (round 4: candidates on a second priority level, or GPU_MAX_HW_QUEUES=8, give the probe no further stream that
    // overlaps with the four in use — the process has four hardware queues, the encoder's and three decoders')
    for (auto& ds : dstream_) HIPCHK(hipStreamCreateWithPriority(&ds, hipStreamNonBlocking, prio));
  }
  pick_decoder_streams();
  for (auto& e : ev_) HIPCHK(hipEventCreate(&e));
  for (Slot& sl : slots_) {
    for (hipEvent_t* e : {&sl.enc_begin, &sl.enc_mid, &sl.enc_done, &sl.dec_begin, &sl.dec_done}) {
      HIPCHK(hipEventCreate(e));
    }
    sl.h_ids = pinned<long long>(4096 * 32);
    sl.h_n = pinned<int>(4096);
    sl.h_flag = pinned<int>(1);
    *sl.h_flag = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&sl.d_flag), sizeof(int)));
  }
}

Engine::Engine(const std::string& model_prefix, const std::string& vocab_path, bool multilingual,
               int device_id, bool monolith, const std::string& weights_path)
    : device_(device_id), monolith_(monolith), multilingual_(multilingual) {
  // vocab first: a missing vocab file throws exactly like the reference's MmapFile
  read_vocab_file(vocab_path, multilingual, &filters_, &vocab_);
  if (monolith) language = 0;  // HF generate() forces <|en|> for a multilingual checkpoint (export/generate.py:24-30)
  open_device();
  // A constructor that throws does not run the destructor: everything acquired below (streams, events,
  // pinned host memory, device allocations) is released here before the exception leaves, so a failed
  // wt_engine_create (missing or malformed .wtw) leaks nothing.
  try {
    create_streams();
    upload_weights(weights_path.empty() ? model_prefix + ".wtw" : weights_path);
    if (vocab_.n_vocab != dims_.n_vocab && verbose) {
      std::fprintf(stderr, "[wt] note: vocab file n_vocab %d != model n_vocab %d\n", vocab_.n_vocab,
                   dims_.n_vocab);
    }
    build_frontend_tables();
  } catch (...) {
    release();
    throw;
  }
}

Engine::Engine(const FilterBank& filters, int device_id) : device_(device_id), filters_(filters) {
  // front end only (whisper::log_mel_spectrogram as a free function, whisper.h:123): no weights, the
  // reference's fixed audio geometry (whisper.h:34-39)
  dims_ = wtw::Dims{};
  dims_.n_mels = filters.n_mel;
  dims_.n_audio_ctx = 1500;
  open_device();
  try {
    create_streams();
    build_frontend_tables();
  } catch (...) {
    release();
    throw;
  }
}

Engine::~Engine() { release(); }

void Engine::release() noexcept {
  (void)hipSetDevice(device_);
  for (hipStream_t st : {stream_full_, stream_masked_})
    if (st) (void)hipStreamSynchronize(st);
  for (auto& ds : dstream_)
    if (ds) (void)hipStreamSynchronize(ds);
  for (auto& g : graphs_) (void)hipGraphExecDestroy(g.second.exec);
  graphs_.clear();
  for (void* p : ws_.owned) (void)hipFree(p);
  ws_.owned.clear();
  for (void* p : allocations_) (void)hipFree(p);
  allocations_.clear();
  for (auto& e : ev_) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  for (Slot& sl : slots_) {
    for (hipEvent_t* e : {&sl.enc_begin, &sl.enc_mid, &sl.enc_done, &sl.dec_begin, &sl.dec_done}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
    for (auto& e : sl.kt_events) (void)hipEventDestroy(e);
    for (auto& e : sl.dt_events) (void)hipEventDestroy(e);
    sl.kt_events.clear();
    sl.dt_events.clear();
    if (sl.d_flag) (void)hipFree(sl.d_flag);
    sl.h_ids = nullptr, sl.h_n = nullptr, sl.h_flag = nullptr, sl.d_flag = nullptr;
  }
  for (void* p : pinned_) (void)hipHostFree(p);
  pinned_.clear();
  // (the workspaces' device buffers were in allocations_, their pinned ones in pinned_)
  bw_ = BeamWorkspace();
  bf_ = BeamFullWorkspace();
  bo_ = BestOfWorkspace();
  fw_ = FullWorkspace();
  d_suppress_ = nullptr;
  rw_ = RaggedWorkspace();
  aw_ = AlignWorkspace();
  h_lang_probs_ = nullptr, h_lang_prob_ = nullptr, h_lang_ = nullptr;
  for (LangWorkspace& lw : lw_) lw = LangWorkspace();
  if (ev_switch_) (void)hipEventDestroy(ev_switch_);
  if (trace_base_) (void)hipEventDestroy(trace_base_);
  ev_switch_ = nullptr, trace_base_ = nullptr;
  for (hipStream_t* st : {&stream_full_, &stream_masked_}) {
    if (*st) (void)hipStreamDestroy(*st);
    *st = nullptr;
  }
  for (auto& ds : dstream_) {
    if (ds) (void)hipStreamDestroy(ds);
    ds = nullptr;
  }
  stream_ = nullptr;
}

// The runtime multiplexes the streams of a process onto a few hardware queues, and two streams that share a queue run
// their kernels one after the other.  Which streams share depends on everything the process created before (a second
// engine in one process measured 108 k instead of 131 k audio-sec/s: one of its decoder streams sat on the encoder
// stream's queue).  So the engine does not trust creation order: it times a 300 us one-wavefront kernel on pairs of
// streams (concurrent ~0.3 ms, serialised ~0.6 ms) and moves to the front of dstream_ decoder streams that overlap with
// the pipelined encoder stream and with each other.  ~10 ms at engine creation; WT_NO_STREAM_PROBE=1 skips it.
void Engine::pick_decoder_streams() {
  if (getenv("WT_NO_STREAM_PROBE") || getenv("WT_DEC_PARTITION")) return;
  hipStream_t enc = stream_masked_ ? stream_masked_ : stream_full_;
  constexpr int kSpinUs = 10, kChain = 20;  // a chain of dependent short kernels per stream, like a decoder chain
  const bool trace = getenv("WT_STREAM_PROBE_TRACE") != nullptr;
  auto chain_us = [&](hipStream_t a, hipStream_t b) {
    HIPCHK(hipStreamSynchronize(a));
    if (b) HIPCHK(hipStreamSynchronize(b));
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < kChain; ++i) {
      launch_spin(kSpinUs, a);
      if (b) launch_spin(kSpinUs, b);
    }
    HIPCHK(hipStreamSynchronize(a));
    if (b) HIPCHK(hipStreamSynchronize(b));
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  };
  launch_spin(50, enc);  // first launch of the kernel (code object load) outside the timed pairs
  double alone = chain_us(enc, nullptr);  // the reference is the fastest of three (a slow first run would hide clashes)
  for (int i = 0; i < 2; ++i) alone = std::min(alone, chain_us(enc, nullptr));
  // a pair shares a hardware queue when it is slow in BOTH of two runs: the timing is host wall-clock over ~0.5 ms, and a
  // single run disturbed by the host (a page fault, another rank starting) would otherwise reject a good stream — or the
  // choice, and with it the throughput, would differ between two runs of the same program
  auto serialised = [&](hipStream_t a, hipStream_t b) {
    const double us = std::min(chain_us(a, b), chain_us(a, b));
    if (trace) std::fprintf(stderr, "[wt] stream probe: pair %p %p %.0f us (one chain alone %.0f us)\n", (void*)a, (void*)b, us, alone);
    return us > 1.5 * alone;
  };
  int chosen = 0;
  const int want = std::min(kDecStreams, n_dec_streams_ + 2);  // + spare streams for the latency form (submit_decoder)
  for (int i = 0; i < kDecStreams && chosen < want; ++i) {
    bool clash = serialised(enc, dstream_[i]);
    for (int j = 0; j < chosen && !clash; ++j) clash = serialised(dstream_[j], dstream_[i]);
    if (clash) continue;
    std::swap(dstream_[chosen], dstream_[i]);
    ++chosen;
  }
  n_spare_streams_ = std::max(0, chosen - n_dec_streams_);
  if (trace || verbose) {
    std::fprintf(stderr, "[wt] stream probe: %d decoder streams (%d wanted + spares) run beside the encoder stream:", chosen, n_dec_streams_);
    for (int i = 0; i < chosen; ++i) std::fprintf(stderr, " %p", (void*)dstream_[i]);
    std::fprintf(stderr, "\n");
  }
}

void Engine::select_stream(bool pipelined) {
  pipelined_call_ = pipelined;
  hipStream_t target = pipelined && stream_masked_ ? stream_masked_ : stream_full_;
  if (target == stream_) return;
  // everything already enqueued on the old stream stays ahead of what follows on the new one
  HIPCHK(hipEventRecord(ev_switch_, stream_));
  HIPCHK(hipStreamWaitEvent(target, ev_switch_, 0));
  stream_ = target;
}

void Engine::bind_device() { HIPCHK(hipSetDevice(device_)); }

void Engine::sync() {
  HIPCHK(hipStreamSynchronize(stream_full_));
  if (stream_masked_) HIPCHK(hipStreamSynchronize(stream_masked_));
  for (auto& ds : dstream_) HIPCHK(hipStreamSynchronize(ds));
}

// The cross K/V cache (layers x 2 x clips x 1500 x d fp32: 590 MB per slot for tiny at 32 clips, 1.2 GB for base at 64)
// belongs to the cached decoder form only — cross_absorb = 0, synchronous calls below 32 clips, a flagged cross
// operand — so it is allocated per slot the first time a batch of that form is encoded into the slot, not for all
// every slot up front (the default absorbed form never touches it).
void Engine::need_cross_kv(Slot& slot) {
  if (slot.cross_kv) return;
  const wtw::Dims& c = dims_;
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, size_t(c.n_text_layer) * 2 * size_t(ws_.batch) * c.n_audio_ctx * c.n_audio_state * sizeof(float)));
  ws_.owned.push_back(p);
  slot.cross_kv = static_cast<float*>(p);
}

void Engine::ensure_batch(int batch) {
  if (batch <= 0 || batch > 4096) throw Error(1, "batch must be in [1, 4096]");
  HIPCHK(hipSetDevice(device_));
  if (batch <= ws_.batch) return;
  if (!inflight_.empty()) throw Error(1, "cannot grow the workspace while batches are in flight");
  HIPCHK(hipStreamSynchronize(stream_));
  for (auto& ds : dstream_) HIPCHK(hipStreamSynchronize(ds));
  for (auto& g : graphs_) (void)hipGraphExecDestroy(g.second.exec);  // captured pointers die with the workspace
  graphs_.clear();
  for (void* p : ws_.owned) (void)hipFree(p);
  ws_ = Workspace();
  const wtw::Dims& c = dims_;
  const size_t B = batch, T0 = mel_frames(), T = c.n_audio_ctx, d = c.n_audio_state;
  auto alloc = [&](size_t n_floats, bool zero) -> float* {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, n_floats * sizeof(float)));
    ws_.owned.push_back(p);
    if (zero) HIPCHK(hipMemsetAsync(p, 0, n_floats * sizeof(float), stream_));
    return static_cast<float*>(p);
  };
  // time-major, one zero row before and after each clip: the k=3 convolutions become
  // plain GEMMs over three consecutive rows
  if (d == 0) {  // front-end-only engine: the staging mel buffer is all the batch needs
    ws_.mel_stage = alloc(B * mel_elems(), false);
    ws_.batch = batch;
    HIPCHK(hipStreamSynchronize(stream_));
    return;
  }
  ws_.melT = alloc(B * (T0 + 2) * c.n_mels + 256, true);
  ws_.h1p = alloc(B * (T0 + 2) * d + 256, true);
  ws_.melTp = reinterpret_cast<unsigned short*>(alloc(B * (T0 + 2) * c.n_mels + 256, true));  // 2 planes of halfs
  ws_.h1pp = reinterpret_cast<unsigned short*>(alloc(B * (T0 + 2) * d + 256, true));
  ws_.x = alloc(B * T * d, false);
  ws_.ln = alloc(B * T * d, false);
  ws_.qkv = alloc(B * T * 3 * d, false);
  ws_.att = alloc(B * T * d, false);
  ws_.hid = alloc(B * T * 4 * d, false);
  ws_.enc_out = alloc(B * T * d, false);
  ws_.cvt = reinterpret_cast<unsigned short*>(alloc(B * T * 4 * d, false));
  for (Slot& sl : slots_) {
    sl.cross_kv = nullptr;  // the cross K/V cache of the CACHED decoder form: allocated when a batch first takes that form (need_cross_kv)
    sl.e_planes = reinterpret_cast<unsigned short*>(alloc(B * T * d, false));  // two planes of halfs
    sl.used = false;
  }
  // decoder rows: one position of the batch, or all prompt positions of a <= 32-clip batch in one pass
  const size_t R = std::max<size_t>(B, kDecRowsMax);
  for (DecWorkspace& dw : dws_) {
    dw.xd = alloc(R * d, false);
    dw.xb = alloc(R * d, false);
    dw.xpart = alloc(R * d, false);
    dw.qkvd = alloc(R * 3 * d, false);
    dw.attd = alloc(R * d, false);
    dw.hd = alloc(R * 4 * d, false);
    dw.cross_ws = alloc(R * c.n_text_head * 8 * 68, false);
    dw.qp = alloc(R * c.n_text_head * d, false);
    dw.abs_ws = alloc(R * c.n_text_head * 16 * (d + 4), false);
    dw.cabs = alloc(R * c.n_text_head * d, false);
    dw.self_kv = alloc(size_t(c.n_text_layer) * 2 * B * self_cap_ * d, true);
    dw.logits = alloc(B * c.n_vocab, false);
    dw.best = reinterpret_cast<unsigned long long*>(alloc(B * 2 * size_t((c.n_vocab + 31) / 32), true));
    dw.ids = reinterpret_cast<long long*>(alloc(B * 32 * 2, true));
    dw.n_ids = reinterpret_cast<int*>(alloc(B, true));
    dw.finished = reinterpret_cast<int*>(alloc(B, true));
  }
  ws_.mel_stage = alloc(B * mel_elems(), false);
  ws_.batch = batch;
  HIPCHK(hipStreamSynchronize(stream_));
}

float* Engine::staging_mel(int batch) {
  ensure_batch(batch);
  return ws_.mel_stage;
}

float* Engine::upload_pcm(const float* pcm, int batch) {
  float* d_pcm = staging_pcm(batch);
  const hipError_t rc = hipMemcpyAsync(d_pcm, pcm, size_t(batch) * pcm_elems() * sizeof(float), hipMemcpyHostToDevice, stream_);
  if (rc != hipSuccess) throw Error(kErrDevice, std::string("H2D pcm: ") + hipGetErrorString(rc));
  return d_pcm;
}

float* Engine::staging_pcm(int batch) {
  ensure_batch(batch);
  if (!ws_.pcm_stage) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, size_t(ws_.batch) * pcm_elems() * sizeof(float)));
    ws_.owned.push_back(p);
    ws_.pcm_stage = static_cast<float*>(p);
  }
  return ws_.pcm_stage;
}

// ---------------------------------------------------------- front end ---

Engine::FrontendView Engine::frontend_view() const {
  FrontendView v;
  v.pcm_planes = ws_.pcm_planes;
  v.pcm_plane = pcm_plane_;
  v.pcm_stride = long(pcm_elems()) + 512;
  v.pcm_scale = f16_scale_for(kPcmBound);
  v.pw = ws_.pw;
  v.melacc = ws_.melacc;
  v.clip_max = ws_.clip_max;
  v.pw_ld = pw_ld_;
  v.mel_n = mel_n;
  v.mel_k = mel_k;
  v.dft_n = dft_n;
  v.dft_k = dft_k;
  v.basis = dft_basis_host_.data();
  v.mel_matrix = mel_w_host_.data();
  return v;
}

void Engine::logmel(const float* d_pcm, int batch, float* d_mel, int valid_frames, float* d_raw) {
  if (!have_logmel_) throw Error(3, "vocab file carries no 80x201 mel filter bank");
  ensure_batch(batch);
  const size_t T0 = mel_frames(), n_samples = pcm_elems(), pad = n_samples + 512;
  if (!ws_.pcm_planes) {
    const size_t Bc = ws_.batch;
    auto alloc = [&](size_t n_floats) -> float* {
      void* p = nullptr;
      HIPCHK(hipMalloc(&p, n_floats * sizeof(float)));
      ws_.owned.push_back(p);
      HIPCHK(hipMemsetAsync(p, 0, n_floats * sizeof(float), stream_));
      return static_cast<float*>(p);
    };
    // PCM as two fp16 planes, [clip][480000 + 512] each, the tail of every clip zero for good (the reference's zero fill
    // past the last sample, whisper.cpp:149-153: only the first 480000 columns are ever written)
    pcm_plane_ = long(Bc * pad + 1024);
    ws_.pcm_planes = reinterpret_cast<unsigned short*>(alloc((size_t(pcm_plane_) * 2 * sizeof(unsigned short) + 3) / 4 + 64));
    ws_.pw = alloc(Bc * T0 * size_t(pw_ld_));
    ws_.melacc = alloc(Bc * T0 * mel_n);
    ws_.clip_max = reinterpret_cast<unsigned*>(alloc(Bc * kClipMaxStride * kClipMaxWays));
  }
  HIPCHK(hipEventRecord(ev_[0], stream_));
  const long M = long(batch) * long(T0);
  // STFT as a plane GEMM: frame i of a clip is the 416 samples from 160 i (hop-strided rows read in place), PCM within
  // +-kPcmBound (beyond: clamped), power spectrum out of the epilogue
  launch_pcm_to_planes(d_pcm, ws_.pcm_planes, pcm_plane_, f16_scale_for(kPcmBound), kPcmBound, batch, long(n_samples), long(pad),
                       stream_);
  PlaneGemmArgs g;
  g.A = ws_.pcm_planes;
  g.a_plane = pcm_plane_;
  g.a_rpb = int(T0);
  g.a_bs = long(pad);
  g.lda = 160;  // hop: frame i starts at sample 160 * i
  g.W = dft_basis_p_;
  g.bias = dft_zero_bias_;
  g.C = ws_.pw;
  g.M = int(M);
  g.N = dft_n;
  g.K = dft_k;
  g.ldc = pw_ld_;
  g.a_scale = f16_scale_for(kPcmBound);
  g.w_scale = dft_w_scale_;
  g.n_cu = stream_ == stream_masked_ && enc_cus_masked_ > 0 ? enc_cus_masked_ : n_cu_;
  launch_gemm_planes(g, kEpiBias | kEpiPower, stream_);
  GemmArgs m;
  m.A = ws_.pw;
  m.lda = pw_ld_;
  m.W = mel_w;
  m.C = ws_.melacc;
  m.M = int(M);
  m.N = mel_n;
  m.K = mel_k;
  m.ldc = mel_n;
  // the mel GEMM stays on the full-range three-plane kernel: power values span more decades than two fp16 planes keep
  m.variant = gemm_variant >= 0 ? int(gemm_variant) : 13;
  launch_gemm(m, 0, stream_);
  HIPCHK(hipMemsetAsync(ws_.clip_max, 0, sizeof(unsigned) * batch * kClipMaxStride * kClipMaxWays, stream_));
  launch_log_clipmax(ws_.melacc, mel_n, d_mel, ws_.clip_max, batch, dims_.n_mels, int(T0), stream_, valid_frames);
  if (d_raw) HIPCHK(hipMemcpyAsync(d_raw, d_mel, size_t(batch) * mel_elems() * sizeof(float), hipMemcpyDeviceToDevice, stream_));
  launch_mel_normalize(d_mel, ws_.clip_max, batch, dims_.n_mels, int(T0), stream_);
  HIPCHK(hipEventRecord(ev_[1], stream_));
  timings_.logmel_ms = -1.0f;  // resolved lazily in decode()/sync by the C ABI
}

// ------------------------------------------------------- kernel timer ---

thread_local LaunchTimer g_launch_timer;

namespace {
// The dispatch-attached event pair must not outlive the encoder pass that armed it: a launcher that throws (shape or span
// error) between kt_begin and kt_end would leave it armed for the thread's next timed launch — possibly another engine's.
struct TimerDisarm {
  ~TimerDisarm() { g_launch_timer = LaunchTimer{}; }
};
}  // namespace

void Engine::kt_begin(int cls, double flops, double bytes) {
  if (!kt_on_) return;
  Slot& sl = slots_[enc_slot_];
  const size_t idx = sl.kt_cls.size() * 2;
  while (sl.kt_events.size() < idx + 2) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    sl.kt_events.push_back(e);
  }
  sl.kt_cls.push_back(cls);
  sl.kt_flops.push_back(flops);
  sl.kt_bytes.push_back(bytes);
  // the default contraction kernels take the pair on the dispatch itself (kernels.h, LaunchTimer): kernel begin -> end
  if (cls == kKcGemm || cls == kKcEncAttn) {
    g_launch_timer.start = sl.kt_events[idx];
    g_launch_timer.stop = sl.kt_events[idx + 1];
    return;
  }
  HIPCHK(hipEventRecord(sl.kt_events[idx], stream_));
}

void Engine::kt_end() {
  if (!kt_on_) return;
  if (g_launch_timer.start) {
    g_launch_timer = LaunchTimer{};
    return;
  }
  Slot& sl = slots_[enc_slot_];
  HIPCHK(hipEventRecord(sl.kt_events[(sl.kt_cls.size() - 1) * 2 + 1], stream_));
}

void Engine::resolve_kernel_stats(int slot) {
  Slot& sl = slots_[slot];
  // class names = the kernels the current options select (what rocprofv3 lists)
  const long gv = gemm_variant;
  kstats_[kKcGemm].name = bf16 ? "gemm_bf16_planes" : "gemm_planes";  // the class: gemm_planes_pp16 / _tile instantiations
  kstats_[kKcEncAttn].name = bf16 ? "encoder_attention_bf16" : "encoder_attention_planes";
  kstats_[kKcGemmAlt].name = gv == 0 ? "gemm_f32_tile" : "gemm_split16_tile";
  kstats_[kKcEncAttnAlt].name = attn_variant == 0 ? "encoder_attention_f32" : "encoder_attention_split";
  for (auto& k : kstats_) k.launches = 0, k.ms = 0, k.flops = 0, k.bytes = 0;
  for (size_t i = 0; i < sl.kt_cls.size(); ++i) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, sl.kt_events[2 * i], sl.kt_events[2 * i + 1]) != hipSuccess) continue;
    KernelStat& k = kstats_[sl.kt_cls[i]];
    k.launches += 1;
    k.ms += ms;
    k.flops += sl.kt_flops[i];
    k.bytes += sl.kt_bytes[i];
  }
}

// ------------------------------------------------------------ encoder ---

void Engine::require_idle() const {
  // A synchronous call would take the next pipeline slot: with batches in flight that slot may still hold an
  // uncollected batch (its cross-KV cache, its id buffers).  Refuse BEFORE anything is enqueued.
  if (!inflight_.empty()) throw Error(kErrInvalidArg, "collect the submitted batches before a synchronous call");
}

void Engine::encode(const float* d_mel, int batch) {
  require_idle();
  check_beam_call(false, max_positions > 0 && full_bf16 != 0);  // (a full-length call: check_full_call holds the rest)
  select_stream(false);
  encode_enqueue(d_mel, batch);
}

namespace {
// One encoder contraction as encode_enqueue describes it, once, for whichever kernel runs it.  `g` holds the addressing
// (M, lda, a_rpb, a_bs, c_rpb, c_bs, ldc, pos, kv_*, R), the A operand as planes (A, a_plane) and the LayerNorm-fusion
// request (ln_*); its weight side (W, bias, N, K, scales) comes from the record, its output from the fields below.
struct EncGemm {
  PlaneGemmArgs g;
  const EncLinear* w = nullptr;
  int epi = 0;
  const float* A32 = nullptr;  // the A operand as fp32
  // The output in both forms: the consumer decides (to_planes).  The residual stream and the fp32 cross-KV cache have C32 only.
  float* C32 = nullptr;
  unsigned short* P = nullptr;
  long p_plane = 0;
  const float* out_scale = nullptr;  // of P: one scale, or three with `seg` columns each; null = 1
  int seg = 0;
  bool to_planes = false;
  // the hand-over behind a fall-back kernel in front of a plane consumer, where it is not "the rows [M][ldc] at C32 ->
  // ws_.cvt": the padded rows of conv1's output
  const float* cvt_src = nullptr;
  unsigned short* cvt_dst = nullptr;
  long cvt_plane = 0, cvt_rows = 0;
};
struct PlaneOperand {  // where a plane consumer finds its A operand
  const unsigned short* p;
  long plane;
};
}  // namespace

void Engine::encode_enqueue(const float* d_mel, int batch) {
  if (dims_.n_audio_state == 0) throw Error(kErrUnsupported, "front-end-only engine: no model weights loaded");
  ensure_batch(batch);
  TimerDisarm disarm_on_exit;
  // per-launch event pairs (bench.py's live roofline figures) on every kernel_timers-th encoder pass: an event pair
  // costs the stream a few microseconds per launch, which 41 launches per pass make visible in the pipeline period
  kt_on_ = kernel_timers > 0 && (enc_count_++ % kernel_timers) == 0;
  // The encoder graph.  Every contraction chooses its kernel BY ITSELF: the plane kernels
  // (k_gemm_planes.hip, k_attention_planes.hip: operands as two fp16 planes, made by the kernel that produces them)
  // unless the load-time slack check flagged that contraction's operand (GemmScale::f16_ok, upload_weights) or an
  // explicit gemm_variant / attn_variant asks for the fp32-storage kernels (k_gemm.hip, k_attention.hip: full fp32
  // operand range).  A tensor has exactly one consumer, so its format follows the consumer: a plane kernel that feeds a
  // flagged contraction writes fp32 (C instead of P), LayerNorm has both forms, and where a fall-back kernel feeds a
  // plane kernel its fp32 output is split by launch_f32_to_planes into the scratch planes ws_.cvt.  The residual
  // stream x stays fp32 throughout.  That rule is enc_gemm below; every contraction is described once and handed to it.
  // bf16 storage mode (option "bf16") is the same graph with every contraction "on planes": each operand is ONE bf16
  // matrix (k_gemm_bf16.hip, encoder_attention_planes<true>), so every plane offset is 0 and every scale 1; x and the
  // API's enc_out stay fp32, the cross-KV cache of the slot is written as bf16 (half the bytes, same layout).
  const wtw::Dims& c = dims_;
  const int T0 = mel_frames(), T = c.n_audio_ctx, d = c.n_audio_state, M = batch * T, nm = c.n_mels;
  const bool bf = bf16 != 0;
  const long Bw = ws_.batch;  // plane strides follow the workspace, not the call
  const int cus = (stream_ == stream_masked_ && stream_masked_) ? enc_cus_masked_ : n_cu_;  // CUs of this stream
  Slot& slot = slots_[enc_slot_];
  // the slot's cross-KV cache may still be read by the decoder of the batch before last
  if (slot.used) HIPCHK(hipStreamWaitEvent(stream_, slot.dec_done, 0));
  slot.kt_cls.clear();
  slot.kt_flops.clear();
  slot.kt_bytes.clear();
  slot.batch = batch;
  if (!trace_base_ && getenv("WT_TRACE_PIPELINE")) {
    HIPCHK(hipEventCreate(&trace_base_));
    HIPCHK(hipEventRecord(trace_base_, stream_));
  }
  HIPCHK(hipMemsetAsync(slot.d_flag, 0, sizeof(int), stream_));
  HIPCHK(hipEventRecord(slot.enc_begin, stream_));
  unsigned short* const lnp = reinterpret_cast<unsigned short*>(ws_.ln);
  unsigned short* const qkvp = reinterpret_cast<unsigned short*>(ws_.qkv);
  unsigned short* const attp = reinterpret_cast<unsigned short*>(ws_.att);
  unsigned short* const hidp = reinterpret_cast<unsigned short*>(ws_.hid);
  auto plane = [&](long elems) { return bf ? 0 : elems; };  // elements between the hi and the lo plane of a tensor
  const long melT_plane = plane(Bw * (T0 + 2) * nm + 128), h1p_plane = plane(Bw * (T0 + 2) * d + 128);
  const long ln_plane = plane(Bw * T * d), qkv_plane = plane(Bw * T * 3 * d), hid_plane = plane(Bw * T * 4 * d);
  const long cvt_plane = plane(Bw * T * 4 * d), e_plane = plane(Bw * T * d);
  const bool absorb = absorb_for(batch);
  const int alt = alt_gemm_variant();
  auto on_planes = [&](const EncLinear& w) { return bf || gemm_on_planes(w.sc); };
  auto a_scale = [&](const EncLinear& w) { return bf ? 1.0f : w.sc.a; };  // the scale of the A planes made for `w`
  // a transpose or LayerNorm into planes counts 2 x its fp32 bytes; into one bf16 plane 1.5 x (bench.py's roofline table)
  const double planes_io = bf ? 1.5 : 2.0;

  auto hand_over = [&](const float* src, unsigned short* dst, long dst_plane, long rows, int ld, const float* scales, int seg) {
    kt_begin(kKcConvert, 0, 2.0 * rows * ld * 4);
    launch_f32_to_planes(src, dst, dst_plane, rows, ld, scales, seg, stream_);
    kt_end();
    return PlaneOperand{dst, dst_plane};
  };
  // The LayerNorm that follows a GEMM whose output is the residual stream x (conv2, out-projection, fc2) is made by
  // that GEMM's epilogue when its tile owns whole rows and both sides run on planes; ln_done then tells the
  // consumer's side not to launch the LayerNorm kernel.
  bool ln_done = false;
  static const bool no_ln_fuse = getenv("WT_NO_LN_FUSE") != nullptr;  // measurement knob: separate LayerNorm launches
  auto fuse_ln = [&](EncGemm& e, const float* gain, const float* shift, const EncLinear& consumer) {
    if (no_ln_fuse || !on_planes(consumer)) return;
    e.g.ln_g = gain; e.g.ln_b = shift; e.g.ln_P = lnp; e.g.ln_plane = ln_plane; e.g.ln_scale = a_scale(consumer);
  };
  // Runs a contraction on the kernel its record and the mode select and leaves the result in the consumer's format;
  // returns where a plane consumer finds it.
  auto enc_gemm = [&](const EncGemm& e) {
    const EncLinear& w = *e.w;
    const double flops = 2.0 * e.g.M * w.N * double(w.k);
    if (on_planes(w)) {
      PlaneGemmArgs g = e.g;
      g.W = bf ? w.wbf : w.wp; g.bias = w.bias; g.N = w.N; g.K = bf ? w.kbf : w.kp;
      if (e.to_planes) {
        g.P = e.P; g.p_plane = e.p_plane; g.seg = e.seg;
        for (int i = 0; e.out_scale && i < (e.seg ? 3 : 1); ++i) g.out_scale[i] = e.out_scale[i];
      } else {
        g.C = e.C32;
      }
      if (!bf) g.n_cu = cus, g.a_scale = w.sc.a, g.w_scale = w.sc.w;
      kt_begin(kKcGemm, flops, 0);
      ln_done = bf ? launch_gemm_bf16_planes(g, e.epi, stream_) : launch_gemm_planes(g, e.epi, stream_);
      kt_end();
      return PlaneOperand{g.P, g.p_plane};
    }
    GemmArgs g;
    g.A = e.A32; g.W = w.w32; g.C = e.C32; g.bias = w.bias; g.R = e.g.R; g.pos = e.g.pos;
    g.M = e.g.M; g.N = w.N; g.K = w.k32;
    g.a_rpb = e.g.a_rpb; g.a_bs = e.g.a_bs; g.lda = e.g.lda; g.c_rpb = e.g.c_rpb; g.c_bs = e.g.c_bs; g.ldc = e.g.ldc;
    g.pos_period = e.g.pos_period; g.kv_batch = e.g.kv_batch; g.kv_heads = e.g.kv_heads; g.kv_dmodel = e.g.kv_dmodel;
    g.variant = alt; g.a_scale = w.sc.a; g.w_scale = w.sc.w;
    kt_begin(kKcGemmAlt, flops, 0);
    launch_gemm(g, e.epi, stream_);
    kt_end();
    if (!e.to_planes) return PlaneOperand{nullptr, 0};
    if (e.cvt_src) return hand_over(e.cvt_src, e.cvt_dst, e.cvt_plane, e.cvt_rows, e.g.ldc, e.out_scale, e.seg);
    return hand_over(e.C32, ws_.cvt, cvt_plane, e.g.M, e.g.ldc, e.out_scale, e.seg);
  };
  auto layernorm_for = [&](const EncLinear& consumer, const float* g, const float* b) {
    if (ln_done) {  // the producing GEMM's epilogue has written these planes
      ln_done = false;
      return;
    }
    kt_begin(kKcLayerNorm, 0, planes_io * M * d * 4);
    if (on_planes(consumer)) {
      launch_layernorm_planes(ws_.x, lnp, ln_plane, a_scale(consumer), nullptr, g, b, M, d, stream_, nullptr, bf);
    } else {
      launch_layernorm(ws_.x, ws_.ln, g, b, M, d, stream_);
    }
    kt_end();
  };

  kt_begin(kKcTranspose, 0, planes_io * batch * nm * T0 * 4);
  if (on_planes(conv1_)) {
    launch_mel_transpose_planes(d_mel, ws_.melTp, melT_plane, a_scale(conv1_), batch, nm, T0, nm, stream_, bf);
  } else {
    launch_mel_transpose(d_mel, ws_.melT, batch, nm, T0, stream_);
  }
  kt_end();
  const float s_conv2 = a_scale(conv2_);
  {
    EncGemm e;  // conv1 + GELU: rows (clip, t) read melT rows t..t+2 (input t-1..t+1); row t lands at padded row t + 1 of h1
    e.w = &conv1_; e.epi = kEpiBias | kEpiGelu;
    e.A32 = ws_.melT; e.g.A = ws_.melTp; e.g.a_plane = melT_plane;
    e.g.M = batch * T0; e.g.a_rpb = T0; e.g.a_bs = long(T0 + 2) * nm; e.g.lda = nm;
    e.g.c_rpb = T0; e.g.c_bs = long(T0 + 2) * d; e.g.ldc = d;
    e.to_planes = on_planes(conv2_); e.C32 = ws_.h1p + d; e.P = ws_.h1pp + d; e.p_plane = h1p_plane; e.out_scale = &s_conv2;
    // (the pad rows of h1p are zero and stay zero as planes)
    e.cvt_src = ws_.h1p; e.cvt_dst = ws_.h1pp; e.cvt_plane = h1p_plane; e.cvt_rows = long(batch) * (T0 + 2);
    enc_gemm(e);
  }
  {
    EncGemm e;  // conv2 (stride 2) + GELU + positional embedding: output t reads padded rows 2t..2t+2
    e.w = &conv2_; e.epi = kEpiBias | kEpiGelu | kEpiPos;
    e.A32 = ws_.h1p; e.g.A = ws_.h1pp; e.g.a_plane = h1p_plane;
    e.g.M = M; e.g.a_rpb = T; e.g.a_bs = long(T0 + 2) * d; e.g.lda = 2 * d; e.g.ldc = d;
    e.g.pos = enc_pos; e.g.pos_period = T;
    e.C32 = ws_.x;
    fuse_ln(e, enc_layers_[0].attn_ln_g, enc_layers_[0].attn_ln_b, enc_layers_[0].qkv);
    enc_gemm(e);
  }
  constexpr float kQScale = 0.125f * 1.44269504088896340736f;  // d_head^-1/2 * log2(e): softmax as exp2
  for (int l = 0; l < c.n_audio_layer; ++l) {
    const EncLayer& L = enc_layers_[l];
    const bool op = on_planes(L.out);
    // the plane attention writes planes, so its consumer (the out-projection) must take them
    const bool ap = bf || (gemm_variant < 0 && attn_variant == 4 && L.attn_f16_ok && op);
    const int attn_alt = attn_variant == 4 ? 1 : int(attn_variant);  // fall-back form: three bf16 planes
    const float qkv_scales[3] = {kQScale * L.q, L.k, L.v}, s_out = a_scale(L.out), s_fc2 = a_scale(L.fc2);

    layernorm_for(L.qkv, L.attn_ln_g, L.attn_ln_b);
    EncGemm q;  // q | k | v: the attention kernel's operand planes, or fp32 for the fall-back attention
    q.w = &L.qkv; q.epi = kEpiBias;
    q.A32 = ws_.ln; q.g.A = lnp; q.g.a_plane = ln_plane; q.g.M = M; q.g.lda = d; q.g.ldc = 3 * d;
    q.to_planes = ap; q.C32 = ws_.qkv; q.P = qkvp; q.p_plane = qkv_plane;
    if (!bf) q.out_scale = qkv_scales, q.seg = d;  // (the bf16 attention takes q unscaled)
    const PlaneOperand qkv_src = enc_gemm(q);
    PlaneOperand att_src{attp, ln_plane};  // the plane out-projection's operand
    const double attn_flops = 4.0 * batch * c.n_audio_head * double(T) * T * 64;
    if (ap) {
      kt_begin(kKcEncAttn, attn_flops, 0);
      if (bf) {
        launch_encoder_attention_bf16(qkv_src.p, attp, batch, T, c.n_audio_head, stream_);
      } else {
        launch_encoder_attention_planes(qkv_src.p, qkv_src.plane, attp, ln_plane, batch, T, c.n_audio_head, L.q, L.k, L.v,
                                        L.out.sc.a, stream_);
      }
      kt_end();
    } else {
      kt_begin(kKcEncAttnAlt, attn_flops, 0);
      launch_encoder_attention(ws_.qkv, ws_.att, batch, T, c.n_audio_head, attn_alt, stream_);
      kt_end();
      if (op) att_src = hand_over(ws_.att, ws_.cvt, cvt_plane, M, d, &s_out, 0);
    }
    EncGemm o;
    o.w = &L.out; o.epi = kEpiBias | kEpiResidual;
    o.A32 = ws_.att; o.g.A = att_src.p; o.g.a_plane = att_src.plane; o.g.M = M; o.g.lda = d; o.g.ldc = d;
    o.C32 = ws_.x; o.g.R = ws_.x;
    fuse_ln(o, L.mlp_ln_g, L.mlp_ln_b, L.fc1);
    enc_gemm(o);
    layernorm_for(L.fc1, L.mlp_ln_g, L.mlp_ln_b);
    EncGemm f1;
    f1.w = &L.fc1; f1.epi = kEpiBias | kEpiGelu;
    f1.A32 = ws_.ln; f1.g.A = lnp; f1.g.a_plane = ln_plane; f1.g.M = M; f1.g.lda = d; f1.g.ldc = 4 * d;
    f1.to_planes = on_planes(L.fc2); f1.C32 = ws_.hid; f1.P = hidp; f1.p_plane = hid_plane; f1.out_scale = &s_fc2;
    const PlaneOperand hid_src = enc_gemm(f1);
    EncGemm f2;
    f2.w = &L.fc2; f2.epi = kEpiBias | kEpiResidual;
    f2.A32 = ws_.hid; f2.g.A = hid_src.p; f2.g.a_plane = hid_src.plane; f2.g.M = M; f2.g.lda = 4 * d; f2.g.ldc = d;
    f2.C32 = ws_.x; f2.g.R = ws_.x;
    if (l + 1 < c.n_audio_layer) {
      fuse_ln(f2, enc_layers_[l + 1].attn_ln_g, enc_layers_[l + 1].attn_ln_b, enc_layers_[l + 1].qkv);
    } else {  // the encoder's final LayerNorm: also the API's fp32 enc_out and the non-finite flag
      fuse_ln(f2, enc_ln_post_g, enc_ln_post_b, cross_kv_);
      if (f2.g.ln_P) {
        f2.g.ln_y32 = ws_.enc_out; f2.g.nonfinite = slot.d_flag;
        // absorbed cross-attention: these planes ARE what the decoder streams (no cross-KV projection)
        if (absorb) f2.g.ln_P = slot.e_planes, f2.g.ln_plane = e_plane;
      }
    }
    enc_gemm(f2);
  }
  const bool kp = on_planes(cross_kv_), post_fused = ln_done;
  ln_done = false;
  // bf16 storage mode keeps two habits of its own here, both inputs of bench.py's roofline table: it makes the ln_post
  // record even when the LayerNorm was fused, with the flag copy inside its event pair, ...
  if (bf || !post_fused) kt_begin(kKcLayerNorm, 0, (bf ? 2.5 : 2.0) * M * d * 4);  // ... and counts 2.5 x the fp32 bytes
  if (!post_fused) {
    if (kp) {
      launch_layernorm_planes(ws_.x, absorb ? slot.e_planes : lnp, absorb ? e_plane : ln_plane, a_scale(cross_kv_), ws_.enc_out,
                              enc_ln_post_g, enc_ln_post_b, M, d, stream_, slot.d_flag, bf);
    } else {
      launch_layernorm(ws_.x, ws_.enc_out, enc_ln_post_g, enc_ln_post_b, M, d, stream_, slot.d_flag);
    }
    if (!bf) kt_end();
  }
  HIPCHK(hipMemcpyAsync(slot.h_flag, slot.d_flag, sizeof(int), hipMemcpyDeviceToHost, stream_));
  if (bf) kt_end();
  HIPCHK(hipEventRecord(slot.enc_mid, stream_));
  // cross-attention K/V of every decoder layer, projected once per clip into the persistent cache
  // [layer][k|v][clip][head][t][64] (the reference recomputes them inside every decoder Invoke(), whisper.cpp:375) —
  // unless the decoder runs the absorbed form, which needs the planes of the encoder output and nothing else
  slot.absorbed = absorb;
  if (!absorb) {
    need_cross_kv(slot);
    EncGemm e;
    e.w = &cross_kv_; e.epi = kEpiBias | kEpiKvLayout;
    e.A32 = ws_.enc_out; e.g.A = lnp; e.g.a_plane = ln_plane; e.g.M = M; e.g.lda = d;
    e.g.c_rpb = T; e.g.kv_batch = batch; e.g.kv_heads = c.n_text_head; e.g.kv_dmodel = d;
    // its consumer, the cached cross-attention, reads fp32, or in bf16 storage mode bf16 in the same layout
    e.to_planes = bf; e.C32 = slot.cross_kv; e.P = reinterpret_cast<unsigned short*>(slot.cross_kv);
    enc_gemm(e);
  }
  HIPCHK(hipEventRecord(slot.enc_done, stream_));
  slot.used = true;
  last_enc_slot_ = enc_slot_;
  enc_slot_ = (enc_slot_ + 1) % kSlots;
}

void Engine::set_bf16(bool on) {
  require_idle();
  if (on) ensure_bf16_weights();
  if ((bf16 != 0) != on && ws_.batch > 0 && dims_.n_audio_state != 0) {
    // the zero pad rows of the two convolution inputs sit at different offsets in the two layouts
    const size_t B = ws_.batch, T0 = mel_frames();
    sync();
    HIPCHK(hipMemset(ws_.melTp, 0, (B * (T0 + 2) * dims_.n_mels + 256) * sizeof(float)));
    HIPCHK(hipMemset(ws_.h1pp, 0, (B * (T0 + 2) * dims_.n_audio_state + 256) * sizeof(float)));
    for (DecWorkspace& dw : dws_) {
      if (dw.self_kv) HIPCHK(hipMemset(dw.self_kv, 0, size_t(dims_.n_text_layer) * 2 * B * self_cap_ * dims_.n_text_state * sizeof(float)));
    }
  }
  bf16 = on ? 1 : 0;
}

// ------------------------------------------------------------ decoder ---

void Engine::decode(int batch, int64_t* ids, int32_t* n_ids, float* logits_host,
                    int logits_steps_cap) {
  require_idle();
  check_timestamp_call();
  check_language_call();
  check_beam_call(logits_host != nullptr);
  last.forget(kForgetSyncDecode);
  if (beam_size > 1) {
    decode_beam(batch, last_enc_slot_, ids, n_ids);
    return;
  }
  decode_enqueue(batch, last_enc_slot_, logits_host, logits_steps_cap);
  decode_collect(last_enc_slot_, ids, n_ids);
  if (language < 0) {  // the chain's language_head results came back with the ids (pinned copies, decode_enqueue)
    last.lang.assign(h_lang_, h_lang_ + batch);
    last.lang_prob.assign(h_lang_prob_, h_lang_prob_ + batch);
    last.lang_valid = true;
  }
}

void Engine::decode_windows(const float* pcm, int batch, const std::vector<long long>* valid_samples, std::vector<int64_t>* ids,
                            std::vector<int32_t>* n_ids) {
  float* d_mel = staging_mel(batch);
  logmel(upload_pcm(pcm, batch), batch, d_mel);
  const size_t row = max_positions > 0 ? size_t(max_positions) + 1 : 32;
  ids->assign(size_t(batch) * row, 0);
  n_ids->assign(size_t(batch), 0);
  if (max_positions > 0) {
    encode_full(d_mel, batch);
    decode_full(batch, ids->data(), int(row), n_ids->data(), valid_samples);
  } else {
    encode(d_mel, batch);
    decode(batch, ids->data(), n_ids->data(), nullptr, 0);
  }
  sync();  // pcm is read by the H2D copy on the encoder stream
}

// -------------------------------------------------- language detection ---

int Engine::lang_tokens() const {
  if (!multilingual_ || vocab_.token_translate > dims_.n_vocab) return 0;
  return int(std::max<long>(0, std::min<long>(std::min(language_count(), kLangMax), vocab_.token_translate - kLangLo)));
}

void Engine::check_language_call() const {
  if (language >= 0) return;
  auto no = [](const char* why) { throw Error(kErrUnsupported, std::string("automatic language: ") + why); };
  if (lang_tokens() < 1) no("this engine's vocabulary has no language tokens");
  if (monolith_) no("the Monolith engine forces <|en|>");
  if (beam_size > 1) no("not with beam search (beam_size > 1)");
  if (!prompt_override.empty()) no("not with a caller prompt (wt_engine_set_prompt)");
  if (!forced_ids.empty()) no("not with forced ids");
}

void Engine::set_language(long value) {
  if (value < -1 || value >= language_count()) throw Error(kErrInvalidArg, "language id out of range (-1 = automatic)");
  if (value < 0) {
    if (monolith_) throw Error(kErrUnsupported, "automatic language: the Monolith engine forces <|en|>");
    if (lang_tokens() < 1) throw Error(kErrUnsupported, "automatic language: this engine's vocabulary has no language tokens");
  }
  language = value;
}

void Engine::ensure_lang_workspace() {
  if (h_lang_) return;  // (allocated last)
  for (LangWorkspace& lw : lw_) {
    lw.probs = dev_zeroed<float>(size_t(kDecRowsMax) * kLangMax);
    lw.prob = dev_zeroed<float>(kDecRowsMax);
    lw.lang = dev_zeroed<int>(kDecRowsMax);
  }
  h_lang_probs_ = pinned<float>(size_t(kDecRowsMax) * kLangMax);
  h_lang_prob_ = pinned<float>(kDecRowsMax);
  h_lang_ = pinned<int>(kDecRowsMax);
}

void Engine::detect_language(int batch, int32_t* lang, float* probs, float* prob) {
  require_idle();
  const int n_lang = lang_tokens();
  if (n_lang < 1) throw Error(kErrUnsupported, "language detection: this engine's vocabulary has no language tokens");
  if (batch < 1 || batch > 64) throw Error(kErrInvalidArg, "language detection takes 1 to 64 clips per call");
  detect_only_ = true;
  try {
    decode_enqueue(batch, last_enc_slot_, nullptr, 0);
  } catch (...) {
    detect_only_ = false;
    throw;
  }
  detect_only_ = false;
  std::vector<int64_t> ids(size_t(batch) * 32);
  std::vector<int32_t> n(batch);
  decode_collect(last_enc_slot_, ids.data(), n.data());
  for (int b = 0; b < batch; ++b) {
    if (lang) lang[b] = h_lang_[b];
    if (prob) prob[b] = h_lang_prob_[b];
    if (probs) std::memcpy(probs + size_t(b) * n_lang, h_lang_probs_ + size_t(b) * n_lang, size_t(n_lang) * sizeof(float));
  }
}

void Engine::flush_pending() {
  if (pending_.empty()) return;
  const int p = pending_.front(), n = int(pending_.size());
  pending_.clear();
  decode_enqueue(slots_[p].batch, p, nullptr, 0, n, true);  // the rest of the group never came: a shorter chain
}

// decoder side of a pipelined submit: alone, or together with the neighbouring submits' batches (dec_pair, dec_group)
int Engine::group_of(int batch) const {
  // (WT_PAIR_MAX_BATCH: largest batch that is grouped — 32 until round 4, when a chain's rows were limited to 64)
  static const int pair_max = [] {
    const char* v = getenv("WT_PAIR_MAX_BATCH");
    return v ? atoi(v) : 32;
  }();
  if (dec_pair == 0 || !absorb_active() || batch > pair_max) return 1;
  const int g = int(std::min<long>(std::max<long>(dec_group, 2), 4));
  return std::max(1, std::min(g, kDecRowsMax / batch));
}

// Throughput form: `group` consecutive batches share one decoder chain.  Latency form — the last `last_batches` submits
// of a job (option, counted down here): a chain per batch, on spare decoder streams when the probe found any, so that the
// pipeline drains in one short chain instead of a long shared one behind two others (measured on the driver's 20-step
// command: 16.7 ms from the last encoder pass to the last token with the paired form).
void Engine::submit_decoder(int batch, int s) {
  const bool tail = last_batches > 0;
  if (tail) --last_batches;
  const int group = group_of(batch);
  if (!tail && group > 1 && ws_.batch >= group * batch) {
    if (!pending_.empty() && (slots_[pending_.front()].batch != batch || (pending_.back() + 1) % kSlots != s)) flush_pending();
    pending_.push_back(s);
    if (int(pending_.size()) == group) {
      const int a = pending_.front();
      pending_.clear();
      decode_enqueue(batch, a, nullptr, 0, group, true);
    }
  } else {
    flush_pending();
    int spare = -1;
    // The very last batch decodes on the encoder's own stream, right behind its encoder pass: that hardware queue has
    // nothing else to do once the last encoder pass is through, and the decoder streams are still busy with earlier
    // chains.  (Submitting more batches after "the last" is allowed: their encoder passes queue behind that chain.)
    // The batches before it use a spare decoder stream when the probe found one.
    if (tail && last_batches == 0) spare = kEncAsDec;
    else if (tail && n_spare_streams_ > 0) spare = n_dec_streams_ + int(last_batches % n_spare_streams_);
    decode_enqueue(batch, s, nullptr, 0, 1, true, spare);
  }
  inflight_.push_back(s);
}

void Engine::submit(const float* d_mel, int batch) {
  check_timestamp_call();
  if (max_positions > 0) throw Error(kErrUnsupported, "full-length decoding (max_positions) runs on the synchronous entry points only, not in the pipeline");
  if (beam_size > 1) throw Error(kErrUnsupported, "beam search runs on the synchronous entry points only, not in the pipeline");
  check_language_call();
  last.forget(kForgetSubmit);  // (the getters report the last decode, and this one has no scores)
  if (int(inflight_.size()) >= kSlots) throw Error(1, "pipeline is full (24 batches in flight): collect() first");
  if (batch > 64) throw Error(1, "decoder batches are limited to 64 clips per call");
  select_stream(true);
  if (inflight_.empty()) ensure_batch(group_of(batch) * batch);  // the group's decoder rows; never grown in flight
  encode_enqueue(d_mel, batch);
  submit_decoder(batch, last_enc_slot_);
}

void Engine::submit_pcm(const float* d_pcm, int batch) {
  check_timestamp_call();
  if (max_positions > 0) throw Error(kErrUnsupported, "full-length decoding (max_positions) runs on the synchronous entry points only, not in the pipeline");
  if (beam_size > 1) throw Error(kErrUnsupported, "beam search runs on the synchronous entry points only, not in the pipeline");
  check_language_call();
  last.forget(kForgetSubmit);  // (the getters report the last decode, and this one has no scores)
  if (int(inflight_.size()) >= kSlots) throw Error(1, "pipeline is full (24 batches in flight): collect() first");
  if (batch > 64) throw Error(1, "decoder batches are limited to 64 clips per call");
  select_stream(true);
  if (inflight_.empty()) ensure_batch(group_of(batch) * batch);
  // one staging mel buffer: the front end of batch k+1 follows the encoder of batch k on the same stream
  float* d_mel = staging_mel(batch);
  logmel(d_pcm, batch, d_mel);
  encode_enqueue(d_mel, batch);
  submit_decoder(batch, last_enc_slot_);
}

void Engine::collect(int64_t* ids, int32_t* n_ids) {
  if (inflight_.empty()) throw Error(1, "collect() without a submitted batch");
  const int slot = inflight_.front();
  if (std::find(pending_.begin(), pending_.end(), slot) != pending_.end()) flush_pending();  // its group never filled: decode now
  inflight_.erase(inflight_.begin());
  decode_collect(slot, ids, n_ids);
}

std::vector<long long> Engine::prompt() const {
  if (!prompt_override.empty()) return prompt_override;
  // EncDec (whisper.cpp:327-339): [sot, 50259 + language, transcribe, notimestamps] whatever `multilingual` is
  // (the ids come from the Vocab, which transform_vocab_multilingual shifted or not, whisper.cpp:218-226).
  // Monolith: the forced decoder ids HF generate() applies inside the reference's single graph
  // (export/generate.py:24-30): English-only checkpoints [sot, notimestamps] — the head of kGoldenGeneratedIDs,
  // whisper.h:27-32 — multilingual ones [sot, language, transcribe, notimestamps].
  // option timestamps: the same prompts without their last id, <|notimestamps|>
  if (monolith_ && !multilingual_) {
    if (timestamps) return {vocab_.token_sot};
    return {vocab_.token_sot, vocab_.token_not};
  }
  const long long task_id = task ? vocab_.token_translate : vocab_.token_transcribe;  // option task (set_task)
  if (timestamps) return {vocab_.token_sot, kLangLo + std::max<long>(language, 0), task_id};
  // (language = -1: position 1 is a placeholder that language_head overwrites on the device, decode_enqueue)
  return {vocab_.token_sot, kLangLo + std::max<long>(language, 0), task_id, vocab_.token_not};
}

void Engine::set_task(long value) {
  if (value < 0 || value > 1) throw Error(kErrInvalidArg, "task must be 0 (transcribe) or 1 (translate)");
  if (value == 1) {
    auto no = [](const char* why) { throw Error(kErrUnsupported, std::string("task = translate: ") + why); };
    if (!multilingual_) no("the engine was created with multilingual = 0");
    if (monolith_) no("the Monolith engine's single graph takes no task");
    if (vocab_.token_translate < 0 || vocab_.token_translate >= dims_.n_vocab) no("the model's vocabulary has no <|translate|> id");
  }
  task = value;
}

void Engine::check_task_call() const {
  if (task && !prompt_override.empty()) {
    throw Error(kErrUnsupported, "task = translate: not with a caller prompt (wt_engine_set_prompt), which names its own task");
  }
}

void Engine::set_language_candidates(const int32_t* langs, int n) {
  require_idle();
  if (n < 0 || n > kLangMax || (n > 0 && !langs)) throw Error(kErrInvalidArg, "language candidates: 0 (clears the list) to 128 language ids");
  if (monolith_) throw Error(kErrUnsupported, "language candidates: the Monolith engine forces <|en|>");
  if (lang_tokens() < 1) throw Error(kErrUnsupported, "language candidates: this engine's vocabulary has no language tokens");
  unsigned words[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    if (langs[i] < 0 || langs[i] >= lang_tokens()) throw Error(kErrInvalidArg, "language candidates: an id outside [0, wt_language_count())");
    words[langs[i] >> 5] |= 1u << (langs[i] & 31);
  }
  std::vector<int> v;
  for (int r = 0; r < lang_tokens(); ++r) {
    if ((words[r >> 5] >> (r & 31)) & 1u) v.push_back(r);
  }
  if (n > 0) {  // (a list always holds an id below lang_tokens(): the kernel's contract)
    if (!d_lang_allow_) d_lang_allow_ = dev_zeroed<unsigned>(4);
    sync();
    HIPCHK(hipMemcpy(d_lang_allow_, words, sizeof(words), hipMemcpyHostToDevice));
  }
  language_candidates = v;
}

void Engine::ensure_full_language_workspace() {
  ensure_lang_workspace();
  if (fl_.sot_ids) return;  // (allocated last)
  fl_.hold = dev_zeroed<int>(kFullClipsMax);
  fl_.h_hold = pinned<int>(kFullClipsMax);
  long long* const ids = dev_zeroed<long long>(kFullClipsMax);
  const std::vector<long long> sot(size_t(kFullClipsMax), vocab_.token_sot);
  HIPCHK(hipMemcpy(ids, sot.data(), sot.size() * sizeof(long long), hipMemcpyHostToDevice));
  fl_.sot_ids = ids;
}

void Engine::enqueue_full_language(const DecWorkspace& dw, int dec, bool split, int batch, long long* ids, int stride, int id_pos,
                                   hipStream_t st) {
  LangWorkspace& lw = lw_[dec];
  LanguageRowsArgs a;
  a.x = split ? dw.xb : dw.xd; a.xpart = split ? dw.xpart : nullptr; a.ln_g = dec_ln_g; a.ln_b = dec_ln_b; a.tok_emb = tok_emb;
  a.clips = a.x_rows = batch; a.x_rows_per_clip = 1; a.d = dims_.n_text_state; a.n_vocab = dims_.n_vocab;
  a.lang_lo = int(kLangLo); a.n_lang = lang_tokens();
  a.allow = language_candidates.empty() ? nullptr : d_lang_allow_; a.hold = fl_.hold;
  a.probs = lw.probs; a.lang = lw.lang; a.lang_prob = lw.prob;
  a.ids[0] = ids; a.ids_rows[0] = kFullClipsMax;  // (the rows both tables are allocated with)
  a.ids_stride[0] = stride; a.id_pos = id_pos; a.fan = 1;
  launch_language_head_rows(a, st);
  HIPCHK(hipMemcpyAsync(h_lang_, lw.lang, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_lang_prob_, lw.prob, size_t(batch) * sizeof(float), hipMemcpyDeviceToHost, st));
}

void Engine::detect_windows(const float* pcm, int batch, int32_t* lang, float* prob) {
  float* d_mel = staging_mel(batch);
  logmel(upload_pcm(pcm, batch), batch, d_mel);
  encode_full(d_mel, batch);
  detect_language(batch, lang, nullptr, prob);
  sync();  // pcm is read by the H2D copy on the encoder stream
}

std::vector<long long> Engine::fed_prompt() const {
  std::vector<long long> out;
  if (!context_ids.empty()) {  // Whisper's initial_prompt / condition_on_previous_text: <|startofprev|> + the previous ids
    out.push_back(vocab_.token_prev);
    out.insert(out.end(), context_ids.begin(), context_ids.end());
  }
  const std::vector<long long> tail = prompt();
  out.insert(out.end(), tail.begin(), tail.end());
  return out;
}

void Engine::set_context(const int64_t* ids, int n) {
  if (n < 0 || n > kContextIdsMax || (n > 0 && !ids)) throw Error(kErrInvalidArg, "context: 0 .. 4096 ids");
  if (n == 0) {
    context_ids.clear();
    return;
  }
  if (monolith_) throw Error(kErrUnsupported, "context: not on a Monolith engine (the reference's single graph takes no prompt)");
  if (!has_prev_token()) {
    throw Error(kErrUnsupported, "context: the model's vocabulary has no <|startofprev|> id (token_prev >= n_vocab)");
  }
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= dims_.n_vocab) throw Error(kErrInvalidArg, "context token id outside the model's vocabulary");
  }
  const int keep = std::min(n, context_keep());  // the LAST n_text_ctx / 2 - 1 ids, as Whisper's decoder keeps them
  context_ids.assign(ids + (n - keep), ids + n);
  clip_contexts.clear();  // one kind of context at a time
}

void Engine::set_contexts(const int64_t* ids, const int32_t* offsets, int n_clips) {
  if (n_clips < 0 || n_clips > 64 || (n_clips > 0 && !offsets)) throw Error(kErrInvalidArg, "contexts: 0 .. 64 clips");
  if (n_clips == 0) {
    clip_contexts.clear();
    return;
  }
  if (offsets[0] < 0) throw Error(kErrInvalidArg, "contexts: offsets must start at 0 or above and never decrease");
  for (int b = 0; b < n_clips; ++b) {
    if (offsets[b + 1] < offsets[b] || offsets[b + 1] - offsets[b] > kContextIdsMax) {
      throw Error(kErrInvalidArg, "contexts: offsets must never decrease, at most 4096 ids per clip");
    }
  }
  if (offsets[n_clips] > offsets[0] && !ids) throw Error(kErrInvalidArg, "contexts: NULL ids");
  if (offsets[n_clips] > offsets[0]) {  // some clip has a context (empty ones all round need no <|startofprev|>)
    if (monolith_) throw Error(kErrUnsupported, "contexts: not on a Monolith engine (the reference's single graph takes no prompt)");
    if (!has_prev_token()) {
      throw Error(kErrUnsupported, "contexts: the model's vocabulary has no <|startofprev|> id (token_prev >= n_vocab)");
    }
  }
  for (int32_t i = offsets[0]; i < offsets[n_clips]; ++i) {
    if (ids[i] < 0 || ids[i] >= dims_.n_vocab) throw Error(kErrInvalidArg, "context token id outside the model's vocabulary");
  }
  std::vector<std::vector<long long>> v(static_cast<size_t>(n_clips));
  for (int b = 0; b < n_clips; ++b) {
    const int n = offsets[b + 1] - offsets[b], keep = std::min(n, context_keep());
    v[size_t(b)].assign(ids + offsets[b] + (n - keep), ids + offsets[b + 1]);
  }
  clip_contexts = v;
  context_ids.clear();
}

void Engine::set_suppress(const int64_t* ids, int n, const int64_t* first_ids, int n_first) {
  if (n < 0 || n > kSuppressIdsMax || n_first < 0 || n_first > kSuppressIdsMax || (n > 0 && !ids) || (n_first > 0 && !first_ids)) {
    throw Error(kErrInvalidArg, "suppress: 0 .. 1024 ids per list");
  }
  require_idle();  // (a chain in flight reads the buffer)
  if (n == 0 && n_first == 0) {
    suppress_ids.clear(), suppress_first_ids.clear();
    return;
  }
  if (monolith_) throw Error(kErrUnsupported, "suppress: not on a Monolith engine (the reference's single graph takes no logit filter)");
  std::vector<int> host;
  for (int i = 0; i < n + n_first; ++i) {
    const int64_t id = i < n ? ids[i] : first_ids[i - n];
    if (id < 0 || id >= dims_.n_vocab) throw Error(kErrInvalidArg, "suppress: a token id outside the model's vocabulary");
    if (i < n && id == vocab_.token_eot) {
      throw Error(kErrInvalidArg, "suppress: EOT cannot be suppressed at every position (the allowed set must never be empty)");
    }
    host.push_back(int(id));
  }
  bind_device();
  if (!d_suppress_) d_suppress_ = dev_zeroed<int>(2 * size_t(kSuppressIdsMax));
  sync();  // full-length calls are synchronous: nothing reads the buffer now
  HIPCHK(hipMemcpy(d_suppress_, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));  // (blocking)
  suppress_ids.assign(host.begin(), host.begin() + n);
  suppress_first_ids.assign(host.begin() + n, host.end());
}

void Engine::set_suppress_default(bool on) {
  if (!on) return set_suppress(nullptr, 0, nullptr, 0);
  std::vector<long long> a, f;
  default_suppress(vocab_, dims_.n_vocab, &a, &f);
  if (a.empty() && f.empty()) throw Error(kErrUnsupported, "suppress_default: the vocabulary yields no id below the model's n_vocab");
  if (a.size() > size_t(kSuppressIdsMax) || f.size() > size_t(kSuppressIdsMax)) throw Error(kErrUnsupported, "suppress_default: more than 1024 ids");
  static_assert(sizeof(long long) == sizeof(int64_t), "id lists are int64");
  set_suppress(reinterpret_cast<const int64_t*>(a.data()), int(a.size()), reinterpret_cast<const int64_t*>(f.data()), int(f.size()));
}

std::vector<long long> Engine::fed_prompt_of(int clip) const {
  std::vector<long long> out;
  const std::vector<long long>& c = clip_contexts[size_t(clip)];
  if (!c.empty()) {
    out.push_back(vocab_.token_prev);
    out.insert(out.end(), c.begin(), c.end());
  }
  const std::vector<long long> tail = prompt();
  out.insert(out.end(), tail.begin(), tail.end());
  return out;
}

// ------------------------------------------------------ the decoder pass ---

namespace {
// WT_DEC_KERNEL_TIMERS=1 (diagnostics, eager launches only): an event pair around a decoder launch of class `cls`
// (finish_slot's kNames); without timers the launch alone
template <class F>
void timed(DecTimers* t, int cls, F&& launch) {
  if (!t) return launch();
  while (t->ev.size() < t->used + 2) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    t->ev.push_back(e);
  }
  HIPCHK(hipEventRecord(t->ev[t->used], t->stream));
  launch();
  HIPCHK(hipEventRecord(t->ev[t->used + 1], t->stream));
  t->cls.push_back(cls);
  t->used += 2;
}
}  // namespace

int Engine::replay_or_capture(const std::vector<long long>& key, hipStream_t st, bool graphs, const char* label,
                              const std::function<int()>& enqueue) {
  if (graphs) {
    auto it = graphs_.find(key);
    if (it != graphs_.end()) {
      HIPCHK(hipGraphLaunch(it->second.exec, st));
      return it->second.steps;
    }
  }
  const int steps = enqueue();  // eager the first time (the kernels' one-time set-up), then captured for the next calls
  if (graphs) {
    try {
      graphs_.emplace(key, GraphEntry{capture_graph(st, [&] { enqueue(); }), steps});
    } catch (const std::exception& e) {
      (void)hipGetLastError();
      use_graphs = 0;
      std::fprintf(stderr, "[wt] %s hipGraph capture failed (%s): continuing with eager launches\n", label, e.what());
    }
  }
  return steps;
}

int Engine::run_segments(int len, hipStream_t st, bool capturable, const char* label,
                         const std::function<std::vector<long long>(int)>& key_of,
                         const std::function<int(int, int)>& enqueue_segment, const DonePoll& poll, int& steps) {
  for (int lo = 0; lo < len; lo += 32) {
    const int hi = std::min(len, lo + 32);
    steps += replay_or_capture(key_of(lo), st, use_graphs && capturable, label, [&] { return enqueue_segment(lo, hi); });
    if (hi == len || !poll.flags) continue;
    // every flag set: the remaining segments would change nothing
    HIPCHK(hipMemcpyAsync(poll.mirror, poll.flags, size_t(poll.n) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    bool all = true;
    for (int i = 0; i < poll.n; ++i) all = all && poll.mirror[i] != 0;
    if (all) return hi;
  }
  return len;
}

int Engine::cross_chunks_for(int batch) const {
  int chunks = int(cross_chunks);  // 1, 2, 4 or 8 (wt_engine_set_option), 0 = by batch size
  if (chunks == 0) {
    chunks = 1;
    while (chunks < 8 && batch * dims_.n_text_head * chunks < 192) chunks *= 2;
  }
  return chunks;
}

// key chunks of the absorbed form: clips x chunks ~ `blocks` blocks, a chunk a whole number of 32-key tiles
// (option abs_chunks; 0 = 256 / clips: one block per CU when the decoder has the chip; pipelined 128 / clips — fewer,
// longer blocks: a block costs ~9 us before its first tile, and the decoders share the CUs the encoder leaves)
// (bf16 storage mode: half the bytes per key row, so half as many blocks again: 122.5 k against 120.5 k on configs[3])
int Engine::abs_chunks_for(int clips, int blocks) const {
  const int n_abs = abs_chunks > 0 ? int(abs_chunks) : std::min(16, std::max(1, (blocks + clips - 1) / clips));
  return std::min(n_abs, (dims_.n_audio_ctx + 31) / 32);
}

void Engine::check_prompt_ids(const std::vector<long long>& prompt, int code) const {
  for (long long id : prompt) {
    if (id < 0 || id >= dims_.n_vocab) throw Error(code, "prompt token id outside the model's vocabulary");
  }
}

// One decoder pass: every layer over the M = np * B rows of positions pos0 .. pos0 + np - 1 (row = p * B + sequence)
// and, when p.best is set, the final LayerNorm + logits GEMM of the last position's rows.  This is the launch sequence
// of every decode chain; greedy, beam search and full-length decoding differ in what they put into the DecPass only.
void Engine::decoder_pass(const DecPass& p, hipStream_t st) {
  const wtw::Dims& c = dims_;
  const int d = c.n_text_state, T = c.n_audio_ctx, H = c.n_text_head, V = c.n_vocab;
  const DecWorkspace& dw = *p.dw;
  DecTimers* const tm = p.timers;
  const int B = p.B, M = p.np * B;
  const bool bf = p.bf, split = p.split;  // bf16 storage mode: bf16 weights and caches (element size 2 in the cache offsets)
  const size_t kv_slab = size_t(p.clips) * T * d;  // one (layer, k|v) slab of the cross cache
  const size_t self_slab = size_t(p.self_rows > 0 ? p.self_rows : B) * p.self_cap * d;
  auto cache_at = [&](float* base, size_t elems) -> void* {
    return bf ? static_cast<void*>(reinterpret_cast<unsigned short*>(base) + elems) : static_cast<void*>(base + elems);
  };
  float* const x = dw.xd;  // residual stream [rows][d], updated in place by the residual GEMMs
  for (int l = 0; l < c.n_text_layer; ++l) {
    const DecBlockWeights& w = bf ? dec_blocks_bf_[l] : dec_blocks_[l];
    DecGemmArgs q;  // LN + fused q|k|v projection (+ token/positional embedding at layer 0)
    q.bf16 = bf;
    q.Wt = w.wqkv.w; q.w_scale = w.wqkv.scale; q.N = 3 * d; q.K = d; q.B = B; q.M = M;
    q.xin = x; q.ln_g = w.attn_ln_g; q.ln_b = w.attn_ln_b;
    if (l > 0 && split) {  // the previous layer's fc2 left x in two halves: sum them, block 0 completes x
      q.xin = dw.xb; q.xpart = dw.xpart; q.xout = x;
    }
    if (l == 0) {
      q.ids = p.ids; q.ids_stride = p.ids_stride; q.pos = p.pos0; q.tok_emb = tok_emb; q.pos_emb = dec_pos;
      q.n_vocab = V; q.xout = x;
      q.pos_start = p.pos_start; q.n_ctx = c.n_text_ctx;
    }
    q.bias = w.bqkv; q.Y = dw.qkvd; q.ldy = 3 * d;
    timed(tm, 0, [&] { launch_dec_gemm(q, kProLn, kDecBias, st); });
    void* const kc = cache_at(p.self_kv, (size_t(l) * 2 + 0) * self_slab);
    void* const vc = cache_at(p.self_kv, (size_t(l) * 2 + 1) * self_slab);
    timed(tm, 1, [&] {
      if (p.self_anc) {  // full-length beam search: the hypotheses share one cache through their ancestor tables
        launch_self_attention_long_gather(dw.qkvd, kc, vc, p.self_cap, p.pos0, p.self_anc, dw.attd, B, H, st, bf);
      } else if (p.pos_start && p.self_prefill) {  // the ragged chain: prompt slots, then one generated slot per pass
        launch_self_attention_prefill_ragged(dw.qkvd, kc, vc, p.self_cap, p.pos0, p.np, p.pos_start, p.pos_limit, dw.attd, B, H,
                                             st, bf);
      } else if (p.pos_start) {
        launch_self_attention_long_ragged(dw.qkvd, kc, vc, p.self_cap, p.pos0, p.pos_start, p.pos_limit, dw.attd, B, H, st, bf);
      } else if (p.self_prefill) {  // np positions of a prompt behind a context
        launch_self_attention_prefill(dw.qkvd, kc, vc, p.self_cap, p.pos0, p.np, dw.attd, B, H, st, bf);
      } else if (p.self_long) {  // one position past 32 (full-length decoding)
        launch_self_attention_long(dw.qkvd, kc, vc, p.self_cap, p.pos0, dw.attd, B, H, st, bf);
      } else {
        launch_self_attention(dw.qkvd, kc, vc, p.self_cap, p.pos0, p.np, dw.attd, B, H, st, bf);
      }
    });
    DecGemmArgs o;  // x += attn . Wo^T + bo
    o.bf16 = bf;
    o.Wt = w.wo.w; o.w_scale = w.wo.scale; o.N = d; o.K = d; o.B = B; o.M = M; o.X = dw.attd; o.ldx = d;
    o.bias = w.bo; o.R = x; o.Y = x; o.ldy = d;
    timed(tm, 2, [&] { launch_dec_gemm(o, kProNone, kDecResid, st); });

    DecGemmArgs co;  // x += (cross-attention context) . Wco^T + bco
    co.bf16 = bf;
    co.Wt = w.cross_wo.w; co.w_scale = w.cross_wo.scale; co.N = d; co.K = d; co.B = B; co.M = M;
    co.bias = w.cross_bo; co.R = x; co.Y = x; co.ldy = d;
    if (p.absorbed) {
      // Cross attention against the encoder output itself (k_cross_absorbed.hip): LN + absorbed query projection
      // q'_h = c0 Wk_h^T (Wq_h LN(x) + bq_h) for all heads in one GEMM, the matrix-core sweep of E per key chunk
      // (the M / clips query rows of a clip in groups of 16 / heads query columns), the chunk combine with the heads'
      // value projections, and the ordinary out-projection.
      DecGemmArgs qa;
      qa.bf16 = bf; qa.Wt = w.wq_abs.w; qa.w_scale = w.wq_abs.scale; qa.N = H * d; qa.K = d; qa.B = B; qa.M = M;
      qa.xin = x; qa.ln_g = w.cross_ln_g; qa.ln_b = w.cross_ln_b; qa.bias = w.bq_abs; qa.Y = dw.qp; qa.ldy = H * d;
      timed(tm, 3, [&] { launch_dec_gemm(qa, kProLn, kDecBias, st); });
      if (p.align && !p.align->layer[size_t(l)].empty()) {  // word timestamps: keep this layer's alignment heads' weights
        const AlignSink& sk = *p.align;
        AlignScoresArgs as;
        as.qp = dw.qp; as.e = p.e; as.e_plane = long(ws_.batch) * T * d; as.e_scale = cross_kv_.sc.a; as.bf16 = bf;
        as.batch = p.clips; as.H = H; as.d_model = d; as.T = T; as.np = p.np; as.pos0 = p.pos0;
        as.n_heads = int(sk.layer[size_t(l)].size());
        for (int i = 0; i < as.n_heads; ++i) as.head[i] = sk.layer[size_t(l)][size_t(i)].first, as.slot[i] = sk.layer[size_t(l)][size_t(i)].second;
        for (int b = 0; b < p.clips; ++b) as.F[b] = sk.F[b];
        as.W = sk.W; as.heads_total = sk.heads_total; as.L_max = sk.L_max; as.ldw = sk.ldw; as.mode = int(align_mode);
        launch_align_scores(as, st);
      }
      const int nq_max = cross_absorbed_max_nq(H), nq_all = M / p.clips;
      for (int p0 = 0; p0 < nq_all; p0 += nq_max) {
        CrossAbsorbedArgs ca;
        ca.qp = dw.qp; ca.e = p.e; ca.e_plane = long(ws_.batch) * T * d; ca.e_scale = cross_kv_.sc.a;
        ca.bf16 = bf; ca.split = p.e_split; ca.e2 = p.e2; ca.e3 = p.e3; ca.e4 = p.e4;
        ca.ws = dw.abs_ws; ca.batch = p.clips; ca.heads = H; ca.d_model = d; ca.T = T; ca.chunks = p.n_abs;
        ca.nq = std::min(nq_max, nq_all - p0); ca.p0 = p0;
        timed(tm, 4, [&] { launch_cross_absorbed(ca, st); });
      }
      timed(tm, 8, [&] { launch_cross_absorbed_combine(dw.abs_ws, w.cross_wv_t, w.cross_bv, dw.cabs, M, H, p.n_abs, d, st); });
      co.X = dw.cabs; co.ldx = d;
    } else {
      CrossAttnArgs ca;  // LN + query projection + attention over the cached encoder keys, per key chunk
      ca.x = x; ca.ln_g = w.cross_ln_g; ca.ln_b = w.cross_ln_b; ca.wq_t = w.cross_wq_t; ca.bq = w.cross_bq;
      ca.kc = cache_at(p.cross_kv, (size_t(l) * 2 + 0) * kv_slab); ca.vc = cache_at(p.cross_kv, (size_t(l) * 2 + 1) * kv_slab);
      ca.bf16 = bf; ca.batch = p.clips; ca.heads = H; ca.T = T; ca.chunks = p.chunks;
      // four query rows per launch (cross_attention_step's NQ); only a prompt behind a context has more positions
      for (int p0 = 0; p0 < p.np; p0 += 4) {
        ca.x = x + size_t(p0) * B * d; ca.ws = dw.cross_ws + size_t(p0) * B * H * p.chunks * 68; ca.nq = std::min(4, p.np - p0);
        timed(tm, 4, [&] { launch_cross_attention(ca, st); });
      }
      co.cross_ws = dw.cross_ws; co.heads = H; co.chunks = p.chunks;  // the out-projection's prologue combines the chunks
    }
    timed(tm, 5, [&] { launch_dec_gemm(co, p.absorbed ? kProNone : kProCombine, kDecResid, st); });

    DecGemmArgs f1;  // LN + fc1 + GELU
    f1.bf16 = bf;
    f1.Wt = w.w1.w; f1.w_scale = w.w1.scale; f1.N = 4 * d; f1.K = d; f1.B = B; f1.M = M;
    f1.xin = x; f1.ln_g = w.mlp_ln_g; f1.ln_b = w.mlp_ln_b;
    f1.bias = w.b1; f1.Y = dw.hd; f1.ldy = 4 * d;
    timed(tm, 6, [&] { launch_dec_gemm(f1, kProLn, kDecBiasGelu, st); });
    DecGemmArgs f2;  // x += h . W2^T + b2
    f2.bf16 = bf;
    f2.Wt = w.w2.w; f2.w_scale = w.w2.scale; f2.N = d; f2.K = 4 * d; f2.B = B; f2.M = M; f2.X = dw.hd; f2.ldx = 4 * d;
    f2.bias = w.b2; f2.R = x; f2.Y = x; f2.ldy = d;
    if (split) {  // x stays in two halves for the next kProLn consumer: the next layer's qkv, the logits GEMM, language_head
      f2.Y = dw.xb; f2.ksplit = 2; f2.part = dw.xpart;
    }
    timed(tm, 7, [&] { launch_dec_gemm(f2, kProNone, kDecResid, st); });
  }
  if (!p.best) return;
  // logits against the tied embedding + argmax records (whisper.cpp:379-399); only the last position's rows exist
  // here, the reference computes and drops the others
  const size_t off = size_t(p.np - 1) * B * d;
  const TiledW& emb = bf ? tok_emb_tiled_bf_ : tok_emb_tiled;
  DecGemmArgs lg;  // final LayerNorm (of x, or of the two halves a K-split fc2 left) + logits + argmax records
  lg.bf16 = bf; lg.logits_blocks = p.logits_blocks;
  lg.Wt = emb.w; lg.w_scale = emb.scale; lg.N = V; lg.K = d; lg.B = B;
  lg.xin = (split ? dw.xb : x) + off; lg.xpart = split ? dw.xpart + off : nullptr; lg.ln_g = dec_ln_g; lg.ln_b = dec_ln_b;
  lg.Y = p.Y; lg.ldy = p.ldy; lg.best = p.best;
  timed(tm, 9, [&] { launch_dec_gemm(lg, kProLn, kDecLogits, st); });
}

void Engine::decode_enqueue(int batch, int slot_idx, float* logits_host, int logits_steps_cap, int group, bool pipelined,
                            int stream_override) {
  const bool paired = group > 1;
  const int per = batch;            // clips per encoder batch
  if (group < 1 || group > 4) throw Error(kErrInvalidArg, "decoder chains take one to four batches");
  batch = group * per;              // the chain decodes them all: rows / clips below count the group
  if (batch > (paired ? kDecRowsMax : 64)) throw Error(1, "decoder batches are limited to 64 clips per call");  // before any stream operation
  for (int j = 0; paired && j < group; ++j) {
    if (!slots_[(slot_idx + j) % kSlots].absorbed || logits_host) throw Error(kErrInvalidArg, "decoder groups: the absorbed form only");
  }
  ensure_batch(batch);
  Slot& slot = slots_[slot_idx];
  // fixed slot -> stream map (few captured graphs); pair leaders are the even slots, so a pair counts as one
  // (stream_override: a spare stream + workspace for a batch decoded in the latency form, submit_decoder)
  auto dec_of = [&](int si) { return stream_override >= 0 ? stream_override : (si / group) % n_dec_streams_; };
  slot.dec = dec_of(slot_idx);
  slot.pair_leader = -1;
  hipStream_t const stream_ = dec_stream_at(slot.dec);  // everything below runs on this decoder stream
  HIPCHK(hipStreamWaitEvent(stream_, slot.enc_done, 0));
  for (int j = 1; j < group; ++j) HIPCHK(hipStreamWaitEvent(stream_, slots_[(slot_idx + j) % kSlots].enc_done, 0));
  HIPCHK(hipEventRecord(slot.dec_begin, stream_));
  long long* const h_ids_ = slot.h_ids;
  int* const h_n_ = slot.h_n;
  const wtw::Dims& c = dims_;
  const int d = c.n_text_state, V = c.n_vocab;
  // Language mode of the chain: 0 = the prompt names the language; 1 = language -1: position 0 goes through the layers
  // alone, language_head writes ids[b][1] on the device, and the rest of the prompt follows in the usual grouping;
  // 2 = detection alone (detect_language): that first pass over [sot] and the head, nothing else
  const int lang_mode = detect_only_ ? 2 : (language < 0 ? 1 : 0);
  const int n_lang = lang_mode ? lang_tokens() : 0;
  const bool cand = lang_mode && !language_candidates.empty();  // (the mask itself is device data)
  if (lang_mode) {
    if (n_lang < 1) throw Error(kErrUnsupported, "language detection: this engine's vocabulary has no language tokens");
    ensure_lang_workspace();  // (before any capture: nothing may be allocated inside one)
  }
  const std::vector<long long> prompt = lang_mode == 2 ? std::vector<long long>{vocab_.token_sot} : this->prompt();
  const int n_prompt = int(prompt.size()), stride = 32;
  check_prompt_ids(prompt, 1);
  const int max_pos = lang_mode == 2 ? 1 : int(std::min<long>(std::max<long>(max_tokens, n_prompt), 31));
  const bool forced = !forced_ids.empty() && lang_mode != 2;
  if (forced && forced_ids.size() != size_t(batch) * stride) {
    throw Error(kErrInvalidArg, "forced ids are set for another number of clips than this decode has");
  }
  for (long long id : forced_ids) {
    if (!forced) break;
    if (id < 0 || id >= V) throw Error(kErrInvalidArg, "forced token id outside the model's vocabulary");
  }
  for (int b = 0; b < batch; ++b) {
    for (int i = 0; i < stride; ++i) {
      h_ids_[size_t(b) * stride + i] = forced ? forced_ids[size_t(b) * stride + i] : (i < n_prompt ? prompt[i] : 0);
    }
    h_n_[b] = n_prompt;
  }
  const int chunks = cross_chunks_for(batch);
  const bool absorbed = slot.absorbed;  // the form this slot's encoder pass prepared (the same for every slot of a graph set)
  const int n_abs = abs_chunks_for(batch, pipelined ? (bf16 ? 64 : 128) : 256);
  int steps = 0;
  static const bool dec_timers = getenv("WT_DEC_KERNEL_TIMERS") != nullptr;
  auto enqueue_all = [&](int si, DecTimers* tm) {
    Slot& slot = slots_[si];
    const Slot* const member[4] = {&slot, &slots_[(si + 1) % kSlots], &slots_[(si + 2) % kSlots], &slots_[(si + 3) % kSlots]};  // the group's batches
    DecWorkspace& dw = dws_[dec_of(si)];
    hipStream_t const stream_ = dec_stream_at(dec_of(si));
    long long* const h_ids_ = slot.h_ids;
    int* const h_n_ = slot.h_n;
    steps = 0;
    HIPCHK(hipMemcpyAsync(dw.ids, h_ids_, size_t(batch) * stride * sizeof(long long), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipMemcpyAsync(dw.n_ids, h_n_, size_t(batch) * sizeof(int), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipMemsetAsync(dw.finished, 0, size_t(batch) * sizeof(int), stream_));

    DecPass p;  // what stays the same over the chain's passes
    p.B = p.clips = batch; p.ids = dw.ids; p.ids_stride = stride; p.self_kv = dw.self_kv; p.self_cap = self_cap_;
    p.absorbed = absorbed; p.n_abs = n_abs; p.chunks = chunks; p.e = slot.e_planes; p.cross_kv = slot.cross_kv;
    if (paired) {
      p.e_split = per;
      p.e2 = member[1]->e_planes;
      if (group > 2) p.e3 = member[2]->e_planes;
      if (group > 3) p.e4 = member[3]->e_planes;
    }
    p.bf = bf16 != 0; p.split = fc2_split(); p.dw = &dw; p.timers = tm;
    p.ldy = V; p.logits_blocks = pipelined ? 256 : 0;
    // Passes.  The prompt positions of every clip go through the layers TOGETHER when they fit one pass (rows =
    // positions x clips <= 128, at most 4 positions: causal self-attention inside the pass, one sweep of the
    // cross-KV cache for all of them); the reference feeds the same prefix to its graph at once, whisper.cpp:367-375.
    // Every later position is one pass of `batch` rows.
    // (a pair's 64 clips, or a 64-clip batch: the four prompt positions go two and two — 28 passes instead of 30)
    const int np_max = std::max(1, std::min(4, kDecRowsMax / batch));
    const int prompt_end = std::min(n_prompt, max_pos);
    for (int pos0 = 0, np = 1; pos0 < max_pos; pos0 += np) {
      np = pos0 < prompt_end ? std::min(np_max, prompt_end - pos0) : 1;
      if (lang_mode && pos0 == 0) np = 1;  // the language is read off position 0 before position 1 can be embedded
      const int last = pos0 + np - 1;
      const bool logits = last >= n_prompt - 1 && lang_mode != 2;  // then greedy argmax (whisper.cpp:379-399)
      p.pos0 = pos0; p.np = np; p.best = logits ? dw.best : nullptr; p.Y = logits_host ? dw.logits : nullptr;
      decoder_pass(p, stream_);
      if (lang_mode && pos0 == 0) {
        // position 0's residual rows -> language probabilities and ids[b][1]; no logits GEMM at this position
        LangWorkspace& lw = lw_[dec_of(si)];
        if (cand) {  // a candidate list: language_head_rows under its mask
          LanguageRowsArgs la;
          la.x = p.split ? dw.xb : dw.xd; la.xpart = p.split ? dw.xpart : nullptr; la.ln_g = dec_ln_g; la.ln_b = dec_ln_b;
          la.tok_emb = tok_emb; la.clips = la.x_rows = batch; la.d = d; la.n_vocab = V; la.lang_lo = int(kLangLo); la.n_lang = n_lang;
          la.allow = d_lang_allow_; la.probs = lw.probs; la.lang = lw.lang; la.lang_prob = lw.prob;
          if (lang_mode == 1) la.ids[0] = dw.ids, la.ids_rows[0] = batch, la.ids_stride[0] = stride, la.id_pos = 1, la.fan = 1;
          timed(tm, 10, [&] { launch_language_head_rows(la, stream_); });
        } else {
          LanguageHeadArgs la;
          la.x = p.split ? dw.xb : dw.xd; la.xpart = p.split ? dw.xpart : nullptr; la.ln_g = dec_ln_g; la.ln_b = dec_ln_b;
          la.tok_emb = tok_emb; la.rows = batch; la.d = d; la.n_vocab = V; la.lang_lo = int(kLangLo); la.n_lang = n_lang;
          la.probs = lw.probs; la.lang = lw.lang; la.lang_prob = lw.prob;
          if (lang_mode == 1) la.ids = dw.ids, la.ids_stride = stride, la.id_pos = 1;
          timed(tm, 10, [&] { launch_language_head(la, stream_); });
        }
        if (!pipelined) {  // a synchronous call reads them after decode_collect (pipelined callers read ids[b][1])
          HIPCHK(hipMemcpyAsync(h_lang_, lw.lang, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, stream_));
          HIPCHK(hipMemcpyAsync(h_lang_prob_, lw.prob, size_t(batch) * sizeof(float), hipMemcpyDeviceToHost, stream_));
          if (lang_mode == 2) {
            HIPCHK(hipMemcpyAsync(h_lang_probs_, lw.probs, size_t(batch) * n_lang * sizeof(float), hipMemcpyDeviceToHost, stream_));
          }
        }
      }
      if (logits) {
        if (logits_host && steps < logits_steps_cap) {
          HIPCHK(hipMemcpy2DAsync(logits_host + size_t(steps) * V, size_t(logits_steps_cap) * V * sizeof(float),
                                  dw.logits, size_t(V) * sizeof(float), size_t(V) * sizeof(float), batch,
                                  hipMemcpyDeviceToHost, stream_));
        }
        timed(tm, 10, [&] { launch_select_token(dw.best, (V + 31) / 32, dw.ids, stride, last, dw.n_ids, dw.finished,
                                                vocab_.token_eot, int(stop_at_eot), batch, stream_, forced); });
        ++steps;
      }
    }
    // Every slot receives its OWN clips' ids in its own pinned buffers: a pair's second batch used to be read out of
    // the leader's buffers, which the leader's next submit (collected first, reused first) could overwrite.
    for (int j = 0; j < group; ++j) {
      HIPCHK(hipMemcpyAsync(member[j]->h_ids, dw.ids + size_t(j) * per * stride, size_t(per) * stride * sizeof(long long),
                            hipMemcpyDeviceToHost, stream_));
      HIPCHK(hipMemcpyAsync(member[j]->h_n, dw.n_ids + size_t(j) * per, size_t(per) * sizeof(int), hipMemcpyDeviceToHost, stream_));
    }
  };
  // The ~1050 launches of a decode are identical from call to call for a given (slot, batch,
  // options). The first call with a signature runs them eagerly (which also performs the
  // kernels' one-time attribute set-up) and then captures one hipGraph per slot; later calls
  // replay the slot's graph: one host call instead of ~1100. The logits tap stays eager.
  auto key_of = [&](int si) {
    return std::vector<long long>{si, batch, max_pos, n_prompt, chunks, long(stop_at_eot), fc2_ksplit, bf16, absorbed ? 1 : 0, n_abs, group, stream_override, forced ? 1 : 0, pipelined ? 1 : 0, lang_mode + (cand ? 2 : 0)};
  };
  // the cached form's graphs are captured for EVERY slot at once (below) and hold each slot's cache pointer: all of
  // them must exist before the capture (need_cross_kv allocates; nothing may be allocated inside a capture)
  if (!absorbed && use_graphs && !logits_host) {
    for (Slot& s : slots_) need_cross_kv(s);
  }
  hipGraphExec_t exec = nullptr;
  if (use_graphs && !logits_host) {
    auto it = graphs_.find(key_of(slot_idx));
    if (it != graphs_.end()) {
      exec = it->second.exec;
      steps = it->second.steps;
    }
  }
  if (exec) {
    HIPCHK(hipGraphLaunch(exec, stream_));
  } else {
    DecTimers timers{slot.dt_events, slot.dt_cls, stream_};
    slot.dt_cls.clear();
    enqueue_all(slot_idx, dec_timers && !logits_host ? &timers : nullptr);
    const int eager_steps = steps;
    // the eager work of THIS batch is queued: its completion event and step count are set before anything that can
    // fail, so that submit() / collect() stay consistent whatever happens to the captures below
    HIPCHK(hipEventRecord(slot.dec_done, stream_));
    slot.steps = eager_steps;
    for (int j = 1; j < group; ++j) {
      Slot& sb = slots_[(slot_idx + j) % kSlots];
      HIPCHK(hipEventRecord(sb.dec_done, stream_));
      sb.pair_leader = slot_idx, sb.steps = eager_steps, sb.dec = slot.dec;
    }
    if (use_graphs && !logits_host) {
      // A capture or instantiation failure is not fatal: the decoder keeps launching eagerly (same kernels, same
      // results, more host time per batch) and the engine stops trying.
      std::map<std::vector<long long>, GraphEntry> fresh;
      try {
        for (int si = 0; si < kSlots; ++si) {
          hipGraphExec_t const ge = capture_graph(dec_stream_at(dec_of(si)), [&] { enqueue_all(si, nullptr); });
          fresh[key_of(si)] = GraphEntry{ge, steps};  // (steps: as enqueue_all has just counted them)
        }
        for (auto& g : fresh) graphs_[g.first] = g.second;  // all slots or none
      } catch (const std::exception& e) {
        for (auto& g : fresh) (void)hipGraphExecDestroy(g.second.exec);
        (void)hipGetLastError();
        use_graphs = 0;
        std::fprintf(stderr, "[wt] decoder hipGraph capture failed (%s): continuing with eager launches\n", e.what());
      }
    }
    steps = eager_steps;
    return;
  }
  HIPCHK(hipEventRecord(slot.dec_done, stream_));
  slot.steps = steps;
  for (int j = 1; j < group; ++j) {
    Slot& sb = slots_[(slot_idx + j) % kSlots];
    HIPCHK(hipEventRecord(sb.dec_done, stream_));
    sb.pair_leader = slot_idx, sb.steps = steps, sb.dec = slot.dec;
  }
}

void Engine::debug_concurrency(const float* d_mel, int batch, int n_dec, int n_enc, float* dec_ms,
                               float* enc_ms) {
  if (!inflight_.empty()) throw Error(1, "collect the submitted batches first");
  if (n_dec < 0 || n_dec > 4 || n_enc < 0 || n_enc > 4) throw Error(1, "debug_concurrency: 0..4 decodes, 0..4 encoder passes");
  ensure_batch(batch);
  sync();
  for (int i = 0; i < n_dec; ++i)
    if (!slots_[i].used) throw Error(1, "debug_concurrency: run a batch per slot first so every slot holds a cross-KV cache");
  select_stream(true);
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  for (int i = 0; i < n_dec; ++i) decode_enqueue(batch, i, nullptr, 0);
  HIPCHK(hipEventRecord(e0, stream_));
  for (int i = 0; i < n_enc; ++i) {
    if (enc_slot_ < 4) enc_slot_ = 4;  // encoder passes alternate over slots 4 and 5, away from the decoders' caches
    encode_enqueue(d_mel, batch);
  }
  HIPCHK(hipEventRecord(e1, stream_));
  sync();
  for (int i = 0; i < n_dec; ++i) HIPCHK(hipEventElapsedTime(&dec_ms[i], slots_[i].dec_begin, slots_[i].dec_done));
  HIPCHK(hipEventElapsedTime(enc_ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
}

void Engine::decode_collect(int slot_idx, int64_t* ids, int32_t* n_ids) {
  finish_slot(slot_idx);
  const Slot& slot = slots_[slot_idx];
  const int batch = slot.batch, stride = 32;
  for (int b = 0; b < batch; ++b) {
    n_ids[b] = slot.h_n[b];
    for (int i = 0; i < stride; ++i)
      ids[size_t(b) * stride + i] = i < slot.h_n[b] ? slot.h_ids[size_t(b) * stride + i] : 0;
  }
}

// waits for the slot's decoder chain; the encoder's non-finite flag, kernel statistics and timings of the batch
void Engine::finish_slot(int slot_idx) {
  Slot& slot = slots_[slot_idx];
  HIPCHK(hipEventSynchronize(slot.dec_done));
  HIPCHK(hipGetLastError());
  if (*slot.h_flag != 0) {
    *slot.h_flag = 0;
    throw Error(5, "non-finite encoder output: an operand left the fp16 range of the default contraction kernels "
                   "(|activation| > 65504 or |weight| > 1023) or the input holds NaN/Inf; gemm_variant 16 and "
                   "attn_variant 1 (bf16 three-plane split) have the full fp32 range");
  }
  const int batch = slot.batch;
  // (a batch decoded by its pair leader's chain has its ids in its OWN buffers; the leader only times the chain)
  const Slot& src = slot.pair_leader >= 0 ? slots_[slot.pair_leader] : slot;
  resolve_kernel_stats(slot_idx);
  float ms = 0;
  timings_.batch = batch;
  timings_.decoder_steps = slot.steps;
  if (hipEventElapsedTime(&ms, slot.enc_begin, slot.enc_mid) == hipSuccess) timings_.encoder_ms = ms;
  if (hipEventElapsedTime(&ms, slot.enc_mid, slot.enc_done) == hipSuccess) timings_.cross_kv_ms = ms;
  if (hipEventElapsedTime(&ms, src.dec_begin, slot.dec_done) == hipSuccess) timings_.decoder_ms = ms;
  if (hipEventElapsedTime(&ms, slot.enc_begin, slot.dec_done) == hipSuccess) timings_.total_ms = ms;
  if (!slot.dt_cls.empty()) {
    static const char* kNames[11] = {"qkv(LN)", "self_attn", "o_proj", "q_abs(LN)", "cross_attn", "co",
                                     "fc1(LN)", "fc2", "abs_combine", "logits", "select"};
    double tot[11] = {0};
    int cnt[11] = {0};
    for (size_t i = 0; i < slot.dt_cls.size(); ++i) {
      float ms_k = 0;
      if (hipEventElapsedTime(&ms_k, slot.dt_events[2 * i], slot.dt_events[2 * i + 1]) == hipSuccess) {
        tot[slot.dt_cls[i]] += ms_k;
        cnt[slot.dt_cls[i]] += 1;
      }
    }
    fprintf(stderr, "[wt-dec-timers] slot %d:", slot_idx);
    for (int c = 0; c < 11; ++c)
      if (cnt[c]) fprintf(stderr, " %s %.2f ms (%d x %.1f us)", kNames[c], tot[c], cnt[c], 1e3 * tot[c] / cnt[c]);
    fprintf(stderr, "\n");
    slot.dt_cls.clear();
  }
  static const bool trace = getenv("WT_TRACE_PIPELINE") != nullptr;
  if (trace) {  // device timeline of the batch relative to the first traced batch, for pipeline analysis
    hipEvent_t base = trace_base_;
    float t[4] = {0, 0, 0, 0};
    hipEvent_t evs[4] = {slot.enc_begin, slot.enc_done, src.dec_begin, slot.dec_done};  // a paired batch: its leader's chain
    for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&t[i], base, evs[i]);
    (void)hipGetLastError();
    fprintf(stderr, "[wt-trace] slot %d enc %.3f..%.3f dec %.3f..%.3f\n", slot_idx, t[0], t[1], t[2], t[3]);
  }
  if (timings_.logmel_ms < 0) {
    timings_.logmel_ms = 0;
    if (hipEventElapsedTime(&ms, ev_[0], ev_[1]) == hipSuccess) timings_.logmel_ms = ms;
  }
}

// -------------------------------------------------------- beam search ---

void Engine::check_beam_call(bool logits_tap, bool allow_bf16) const {
  if (beam_size <= 1) return;
  auto no = [](const char* why) { throw Error(kErrUnsupported, std::string("beam search: ") + why); };
  if (bf16 && !allow_bf16) no("not in the bf16 storage mode");
  if (!cross_absorb) no("needs the absorbed cross-attention (cross_absorb = 1)");
  if (!absorb_active()) no("the absorbed cross-attention is not available with these weights or this gemm_variant");
  if (!stop_at_eot) no("needs stop_at_eot = 1");
  if (!forced_ids.empty()) no("not with forced ids");
  if (logits_tap) no("no logits tap");
  if (dims_.n_vocab > kBeamChunk * kBeamMaxChunks) no("vocabularies of at most 65536 entries");
}

void Engine::ensure_beam_workspace() {
  if (bw_.h_len) return;  // (allocated last)
  const wtw::Dims& c = dims_;
  const size_t R = kDecRowsMax, d = c.n_text_state, V = c.n_vocab, C = kBeamClipsMax, S = kBeamMax;
  for (int i = 0; i < 2; ++i) {
    bw_.kv[i] = dev_zeroed<float>(size_t(c.n_text_layer) * 2 * R * self_cap_ * d);
    bw_.ids[i] = dev_zeroed<long long>(R * 32);
  }
  bw_.logits = dev_zeroed<float>(R * V);
  bw_.best = dev_zeroed<unsigned long long>(R * ((V + 31) / 32));
  bw_.part = dev_zeroed<BeamPart>(R * beam_chunks(int(V)));
  bw_.parent = dev_zeroed<int>(R);
  bw_.token = dev_zeroed<long long>(R);
  bw_.live_sum = dev_zeroed<float>(C * S);
  bw_.fin_sum = dev_zeroed<float>(C * S);
  bw_.fin_len = dev_zeroed<int>(C * S);
  bw_.fin_tok = dev_zeroed<int>(C * S * 32);
  bw_.n_fin = dev_zeroed<int>(C);
  bw_.done = dev_zeroed<int>(C);
  bw_.out_ids = dev_zeroed<long long>(C * 32);
  bw_.out_n = dev_zeroed<int>(C);
  bw_.out_sum = dev_zeroed<float>(C);
  bw_.out_len = dev_zeroed<int>(C);
  bw_.h_prompt = pinned<long long>(C * 32);
  bw_.h_sum = pinned<float>(C);
  bw_.h_len = pinned<int>(C);
}

// Beam search.  A chain decodes nc <= 128 / K clips: the prompt passes over nc rows as greedy runs
// them, then per step the K live hypotheses of every clip as K * nc rows, row = k * nc + c — one position per pass, so
// every per-row kernel sees K * nc independent sequences, and the absorbed cross-attention sees nc clips with K query
// rows each (its position loop).  Between the logits GEMM and the next pass: top-k, select, reorder (k_beam.hip).
// Chains of one call run one after the other on the slot's decoder stream, each reading the encoder planes at its clip
// offset.  Like greedy's, a chain's launch sequence is fixed for its key and replayed from a hipGraph.
void Engine::decode_beam(int batch, int slot_idx, int64_t* ids, int32_t* n_ids) {
  const int K = int(beam_size);
  if (batch < 1 || batch > kBeamClipsMax) throw Error(kErrInvalidArg, "decoder batches are limited to 64 clips per call");
  Slot& slot = slots_[slot_idx];
  if (!slot.absorbed) throw Error(kErrUnsupported, "beam search: the encoder pass did not prepare the absorbed cross-attention");
  ensure_beam_workspace();
  const wtw::Dims& c = dims_;
  const int d = c.n_text_state, T = c.n_audio_ctx, V = c.n_vocab, L = c.n_text_layer;
  const std::vector<long long> prompt = this->prompt();
  const int n_prompt = int(prompt.size()), stride = 32;
  check_prompt_ids(prompt, 1);
  const int max_pos = int(std::min<long>(std::max<long>(max_tokens, n_prompt), 31));
  const int n_steps = max_pos - n_prompt + 1;  // the positions at which greedy takes an argmax
  const int per_chain = kDecRowsMax / K;
  slot.dec = slot_idx % n_dec_streams_;
  slot.pair_leader = -1;
  DecWorkspace& dw = dws_[slot.dec];
  hipStream_t const st = dec_stream_at(slot.dec);
  for (int b = 0; b < kBeamClipsMax; ++b) {
    for (int i = 0; i < stride; ++i) bw_.h_prompt[size_t(b) * stride + i] = i < n_prompt ? prompt[i] : 0;
  }
  HIPCHK(hipStreamWaitEvent(st, slot.enc_done, 0));
  HIPCHK(hipEventRecord(slot.dec_begin, st));

  auto enqueue_chain = [&](int c0, int nc) {
    const int rows = K * nc;
    HIPCHK(hipMemcpyAsync(bw_.ids[0], bw_.h_prompt, size_t(nc) * stride * sizeof(long long), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(bw_.n_fin + c0, 0, size_t(nc) * sizeof(int), st));
    HIPCHK(hipMemsetAsync(bw_.done + c0, 0, size_t(nc) * sizeof(int), st));
    DecPass p;
    p.clips = nc; p.ids_stride = stride; p.self_cap = self_cap_; p.absorbed = true; p.n_abs = abs_chunks_for(nc, 256);
    p.e = slot.e_planes + size_t(c0) * T * d; p.split = fc2_split(); p.dw = &dw; p.Y = bw_.logits; p.ldy = V;
    // one decoder pass: np positions from pos0 of `seqs` sequences (rows p * seqs + s, caches of seqs rows); the
    // cross-attention sees the nc clips with np * seqs / nc query rows each (row = q * nc + clip).  logits: the last
    // position's rows, written out for the top-k pass
    auto pass = [&](int pos0, int np, int seqs, const long long* idsb, float* kv, bool logits) {
      p.pos0 = pos0; p.np = np; p.B = seqs; p.ids = idsb; p.self_kv = kv; p.best = logits ? bw_.best : nullptr;
      decoder_pass(p, st);
    };
    const int np_max = std::max(1, std::min(4, kDecRowsMax / nc));
    for (int pos0 = 0, np = 1; pos0 < n_prompt; pos0 += np) {
      np = std::min(np_max, n_prompt - pos0);
      pass(pos0, np, nc, bw_.ids[0], bw_.kv[0], pos0 + np == n_prompt);
    }
    int cur = 0;
    for (int t = 0; t < n_steps; ++t) {
      const int pos = n_prompt - 1 + t, live_rows = t == 0 ? nc : rows;
      const bool more = t + 1 < n_steps;
      launch_beam_topk(bw_.logits, V, V, live_rows, K + 1, bw_.part, st);
      BeamStepArgs sa;
      sa.part = bw_.part; sa.n_chunks = beam_chunks(V); sa.ids = bw_.ids[cur];
      sa.clips = nc; sa.K = K; sa.n_live = t == 0 ? 1 : K; sa.pos = pos; sa.n_prompt = n_prompt; sa.V = V; sa.c0 = c0;
      sa.eot = vocab_.token_eot;
      sa.live_sum = bw_.live_sum; sa.fin_tok = bw_.fin_tok; sa.fin_sum = bw_.fin_sum; sa.fin_len = bw_.fin_len;
      sa.n_fin = bw_.n_fin; sa.done = bw_.done; sa.parent = bw_.parent; sa.token = bw_.token;
      launch_beam_select(sa, st);
      BeamReorderArgs ra;  // (after the last step only the id rows: finalize reads the live hypotheses from them)
      ra.kv_src = bw_.kv[cur]; ra.kv_dst = bw_.kv[cur ^ 1]; ra.src_rows = live_rows; ra.dst_rows = rows; ra.cap = self_cap_;
      ra.d = d; ra.slabs = more ? 2 * L : 0; ra.pos = pos; ra.V = V;
      ra.ids_src = bw_.ids[cur]; ra.ids_dst = bw_.ids[cur ^ 1]; ra.parent = bw_.parent; ra.token = bw_.token;
      launch_beam_reorder(ra, st);
      cur ^= 1;
      if (more) pass(pos + 1, 1, rows, bw_.ids[cur], bw_.kv[cur], true);
    }
    BeamFinalArgs fa;
    fa.ids = bw_.ids[cur]; fa.clips = nc; fa.K = K; fa.c0 = c0; fa.pos = max_pos - 1; fa.n_prompt = n_prompt;
    fa.live_sum = bw_.live_sum; fa.fin_tok = bw_.fin_tok; fa.fin_sum = bw_.fin_sum; fa.fin_len = bw_.fin_len;
    fa.n_fin = bw_.n_fin; fa.done = bw_.done;
    fa.out_ids = bw_.out_ids; fa.out_n = bw_.out_n; fa.out_sum = bw_.out_sum; fa.out_len = bw_.out_len;
    launch_beam_finalize(fa, st);
  };

  for (int c0 = 0; c0 < batch; c0 += per_chain) {
    const int nc = std::min(per_chain, batch - c0);
    // (greedy's keys have 14 entries and start with the slot; a beam key starts with -beam_size)
    const std::vector<long long> key{-K, slot_idx, c0, nc, max_pos, n_prompt, abs_chunks, fc2_ksplit, slot.dec};
    replay_or_capture(key, st, use_graphs != 0, "beam-search", [&] {
      enqueue_chain(c0, nc);
      return n_steps;
    });
  }
  HIPCHK(hipMemcpyAsync(slot.h_ids, bw_.out_ids, size_t(batch) * stride * sizeof(long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(slot.h_n, bw_.out_n, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(bw_.h_sum, bw_.out_sum, size_t(batch) * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(bw_.h_len, bw_.out_len, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(slot.dec_done, st));
  slot.steps = n_steps;
  decode_collect(slot_idx, ids, n_ids);  // waits; the encoder's non-finite flag, timings
  last.beam_sum.assign(bw_.h_sum, bw_.h_sum + batch);
  last.beam_len.assign(bw_.h_len, bw_.h_len + batch);
  last.beam_valid = true;
}

}  // namespace wt
