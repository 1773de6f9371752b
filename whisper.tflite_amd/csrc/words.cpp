// Word-level timestamps, the host side (words.h).
#include "words.h"

#include <algorithm>
#include <limits>
#include <string>

namespace wt {

std::vector<uint32_t> decode_utf8_replace(const unsigned char* s, size_t n) {
  std::vector<uint32_t> out;
  out.reserve(n);
  size_t i = 0;
  while (i < n) {
    const unsigned b0 = s[i];
    if (b0 < 0x80) {
      out.push_back(b0);
      ++i;
      continue;
    }
    int need = 0;
    unsigned lo = 0x80, hi = 0xBF;  // the range of the SECOND byte; later ones are 80 .. BF
    uint32_t cp = 0;
    if (b0 >= 0xC2 && b0 <= 0xDF) {
      need = 1, cp = b0 & 0x1F;
    } else if (b0 >= 0xE0 && b0 <= 0xEF) {
      need = 2, cp = b0 & 0x0F;
      if (b0 == 0xE0) lo = 0xA0;
      if (b0 == 0xED) hi = 0x9F;
    } else if (b0 >= 0xF0 && b0 <= 0xF4) {
      need = 3, cp = b0 & 0x07;
      if (b0 == 0xF0) lo = 0x90;
      if (b0 == 0xF4) hi = 0x8F;
    }
    size_t k = 1;  // bytes of the sequence accepted so far
    bool ok = need > 0;
    for (int c = 0; ok && c < need; ++c) {
      if (i + k >= n || s[i + k] < lo || s[i + k] > hi) {
        ok = false;
        break;
      }
      cp = (cp << 6) | (s[i + k] & 0x3F);
      ++k, lo = 0x80, hi = 0xBF;
    }
    out.push_back(ok ? cp : 0xFFFDu);
    i += k;  // an ill-formed sequence consumes its maximal well-formed prefix (at least the lead byte)
  }
  return out;
}

namespace {

constexpr uint32_t kReplacement = 0xFFFD;

const std::string& token_bytes(const VocabData& vocab, int64_t id) {
  static const std::string none;
  auto it = vocab.id_to_token.find(static_cast<int>(id));
  return it == vocab.id_to_token.end() ? none : it->second;
}

std::vector<uint32_t> decode_replace(const std::string& s) {
  return decode_utf8_replace(reinterpret_cast<const unsigned char*>(s.data()), s.size());
}

bool is_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

std::string strip(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && is_space(s[a])) ++a;
  while (b > a && is_space(s[b - 1])) --b;
  return s.substr(a, b - a);
}

bool is_ascii_punct(char c) { return (c >= 33 && c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || (c >= 123 && c <= 126); }

bool one_of(const std::string& s, const char* const* set, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (s == set[i]) return true;
  return false;
}

// Whisper's defaults of prepend_punctuations and append_punctuations
const char* const kPrepend[] = {"\"", "'", "\xE2\x80\x9C", "\xC2\xBF", "(", "[", "{", "-"};
const char* const kAppend[] = {"\"", "'", ".", "\xE3\x80\x82", ",", "\xEF\xBC\x8C", "!", "\xEF\xBC\x81", "?", "\xEF\xBC\x9F",
                               ":", "\xEF\xBC\x9A", "\xE2\x80\x9D", ")", "]", "}", "\xE3\x80\x81"};

}  // namespace

std::vector<int> split_unicode(const VocabData& vocab, const int64_t* ids, int n) {
  std::string whole;
  for (int i = 0; i < n; ++i) whole += token_bytes(vocab, ids[i]);
  const std::vector<uint32_t> full = decode_replace(whole);
  std::vector<int> groups;
  std::string cur;
  int count = 0;
  size_t offset = 0;  // code points of the groups closed so far
  for (int i = 0; i < n; ++i) {
    cur += token_bytes(vocab, ids[i]);
    ++count;
    const std::vector<uint32_t> dec = decode_replace(cur);
    const size_t at = size_t(std::find(dec.begin(), dec.end(), kReplacement) - dec.begin());
    if (at == dec.size() || (offset + at < full.size() && full[offset + at] == kReplacement)) {
      groups.push_back(count);
      offset += dec.size();
      cur.clear();
      count = 0;
    }
  }
  if (count) groups.push_back(count);
  return groups;
}

std::vector<int> split_words(const VocabData& vocab, const int64_t* ids, int n, bool unicode_only) {
  const std::vector<int> groups = split_unicode(vocab, ids, n);
  if (unicode_only) return groups;
  std::vector<int> words;
  int at = 0;
  for (int len : groups) {
    std::string text;
    for (int k = 0; k < len; ++k) text += token_bytes(vocab, ids[at + k]);
    const std::string core = strip(text);
    const bool special = ids[at] >= vocab.token_eot;
    const bool with_space = !text.empty() && text[0] == ' ';
    const bool punctuation = core.size() == 1 && is_ascii_punct(core[0]);
    if (special || with_space || punctuation || words.empty()) {
      words.push_back(len);
    } else {
      words.back() += len;
    }
    at += len;
  }
  return words;
}

std::vector<int> merge_punctuation(const VocabData& vocab, const int64_t* ids, int n, const int* word_len, int n_words) {
  struct Word {
    std::string text;
    int count;
  };
  std::vector<Word> w;
  w.reserve(size_t(n_words));
  int at = 0;
  for (int k = 0; k < n_words; ++k) {
    Word x{std::string(), word_len[k]};
    for (int i = 0; i < word_len[k] && at + i < n; ++i) x.text += token_bytes(vocab, ids[at + i]);
    at += word_len[k];
    w.push_back(std::move(x));
  }
  // the marks that lead a word, from the back: a run of them ends up in front of the same word
  for (int i = n_words - 2, j = n_words - 1; i >= 0; --i) {
    Word &prev = w[size_t(i)], &next = w[size_t(j)];
    if (!prev.text.empty() && prev.text[0] == ' ' && one_of(strip(prev.text), kPrepend, sizeof(kPrepend) / sizeof(*kPrepend))) {
      next.text = prev.text + next.text, next.count += prev.count;
      prev.text.clear(), prev.count = 0;
    } else {
      j = i;
    }
  }
  // the marks that trail a word, from the front
  for (int i = 0, j = 1; j < n_words; ++j) {
    Word &prev = w[size_t(i)], &next = w[size_t(j)];
    const bool ends_in_space = !prev.text.empty() && prev.text.back() == ' ';
    if (!ends_in_space && one_of(next.text, kAppend, sizeof(kAppend) / sizeof(*kAppend))) {
      prev.text += next.text, prev.count += next.count;
      next.text.clear(), next.count = 0;
    } else {
      i = j;
    }
  }
  std::vector<int> out;
  for (const Word& x : w)
    if (x.count) out.push_back(x.count);
  return out;
}

int dtw_path(const float* cost, int N, int F, long ld, int32_t* jump, std::vector<int32_t>* path, unsigned char* trace_out) {
  const float inf = std::numeric_limits<float>::infinity();
  const size_t W = size_t(F) + 1;
  std::vector<float> D((size_t(N) + 1) * W, inf);
  std::vector<unsigned char> trace((size_t(N) + 1) * W, 2);
  D[0] = 0.0f;
  for (int i = 1; i <= N; ++i) {
    trace[size_t(i) * W] = 1;
    for (int j = 1; j <= F; ++j) {
      const float c0 = D[size_t(i - 1) * W + size_t(j - 1)], c1 = D[size_t(i - 1) * W + size_t(j)], c2 = D[size_t(i) * W + size_t(j - 1)];
      // the code is 2 on c0 == c1 < c2 as well, where c2 is not the minimum: the cost is the minimum's all the same
      const unsigned char t = (c0 < c1 && c0 < c2) ? 0 : (c1 < c0 && c1 < c2) ? 1 : 2;
      D[size_t(i) * W + size_t(j)] = cost[size_t(i - 1) * size_t(ld) + size_t(j - 1)] + std::min(std::min(c0, c1), c2);
      trace[size_t(i) * W + size_t(j)] = t;
      if (trace_out) trace_out[size_t(i - 1) * size_t(F) + size_t(j - 1)] = t;
    }
  }
  std::vector<int32_t> back;
  int i = N, j = F;
  while (i > 0 || j > 0) {
    if (i > 0 && j > 0) back.push_back(i - 1), back.push_back(j - 1);  // a border cell (costs that are not finite) is no cell of cost
    const unsigned char t = trace[size_t(i) * W + size_t(j)];
    if (t == 0) {
      --i, --j;
    } else if (t == 1) {
      --i;
    } else {
      --j;
    }
  }
  const int cells = int(back.size() / 2);
  for (int r = 0; r < N; ++r) jump[r] = 0;
  for (int k = 0; k < cells; ++k) jump[back[size_t(2 * k)]] = back[size_t(2 * k + 1)];  // walking back: the last write is the first frame
  if (path) {
    path->resize(back.size());
    for (int k = 0; k < cells; ++k) {
      (*path)[size_t(2 * k)] = back[size_t(2 * (cells - 1 - k))];
      (*path)[size_t(2 * k + 1)] = back[size_t(2 * (cells - 1 - k) + 1)];
    }
  }
  return cells;
}

}  // namespace wt
