// encdec — same command line as the reference's app/encdec.cpp:30-36:
//   encdec --model-prefix P --vocab V --input WAV
// prints the transcript followed by '\n' as the last line of stdout (with --lang auto, a line
// "language: <code> (p=...)" per 30 s window before it; with --max-positions per file).  The reference pulls
// in the 11 kLoC CLI11 header for three required options; a minimal parser keeps the same
// flags (and --flag=value spelling) and exit status on a usage error.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>

#include <vector>

#include "whisper.tflite/whisper.h"
#include "wt_capi.h"

namespace {
void usage(const char* argv0) {
  std::cerr << "Usage: " << argv0 << " --model-prefix <prefix> --vocab <vocab.bin> --input <wav>\n"
            << "  --model-prefix  Model prefix (loads <prefix>.wtw)   REQUIRED\n"
            << "  --vocab         Path to vocabulary                 REQUIRED\n"
            << "  --input         Path to the 16 kHz mono WAV        REQUIRED\n"
            << "  --lang          language code of the prompt (default de, as the reference hard-codes), or auto:\n"
            << "                  detected per 30 s window, printed as \"language: <code> (p=...)\" before the transcript\n"
            << "                  with --max-positions: detected once per file, on its first window (option full_language)\n"
            << "  --languages en,de,fr  the candidates --lang auto and every other detection choose among\n"
            << "  --task translate|transcribe  the task token of the prompt (default transcribe)\n"
            << "  --english       English-only vocabulary ids (multilingual = false; the reference hard-codes true)\n"
            << "  --long          transcribe every 30 s window of the file, not only the first\n"
            << "  --beam N        beam search with N hypotheses, 2..8 (default: greedy, as the reference)\n"
            << "                  with --max-positions: full-length beam search, with or without --timestamps and --scores\n"
            << "  --bf16          the bf16 storage mode (option bf16): bf16 weights, activations and caches, fp32 accumulation\n"
            << "                  with --max-positions: full-length decoding in that mode (option full_bf16)\n"
            << "                  with --max-positions and --inputs a,b --long, --lang auto or --word-timestamps: these too\n"
            << "                  (option full_bf16_all)\n"
            << "  --max-positions N  full-length greedy decoding over N positions, 32 .. n_text_ctx (default: the\n"
            << "                  reference's 31 positions)\n"
            << "  --timestamps    with --max-positions: decode with timestamps and print one line per segment,\n"
            << "                  [mm:ss.mmm --> mm:ss.mmm] text\n"
            << "  --scores        with --max-positions: print avg_logprob and no_speech_prob of every 30 s window (with\n"
            << "                  --timestamps also each segment's mean log-probability on its line)\n"
            << "  --skip-silence  with --scores: windows Whisper's no-speech rule calls silent yield no text\n"
            << "  --temperature T with --max-positions: sample every id at temperature T in [0, 1] (default 0: greedy)\n"
            << "  --best-of N     with --temperature or --fallback: N samples, 1..8, per window at every temperature above 0,\n"
            << "                  the one with the best average log-probability kept (default 1)\n"
            << "  --seed N        the sampler's 64-bit seed (default 0): same audio, options and seed, same text\n"
            << "  --fallback      with --scores: Whisper's temperature fall-back, T, T + 0.2, ... 1.0 per window, and one\n"
            << "                  line per window with the temperature kept, the attempts and the compression ratio\n"
            << "  --compression-ratio-threshold X  with --fallback: decode again above this ratio (default 2.4, 0 = off)\n"
            << "  --seek          with --long --timestamps: every window starts at the last closed timestamp of the one\n"
            << "                  before and is decoded behind the text kept so far (Whisper's transcribe loop)\n"
            << "  --no-condition  with --seek: do not feed the previous windows' text to the next (condition_on_previous_text = 0)\n"
            << "  --inputs a.wav,b.wav  with --long --timestamps --seek: the recordings side by side, one window of every file\n"
            << "                  per decoder chain; prints every file's text under a \"== <path>\" line\n"
            << "  --context-ids 1,2,3  with --max-positions: token ids fed in front of the prompt (Whisper's initial_prompt)\n"
            << "  --suppress-default  with --max-positions: Whisper's default logit suppression (the non-speech symbols and\n"
            << "                  the special ids at every position, the bare space and EOT at the first)\n"
            << "  --suppress-tokens 1,2,3  with --max-positions: token ids never generated; --suppress-blank adds the bare\n"
            << "                  space and EOT at the first generated position\n"
            << "  --word-timestamps  with --timestamps: align every word to the audio and print, behind the segment lines,\n"
            << "                  one line per word: t0 t1 text (seconds)\n"
            << "  --alignment-heads 2:2,3:0,...  with --word-timestamps: the layer:head pairs to align on (default: every\n"
            << "                  head of the upper half of the decoder layers)\n";
}
}  // namespace

int main(int argc, char* argv[]) {
  std::string model_prefix, vocab, input, inputs, lang, languages, task, beam, max_positions, temperature, seed, best_of, cr_threshold, context_ids, alignment_heads,
      suppress_tokens;
  bool word_timestamps = false, suppress_default = false, suppress_blank = false;
  bool long_audio = false, english = false, timestamps = false, scores = false, skip_silence = false, fallback = false, seek = false,
       no_condition = false, bf16 = false;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i], v;
    if (a == "-h" || a == "--help") {
      usage(argv[0]);
      return 0;
    }
    if (a == "--long") {
      long_audio = true;
      continue;
    }
    if (a == "--english") {
      english = true;
      continue;
    }
    if (a == "--bf16") {
      bf16 = true;
      continue;
    }
    if (a == "--timestamps") {
      timestamps = true;
      continue;
    }
    if (a == "--scores") {
      scores = true;
      continue;
    }
    if (a == "--word-timestamps") {
      word_timestamps = true;
      continue;
    }
    if (a == "--suppress-default") {
      suppress_default = true;
      continue;
    }
    if (a == "--suppress-blank") {
      suppress_blank = true;
      continue;
    }
    if (a == "--skip-silence") {
      skip_silence = true;
      continue;
    }
    if (a == "--fallback") {
      fallback = true;
      continue;
    }
    if (a == "--seek") {
      seek = true;
      continue;
    }
    if (a == "--no-condition") {
      no_condition = true;
      continue;
    }
    const size_t eq = a.find('=');
    if (eq != std::string::npos) {
      v = a.substr(eq + 1);
      a = a.substr(0, eq);
    } else if (i + 1 < argc) {
      v = argv[++i];
    } else {
      std::cerr << a << ": 1 required TEXT missing\n";
      return 106;
    }
    if (a == "--model-prefix") model_prefix = v;
    else if (a == "--vocab") vocab = v;
    else if (a == "--input") input = v;
    else if (a == "--inputs") inputs = v;
    else if (a == "--lang") lang = v;
    else if (a == "--languages") languages = v;
    else if (a == "--task") task = v;
    else if (a == "--beam") beam = v;
    else if (a == "--max-positions") max_positions = v;
    else if (a == "--temperature") temperature = v;
    else if (a == "--seed") seed = v;
    else if (a == "--best-of") best_of = v;
    else if (a == "--compression-ratio-threshold") cr_threshold = v;
    else if (a == "--context-ids") context_ids = v;
    else if (a == "--alignment-heads") alignment_heads = v;
    else if (a == "--suppress-tokens") suppress_tokens = v;
    else {
      std::cerr << "The following argument was not expected: " << a << "\n";
      usage(argv[0]);
      return 109;
    }
  }
  if (!inputs.empty() && !(long_audio && timestamps && seek)) {
    std::cerr << "--inputs requires --long --timestamps --seek\n";
    return 105;
  }
  if (model_prefix.empty() || vocab.empty() || (input.empty() && inputs.empty())) {
    std::cerr << (model_prefix.empty() ? "--model-prefix" : vocab.empty() ? "--vocab" : "--input")
              << " is required\n";
    usage(argv[0]);
    return 106;
  }
  using namespace whisper;  // NOLINT
  const bool multilingual = !english;  // true is hard-coded in the reference (app/encdec.cpp:47)
  std::unique_ptr<EncDec> engine;
  try {
    engine.reset(new EncDec(model_prefix, vocab, multilingual));
  } catch (const std::exception& e) {  // the reference lets it terminate the process
    std::cerr << "encdec: " << e.what() << "\n";
    return 1;
  }
  EncDec& encdec = *engine;
  if (!lang.empty()) {
    const int id = lang == "auto" ? WT_LANGUAGE_AUTO : language_id(lang);
    const int rc = wt_engine_set_option(encdec.handle(), "language", id);
    if (rc == WT_ERR_UNSUPPORTED) {
      std::cerr << "--lang auto: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
    if (rc != WT_OK) {
      std::cerr << "--lang: unknown language code " << lang << "\n";
      return 105;
    }
  }
  if (!languages.empty()) {
    std::vector<int32_t> ids;
    for (size_t at = 0; at <= languages.size();) {
      const size_t comma = std::min(languages.find(',', at), languages.size());
      if (comma > at) ids.push_back(int32_t(language_id(languages.substr(at, comma - at))));
      at = comma + 1;
    }
    if (ids.empty() || wt_engine_set_language_candidates(encdec.handle(), ids.data(), int(ids.size())) != WT_OK) {
      std::cerr << "--languages: " << (ids.empty() ? "expected language codes, got " + languages : std::string(wt_last_error(encdec.handle()))) << "\n";
      return 105;
    }
  }
  if (!task.empty()) {
    if ((task != "translate" && task != "transcribe") ||
        wt_engine_set_option(encdec.handle(), "task", task == "translate" ? 1 : 0) != WT_OK) {
      std::cerr << "--task: " << (task != "translate" && task != "transcribe" ? "expected translate or transcribe, got " + task : std::string(wt_last_error(encdec.handle()))) << "\n";
      return 105;
    }
  }
  if (bf16 && wt_engine_set_option(encdec.handle(), "bf16", 1) != WT_OK) {
    std::cerr << "--bf16: " << wt_last_error(encdec.handle()) << "\n";
    return 105;
  }
  if (!beam.empty()) {
    char* end = nullptr;
    const long n = std::strtol(beam.c_str(), &end, 10);
    if (end == beam.c_str() || *end || wt_engine_set_option(encdec.handle(), "beam_size", n) != WT_OK) {
      std::cerr << "--beam: expected a beam size in [1, 8], got " << beam << "\n";
      return 105;
    }
  }
  if (!max_positions.empty()) {
    char* end = nullptr;
    const long n = std::strtol(max_positions.c_str(), &end, 10);
    if (end == max_positions.c_str() || *end || wt_engine_set_option(encdec.handle(), "max_positions", n) != WT_OK) {
      std::cerr << "--max-positions: expected 0 or a position count in [32, n_text_ctx], got " << max_positions << "\n";
      return 105;
    }
    // --lang auto with --max-positions: the automatic language of the full-length paths (the library's default refuses it)
    if (lang == "auto" && n > 0 && wt_engine_set_option(encdec.handle(), "full_language", 1) != WT_OK) {
      std::cerr << "--lang auto with --max-positions: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
    // --bf16 with --max-positions: full-length decoding in the bf16 storage mode (the library's default refuses it)
    if (bf16 && n > 0 && wt_engine_set_option(encdec.handle(), "full_bf16", 1) != WT_OK) {
      std::cerr << "--bf16 with --max-positions: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
    // ... and with --inputs, --lang auto or --word-timestamps: the rest of the full-length chains in that mode
    if (bf16 && n > 0 && ((!inputs.empty() && long_audio) || lang == "auto" || word_timestamps) &&
        wt_engine_set_option(encdec.handle(), "full_bf16_all", 1) != WT_OK) {
      std::cerr << "--bf16 with --max-positions: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
    // --beam N with --max-positions: full-length beam search (the option full_beam; the library's default refuses it)
    if (!beam.empty() && n > 0 && wt_engine_set_option(encdec.handle(), "full_beam", 1) != WT_OK) {
      std::cerr << "--beam with --max-positions: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
  }
  if (timestamps) {
    if (max_positions.empty()) {
      std::cerr << "--timestamps requires --max-positions\n";
      return 105;
    }
    if (wt_engine_set_option(encdec.handle(), "timestamps", 1) != WT_OK) {
      std::cerr << "--timestamps: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
  }
  if (scores) {
    if (max_positions.empty()) {
      std::cerr << "--scores requires --max-positions\n";
      return 105;
    }
    if (wt_engine_set_option(encdec.handle(), "scores", 1) != WT_OK) {
      std::cerr << "--scores: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
  }
  if (skip_silence) {
    if (!scores) {
      std::cerr << "--skip-silence requires --scores\n";
      return 105;
    }
    if (wt_engine_set_option(encdec.handle(), "skip_silence", 1) != WT_OK) {
      std::cerr << "--skip-silence: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
  }
  if (!temperature.empty() || fallback || !seed.empty() || !cr_threshold.empty() || !best_of.empty()) {
    if (max_positions.empty()) {
      std::cerr << "--temperature, --seed, --best-of, --fallback and --compression-ratio-threshold require --max-positions\n";
      return 105;
    }
    if (fallback && !scores) {
      std::cerr << "--fallback requires --scores\n";
      return 105;
    }
    auto thousandths = [&](const std::string& text, const char* flag, const char* key) {  // "0.6" -> 600
      char* end = nullptr;
      const double x = std::strtod(text.c_str(), &end);
      if (end == text.c_str() || *end || !(x >= 0.0 && x <= 1000.0) ||
          wt_engine_set_option(encdec.handle(), key, long(x * 1000.0 + 0.5)) != WT_OK) {
        std::cerr << flag << ": " << (end == text.c_str() || *end ? "expected a number" : wt_last_error(encdec.handle())) << ", got " << text << "\n";
        return false;
      }
      return true;
    };
    if (!temperature.empty() && !thousandths(temperature, "--temperature", "temperature")) return 105;
    if (!cr_threshold.empty() && !thousandths(cr_threshold, "--compression-ratio-threshold", "compression_ratio_threshold")) return 105;
    if (!seed.empty()) {
      char* end = nullptr;
      const unsigned long long n = std::strtoull(seed.c_str(), &end, 10);
      if (end == seed.c_str() || *end || wt_engine_set_option(encdec.handle(), "seed", long(n)) != WT_OK) {
        std::cerr << "--seed: expected an unsigned 64-bit number, got " << seed << "\n";
        return 105;
      }
    }
    if (!best_of.empty()) {
      char* end = nullptr;
      const long n = std::strtol(best_of.c_str(), &end, 10);
      if (end == best_of.c_str() || *end || wt_engine_set_option(encdec.handle(), "best_of", n) != WT_OK) {
        std::cerr << "--best-of: expected a number of samples in [1, 8], got " << best_of << "\n";
        return 105;
      }
    }
    if (fallback && wt_engine_set_option(encdec.handle(), "temperature_fallback", 1) != WT_OK) {
      std::cerr << "--fallback: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
    // --beam N with --max-positions and --fallback: beam search is the fall-back's attempt at temperature 0
    if (fallback && !beam.empty() && wt_engine_set_option(encdec.handle(), "fallback_beam", 1) != WT_OK) {
      std::cerr << "--beam with --fallback: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
  }
  if (!context_ids.empty()) {
    if (max_positions.empty()) {
      std::cerr << "--context-ids requires --max-positions\n";
      return 105;
    }
    std::vector<int64_t> ids;
    const char* p = context_ids.c_str();
    bool ok = true;
    while (ok) {
      char* end = nullptr;
      const long long id = std::strtoll(p, &end, 10);
      ok = end != p && id >= 0;
      if (!ok) break;
      ids.push_back(id);
      if (!*end) break;
      ok = *end == ',';
      p = end + 1;
    }
    if (!ok) {
      std::cerr << "--context-ids: expected token ids separated by commas, got " << context_ids << "\n";
      return 105;
    }
    if (ids.size() > 4096) {
      std::cerr << "--context-ids: at most 4096 ids, got " << ids.size() << "\n";
      return 105;
    }
    if (wt_engine_set_context(encdec.handle(), ids.data(), int(ids.size())) != WT_OK) {
      std::cerr << "--context-ids: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
  }
  if (suppress_default || suppress_blank || !suppress_tokens.empty()) {
    if (max_positions.empty()) {
      std::cerr << "--suppress-default, --suppress-tokens and --suppress-blank require --max-positions\n";
      return 105;
    }
    if (suppress_default && (suppress_blank || !suppress_tokens.empty())) {
      std::cerr << "--suppress-default: not together with --suppress-tokens or --suppress-blank\n";
      return 105;
    }
    if (suppress_blank && suppress_tokens.empty()) {
      std::cerr << "--suppress-blank requires --suppress-tokens\n";
      return 105;
    }
    if (suppress_default) {
      if (wt_engine_set_option(encdec.handle(), "suppress_default", 1) != WT_OK) {
        std::cerr << "--suppress-default: " << wt_last_error(encdec.handle()) << "\n";
        return 105;
      }
    } else {
      std::vector<int64_t> ids, first;
      const char* p = suppress_tokens.c_str();
      bool ok = true;
      while (ok) {
        char* end = nullptr;
        const long long id = std::strtoll(p, &end, 10);
        ok = end != p && id >= 0;
        if (!ok) break;
        ids.push_back(id);
        if (!*end) break;
        ok = *end == ',';
        p = end + 1;
      }
      if (!ok || ids.size() > 1024) {
        std::cerr << "--suppress-tokens: expected at most 1024 token ids separated by commas, got " << suppress_tokens << "\n";
        return 105;
      }
      if (suppress_blank) {  // the default first-list of the vocabulary, below the model's n_vocab
        wt_vocab* vv = nullptr;
        wt_dims dims;
        std::vector<int64_t> all(1024), f(1024);
        int32_t n = 0, nf = 0;
        if (wt_vocab_open(vocab.c_str(), multilingual ? 1 : 0, &vv) != WT_OK || wt_engine_dims(encdec.handle(), &dims) != WT_OK ||
            wt_vocab_default_suppress(vv, all.data(), 1024, &n, f.data(), 1024, &nf) != WT_OK) {
          std::cerr << "--suppress-blank: could not form the list from " << vocab << "\n";
          wt_vocab_close(vv);
          return 105;
        }
        wt_vocab_close(vv);
        for (int i = 0; i < nf; ++i) {
          if (f[size_t(i)] < dims.n_vocab) first.push_back(f[size_t(i)]);
        }
      }
      if (wt_engine_set_suppress(encdec.handle(), ids.data(), int(ids.size()), first.data(), int(first.size())) != WT_OK) {
        std::cerr << "--suppress-tokens: " << wt_last_error(encdec.handle()) << "\n";
        return 105;
      }
    }
  }
  if (seek || no_condition) {
    if (no_condition && !seek) {
      std::cerr << "--no-condition requires --seek\n";
      return 105;
    }
    if (!long_audio || !timestamps) {
      std::cerr << "--seek requires --long --timestamps\n";
      return 105;
    }
    if (wt_engine_set_option(encdec.handle(), "seek", 1) != WT_OK ||
        wt_engine_set_option(encdec.handle(), "condition_on_previous_text", no_condition ? 0 : 1) != WT_OK) {
      std::cerr << "--seek: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
  }
  if (word_timestamps || !alignment_heads.empty()) {
    if (!word_timestamps || !timestamps) {
      std::cerr << (word_timestamps ? "--word-timestamps requires --timestamps\n" : "--alignment-heads requires --word-timestamps\n");
      return 105;
    }
    std::vector<int32_t> pairs;  // layer:head,layer:head,...
    for (size_t at = 0; at < alignment_heads.size();) {
      char* end = nullptr;
      const long l = std::strtol(alignment_heads.c_str() + at, &end, 10);
      if (end == alignment_heads.c_str() + at || *end != ':') {
        pairs.clear(), pairs.push_back(-1), pairs.push_back(-1);
        break;
      }
      const char* const hs = end + 1;
      const long hd = std::strtol(hs, &end, 10);
      if (end == hs || (*end && *end != ',')) {
        pairs.clear(), pairs.push_back(-1), pairs.push_back(-1);
        break;
      }
      pairs.push_back(int32_t(l)), pairs.push_back(int32_t(hd));
      at = size_t(end - alignment_heads.c_str()) + (*end ? 1 : 0);
    }
    if (wt_engine_set_alignment_heads(encdec.handle(), pairs.data(), int(pairs.size() / 2)) != WT_OK ||
        wt_engine_set_option(encdec.handle(), "word_timestamps", 1) != WT_OK) {
      std::cerr << "--word-timestamps: " << wt_last_error(encdec.handle()) << "\n";
      return 105;
    }
  }
  if (!inputs.empty()) {  // several recordings side by side: every file's text under a "== <path>" line
    std::vector<std::string> paths;
    for (size_t at = 0; at <= inputs.size();) {
      const size_t comma = std::min(inputs.find(',', at), inputs.size());
      if (comma > at) paths.push_back(inputs.substr(at, comma - at));
      at = comma + 1;
    }
    std::vector<std::vector<float>> pcms;
    std::vector<const float*> ptrs;
    std::vector<size_t> sizes;
    for (const std::string& path : paths) pcms.push_back(wav_read_legacy(path.c_str()));
    for (const std::vector<float>& x : pcms) ptrs.push_back(x.data()), sizes.push_back(x.size());
    if (wt_transcribe_long_batch(encdec.handle(), ptrs.data(), sizes.data(), int(paths.size())) != WT_OK) {
      std::cerr << "transcribe failed: " << wt_last_error(encdec.handle()) << "\n";
      return 1;
    }
    for (size_t f = 0; f < paths.size(); ++f) {
      size_t len = 0;
      wt_last_file_text(encdec.handle(), int(f), nullptr, 0, &len);  // the length first
      std::string text(len + 1, '\0');
      if (wt_last_file_text(encdec.handle(), int(f), &text[0], text.size(), &len) != WT_OK) {
        std::cerr << "transcribe failed: " << wt_last_error(encdec.handle()) << "\n";
        return 1;
      }
      text.resize(len);
      std::cout << "== " << paths[f] << "\n";
      if (lang == "auto") {  // the file's language: what its first window carries
        const int n = wt_last_languages(encdec.handle(), nullptr, nullptr, 0);
        std::vector<int32_t> l(size_t(std::max(n, 1))), wf(size_t(std::max(n, 1)));
        std::vector<float> p(size_t(std::max(n, 1)));
        if (n > 0 && wt_last_languages(encdec.handle(), l.data(), p.data(), n) == n && wt_last_window_files(encdec.handle(), wf.data(), n) == n) {
          const auto w = std::find(wf.begin(), wf.begin() + n, int32_t(f)) - wf.begin();
          if (w < n) std::cout << "language: " << lang_code(size_t(l[size_t(w)])) << " (p=" << p[size_t(w)] << ")\n";
        }
      }
      std::cout << text << "\n";
    }
    return 0;
  }
  std::string text;
  if (long_audio) {
    std::vector<float> pcm = wav_read_legacy(input.c_str());
    std::vector<char> buf(1 << 20);
    size_t len = 0;
    if (wt_transcribe_long_pcm(encdec.handle(), pcm.data(), pcm.size(), buf.data(), buf.size(), &len) != WT_OK) {
      std::cerr << "transcribe failed: " << wt_last_error(encdec.handle()) << "\n";
      return 1;
    }
    text.assign(buf.data(), len);
  } else {
    text = encdec.transcribe(input.c_str());
    // Engine::transcribe returns "" on failure like the reference (whisper.cpp:760): a device error must not
    // look like an empty transcript
    const char* err = wt_last_error(encdec.handle());
    if (err && *err) return 2;
  }
  if (lang == "auto") {  // the languages the decode just used, one per window
    std::vector<int32_t> l(1);
    std::vector<float> p(1);
    const int n = wt_last_languages(encdec.handle(), l.data(), p.data(), 0);
    if (n > 0) {
      l.resize(size_t(n)), p.resize(size_t(n));
      wt_last_languages(encdec.handle(), l.data(), p.data(), n);
      // (a full-length call, --max-positions above 0: every window carries its file's language, one line per file)
      long positions = 0;
      const bool full_length = wt_engine_get_option(encdec.handle(), "max_positions", &positions) == WT_OK && positions > 0;
      for (int i = 0; i < (full_length ? 1 : n); ++i) std::cout << "language: " << lang_code(size_t(l[i])) << " (p=" << p[i] << ")\n";
    }
  }
  if (scores) {  // one line per window
    int w = 0;
    for (const ClipScore& c : encdec.scores()) {
      std::cout << "window " << w++ << ": avg_logprob=" << c.avg_logprob << " no_speech_prob=" << c.no_speech_prob
                << (c.skipped ? " (skipped)" : "") << "\n";
    }
  }
  {  // sampling or fall-back: one line per window
    int w = 0;
    for (const ClipDecode& d : encdec.decode_info()) {
      std::cout << "window " << w++ << ": temperature=" << d.temperature << " attempts=" << d.attempts
                << " compression_ratio=" << d.compression_ratio << (d.needs_fallback ? " (schedule exhausted)" : "") << "\n";
    }
  }
  if (timestamps) {
    auto stamp = [](int ms) {
      char b[32];
      std::snprintf(b, sizeof b, "%02d:%02d.%03d", ms / 60000, ms / 1000 % 60, ms % 1000);
      return std::string(b);
    };
    for (const EncDec::Segment& s : encdec.segments()) {
      std::cout << "[" << stamp(s.t0_ms) << " --> " << stamp(s.t1_ms) << "] " << s.text;
      if (scores) std::cout << " (avg_logprob=" << s.avg_logprob << ")";
      std::cout << "\n";
    }
    if (word_timestamps) {  // behind the segment lines, one line per word: t0 t1 text
      const int n = wt_last_words(encdec.handle(), nullptr, 0);
      std::vector<wt_word> words(size_t(std::max(n, 0)));
      if (n > 0) wt_last_words(encdec.handle(), words.data(), n);
      for (int i = 0; i < n; ++i) {
        size_t len = 0;
        wt_last_word_text(encdec.handle(), i, nullptr, 0, &len);  // the length first: a word is as long as its ids make it
        std::string word(len + 1, '\0');
        wt_last_word_text(encdec.handle(), i, &word[0], word.size(), &len);
        word.resize(len);
        char line[64];
        std::snprintf(line, sizeof line, "%.2f %.2f ", words[size_t(i)].t0_ms / 1000.0, words[size_t(i)].t1_ms / 1000.0);
        std::cout << line << word << "\n";
      }
    }
    return 0;
  }
  std::cout << text << "\n";
  return 0;
}
