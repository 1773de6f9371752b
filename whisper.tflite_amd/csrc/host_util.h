// Host-side (CPU, load-time / per-call trivial) pieces of the EncDec path that stay on
// the host in the MI355X build, mirroring the reference's own helpers:
//   WAV reader          whisper.tflite/wav_util.cpp:18-87
//   vocab+filter file   whisper.tflite/whisper.cpp:519-611, :218-226, :746-749
//   token -> text       whisper.tflite/whisper.cpp:634-665, :613-631
//   language table      whisper.tflite/whisper.cpp:405-517
// plus writers for the two on-disk assets, used to create synthetic
// fixtures where the upstream assets are absent.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace wt {

struct VocabData {
  std::map<int, std::string> id_to_token;
  int n_vocab = 51864;  // English defaults (reference whisper.h:69-91)
  int token_eot = 50256;
  int token_sot = 50257;
  int token_translate = 50358;
  int token_transcribe = 50359;
  int token_prev = 50360;
  int token_solm = 50361;
  int token_not = 50362;
  int token_beg = 50363;
};

struct FilterBank {
  int n_mel = 0;
  int n_fft = 0;  // number of frequency bins (201)
  std::vector<float> data;  // [n_mel][n_fft]
};

// Parses the vocab/filter file EncDec consumes.  Throws std::runtime_error when the file
// cannot be opened (as the reference's MmapFile does) or is truncated.
void read_vocab_file(const std::string& path, bool multilingual, FilterBank* filters,
                     VocabData* vocab);
// The same parse over memory that starts at the u32 magic (i.e. after the file's leading u64 payload size),
// as the reference's Reader does (whisper.cpp:519-611); never reads at or past `end`.
void parse_vocab(const char* head, const char* end, bool multilingual, FilterBank* filters, VocabData* vocab);
// whisper.cpp:218-226
void transform_vocab_multilingual(VocabData* vocab);

// Inverse of read_vocab_file: [u64 payload][u32 magic "USEN"][n_mel][n_fft][filters]
// [n_vocab]{u32 len, bytes}.
void write_vocab_file(const std::string& path, const FilterBank& filters,
                      const std::vector<std::string>& tokens);

// Slaney-normalised triangular mel filter bank (librosa.filters.mel defaults; what the
// upstream filters_vocab_*.bin assets contain).
FilterBank make_slaney_filterbank(int n_mel, int n_fft_size, int sample_rate);

// Synthetic token table: the 256 single-byte tokens followed by printable "<tN>" words.
std::vector<std::string> make_synthetic_tokens(int n_tokens);

// Returns false where the reference returns an empty vector (open failure / bad magic).
bool wav_read_legacy(const std::string& path, std::vector<float>* samples, bool verbose);
// Writes a canonical 44-byte-header PCM16 mono WAV (test/bench fixture helper).
bool wav_write_pcm16(const std::string& path, const std::vector<float>& samples, int sample_rate);

std::string decode_tokens(const VocabData& vocab, const int64_t* ids, int n,
                          bool omit_special_tokens, bool* missing);
std::string remove_extra_spaces(const std::string& in);

// Timestamp segments of one id row: the text ids between an opening and a closing timestamp
// (ids >= token_beg, 20 ms per tick).  ids[sample_begin .. n) are read up to the first EOT.  A timestamp behind text
// closes the segment and opens the next; one behind a timestamp opens anew; text left unclosed at the end of the row
// closes at the window end (30 000 ms) with open = 1; text without an opening timestamp starts at 0.  Every id below
// token_beg other than EOT counts as text.  Appends to *out.
struct Segment {
  int32_t clip, t0_ms, t1_ms, id_begin, id_count, open;  // ids[id_begin .. id_begin + id_count): the text, timestamps excluded
};
constexpr int kWindowMs = 30000;
void parse_segments(const VocabData& vocab, const int64_t* ids, int n, int sample_begin, int clip, std::vector<Segment>* out);

// Whisper's default suppression lists from a vocabulary (wt_vocab_default_suppress), ids below
// n_limit only, each list sorted and unique.  *first: the id whose bytes are exactly " " (the smallest such id) and EOT.
// *ids: token_sot, token_prev, token_prev - 1 (Whisper's <|startoflm|>, which this table does not name), token_solm (this
// table's name of the <|nospeech|> id), token_translate, token_transcribe, then the non-speech symbols: for every symbol
// s of Whisper's list the ids whose bytes are exactly s and " " + s,
// the exact " -" and " '", and for a musical symbol without an exact match the longest token whose bytes are a proper
// prefix of the string (the smallest id among equally long ones).  Text matches are taken among the ids below EOT; EOT
// itself never enters *ids.  The prefix rule is not BPE: see the header.
void default_suppress(const VocabData& vocab, int n_limit, std::vector<long long>* ids, std::vector<long long>* first);

int language_count();
int language_id(const std::string& code);  // == language_count() when absent
const std::string& lang_code(size_t id);
const std::string& lang_name(size_t id);

}  // namespace wt
