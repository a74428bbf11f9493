// ngram_lm.cpp -- w2l_ngram_lm_*: the back-off n-gram LM table of the fused CTC beam search, built from n-gram arrays or from an
// ARPA text file, and scored on the host (contract: include/w2l_hip.h; layout and score rule: ../ngram_lm.hpp).  Host only: nothing
// here touches the GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/w2l_hip.h"
#include "../ngram_lm.hpp"

#define W2L_API extern "C" __attribute__((visibility("default")))

namespace w2l {
void setHostError(const std::string& m);   // w2l_host_last_error's message (trainer.cpp)

namespace {

struct Unsupported : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct Ngrams {   // order k's n-grams: words [count][k], logp [count], backoff [count]
  std::vector<std::vector<int>> words;
  std::vector<std::vector<float>> logp, bo;
};

std::string spell(const std::vector<int>& g) {
  std::string s = "(";
  for (size_t i = 0; i < g.size(); ++i) s += (i ? " " : "") + std::to_string(g[i]);
  return s + ")";
}

std::vector<char> buildBlob(const Ngrams& in, int numTokens, float unkLogp) {
  const int M = (int)in.words.size();
  if (M < 1) throw std::invalid_argument("ngram lm: order must be at least 1");
  if (M > kNgramMaxOrder)
    throw Unsupported("ngram lm: order " + std::to_string(M) + " is above the format's " + std::to_string(kNgramMaxOrder));
  if (numTokens < 1) throw std::invalid_argument("ngram lm: numTokens must be at least 1");
  if (!std::isfinite(unkLogp)) throw std::invalid_argument("ngram lm: the <unk> log-probability is not finite");
  const int bos = numTokens, eos = numTokens + 1;
  std::map<std::vector<int>, int> stateOf;   // n-gram of order < M -> state; the top order: -1 (only to find duplicates)
  stateOf[{}] = 0;
  uint32_t numStates = 1;
  size_t edges = 0;
  for (int k = 1; k <= M; ++k) {
    const auto& w = in.words[k - 1];
    const size_t cnt = in.logp[k - 1].size();
    if (w.size() != cnt * k) throw std::invalid_argument("ngram lm: order " + std::to_string(k) + ": words and values disagree in size");
    for (size_t i = 0; i < cnt; ++i) {
      std::vector<int> g(w.begin() + i * k, w.begin() + (i + 1) * k);
      for (int x : g)
        if (x < 0 || x > eos) throw std::invalid_argument("ngram lm: word id out of range in the " + std::to_string(k) + "-gram " + spell(g));
      if (!std::isfinite(in.logp[k - 1][i]) || (k < M && !std::isfinite(in.bo[k - 1][i])))
        throw std::invalid_argument("ngram lm: non-finite value in the " + std::to_string(k) + "-gram " + spell(g));
      if (k > 1 && !stateOf.count(std::vector<int>(g.begin(), g.end() - 1)))
        throw std::invalid_argument("ngram lm: the context of the " + std::to_string(k) + "-gram " + spell(g) + " is not itself an n-gram");
      if (!stateOf.emplace(g, k < M ? (int)numStates : -1).second)
        throw std::invalid_argument("ngram lm: duplicate " + std::to_string(k) + "-gram " + spell(g));
      if (k < M) ++numStates;
      ++edges;
    }
  }
  if (edges > ((size_t)1 << 29)) throw Unsupported("ngram lm: more than 2^29 n-grams");
  auto longestSuffixState = [&](const std::vector<int>& g) {   // proper suffixes, longest first
    for (size_t d = 1; d <= g.size(); ++d) {
      auto it = stateOf.find(std::vector<int>(g.begin() + d, g.end()));
      if (it != stateOf.end() && it->second >= 0) return it->second;
    }
    return 0;
  };
  uint32_t cap = 2;
  while (cap < 2 * edges) cap <<= 1;
  const size_t slotOff = (sizeof(NgramHeader) + (size_t)numStates * 8 + 15) & ~(size_t)15;
  std::vector<char> blob(slotOff + (size_t)cap * sizeof(NgramSlot), 0);
  NgramHeader* h = (NgramHeader*)blob.data();
  float* bo = (float*)(blob.data() + sizeof(NgramHeader));
  int32_t* suf = (int32_t*)(bo + numStates);
  NgramSlot* slot = (NgramSlot*)(blob.data() + slotOff);
  for (int k = 1; k <= M; ++k) {
    const auto& w = in.words[k - 1];
    for (size_t i = 0; i < in.logp[k - 1].size(); ++i) {
      const std::vector<int> g(w.begin() + i * k, w.begin() + (i + 1) * k);
      const int ctx = stateOf[std::vector<int>(g.begin(), g.end() - 1)];
      int next;
      if (k < M) {
        next = stateOf[g];
        bo[next] = in.bo[k - 1][i];
        suf[next] = longestSuffixState(g);
      } else {
        next = longestSuffixState(g);
      }
      const uint64_t key = ((uint64_t)(uint32_t)ctx << 32) | (uint64_t)(uint32_t)(g.back() + 1);
      uint32_t at = ngram_hash(key) & (cap - 1);
      while (slot[at].key) at = (at + 1) & (cap - 1);
      slot[at].key = key;
      slot[at].p = in.logp[k - 1][i];
      slot[at].next = next;
    }
  }
  h->magic = kNgramMagic;
  h->order = (uint32_t)M;
  h->numTokens = (uint32_t)numTokens;
  h->numStates = numStates;
  h->cap = cap;
  h->hasBos = stateOf.count({bos}) ? 1u : 0u;
  h->hasEos = stateOf.count({eos}) ? 1u : 0u;
  h->start = (h->hasBos && M > 1) ? (uint32_t)stateOf[{bos}] : 0u;
  h->unkLogp = unkLogp;
  h->edges = (uint32_t)edges;
  h->bytes = blob.size();
  return blob;
}

// the two-call pattern: blob == NULL reports the size; else *blobBytes is the room and becomes the size
void deliver(const std::vector<char>& b, void* blob, size_t* blobBytes) {
  if (blob) {
    if (*blobBytes < b.size()) throw std::invalid_argument("ngram lm: the blob needs " + std::to_string(b.size()) + " bytes");
    std::memcpy(blob, b.data(), b.size());
  }
  *blobBytes = b.size();
}

std::vector<std::string> fields(const std::string& line) {
  std::vector<std::string> out;
  size_t i = 0;
  while (i < line.size()) {
    while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) ++i;
    size_t j = i;
    while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') ++j;
    if (j > i) out.push_back(line.substr(i, j - i));
    i = j;
  }
  return out;
}

float log10ToNat(const std::string& f, const std::string& path, size_t lineNo) {
  char* end = nullptr;
  const double v = std::strtod(f.c_str(), &end);
  if (end == f.c_str() || *end || !std::isfinite(v))
    throw std::invalid_argument("arpa " + path + ":" + std::to_string(lineNo) + ": `" + f + "` is not a finite number");
  return (float)(v * 2.302585092994045684);
}

std::vector<char> parseArpa(const std::string& path, int numTokens, const char* const* tokens, int* skippedOut) {
  FILE* fp = std::fopen(path.c_str(), "rb");
  if (!fp) throw std::invalid_argument("arpa: cannot read " + path);
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof(buf), fp)) > 0) text.append(buf, got);
  std::fclose(fp);
  static const char kBin[] = "mmap lm http://kheafield.com/code format version";
  if (text.compare(0, sizeof(kBin) - 1, kBin) == 0)
    throw std::invalid_argument("arpa " + path + ": this is a KenLM binary file; supply the ARPA text it was built from");
  if (text.size() >= 2 && (unsigned char)text[0] == 0x1f && (unsigned char)text[1] == 0x8b)
    throw std::invalid_argument("arpa " + path + ": gzip is not read; supply the uncompressed ARPA text");
  std::unordered_map<std::string, int> id;
  for (int i = 0; i < numTokens; ++i) {
    if (!tokens[i]) throw std::invalid_argument("arpa: token " + std::to_string(i) + " is NULL");
    id.emplace(tokens[i], i);
  }
  id.emplace("<s>", numTokens);
  id.emplace("</s>", numTokens + 1);
  const bool unkIsToken = id.count("<unk>") != 0;

  std::vector<size_t> declared;   // \data\ counts per order
  Ngrams ng;
  std::vector<size_t> seen;
  int section = 0;                // 0 before \data\, -1 in \data\, k in \k-grams:
  bool ended = false, haveUnk = false;
  float unkLogp = 0.f;
  int skipped = 0;
  size_t pos = 0, lineNo = 0;
  while (pos < text.size() && !ended) {
    size_t nl = text.find('\n', pos);
    if (nl == std::string::npos) nl = text.size();
    const std::string line = text.substr(pos, nl - pos);
    pos = nl + 1;
    ++lineNo;
    const auto f = fields(line);
    if (f.empty()) continue;
    const std::string where = "arpa " + path + ":" + std::to_string(lineNo) + ": ";
    if (f[0][0] == '\\') {
      if (f[0] == "\\data\\" && section == 0) { section = -1; continue; }
      if (f[0] == "\\end\\" && section != 0) { ended = true; continue; }
      int k = 0;
      char tail[16] = {0};
      if (section != 0 && std::sscanf(f[0].c_str(), "\\%d-grams%15s", &k, tail) == 2 && std::string(tail) == ":") {
        if (k != (section == -1 ? 1 : section + 1) || k > (int)declared.size())
          throw std::invalid_argument(where + "section " + f[0] + " is out of order or not declared in \\data\\");
        section = k;
        continue;
      }
      throw std::invalid_argument(where + "unexpected `" + f[0] + "`");
    }
    if (section == 0) continue;   // text before \data\ is a comment
    if (section == -1) {
      int k = 0;
      long long c = -1;
      if (f.size() != 2 || f[0] != "ngram" || std::sscanf(f[1].c_str(), "%d=%lld", &k, &c) != 2 || k != (int)declared.size() + 1 || c < 0)
        throw std::invalid_argument(where + "expected `ngram " + std::to_string(declared.size() + 1) + "=<count>`");
      if (k > kNgramMaxOrder) throw Unsupported(where + "order " + std::to_string(k) + " is above the format's " + std::to_string(kNgramMaxOrder));
      declared.push_back((size_t)c);
      ng.words.emplace_back(); ng.logp.emplace_back(); ng.bo.emplace_back();
      seen.push_back(0);
      continue;
    }
    const int k = section;
    if ((int)f.size() != k + 1 && (int)f.size() != k + 2)
      throw std::invalid_argument(where + "a " + std::to_string(k) + "-gram line has " + std::to_string(f.size()) + " fields");
    ++seen[k - 1];
    const float p = log10ToNat(f[0], path, lineNo);
    const float b = (int)f.size() == k + 2 ? log10ToNat(f[k + 1], path, lineNo) : 0.f;
    if (k == 1 && f[1] == "<unk>" && !unkIsToken) { haveUnk = true; unkLogp = p; continue; }
    int w[kNgramMaxOrder];
    bool known = true;
    for (int i = 0; i < k && known; ++i) {
      auto it = id.find(f[1 + i]);
      known = it != id.end();
      if (known) w[i] = it->second;
    }
    if (!known) { ++skipped; continue; }
    ng.words[k - 1].insert(ng.words[k - 1].end(), w, w + k);
    ng.logp[k - 1].push_back(p);
    ng.bo[k - 1].push_back(b);
  }
  if (section == 0) throw std::invalid_argument("arpa " + path + ": no \\data\\ section");
  if (!ended) throw std::invalid_argument("arpa " + path + ": the file ends before \\end\\");
  if (declared.empty()) throw std::invalid_argument("arpa " + path + ": \\data\\ declares no order");
  for (size_t k = 0; k < declared.size(); ++k)
    if (seen[k] != declared[k])
      throw std::invalid_argument("arpa " + path + ": \\data\\ declares " + std::to_string(declared[k]) + " " + std::to_string(k + 1) +
                                  "-grams, the section holds " + std::to_string(seen[k]));
  if (!haveUnk) {
    std::vector<char> has(numTokens, 0);
    for (int x : ng.words[0])
      if (x < numTokens) has[x] = 1;
    for (int i = 0; i < numTokens; ++i)
      if (!has[i])
        throw std::invalid_argument("arpa " + path + ": token `" + tokens[i] + "` has no unigram and the file has no <unk>");
  }
  *skippedOut = skipped;
  return buildBlob(ng, numTokens, unkLogp);
}

const NgramHeader* header(const void* blob) {
  if (!blob) throw std::invalid_argument("ngram lm: NULL blob");
  if (((uintptr_t)blob & 15) != 0) throw std::invalid_argument("ngram lm: the blob must be 16-byte aligned");
  const NgramHeader* h = (const NgramHeader*)blob;
  if (h->magic != kNgramMagic || h->cap == 0 || (h->cap & (h->cap - 1)) || h->numStates == 0 || h->order == 0)
    throw std::invalid_argument("ngram lm: not a table built by w2l_ngram_lm_build");
  return h;
}

template <class F>
int guarded(F&& f) {
  try {
    f();
    return W2L_OK;
  } catch (const Unsupported& e) {
    setHostError(e.what());
    return W2L_EUNSUPPORTED;
  } catch (const std::exception& e) {
    setHostError(e.what());
    return W2L_EINVAL;
  }
}

}  // namespace
}  // namespace w2l

using namespace w2l;

W2L_API int w2l_ngram_lm_build(int order, const size_t* counts, const int* words, const float* logp, const float* backoff,
                               int numTokens, float unkLogp, void* blob, size_t* blobBytes) {
  return guarded([&] {
    if (!counts || !blobBytes || order < 1) throw std::invalid_argument("ngram lm: NULL counts / blobBytes or order < 1");
    if (order > kNgramMaxOrder)
      throw Unsupported("ngram lm: order " + std::to_string(order) + " is above the format's " + std::to_string(kNgramMaxOrder));
    Ngrams ng;
    size_t wAt = 0, vAt = 0;
    for (int k = 1; k <= order; ++k) {
      const size_t c = counts[k - 1];
      if (c && (!words || !logp)) throw std::invalid_argument("ngram lm: NULL words / logp");
      ng.words.emplace_back(words + wAt, words + wAt + c * k);
      ng.logp.emplace_back(logp + vAt, logp + vAt + c);
      if (backoff) ng.bo.emplace_back(backoff + vAt, backoff + vAt + c);
      else ng.bo.emplace_back(c, 0.f);
      wAt += c * k;
      vAt += c;
    }
    deliver(buildBlob(ng, numTokens, unkLogp), blob, blobBytes);
  });
}

W2L_API int w2l_ngram_lm_from_arpa(const char* path, int numTokens, const char* const* tokens, void* blob, size_t* blobBytes,
                                   int* skipped) {
  return guarded([&] {
    if (!path || !tokens || !blobBytes || numTokens < 1) throw std::invalid_argument("arpa: NULL path / tokens / blobBytes or no tokens");
    int sk = 0;
    deliver(parseArpa(path, numTokens, tokens, &sk), blob, blobBytes);
    if (skipped) *skipped = sk;
    setHostError("arpa " + std::string(path) + ": skipped " + std::to_string(sk) + " n-grams with a word outside the token dictionary");
  });
}

W2L_API int w2l_ngram_lm_info(const void* blob, int* order, int* numTokens, int* numStates, int* hasBos, int* hasEos) {
  return guarded([&] {
    const NgramHeader* h = header(blob);
    if (order) *order = (int)h->order;
    if (numTokens) *numTokens = (int)h->numTokens;
    if (numStates) *numStates = (int)h->numStates;
    if (hasBos) *hasBos = (int)h->hasBos;
    if (hasEos) *hasEos = (int)h->hasEos;
  });
}

W2L_API int w2l_ngram_lm_start(const void* blob, int* state) {
  return guarded([&] {
    const NgramHeader* h = header(blob);
    if (!state) throw std::invalid_argument("ngram lm: NULL state");
    *state = (int)h->start;
  });
}

W2L_API int w2l_ngram_lm_score(const void* blob, int state, int word, float* logp, int* next) {
  return guarded([&] {
    const NgramHeader* h = header(blob);
    if (!logp || !next) throw std::invalid_argument("ngram lm: NULL logp / next");
    if (state < 0 || (uint32_t)state >= h->numStates) throw std::invalid_argument("ngram lm: state out of range");
    if (word < 0 || (uint32_t)word > h->numTokens + 1) throw std::invalid_argument("ngram lm: word id out of range");
    const NgramView v = ngram_view(blob);
    *logp = ngram_q(v, state, word, next);
  });
}
