// lexicon.cpp -- w2l_lexicon_*: the lexicon trie of the lexicon-constrained CTC beam search, built from spelling rows and walked
// on the host (contract: include/w2l_hip.h; layout and lookups: ../lexicon.hpp).  Host only: nothing here touches the GPU.
#include <cmath>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/w2l_hip.h"
#include "../lexicon.hpp"

#define W2L_API extern "C" __attribute__((visibility("default")))

namespace w2l {
void setHostError(const std::string& m);   // w2l_host_last_error's message (trainer.cpp)

namespace {

struct LexUnsupported : std::runtime_error {
  using std::runtime_error::runtime_error;
};

std::vector<char> buildLexicon(int numTokens, int numWords, size_t S, const int* spellWord, const size_t* spellOff,
                               const int* spellTokens, const float* wordSmear, int silToken, size_t* droppedOut) {
  if (numTokens < 1 || numWords < 1) throw std::invalid_argument("lexicon: numTokens and numWords must be at least 1");
  if (silToken < -1 || silToken >= numTokens) throw std::invalid_argument("lexicon: silToken is outside -1 .. numTokens-1");
  if (S && (!spellWord || !spellOff || !spellTokens)) throw std::invalid_argument("lexicon: NULL spellWord / spellOff / spellTokens");
  if (wordSmear)
    for (int w = 0; w < numWords; ++w)
      if (!std::isfinite(wordSmear[w])) throw std::invalid_argument("lexicon: the smear value of word " + std::to_string(w) + " is not finite");
  std::vector<LexNode> nodes(1);
  std::vector<int> parent(1, -1);
  std::unordered_map<uint64_t, int> childOf;
  std::set<std::pair<int, int>> ends;   // (node, word): every row, dropped ones included, to find duplicates
  size_t dropped = 0;
  nodes[0].smear = 0.f; nodes[0].meta = 0; nodes[0].tok = -1; nodes[0].pad = 0;
  for (int i = 0; i < 8; ++i) nodes[0].words[i] = -1;
  for (size_t r = 0; r < S; ++r) {
    const std::string row = "lexicon: row " + std::to_string(r) + ": ";
    const int w = spellWord[r];
    if (w < 0 || w >= numWords) throw std::invalid_argument(row + "word id " + std::to_string(w) + " is outside 0 .. numWords-1");
    if (spellOff[r + 1] < spellOff[r]) throw std::invalid_argument(row + "spellOff is not ascending");
    const size_t len = spellOff[r + 1] - spellOff[r];
    if (len == 0) throw std::invalid_argument(row + "empty spelling");
    const int* sp = spellTokens + spellOff[r];
    for (size_t i = 0; i < len; ++i)
      if (sp[i] < 0 || sp[i] >= numTokens)
        throw std::invalid_argument(row + "token " + std::to_string(sp[i]) + " is outside 0 .. numTokens-1 (blank cannot be spelled)");
    if (sp[0] == silToken) throw std::invalid_argument(row + "the spelling begins with the silence token");
    int u = 0;
    for (size_t i = 0; i < len; ++i) {
      const uint64_t key = ((uint64_t)(uint32_t)u << 32) | (uint64_t)(uint32_t)(sp[i] + 1);
      auto it = childOf.find(key);
      if (it == childOf.end()) {
        if (nodes.size() + 1 >= (size_t)kLexMaxNodes) throw LexUnsupported("lexicon: 2^28 nodes or more");
        LexNode n;
        n.smear = 0.f; n.meta = 0; n.tok = sp[i]; n.pad = 0;
        for (int j = 0; j < 8; ++j) n.words[j] = -1;
        it = childOf.emplace(key, (int)nodes.size()).first;
        nodes.push_back(n);
        parent.push_back(u);
        nodes[u].meta |= 8u;
      }
      u = it->second;
    }
    if (!ends.emplace(u, w).second) throw std::invalid_argument(row + "duplicate (word, spelling) row, word " + std::to_string(w));
    const int nw = (int)(nodes[u].meta & 7u);
    if (nw < kLexMaxWords) {
      nodes[u].words[nw] = w;
      nodes[u].meta = (nodes[u].meta & ~7u) | (uint32_t)(nw + 1);
    } else {
      ++dropped;
    }
  }
  const size_t numNodes = nodes.size(), edges = numNodes - 1;
  // smear: the exact max over the kept words at or below; children have larger ids than their parents
  std::vector<float> sm(numNodes, -INFINITY);
  for (size_t v = 0; v < numNodes; ++v)
    for (int i = 0; i < (int)(nodes[v].meta & 7u); ++i) sm[v] = std::fmax(sm[v], wordSmear ? wordSmear[nodes[v].words[i]] : 0.f);
  for (size_t v = numNodes - 1; v >= 1; --v) sm[parent[v]] = std::fmax(sm[parent[v]], sm[v]);
  for (size_t v = 0; v < numNodes; ++v) nodes[v].smear = sm[v] == -INFINITY ? 0.f : sm[v];   // -inf: the root of an empty lexicon
  uint32_t cap = 2;
  while (cap < 2 * edges) cap <<= 1;
  const size_t slotOff = sizeof(LexHeader) + numNodes * sizeof(LexNode);
  std::vector<char> blob(slotOff + (size_t)cap * sizeof(LexSlot), 0);
  LexHeader* h = (LexHeader*)blob.data();
  std::memcpy(blob.data() + sizeof(LexHeader), nodes.data(), numNodes * sizeof(LexNode));
  LexSlot* slot = (LexSlot*)(blob.data() + slotOff);
  for (size_t v = 1; v < numNodes; ++v) {   // in node order: the blob is a function of the rows
    const uint64_t key = ((uint64_t)(uint32_t)parent[v] << 32) | (uint64_t)(uint32_t)(nodes[v].tok + 1);
    uint32_t at = lex_hash(key) & (cap - 1);
    while (slot[at].key) at = (at + 1) & (cap - 1);
    slot[at].key = key;
    slot[at].child = (int32_t)v;
  }
  h->magic = kLexMagic;
  h->numTokens = (uint32_t)numTokens;
  h->numWords = (uint32_t)numWords;
  h->numNodes = (uint32_t)numNodes;
  h->cap = cap;
  h->edges = (uint32_t)edges;
  h->smeared = wordSmear ? 1u : 0u;
  h->silToken = silToken;
  h->bytes = blob.size();
  *droppedOut = dropped;
  return blob;
}

const LexHeader* lexHeader(const void* blob) {
  if (!blob) throw std::invalid_argument("lexicon: NULL blob");
  if (((uintptr_t)blob & 15) != 0) throw std::invalid_argument("lexicon: the blob must be 16-byte aligned");
  const LexHeader* h = (const LexHeader*)blob;
  if (h->magic != kLexMagic || h->cap == 0 || (h->cap & (h->cap - 1)) || h->numNodes == 0)
    throw std::invalid_argument("lexicon: not a table built by w2l_lexicon_build");
  return h;
}

template <class F>
int lexGuarded(F&& f) {
  try {
    f();
    return W2L_OK;
  } catch (const LexUnsupported& e) {
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

W2L_API int w2l_lexicon_build(int numTokens, int numWords, size_t numSpellings, const int* spellWord, const size_t* spellOff,
                              const int* spellTokens, const float* wordSmear, int silToken, void* blob, size_t* blobBytes,
                              size_t* dropped) {
  return lexGuarded([&] {
    if (!blobBytes) throw std::invalid_argument("lexicon: NULL blobBytes");
    size_t dr = 0;
    const std::vector<char> b = buildLexicon(numTokens, numWords, numSpellings, spellWord, spellOff, spellTokens, wordSmear, silToken, &dr);
    if (blob) {
      if (((uintptr_t)blob & 15) != 0) throw std::invalid_argument("lexicon: the blob must be 16-byte aligned");
      if (*blobBytes < b.size()) throw std::invalid_argument("lexicon: the blob needs " + std::to_string(b.size()) + " bytes");
      std::memcpy(blob, b.data(), b.size());
    }
    *blobBytes = b.size();
    if (dropped) *dropped = dr;
  });
}

W2L_API int w2l_lexicon_info(const void* blob, int* numTokens, int* numWords, int* numNodes, int* silToken, int* smeared) {
  return lexGuarded([&] {
    const LexHeader* h = lexHeader(blob);
    if (numTokens) *numTokens = (int)h->numTokens;
    if (numWords) *numWords = (int)h->numWords;
    if (numNodes) *numNodes = (int)h->numNodes;
    if (silToken) *silToken = (int)h->silToken;
    if (smeared) *smeared = (int)h->smeared;
  });
}

W2L_API int w2l_lexicon_child(const void* blob, int node, int token, int* child) {
  return lexGuarded([&] {
    const LexHeader* h = lexHeader(blob);
    if (!child) throw std::invalid_argument("lexicon: NULL child");
    if (node < 0 || (uint32_t)node >= h->numNodes) throw std::invalid_argument("lexicon: node out of range");
    if (token < 0 || (uint32_t)token >= h->numTokens) throw std::invalid_argument("lexicon: token out of range");
    *child = lex_child(lex_view(blob), node, token);
  });
}

W2L_API int w2l_lexicon_node(const void* blob, int node, float* smear, int* nw, int* words, int* hasChildren) {
  return lexGuarded([&] {
    const LexHeader* h = lexHeader(blob);
    if (node < 0 || (uint32_t)node >= h->numNodes) throw std::invalid_argument("lexicon: node out of range");
    const LexView v = lex_view(blob);
    const LexNode& n = lex_node(v, node);
    if (smear) *smear = n.smear;
    if (nw) *nw = lex_nw(n);
    if (words)
      for (int i = 0; i < kLexMaxWords; ++i) words[i] = i < lex_nw(n) ? n.words[i] : -1;
    if (hasChildren) *hasChildren = lex_has_children(n) ? 1 : 0;
  });
}
