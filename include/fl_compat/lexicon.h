// fl_compat/lexicon.h -- the lexicon trie of the lexicon-constrained CTC beam search as a C++ object (header only): the table
// w2l_lexicon_build makes (contract: w2l_hip.h -- nodes, edges, the six words of a node, smear, the blob) on the host, and its copy
// on the device for CTCLoss::BeamSearchOptions::lexicon.  Word ids are the ranks of the words sorted bytewise; words() is that list,
// the one NGramLM::fromArpa(path, lexicon.words()) takes for a LM over words.  A refusal of the library throws
// std::invalid_argument (std::runtime_error for a trie beyond the format) with the library's message.
#pragma once
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../w2l_hip.h"
#include "flashlight.h"
#include "lm.h"
#include "text.h"

namespace fl {
namespace pkg {
namespace speech {

class Lexicon {
 public:
  struct Node {
    float smear;
    std::vector<int> words;
    bool hasChildren;
  };
  // rows (word id, token ids) in the order that decides which six words a node keeps; wordSmear: one value per word, or empty (no
  // smearing); silToken: the silence token or -1
  static Lexicon fromSpellings(const std::vector<std::pair<int, std::vector<int>>>& rows, int numTokens, int numWords,
                               const std::vector<float>& wordSmear = {}, int silToken = -1, std::vector<std::string> words = {}) {
    if (!wordSmear.empty() && (int)wordSmear.size() != numWords)
      throw std::invalid_argument("Lexicon::fromSpellings: wordSmear must have one entry per word");
    std::vector<int> sw, toks;
    std::vector<size_t> off(1, 0);
    for (auto& r : rows) {
      sw.push_back(r.first);
      toks.insert(toks.end(), r.second.begin(), r.second.end());
      off.push_back(toks.size());
    }
    Lexicon lx;
    size_t bytes = 0, dropped = 0;
    auto call = [&](void* blob, size_t* n) {
      return w2l_lexicon_build(numTokens, numWords, rows.size(), sw.data(), off.data(), toks.data(),
                               wordSmear.empty() ? nullptr : wordSmear.data(), silToken, blob, n, &dropped);
    };
    check(call(nullptr, &bytes));
    lx.mem_->assign(bytes + 16, 0);
    lx.offset_ = (16 - ((uintptr_t)lx.mem_->data() & 15)) & 15;   // the blob must be 16-byte aligned
    check(call(lx.mem_->data() + lx.offset_, &bytes));
    lx.bytes_ = bytes;
    lx.dropped_ = dropped;
    int smeared = 0;
    check(w2l_lexicon_info(lx.blob(), &lx.numTokens_, &lx.numWords_, &lx.numNodes_, &lx.sil_, &smeared));
    lx.smeared_ = smeared != 0;
    if (words.empty())
      for (int i = 0; i < numWords; ++i) words.push_back(std::to_string(i));
    lx.words_ = std::move(words);
    return lx;
  }
  // a lexicon file (`word tok tok ...`, every spelling of a word a line) over the token dictionary's entries (without blank).  Rows
  // go word by word in the order the words first appear, a word's spellings in file order.  sil: the spelling of the silence token
  // or empty.  smearing "max": wordSmear[w] = q(start, w) of lm (a LM over words(), or null: no smearing); "none": no smearing.
  // replabel > 0 (an ASG model's --replabel): every spelling is packed with packReplabels before the trie is built -- `h e l l o`
  // becomes `h e l <1> o` -- and the tokens `<1>` .. `<replabel>` must be among `tokens`.
  static Lexicon fromFile(const std::string& path, const std::vector<std::string>& tokens, const NGramLM* lm = nullptr,
                          const std::string& sil = "", const std::string& smearing = "max", int replabel = 0) {
    if (smearing != "max" && smearing != "none")
      throw std::invalid_argument("Lexicon::fromFile: smearing '" + smearing + "' is not built: `max` or `none`");
    const lib::text::Dictionary dict = replabel > 0 ? lib::text::Dictionary(tokens) : lib::text::Dictionary();
    for (int r = 1; r <= replabel; ++r)
      if (!dict.contains(replabelToken(r)))
        throw std::invalid_argument("Lexicon::fromFile: replabel=" + std::to_string(replabel) + " needs the token `" +
                                    replabelToken(r) + "` in the token dictionary");
    std::ifstream f(path);
    if (!f) throw std::invalid_argument("Lexicon::fromFile: cannot read " + path);
    std::unordered_map<std::string, int> tokenId, seen;
    for (size_t i = 0; i < tokens.size(); ++i) tokenId.emplace(tokens[i], (int)i);
    std::vector<std::string> order;                                  // words as they first appear
    std::vector<std::vector<std::vector<int>>> spellings;
    for (std::string line; std::getline(f, line);) {
      std::istringstream ss(line);
      std::string word, tok;
      if (!(ss >> word)) continue;
      std::vector<int> sp;
      while (ss >> tok) {
        auto it = tokenId.find(tok);
        if (it == tokenId.end())
          throw std::invalid_argument("Lexicon::fromFile: the spelling of `" + word + "` has the token `" + tok +
                                      "`, which the token dictionary lacks");
        sp.push_back(it->second);
      }
      if (sp.empty()) continue;
      sp = packReplabels(sp, dict, replabel);
      auto at = seen.emplace(word, (int)order.size());
      if (at.second) { order.push_back(word); spellings.emplace_back(); }
      spellings[(size_t)at.first->second].push_back(sp);
    }
    std::vector<std::string> words = order;
    std::sort(words.begin(), words.end());                           // std::string compares bytes
    std::unordered_map<std::string, int> wid;
    for (size_t i = 0; i < words.size(); ++i) wid.emplace(words[i], (int)i);
    std::vector<std::pair<int, std::vector<int>>> rows;
    for (size_t i = 0; i < order.size(); ++i)
      for (auto& sp : spellings[i]) rows.emplace_back(wid[order[i]], sp);
    std::vector<float> smear;
    if (smearing == "max" && lm) {
      if (lm->numTokens() != (int)words.size())
        throw std::invalid_argument("Lexicon::fromFile: the LM has " + std::to_string(lm->numTokens()) + " words, the lexicon " +
                                    std::to_string(words.size()));
      for (size_t i = 0; i < words.size(); ++i) smear.push_back(lm->score(lm->start(), (int)i).first);
    }
    int silId = -1;
    if (!sil.empty()) {
      auto it = tokenId.find(sil);
      if (it == tokenId.end()) throw std::invalid_argument("Lexicon::fromFile: the silence token `" + sil + "` is not in the token dictionary");
      silId = it->second;
    }
    return fromSpellings(rows, (int)tokens.size(), (int)words.size(), smear, silId, words);
  }

  int numTokens() const { return numTokens_; }
  int numWords() const { return numWords_; }
  int numNodes() const { return numNodes_; }
  int silToken() const { return sil_; }
  bool smeared() const { return smeared_; }
  size_t dropped() const { return dropped_; }
  const std::vector<std::string>& words() const { return words_; }
  const void* blob() const { return mem_->data() + offset_; }
  size_t blobBytes() const { return bytes_; }
  // the child of `node` by `token`, -1 when the edge is absent
  int child(int node, int token) const {
    int c = -1;
    check(w2l_lexicon_child(blob(), node, token, &c));
    return c;
  }
  Node node(int node) const {
    Node n;
    int nw = 0, w[6], hc = 0;
    check(w2l_lexicon_node(blob(), node, &n.smear, &nw, w, &hc));
    n.words.assign(w, w + nw);
    n.hasChildren = hc != 0;
    return n;
  }
  // a row of word ids of CTCLoss::BeamSearchResult::words -> the words; the -1 padding of the row ends it
  std::vector<std::string> wordIds2Words(const std::vector<int>& ids) const {
    std::vector<std::string> out;
    for (int i : ids) {
      if (i < 0) break;
      out.push_back(words_.at((size_t)i));
    }
    return out;
  }
  // the table on the device, copied at the first call (copies of this object share it)
  const void* deviceBlob() const {
    if (dev_->isempty()) *dev_ = af::array(af::dim4((af::dim_t)(bytes_ / 4)), (const int*)blob());
    return dev_->device<void>();
  }

 private:
  Lexicon() : mem_(std::make_shared<std::vector<unsigned char>>()), dev_(std::make_shared<af::array>()) {}
  static void check(int status) {
    if (status == W2L_OK) return;
    const std::string msg = w2l_host_last_error();
    if (status == W2L_EINVAL) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
  }
  std::shared_ptr<std::vector<unsigned char>> mem_;
  std::shared_ptr<af::array> dev_;
  size_t offset_ = 0, bytes_ = 0, dropped_ = 0;
  int numTokens_ = 0, numWords_ = 0, numNodes_ = 0, sil_ = -1;
  bool smeared_ = false;
  std::vector<std::string> words_;
};

}  // namespace speech
}  // namespace pkg
}  // namespace fl
