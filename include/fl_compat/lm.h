// fl_compat/lm.h -- the back-off n-gram language model of the LM-fused CTC beam search as a C++ object (header only): the table
// w2l_ngram_lm_build / w2l_ngram_lm_from_arpa make (contract: w2l_hip.h -- words, states, edges, the score rule q, the blob) on the
// host, and its copy on the device for CTCLoss::BeamSearchOptions::lm.  Words 0 .. numTokens()-1 are the token classes, bos() and
// eos() follow.  A refusal of the library throws std::invalid_argument (std::runtime_error for an order beyond the format) with
// the library's message.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../w2l_hip.h"
#include "flashlight.h"

namespace fl {
namespace pkg {
namespace speech {

class NGramLM {
 public:
  // ARPA text; tokens[i] spells class i (the token dictionary's entries without blank).  skipped(): n-grams left out for a word
  // outside the dictionary.
  static NGramLM fromArpa(const std::string& path, const std::vector<std::string>& tokens) {
    std::vector<const char*> spell;
    for (auto& t : tokens) spell.push_back(t.c_str());
    NGramLM lm;
    int skipped = 0;
    lm.twoCalls([&](void* blob, size_t* bytes) {
      return w2l_ngram_lm_from_arpa(path.c_str(), (int)spell.size(), spell.data(), blob, bytes, &skipped);
    });
    lm.skipped_ = skipped;
    lm.message_ = w2l_host_last_error();
    lm.readInfo();
    return lm;
  }
  // n-grams per order, concatenated as w2l_ngram_lm_build takes them (natural logs; backoff may be empty: all 0)
  static NGramLM fromNgrams(const std::vector<size_t>& counts, const std::vector<int>& words, const std::vector<float>& logp,
                            const std::vector<float>& backoff, int numTokens, float unkLogp) {
    size_t values = 0, ids = 0;
    for (size_t k = 0; k < counts.size(); ++k) { values += counts[k]; ids += counts[k] * (k + 1); }
    if (logp.size() != values || words.size() != ids || (!backoff.empty() && backoff.size() != values))
      throw std::invalid_argument("NGramLM::fromNgrams: counts, words, logp and backoff disagree in size");
    NGramLM lm;
    lm.twoCalls([&](void* blob, size_t* bytes) {
      return w2l_ngram_lm_build((int)counts.size(), counts.data(), words.data(), logp.data(), backoff.empty() ? nullptr : backoff.data(),
                                numTokens, unkLogp, blob, bytes);
    });
    lm.readInfo();
    return lm;
  }

  int order() const { return order_; }
  int numTokens() const { return numTokens_; }
  int numStates() const { return numStates_; }
  bool hasBos() const { return hasBos_; }
  bool hasEos() const { return hasEos_; }
  int bos() const { return numTokens_; }
  int eos() const { return numTokens_ + 1; }
  int start() const { return start_; }
  int skipped() const { return skipped_; }
  const std::string& message() const { return message_; }
  const void* blob() const { return mem_->data() + offset_; }
  size_t blobBytes() const { return bytes_; }
  // q(state, word) -> (log p, next state)
  std::pair<float, int> score(int state, int word) const {
    float p = 0.f;
    int next = 0;
    check(w2l_ngram_lm_score(blob(), state, word, &p, &next));
    return {p, next};
  }
  // the unweighted LM score of a label row as lmScores defines it: q in label order from the start state, then the EOS term
  float sentence(const std::vector<int>& labels) const {
    float acc = 0.f;
    int s = start_;
    for (int c : labels) { auto r = score(s, c); acc = acc + r.first; s = r.second; }
    if (hasEos_) acc = acc + score(s, eos()).first;
    return acc;
  }
  // the table on the device, copied at the first call (copies of this object share it)
  const void* deviceBlob() const {
    if (dev_->isempty()) *dev_ = af::array(af::dim4((af::dim_t)(bytes_ / 4)), (const int*)blob());
    return dev_->device<void>();
  }

 private:
  NGramLM() : mem_(std::make_shared<std::vector<unsigned char>>()), dev_(std::make_shared<af::array>()) {}
  static void check(int status) {
    if (status == W2L_OK) return;
    const std::string msg = w2l_host_last_error();
    if (status == W2L_EINVAL) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
  }
  template <class F>
  void twoCalls(F&& call) {
    size_t bytes = 0;
    check(call(nullptr, &bytes));
    mem_->assign(bytes + 16, 0);
    offset_ = (16 - ((uintptr_t)mem_->data() & 15)) & 15;   // the blob must be 16-byte aligned
    check(call(mem_->data() + offset_, &bytes));
    bytes_ = bytes;
  }
  void readInfo() {
    int bosFlag = 0, eosFlag = 0;
    check(w2l_ngram_lm_info(blob(), &order_, &numTokens_, &numStates_, &bosFlag, &eosFlag));
    check(w2l_ngram_lm_start(blob(), &start_));
    hasBos_ = bosFlag != 0;
    hasEos_ = eosFlag != 0;
  }
  std::shared_ptr<std::vector<unsigned char>> mem_;
  std::shared_ptr<af::array> dev_;
  size_t offset_ = 0, bytes_ = 0;
  int order_ = 0, numTokens_ = 0, numStates_ = 0, start_ = 0, skipped_ = 0;
  bool hasBos_ = false, hasEos_ = false;
  std::string message_;
};

}  // namespace speech
}  // namespace pkg
}  // namespace fl
