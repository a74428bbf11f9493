// fl_compat/ipl.h -- the host state of slimIPL: training on a second, unlabelled list whose transcripts the model writes itself
// (header only, nothing of the device; Python twin: tests/ipl_ref.py; tests: tests/cpp/ipl_test.cpp compiled with g++ by
// tests/test_ipl_host.py).  Restated from recipes/slimIPL/src/Train.cpp:
//
//   order of supervised / unsupervised updates   :1214-1225 (per epoch: --slimIPL_sup_updates `true`s then --slimIPL_unsup_updates
//                                                `false`s, shuffled), :1229, :1329-1333 (reshuffled whenever it has been walked)
//   unsupervised batch of naive | cache | pre-cache   :1186-1192, :1309-1327 (a shuffled walk, reshuffled at its end and per epoch)
//   fixed-pre-cache                              :1143-1168, :1193-1207, :1238-1307 -- `fixedCache` (plBatchCacheFixedSize) holds
//                                                --slimIPL_fixed_cache_updates BATCH indices; while it fills the unsupervised step only
//                                                labels ("Skip usage of unsup batch as fixed cache is not ready"); then each step trains
//                                                on the next entry of a shuffled SNAPSHOT of it and, with probability
//                                                --slimIPL_fixed_cache_update_prob, labels the next batch of a shuffled walk over the
//                                                whole list (`fixedCacheIndexToLabel`) and puts it in that entry's place
//   which samples have labels, labelling before / after the update   :1556-1609, :1786-1788, :1833-1840
//   the text caches and their files              :490-545 (read: every rank's `NNN_model_last_cache<rank>`, `id|text` per line, into
//                                                the read-only plCacheDump; this rank's `NNN_model_last_fixed_cache<rank>`, indices
//                                                separated by spaces), :718-746 (written by every rank)
//
// Random draws.  The reference draws from an unseeded std::rand / std::random_shuffle.  Here EVERY draw comes from one splitmix64
// stream seeded with --seed alone -- the same on every rank, so all ranks take a supervised or an unsupervised step together:
//     state += 0x9E3779B97F4A7C15;  z = state;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
//     next = z ^ (z >> 31)                                              (64-bit wrap-around arithmetic, state starts at the seed)
//     uniform = (next >> 11) * 2^-53                                    (the relabel draw: `uniform < update_prob`)
//     shuffle(v): for i = size - 1 down to 1:  j = next % (i + 1);  swap(v[i], v[j])          (Fisher-Yates from the back)
// One draw per fixed-pre-cache step is taken whether or not it is needed (the reference calls std::rand unconditionally, :1239).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace fl {
namespace pkg {
namespace speech {

struct IplRng {
  uint64_t state = 0;
  uint64_t next() {
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
  template <class V> void shuffle(V& v) {
    for (size_t i = v.size(); i-- > 1;) {
      const size_t j = (size_t)(next() % (uint64_t)(i + 1));
      const typename V::value_type t = v[i];   // (a value: std::vector<bool> hands out proxies)
      v[i] = v[j];
      v[j] = t;
    }
  }
};

enum class IplType { Naive, Cache, PreCache, FixedPreCache };
inline IplType parseIplType(const std::string& s) {
  if (s == "naive") return IplType::Naive;
  if (s == "cache") return IplType::Cache;
  if (s == "pre-cache") return IplType::PreCache;
  if (s == "fixed-pre-cache") return IplType::FixedPreCache;
  throw std::invalid_argument("--slimIPL_type=" + s + ": expected naive | cache | pre-cache | fixed-pre-cache");
}

class SlimIPL {
 public:
  struct Options {
    IplType type = IplType::Naive;
    long supUpdates = 1, unsupUpdates = 3;   // --slimIPL_sup_updates / --slimIPL_unsup_updates (0 unsup: no unsupervised list in use)
    long fixedCacheUpdates = 1000;           // --slimIPL_fixed_cache_updates
    double fixedCacheUpdateProb = 1.0;       // --slimIPL_fixed_cache_update_prob
  };
  // what an unsupervised step does before the labels are looked up
  struct Unsup {
    long trainBatch = -1;   // the unsupervised batch to train on; -1: none ("Skip usage of unsup batch as fixed cache is not ready")
    long labelNext = -1;    // fixed-pre-cache: the batch to label with the teacher BEFORE the update ("next batch"); -1: none
    long position = 0;      // what the "Unsup batch n | position" log line shows: the walk's index, or the fixed cache's entry
    bool relabel = true;    // fixed-pre-cache: "update cache 0|1"
  };
  struct Labelled {
    std::vector<int> rows;              // the batch's samples that have a label, in batch order
    std::vector<std::string> texts;     // their labels
    std::vector<std::string> reused;    // ids taken over from the cache files of the run `continue` resumes ("Reuse extra loaded cache")
  };

  std::map<std::string, std::string> plCache;       // sample id -> text, written by this run
  std::map<std::string, std::string> plCacheDump;   // read-only: what `continue` loaded from every rank's cache file
  std::vector<long> fixedCache;                     // plBatchCacheFixedSize

  SlimIPL(const Options& o, long nUnsupBatches, uint64_t seed) : o_(o), nUnsup_(nUnsupBatches) {
    if (o.supUpdates < 0 || o.unsupUpdates < 0 || o.supUpdates + (nUnsup_ > 0 ? o.unsupUpdates : 0) <= 0)
      throw std::invalid_argument("--slimIPL_sup_updates / --slimIPL_unsup_updates: negative, or no update of either kind");
    if (o.type == IplType::FixedPreCache && o.fixedCacheUpdates <= 0) throw std::invalid_argument("--slimIPL_fixed_cache_updates must be positive");
    rng_.state = seed;
    walk_.resize((size_t)std::max<long>(0, nUnsup_));
    for (size_t i = 0; i < walk_.size(); ++i) walk_[i] = (long)i;
  }
  const Options& options() const { return o_; }
  bool useUnsup() const { return nUnsup_ > 0; }

  // once, after the caches of a `continue` are in (:1149-1168)
  void begin() {
    cacheHits_ = std::min<long>((long)fixedCache.size(), o_.fixedCacheUpdates);
    if (o_.type == IplType::FixedPreCache && (long)fixedCache.size() >= o_.fixedCacheUpdates) {
      rng_.shuffle(fixedCache);
      snapshot_ = fixedCache;
    }
  }
  // at the start of every pass over the supervised list (:1186-1225)
  void startEpoch() {
    if (useUnsup()) {
      if (o_.type != IplType::FixedPreCache) {
        for (size_t i = 0; i < walk_.size(); ++i) walk_[i] = (long)i;   // a fresh shuffle of the list, not of the last order
      }
      rng_.shuffle(walk_);   // fixed-pre-cache: unsupBatchesIndices, shuffled in place
    }
    walkIdx_ = 0;
    order_.assign((size_t)o_.supUpdates, true);
    order_.resize((size_t)(o_.supUpdates + (useUnsup() ? o_.unsupUpdates : 0)), false);
    orderIdx_ = 0;
    rng_.shuffle(order_);
  }
  bool nextIsSup() const { return order_.at((size_t)orderIdx_); }   // :1229
  void advanceOrder() {                                            // :1329-1333, after the batch has been chosen
    if (++orderIdx_ >= (long)order_.size()) { orderIdx_ = 0; rng_.shuffle(order_); }
  }
  // the unsupervised batch of this step (:1238-1327)
  Unsup nextUnsup() {
    Unsup u;
    if (o_.type != IplType::FixedPreCache) {
      u.position = walkIdx_;
      u.trainBatch = walk_[(size_t)(walkIdx_ % nUnsup_)];
      if (++walkIdx_ >= nUnsup_) {
        walkIdx_ = 0;
        for (size_t i = 0; i < walk_.size(); ++i) walk_[i] = (long)i;
        rng_.shuffle(walk_);
      }
      return u;
    }
    const double r = rng_.uniform();
    if ((long)fixedCache.size() < o_.fixedCacheUpdates || r < o_.fixedCacheUpdateProb) { ++toLabel_; u.relabel = true; }
    else u.relabel = false;
    // (the reference compares the int with a size_t: the initial -1 counts as past the end, too)
    if (toLabel_ < 0 || toLabel_ >= nUnsup_) { toLabel_ = 0; rng_.shuffle(walk_); }
    if (cacheHits_ == o_.fixedCacheUpdates) {   // the whole cache has been read: take another order of it
      cacheHits_ = 0;
      rng_.shuffle(fixedCache);
      snapshot_ = fixedCache;
    }
    u.position = cacheHits_;
    if ((long)fixedCache.size() >= o_.fixedCacheUpdates) {
      u.trainBatch = snapshot_[(size_t)(cacheHits_ % (long)snapshot_.size())];
      if (u.relabel) fixedCache[(size_t)cacheHits_] = walk_[(size_t)toLabel_];
    } else {
      fixedCache.push_back(walk_[(size_t)toLabel_]);
    }
    if (u.relabel) u.labelNext = walk_[(size_t)toLabel_];
    ++cacheHits_;
    return u;
  }
  // cache | pre-cache | fixed-pre-cache: the samples of a batch that have a label (:1568-1586)
  Labelled labelled(const std::vector<std::string>& ids) {
    Labelled l;
    for (auto& id : ids)
      if (!plCache.count(id) && plCacheDump.count(id)) { plCache[id] = plCacheDump[id]; l.reused.push_back(id); }
    for (size_t i = 0; i < ids.size(); ++i) {
      auto it = plCache.find(ids[i]);
      if (it != plCache.end()) { l.rows.push_back((int)i); l.texts.push_back(it->second); }
    }
    return l;
  }
  // label the training batch with the teacher BEFORE the update, store the texts after it (:1587-1591, :1786-1788)
  bool labelBeforeUpdate(size_t nLabelled) const { return o_.type == IplType::PreCache || (o_.type != IplType::Naive && nLabelled == 0); }
  // label the training batch AFTER the update -- and after the averaged network has moved (:1833-1840)
  bool labelAfterUpdate() const { return o_.type == IplType::Cache; }
  void store(const std::vector<std::string>& ids, const std::vector<std::string>& texts) {
    for (size_t i = 0; i < ids.size() && i < texts.size(); ++i) plCache[ids[i]] = texts[i];
  }

  // ---- files.  `id|text` per line; a text holds no '|' (word separator and line syntax) and no line break: both become spaces
  void saveCache(const std::string& path) const {
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    for (auto& kv : plCache) f << kv.first << "|" << clean(kv.second) << "\n";
  }
  // into plCacheDump; returns the number of lines taken, -1 when the file does not exist (:494-516)
  long loadCacheDump(const std::string& path) {
    std::ifstream f(path);
    if (!f) return -1;
    long n = 0;
    std::string line;
    while (std::getline(f, line)) {
      if (line.empty()) continue;
      const size_t bar = line.find('|');
      if (bar == 0) continue;   // (fl::lib::split drops nothing, but an empty id names no sample)
      if (bar == std::string::npos) plCacheDump[line] = "";
      else {
        const size_t bar2 = line.find('|', bar + 1);   // tmp[1] of split("|", line)
        plCacheDump[line.substr(0, bar)] = line.substr(bar + 1, bar2 == std::string::npos ? std::string::npos : bar2 - bar - 1);
      }
      ++n;
    }
    return n;
  }
  void saveFixedCache(const std::string& path) const {
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    for (long v : fixedCache) f << v << " ";
  }
  // at most --slimIPL_fixed_cache_updates indices (:529-539); false when the file does not exist
  bool loadFixedCache(const std::string& path) {
    std::ifstream f(path);
    if (!f) return false;
    long v;
    while ((long)fixedCache.size() < o_.fixedCacheUpdates && (f >> v)) {
      if (v < 0 || v >= nUnsup_) throw std::runtime_error(path + ": batch index " + std::to_string(v) + " outside the unsupervised list");
      fixedCache.push_back(v);
    }
    return true;
  }

  // ---- everything but the caches, as one line of numbers: what `continue` needs to go on where the saved run stopped (the
  // checkpoint config carries it beside w2l_data_rng.*)
  std::string state() const {
    std::ostringstream s;
    s << rng_.state << " " << orderIdx_ << " " << walkIdx_ << " " << toLabel_ << " " << cacheHits_ << " " << order_.size();
    for (bool b : order_) s << " " << (b ? 1 : 0);
    s << " " << walk_.size();
    for (long v : walk_) s << " " << v;
    s << " " << snapshot_.size();
    for (long v : snapshot_) s << " " << v;
    return s.str();
  }
  void setState(const std::string& text) {
    std::istringstream s(text);
    size_t n = 0;
    if (!(s >> rng_.state >> orderIdx_ >> walkIdx_ >> toLabel_ >> cacheHits_ >> n)) throw std::invalid_argument("slimIPL state: malformed");
    order_.assign(n, false);
    for (size_t i = 0; i < n; ++i) { int b = 0; s >> b; order_[i] = b != 0; }
    s >> n;
    if (n != walk_.size()) throw std::invalid_argument("slimIPL state: written for another unsupervised list");
    for (size_t i = 0; i < n; ++i) s >> walk_[i];
    s >> n;
    snapshot_.assign(n, 0);
    for (size_t i = 0; i < n; ++i) s >> snapshot_[i];
    if (!s) throw std::invalid_argument("slimIPL state: malformed");
  }

 private:
  static std::string clean(std::string t) {
    for (auto& c : t) if (c == '|' || c == '\n' || c == '\r') c = ' ';
    return t;
  }
  Options o_;
  long nUnsup_ = 0;
  IplRng rng_;
  std::vector<bool> order_;     // setsOrder
  long orderIdx_ = 0;           // setsOrderIdx
  std::vector<long> walk_;      // the shuffled walk over the unsupervised batches (fixed-pre-cache: unsupBatchesIndices)
  long walkIdx_ = 0;            // unsupBatchIdx
  long toLabel_ = -1;           // fixedCacheIndexToLabel
  long cacheHits_ = 0;
  std::vector<long> snapshot_;  // the order of the fixed cache that is being read (its entries are replaced in fixedCache meanwhile)
};

}  // namespace speech
}  // namespace pkg
}  // namespace fl
