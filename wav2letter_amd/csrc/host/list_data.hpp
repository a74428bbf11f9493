// list_data.hpp -- what the command-line tools of this directory share (train_main.cpp: Train; align_main.cpp: Align): small file
// helpers and ListData, the list files -> padded device batches pipeline of the reference Trainer (Train.cpp:277-339).  Header only,
// included by the mains alone (the library does not carry it).
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <fstream>
#include <future>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/fl_compat/flashlight.h"
#include "../../../include/fl_compat/audio.h"
#include "../../../include/fl_compat/data.h"
#include "../../../include/fl_compat/text.h"
#include "w2l_host.hpp"

namespace w2l {
namespace cli {

inline bool fileExists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }
inline void mkdirs(const std::string& p) {
  std::string cur;
  for (size_t i = 0; i <= p.size(); ++i) {
    if (i == p.size() || p[i] == '/') { if (!cur.empty()) mkdir(cur.c_str(), 0755); }
    if (i < p.size()) cur += p[i];
  }
}
inline std::string pathJoin(const std::string& a, const std::string& b) {
  if (a.empty() || (!b.empty() && b[0] == '/')) return b;
  return a.back() == '/' ? a + b : a + "/" + b;
}

inline int countTokens(const std::string& path) {
  std::ifstream f(path);
  if (!f) return -1;
  int n = 0;
  std::string line;
  while (std::getline(f, line)) if (!line.empty()) ++n;
  return n;
}

// ---- list files -> padded device batches (Train.cpp:277-339)
struct ListData {
  std::vector<fl::pkg::speech::ListSample> samples;
  std::vector<long> mine;                       // this rank's sample indices, in list order
  fl::lib::text::Dictionary dict;
  fl::lib::text::LexiconMap lexicon;
  std::string wordsep, criterion;
  int replabel = 0, nFeat = 0, batch = 1, padFrames = 64, rate = 16000;
  int localLeft = 0, localRight = 0;            // --localnrmlleftctx / --localnrmlrightctx: both 0 = whole-utterance normalisation
  std::unique_ptr<fl::lib::audio::Mfsc> mfsc;
  af::array unit;                               // LayerNorm (gamma, beta) = (1, 0): the per-utterance normalisation
  long batches() const { return ((long)mine.size() + batch - 1) / batch; }
  // the samples of batch k, in batch order (slimIPL: the keys of the label cache, the transcript column the labels are scored against)
  std::vector<const fl::pkg::speech::ListSample*> samplesOf(long k) const {
    std::vector<const fl::pkg::speech::ListSample*> v;
    for (long i = k * batch; i < std::min<long>((k + 1) * batch, (long)mine.size()); ++i) v.push_back(&samples[(size_t)mine[(size_t)i]]);
    return v;
  }
  // the batch an update trains on: every epoch walks this rank's batches in a fresh order, the SAME order on every rank (the
  // global batch g stays the union of the ranks' batches g), a function of (--seed, epoch) only so that `continue` resumes on the
  // batch the uninterrupted run would have taken (the reference reshuffles per epoch with the epoch as seed:
  // loadPrefetchDataset(trainset, nthread, true /*shuffle*/, curEpoch), recipes/slimIPL/src/Train.cpp:1183)
  uint64_t shuffleSeed = 0;
  mutable long permEpoch = -1;
  mutable std::vector<long> perm;
  long batchOfUpdate(long update) const {   // update = 1, 2, ...
    const long nb = batches(), epoch = (update - 1) / nb, pos = (update - 1) % nb;
    if (epoch != permEpoch) {
      perm.resize((size_t)nb);
      for (long i = 0; i < nb; ++i) perm[(size_t)i] = i;
      std::mt19937_64 g(0x9E3779B97F4A7C15ull * (shuffleSeed + 1) + (uint64_t)epoch);
      for (long i = nb - 1; i > 0; --i) std::swap(perm[(size_t)i], perm[(size_t)(g() % (uint64_t)(i + 1))]);   // (std::shuffle is not portable across libraries)
      permEpoch = epoch;
    }
    return perm[(size_t)pos];
  }

  // host half of a batch: decoded audio + target rows.  Prepared AHEAD of the step by `nthread` decode threads (the reference's
  // --nthread prefetch workers, Train.cpp:331): a LibriSpeech batch is 32 FLAC files x ~10 ms each
  struct HostBatch {
    std::vector<std::vector<float>> audio;
    std::vector<std::vector<int>> rows;
    std::vector<float> sizes;
    std::string error;
  };
  int nthread = 6;
  bool tolerateTextErrors = false;
  std::future<std::shared_ptr<HostBatch>> pending;
  long pendingK = -1;

  std::shared_ptr<HostBatch> decode(long k) const {
    auto hb = std::make_shared<HostBatch>();
    const long lo = k * batch, hi = std::min<long>(lo + batch, (long)mine.size());
    const int B = (int)(hi - lo);
    hb->audio.resize((size_t)B); hb->rows.resize((size_t)B); hb->sizes.assign((size_t)B, 0.f);
    std::vector<std::string> errs((size_t)B);
    auto one = [&](int b) {
      try {
        const auto& smp = samples[(size_t)mine[(size_t)(lo + b)]];
        fl::pkg::speech::Sound snd = fl::pkg::speech::loadSound(smp.path);
        if (snd.rate != rate) throw std::runtime_error(smp.path + ": sample rate " + std::to_string(snd.rate) + ", --samplerate is " + std::to_string(rate));
        if ((long)snd.samples.size() < mfsc->frameSize()) throw std::runtime_error(smp.path + ": shorter than one analysis frame");
        hb->sizes[(size_t)b] = (float)snd.samples.size();
        hb->audio[(size_t)b] = std::move(snd.samples);
        if (!tolerateTextErrors) {
          hb->rows[(size_t)b] = fl::pkg::speech::targetIndices(smp.transcript, lexicon, dict, criterion, replabel, wordsep);
        } else {   // Align: a transcript that cannot be spelled gets an empty target and is reported by the caller, the batch goes on
          try { hb->rows[(size_t)b] = fl::pkg::speech::targetIndices(smp.transcript, lexicon, dict, criterion, replabel, wordsep); }
          catch (const std::invalid_argument&) { hb->rows[(size_t)b].clear(); }
        }
      } catch (const std::exception& e) { errs[(size_t)b] = e.what(); }
    };
    const int nt = std::max(1, std::min(nthread, B));
    std::vector<std::thread> pool;
    std::atomic<int> next{0};
    for (int t = 0; t < nt; ++t)
      pool.emplace_back([&]() { for (int b = next++; b < B; b = next++) one(b); });
    for (auto& th : pool) th.join();
    for (auto& e : errs) if (!e.empty()) { hb->error = e; break; }
    return hb;
  }

  // batch k -> features (T, NFEAT, 1, B) on the device, zero beyond every utterance's own frames; targets [B][L] (-1 padded);
  // sizes [B] in samples.  Returns B (the last batch of an epoch may be short).  The NEXT batch's files are decoded in the
  // background while the caller trains on this one (kNext < 0: the caller does not know it -- slimIPL's unsupervised batches).
  int get(long k, long kNext, af::array& input, std::vector<int>& tgt, int& L, std::vector<float>& sizes, int& T) {
    std::shared_ptr<HostBatch> hb;
    if (pending.valid() && pendingK == k) hb = pending.get();
    else { if (pending.valid()) pending.get(); hb = decode(k); }
    pendingK = kNext;
    if (kNext >= 0) pending = std::async(std::launch::async, [this]() { return decode(pendingK); });
    if (!hb->error.empty()) throw std::runtime_error(hb->error);
    const int B = (int)hb->audio.size();
    const int S = mfsc->frameStride();
    auto& audio = hb->audio;
    auto& rows = hb->rows;
    sizes = hb->sizes;   // (+ one entry below: the sample count the T padded frames stand for)
    long nsMax = 0;
    L = 1;
    for (int b = 0; b < B; ++b) {
      nsMax = std::max<long>(nsMax, (long)audio[(size_t)b].size());
      L = std::max<int>(L, (int)rows[(size_t)b].size());
    }
    // pad to whole strides and to a multiple of padFrames frames: few distinct (B, T) plans of the network
    int Tb = mfsc->numFrames(nsMax);
    Tb = (Tb + padFrames - 1) / padFrames * padFrames;
    const long ns = (long)(Tb - 1) * S + mfsc->frameSize();
    const long nsP = (ns + S - 1) / S * S;
    // T is rounded up beyond the longest utterance: the Transformer blocks' padding mask must divide by what T frames span, not by
    // the longest utterance (the reference pads to the longest only; cpc/SequentialBuilder.cpp:58-81)
    sizes.push_back((float)ns);
    std::vector<float> host((size_t)B * nsP, 0.f);
    for (int b = 0; b < B; ++b) memcpy(host.data() + (size_t)b * nsP, audio[(size_t)b].data(), audio[(size_t)b].size() * sizeof(float));
    af::array dev(af::dim4(nsP, B), host.data());
    af::array feats = mfsc->apply(dev);          // (Tall, NFEAT, 1, B), Tall >= Tb
    const int Tall = (int)feats.dims(0);
    T = Tb;
    input = af::constant(0.0, af::dim4(T, nFeat, 1, B));
    if (localLeft > 0 || localRight > 0) {
      tgt.assign((size_t)B * L, -1);
      for (int b = 0; b < B; ++b) std::copy(rows[(size_t)b].begin(), rows[(size_t)b].end(), tgt.begin() + (size_t)b * L);
      // --localnrmlleftctx / --localnrmlrightctx (Train.cpp:311-315): every frame over its window of the utterance's OWN frames, the
      // whole batch in one w2l_local_norm call on the MFSC output, written into the zeroed batch
      std::vector<int> fr((size_t)B);
      for (int b = 0; b < B; ++b) fr[(size_t)b] = std::min(mfsc->numFrames((long)sizes[(size_t)b]), T);
      af::array frames(af::dim4((af::dim_t)B), fr.data());
      af::array ws(af::dim4((af::dim_t)(w2l_local_norm_workspace_size(B, T) / 4 + 64)));
      void* wsp = (void*)(((uintptr_t)ws.device<float>() + 255) & ~(uintptr_t)255);
      // a context of T - 1 frames already reaches every frame of the batch: the recipes' "whole utterance" values stay inside the
      // call's window limit
      w2l::w2lCheck(w2l_local_norm(B, nFeat, T, (size_t)Tall, feats.device<float>(), frames.device<int>(), std::min(localLeft, T - 1),
                                   std::min(localRight, T - 1), (size_t)T,
                                   input.device<float>(), wsp, (hipStream_t)fl::currentStream()), "local normalisation of the features");
      af::sync();   // frames / ws go out of scope
      return B;
    }
    // per-utterance normalisation over the utterance's OWN frames (fl::lib::audio normalize(): zero mean, unit variance; applied
    // before padding in the reference): gather [NFEAT][T_b] -> LayerNorm with (1, 0) -> scatter into the zeroed batch
    hipStream_t st = (hipStream_t)fl::currentStream();
    const size_t cap = (size_t)nFeat * Tall;
    af::array tmp(af::dim4((af::dim_t)cap)), nrm(af::dim4((af::dim_t)cap)), mr(af::dim4(2));
    af::array stats(af::dim4((af::dim_t)(2 * w2l_layernorm_scratch_doubles(1, cap) + 2)));
    for (int b = 0; b < B; ++b) {
      const int tb = std::min(mfsc->numFrames((long)sizes[(size_t)b]), T);
      const float* src = feats.device<float>() + (size_t)b * nFeat * Tall;
      w2l::hipCheck(hipMemcpy2DAsync(tmp.device<float>(), (size_t)tb * 4, src, (size_t)Tall * 4, (size_t)tb * 4, (size_t)nFeat, hipMemcpyDeviceToDevice, st), "gather features");
      w2l::w2lCheck(w2l_residual_layernorm_forward(1, (size_t)nFeat * tb, tmp.device<float>(), nullptr, tmp.device<float>(), nrm.device<float>(),
                                                   unit.device<float>(), 1e-10f, 0.0, 0, 0, (double*)stats.device<float>(), mr.device<float>(), st), "normalise features");
      w2l::hipCheck(hipMemcpy2DAsync(input.device<float>() + (size_t)b * nFeat * T, (size_t)T * 4, nrm.device<float>(), (size_t)tb * 4, (size_t)tb * 4, (size_t)nFeat,
                                     hipMemcpyDeviceToDevice, st), "scatter features");
    }
    tgt.assign((size_t)B * L, -1);
    for (int b = 0; b < B; ++b) std::copy(rows[(size_t)b].begin(), rows[(size_t)b].end(), tgt.begin() + (size_t)b * L);
    af::sync();   // tmp / nrm / stats go out of scope
    return B;
  }
};

// list files -> ListData with the lists' text pipeline (tokens, lexicon, replabel, wordseparator; surround and usewordpiece are read
// where the paths are turned into words); `which` names the flag in the error messages (validation / alignment sets: allowEmpty --
// every sample on exactly one rank, the tail included)
inline void loadListData(ListData& d, const std::vector<std::string>& paths, int bsz, const std::string& which, bool allowEmpty,
                         const w2l::Flags& flags, const std::string& criterionName, int nFeat, int numClasses, uint64_t seed,
                         const std::string& dataDir) {
  for (auto& lp : paths) {
    std::ifstream lf(lp);
    if (!lf) throw std::invalid_argument("cannot read the list file '" + lp + "' (" + which + " / --datadir)");
    std::stringstream buf;
    buf << lf.rdbuf();
    for (auto& smp : fl::pkg::speech::parseList(buf.str())) {
      d.samples.push_back(smp);
      auto& pth = d.samples.back().path;   // the recipes' lists hold absolute paths; a relative one is taken from --datadir
      if (!pth.empty() && pth[0] != '/' && !fileExists(pth)) pth = pathJoin(dataDir, pth);
    }
  }
  if (d.samples.empty()) throw std::invalid_argument("the " + which + " lists hold no samples");
  d.criterion = criterionName;
  d.replabel = criterionName == "asg" ? (int)flags.geti("replabel", 0) : 0;
  d.wordsep = flags.get("wordseparator", "|");
  d.dict = fl::pkg::speech::createTokenDict(fl::lib::text::Dictionary(pathJoin(flags.get("tokensdir", ""), flags.get("tokens", "tokens.txt"))),
                                            criterionName, d.replabel);
  if ((int)d.dict.indexSize() != numClasses) throw std::invalid_argument("token dictionary size != number of classes");
  const std::string lexPath = flags.get("lexicon", "");
  if (!lexPath.empty() && fileExists(lexPath)) d.lexicon = fl::lib::text::loadWords(lexPath, (int)flags.geti("maxword", -1));
  d.nFeat = nFeat;
  d.batch = bsz;
  d.shuffleSeed = seed;
  d.rate = (int)flags.geti("samplerate", 16000);
  d.padFrames = (int)flags.geti("w2l_pad_frames", 64);
  d.nthread = (int)flags.geti("nthread", 6);
  const long lnLeft = flags.geti("localnrmlleftctx", 0), lnRight = flags.geti("localnrmlrightctx", 0);
  if (lnLeft < 0) throw std::invalid_argument("--localnrmlleftctx=" + std::to_string(lnLeft) + " is negative");
  if (lnRight < 0) throw std::invalid_argument("--localnrmlrightctx=" + std::to_string(lnRight) + " is negative");
  d.localLeft = (int)std::min<long>(lnLeft, 1 << 30);
  d.localRight = (int)std::min<long>(lnRight, 1 << 30);
  fl::lib::audio::FeatureParams fp;
  fp.samplingFreq = d.rate; fp.frameSizeMs = (int)flags.geti("framesizems", 25); fp.frameStrideMs = (int)flags.geti("framestridems", 10);
  fp.numFilterbankChans = nFeat; fp.preemCoef = (float)flags.getd("preemcoef", 0.97); fp.melFloor = (float)flags.getd("melfloor", 1.0);
  if (flags.getb("mfcc", false) || flags.getb("pow", false)) throw std::invalid_argument("list data: only --mfsc features are built (--mfcc / --pow are not)");
  d.mfsc.reset(new fl::lib::audio::Mfsc(fp));
  const float unit[2] = {1.f, 0.f};
  d.unit = af::array(af::dim4(2), unit);
  for (long i : fl::lib::partitionByRoundRobin((long)d.samples.size(), fl::getWorldRank(), fl::getWorldSize(), bsz, allowEmpty))
    d.mine.push_back(i);
}

}  // namespace cli
}  // namespace w2l
