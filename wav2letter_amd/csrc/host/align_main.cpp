// align_main.cpp -- `Align <outfile> --am=<NNN_model_*.bin> --test=<list> [--datadir=] [--batchsize=] [--lexicon=] [--tokens=
// --tokensdir=] [--k=v ...]`: the reference's forced-alignment tool (command line: recipes/sota/2019/lm_analysis/README.md:81-92; its
// output is read by filter_segmentations.py / shuffle_segments.py of that directory) over the fl:: surface.
//
// Flags come from the checkpoint's `gflags` entry as `Train fork` reads them, then from the command line (the last definition wins).
// The tool builds the network and the criterion, loads both from --am, and runs the eval-mode network over the --test list in list
// order in batches of --batchsize (the short last batch included), through the Trainer's own list pipeline (list_data.hpp: audio
// decoded on the host, MFSC and the per-utterance normalisation on the device, targets from --tokens / --lexicon).
//   CTC: one CTCLoss::viterbiPathWithTarget call per batch with the utterances' emission-frame counts (w2l_ctc_align).
//   ASG: w2l_fac_viterbi has no frame counts, so it is called per utterance on the [1][frames_b][N] prefix of that utterance's
//        emissions (contiguous in the [B][T][N] layout).
// Emission frames of utterance b: with Tin the padded input frames of the batch, Tout the emission frames and tb the utterance's
// own MFSC frames, frames_b = clamp(ceil(tb * Tout / Tin), 1, Tout); one emission frame lasts framestridems / 1000 * Tin / Tout s.
// One line per sample (fl_compat/text.h: alignmentTokenSpans, targetWordIndex, wordSegments, formatAlignmentLine):
//   <sample id>\t<seg>\n<seg>...   the two characters backslash-n between segments, a real newline at the end
//   <seg> = ID A <begin> <length> <word>, seconds with 2 decimals; silence is the word `$`, and the first segment always is one
// An utterance whose target does not fit its frames, or whose transcript has a word outside the lexicon, is reported on stderr and
// left out of the file.  Exit status 0 if at least one line was written.
// --w2l_dump_features=<prefix> writes batch k's features (k = 1, 2, ...) to <prefix>.<k> in Train's format.
#include <cmath>
#include <cstdio>
#include <iostream>

#include "list_data.hpp"

using namespace fl;
using namespace fl::pkg::speech;
using namespace w2l::cli;

namespace {
int usage(const char* exe) {
  std::cerr << "Usage: \n " << exe << " <outfile> --am=<model> --test=<list> [--datadir=...] [--batchsize=...] [flags]" << std::endl;
  return 2;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc <= 2 || std::string(argv[1]).rfind("--", 0) == 0) return usage(argv[0]);
  const std::string outPath = argv[1];
  try {
    using Serializer = fl::pkg::runtime::Serializer;
    w2l::Flags cmd;
    for (int i = 2; i < argc; ++i)
      for (auto& kv : w2l::parseFlagsText(argv[i]).kv) cmd.kv.push_back(kv);
    const std::string am = cmd.get("am", "");
    if (am.empty()) throw std::invalid_argument("--am=<model file> is required");
    std::string version;
    Serializer::Config cfg;
    Serializer::load(am, version, cfg);
    auto it = cfg.find("gflags");
    if (it == cfg.end()) throw std::invalid_argument("Invalid config loaded from " + am);
    w2l::Flags flags = w2l::parseFlagsText(it->second);
    for (auto& kv : cmd.kv) flags.kv.push_back(kv);
    w2l::checkFlagDependencies(flags);

    const std::string criterionName = flags.get("criterion", "asg");
    const int batch = (int)flags.geti("batchsize", 1);
    if (batch <= 0) throw std::invalid_argument("--batchsize must be positive");
    const int nFeat = flags.getb("mfcc", false) ? (int)flags.geti("mfcccoeffs", 13) * 3
                      : flags.getb("pow", false) ? (int)flags.geti("framesizems", 25) * 8 + 1 : (int)flags.geti("filterbanks", 40);
    const std::string tok = pathJoin(flags.get("tokensdir", ""), flags.get("tokens", "tokens.txt"));
    int numClasses = countTokens(tok);
    if (numClasses <= 0) throw std::invalid_argument("cannot read the token dictionary '" + tok + "' (--tokensdir / --tokens)");
    if (criterionName == "asg") numClasses += (int)flags.geti("replabel", 0);
    if (criterionName == "ctc") numClasses += 1;  // blank, appended LAST

    // ---- network and criterion, both from the model file (Train fork's construction)
    const std::string archPath = pathJoin(flags.get("archdir", ""), flags.get("arch", ""));
    if (!fileExists(archPath)) throw std::invalid_argument("arch file / plugin '" + archPath + "' not found (--archdir / --arch)");
    auto scalemode = getCriterionScaleMode(flags.get("onorm", "none"), flags.getb("sqnorm", false));
    std::shared_ptr<fl::Module> network = fl::pkg::runtime::ModulePlugin(archPath).arch(nFeat, numClasses);
    if (flags.getb("fl_amp_use_mixed_precision", false)) setMixedPrecision(network, true);
    if (flags.getb("fl_amp_use_mixed_precision", false) && flags.getb("w2l_amp_convs", false)) setMixedPrecisionConvolutions(network, true);
    std::shared_ptr<SequenceCriterion> criterion;
    if (criterionName == "ctc") criterion = std::make_shared<CTCLoss>(scalemode);
    else if (criterionName == "asg") criterion = std::make_shared<ASGLoss>(numClasses, scalemode, flags.getd("transdiag", 0.0));
    else throw std::invalid_argument("unsupported criterion '" + criterionName + "' (this build: ctc, asg)");
    Serializer::Config unused;
    Serializer::load(am, version, unused, network, criterion);
    network->eval();
    criterion->eval();
    std::cerr << "[Align] " << criterion->prettyString() << ", " << numClasses << " classes, model " << am << std::endl;

    // ---- the list
    const std::string dataDir = flags.get("datadir", "");
    std::vector<std::string> listPaths;
    {
      std::istringstream ls(flags.get("test", ""));
      for (std::string one; std::getline(ls, one, ',');) if (!one.empty()) listPaths.push_back(pathJoin(dataDir, one));
    }
    if (listPaths.empty()) throw std::invalid_argument("--test=<list file> is required");
    ListData d;
    d.tolerateTextErrors = true;
    loadListData(d, listPaths, batch, "--test", true, flags, criterionName, nFeat, numClasses, (uint64_t)flags.geti("seed", 0), dataDir);
    const bool wp = flags.getb("usewordpiece", false);
    const double strideMs = flags.getd("framestridems", 10);
    const std::string dump = flags.get("w2l_dump_features", "");

    std::ofstream outFile(outPath);
    if (!outFile) throw std::runtime_error("cannot open '" + outPath + "' for writing");
    long written = 0, skipped = 0;
    const long nb = d.batches();
    for (long k = 0; k < nb; ++k) {
      af::array feats;
      std::vector<float> sizes;
      std::vector<int> tgt;
      int L = 1, Tin = 0;
      const int B = d.get(k, k + 1 < nb ? k + 1 : 0, feats, tgt, L, sizes, Tin);
      if (!dump.empty()) {   // [B][NFEAT][T] float32, Train's --w2l_dump_features format
        std::vector<float> hf((size_t)feats.elements());
        feats.host(hf.data());
        std::ofstream df(dump + "." + std::to_string(k + 1), std::ios::binary);
        const int hd[3] = {B, nFeat, Tin};
        df.write((const char*)hd, sizeof hd);
        df.write((const char*)hf.data(), (std::streamsize)(hf.size() * 4));
      }
      af::array inSizes(af::dim4(1, (af::dim_t)sizes.size()), sizes.data());
      auto out = network->forward({fl::input(feats), fl::noGrad(inSizes)}).front();
      const int N = (int)out.dims(0), Tout = (int)out.dims(1);
      if (N != numClasses || (int)out.dims(2) != B) throw std::runtime_error("the network's output is not (classes, frames, batch)");
      std::vector<int> frames((size_t)B);
      for (int b = 0; b < B; ++b) {
        const long tb = std::min(d.mfsc->numFrames((long)sizes[(size_t)b]), Tin);
        frames[(size_t)b] = (int)std::min<long>(std::max<long>((tb * Tout + Tin - 1) / Tin, 1), Tout);
      }
      const double secondsPerFrame = strideMs / 1000.0 * (double)Tin / (double)Tout;
      af::array target(af::dim4(L, B), tgt.data());
      std::vector<int> path((size_t)B * Tout, -1);
      if (criterionName == "ctc") {
        criterion->viterbiPathWithTarget(out.array(), target, af::array(af::dim4(1, B), frames.data())).host(path.data());
      } else {
        hipStream_t st = (hipStream_t)fl::currentStream();
        af::array dpath(af::dim4(Tout, B), af::s32), ts(af::dim4(1), af::s32);
        af::array ws(af::dim4((af::dim_t)(w2l_fac_workspace_size(1, Tout, N, L) / 4 + 64)));
        const float* trans = criterion->param(0).array().device<float>();
        w2l::hipCheck(hipMemsetAsync(dpath.device<int>(), 0xff, (size_t)B * Tout * sizeof(int), st), "clear paths");
        for (int b = 0; b < B; ++b) {
          if (tgt[(size_t)b * L] < 0) continue;   // no target (an unspellable transcript): the row stays -1 and is reported below
          const int F = frames[(size_t)b];
          const int* yb = target.device<int>() + (size_t)b * L;
          w2l::w2lCheck(w2l_batch_target_size(1, L, F, yb, ts.device<int>(), st), "target size");
          w2l::w2lCheck(w2l_fac_viterbi(1, F, N, L, out.array().device<float>() + (size_t)b * Tout * N, yb, ts.device<int>(), trans,
                                        dpath.device<int>() + (size_t)b * Tout, ws.device<float>(), st), "fac viterbi");
        }
        dpath.host(path.data());
      }
      for (int b = 0; b < B; ++b) {
        const auto& smp = d.samples[(size_t)d.mine[(size_t)(k * batch + b)]];
        try {
          for (auto& w : smp.transcript)
            if (d.lexicon.find(w) == d.lexicon.end()) throw std::invalid_argument("word '" + w + "' is not in the lexicon");
          std::vector<int> row;
          for (int i = 0; i < L && tgt[(size_t)b * L + i] >= 0; ++i) row.push_back(tgt[(size_t)b * L + i]);
          const auto widx = targetWordIndex(smp.transcript, d.lexicon, d.dict, criterionName, d.replabel, d.wordsep, "", wp);
          if (widx.size() != row.size()) throw std::logic_error("word index and target differ in length");
          const int F = frames[(size_t)b];
          std::vector<int> pv(path.begin() + (size_t)b * Tout, path.begin() + (size_t)b * Tout + F);
          const auto spans = alignmentTokenSpans(pv, row, criterionName == "ctc" ? N - 1 : -1);
          outFile << formatAlignmentLine(smp.id, wordSegments(spans, widx, smp.transcript, F, secondsPerFrame));
          ++written;
        } catch (const std::invalid_argument& e) {
          std::cerr << "[Align] " << smp.id << " left out: " << e.what() << std::endl;
          ++skipped;
        }
      }
    }
    outFile.close();
    std::cerr << "[Align] " << written << " of " << written + skipped << " samples written to " << outPath << std::endl;
    return written > 0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::cerr << "Align: " << e.what() << std::endl;
    return 1;
  }
}
