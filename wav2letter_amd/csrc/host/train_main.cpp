// train_main.cpp -- `Train train --flagsfile=... [--k=v ...]`: the reference Trainer's command line
// (recipes/slimIPL/src/Train.cpp:110-179: `train [flags]` | `continue [directory] [flags]` | `fork [model] [flags]`)
// over the fl:: surface of include/fl_compat/flashlight.h.
//
// It reads the recipes' own train.cfg / *.arch files UNCHANGED (gflags `--flagsfile`, later flags win), builds
//   network   = fl::pkg::runtime::ModulePlugin(FLAGS_arch).arch(numFeatures, numClasses)   (Train.cpp:390-395)
//   criterion = CTCLoss(scalemode) | ASGLoss(numClasses, scalemode, FLAGS_transdiag)         (:406-410)
//   netoptim / critoptim = initOptimizer(--netoptim / --critoptim: sgd | adagrad | adadelta | adam)                       (:577-582)
// and runs the hot loop of Train.cpp:1454-1804 (forward, criterion, zeroGrad, backward, grads / batch, clipGradNorm,
// critopt->step, netopt->step) with the reference's meters, printing the log line of MyLogger.cpp:40-106
// (`epoch | nupdates | lr | lrcriterion | runtime | bch(ms) | smp(ms) | fwd(ms) | crit-fwd(ms) | bwd(ms) | optim(ms) |
// loss | train-TER | train-WER | ...`) to stdout and to <rundir>/<runname>/001_log, next to 001_config (:644-651).
//
// `Train continue <directory>` / `Train fork <model>` (Train.cpp:124-179, :452-463): the run directory holds NNN_log, NNN_config and
// NNN_model_last.bin (getRunFile, :644-651, :767-790); `continue` looks for the highest NNN_model_last.bin, re-reads the flags
// stored in it (the command line overrides them), restores network, criterion, both optimizers, the update counter and the
// position of every random stream, and goes on as run NNN+1 -- bit for bit where an uninterrupted run would be; `fork` takes
// flags + network + criterion from a model file and starts a fresh run in --rundir.  The container is the documented
// W2LAMD01 layout of wav2letter_amd/checkpoint.py (fl::pkg::runtime::Serializer), not cereal.
//
// Data (Train.cpp:277-339): when --train names list files that exist (relative to --datadir, comma separated), the step consumes
// THEM -- `id path duration transcript` lines, audio decoded on the host (WAV / FLAC / raw PCM: fl_compat/audio.h), MFSC features
// and the per-utterance normalisation on the device, targets from --tokens / --lexicon through fl_compat/text.h (replabels for
// ASG), batches of --batchsize in list order, rank r taking its share of every global batch (partitionByRoundRobin); train-TER /
// train-WER of the log line come from the Viterbi path through tknPrediction2Ltr / tkn2Wrd (Train.cpp:829-872).  Without lists the
// data is SYNTHETIC: LibriSpeech-shaped padded batches (--w2l_synth_frames frames of --filterbanks features, random targets), which
// is exactly what bench.py times.  Not here (out of scope): the decoder (beam search, LM), cereal checkpoints.
// Validation (test(), Train.cpp:874-980): --valid=[tag:]list,... (relative to --datadir; the tag defaults to the path) and
// --validbatchsize (-1: --batchsize) -- at every log line each set goes, unshuffled and shared round-robin among the ranks,
// through the eval-mode network and w2lScore (loss + greedy / Viterbi path in one call); `<tag>-loss | <tag>-TER | <tag>-WER`
// follow train-WER (MyLogger.cpp:60-70), and NNN_model_<tag>.bin is written when a set's WER beats this run's best.  A
// synthetic run ignores --valid.
// slimIPL (the reference file's own purpose; Train.cpp:73-102, :1141-1168, :1214-1333, :1362-1415, :1478-1660, :1786-1841): with
// --unsup_train=list,... (relative to --unsup_datadir) updates after --slimIPL_start interleave supervised batches with batches of
// the unlabelled lists, --slimIPL_sup_updates : --slimIPL_unsup_updates, whose transcripts the TEACHER writes -- the network
// itself or, with --slimIPL_ema, a second network of the same arch that follows it as an exponential moving average after every
// update (fl::ext::emaUpdate: one launch over the parameter arena; NNN_model_last_ema.bin).  --slimIPL_type = naive (label, then
// train) | cache (train on the cached labels, relabel after the update) | pre-cache (relabel before it) | fixed-pre-cache (a cache
// of --slimIPL_fixed_cache_updates batch indices, relabelled with --slimIPL_fixed_cache_update_prob).  The schedule and the caches
// are fl_compat/ipl.h (NNN_model_last_cache<rank>, NNN_model_last_fixed_cache<rank>, written by every rank); only the samples that
// have a label enter the criterion (fl::ext::selectBatch), and an update for which ANY rank has none is skipped on all ranks.
// --slimIPL_dyn_dropout sets the `TR` layers' dropout and layer drop for those updates, --slimIPL_saug a stronger SpecAugment on the
// supervised batches.  Refused: --slimIPL_use_soft (soft labels), --unsup_train on synthetic data.
// Flags of this driver that the reference does not have are prefixed w2l_.
// Data parallelism is the reference's: --enable_distributed --world_rank --world_size --max_devices_per_node
// --rndv_filepath (Train.cpp:188-199; RANK / WORLD_SIZE / LOCAL_WORLD_SIZE of a torchrun-style launcher are read when the
// flags are absent): one process per GPU, fl::CoalescingReducer over RCCL, batch size all-reduced with the gradients.
#include <limits>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <atomic>
#include <fstream>
#include <future>
#include <iostream>
#include <memory>
#include <random>
#include <sstream>
#include <thread>

#include "../../../include/fl_compat/flashlight.h"
#include "../../../include/fl_compat/audio.h"
#include "../../../include/fl_compat/data.h"
#include "../../../include/fl_compat/ipl.h"
#include "../../../include/fl_compat/text.h"
#include "w2l_host.hpp"
#include "list_data.hpp"

using namespace fl;
using namespace fl::pkg::speech;
using namespace w2l::cli;

namespace {

struct Timer {
  double total = 0;
  int n = 0;
  std::chrono::steady_clock::time_point t0;
  void resume() { t0 = std::chrono::steady_clock::now(); }
  void stop() { total += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
  void stopAndIncUnit() { stop(); ++n; }
  double value() const { return n ? total / n : 0.0; }  // seconds per unit, like fl::TimeMeter(true)
  void reset() { total = 0; n = 0; }
};

std::string fmt(const char* f, double v) { char b[64]; snprintf(b, sizeof b, f, v); return b; }
std::string fmti(const char* f, long v) { char b[64]; snprintf(b, sizeof b, f, v); return b; }

int editDistance(const std::vector<int>& a, const std::vector<int>& b) {
  std::vector<int> prev(b.size() + 1), cur(b.size() + 1);
  for (size_t j = 0; j <= b.size(); ++j) prev[j] = (int)j;
  for (size_t i = 1; i <= a.size(); ++i) {
    cur[0] = (int)i;
    for (size_t j = 1; j <= b.size(); ++j)
      cur[j] = std::min({prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1])});
    std::swap(prev, cur);
  }
  return prev[b.size()];
}

// (fileExists / mkdirs / pathJoin / countTokens and ListData, the list files -> padded device batches pipeline: list_data.hpp,
// shared with align_main.cpp)

int usage(const char* exe) {
  std::cerr << "Usage: \n " << exe << " train [flags]\n or " << exe << " continue [directory] [flags]\n or " << exe
            << " fork [directory/model] [flags]" << std::endl;
  return 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc <= 1) return usage(argv[0]);
  const std::string runStatus = argv[1];
  try {
    int first = 2;
    int runIdx = 1;                 // current #runs in this path (Train.cpp:124)
    std::string runPath, reloadPath;
    long startUpdate = 0;
    using Serializer = fl::pkg::runtime::Serializer;
    Serializer::Config reloadCfg;
    auto getRunFile = [](const std::string& name, int idx, const std::string& path) {
      char b[16];
      snprintf(b, sizeof b, "%03d_", idx);
      return pathJoin(path, std::string(b) + name);
    };
    w2l::Flags flags;
    if (runStatus == "continue") {
      if (argc <= 2) return usage(argv[0]);
      runPath = argv[2];
      first = 3;
      while (fileExists(getRunFile("model_last.bin", runIdx, runPath))) ++runIdx;
      if (runIdx == 1) throw std::invalid_argument("continue: no 001_model_last.bin in '" + runPath + "'");
      reloadPath = getRunFile("model_last.bin", runIdx - 1, runPath);
      std::cout << "reload path is " << reloadPath << std::endl;
    } else if (runStatus == "fork") {
      if (argc <= 2) return usage(argv[0]);
      reloadPath = argv[2];
      first = 3;
    } else if (runStatus != "train") {
      return usage(argv[0]);
    }
    if (!reloadPath.empty()) {
      std::string version;
      Serializer::load(reloadPath, version, reloadCfg);
      auto it = reloadCfg.find("gflags");
      if (it == reloadCfg.end()) throw std::invalid_argument("Invalid config loaded from " + reloadPath);
      std::cout << "Reading flags from config file " << reloadPath << std::endl;
      flags = w2l::parseFlagsText(it->second);
      if (runStatus == "continue") {
        auto up = reloadCfg.find("nbupdates");
        if (up == reloadCfg.end()) std::cout << "Did not find #updates to start from, starting from 0." << std::endl;
        else startUpdate = std::stol(up->second);
      }
    }
    // ---- flags: (the checkpoint's,) --flagsfile, then the command line in order (gflags semantics: the last definition wins)
    for (int i = first; i < argc; ++i) {
      w2l::Flags one = w2l::parseFlagsText(argv[i]);
      for (auto& kv : one.kv) flags.kv.push_back(kv);
    }
    w2l::checkFlagDependencies(flags);
    const std::string criterionName = flags.get("criterion", "asg");    // the reference default (FLAGS_criterion)
    const int batch = (int)flags.geti("batchsize", 1);
    const int nFeat = flags.getb("mfcc", false) ? (int)flags.geti("mfcccoeffs", 13) * 3
                      : flags.getb("pow", false) ? (int)flags.geti("framesizems", 25) * 8 + 1 : (int)flags.geti("filterbanks", 40);
    const double lr0 = flags.getd("lr", 1.0), lrcrit0 = flags.getd("lrcrit", 0.0), momentum = flags.getd("momentum", 0.0);
    const double maxgradnorm = flags.getd("maxgradnorm", 0.0);
    const long iters = flags.geti("w2l_synth_updates", flags.geti("iter", 8));
    const long reportiters = flags.geti("reportiters", 0);
    const int T = (int)flags.geti("w2l_synth_frames", 1500);
    const int Lmax = (int)flags.geti("w2l_synth_target_len", criterionName == "ctc" ? 80 : 300);
    const long linseg = flags.geti("linseg", 0);
    const long warmup = flags.geti("warmup", 1);
    const uint64_t seed = (uint64_t)flags.geti("seed", 0);
    // ---- slimIPL flags (Train.cpp:73-102), refused before anything touches the device
    const std::string unsupTrain = flags.get("unsup_train", "");
    if (flags.getb("slimIPL_use_soft", false))
      throw std::invalid_argument("--slimIPL_use_soft=true is not built (soft labels: the reference's branch prints whole tensors per step)");
    SlimIPL::Options iplOpt;
    iplOpt.type = parseIplType(flags.get("slimIPL_type", "naive"));
    iplOpt.supUpdates = flags.geti("slimIPL_sup_updates", 1);
    iplOpt.unsupUpdates = flags.geti("slimIPL_unsup_updates", 3);
    iplOpt.fixedCacheUpdates = flags.geti("slimIPL_fixed_cache_updates", 1000);
    iplOpt.fixedCacheUpdateProb = flags.getd("slimIPL_fixed_cache_update_prob", 1.0);
    const long iplStart = flags.geti("slimIPL_start", 0);
    const double dynDropout = flags.getd("slimIPL_dyn_dropout", -1.0);
    const bool useEma = flags.getb("slimIPL_ema", false);
    const double emaDecay = flags.getd("slimIPL_ema_decay", 0.999);
    if (!(emaDecay >= 0.0 && emaDecay <= 1.0)) throw std::invalid_argument("--slimIPL_ema_decay=" + flags.get("slimIPL_ema_decay") + ": must lie in [0, 1]");
    if (dynDropout >= 1.0) throw std::invalid_argument("--slimIPL_dyn_dropout must be below 1");
    const long plPrintEvery = std::max<long>(1, flags.geti("w2l_ipl_print_every", 100));   // "PL for index" lines (Train.cpp:1383: every 100th update)
    {
      std::string trainLists0 = flags.get("train", "");
      const std::string first0 = trainLists0.substr(0, trainLists0.find(','));
      const bool lists0 = !first0.empty() && trainLists0.find("[DATA_DST]") == std::string::npos && fileExists(pathJoin(flags.get("datadir", ""), first0));
      if (!unsupTrain.empty() && !lists0)
        throw std::invalid_argument("--unsup_train needs --train list files: a synthetic run has no audio to label");
    }

    // ---- number of classes: the token dictionary (+ replabels for ASG, + blank for CTC: Train.cpp:230-251)
    int numClasses = (int)flags.geti("w2l_nlabel", 0);
    if (!numClasses) {
      const std::string tok = pathJoin(flags.get("tokensdir", ""), flags.get("tokens", "tokens.txt"));
      const int n = countTokens(tok);
      if (n <= 0) throw std::invalid_argument("cannot read the token dictionary '" + tok + "' (--tokensdir / --tokens); pass --w2l_nlabel=N for a synthetic run");
      numClasses = n;
      if (criterionName == "asg") numClasses += (int)flags.geti("replabel", 0);
      if (criterionName == "ctc") numClasses += 1;  // blank, appended LAST
    }

    // ---- run directory: NNN_log, NNN_config, NNN_model_last.bin (Train.cpp:644-651, :767)
    if (runStatus != "continue") runPath = pathJoin(flags.get("rundir", ""), flags.get("runname", ""));
    const bool haveRunDir = runStatus == "continue" || (!flags.get("rundir", "").empty() && flags.get("rundir", "") != "[...]");
    std::string gflagsText;   // what `continue` / `fork` read back (the reference serialises its gflags the same way)
    {
      // later definitions win, so the effective value of every flag once, in first-appearance order
      std::vector<std::string> order;
      for (auto& kv : flags.kv) if (std::find(order.begin(), order.end(), kv.first) == order.end()) order.push_back(kv.first);
      for (auto& k : order) if (k != "flagsfile") gflagsText += "--" + k + "=" + flags.get(k) + "\n";
    }
    std::ofstream logFile;

    // ---- network / criterion / optimizers
    const std::string archPath = pathJoin(flags.get("archdir", ""), flags.get("arch", ""));
    if (!fileExists(archPath)) throw std::invalid_argument("arch file / plugin '" + archPath + "' not found (--archdir / --arch)");
    auto scalemode = getCriterionScaleMode(flags.get("onorm", "none"), flags.getb("sqnorm", false));
    std::cout << "Loading architecture file from " << archPath << std::endl;
    std::shared_ptr<fl::Module> network = fl::pkg::runtime::ModulePlugin(archPath).arch(nFeat, numClasses);
    if (flags.getb("fl_amp_use_mixed_precision", false)) {
      setMixedPrecision(network, true);   // bf16 multiplies in the fl::Linear GEMMs, fp32 master weights / criterion
      std::cout << "Mixed precision training enabled (bf16 matrix multiplies, fp32 accumulation and storage)" << std::endl;
      if (flags.getb("w2l_amp_convs", false)) {
        setMixedPrecisionConvolutions(network, true);   // ... and in the wide time convolutions at H == 1 (conv_glu, Transformer front end)
        std::cout << "Mixed precision: the wide time convolutions multiply bf16 operands too (--w2l_amp_convs)" << std::endl;
      }
    }
    std::shared_ptr<SequenceCriterion> criterion;
    if (criterionName == "ctc") criterion = std::make_shared<CTCLoss>(scalemode);
    else if (criterionName == "asg") criterion = std::make_shared<ASGLoss>(numClasses, scalemode, flags.getd("transdiag", 0.0));
    else throw std::invalid_argument("unsupported criterion '" + criterionName + "' (this build: ctc, asg)");
    if (linseg > 0 && criterionName != "asg") throw std::invalid_argument("linseg may only be used with ASG criterion");  // Train.cpp:593
    size_t nparams = 0;
    for (auto& p : network->params()) nparams += (size_t)p.elements();
    std::cout << "[Network] " << network->prettyString() << std::endl;
    std::cout << "[Network Params: " << nparams << "]" << std::endl;
    std::cout << "[Criterion] " << criterion->prettyString() << std::endl;
    // initOptimizer(nets, --netoptim, lr, momentum, weightdecay) (Train.cpp:577-582): sgd, adadelta (librispeech/train_am_transformer_ctc.cfg:23-24)
    // and adagrad (librivox/train_am_transformer_ctc.cfg:25-26) are the ones the BASELINE recipes name
    const double optimrho = flags.getd("optimrho", 0.9), optimepsilon = flags.getd("optimepsilon", 1e-8);
    // adam (joint_training_vox_populi/sh_voxpopuli/pretrain.sh; cpc/Train.cpp:569-580): --adambeta1 --adambeta2 --optimepsilon, and
    // --weightdecay for the network's optimizer alone -- the criterion's gets 0.  The other three leave --weightdecay unread.
    const double adambeta1 = flags.getd("adambeta1", 0.9), adambeta2 = flags.getd("adambeta2", 0.999);
    auto initOptimizer = [&](const std::vector<fl::Variable>& params, const std::string& kind, double lr, double mom, double wd) -> std::shared_ptr<fl::FirstOrderOptimizer> {
      if (kind == "sgd") return std::make_shared<SGDOptimizer>(params, lr, mom, 0.0);
      if (kind == "adagrad") return std::make_shared<fl::AdagradOptimizer>(params, lr);
      if (kind == "adadelta") return std::make_shared<fl::AdadeltaOptimizer>(params, lr, optimrho, optimepsilon);
      if (kind == "adam") return std::make_shared<fl::AdamOptimizer>(params, lr, adambeta1, adambeta2, optimepsilon, wd);
      throw std::invalid_argument("unsupported optimizer '" + kind + "' (this build: sgd, adagrad, adadelta, adam)");
    };
    auto netoptim = initOptimizer(network->params(), flags.get("netoptim", "sgd"), lr0, momentum, flags.getd("weightdecay", 0.0));
    auto critoptim = initOptimizer(criterion->params(), flags.get("critoptim", "sgd"), lrcrit0, 0.0, 0.0);
    std::cout << "[Network Optimizer] " << netoptim->prettyString() << std::endl;
    std::cout << "[Criterion Optimizer] " << critoptim->prettyString() << std::endl;
    // the teacher of slimIPL: the network itself, or with --slimIPL_ema a second network of the same arch (Train.cpp:396-405) --
    // initialised as a copy once the student's parameters are final (below), saved as NNN_model_last_ema.bin
    std::shared_ptr<fl::Module> networkEMA = network;
    if (useEma) {
      networkEMA = fl::pkg::runtime::ModulePlugin(archPath).arch(nFeat, numClasses);
      if (flags.getb("fl_amp_use_mixed_precision", false)) setMixedPrecision(networkEMA, true);
      if (flags.getb("fl_amp_use_mixed_precision", false) && flags.getb("w2l_amp_convs", false)) setMixedPrecisionConvolutions(networkEMA, true);
    }
    // (the file of the averaged network holds the network alone, Train.cpp:776-781: a parameter-free criterion fills the container's slot)
    std::shared_ptr<fl::Module> emaFileCrit = std::make_shared<CTCLoss>(scalemode);
    if (runStatus == "fork") {            // Train.cpp:452-459: network + criterion, fresh optimizers
      std::string version;
      Serializer::Config unused;
      Serializer::load(reloadPath, version, unused, network, criterion);
      fl::pkg::speech::setNetworkStep(network, 0);
      std::cout << "Loaded model " << reloadPath << " for fork" << std::endl;
    } else if (runStatus == "continue") { // Train.cpp:460-467
      std::string version;
      Serializer::Config unused;
      Serializer::load(reloadPath, version, unused, network, criterion, netoptim, critoptim);
      if (useEma) {                       // Train.cpp:469-475
        Serializer::Config unusedEma;
        Serializer::load(getRunFile("model_last_ema.bin", runIdx - 1, runPath), version, unusedEma, networkEMA, emaFileCrit);
      }
      std::cout << "Loaded model for continue training" << std::endl;
    }

    // ---- data parallelism (Train.cpp:188-199, :1078-1079)
    std::shared_ptr<fl::Reducer> reducer;
    if (flags.getb("enable_distributed", false)) {
      auto envi = [](const char* k, long dflt) { const char* v = getenv(k); return v ? atol(v) : dflt; };
      const int worldRank = (int)flags.geti("world_rank", envi("RANK", 0));
      const int worldSize = (int)flags.geti("world_size", envi("WORLD_SIZE", 1));
      fl::pkg::runtime::initDistributed(worldRank, worldSize, (int)flags.geti("max_devices_per_node", envi("LOCAL_WORLD_SIZE", 8)),
                                        flags.get("rndv_filepath", ""));
      reducer = std::make_shared<fl::CoalescingReducer>(1.0, true, true);
      fl::allReduceParameters(network);     // replicas start identical
      fl::allReduceParameters(criterion);
      std::cout << "[Distributed] world rank " << fl::getWorldRank() << " of " << fl::getWorldSize()
                << (flags.get("rndv_filepath", "").rfind("shm:", 0) == 0 ? " (host-memory test collective)" : " (RCCL)") << std::endl;
    }
    if (useEma && runStatus != "continue") fl::ext::emaUpdate(networkEMA, network, 0.0);   // decay 0: a copy of the student
    const bool isMaster = fl::getWorldRank() == 0;
    if (haveRunDir && isMaster) {
      mkdirs(runPath);
      logFile.open(getRunFile("log", runIdx, runPath));
      if (!logFile) throw std::runtime_error("failed to open log file for writing");
      std::ofstream cfg(getRunFile("config", runIdx, runPath));
      cfg << gflagsText;
    }

    // ---- data
    std::string trainLists = flags.get("train", "");
    const std::string dataDir = flags.get("datadir", "");
    std::vector<std::string> listPaths;
    {
      std::istringstream ls(trainLists);
      for (std::string one; std::getline(ls, one, ',');) if (!one.empty()) listPaths.push_back(pathJoin(dataDir, one));
    }
    const bool haveLists = !listPaths.empty() && trainLists.find("[DATA_DST]") == std::string::npos && fileExists(listPaths[0]);
    // list files -> ListData with the train lists' text pipeline (tokens, lexicon, replabel, wordseparator; surround and usewordpiece
    // are read where the paths are turned into words); `which` names the flag in the error messages
    // (validation sets: allowEmpty -- every sample on exactly one rank, the tail included)
    auto loadLists = [&](ListData& d, const std::vector<std::string>& paths, int bsz, const std::string& which, bool allowEmpty) {
      loadListData(d, paths, bsz, which, allowEmpty, flags, criterionName, nFeat, numClasses, seed, dataDir);
    };
    ListData data;
    if (haveLists) {
      loadLists(data, listPaths, batch, "--train", false);
      if (data.mine.empty()) throw std::invalid_argument("this rank has no samples (fewer samples than world_size * batchsize)");
      std::cout << "[Data] " << data.samples.size() << " samples in " << listPaths.size() << " list(s), " << data.mine.size() << " on this rank, "
                << data.batches() << " batches of " << batch << " per epoch; " << nFeat << " MFSC features; " << data.dict.indexSize() << " classes" << std::endl;
    }
    // --unsup_train=list,... relative to --unsup_datadir (Train.cpp:326, :341-361): the same pipeline; the transcript column only
    // serves "PL Quality" (a transcript that cannot be spelled is no error there)
    ListData unsupData;
    std::unique_ptr<SlimIPL> ipl;
    if (!unsupTrain.empty()) {
      const std::string unsupDir = flags.get("unsup_datadir", "");
      std::vector<std::string> up;
      std::istringstream us(unsupTrain);
      for (std::string one; std::getline(us, one, ',');) if (!one.empty()) up.push_back(pathJoin(unsupDir, one));
      unsupData.tolerateTextErrors = true;
      loadListData(unsupData, up, batch, "--unsup_train", false, flags, criterionName, nFeat, numClasses, seed, unsupDir);
      if (unsupData.mine.empty()) throw std::invalid_argument("this rank has no samples of --unsup_train (fewer samples than world_size * batchsize)");
      std::cout << "Unsup batches " << unsupData.batches() << std::endl;
      ipl.reset(new SlimIPL(iplOpt, unsupData.batches(), seed));
    }
    std::cout << "Unsup is in use " << (ipl ? 1 : 0) << std::endl;
    long supDone = startUpdate;   // supervised batches consumed so far = the position in the supervised lists
    if (ipl && runStatus == "continue") {   // Train.cpp:477-545: every rank's text cache (read-only), this rank's fixed cache
      if (iplOpt.type != IplType::Naive) {
        std::cout << "Reading PL cache" << std::endl;
        for (int r = 0; r < fl::getWorldSize(); ++r) {
          const std::string name = getRunFile("model_last_cache", runIdx - 1, runPath) + std::to_string(r);
          const long n = ipl->loadCacheDump(name);
          if (n < 0) std::cout << "Read cache from " << name << "; Skip, file doesn't exist" << std::endl;
          else std::cout << "Read cache from " << name << " with number of samples " << n << std::endl;
        }
        std::cout << "Reading PL cache is done; total size " << ipl->plCacheDump.size() << std::endl;
      }
      if (iplOpt.type == IplType::FixedPreCache) {
        const std::string name = getRunFile("model_last_fixed_cache", runIdx - 1, runPath) + std::to_string(fl::getWorldRank());
        if (!ipl->loadFixedCache(name)) std::cout << "Read fixed cache from " << name << "; Skip, file doesn't exist" << std::endl;
        else std::cout << "Reading PL fixed cache is done; total size " << ipl->fixedCache.size() << std::endl;
      }
    }
    bool iplNeedEpoch = true;   // the next slimIPL step opens a pass over the supervised lists (SlimIPL::startEpoch)
    {
      auto st = reloadCfg.find("w2l_ipl_state");
      auto sd = reloadCfg.find("w2l_ipl_sup_batches");
      if (ipl && runStatus == "continue" && st != reloadCfg.end() && sd != reloadCfg.end()) {
        ipl->setState(st->second);   // the schedule goes on where the saved run stopped
        supDone = std::stol(sd->second);
        iplNeedEpoch = supDone > 0 && supDone % std::max<long>(1, data.batches()) == 0;
      } else if (ipl) {
        ipl->begin();
      }
    }
    // --valid=[tag:]list,... (parseValidSets, Train.cpp:232-233, :362-370): each set is scored in list order (no shuffle), every
    // rank its round-robin share, the short last batch included; --validbatchsize = -1: --batchsize
    struct ValidSet {
      std::string tag;
      ListData data;
      double bestWer = std::numeric_limits<double>::infinity();
      double loss = 0, ter = 0, wer = 0;
    };
    std::vector<std::unique_ptr<ValidSet>> validSets;
    if (!flags.get("valid", "").empty()) {
      if (!haveLists) {
        std::cout << "[Valid] --valid is ignored: no --train list files (synthetic data)" << std::endl;
      } else {
        const long vb = flags.geti("validbatchsize", -1);
        const int validBatch = vb == -1 ? batch : (int)vb;
        if (validBatch <= 0) throw std::invalid_argument("--validbatchsize must be positive (or -1: --batchsize)");
        std::istringstream vs(flags.get("valid"));
        for (std::string one; std::getline(vs, one, ',');) {
          if (one.empty()) continue;
          auto v = std::make_unique<ValidSet>();
          const size_t colon = one.find(':');
          const std::string path = colon == std::string::npos ? one : one.substr(colon + 1);
          v->tag = colon == std::string::npos ? one : one.substr(0, colon);
          loadLists(v->data, {pathJoin(dataDir, path)}, validBatch, "--valid", true);
          std::cout << "[Valid] " << v->tag << ": " << v->data.samples.size() << " samples, " << v->data.mine.size() << " on this rank, "
                    << v->data.batches() << " batches of " << validBatch << std::endl;
          validSets.push_back(std::move(v));
        }
      }
    }
    std::mt19937_64 rng(2026 + seed + 7919ull * (uint64_t)fl::getWorldRank());   // every rank draws its own shard of the (synthetic) minibatch
    std::normal_distribution<float> gauss(0.f, 1.f);
    // --w2l_synth_emulate_world=W (one process): the batch is the concatenation of the shards W ranks of --batchsize / W would
    // draw -- the reference run a data-parallel run of W ranks must reproduce (tests)
    const int emuWorld = (int)flags.geti("w2l_synth_emulate_world", 1);
    if (emuWorld < 1 || batch % emuWorld) throw std::invalid_argument("--w2l_synth_emulate_world must divide --batchsize");
    std::vector<std::mt19937_64> emuRng;
    std::vector<std::normal_distribution<float>> emuGauss((size_t)emuWorld, std::normal_distribution<float>(0.f, 1.f));
    for (int r = 0; r < emuWorld; ++r) emuRng.emplace_back(2026 + seed + 7919ull * (uint64_t)r);
    const int nTok = criterionName == "ctc" ? numClasses - 1 : std::max(1, numClasses - (int)flags.geti("replabel", 0));
    std::vector<float> hx((size_t)batch * nFeat * T);
    std::vector<int> ht((size_t)batch * Lmax);
    const long synthPool = flags.geti("w2l_synth_pool", 0);
    std::vector<float> hxPool;
    std::vector<int> htPool;
    if (runStatus == "continue") {   // the sample stream goes on where the saved run stopped (per rank)
      auto it = reloadCfg.find("w2l_data_rng." + std::to_string(fl::getWorldRank()));
      if (it != reloadCfg.end()) { std::istringstream is(it->second); is >> rng >> gauss; }
    }

    // ---- meters (MyLogger.cpp:40-106)
    Timer runtime, timer, sampletimer, fwdtimer, critfwdtimer, bwdtimer, optimtimer;
    double lossSum = 0;
    long lossN = 0, editErr = 0, editLen = 0, tszTotal = 0, tszMax = 0, nsamples = 0, nbatches = 0;
    fl::EditDistanceMeter wordMeter;   // list data: train-WER over words
    double lossUnsupSum = 0;           // meters.trainUnsup (MyLogger.cpp:99-106)
    long lossUnsupN = 0;
    fl::EditDistanceMeter tknUnsupMeter, wordUnsupMeter;
    long framesTotal = 0;              // list data: padded input frames consumed (avg-isz, hrs)
    runtime.resume();
    network->train();
    criterion->train();
    const bool clampCrit = true;

    auto logStatus = [&](long epoch, long nupdates, double lr, double lrcrit) {
      runtime.stop();
      std::ostringstream s;
      auto item = [&](const std::string& k, const std::string& v) { s << (s.tellp() > 0 ? " | " : "") << k << ": " << v; };
      const int rt = (int)runtime.total;
      char rtb[32];
      snprintf(rtb, sizeof rtb, "%02d:%02d:%02d", rt / 3600, (rt / 60) % 60, rt % 60);
      item("epoch", fmti("%8ld", epoch));
      item("nupdates", fmti("%12ld", nupdates));
      item("lr", fmt("%4.6lf", lr));
      item("lrcriterion", fmt("%4.6lf", lrcrit));
      item("runtime", rtb);
      item("bch(ms)", fmt("%.2f", timer.value() * 1000));
      item("smp(ms)", fmt("%.2f", sampletimer.value() * 1000));
      item("fwd(ms)", fmt("%.2f", fwdtimer.value() * 1000));
      item("crit-fwd(ms)", fmt("%.2f", critfwdtimer.value() * 1000));
      item("bwd(ms)", fmt("%.2f", bwdtimer.value() * 1000));
      item("optim(ms)", fmt("%.2f", optimtimer.value() * 1000));
      item("loss", fmt("%10.5f", lossN ? lossSum / lossN : 0.0));
      const double ter = editLen ? 100.0 * editErr / editLen : 0.0;
      item("train-TER", fmt("%5.2f", ter));
      item("train-WER", fmt("%5.2f", haveLists ? wordMeter.value() : ter));  // synthetic targets: every token is its own word
      for (auto& v : validSets) {   // MyLogger.cpp:60-70
        item(v->tag + "-loss", fmt("%10.5f", v->loss));
        item(v->tag + "-TER", fmt("%5.2f", v->ter));
        item(v->tag + "-WER", fmt("%5.2f", v->wer));
      }
      const double framesPerSample = haveLists && nsamples ? (double)framesTotal / nsamples : T;
      item("avg-isz", fmti("%03ld", (long)framesPerSample));
      item("avg-tsz", fmti("%03ld", nsamples ? tszTotal / nsamples : 0));
      item("max-tsz", fmti("%03ld", tszMax));
      item("avr-batchsz", fmt("%7.2f", nbatches ? (double)nsamples / nbatches : 0.0));
      const double audioSec = nsamples * framesPerSample * flags.getd("framestridems", 10) / 1000.0;
      item("hrs", fmt("%7.2f", audioSec / 3600.0));
      const double timeTaken = timer.value() * nbatches;
      item("thrpt(sec/sec)", timeTaken > 0 ? fmt("%.2f", audioSec / timeTaken) : std::string("n/a"));
      std::time_t now = std::time(nullptr);
      char ts[64];
      std::strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S", std::localtime(&now));
      item("timestamp", ts);
      if (ipl) {   // MyLogger.cpp:99-106
        item("loss Unsup", fmt("%10.5f", lossUnsupN ? lossUnsupSum / lossUnsupN : 0.0));
        item("train-TER Unsup", fmt("%5.2f", tknUnsupMeter.value()));
        item("train-WER Unsup", fmt("%5.2f", wordUnsupMeter.value()));
      }
      std::cout << s.str() << std::endl;
      if (logFile.is_open()) logFile << s.str() << std::endl;
      runtime.resume();
    };

    const long batchesPerEpoch = haveLists ? data.batches() : std::max<long>(1, flags.geti("w2l_synth_batches_per_epoch", iters));
    const long lrDecay = flags.geti("lr_decay", std::numeric_limits<int>::max());
    const long lrDecayStep = std::max<long>(1, flags.geti("lr_decay_step", std::numeric_limits<int>::max()));
    // --saug_start_update (Train.cpp:1026-1048): SpecAugment on the features from that update on (archs without a SAUG line)
    const long saugStart = flags.geti("saug_start_update", -1);
    std::shared_ptr<fl::SpecAugment> saug;
    if (saugStart >= 0)
      saug = std::make_shared<fl::SpecAugment>((int)flags.geti("filterbanks", 40), (int)flags.geti("saug_fmaskf", 27), (int)flags.geti("saug_fmaskn", 2),
                                               (int)flags.geti("saug_tmaskt", 100), (float)flags.getd("saug_tmaskp", 1.0), (int)flags.geti("saug_tmaskn", 2));
    if (saug) std::cout << "[SpecAugment from update " << saugStart << "] " << saug->prettyString() << std::endl;
    if (saug && runStatus == "continue") {
      auto it = reloadCfg.find("w2l_saug_calls");
      if (it != reloadCfg.end()) saug->setCalls((uint32_t)std::stoul(it->second));
    }
    // --slimIPL_saug (Train.cpp:1052-1076): a stronger augmentation of the SUPERVISED batches -- one frequency mask more, half as
    // many time masks again; the unsupervised batches keep the one above (saugUnsup)
    std::shared_ptr<fl::SpecAugment> saugSup = saug;
    if (saug && flags.getb("slimIPL_saug", false)) {
      saugSup = std::make_shared<fl::SpecAugment>((int)flags.geti("filterbanks", 40), (int)flags.geti("saug_fmaskf", 27), (int)flags.geti("saug_fmaskn", 2) + 1,
                                                  (int)flags.geti("saug_tmaskt", 100), (float)flags.getd("saug_tmaskp", 1.0),
                                                  (int)((double)flags.geti("saug_tmaskn", 2) * 1.5));
      std::cout << "[SpecAugment of the supervised batches] " << saugSup->prettyString() << std::endl;
      auto it = reloadCfg.find("w2l_saug_sup_calls");
      if (runStatus == "continue" && it != reloadCfg.end()) saugSup->setCalls((uint32_t)std::stoul(it->second));
    }

    // ---- checkpoints (saveModels, Train.cpp:718-790): NNN_model_last.bin after every epoch of the run and at its end
    auto saveModels = [&](long epoch, long totalUpdates) {
      if (!haveRunDir) return;
      if (ipl && iplOpt.type != IplType::Naive) {   // Train.cpp:719-746: by every rank
        mkdirs(runPath);
        ipl->saveCache(getRunFile("model_last_cache", runIdx, runPath) + std::to_string(fl::getWorldRank()));
        ipl->saveFixedCache(getRunFile("model_last_fixed_cache", runIdx, runPath) + std::to_string(fl::getWorldRank()));
      }
      // every rank's sample-stream position travels in rank 0's file: the others hand theirs over through the run directory
      std::ostringstream rs;
      rs << rng << " " << gauss;
      const std::string mine = getRunFile("rng." + std::to_string(fl::getWorldRank()), runIdx, runPath);
      if (!isMaster) { std::ofstream f(mine); f << rs.str(); }
      if (fl::getWorldSize() > 1) fl::barrier();
      if (!isMaster) {
        if (flags.getb("w2l_save_all_ranks", false)) {   // tests: the replica of a rank other than 0 (the replicas must stay in step)
          mkdirs(runPath);
          Serializer::Config rc;
          rc["nbupdates"] = std::to_string(totalUpdates);
          Serializer::save(getRunFile("model_last.bin.rank" + std::to_string(fl::getWorldRank()), runIdx, runPath), "0.1", rc, network, criterion,
                           netoptim, critoptim);
        }
        return;
      }
      Serializer::Config config;
      config["gflags"] = gflagsText;
      config["epoch"] = std::to_string(epoch);
      config["nbupdates"] = std::to_string(totalUpdates);
      config["runIdx"] = std::to_string(runIdx);
      config["w2l_data_rng.0"] = rs.str();
      for (int r = 1; r < fl::getWorldSize(); ++r) {
        std::ifstream f(getRunFile("rng." + std::to_string(r), runIdx, runPath));
        std::stringstream b;
        b << f.rdbuf();
        config["w2l_data_rng." + std::to_string(r)] = b.str();
      }
      if (saug) config["w2l_saug_calls"] = std::to_string(saug->calls());
      if (saugSup != saug) config["w2l_saug_sup_calls"] = std::to_string(saugSup->calls());
      if (ipl) {   // the schedule's position (the draws are the same on every rank)
        config["w2l_ipl_state"] = ipl->state();
        config["w2l_ipl_sup_batches"] = std::to_string(supDone);
      }
      Serializer::save(getRunFile("model_last.bin", runIdx, runPath), "0.1", config, network, criterion, netoptim, critoptim);
      if (useEma) Serializer::save(getRunFile("model_last_ema.bin", runIdx, runPath), "0.1", Serializer::Config(), networkEMA, emaFileCrit, nullptr, nullptr);
    };

    // ---- validation (test(), Train.cpp:874-980): every --valid set through the eval-mode network and w2lScore (one call for the
    // loss and the Viterbi path; a plan and workspaces of their own, so the training steps around it compute what they would
    // without it); the sums are all-reduced exactly, so every rank holds the global loss / TER / WER
    auto runValid = [&]() {
      if (validSets.empty()) return;
      network->eval();
      criterion->eval();
      const bool wp = flags.getb("usewordpiece", false);
      const std::string surround = flags.get("surround", "");
      for (auto& v : validSets) {
        ListData& d = v->data;
        double lossSum = 0;
        long n = 0;
        fl::EditDistanceMeter letters, words;   // TER over the letters of tknPrediction2Ltr / tknTarget2Ltr, WER over tkn2Wrd (evalOutput)
        const long nb = d.batches();
        for (long k = 0; k < nb; ++k) {
          af::array feats;
          std::vector<float> sizes;
          std::vector<int> vt;
          int vL = 1, vT = 0;
          const int vB = d.get(k, k + 1 < nb ? k + 1 : 0, feats, vt, vL, sizes, vT);
          af::array inSizes(af::dim4(1, (af::dim_t)sizes.size()), sizes.data());
          auto out = network->forward({fl::input(feats), fl::noGrad(inSizes)}).front();
          fl::Variable tgt(af::array(af::dim4(vL, vB), vt.data()), false);
          auto sc = w2lScore(*criterion, out, tgt);
          const int To = (int)out.dims(1);
          std::vector<float> hl((size_t)vB);
          std::vector<int> path((size_t)vB * To);
          sc.first.host(hl.data());
          sc.second.host(path.data());
          for (int b = 0; b < vB; ++b) {
            lossSum += hl[(size_t)b];
            ++n;
            std::vector<int> ref;
            for (int i = 0; i < vL && vt[(size_t)b * vL + i] >= 0; ++i) ref.push_back(vt[(size_t)b * vL + i]);
            std::vector<int> pv(path.begin() + (size_t)b * To, path.begin() + (size_t)(b + 1) * To);
            const auto hl = tknPrediction2Ltr(pv, d.dict, criterionName, surround, d.replabel, wp, d.wordsep);
            const auto rl = tknTarget2Ltr(ref, d.dict, criterionName, surround, d.replabel, wp, d.wordsep);
            letters.add(hl, rl);
            words.add(tkn2Wrd(hl, d.wordsep), tkn2Wrd(rl, d.wordsep));
          }
        }
        double sums[6] = {lossSum, (double)n, (double)letters.errors(), (double)letters.length(), (double)words.errors(), (double)words.length()};
        if (fl::getWorldSize() > 1) {
          // the collective sums f32: every rank puts its six doubles, each as three floats that add up to it exactly, into a slot of
          // its own (zeros elsewhere), so the sum hands every rank every rank's numbers unrounded; they are added in double, in
          // rank order -- the same exact global numbers on every rank
          const int W = fl::getWorldSize(), R = fl::getWorldRank();
          std::vector<float> g((size_t)W * 6 * 3, 0.f);
          for (int i = 0; i < 6; ++i) {
            float* q = g.data() + ((size_t)R * 6 + i) * 3;
            const double x = sums[i];
            q[0] = (float)x;
            if (std::isfinite(x)) {
              const double r = x - (double)q[0];
              q[1] = (float)r;
              q[2] = (float)(r - (double)q[1]);
            }
          }
          af::array a(af::dim4((af::dim_t)g.size()), g.data());
          fl::allReduce(a);
          a.host(g.data());
          for (int i = 0; i < 6; ++i) {
            sums[i] = 0;
            for (int r = 0; r < W; ++r) {
              const float* q = g.data() + ((size_t)r * 6 + i) * 3;
              sums[i] += ((double)q[0] + (double)q[1]) + (double)q[2];
            }
          }
        }
        v->loss = sums[1] > 0 ? sums[0] / sums[1] : 0.0;
        v->ter = sums[3] > 0 ? 100.0 * sums[2] / sums[3] : 0.0;
        v->wer = sums[5] > 0 ? 100.0 * sums[4] / sums[5] : 0.0;
      }
      network->train();
      criterion->train();
    };
    // NNN_model_<tag>.bin whenever a set's WER is below the best of this run ('/' in the tag -> '#'; Train.cpp:783-800)
    auto saveBestValid = [&](long epoch, long totalUpdates) {
      for (auto& v : validSets) {
        if (!(v->wer < v->bestWer)) continue;
        v->bestWer = v->wer;
        if (!haveRunDir || !isMaster) continue;
        std::string clean = v->tag;
        std::replace(clean.begin(), clean.end(), '/', '#');
        std::ostringstream rs;
        rs << rng << " " << gauss;
        Serializer::Config config;
        config["gflags"] = gflagsText;
        config["epoch"] = std::to_string(epoch);
        config["nbupdates"] = std::to_string(totalUpdates);
        config["runIdx"] = std::to_string(runIdx);
        config["w2l_data_rng.0"] = rs.str();
        if (saug) config["w2l_saug_calls"] = std::to_string(saug->calls());
        Serializer::save(getRunFile("model_" + clean + ".bin", runIdx, runPath), "0.1", config, network, criterion, netoptim, critoptim);
      }
    };

    // ---- labelling with the teacher (predictPLCommon, Train.cpp:1362-1407): teacher and criterion in eval mode, the forward on the
    // UN-augmented features and on the eval-mode plan of the teacher (a plan and an arena of its own, as runValid's: no training
    // buffer is touched, no step counter, dropout seed or SpecAugment call counter moves), Viterbi path -> letters -> words, joined
    // with spaces.  "PL Quality" is the WER of the labels against the list's transcript column, summed over the ranks.
    auto predictPL = [&](const af::array& feats, const af::array& inSizes, const std::vector<const ListSample*>& smp, long curBatch) {
      networkEMA->eval();
      criterion->eval();
      auto out = networkEMA->forward({fl::input(feats), fl::noGrad(inSizes)}).front();
      const int To = (int)out.dims(1), pB = (int)out.dims(2);
      std::vector<int> path((size_t)pB * To);
      criterion->viterbiPath(out.array(), inSizes).host(path.data());
      networkEMA->train();
      criterion->train();
      const bool print = isMaster && curBatch % plPrintEvery == 0;
      if (print) {
        std::cout << "PL for samples ";
        for (size_t b = 0; b < smp.size(); ++b) std::cout << (b ? "," : "") << smp[b]->id;
        std::cout << std::endl;
      }
      const bool wp = flags.getb("usewordpiece", false);
      fl::EditDistanceMeter quality;
      std::vector<std::string> texts;
      for (int b = 0; b < pB; ++b) {
        std::vector<int> pv(path.begin() + (size_t)b * To, path.begin() + (size_t)(b + 1) * To);
        const auto words = tkn2Wrd(tknPrediction2Ltr(pv, unsupData.dict, criterionName, flags.get("surround", ""), unsupData.replabel, wp, unsupData.wordsep),
                                   unsupData.wordsep);
        std::string text;
        for (size_t w = 0; w < words.size(); ++w) text += (w ? " " : "") + words[w];
        if (print) std::cout << "PL for index " << b << ": " << text << std::endl;
        quality.add(words, smp[(size_t)b]->transcript);
        texts.push_back(text);
      }
      float q[2] = {(float)quality.errors(), (float)quality.length()};   // (word counts of a batch: exact in f32)
      if (fl::getWorldSize() > 1) {
        af::array a(af::dim4(2), q);
        fl::allReduce(a);
        a.host(q);
      }
      if (isMaster) std::cout << "PL Quality for Batch " << curBatch << " : " << (q[1] > 0 ? 100.0 * (double)q[0] / (double)q[1] : 0.0) << std::endl;
      return texts;
    };
    // --slimIPL_dyn_dropout (Train.cpp:1465-1469): the student's `TR` layers from the first slimIPL update on (the teacher labels
    // in eval mode anyway)
    bool dynDropoutSet = false;

    // ---- the hot loop (Train.cpp:1454-1804)
    double lr = lr0, lrcrit = lrcrit0;
    for (long curBatch = startUpdate + 1; curBatch <= iters; ++curBatch) {
      // learning rate (Train.cpp:1170-1175, :1334-1348): 0.5^(epoch steps after --lr_decay) * (cosine | gamma^(batch / stepsize)) * warm-up;
      // an epoch of the synthetic run is --w2l_synth_batches_per_epoch updates (default: the whole run is epoch 1)
      const long curEpoch = 1 + supDone / batchesPerEpoch;   // (without slimIPL every update is supervised: supDone == curBatch - 1)
      const long afterDecay = curEpoch - lrDecay;
      const double lrDecayScale = std::pow(0.5, afterDecay < 0 ? 0.0 : (double)(1 + afterDecay / lrDecayStep));
      const double lrScheduleScale = flags.getb("lrcosine", false)
                                         ? std::cos((double)curBatch / (double)iters * std::acos(-1.0) / 2.0)
                                         : std::pow(flags.getd("gamma", 1.0), (double)curBatch / flags.getd("stepsize", 1e18));
      const double sched = lrDecayScale * lrScheduleScale * std::min((double)curBatch / std::max<long>(1, warmup), 1.0);
      lr = lr0 * sched;
      lrcrit = lrcrit0 * sched;
      netoptim->setLr(lr);
      critoptim->setLr(lrcrit);

      // slimIPL (Train.cpp:1214-1333): a supervised or an unsupervised step, and which unsupervised batch
      bool isSup = true, haveBatch = true;
      SlimIPL::Unsup us;
      if (ipl && curBatch > iplStart) {
        if (!dynDropoutSet && dynDropout >= 0) {
          auto seq = std::dynamic_pointer_cast<fl::Sequential>(network);
          if (!seq) throw std::invalid_argument("--slimIPL_dyn_dropout needs a network built from an arch file or layer objects");
          seq->setTransformerDropout(dynDropout, dynDropout);
          dynDropoutSet = true;
        }
        if (iplNeedEpoch) { ipl->startEpoch(); iplNeedEpoch = false; }
        isSup = ipl->nextIsSup();
        if (!isSup) us = ipl->nextUnsup();
        ipl->advanceOrder();
        haveBatch = isSup || us.trainBatch >= 0;
      }
      timer.resume();
      sampletimer.resume();
      int curB = batch, curT = T, curL = Lmax;   // this batch's shape (list data: per batch)
      fl::Variable input;
      af::array inputSizes, cleanFeats;   // cleanFeats: the features before SpecAugment (what the teacher labels)
      std::vector<const ListSample*> unsupSamples;
      if (haveLists && !isSup) {
        if (haveBatch) {
          std::vector<float> sizes;
          curB = unsupData.get(us.trainBatch, -1, cleanFeats, ht, curL, sizes, curT);
          unsupSamples = unsupData.samplesOf(us.trainBatch);
          input = fl::input(cleanFeats);
          inputSizes = af::array(af::dim4(1, (af::dim_t)sizes.size()), sizes.data());
          std::cout << "Unsup batch " << curBatch << " | " << us.position << " | " << curT << " " << nFeat << " 1 " << curB;
          if (iplOpt.type == IplType::FixedPreCache) std::cout << " update cache " << (us.relabel ? 1 : 0);
          std::cout << std::endl;
        } else {
          curB = 0;
          std::cout << "Skip usage of unsup batch as fixed cache is not ready " << curBatch << std::endl;
        }
      } else if (haveLists) {
        af::array feats;
        std::vector<float> sizes;
        curB = data.get(data.batchOfUpdate(supDone + 1), data.batchOfUpdate(supDone + 2), feats, ht, curL, sizes, curT);
        if (ipl) std::cout << "Sup batch " << curBatch << " | " << supDone % batchesPerEpoch << " | " << curT << " " << nFeat << " 1 " << curB << std::endl;
        for (int b = 0; b < curB; ++b) {
          long len = 0;
          while (len < curL && ht[(size_t)b * curL + len] >= 0) ++len;
          tszTotal += len;
          tszMax = std::max<long>(tszMax, len);
        }
        input = fl::input(feats);
        inputSizes = af::array(af::dim4(1, (af::dim_t)sizes.size()), sizes.data());   // curB sizes + the padded length
        if (curBatch <= 2 && !flags.get("w2l_dump_features", "").empty()) {   // debugging aid: [B][NFEAT][T] float32 of the first two batches
          std::vector<float> hf((size_t)feats.elements());
          feats.host(hf.data());
          std::ofstream df(flags.get("w2l_dump_features") + "." + std::to_string(curBatch), std::ios::binary);
          const int hd[3] = {curB, nFeat, curT};
          df.write((const char*)hd, sizeof hd);
          df.write((const char*)hf.data(), (std::streamsize)(hf.size() * 4));
        }
      } else {
      // --w2l_synth_pool=K: K batches are drawn once (before the first timed update) and update u trains on batch (u - 1) % K --
      // what a prefetching loader hides in a real run; the default draws every batch inside smp(ms) (3.8 M normal deviates)
      auto draw = [&](float* hxd, int* htd) {
        const int shard = batch / emuWorld;
        for (int r = 0; r < emuWorld; ++r) {   // (emuWorld = 1: this rank's own stream)
          auto& rg = emuWorld > 1 ? emuRng[(size_t)r] : rng;
          auto& gs = emuWorld > 1 ? emuGauss[(size_t)r] : gauss;
          float* hxr = hxd + (size_t)r * shard * nFeat * T;
          for (size_t k = 0; k < (size_t)shard * nFeat * T; ++k) hxr[k] = gs(rg);
          for (int bb = 0; bb < shard; ++bb) {
            const int b = r * shard + bb;
            const int lo = criterionName == "ctc" ? 20 : 60;
            const int len = lo + (int)(rg() % (uint64_t)std::max(1, Lmax - lo + 1));
            int prev = -1;
            for (int i = 0; i < Lmax; ++i) {
              int y = -1;
              if (i < len) {
                y = (int)(rg() % (uint64_t)nTok);
                if (criterionName == "asg" && y == prev) y = (y + 1) % nTok;  // replabel convention: no identical neighbours
                prev = y;
              }
              htd[(size_t)b * Lmax + i] = y;
            }
          }
        }
      };
      if (synthPool > 0) {
        if (hxPool.empty()) {
          sampletimer.stop(); timer.stop();
          hxPool.resize((size_t)synthPool * hx.size());
          htPool.resize((size_t)synthPool * ht.size());
          for (long k = 0; k < synthPool; ++k) draw(hxPool.data() + (size_t)k * hx.size(), htPool.data() + (size_t)k * ht.size());
          timer.resume(); sampletimer.resume();
        }
        const size_t slot = (size_t)((curBatch - 1) % synthPool);
        std::memcpy(hx.data(), hxPool.data() + slot * hx.size(), hx.size() * sizeof(float));
        std::memcpy(ht.data(), htPool.data() + slot * ht.size(), ht.size() * sizeof(int));
      } else {
        draw(hx.data(), ht.data());
      }
      for (int b = 0; b < batch; ++b) {
        long len = 0;
        while (len < Lmax && ht[(size_t)b * Lmax + len] >= 0) ++len;
        tszTotal += len;
        tszMax = std::max<long>(tszMax, len);
      }
      input = fl::input(af::array(af::dim4(T, nFeat, 1, batch), hx.data()));
      inputSizes = af::constant(T, af::dim4(1, batch));
      }
      if (saug && curBatch >= saugStart && haveBatch) input = (isSup ? saugSup : saug)->forward({input}).front();   // Train.cpp:1453-1461
      af::sync();
      sampletimer.stopAndIncUnit();

      // forward
      fwdtimer.resume();
      fl::Variable output, critInput, target;
      if (haveBatch) output = network->forward({input, fl::noGrad(inputSizes)}).front();
      std::vector<std::string> unsupIds, plToSave;   // pre-cache: labels taken before the update, stored after it (Train.cpp:1786-1788)
      bool savePl = false;
      if (isSup) {
        critInput = output;
        target = fl::Variable(af::array(af::dim4(curL, curB), ht.data()), false);
      } else {   // Train.cpp:1478-1649: which samples have a label, and what the teacher labels before the update
        std::vector<int> rows;
        std::vector<std::string> texts;
        for (auto* q : unsupSamples) unsupIds.push_back(q->id);
        if (iplOpt.type == IplType::Naive) {
          texts = predictPL(cleanFeats, inputSizes, unsupSamples, curBatch);
          for (int b = 0; b < curB; ++b) rows.push_back(b);
        } else {
          if (haveBatch) {
            auto l = ipl->labelled(unsupIds);
            for (auto& id : l.reused) std::cout << "Reuse extra loaded cache for sample " << id << " for batch " << curBatch << std::endl;
            rows = l.rows;
            texts = l.texts;
            if (ipl->labelBeforeUpdate(rows.size())) {
              plToSave = predictPL(cleanFeats, inputSizes, unsupSamples, curBatch);
              savePl = true;
            }
          }
          if (us.labelNext >= 0) {   // fixed-pre-cache: the next batch of the walk goes into the cache
            af::array nf;
            std::vector<float> ns;
            std::vector<int> nt;
            int nL = 1, nT = 0;
            unsupData.get(us.labelNext, -1, nf, nt, nL, ns, nT);
            const auto smp = unsupData.samplesOf(us.labelNext);
            std::vector<std::string> ids;
            for (auto* q : smp) ids.push_back(q->id);
            ipl->store(ids, predictPL(nf, af::array(af::dim4(1, (af::dim_t)ns.size()), ns.data()), smp, curBatch));
          }
        }
        if (!rows.empty()) {
          // text -> target through the transform of the list reader's transcript column (an empty text: an empty target)
          std::vector<std::vector<int>> tr;
          curL = 1;
          for (auto& text : texts) {
            std::vector<std::string> words;
            std::istringstream ws(text);
            for (std::string w; ws >> w;) words.push_back(w);
            tr.push_back(targetIndices(words, unsupData.lexicon, unsupData.dict, criterionName, unsupData.replabel, unsupData.wordsep));
            curL = std::max<int>(curL, (int)tr.back().size());
            tszTotal += (long)tr.back().size();
            tszMax = std::max<long>(tszMax, (long)tr.back().size());
          }
          ht.assign(rows.size() * (size_t)curL, -1);
          for (size_t r = 0; r < tr.size(); ++r) std::copy(tr[r].begin(), tr[r].end(), ht.begin() + r * (size_t)curL);
          curB = (int)rows.size();   // totalBatchSize counts the samples that have a label
          critInput = fl::ext::selectBatch(output, rows);
          target = fl::Variable(af::array(af::dim4(curL, curB), ht.data()), false);
        } else {
          curB = 0;
          std::cout << "Skip unsupervised part of data as PL are not available yet" << std::endl;
        }
      }
      // Train.cpp:1651-1660: the update happens only if EVERY rank has something to train on
      bool doUpdate = !critInput.isempty();
      if (ipl && fl::getWorldSize() > 1) {
        const float mine = doUpdate ? 1.f : 0.f;
        af::array du(af::dim4(1), &mine);
        fl::allReduce(du);
        doUpdate = du.scalar<float>() >= (float)fl::getWorldSize();
      }
      af::sync();
      if (!doUpdate) {
        fwdtimer.stop();
      } else {
        critfwdtimer.resume();
        auto loss = criterion->forward({critInput, target}).front();
        af::sync();
        fwdtimer.stopAndIncUnit();
        critfwdtimer.stopAndIncUnit();
        std::vector<float> hl((size_t)curB);
        loss.host(hl.data());
        for (float v : hl) {
          if (!std::isfinite(v)) {   // LOG(FATAL), Train.cpp:1686-1698
            std::ostringstream m;
            m << "Loss has NaN values (update " << curBatch << ", per-utterance losses:";
            for (float q : hl) m << " " << q;
            std::vector<float> he((size_t)critInput.elements());
            critInput.array().host(he.data());
            float mx = 0.f;
            size_t bad = 0;
            for (float q : he) { if (std::isfinite(q)) mx = std::max(mx, std::fabs(q)); else ++bad; }
            m << "; emissions: max |x| " << mx << ", " << bad << " non-finite of " << he.size() << ")";
            throw std::runtime_error(m.str());
          }
          if (isSup) { lossSum += v; ++lossN; }
          else { lossUnsupSum += v; ++lossUnsupN; }
        }
        if (reportiters > 0 && curBatch % reportiters == 0) {  // token error of the Viterbi path (evalOutput, Train.cpp:1699-1716)
          std::vector<int> path((size_t)curB * critInput.dims(1));
          criterion->viterbiPath(critInput.array()).host(path.data());
          const int To = (int)critInput.dims(1);
          for (int b = 0; b < curB; ++b) {
            std::vector<int> hyp, ref;
            int prev = -1;
            for (int t = 0; t < To; ++t) {
              const int y = path[(size_t)b * To + t];
              if (y != prev && !(criterionName == "ctc" && y == numClasses - 1)) hyp.push_back(y);
              prev = y;
            }
            for (int i = 0; i < curL && ht[(size_t)b * curL + i] >= 0; ++i) ref.push_back(ht[(size_t)b * curL + i]);
            if (isSup) {
              editErr += editDistance(hyp, ref);
              editLen += (long)ref.size();
            } else {
              tknUnsupMeter.add(hyp, ref);
            }
            if (haveLists) {   // words: path -> letters (replabels undone, blank dropped) -> split at the word separator (Train.cpp:829-872)
              std::vector<int> pv(path.begin() + (size_t)b * To, path.begin() + (size_t)(b + 1) * To);
              const bool wp = flags.getb("usewordpiece", false);
              auto hw = tkn2Wrd(tknPrediction2Ltr(pv, data.dict, criterionName, flags.get("surround", ""), data.replabel, wp, data.wordsep), data.wordsep);
              auto rw = tkn2Wrd(tknTarget2Ltr(ref, data.dict, criterionName, flags.get("surround", ""), data.replabel, wp, data.wordsep), data.wordsep);
              (isSup ? wordMeter : wordUnsupMeter).add(hw, rw);
            }
          }
        }

        // backward
        bwdtimer.resume();
        netoptim->zeroGrad();
        critoptim->zeroGrad();
        loss.backward();
        if (reducer) {   // Train.cpp:1721-1735
          for (auto& p : network->params()) {
            if (!p.isGradAvailable()) p.addGrad(fl::Variable(af::constant(0.0, p.dims(), p.type()), false));
            reducer->add(p.grad());
          }
          for (auto& p : criterion->params()) {
            if (!p.isGradAvailable()) p.addGrad(fl::Variable(af::constant(0.0, p.dims(), p.type()), false));
            reducer->add(p.grad());
          }
          reducer->finalize();
        }
        af::sync();
        bwdtimer.stopAndIncUnit();

        // optimizer: scale down gradients by batchsize, clamp, update
        optimtimer.resume();
        af::array totalBatchSizeArr = af::constant((double)loss.dims(0), af::dim4(1), af::f32);   // Train.cpp:1743-1747
        if (reducer) fl::allReduce(totalBatchSizeArr);
        const double totalBatchSize = (double)totalBatchSizeArr.scalar<float>();
        // (Train.cpp:1748-1760: `p.grad() = p.grad() / totalBatchSize` per parameter -- here in place, the planned network's
        // gradient arena in one launch)
        fl::scaleGradients(network->params(), 1.0 / totalBatchSize);
        fl::scaleGradients(criterion->params(), 1.0 / totalBatchSize);
        if (maxgradnorm > 0) {
          auto params = network->params();
          if (clampCrit) {
            auto cp = criterion->params();
            params.insert(params.end(), cp.begin(), cp.end());
          }
          const bool dbg = flags.getb("w2l_debug_gradnorm", false);
          double gEm = 0, gCrit = 0, gNet = 0;
          if (dbg) {   // (norms after the division by the batch size; 1e30 never clips)
            if (critInput.isGradAvailable()) gEm = fl::clipGradNorm({critInput}, 1e30);
            gCrit = fl::clipGradNorm(criterion->params(), 1e30);
            gNet = fl::clipGradNorm(network->params(), 1e30);
          }
          const double gnorm = fl::clipGradNorm(params, maxgradnorm);
          if (dbg) std::cout << "[debug] update " << curBatch << " gradient norm " << gnorm << " (network " << gNet << ", criterion " << gCrit
                             << ", emissions (unscaled) " << gEm << ")" << std::endl;
        }
        critoptim->step();
        netoptim->step();
        af::sync();
        optimtimer.stopAndIncUnit();
      }
      if (savePl) ipl->store(unsupIds, plToSave);
      if (!doUpdate) std::cout << "Skip update step as unsup data has no label " << curBatch << std::endl;
      if (useEma) {   // Train.cpp:1823-1832: after EVERY update, skipped or not -- one launch over the parameter arena
        optimtimer.resume();
        fl::ext::emaUpdate(networkEMA, network, emaDecay);
        af::sync();
        optimtimer.stop();
      }
      if (!isSup && haveBatch && ipl->labelAfterUpdate()) ipl->store(unsupIds, predictPL(cleanFeats, inputSizes, unsupSamples, curBatch));   // Train.cpp:1833-1840
      if (isSup) ++supDone;
      const bool epochEnd = isSup && supDone % batchesPerEpoch == 0;   // a pass over the supervised lists is complete
      if (epochEnd) iplNeedEpoch = true;
      timer.stopAndIncUnit();
      nsamples += curB;
      framesTotal += (long)curB * curT;
      ++nbatches;

      const bool report = (reportiters > 0 && curBatch % reportiters == 0) || curBatch == iters;
      if (report) runValid();   // on every rank (the sums are all-reduced), before the log line that carries them
      if (isMaster && report) logStatus(curEpoch, curBatch, lr, lrcrit);
      if (report) saveBestValid(curEpoch, curBatch);
      if (reportiters > 0 && curBatch % reportiters == 0) {
        // every report starts the next readings afresh (resetTimeStatMeters + the train meters, Train.cpp:1081-1090, :1125-1131,
        // :1844-1847): a report's timers are those of its own window, not of the run so far
        timer.reset(); sampletimer.reset(); fwdtimer.reset(); critfwdtimer.reset(); bwdtimer.reset(); optimtimer.reset();
        runtime.total = 0;
        lossSum = 0; lossN = 0; editErr = 0; editLen = 0; tszTotal = 0; tszMax = 0; nsamples = 0; nbatches = 0; framesTotal = 0;
        wordMeter = fl::EditDistanceMeter();
        lossUnsupSum = 0; lossUnsupN = 0;
        tknUnsupMeter = fl::EditDistanceMeter(); wordUnsupMeter = fl::EditDistanceMeter();
      }
      if (epochEnd || curBatch == iters) saveModels(curEpoch, curBatch);
    }
    if (auto* cr = dynamic_cast<fl::CoalescingReducer*>(reducer.get()))
      std::cout << "[Distributed] gradient collectives of the last update: " << cr->lastCollectives() << " (" << cr->lastOverlapped()
                << " issued on the side stream behind bucket events of the backward pass)" << std::endl;
    std::cout << "Finished training" << std::endl;
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "Train: " << e.what() << std::endl;
    return 1;
  }
}
