// decode_main.cpp -- `Decode --am=<NNN_model_*.bin> --test=<list> [--datadir=] [--batchsize=] [--sclite=<dir>] [--beamsize=]
// [--beamsizetoken=] [--beamthreshold=] [--logadd=] [--isbeamdump=] [--nbest=] [--show=] [--showletters=] [--w2l_beam_xl=] [--w2l_beam_tokens=] [--w2l_silscore=] [--silscore=] [--w2l_lex_tkn=] [--k=v ...]`: the
// reference's Decode tool for its lexicon-free token decoder (`--uselexicon=false --decodertype=tkn`), without LM (the configuration
// of recipes/self_training/librispeech/am/decode_*.cfg) or with a token-level n-gram LM (`--lm=<arpa>`, recipes/lexicon_free and the
// word-piece runs of sota/2019), and for its lexicon decoder with a word LM (recipes/conv_glu/*/decode*.cfg), over the fl::
// surface, for CTC and for ASG models.  Output formats: Decode.cpp:683-739, :840-846.
//
// Flags come from the checkpoint's `gflags` entry, then from the command line (the last definition wins), as in Align.  The tool
// builds the network and the checkpoint's criterion (CTC or ASG), loads both from --am and runs the eval-mode network over the
// --test list in list order in batches of --batchsize through list_data.hpp; one beamSearch call of the criterion per batch
// (CTCLoss: w2l_ctc_beam_search*; ASGLoss: w2l_asg_beam_search* under the checkpoint's transitions) with the utterances'
// emission-frame counts, computed as in align_main.cpp: frames_b = clamp(ceil(tb * Tout / Tin), 1, Tout).
//   --criterion=asg (from the checkpoint): the classes are the tokens plus --replabel, as Train counts them, and there is no blank;
//     a token LM is over all of them (the replabels `<1>`.. are words of the ARPA file), the lexicon's spellings are packed with
//     --replabel (`h e l l o` -> `h e l <1> o`), hypotheses are unpacked by tknLabels2Ltr.  The search runs on the raw emissions in
//     both --logadd modes: ASG scores are unnormalised by design.  With --logadd=false and without LM or lexicon the 1-best is the
//     Viterbi transcript of Train.
//   --beamsize (2500), --beamsizetoken (250000), --beamthreshold (25), --logadd (false), --nbest (1): the reference's names and
//   defaults.  A --beamsize given in the flags (the checkpoint's or the command line's) above 64 runs the wide kernels
//   (BeamSearchOptions::wide), which keep up to 1024 beam entries: larger values are limited to 1024 (said on stderr).  A value up
//   to 64 runs the narrow kernels; so does an absent --beamsize, whose default is limited to 64 (said on stderr).  All kernels keep
//   at most 64 tokens per frame: a larger --beamsizetoken is limited to 64 (said on stderr).
//   --w2l_beam_xl=true (not the reference's; default false): a --beamsize given in the flags and above 1024 runs the xl kernels
//   (BeamSearchOptions::xl), which keep up to 8192 beam entries -- the recipes' 1500, 2500, 5000 and 8000 as they are written;
//   larger values are limited to 8192 (said on stderr).  Values up to 1024 and an absent --beamsize route as without the flag.
//   --w2l_beam_tokens=true (not the reference's; default false): a --beamsizetoken given in the flags and, after clipping to the
//   token count, above 64 runs the many-token kernels (BeamSearchOptions::manyTokens, the w2l_*_mt entry points) at that value --
//   the word-piece recipes' 100 and 150 as they are written -- for any given --beamsize up to 8192; larger values are limited to
//   256 tokens and 8192 entries, each said on stderr (an absent --beamsize is limited to 64 as ever).  With a token count at or
//   under 64 after clipping, or an absent --beamsizetoken, routing is as without the flag.  --w2l_lex_tkn=true with it is refused.
//   --w2l_silscore=true (not the reference's; default false): --silscore (older name: --silweight; both given with different
//   values: refused) takes effect in every search Decode runs (BeamSearchOptions::silToken / silScore, the w2l_*_sil entry points):
//   the silence token is the class of --wordseparator, and after a frame's tokens have been chosen by the acoustic score alone that
//   class's frame score is score + silscore wherever the search reads it.  A non-zero score when the separator is no class of its
//   own (the word-piece recipes) is refused, naming the token.  Without the flag a non-zero --silscore is refused and a non-zero
//   --silweight stays without effect, which one stderr line says.
//   --logadd=false (default): a prefix scores the MAX over its alignments, on the raw emissions as in the reference's decoder; the
//     1-best then equals the greedy transcript (the collapsed per-frame arg-max), the n-best are the next best single alignments.
//   --logadd=true: the labelling-probability search -- a prefix scores the SUM over its alignments, on log-softmax rows (sums only
//     mean something on log-probabilities).
//   --sclite=<dir>: <dir>/<name>.hyp and .ref hold `words (sampleId)\n`, <name> = the list's base name; .log holds what --show
//     prints and the final line.  --show: the |T|: / |P|: (/ |t|: / |p|: with --showletters) / [sample: ...] block per sample.
//   --isbeamdump=true (needs --sclite): .hyp holds one line `sampleId | score | amScore | lmScore | wer | words` per hypothesis,
//     --nbest of them per sample in rank order; without --lm lmScore is 0 and amScore equals score.
//   --lm=<arpa> [--lmtype=kenlm] [--lmweight=0] [--eosscore=0] [--wordscore=0]: the search fused with a back-off n-gram LM over the
//     tokens (w2l_ctc_beam_search_lm).  --lmtype=kenlm (the reference's default) means "n-gram, ARPA text" here: the file is read
//     by this library, KenLM binaries and gzip are refused; convlm is refused by name.  --wordscore is added to the classes that
//     begin a word: the pieces that start with the word separator with --usewordpiece=true, else the separator class.  In the
//     beam dump lmScore is the hypothesis's unweighted LM score and amScore = score - (lmweight * lmScore + its word scores +
//     eosscore), computed on the host in double.
//   --uselexicon=true --decodertype=wrd --lexicon=<file> --lm=<word arpa> [--lmweight=0] [--wordscore=0] [--eosscore=0]
//     [--smearing=none|max]: the search restricted to the spellings of the lexicon and scored by an n-gram LM over its WORDS
//     (w2l_ctc_beam_search_lex; the reference recipes' decoder configuration).  The word-separator class is the silence token the
//     search lets loop between words when the token dictionary has it.  --wordscore is added once per word.  .hyp lines, beam-dump
//     rows and WER come from the hypotheses' word ids; amScore = score - (lmweight * lmScore + wordscore * words + eosscore).
//     A sample none of whose hypotheses ends on a word boundary gets an empty hypothesis.
//   --w2l_lex_tkn=true (not the reference's; default false) --uselexicon=true --decodertype=tkn --lexicon=<file> --lm=<token arpa>:
//     the search restricted to the spellings of the lexicon and scored by an n-gram LM over the TOKENS (w2l_ctc_beam_search_lextok,
//     BeamSearchOptions::lmToken; the reference's lexicon_free recipes).  Every token that moves along a trie edge adds lmweight *
//     its LM score, a completed word adds --wordscore.  --beamsize up to 1024; --w2l_beam_xl=true with the flag is refused.
//     --smearing=none|max is accepted and has no effect (said on stderr).  Output rows are the wrd decoder's.  Without the flag
//     --decodertype=tkn with --uselexicon=true is refused as before.
//   The last line gives the total WER / TER (fl::EditDistanceMeter, the --valid evaluation's).
// Refused, each with a message that names the flag: an unreadable or malformed --lm, --lmtype other than kenlm, --uselexicon=true
// without --lexicon or --lm, --decodertype=wrd without --uselexicon=true, --decodertype=tkn with it unless --w2l_lex_tkn=true, --smearing=logadd, a finite
// --unkscore (no unknown-word arc), a lexicon spelling with a token the dictionary lacks (the message names the word), a non-zero
// --silscore without --w2l_silscore=true, a non-zero --wordscore without --lm, a --criterion other than ctc or asg, a --criterion on the command line that is not
// the checkpoint's (the criterion's parameters come from the checkpoint).  (--uselexicon and --decodertype default to false / tkn
// here, so an invocation without them is the lexicon-free search.)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <iomanip>
#include <iostream>
#include <limits>

#include "../../../include/fl_compat/lexicon.h"
#include "../../../include/fl_compat/lm.h"
#include "list_data.hpp"

using namespace fl;
using namespace fl::pkg::speech;
using namespace w2l::cli;

namespace {
int usage(const char* exe) {
  std::cerr << "Usage: \n " << exe
            << " --am=<model> --test=<list> [--datadir=...] [--batchsize=...] [--sclite=<dir>] [--beamsize=2500] [--beamsizetoken=250000]"
               " [--beamthreshold=25] [--logadd=false] [--isbeamdump=false] [--nbest=1] [--show=false] [--showletters=false] [--w2l_beam_xl=false] [--w2l_beam_tokens=false] [--w2l_silscore=false --silscore=0] [flags]\n"
               " [--lm=<arpa> --lmtype=kenlm --lmweight=0 --eosscore=0 --wordscore=0]\n"
               " [--uselexicon=true --decodertype=wrd --lexicon=<file> --lm=<word arpa> --smearing=none|max]\n"
               " [--w2l_lex_tkn=true --uselexicon=true --decodertype=tkn --lexicon=<file> --lm=<token arpa>]\n"
               " CTC or ASG (as the checkpoint says) token beam search, optionally with a token-level n-gram LM (ARPA text); --beamsize is limited to 1024 when given (above 64: the wide kernels), to 64 when absent; with --w2l_beam_xl=true a given --beamsize above 1024 runs the xl kernels and is limited to 8192; tokens per frame are limited to 64, or with --w2l_beam_tokens=true a given --beamsizetoken above 64 runs the many-token kernels (any given --beamsize up to 8192) and is limited to 256.\n"
               " --w2l_silscore=true: --silscore (older name --silweight) is added to the frame score of the --wordseparator class after the frame's tokens are chosen; without it a non-zero --silscore is refused.\n"
               " --logadd=false (default): max over a prefix's alignments on the raw emissions -- the 1-best equals the greedy transcript.\n"
               " --logadd=true: the labelling-probability search (sum over a prefix's alignments, on log-softmax rows)."
            << std::endl;
  return 2;
}

std::string join(const std::vector<std::string>& v) {
  std::string out;
  for (size_t i = 0; i < v.size(); ++i) out += (i ? " " : "") + v[i];
  return out;
}

std::string baseName(const std::string& path) {
  const size_t slash = path.find_last_of('/');
  std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
  const size_t dot = name.find_last_of('.');
  return dot == std::string::npos || dot == 0 ? name : name.substr(0, dot);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc <= 1) return usage(argv[0]);
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]).rfind("--", 0) != 0 || std::string(argv[i]) == "--help") return usage(argv[0]);
  try {
    using Serializer = fl::pkg::runtime::Serializer;
    w2l::Flags cmd;
    for (int i = 1; i < argc; ++i)
      for (auto& kv : w2l::parseFlagsText(argv[i]).kv) cmd.kv.push_back(kv);
    const std::string am = cmd.get("am", "");
    if (am.empty()) throw std::invalid_argument("--am=<model file> is required");
    std::string version;
    Serializer::Config cfg;
    Serializer::load(am, version, cfg);
    auto it = cfg.find("gflags");
    if (it == cfg.end()) throw std::invalid_argument("Invalid config loaded from " + am);
    w2l::Flags flags = w2l::parseFlagsText(it->second);
    const std::string criterionName = flags.get("criterion", "asg");   // the checkpoint's: its parameters are the checkpoint's too
    for (auto& kv : cmd.kv) flags.kv.push_back(kv);
    w2l::checkFlagDependencies(flags);

    // ---- what this build does not decode
    if (flags.get("criterion", "asg") != criterionName)
      throw std::invalid_argument("--criterion=" + flags.get("criterion", "asg") + ": the model was trained with --criterion=" + criterionName +
                                  ", and Decode searches the lattice of the checkpoint's criterion");
    if (criterionName != "ctc" && criterionName != "asg")
      throw std::invalid_argument("--criterion=" + criterionName + ": Decode searches the CTC and the ASG lattice only");
    const bool asg = criterionName == "asg";
    const std::string lmPath = flags.get("lm", "");
    if (!lmPath.empty()) {
      const std::string lmType = flags.get("lmtype", "kenlm");
      if (lmType == "convlm") throw std::invalid_argument("--lmtype=convlm: no ConvLM in this build (an n-gram model as ARPA text: --lmtype=kenlm)");
      if (lmType != "kenlm") throw std::invalid_argument("--lmtype=" + lmType + ": only kenlm (an n-gram model as ARPA text) is built");
    }
    const bool useLexicon = flags.getb("uselexicon", false);
    const std::string decoderType = flags.get("decodertype", "tkn"), lexiconPath = flags.get("lexicon", "");
    const std::string smearing = flags.get("smearing", "none");
    // the token LM under a lexicon: opt-in (--w2l_lex_tkn=true), taken by --uselexicon=true --decodertype=tkn
    const bool lexTkn = flags.getb("w2l_lex_tkn", false);
    const bool tokenLm = lexTkn && useLexicon && decoderType == "tkn";
    if (lexTkn && flags.getb("w2l_beam_xl", false))
      throw std::invalid_argument("--w2l_beam_xl=true with --w2l_lex_tkn=true: the token LM under a lexicon has no xl kernels (beams up to 1024)");
    if (lexTkn && flags.getb("w2l_beam_tokens", false))
      throw std::invalid_argument("--w2l_beam_tokens=true with --w2l_lex_tkn=true: the token LM under a lexicon has no many-token kernels (64 tokens per frame)");
    if (decoderType != "tkn" && decoderType != "wrd")
      throw std::invalid_argument("--decodertype=" + decoderType + ": tkn (lexicon-free) or wrd (with --uselexicon=true)");
    if (useLexicon) {
      if (lexiconPath.empty()) throw std::invalid_argument("--uselexicon=true needs --lexicon=<file>");
      if (lmPath.empty()) throw std::invalid_argument("--uselexicon=true needs --lm=<arpa of a model over the lexicon's words>");
      if (decoderType != "wrd" && !lexTkn)
        throw std::invalid_argument("--decodertype=tkn with --uselexicon=true: no token LM under a lexicon in this build (--decodertype=wrd)");
      if (smearing == "logadd") throw std::invalid_argument("--smearing=logadd: log-add smearing is not built (none or max)");
      if (smearing != "none" && smearing != "max") throw std::invalid_argument("--smearing=" + smearing + ": none or max");
      if (std::isfinite(flags.getd("unkscore", -std::numeric_limits<double>::infinity())))
        throw std::invalid_argument("--unkscore: no unknown-word arc in this build (leave it -inf)");
      if (tokenLm && flags.has("smearing"))
        std::cerr << "[Decode] --smearing=" << smearing << " has no effect with --decodertype=tkn: the token LM scores every token" << std::endl;
    } else if (decoderType == "wrd") {
      throw std::invalid_argument("--decodertype=wrd needs --uselexicon=true --lexicon=<file> --lm=<word arpa>");
    }
    // the silence score: opt-in (--w2l_silscore=true); --silweight is --silscore's older name
    const bool silFlag = flags.getb("w2l_silscore", false);
    double silScore = flags.getd("silscore", 0.0);
    const double silWeight = flags.getd("silweight", 0.0);
    if (!silFlag) {
      if (silScore != 0.0)
        throw std::invalid_argument("--silscore: no silence score without --w2l_silscore=true (leave it 0, or add --w2l_silscore=true)");
      if (silWeight != 0.0)
        std::cerr << "[Decode] --silweight=" << silWeight << " has no effect without --w2l_silscore=true" << std::endl;
    } else {
      if (flags.has("silscore") && flags.has("silweight") && silScore != silWeight)
        throw std::invalid_argument("--silscore and --silweight (its older name) are both given with different values");
      if (!flags.has("silscore")) silScore = silWeight;
      if (!std::isfinite(silScore)) throw std::invalid_argument("--silscore must be finite");
    }
    const double wordScore = flags.getd("wordscore", 0.0), lmWeight = flags.getd("lmweight", 0.0), eosScore = flags.getd("eosscore", 0.0);
    if (lmPath.empty() && wordScore != 0.0) throw std::invalid_argument("--wordscore: no word score without --lm (leave it 0)");
    if (!std::isfinite(wordScore) || !std::isfinite(lmWeight) || !std::isfinite(eosScore))
      throw std::invalid_argument("--wordscore, --lmweight and --eosscore must be finite");

    const int batch = (int)flags.geti("batchsize", 1);
    if (batch <= 0) throw std::invalid_argument("--batchsize must be positive");
    const bool logAdd = flags.getb("logadd", false), beamDump = flags.getb("isbeamdump", false);
    const bool show = flags.getb("show", false), showLetters = flags.getb("showletters", false);
    const std::string sclite = flags.get("sclite", "");
    if (beamDump && sclite.empty()) throw std::invalid_argument("--isbeamdump needs --sclite=<dir>: nowhere to dump the beam");
    long beamSize = flags.geti("beamsize", 2500), beamToken = flags.geti("beamsizetoken", 250000), nbest = flags.geti("nbest", 1);
    const double threshold = flags.getd("beamthreshold", 25.0);
    if (beamSize <= 0 || beamToken <= 0 || nbest <= 0) throw std::invalid_argument("--beamsize, --beamsizetoken and --nbest must be positive");
    if (!(threshold >= 0)) throw std::invalid_argument("--beamthreshold must be >= 0");

    const int nFeat = flags.getb("mfcc", false) ? (int)flags.geti("mfcccoeffs", 13) * 3
                      : flags.getb("pow", false) ? (int)flags.geti("framesizems", 25) * 8 + 1 : (int)flags.geti("filterbanks", 40);
    const std::string tok = pathJoin(flags.get("tokensdir", ""), flags.get("tokens", "tokens.txt"));
    int numClasses = countTokens(tok);
    if (numClasses <= 0) throw std::invalid_argument("cannot read the token dictionary '" + tok + "' (--tokensdir / --tokens)");
    if (asg) numClasses += (int)flags.geti("replabel", 0);   // tokens, then the replabels; no blank (Train's count)
    else numClasses += 1;                                    // blank, appended LAST
    const int numTokens = asg ? numClasses : numClasses - 1;   // the classes a hypothesis is made of
    // a beam width that was asked for runs the wide kernels above 64, and with --w2l_beam_xl=true the xl kernels above 1024
    // and with --w2l_beam_tokens=true a token count that was asked for and is above 64 after clipping runs the many-token kernels
    const bool xlFlag = flags.getb("w2l_beam_xl", false);
    beamToken = std::min<long>(beamToken, numTokens);
    const bool manyTokens = flags.getb("w2l_beam_tokens", false) && flags.has("beamsizetoken") && beamToken > 64;
    const long beamLimit = flags.has("beamsize") ? (xlFlag || manyTokens ? 8192 : 1024) : 64;
    if (beamSize > beamLimit) {
      std::cerr << "[Decode] --beamsize=" << beamSize << " limited to " << beamLimit << " (the kernel's beam width)" << std::endl;
      beamSize = beamLimit;
    }
    const bool xl = !manyTokens && beamSize > 1024, wide = !manyTokens && beamSize > 64 && !xl;
    if (manyTokens) {
      if (beamToken > 256) { std::cerr << "[Decode] --beamsizetoken limited to 256 tokens per frame" << std::endl; beamToken = 256; }
    } else if (beamToken > 64) { std::cerr << "[Decode] --beamsizetoken limited to 64 tokens per frame" << std::endl; beamToken = 64; }
    const int M = beamDump ? (int)std::min(nbest, beamSize) : 1;

    // ---- network and criterion, both from the model file (Train fork's construction)
    const std::string archPath = pathJoin(flags.get("archdir", ""), flags.get("arch", ""));
    if (!fileExists(archPath)) throw std::invalid_argument("arch file / plugin '" + archPath + "' not found (--archdir / --arch)");
    auto scalemode = getCriterionScaleMode(flags.get("onorm", "none"), flags.getb("sqnorm", false));
    std::shared_ptr<fl::Module> network = fl::pkg::runtime::ModulePlugin(archPath).arch(nFeat, numClasses);
    if (flags.getb("fl_amp_use_mixed_precision", false)) setMixedPrecision(network, true);
    if (flags.getb("fl_amp_use_mixed_precision", false) && flags.getb("w2l_amp_convs", false)) setMixedPrecisionConvolutions(network, true);
    std::shared_ptr<CTCLoss> ctc;
    std::shared_ptr<ASGLoss> asgCrit;
    std::shared_ptr<SequenceCriterion> criterion;
    if (asg) criterion = asgCrit = std::make_shared<ASGLoss>(numClasses, scalemode, flags.getd("transdiag", 0.0));
    else criterion = ctc = std::make_shared<CTCLoss>(scalemode);
    Serializer::Config unused;
    Serializer::load(am, version, unused, network, criterion);
    network->eval();
    criterion->eval();
    std::cerr << "[Decode] " << criterion->prettyString() << ", " << numClasses << " classes, model " << am << ", beam " << beamSize << (manyTokens ? " (many-token)" : xl ? " (xl)" : wide ? " (wide)" : "")
              << ", tokens per frame " << beamToken << ", threshold " << threshold << (logAdd ? ", logadd" : ", max") << std::endl;

    // ---- the list
    const std::string dataDir = flags.get("datadir", ""), testFlag = flags.get("test", "");
    std::vector<std::string> listPaths;
    {
      std::istringstream ls(testFlag);
      for (std::string one; std::getline(ls, one, ',');) if (!one.empty()) listPaths.push_back(pathJoin(dataDir, one));
    }
    if (listPaths.empty()) throw std::invalid_argument("--test=<list file> is required");
    ListData d;
    d.tolerateTextErrors = true;
    loadListData(d, listPaths, batch, "--test", true, flags, criterionName, nFeat, numClasses, (uint64_t)flags.geti("seed", 0), dataDir);
    const bool wp = flags.getb("usewordpiece", false);
    const std::string surround = flags.get("surround", "");
    const std::string dump = flags.get("w2l_dump_features", "");
    int silToken = -1;
    if (silFlag && silScore != 0.0) {
      if (d.wordsep.empty() || !d.dict.contains(d.wordsep) || d.dict.getIndex(d.wordsep) >= numTokens)
        throw std::invalid_argument("--silscore: the word separator `" + d.wordsep + "` is no class of its own in the token dictionary, so there is no silence token to score (leave it 0)");
      silToken = d.dict.getIndex(d.wordsep);
      std::cerr << "[Decode] --silscore=" << silScore << " on the silence token `" << d.wordsep << "` (class " << silToken << ")" << std::endl;
    }

    // ---- the language model over the token classes, and the word score as class scores
    std::unique_ptr<NGramLM> lm;
    std::unique_ptr<Lexicon> lexicon;
    std::vector<float> classScore((size_t)numTokens, 0.f);
    af::array classScoreDev;
    if (useLexicon) {   // the lexicon trie, the LM over its words, and the LM's unigram-context scores smeared down the trie
      std::vector<std::string> tokens;
      for (int c = 0; c < numTokens; ++c) tokens.push_back(d.dict.getEntry(c));
      const std::string sil = !d.wordsep.empty() && d.dict.contains(d.wordsep) && d.dict.getIndex(d.wordsep) < numTokens ? d.wordsep : "";
      try {
        lexicon.reset(new Lexicon(Lexicon::fromFile(lexiconPath, tokens, nullptr, sil, "none", d.replabel)));
      } catch (const std::exception& e) {
        throw std::invalid_argument("--lexicon=" + lexiconPath + ": " + e.what());
      }
      try {
        lm.reset(new NGramLM(NGramLM::fromArpa(lmPath, tokenLm ? tokens : lexicon->words())));
      } catch (const std::exception& e) {
        throw std::invalid_argument("--lm=" + lmPath + ": " + e.what());
      }
      if (smearing == "max" && !tokenLm) lexicon.reset(new Lexicon(Lexicon::fromFile(lexiconPath, tokens, lm.get(), sil, "max", d.replabel)));
      if (!lm->hasEos() && eosScore != 0.0) throw std::invalid_argument("--eosscore: the model of --lm has no </s> (leave it 0)");
      std::cerr << "[Decode] --lexicon: " << lexicon->numWords() << " words, " << lexicon->numNodes() << " nodes, " << lexicon->dropped()
                << " homophones beyond the sixth dropped, smearing " << smearing << ", silence token " << (sil.empty() ? "none" : sil)
                << "; --lm over the " << (tokenLm ? "tokens" : "words") << ": order " << lm->order() << ", " << lm->numStates() << " states; " << lm->message() << std::endl;
    } else if (!lmPath.empty()) {
      std::vector<std::string> tokens;
      for (int c = 0; c < numTokens; ++c) tokens.push_back(d.dict.getEntry(c));
      try {
        lm.reset(new NGramLM(NGramLM::fromArpa(lmPath, tokens)));
      } catch (const std::exception& e) {
        throw std::invalid_argument("--lm=" + lmPath + ": " + e.what());
      }
      if (!lm->hasEos() && eosScore != 0.0) throw std::invalid_argument("--eosscore: the model of --lm has no </s> (leave it 0)");
      std::cerr << "[Decode] --lm: order " << lm->order() << ", " << lm->numStates() << " states; " << lm->message() << std::endl;
      if (wordScore != 0.0) {
        for (int c = 0; c < numTokens; ++c) {
          const bool begins = wp ? (!d.wordsep.empty() && tokens[(size_t)c].rfind(d.wordsep, 0) == 0) : tokens[(size_t)c] == d.wordsep;
          if (begins) classScore[(size_t)c] = (float)wordScore;
        }
        classScoreDev = af::array(af::dim4((af::dim_t)classScore.size()), classScore.data());
      }
    }

    std::ofstream hypFile, refFile, logFile;
    if (!sclite.empty()) {
      const std::string stem = pathJoin(sclite, baseName(listPaths.front()));
      hypFile.open(stem + ".hyp");
      refFile.open(stem + ".ref");
      logFile.open(stem + ".log");
      if (!hypFile || !refFile || !logFile) throw std::runtime_error("cannot open '" + stem + ".hyp / .ref / .log' for writing");
    }

    fl::EditDistanceMeter sliceWords, sliceLetters;
    long decoded = 0;
    const auto t0 = std::chrono::steady_clock::now();
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
      BeamSearchOptions opt;
      opt.beamSize = (int)beamSize;
      opt.wide = wide;
      opt.xl = xl;
      opt.manyTokens = manyTokens;
      opt.beamSizeToken = (int)beamToken;
      opt.beamThreshold = (float)threshold;
      opt.logAdd = logAdd;
      // the reference's decoder consumes the raw emissions; CTC sums need log-probabilities, ASG scores are unnormalised by design
      opt.normalize = logAdd && !asg ? 1 : 0;
      opt.nbest = M;
      opt.silToken = silToken;
      opt.silScore = silToken >= 0 ? (float)silScore : 0.f;
      if (lm) {
        opt.lm = lm.get();
        opt.lmWeight = (float)lmWeight;
        opt.classScore = classScoreDev;
        opt.eosScore = (float)eosScore;
      }
      if (lexicon) {
        opt.lexicon = lexicon.get();
        opt.wordScore = (float)wordScore;
        opt.maxWords = Tout;
        opt.lmToken = tokenLm;
      }
      const af::array framesDev(af::dim4(1, B), frames.data());
      auto res = asg ? asgCrit->beamSearch(out.array(), framesDev, opt) : ctc->beamSearch(out.array(), framesDev, opt);
      std::vector<int> labels((size_t)B * M * Tout), lengths((size_t)B * M);
      std::vector<float> scores((size_t)B * M);
      res.labels.host(labels.data());
      res.lengths.host(lengths.data());
      res.scores.host(scores.data());
      std::vector<float> lmScores((size_t)B * M, 0.f);
      if (lm) res.lmScores.host(lmScores.data());
      std::vector<int> words, wordCounts;
      if (lexicon) {
        words.resize((size_t)B * M * Tout);
        wordCounts.resize((size_t)B * M);
        res.words.host(words.data());
        res.wordCounts.host(wordCounts.data());
      }

      for (int b = 0; b < B; ++b) {
        const auto& smp = d.samples[(size_t)d.mine[(size_t)(k * batch + b)]];
        std::vector<int> ref;
        for (int i = 0; i < L && tgt[(size_t)b * L + i] >= 0; ++i) ref.push_back(tgt[(size_t)b * L + i]);
        const auto letterTarget = tknTarget2Ltr(ref, d.dict, criterionName, surround, d.replabel, wp, d.wordsep);
        const std::vector<std::string>& wordTarget = smp.transcript;
        for (int m = 0; m < M; ++m) {
          int len = lengths[(size_t)b * M + m];
          if (len < 0 && (beamDump || m > 0)) break;   // fewer surviving hypotheses than asked for
          if (len < 0) len = 0;   // nothing survived (a row of -inf or NaN emissions): an empty hypothesis, so every sample has its line
          const int* row = labels.data() + ((size_t)b * M + m) * Tout;
          const auto letterPrediction = tknLabels2Ltr(std::vector<int>(row, row + len), d.dict, criterionName, surround, d.replabel, wp, d.wordsep);
          const int* wrow = lexicon ? words.data() + ((size_t)b * M + m) * Tout : nullptr;
          const int nWords = lexicon ? std::max(wordCounts[(size_t)b * M + m], 0) : 0;
          const auto wordPrediction = lexicon ? lexicon->wordIds2Words(std::vector<int>(wrow, wrow + nWords)) : tkn2Wrd(letterPrediction, d.wordsep);
          if (beamDump) {
            fl::EditDistanceMeter one;
            one.add(wordPrediction, wordTarget);
            const double score = (double)scores[(size_t)b * M + m];
            double amScore = score, lmScore = 0.0;
            if (lm) {
              lmScore = (double)lmScores[(size_t)b * M + m];
              double extra = (double)(float)lmWeight * lmScore + (lm->hasEos() ? (double)(float)eosScore : 0.0);
              for (int i = 0; i < len; ++i) extra += (double)classScore[(size_t)row[i]];
              if (lexicon) extra += (double)(float)wordScore * nWords;
              amScore = score - extra;
            }
            hypFile << smp.id << " | " << std::to_string(score) << " | " << std::to_string(amScore) << " | " << std::to_string(lmScore) << " | "
                    << std::to_string(one.value()) << " | " << join(wordPrediction) << "\n";
            continue;
          }
          sliceWords.add(wordPrediction, wordTarget);
          sliceLetters.add(letterPrediction, letterTarget);
          if (!sclite.empty()) {
            hypFile << join(wordPrediction) << " (" << smp.id << ")\n";
            refFile << join(wordTarget) << " (" << smp.id << ")\n";
          }
          if (show) {
            fl::EditDistanceMeter w1, t1;
            w1.add(wordPrediction, wordTarget);
            t1.add(letterPrediction, letterTarget);
            std::stringstream buffer;
            buffer << "|T|: " << join(wordTarget) << std::endl;
            buffer << "|P|: " << join(wordPrediction) << std::endl;
            if (showLetters) {
              buffer << "|t|: " << join(letterTarget) << std::endl;
              buffer << "|p|: " << join(letterPrediction) << std::endl;
            }
            buffer << "[sample: " << smp.id << ", WER: " << w1.value() << "%, TER: " << t1.value() << "%, slice WER: " << sliceWords.value()
                   << "%, slice TER: " << sliceLetters.value() << "%, decoded samples (thread 0): " << decoded + 1 << "]" << std::endl;
            std::cout << buffer.str();
            if (!sclite.empty()) logFile << buffer.str();
          }
        }
        ++decoded;
      }
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::stringstream buffer;
    buffer << "------\n";
    buffer << "[Decode " << testFlag << " (" << decoded << " samples) in " << seconds << "s (actual decoding time " << std::setprecision(3)
           << (decoded ? seconds / (double)decoded : 0.0) << "s/sample) -- WER: " << std::setprecision(6) << sliceWords.value() << "%, TER: "
           << sliceLetters.value() << "%]" << std::endl;
    std::cout << buffer.str();
    if (!sclite.empty()) logFile << buffer.str();
    return decoded > 0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::cerr << "Decode: " << e.what() << std::endl;
    return 1;
  }
}
