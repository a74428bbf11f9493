// Compiled C++ caller of fl::pkg::speech::ASGLoss::beamSearch (include/fl_compat/flashlight.h, fl_compat/lm.h, fl_compat/lexicon.h),
// built with plain g++ against libw2l_hip.so and driven by tests/test_gpu_asg_beam.py, which writes the inputs, runs this binary and
// compares its hypotheses with the C ABI's and the Python front end's.  The criterion's transitions are set through setParams.
//
//   decode_asg_caller <in.bin> <out.bin> [<tokens file> <arpa> [<lexicon file> <silence token> <replabel>]]
//       no further argument: no LM; tokens + arpa: a token LM; with a lexicon the arpa is over its words
//       in : int32 N T B W K M Lmax maxWords logAdd normalize | float threshold lmWeight wordScore eosScore | float em[B][T][N] |
//            int32 frames[B] | float trans[N][N]
//       out: twice (inputSizes = frames as (1, B), then no inputSizes):
//            int32 labels[B][M][Lmax] | int32 lengths[B][M] | float scores[B][M] | with an LM float lmScores[B][M] |
//            with a lexicon int32 words[B][M][maxWords] | int32 wordCounts[B][M]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "fl_compat/flashlight.h"
#include "fl_compat/lexicon.h"
#include "fl_compat/lm.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 3 && argc != 5 && argc != 8) { std::cerr << "usage: decode_asg_caller <in.bin> <out.bin> [<tokens> <arpa> [<lexicon> <sil> <replabel>]]\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int N = hd[0], T = hd[1], B = hd[2], W = hd[3], K = hd[4], M = hd[5], Lmax = hd[6], maxWords = hd[7];
  const float* fl4 = (const float*)(hd + 10);
  const float* em = fl4 + 4;
  const int* frames = (const int*)(em + (size_t)B * T * N);
  const float* trans = (const float*)(frames + B);

  std::unique_ptr<NGramLM> lm;
  std::unique_ptr<Lexicon> lex;
  if (argc >= 5) {
    std::vector<std::string> tokens;
    std::ifstream tf(argv[3]);
    for (std::string line; std::getline(tf, line);)
      if (!line.empty()) tokens.push_back(line);
    if (argc == 8) {
      lex.reset(new Lexicon(Lexicon::fromFile(argv[5], tokens, nullptr, argv[6], "none", std::atoi(argv[7]))));
      lm.reset(new NGramLM(NGramLM::fromArpa(argv[4], lex->words())));
      lex.reset(new Lexicon(Lexicon::fromFile(argv[5], tokens, lm.get(), argv[6], "max", std::atoi(argv[7]))));
    } else {
      lm.reset(new NGramLM(NGramLM::fromArpa(argv[4], tokens)));
    }
  }

  ASGLoss crit(N, CriterionScaleMode::NONE, 0.0);
  crit.setParams(Variable(af::array(af::dim4(N, N), trans), true), 0);
  BeamSearchOptions opt;            // the hoisted name; CTCLoss::BeamSearchOptions is the same type
  static_assert(std::is_same<BeamSearchOptions, CTCLoss::BeamSearchOptions>::value, "one options type");
  opt.beamSize = W;
  opt.beamSizeToken = K;
  opt.beamThreshold = fl4[0];
  opt.logAdd = hd[8] != 0;
  opt.normalize = hd[9];
  opt.nbest = M;
  opt.maxLen = Lmax;
  if (lm) {
    opt.lm = lm.get();
    opt.lmWeight = fl4[1];
    opt.eosScore = fl4[3];
  }
  if (lex) {
    opt.lexicon = lex.get();
    opt.wordScore = fl4[2];
    opt.maxWords = maxWords;
  }
  af::array emission(af::dim4(N, T, B), em);
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  for (int pass = 0; pass < 2; ++pass) {
    BeamSearchResult r = crit.beamSearch(emission, pass == 0 ? af::array(af::dim4(1, B), frames) : af::array(), opt);
    if (r.labels.dims(0) != Lmax || r.labels.dims(1) != M || r.labels.dims(2) != B || r.lengths.dims(0) != M || r.lengths.dims(1) != B ||
        r.scores.dims(0) != M || r.scores.dims(1) != B || r.lmScores.isempty() != !lm || r.words.isempty() != !lex) {
      std::cerr << "result dims / types\n";
      return 1;
    }
    std::vector<int> lab((size_t)B * M * Lmax), len((size_t)B * M);
    std::vector<float> sc((size_t)B * M);
    r.labels.host(lab.data());
    r.lengths.host(len.data());
    r.scores.host(sc.data());
    fwrite(lab.data(), 4, lab.size(), out);
    fwrite(len.data(), 4, len.size(), out);
    fwrite(sc.data(), 4, sc.size(), out);
    if (lm) {
      std::vector<float> ls((size_t)B * M);
      r.lmScores.host(ls.data());
      fwrite(ls.data(), 4, ls.size(), out);
    }
    if (lex) {
      std::vector<int> wd((size_t)B * M * maxWords), wc((size_t)B * M);
      r.words.host(wd.data());
      r.wordCounts.host(wc.data());
      fwrite(wd.data(), 4, wd.size(), out);
      fwrite(wc.data(), 4, wc.size(), out);
    }
  }
  fclose(out);
  int refused = 0;
  { auto o = opt; o.nbest = W + 1; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  { auto o = opt; o.beamSize = 65; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) {} catch (const std::runtime_error&) { ++refused; } }
  {
    ASGLoss other(N + 1, CriterionScaleMode::NONE, 0.0);
    try { other.beamSearch(emission, af::array(), opt); } catch (const std::invalid_argument&) { ++refused; }
  }
  if (!lm) { auto o = opt; o.lmWeight = 0.5f; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  else { auto o = opt; o.lmWeight = 1.0f / 0.0f; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  if (refused != 4) { std::cerr << "expected four refusals, got " << refused << "\n"; return 1; }
  std::cout << "decode asg caller ok" << std::endl;
  return 0;
}
