// Compiled C++ caller of CTCLoss::beamSearch and ASGLoss::beamSearch with BeamSearchOptions::lmToken, a token LM under a lexicon
// (include/fl_compat/flashlight.h), built with plain g++ against libw2l_hip.so by `make -f decode_lextok_caller.mk decode_lextok_caller`
// and driven by tests/test_gpu_beam_lextok_surfaces.py, which writes the inputs, runs this binary and compares its hypotheses with
// the C ABI's (w2l_*_beam_search_lextok) and the Python front end's.
//
//   decode_lextok_caller <in.bin> <out.bin> <tokens file> <token arpa> <lexicon file> <silence token> <replabel>
//       in : int32 N T B W K M Lmax maxWords logAdd normalize asg family silToken | float threshold lmWeight wordScore eosScore
//            silScore | float em[B][T][N] | int32 frames[B] | asg: float trans[N][N]
//            family 0 / 1: the narrow or wide (options.wide) kernels; silToken -1: the lexicon's
//       out: int32 labels[B][M][Lmax] | int32 lengths[B][M] | float scores[B][M] | float lmScores[B][M] |
//            int32 words[B][M][maxWords] | int32 wordCounts[B][M]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <vector>

#include "fl_compat/flashlight.h"
#include "fl_compat/lexicon.h"
#include "fl_compat/lm.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 8) { std::cerr << "usage: decode_lextok_caller <in.bin> <out.bin> <tokens> <token arpa> <lexicon> <sil> <replabel>\n"; return 2; }
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
  const bool asg = hd[10] != 0;
  const int family = hd[11], silToken = hd[12];
  const float* fl5 = (const float*)(hd + 13);
  const float* em = fl5 + 5;
  const int* frames = (const int*)(em + (size_t)B * T * N);
  const float* trans = (const float*)(frames + B);

  std::unique_ptr<NGramLM> lm;
  std::unique_ptr<Lexicon> lex;
  {
    std::vector<std::string> tokens;
    std::ifstream tf(argv[3]);
    for (std::string line; std::getline(tf, line);)
      if (!line.empty()) tokens.push_back(line);
    lex.reset(new Lexicon(Lexicon::fromFile(argv[5], tokens, nullptr, argv[6], "none", std::atoi(argv[7]))));
    lm.reset(new NGramLM(NGramLM::fromArpa(argv[4], tokens)));
  }

  std::unique_ptr<ASGLoss> asgCrit;
  CTCLoss ctc(CriterionScaleMode::NONE);
  if (asg) {
    asgCrit.reset(new ASGLoss(N, CriterionScaleMode::NONE, 0.0));
    asgCrit->setParams(Variable(af::array(af::dim4(N, N), trans), true), 0);
  }
  BeamSearchOptions opt;
  opt.beamSize = W;
  opt.beamSizeToken = K;
  opt.beamThreshold = fl5[0];
  opt.logAdd = hd[8] != 0;
  opt.normalize = hd[9];
  opt.nbest = M;
  opt.maxLen = Lmax;
  opt.wide = family == 1;
  opt.lmToken = true;
  opt.silToken = silToken;
  opt.silScore = fl5[4];
  if (lm) {
    opt.lm = lm.get();
    opt.lmWeight = fl5[1];
    opt.eosScore = fl5[3];
  }
  if (lex) {
    opt.lexicon = lex.get();
    opt.wordScore = fl5[2];
    opt.maxWords = maxWords;
  }
  af::array emission(af::dim4(N, T, B), em);
  auto search = [&](const BeamSearchOptions& o) {
    const af::array sizes(af::dim4(1, B), frames);
    return asg ? asgCrit->beamSearch(emission, sizes, o) : ctc.beamSearch(emission, sizes, o);
  };
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  {
    BeamSearchResult r = search(opt);
    if (r.labels.dims(0) != Lmax || r.labels.dims(1) != M || r.labels.dims(2) != B || r.lmScores.isempty() != !lm ||
        r.words.isempty() != !lex) {
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
  // refusals: without a lexicon, with xl, with an LM over another token count, and the streaming decoders
  int refused = 0;
  { auto o = opt; o.lexicon = nullptr; o.wordScore = 0.f; o.maxWords = 0; try { search(o); } catch (const std::invalid_argument&) { ++refused; } }
  { auto o = opt; o.wide = false; o.xl = true; try { search(o); } catch (const std::invalid_argument&) { ++refused; } }
  {
    BeamSearchOptions o;
    o.beamSize = 8; o.beamSizeToken = 4; o.lm = lm.get(); o.lexicon = lex.get(); o.lmToken = true;
    try { StreamingDecoder dec(1, 4, 16, N, o); } catch (const std::invalid_argument&) { ++refused; }
    try { WideStreamingDecoder dec(1, 4, 16, N, o); } catch (const std::invalid_argument&) { ++refused; }
  }
  if (refused != 4) { std::cerr << "expected four refusals, got " << refused << "\n"; return 1; }
  std::cout << "decode lextok caller ok" << std::endl;
  return 0;
}
