// Compiled C++ caller of fl::pkg::speech::CTCLoss::beamSearch with a lexicon and a word-level n-gram LM (include/fl_compat/
// flashlight.h, fl_compat/lexicon.h, fl_compat/lm.h), built with plain g++ against libw2l_hip.so and driven by
// tests/test_gpu_ctc_beam_lex.py, which writes the inputs, the lexicon file and the ARPA file, runs this binary and compares its
// hypotheses with the C ABI's and the Python front end's.
//
//   decode_lex_caller <in.bin> <out.bin> <tokens file> <lexicon file> <arpa> <silence token or ->
//       in : int32 N T B W K M Lmax maxWords logAdd normalize | float threshold lmWeight wordScore eosScore | float em[B][T][N] |
//            int32 frames[B]
//       out: twice (inputSizes = frames as (1, B), then no inputSizes):
//            int32 labels[B][M][Lmax] | int32 lengths[B][M] | float scores[B][M] | float lmScores[B][M] |
//            int32 words[B][M][maxWords] | int32 wordCounts[B][M]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "fl_compat/flashlight.h"
#include "fl_compat/lexicon.h"
#include "fl_compat/lm.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 7) { std::cerr << "usage: decode_lex_caller <in.bin> <out.bin> <tokens file> <lexicon file> <arpa> <sil or ->\n"; return 2; }
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

  std::vector<std::string> tokens;
  std::ifstream tf(argv[3]);
  for (std::string line; std::getline(tf, line);)
    if (!line.empty()) tokens.push_back(line);
  const std::string sil = std::string(argv[6]) == "-" ? "" : argv[6];
  Lexicon plain = Lexicon::fromFile(argv[4], tokens, nullptr, sil, "none");
  NGramLM lm = NGramLM::fromArpa(argv[5], plain.words());
  Lexicon lex = Lexicon::fromFile(argv[4], tokens, &lm, sil);
  if (!lex.smeared() || plain.smeared() || lex.numNodes() != plain.numNodes()) { std::cerr << "smearing flags\n"; return 1; }

  CTCLoss crit(CriterionScaleMode::NONE);
  CTCLoss::BeamSearchOptions opt;
  opt.beamSize = W;
  opt.beamSizeToken = K;
  opt.beamThreshold = fl4[0];
  opt.logAdd = hd[8] != 0;
  opt.normalize = hd[9];
  opt.nbest = M;
  opt.maxLen = Lmax;
  opt.lm = &lm;
  opt.lmWeight = fl4[1];
  opt.lexicon = &lex;
  opt.wordScore = fl4[2];
  opt.eosScore = fl4[3];
  opt.maxWords = maxWords;
  af::array emission(af::dim4(N, T, B), em);
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  for (int pass = 0; pass < 2; ++pass) {
    auto r = crit.beamSearch(emission, pass == 0 ? af::array(af::dim4(1, B), frames) : af::array(), opt);
    if (r.labels.dims(0) != Lmax || r.labels.dims(1) != M || r.labels.dims(2) != B || r.words.dims(0) != maxWords || r.words.dims(1) != M ||
        r.words.dims(2) != B || r.wordCounts.dims(0) != M || r.wordCounts.dims(1) != B || r.words.type() != af::s32 ||
        r.lmScores.dims(0) != M || r.lmScores.dims(1) != B) {
      std::cerr << "result dims / types\n";
      return 1;
    }
    std::vector<int> lab((size_t)B * M * Lmax), len((size_t)B * M), wd((size_t)B * M * maxWords), wc((size_t)B * M);
    std::vector<float> sc((size_t)B * M), ls((size_t)B * M);
    r.labels.host(lab.data());
    r.lengths.host(len.data());
    r.scores.host(sc.data());
    r.lmScores.host(ls.data());
    r.words.host(wd.data());
    r.wordCounts.host(wc.data());
    // the host LM walked along a hypothesis's words gives the kernel's lmScores, bit for bit
    for (int b = 0; b < B; ++b)
      if (wc[(size_t)b * M] >= 0 && wc[(size_t)b * M] <= maxWords) {
        const int* row = wd.data() + (size_t)b * M * maxWords;
        const std::vector<int> ids(row, row + wc[(size_t)b * M]);
        if (lm.sentence(ids) != ls[(size_t)b * M]) { std::cerr << "lmScores != NGramLM::sentence over the words\n"; return 1; }
        if (lex.wordIds2Words(std::vector<int>(row, row + maxWords)).size() != ids.size()) { std::cerr << "wordIds2Words\n"; return 1; }
      }
    fwrite(lab.data(), 4, lab.size(), out);
    fwrite(len.data(), 4, len.size(), out);
    fwrite(sc.data(), 4, sc.size(), out);
    fwrite(ls.data(), 4, ls.size(), out);
    fwrite(wd.data(), 4, wd.size(), out);
    fwrite(wc.data(), 4, wc.size(), out);
  }
  fclose(out);
  int refused = 0;
  {   // without lexicon the call is the LM search: no words, and the lexicon options are refused
    auto o = opt; o.lexicon = nullptr; o.lm = nullptr; o.lmWeight = 0.f; o.eosScore = 0.f; o.wordScore = 0.f; o.maxWords = 0;
    auto r = crit.beamSearch(emission, af::array(), o);
    if (!r.words.isempty() || !r.wordCounts.isempty()) { std::cerr << "words without lexicon\n"; return 1; }
    o.wordScore = 0.5f;
    try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; }
  }
  { auto o = opt; o.lm = nullptr; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  { auto o = opt; o.wordScore = 1.0f / 0.0f; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  { auto o = opt; o.classScore = af::array(af::dim4(N - 1), em); try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  { auto o = opt; o.beamSize = 65; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) {} catch (const std::runtime_error&) { ++refused; } }
  {
    NGramLM other = NGramLM::fromArpa(argv[5], tokens);   // a LM over the tokens, not over the words
    if (other.numTokens() != lex.numWords()) {
      auto o = opt; o.lm = &other;
      try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; }
    } else {
      ++refused;
    }
  }
  if (refused != 6) { std::cerr << "expected six refusals, got " << refused << "\n"; return 1; }
  std::cout << "decode lex caller ok" << std::endl;
  return 0;
}
