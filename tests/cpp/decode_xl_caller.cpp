// Compiled C++ caller of BeamSearchOptions::xl (include/fl_compat/flashlight.h): CTCLoss::beamSearch with a lexicon and a word LM,
// and ASGLoss::beamSearch with a token LM, both on the xl kernels (W above 1024).  Built with plain g++ against libw2l_hip.so and
// driven by tests/test_gpu_beam_xl.py, which writes the inputs, runs this binary and compares its hypotheses with the Python front
// end's (the C ABI's w2l_ctc_beam_search_lex_xl and w2l_asg_beam_search_xl).
//
//   decode_xl_caller ctc_lex|asg_lm <in.bin> <out.bin> <tokens file> <lexicon file> <arpa>
//       ctc_lex: the arpa is over the lexicon's words, the last token of the tokens file is the silence; asg_lm: over the tokens
//       in : int32 N T B W K M Lmax maxWords | int32 frames[B] | float em[B][T][N] | float trans[N][N] (read by asg_lm)
//       out: int32 labels[B][M][Lmax] | int32 lengths[B][M] | float scores[B][M] | float lmScores[B][M] |
//            ctc_lex: int32 words[B][M][maxWords] | int32 wordCounts[B][M]
//   The options the driver uses on its side: threshold 6, logAdd, normalize for CTC only, lmWeight 0.75, eosScore -0.25, wordScore 0.5.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "fl_compat/flashlight.h"
#include "fl_compat/lexicon.h"
#include "fl_compat/lm.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 7) { std::cerr << "usage: decode_xl_caller ctc_lex|asg_lm <in.bin> <out.bin> <tokens> <lexicon> <arpa>\n"; return 2; }
  const std::string mode = argv[1];
  const bool lexMode = mode == "ctc_lex";
  if (!lexMode && mode != "asg_lm") { std::cerr << "mode " << mode << "\n"; return 2; }
  FILE* f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int N = hd[0], T = hd[1], B = hd[2], W = hd[3], K = hd[4], M = hd[5], Lmax = hd[6], maxWords = hd[7];
  const int* frames = hd + 8;
  const float* em = (const float*)(frames + B);
  const float* trans = em + (size_t)B * T * N;

  std::vector<std::string> tokens;
  std::ifstream tf(argv[4]);
  for (std::string line; std::getline(tf, line);)
    if (!line.empty()) tokens.push_back(line);
  std::unique_ptr<NGramLM> lm;
  std::unique_ptr<Lexicon> lex;
  if (lexMode) {
    lex.reset(new Lexicon(Lexicon::fromFile(argv[5], tokens, nullptr, tokens.back(), "none")));
    lm.reset(new NGramLM(NGramLM::fromArpa(argv[6], lex->words())));
    lex.reset(new Lexicon(Lexicon::fromFile(argv[5], tokens, lm.get(), tokens.back(), "max")));
  } else {
    lm.reset(new NGramLM(NGramLM::fromArpa(argv[6], tokens)));
  }

  BeamSearchOptions opt;
  opt.beamSize = W;
  opt.xl = true;
  opt.beamSizeToken = K;
  opt.beamThreshold = 6.0f;
  opt.logAdd = true;
  opt.normalize = lexMode ? 1 : 0;
  opt.nbest = M;
  opt.maxLen = Lmax;
  opt.lm = lm.get();
  opt.lmWeight = 0.75f;
  opt.eosScore = -0.25f;
  if (lexMode) {
    opt.lexicon = lex.get();
    opt.wordScore = 0.5f;
    opt.maxWords = maxWords;
  }
  af::array emission(af::dim4(N, T, B), em);
  af::array sizes(af::dim4(1, B), frames);
  BeamSearchResult r;
  if (lexMode) {
    CTCLoss crit;
    r = crit.beamSearch(emission, sizes, opt);
  } else {
    ASGLoss crit(N, CriterionScaleMode::NONE, 0.0);
    crit.setParams(Variable(af::array(af::dim4(N, N), trans), true), 0);
    r = crit.beamSearch(emission, sizes, opt);
    // without `xl` the same width is beyond the narrow kernels, and with `wide` in its place beyond the wide ones; with `xl` 8193
    // is beyond the xl ones; both families at once are refused as an argument
    int refused = 0;
    { auto o = opt; o.xl = false; try { crit.beamSearch(emission, sizes, o); } catch (const std::runtime_error&) { ++refused; } }
    { auto o = opt; o.xl = false; o.wide = true; try { crit.beamSearch(emission, sizes, o); } catch (const std::runtime_error&) { ++refused; } }
    { auto o = opt; o.beamSize = 8193; try { crit.beamSearch(emission, sizes, o); } catch (const std::runtime_error&) { ++refused; } }
    { auto o = opt; o.nbest = W + 1; try { crit.beamSearch(emission, sizes, o); } catch (const std::invalid_argument&) { ++refused; } }
    { auto o = opt; o.wide = true; try { crit.beamSearch(emission, sizes, o); } catch (const std::invalid_argument&) { ++refused; } }
    if (W > 1024 && refused != 5) { std::cerr << "expected five refusals, got " << refused << "\n"; return 1; }
  }
  if (r.labels.dims(0) != Lmax || r.labels.dims(1) != M || r.labels.dims(2) != B || r.lmScores.isempty() || r.words.isempty() != !lexMode) {
    std::cerr << "result dims / types\n";
    return 1;
  }
  FILE* out = fopen(argv[3], "wb");
  if (!out) { perror(argv[3]); return 2; }
  std::vector<int> lab((size_t)B * M * Lmax), len((size_t)B * M);
  std::vector<float> sc((size_t)B * M), ls((size_t)B * M);
  r.labels.host(lab.data());
  r.lengths.host(len.data());
  r.scores.host(sc.data());
  r.lmScores.host(ls.data());
  fwrite(lab.data(), 4, lab.size(), out);
  fwrite(len.data(), 4, len.size(), out);
  fwrite(sc.data(), 4, sc.size(), out);
  fwrite(ls.data(), 4, ls.size(), out);
  if (lexMode) {
    std::vector<int> wd((size_t)B * M * maxWords), wc((size_t)B * M);
    r.words.host(wd.data());
    r.wordCounts.host(wc.data());
    fwrite(wd.data(), 4, wd.size(), out);
    fwrite(wc.data(), 4, wc.size(), out);
  }
  fclose(out);
  std::cout << "decode xl caller ok" << std::endl;
  return 0;
}
