// Compiled C++ caller of fl::pkg::speech::CTCLoss::beamSearch with an n-gram LM (include/fl_compat/flashlight.h, fl_compat/lm.h),
// built with plain g++ against libw2l_hip.so and driven by tests/test_gpu_ctc_beam_lm.py, which writes the inputs and the ARPA
// file, runs this binary and compares its hypotheses with the C ABI's and the Python front end's.
//
//   decode_lm_caller <in.bin> <out.bin> <tokens file> <arpa>
//       in : int32 N T B W K M Lmax logAdd normalize hasClassScore | float threshold lmWeight eosScore | float em[B][T][N] |
//            int32 frames[B] | float classScore[N-1]
//       out: twice (inputSizes = frames as (1, B), then no inputSizes):
//            int32 labels[B][M][Lmax] | int32 lengths[B][M] | float scores[B][M] | float lmScores[B][M]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "fl_compat/flashlight.h"
#include "fl_compat/lm.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 5) { std::cerr << "usage: decode_lm_caller <in.bin> <out.bin> <tokens file> <arpa>\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int N = hd[0], T = hd[1], B = hd[2], W = hd[3], K = hd[4], M = hd[5], Lmax = hd[6], hasCls = hd[9];
  const float* fl3 = (const float*)(hd + 10);
  const float* em = fl3 + 3;
  const int* frames = (const int*)(em + (size_t)B * T * N);
  const float* cls = (const float*)(frames + B);

  std::vector<std::string> tokens;
  std::ifstream tf(argv[3]);
  for (std::string line; std::getline(tf, line);)
    if (!line.empty()) tokens.push_back(line);
  NGramLM lm = NGramLM::fromArpa(argv[4], tokens);

  CTCLoss crit(CriterionScaleMode::NONE);
  CTCLoss::BeamSearchOptions opt;
  opt.beamSize = W;
  opt.beamSizeToken = K;
  opt.beamThreshold = fl3[0];
  opt.logAdd = hd[7] != 0;
  opt.normalize = hd[8];
  opt.nbest = M;
  opt.maxLen = Lmax;
  opt.lm = &lm;
  opt.lmWeight = fl3[1];
  opt.eosScore = fl3[2];
  if (hasCls) opt.classScore = af::array(af::dim4(N - 1), cls);
  af::array emission(af::dim4(N, T, B), em);
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  for (int pass = 0; pass < 2; ++pass) {
    auto r = crit.beamSearch(emission, pass == 0 ? af::array(af::dim4(1, B), frames) : af::array(), opt);
    if (r.labels.dims(0) != Lmax || r.labels.dims(1) != M || r.labels.dims(2) != B || r.lengths.dims(0) != M || r.lengths.dims(1) != B ||
        r.scores.dims(0) != M || r.scores.dims(1) != B || r.lmScores.dims(0) != M || r.lmScores.dims(1) != B ||
        r.lmScores.type() != af::f32) {
      std::cerr << "result dims / types\n";
      return 1;
    }
    std::vector<int> lab((size_t)B * M * Lmax), len((size_t)B * M);
    std::vector<float> sc((size_t)B * M), ls((size_t)B * M);
    r.labels.host(lab.data());
    r.lengths.host(len.data());
    r.scores.host(sc.data());
    r.lmScores.host(ls.data());
    // the host table walked along a hypothesis gives the kernel's lmScores, bit for bit
    for (int b = 0; b < B; ++b)
      if (len[(size_t)b * M] >= 0 && len[(size_t)b * M] <= Lmax) {
        const int* row = lab.data() + (size_t)b * M * Lmax;
        if (lm.sentence(std::vector<int>(row, row + len[(size_t)b * M])) != ls[(size_t)b * M]) { std::cerr << "lmScores != NGramLM::sentence\n"; return 1; }
      }
    fwrite(lab.data(), 4, lab.size(), out);
    fwrite(len.data(), 4, len.size(), out);
    fwrite(sc.data(), 4, sc.size(), out);
    fwrite(ls.data(), 4, ls.size(), out);
  }
  fclose(out);
  // without lm the call is the old one: no lmScores, and the LM options are refused
  int refused = 0;
  {
    auto o = opt; o.lm = nullptr; o.lmWeight = 0.f; o.eosScore = 0.f; o.classScore = af::array();
    if (!crit.beamSearch(emission, af::array(), o).lmScores.isempty()) { std::cerr << "lmScores without lm\n"; return 1; }
    o.lmWeight = 0.5f;
    try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; }
  }
  { auto o = opt; o.lmWeight = 1.0f / 0.0f; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  { auto o = opt; o.classScore = af::array(af::dim4(N), em); try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  { auto o = opt; o.beamSize = 65; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) {} catch (const std::runtime_error&) { ++refused; } }
  {
    tokens.push_back("one-too-many");
    try { NGramLM other = NGramLM::fromArpa(argv[4], tokens); auto o = opt; o.lm = &other; crit.beamSearch(emission, af::array(), o); }
    catch (const std::invalid_argument&) { ++refused; }
  }
  if (refused != 5) { std::cerr << "expected five refusals, got " << refused << "\n"; return 1; }
  std::cout << "decode lm caller ok" << std::endl;
  return 0;
}
