// Compiled C++ caller of BeamSearchOptions::manyTokens (include/fl_compat/flashlight.h): CTCLoss::beamSearch and
// ASGLoss::beamSearch without LM on the many-token kernels (K above 64), with a silence score when the driver gives one.  Built
// with plain g++ against libw2l_hip.so and driven by tests/test_gpu_beam_mt.py, which writes the inputs, runs this binary and
// compares its hypotheses with the Python front end's (the C ABI's w2l_ctc_beam_search_mt and w2l_asg_beam_search_mt).
//
//   decode_mt_caller ctc|asg <in.bin> <out.bin>
//       in : int32 N T B W K M Lmax silToken | float silScore | int32 frames[B] | float em[B][T][N] | float trans[N][N] (read by asg)
//       out: int32 labels[B][M][Lmax] | int32 lengths[B][M] | float scores[B][M]
//   The options the driver uses on its side: threshold 6, the max search on the raw emissions.
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 4) { std::cerr << "usage: decode_mt_caller ctc|asg <in.bin> <out.bin>\n"; return 2; }
  const std::string mode = argv[1];
  const bool asg = mode == "asg";
  if (!asg && mode != "ctc") { std::cerr << "mode " << mode << "\n"; return 2; }
  FILE* f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int N = hd[0], T = hd[1], B = hd[2], W = hd[3], K = hd[4], M = hd[5], Lmax = hd[6], silToken = hd[7];
  const float silScore = *(const float*)(hd + 8);
  const int* frames = hd + 9;
  const float* em = (const float*)(frames + B);
  const float* trans = em + (size_t)B * T * N;

  BeamSearchOptions opt;
  opt.beamSize = W;
  opt.manyTokens = true;
  opt.beamSizeToken = K;
  opt.beamThreshold = 6.0f;
  opt.logAdd = false;
  opt.normalize = 0;
  opt.nbest = M;
  opt.maxLen = Lmax;
  opt.silToken = silToken;
  opt.silScore = silScore;
  af::array emission(af::dim4(N, T, B), em);
  af::array sizes(af::dim4(1, B), frames);
  BeamSearchResult r;
  int refused = 0;
  if (!asg) {
    CTCLoss crit;
    r = crit.beamSearch(emission, sizes, opt);
    // without manyTokens K is beyond every other family; with it 257 tokens (N allowing) and 8193 entries are beyond this one
    { auto o = opt; o.manyTokens = false; o.xl = true; try { crit.beamSearch(emission, sizes, o); } catch (const std::runtime_error&) { ++refused; } }
    { auto o = opt; o.beamSize = 8193; try { crit.beamSearch(emission, sizes, o); } catch (const std::runtime_error&) { ++refused; } }
    { auto o = opt; o.xl = true; try { crit.beamSearch(emission, sizes, o); } catch (const std::invalid_argument&) { ++refused; } }
    if (K > 64 && N - 1 > 64 && refused != 3) { std::cerr << "expected three refusals, got " << refused << "\n"; return 1; }
  } else {
    ASGLoss crit(N, CriterionScaleMode::NONE, 0.0);
    crit.setParams(Variable(af::array(af::dim4(N, N), trans), true), 0);
    r = crit.beamSearch(emission, sizes, opt);
  }
  if (r.labels.dims(0) != Lmax || r.labels.dims(1) != M || r.labels.dims(2) != B) { std::cerr << "result dims\n"; return 1; }
  FILE* out = fopen(argv[3], "wb");
  if (!out) { perror(argv[3]); return 2; }
  std::vector<int> lab((size_t)B * M * Lmax), len((size_t)B * M);
  std::vector<float> sc((size_t)B * M);
  r.labels.host(lab.data());
  r.lengths.host(len.data());
  r.scores.host(sc.data());
  fwrite(lab.data(), 4, lab.size(), out);
  fwrite(len.data(), 4, len.size(), out);
  fwrite(sc.data(), 4, sc.size(), out);
  fclose(out);
  std::cout << "decode mt caller ok" << std::endl;
  return 0;
}
