// Compiled C++ caller of fl::pkg::speech::CTCLoss::beamSearch (include/fl_compat/flashlight.h), built with plain g++ against
// libw2l_hip.so and driven by tests/test_gpu_ctc_beam.py, which writes the inputs, runs this binary and compares its hypotheses
// with the C ABI's and the Python front end's.
//
//   decode_caller <in.bin> <out.bin>
//       in : int32 N T B W K M Lmax logAdd normalize | float threshold | float em[B][T][N] | int32 frames[B]
//       out: twice (inputSizes = frames as (1, B), then no inputSizes):
//            int32 labels[B][M][Lmax] | int32 lengths[B][M] | float scores[B][M]
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 3) { std::cerr << "usage: decode_caller <in.bin> <out.bin>\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int N = hd[0], T = hd[1], B = hd[2], W = hd[3], K = hd[4], M = hd[5], Lmax = hd[6];
  const float* em = (const float*)(hd + 10);
  const int* frames = (const int*)(em + (size_t)B * T * N);

  CTCLoss crit(CriterionScaleMode::NONE);
  CTCLoss::BeamSearchOptions opt;
  opt.beamSize = W;
  opt.beamSizeToken = K;
  opt.beamThreshold = *(const float*)(hd + 9);
  opt.logAdd = hd[7] != 0;
  opt.normalize = hd[8];
  opt.nbest = M;
  opt.maxLen = Lmax;
  af::array emission(af::dim4(N, T, B), em);
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  for (int pass = 0; pass < 2; ++pass) {
    auto r = crit.beamSearch(emission, pass == 0 ? af::array(af::dim4(1, B), frames) : af::array(), opt);
    if (r.labels.dims(0) != Lmax || r.labels.dims(1) != M || r.labels.dims(2) != B || r.labels.type() != af::s32 ||
        r.lengths.dims(0) != M || r.lengths.dims(1) != B || r.lengths.type() != af::s32 || r.scores.dims(0) != M ||
        r.scores.dims(1) != B || r.scores.type() != af::f32) {
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
  }
  fclose(out);
  // error behaviour: std::invalid_argument on bad inputSizes or options the search refuses, std::runtime_error beyond its limits
  int refused = 0;
  try { crit.beamSearch(emission, af::array(af::dim4(B + 1), (const int*)em), opt); } catch (const std::invalid_argument&) { ++refused; }
  { auto o = opt; o.nbest = W + 1; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  { auto o = opt; o.beamThreshold = -1.f; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) { ++refused; } }
  { auto o = opt; o.beamSize = 65; try { crit.beamSearch(emission, af::array(), o); } catch (const std::invalid_argument&) {} catch (const std::runtime_error&) { ++refused; } }
  if (refused != 4) { std::cerr << "expected four refusals, got " << refused << "\n"; return 1; }
  std::cout << "decode caller ok" << std::endl;
  return 0;
}
