// Compiled C++ caller of fl::pkg::speech::CTCLoss::viterbiPathWithTarget (include/fl_compat/flashlight.h), built with plain g++
// against libw2l_hip.so and driven by tests/test_gpu_ctc_align.py, which writes the inputs, runs this binary and compares its
// paths with the C ABI's and the Python front end's.
//
//   align_caller <in.bin> <out.bin>
//       in : int32 N T B L | float em[B][T][N] | int32 target[B][L] | int32 frames[B]
//       out: int32 path[B][T] (inputSizes = frames as (1, B)) | int32 path[B][T] (frames as (B)) | int32 path[B][T] (no inputSizes)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 3) { std::cerr << "usage: align_caller <in.bin> <out.bin>\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int N = hd[0], T = hd[1], B = hd[2], L = hd[3];
  const float* em = (const float*)(hd + 4);
  const int* tgt = (const int*)(em + (size_t)B * T * N);
  const int* frames = tgt + (size_t)B * L;

  std::shared_ptr<SequenceCriterion> crit = std::make_shared<CTCLoss>(CriterionScaleMode::NONE);
  af::array emission(af::dim4(N, T, B), em), target(af::dim4(L, B), tgt);
  std::vector<int> hp((size_t)B * T);
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  crit->viterbiPathWithTarget(emission, target, af::array(af::dim4(1, B), frames)).host(hp.data());
  fwrite(hp.data(), 4, hp.size(), out);
  crit->viterbiPathWithTarget(emission, target, af::array(af::dim4(B), frames)).host(hp.data());
  fwrite(hp.data(), 4, hp.size(), out);
  af::array path = crit->viterbiPathWithTarget(emission, target);
  if (path.dims(0) != T || path.dims(1) != B || path.type() != af::s32) { std::cerr << "path dims / type\n"; return 1; }
  path.host(hp.data());
  fwrite(hp.data(), 4, hp.size(), out);
  fclose(out);
  // error behaviour: std::invalid_argument on a bad target type / batch or a bad inputSizes, the wording of ASGLoss
  int refused = 0;
  try { crit->viterbiPathWithTarget(emission, af::array(af::dim4(L, B), (const float*)tgt)); } catch (const std::invalid_argument&) { ++refused; }
  try { crit->viterbiPathWithTarget(emission, af::array(af::dim4(L * B, 1), tgt)); } catch (const std::invalid_argument&) { ++refused; }
  try { crit->viterbiPathWithTarget(emission, target, af::array(af::dim4(B + 1), tgt)); } catch (const std::invalid_argument&) { ++refused; }
  if (refused != 3) { std::cerr << "expected three std::invalid_argument, got " << refused << "\n"; return 1; }
  std::cout << "align caller ok" << std::endl;
  return 0;
}
