// Compiled C++ caller of fl::pkg::speech::localNormalize and StreamingLocalNorm (include/fl_compat/flashlight.h), built with plain
// g++ against libw2l_hip.so and driven by tests/test_gpu_local_norm.py, which writes the input, runs this binary and compares its
// output with the C ABI's and the Python front end's, byte for byte.
//
//   local_norm_caller <in.bin> <out.bin>
//       in : int32 B F T left right chunk | int32 frames[B] | float x[B][F][T]
//       out: float batch[B][F][T]   localNormalize(x, frames, left, right)
//            float stream[B][F][T]  StreamingLocalNorm(F, B, chunk, left) over chunks of `chunk` frames, slot b = utterance b, frames
//                                   at or beyond frames[b] zero
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 3) { std::cerr << "usage: local_norm_caller <in.bin> <out.bin>\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int B = hd[0], F = hd[1], T = hd[2], left = hd[3], right = hd[4], chunk = hd[5];
  if ((size_t)n != (6 + (size_t)B) * 4 + (size_t)B * F * T * 4) { std::cerr << "input size\n"; return 1; }
  std::vector<int> frames(hd + 6, hd + 6 + B);
  const float* x = (const float*)(hd + 6 + B);

  af::array X(af::dim4(T, F, 1, B), x);
  af::array Y = localNormalize(X, frames, left, right);
  if (Y.dims(0) != T || Y.dims(1) != F || Y.dims(3) != B || Y.type() != af::f32) { std::cerr << "batch dims\n"; return 1; }
  std::vector<float> y((size_t)B * F * T), z((size_t)B * F * T, 0.f), c((size_t)B * F * chunk);
  Y.host(y.data());

  StreamingLocalNorm norm(F, B, chunk, left);
  if (norm.slots() != B || norm.maxChunk() != chunk || norm.numFeatures() != F) { std::cerr << "session geometry\n"; return 1; }
  for (int t0 = 0; t0 < T; t0 += chunk) {
    std::vector<int> cnt((size_t)B), st((size_t)B, t0 == 0 ? 1 : 0);
    for (int b = 0; b < B; ++b) {
      cnt[(size_t)b] = std::max(0, std::min(chunk, frames[(size_t)b] - t0));
      for (int ft = 0; ft < F; ++ft)
        for (int j = 0; j < chunk; ++j) c[((size_t)b * F + ft) * chunk + j] = t0 + j < T ? x[((size_t)b * F + ft) * T + t0 + j] : 0.f;
    }
    af::array C(af::dim4(chunk, F, 1, B), c.data());
    norm.step(C, cnt, st);
    C.host(c.data());
    for (int b = 0; b < B; ++b)
      for (int ft = 0; ft < F; ++ft)
        for (int j = 0; j < cnt[(size_t)b]; ++j) z[((size_t)b * F + ft) * T + t0 + j] = c[((size_t)b * F + ft) * chunk + j];
  }
  bool active = false;
  long long seen = -1;
  norm.slotState(0, active, seen);
  if (!active || seen != std::max(0, std::min(frames[0], T))) { std::cerr << "slot state\n"; return 1; }

  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  fwrite(y.data(), 4, y.size(), out);
  fwrite(z.data(), 4, z.size(), out);
  fclose(out);

  // error behaviour: std::invalid_argument for a right context (naming the reference's refusal), for a chunk above maxChunk, for
  // frames on a slot that was reset and for a negative context; std::runtime_error for a window above 65536 frames
  int refused = 0;
  try { StreamingLocalNorm bad(F, 1, 4, 3, 1); } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("LocalNorm.cpp:33") != std::string::npos) ++refused;
  }
  af::array C(af::dim4(chunk + 1, F, 1, B), std::vector<float>((size_t)B * F * (chunk + 1), 0.f).data());
  try { norm.step(C, std::vector<int>((size_t)B, chunk + 1), {}); } catch (const std::invalid_argument&) { ++refused; }
  norm.reset(0);
  try { norm.step(C, std::vector<int>((size_t)B, 1), {}); } catch (const std::invalid_argument&) { ++refused; }
  try { localNormalize(X, frames, -1, 0); } catch (const std::invalid_argument&) { ++refused; }
  try { localNormalize(X, frames, 65536, 0); } catch (const std::invalid_argument&) {
  } catch (const std::runtime_error&) { ++refused; }
  if (refused != 5) { std::cerr << "expected five refusals, got " << refused << "\n"; return 1; }
  std::cout << "local norm caller ok" << std::endl;
  return 0;
}
