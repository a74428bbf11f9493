// Compiled C++ caller of fl::pkg::speech::StreamingSession in MIXED PRECISION (include/fl_compat/flashlight.h: mixedPrecision = true
// over a network with setMixedPrecision on), built with plain g++ against libw2l_hip.so and driven by tests/test_gpu_stream_bf16.py,
// which writes the inputs, runs this binary and compares its emissions with the C ABI's and the Python front end's.  The network is the arch text's with the parameters buildSequentialModule gives
// it (Flashlight-style init, seed 1: the Python trainer's init_params(seed=1) is the same arena).
//
//   stream_bf16_caller <in.bin> <out.bin>
//       in : int32 NFEAT NLABEL S Cmax steps archBytes | arch text, zero-padded to a multiple of 4 bytes |
//            per step: int32 n[S] start[S] finish[S] | float x[S][NFEAT][Cmax]
//       out: int32 maxOut | per step: int32 nOut[S] | float emissions[S][maxOut][NLABEL] (zeros when no slot had work)
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
  if (argc != 3) { std::cerr << "usage: stream_bf16_caller <in.bin> <out.bin>\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int nFeat = hd[0], nLabel = hd[1], S = hd[2], Cmax = hd[3], steps = hd[4], archBytes = hd[5];
  const std::string arch((const char*)(hd + 6), (size_t)archBytes);
  const char* p = (const char*)(hd + 6) + (archBytes + 3) / 4 * 4;

  auto net = buildSequentialModuleFromText(arch, nFeat, nLabel);
  net->eval();
  // the rules of the option: a mixed-precision session needs the network's mode on, an fp32 session needs it off
  int ruled = 0;
  try { StreamingSession bad(net, S, Cmax, true); } catch (const std::invalid_argument&) { ++ruled; }
  setMixedPrecision(net, true);
  try { StreamingSession bad(net, S, Cmax); } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("mixed-precision") != std::string::npos) ++ruled;
  }
  if (ruled != 2) { std::cerr << "expected two refusals of the precision option, got " << ruled << "\n"; return 1; }
  StreamingSession sess(net, S, Cmax, true);
  if (!sess.mixedPrecision()) { std::cerr << "session precision\n"; return 1; }
  sess.refreshWeights();   // before the first step: nothing to do, and nothing breaks
  if (sess.slots() != S || sess.maxChunk() != Cmax || sess.numLabels() != nLabel || sess.maxOut() < 1) { std::cerr << "session geometry\n"; return 1; }
  const int maxOut = sess.maxOut();
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  fwrite(&maxOut, 4, 1, out);
  std::vector<float> em((size_t)S * maxOut * nLabel);
  for (int i = 0; i < steps; ++i) {
    const int* c = (const int*)p;
    std::vector<int> cnt(c, c + S), st(c + S, c + 2 * S), fi(c + 2 * S, c + 3 * S), nOut;
    const float* x = (const float*)(c + 3 * S);
    p = (const char*)(x + (size_t)S * nFeat * Cmax);
    af::array feat(af::dim4(Cmax, nFeat, 1, S), x);
    af::array e = sess.step(feat, cnt, st, fi, nOut);
    std::fill(em.begin(), em.end(), 0.f);
    if (!e.isempty()) {
      if (e.dims(0) != nLabel || e.dims(1) != maxOut || e.dims(2) != S || e.type() != af::f32) { std::cerr << "emission dims\n"; return 1; }
      e.host(em.data());
    }
    fwrite(nOut.data(), 4, (size_t)S, out);
    fwrite(em.data(), 4, em.size(), out);
  }
  fclose(out);
  if (p != buf.data() + n) { std::cerr << "input not consumed\n"; return 1; }
  std::cout << "stream bf16 caller ok" << std::endl;
  return 0;
}
