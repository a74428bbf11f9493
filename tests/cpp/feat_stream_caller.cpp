// Compiled C++ caller of fl::pkg::speech::StreamingFeatures (include/fl_compat/flashlight.h, fl_compat/audio.h), built with plain
// g++ against libw2l_hip.so and driven by tests/test_gpu_feat_stream.py, which writes the inputs, runs this binary and compares
// its features with the C ABI's and the Python front end's.  The tables are the ones fl::lib::audio::Mfsc computes; they are
// written out so that the other two surfaces can bind the same numbers.
//
//   feat_stream_caller <in.bin> <out.bin>
//       in : int32 fs frameMs strideMs F usePower S maxSamples steps | per step: int32 n[S] start[S] finish[S] | float pcm[S][maxSamples]
//       out: int32 maxOut N St nbins ldSpec | float G[N][2 nbins] | float H[ldSpec][F] | per step: int32 nOut[S] | float feats[S][F][maxOut]
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "fl_compat/audio.h"
#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 3) { std::cerr << "usage: feat_stream_caller <in.bin> <out.bin>\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int S = hd[5], maxSamples = hd[6], steps = hd[7];
  fl::lib::audio::FeatureParams fp;
  fp.samplingFreq = hd[0]; fp.frameSizeMs = hd[1]; fp.frameStrideMs = hd[2]; fp.numFilterbankChans = hd[3]; fp.usePower = hd[4] != 0;
  const int F = fp.numFilterbankChans;
  const char* p = (const char*)(hd + 8);

  fl::lib::audio::Mfsc mfsc(fp);
  StreamingFeatures feats(mfsc, S, maxSamples);
  if (feats.slots() != S || feats.maxSamples() != maxSamples || feats.numFeatures() != F || feats.maxOut() != (maxSamples - 1) / mfsc.frameStride() + 1) {
    std::cerr << "session geometry\n";
    return 1;
  }
  const int maxOut = feats.maxOut();
  // a streaming network over these features takes the step's output as it is: one strided convolution, maxChunk == maxOut
  auto net = buildSequentialModuleFromText("V -1 NFEAT 1 0\nC2 1 2 3 1 2 1 0 0\nR\nRO 2 1 0 3\nV " + std::to_string(2 * F) + " -1 1 0\nL " +
                                           std::to_string(2 * F) + " NLABEL\n", F, 5);
  net->eval();
  StreamingSession sess(net, S, maxOut);

  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  const int head[5] = {maxOut, mfsc.frameSize(), mfsc.frameStride(), mfsc.numBins(), mfsc.spectrumRows()};
  fwrite(head, 4, 5, out);
  std::vector<float> G((size_t)mfsc.spectrumTable().elements()), H((size_t)mfsc.melTable().elements());
  if (G.size() != (size_t)head[1] * 2 * head[3] || H.size() != (size_t)head[4] * F) { std::cerr << "table dims\n"; return 1; }
  mfsc.spectrumTable().host(G.data());
  mfsc.melTable().host(H.data());
  fwrite(G.data(), 4, G.size(), out);
  fwrite(H.data(), 4, H.size(), out);
  std::vector<float> y((size_t)S * F * maxOut);
  long emitted = 0;
  for (int i = 0; i < steps; ++i) {
    const int* c = (const int*)p;
    std::vector<int> cnt(c, c + S), st(c + S, c + 2 * S), fi(c + 2 * S, c + 3 * S), nOut, nEm;
    const float* x = (const float*)(c + 3 * S);
    p = (const char*)(x + (size_t)S * maxSamples);
    af::array pcm(af::dim4(maxSamples, S), x);
    af::array e = feats.step(pcm, cnt, st, fi, nOut);
    if (e.dims(0) != maxOut || e.dims(1) != F || e.dims(3) != S || e.type() != af::f32) { std::cerr << "feature dims\n"; return 1; }
    e.host(y.data());
    fwrite(nOut.data(), 4, (size_t)S, out);
    fwrite(y.data(), 4, y.size(), out);
    sess.step(e, nOut, st, fi, nEm);   // throws if the hand-over does not fit
    for (int s = 0; s < S; ++s) emitted += nEm[s];
  }
  fclose(out);
  if (p != buf.data() + n) { std::cerr << "input not consumed\n"; return 1; }
  if (emitted < 1) { std::cerr << "the streaming network emitted nothing\n"; return 1; }
  // error behaviour: std::invalid_argument for a chunk above maxSamples and for samples on a slot that was never started;
  // std::runtime_error naming the field for a geometry beyond the kernel
  int refused = 0;
  std::vector<int> nOut;
  af::array pcm(af::dim4(maxSamples, S), std::vector<float>((size_t)S * maxSamples, 0.f).data());
  try { feats.step(pcm, std::vector<int>(S, maxSamples + 1), std::vector<int>(S, 1), {}, nOut); } catch (const std::invalid_argument&) { ++refused; }
  feats.reset(0);
  bool active = true;
  int carry = -1;
  feats.slotState(0, active, carry);
  if (active || carry != 0) { std::cerr << "reset left the slot open\n"; return 1; }
  try { feats.step(pcm, std::vector<int>(S, 1), {}, {}, nOut); } catch (const std::invalid_argument&) { ++refused; }
  try {
    fl::lib::audio::FeatureParams big = fp;
    big.numFilterbankChans = 129;
    fl::lib::audio::Mfsc m2(big);
    StreamingFeatures f2(m2, 1, 160);
  } catch (const std::invalid_argument&) {
  } catch (const std::runtime_error& e) {
    if (std::string(e.what()).find("numFilters") != std::string::npos) ++refused;
  }
  if (refused != 3) { std::cerr << "expected three refusals, got " << refused << "\n"; return 1; }
  std::cout << "feat stream caller ok" << std::endl;
  return 0;
}
