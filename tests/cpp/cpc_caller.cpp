// Compiled C++ caller of fl::pkg::speech::CPCCriterion (include/fl_compat/flashlight.h), built with plain g++ against libw2l_hip.so
// and driven by tests/test_gpu_cpc.py, which writes the input, runs this binary and compares its output with the float64
// restatement and with the Python surface.
//
//   cpc_caller <in.bin> <out.bin> <checkpoint path>
//       in : int32 B T Ce Cc D nNegative maskLength seedLo seedHi nFrames | float tau maskProb | int32 frames[nFrames] (0 or B) |
//            float enc[B][T][Ce] ctx[B][T][Cc] g[B] gy[B][T][Ce] emb[Ce] We[D][Ce] be[D] Wc[D][Cc] bc[D]
//       out: int32 M K numMask | int32 maskIndex[B][M] neg[B][M][K] |
//            float masked[B][T][Ce] loss[B] denc[B][T][Ce] dctx[B][T][Cc] dWe[D][Ce] dbe[D] dWc[D][Cc] dbc[D]
//            float dx[B][T][Ce] demb[Ce]      the masking's backward for the output gradient gy
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

#define EXPECT(c) do { if (!(c)) { std::cerr << "cpc_caller: " #c " failed (line " << __LINE__ << ")\n"; return 1; } } while (0)

static std::vector<float> hostOf(const Variable& v) {
  std::vector<float> h((size_t)v.elements());
  v.host(h.data());
  return h;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::cerr << "usage: cpc_caller <in.bin> <out.bin> <checkpoint path>\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int B = hd[0], T = hd[1], Ce = hd[2], Cc = hd[3], D = hd[4], nNegative = hd[5], maskLength = hd[6], nFrames = hd[9];
  const uint64_t seed = (uint64_t)(uint32_t)hd[7] | ((uint64_t)(uint32_t)hd[8] << 32);
  const float tau = ((const float*)hd)[10], maskProb = ((const float*)hd)[11];
  std::vector<int> frames(hd + 12, hd + 12 + nFrames);
  const float* p = (const float*)(hd + 12 + nFrames);
  const size_t nEnc = (size_t)B * T * Ce, nCtx = (size_t)B * T * Cc;
  const float *enc = p, *ctx = enc + nEnc, *g = ctx + nCtx, *gy = g + B, *emb = gy + nEnc, *We = emb + Ce, *be = We + (size_t)D * Ce,
              *Wc = be + D, *bc = Wc + (size_t)D * Cc;
  EXPECT((const char*)(bc + D) == buf.data() + n);

  CPCCriterion crit(Ce, Cc, D, 1, 2, 3, nNegative, 4, tau);
  EXPECT(crit.prettyString() == "CPCCriterion");
  auto initial = crit.params();
  EXPECT(initial.size() == 5 && initial[0].dims() == af::dim4(Ce) && initial[1].dims() == af::dim4(Ce, D) && initial[2].dims() == af::dim4(D) &&
         initial[3].dims() == af::dim4(Cc, D) && initial[4].dims() == af::dim4(D));
  for (float v : hostOf(initial[0])) EXPECT(v > -1.f && v < 1.f);
  EXPECT(hostOf(crit.getMaskEmbedding()) == hostOf(initial[0]));
  crit.setParams(Variable(af::array(af::dim4(Ce), emb), true), 0);
  crit.setParams(Variable(af::array(af::dim4(Ce, D), We), true), 1);
  crit.setParams(Variable(af::array(af::dim4(D), be), true), 2);
  crit.setParams(Variable(af::array(af::dim4(Cc, D), Wc), true), 3);
  crit.setParams(Variable(af::array(af::dim4(D), bc), true), 4);

  // the fork's step: mask the encoder output, run the criterion on the unmasked output and a context, backward
  Variable encV(af::array(af::dim4(Ce, T, B), enc), true), ctxV(af::array(af::dim4(Cc, T, B), ctx), true);
  Variable masked = crit.getMask(encV, (double)maskProb, maskLength, frames, seed);
  const std::vector<int> maskIndex = crit.maskIndex(), neg = crit.negatives();
  const int M = (int)maskIndex.size() / B, K = (int)(neg.size() / maskIndex.size());
  EXPECT(crit.numMask() == B * M && masked.dims() == encV.dims());
  Variable loss = crit.forward({encV, ctxV}).front();
  EXPECT(loss.dims() == af::dim4(B));
  loss.backward(Variable(af::array(af::dim4(B), g), false));
  std::vector<std::vector<float>> out = {hostOf(masked), hostOf(loss), hostOf(encV.grad()), hostOf(ctxV.grad())};
  for (int i = 1; i < 5; ++i) out.push_back(hostOf(crit.param(i).grad()));
  // the masking's own backward, on a fresh input so that nothing accumulates
  Variable encW(af::array(af::dim4(Ce, T, B), enc), true);
  crit.zeroGrad();
  for (auto& q : crit.params()) q.zeroGrad();
  Variable again = crit.getMask(encW, (double)maskProb, maskLength, frames, seed);
  EXPECT(crit.maskIndex() == maskIndex && crit.negatives() == neg && hostOf(again) == out[0]);
  again.backward(Variable(af::array(af::dim4(Ce, T, B), gy), false));
  out.push_back(hostOf(encW.grad()));
  out.push_back(hostOf(crit.param(0).grad()));

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  const int head[3] = {M, K, crit.numMask()};
  fwrite(head, 4, 3, o);
  fwrite(maskIndex.data(), 4, maskIndex.size(), o);
  fwrite(neg.data(), 4, neg.size(), o);
  for (auto& v : out) fwrite(v.data(), 4, v.size(), o);
  fclose(o);

  // the reference's signature draws too, from the seed set + the number of calls
  crit.setSeed(seed);
  Variable m2 = crit.getMask(encW, maskProb, maskLength);
  EXPECT(crit.numMask() >= 4 * B && m2.dims() == encW.dims());
  if (frames.empty()) EXPECT(crit.maskIndex() == maskIndex);

  // what the reference does not offer
  int refused = 0;
  try { crit.viterbiPath(encV.array()); } catch (const std::logic_error&) { ++refused; }
  try { crit.getMask(encW, 1.0 / T, 3, {}, seed); } catch (const std::invalid_argument& e) {   // one start: at most 3 frames
    if (std::string(e.what()).find("M >= 4") != std::string::npos) ++refused;
  }
  try { crit.forward({encV}); } catch (const std::invalid_argument&) { ++refused; }
  try { CPCCriterion bad(Ce, Cc, D, 1, 2, 3, nNegative, 4, 0.f); } catch (const std::invalid_argument&) { ++refused; }
  EXPECT(refused == 4);

  // Serializer: the five parameters in params() order, into a criterion that starts from other values
  auto net = buildSequentialModuleFromText("V -1 1 NFEAT 0\nRO 2 0 3 1\nL 16 NLABEL\n", 16, 7);
  auto saved = std::make_shared<CPCCriterion>(Ce, Cc, D, 1, 2, 3, nNegative, 4, tau);
  for (int i = 0; i < 5; ++i) saved->setParams(crit.param(i), i);
  fl::pkg::runtime::Serializer::Config cfg{{"criterion", "cpc"}};
  fl::pkg::runtime::Serializer::save(argv[3], "test", cfg, net, saved, nullptr, nullptr);
  auto loaded = std::make_shared<CPCCriterion>(Ce, Cc, D, 1, 2, 3, nNegative, 4, tau);
  EXPECT(hostOf(loaded->param(1)) != hostOf(saved->param(1)));
  std::string version;
  fl::pkg::runtime::Serializer::Config cfg2;
  fl::pkg::runtime::Serializer::load(argv[3], version, cfg2, net, loaded);
  EXPECT(version == "test" && cfg2["criterion"] == "cpc");
  for (int i = 0; i < 5; ++i) EXPECT(hostOf(loaded->param(i)) == hostOf(saved->param(i)) && loaded->param(i).dims() == saved->param(i).dims());
  auto ctc = std::make_shared<CTCLoss>();
  try {
    fl::pkg::runtime::Serializer::load(argv[3], version, cfg2, net, ctc);
    EXPECT(false);
  } catch (const std::runtime_error&) {
  }
  std::cout << "cpc caller ok" << std::endl;
  return 0;
}
