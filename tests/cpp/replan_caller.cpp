// Compiled C++ caller of the fl:: surface (include/fl_compat/flashlight.h), built with plain g++ against libw2l_hip.so and driven by
// tests/test_gpu_replan.py: ONE network put through a sequence of batch shapes against networks built fresh for each shape.
//
//   train mode: S1, S2, S1 -- a forward, the CTC criterion and loss.backward() at each; the planned network plans again whenever
//               (B, T) changes, and the third pass returns to the first shape
//   eval mode:  three shapes, the largest first -- the eval-mode graph keeps one arena that only ever grows, so the second and third
//               run in an arena sized for another plan
// Every network is built from the same arch text (no dropout) and initialised with the same seed, so the emissions of the one that
// re-planned and every parameter gradient must be, bit for bit, those of the fresh one.  Prints OK.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

#define EXPECT(c) do { if (!(c)) { std::cerr << "replan_caller: " #c " failed (line " << __LINE__ << ")\n"; return 1; } } while (0)

static const int kFeat = 8, kLabel = 12;
static const char* kArch =
    "V -1 NFEAT 1 0\nC2 1 4 5 1 2 1 -1 -1\nR\nDO 0.0\nLN 0 1 2\nTDS 4 5 8 0.0 64\nTDS 4 5 8 0.0 0\nV 0 32 1 0\nRO 1 0 3 2\nL 32 NLABEL\n";

struct Shape { int B, T, L; };

static std::vector<float> hostOf(const af::array& a) {
  std::vector<float> h((size_t)a.elements());
  a.host(h.data());
  return h;
}
static bool sameBits(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

struct Batch {
  std::vector<float> x;
  std::vector<int> tgt;
  Batch(const Shape& s, uint32_t seed) : x((size_t)s.B * kFeat * s.T), tgt((size_t)s.B * s.L) {
    uint32_t r = seed;
    auto next = [&r]() { r = r * 1664525u + 1013904223u; return (float)((r >> 8) + 0.5) / 8388608.f - 1.f; };   // (-1, 1)
    for (auto& v : x) v = next();
    for (auto& t : tgt) t = (int)((next() + 1.f) * 0.5f * (kLabel - 1));
  }
};

struct Pass {
  std::vector<float> emissions;
  std::vector<std::vector<float>> grads;
};

// one pass of `network` on the batch: train mode with the criterion and a backward pass, or eval mode (emissions only)
static Pass run(const std::shared_ptr<Sequential>& network, const Shape& s, const Batch& b, bool train) {
  Pass p;
  Variable input = fl::input(af::array(af::dim4(s.T, kFeat, 1, s.B), b.x.data()));
  if (train) network->train(); else network->eval();
  auto output = network->forward({input, fl::noGrad(af::constant(s.T, af::dim4(1, s.B)))}).front();
  p.emissions = hostOf(output.array());
  if (train) {
    CTCLoss criterion(getCriterionScaleMode("target", true));
    Variable target(af::array(af::dim4(s.L, s.B), b.tgt.data()), false);
    auto loss = criterion.forward({output, target}).front();
    for (auto& q : network->params()) q.zeroGrad();
    loss.backward();
    for (auto& q : network->params()) {
      if (!q.isGradAvailable()) throw std::runtime_error("a parameter has no gradient");
      p.grads.push_back(hostOf(q.grad().array()));
    }
  }
  return p;
}

int main() {
  try {
    const Shape trainSeq[3] = {{3, 64, 6}, {2, 41, 3}, {3, 64, 6}};
    const Shape evalSeq[3] = {{4, 90, 1}, {1, 33, 1}, {2, 64, 1}};
    auto network = buildSequentialModuleFromText(kArch, kFeat, kLabel);
    for (int k = 0; k < 3; ++k) {
      const Batch b(trainSeq[k], 100u + k);
      const Pass got = run(network, trainSeq[k], b, true);
      const Pass want = run(buildSequentialModuleFromText(kArch, kFeat, kLabel), trainSeq[k], b, true);
      EXPECT(!got.emissions.empty() && sameBits(got.emissions, want.emissions));
      EXPECT(got.grads.size() == want.grads.size() && !got.grads.empty());
      bool moved = false;
      for (size_t i = 0; i < got.grads.size(); ++i) {
        EXPECT(sameBits(got.grads[i], want.grads[i]));
        for (float v : got.grads[i]) { EXPECT(v == v); moved = moved || v != 0.f; }
      }
      EXPECT(moved);
    }
    for (int k = 0; k < 3; ++k) {   // the same network, now in eval mode: a graph and an arena of its own
      const Batch b(evalSeq[k], 200u + k);
      const Pass got = run(network, evalSeq[k], b, false);
      const Pass want = run(buildSequentialModuleFromText(kArch, kFeat, kLabel), evalSeq[k], b, false);
      EXPECT(got.emissions.size() == (size_t)kLabel * ((evalSeq[k].T + 1) / 2) * evalSeq[k].B);
      EXPECT(sameBits(got.emissions, want.emissions));
    }
    // back in train mode at the first shape after the eval passes: the training graph was not disturbed
    {
      const Batch b(trainSeq[0], 300u);
      const Pass got = run(network, trainSeq[0], b, true);
      const Pass want = run(buildSequentialModuleFromText(kArch, kFeat, kLabel), trainSeq[0], b, true);
      EXPECT(sameBits(got.emissions, want.emissions));
      for (size_t i = 0; i < got.grads.size(); ++i) EXPECT(sameBits(got.grads[i], want.grads[i]));
    }
  } catch (const std::exception& e) {
    std::cerr << "replan_caller: " << e.what() << "\n";
    return 1;
  }
  std::cout << "OK" << std::endl;
  return 0;
}
