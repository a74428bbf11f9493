// Compiled C++ caller of fl::AdamOptimizer (include/fl_compat/flashlight.h), built with plain g++ against libw2l_hip.so and driven by
// tests/test_gpu_adam.py, which compares what it writes with the float64 restatement (tests/adam_ref.py).
//
//   adam_caller <out.bin> <lr> <beta1> <beta2> <eps> <weightDecay>
//       three training steps of a small planned fl::Sequential under CTC with fl::AdamOptimizer over network->params() (the slices of
//       one flat arena: one launch per step), and the SAME gradients applied to copies of the parameters in arrays of their own (one
//       launch per parameter).  Parameters and both moments of the two must agree bit for bit after every step (checked here).
//       out: int32 nParams nSteps | int32 numel[nParams] | float p0[all] | per step: float g[all] p[all] m[all] v[all]
//   then three steps on CPCCriterion::params() (odd sizes, arrays of their own): every parameter that has a gradient changes, the
//   one that has none stays.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

#define EXPECT(c) do { if (!(c)) { std::cerr << "adam_caller: " #c " failed (line " << __LINE__ << ")\n"; return 1; } } while (0)

static std::vector<float> hostOf(const af::array& a) {
  std::vector<float> h((size_t)a.elements());
  a.host(h.data());
  return h;
}
static std::vector<float> hostOf(const Variable& v) { return hostOf(v.array()); }

static uint32_t g_rng = 12345u;
static float uniform() {   // (-1, 1)
  g_rng = g_rng * 1664525u + 1013904223u;
  return (float)((g_rng >> 8) + 0.5) / 8388608.f - 1.f;
}
static std::vector<float> randomVec(size_t n, float scale = 1.f) {
  std::vector<float> v(n);
  for (auto& x : v) x = scale * uniform();
  return v;
}
static void append(std::vector<float>& to, const std::vector<float>& v) { to.insert(to.end(), v.begin(), v.end()); }

int main(int argc, char** argv) {
  if (argc != 7) { std::cerr << "usage: adam_caller <out.bin> <lr> <beta1> <beta2> <eps> <weightDecay>\n"; return 2; }
  const double lr = atof(argv[2]), beta1 = atof(argv[3]), beta2 = atof(argv[4]), eps = atof(argv[5]), wd = atof(argv[6]);
  try {
    const int nfeat = 8, nlabel = 12, B = 3, T = 64, L = 6, steps = 3;
    auto network = buildSequentialModuleFromText(
        "V -1 NFEAT 1 0\nC2 1 4 5 1 2 1 -1 -1\nR\nDO 0.0\nLN 0 1 2\nTDS 4 5 8 0.0 64\nV 0 32 1 0\nRO 1 0 3 2\nL 32 NLABEL\n", nfeat, nlabel);
    auto criterion = std::make_shared<CTCLoss>(getCriterionScaleMode("target", true));
    network->train();
    const std::vector<Variable> params = network->params();
    const int np = (int)params.size();
    AdamOptimizer flat(params, lr, beta1, beta2, eps, wd);
    EXPECT(std::string(flat.kind()) == "adam" && flat.steps() == 0 && flat.state().size() == 2);
    EXPECT(flat.prettyString().find("Adam (beta1=") == 0 && flat.prettyString().find("epsilon") != std::string::npos);
    // one flat buffer per moment, laid out as the parameter arena is
    for (int slot = 0; slot < 2; ++slot)
      for (int i = 0; i < np; ++i)
        EXPECT((*flat.state()[slot])[i].device<float>() - (*flat.state()[slot])[0].device<float>() ==
               params[i].array().device<float>() - params[0].array().device<float>());
    std::vector<Variable> twin;
    std::vector<float> out;
    std::vector<int> head = {np, steps};
    for (auto& p : params) {
      const std::vector<float> h = hostOf(p);
      head.push_back((int)h.size());
      append(out, h);
      twin.push_back(Variable(af::array(p.dims(), h.data()), true));
    }
    AdamOptimizer each(twin, lr, beta1, beta2, eps, wd);

    const std::vector<float> x = randomVec((size_t)B * nfeat * T);
    std::vector<int> tgt((size_t)B * L);
    for (auto& t : tgt) t = (int)((uniform() + 1.f) * 0.5f * (nlabel - 1));
    Variable input = fl::input(af::array(af::dim4(T, nfeat, 1, B), x.data()));
    Variable target(af::array(af::dim4(L, B), tgt.data()), false);
    for (int it = 0; it < steps; ++it) {
      auto output = network->forward({input, fl::noGrad(af::constant(T, af::dim4(1, B)))}).front();
      auto loss = criterion->forward({output, target}).front();
      flat.zeroGrad();
      loss.backward();
      for (int i = 0; i < np; ++i) {
        EXPECT(params[i].isGradAvailable());
        const std::vector<float> g = hostOf(params[i].grad());
        append(out, g);
        twin[i].zeroGrad();
        twin[i].addGrad(Variable(af::array(params[i].dims(), g.data()), false));
      }
      flat.step();
      each.step();
      EXPECT(flat.steps() == (uint64_t)it + 1 && each.steps() == flat.steps());
      for (int i = 0; i < np; ++i) {
        const std::vector<float> h = hostOf(params[i]);
        EXPECT(h == hostOf(twin[i]));
        append(out, h);
      }
      for (int slot = 0; slot < 2; ++slot)
        for (int i = 0; i < np; ++i) {
          const std::vector<float> h = hostOf((*flat.state()[slot])[i]);
          EXPECT(h == hostOf((*each.state()[slot])[i]));
          append(out, h);
        }
    }
    FILE* o = fopen(argv[1], "wb");
    if (!o) { perror(argv[1]); return 2; }
    fwrite(head.data(), 4, head.size(), o);
    fwrite(out.data(), 4, out.size(), o);
    fclose(o);

    // the CPC criterion's parameters: odd sizes, arrays of their own
    const int Bc = 2, Tc = 37, Ce = 21, Cc = 13, D = 7;
    CPCCriterion cpc(Ce, Cc, D, 1, 2, 3, 5, 4, 0.1f);
    const std::vector<float> enc = randomVec((size_t)Bc * Tc * Ce), ctx = randomVec((size_t)Bc * Tc * Cc);
    AdamOptimizer critOpt(cpc.params(), 0.01, beta1, beta2, eps, 0.0);
    for (int it = 0; it < steps; ++it) {
      Variable encV(af::array(af::dim4(Ce, Tc, Bc), enc.data()), true), ctxV(af::array(af::dim4(Cc, Tc, Bc), ctx.data()), true);
      cpc.getMask(encV, 0.3, 4, {}, 77u + it);
      critOpt.zeroGrad();
      cpc.forward({encV, ctxV}).front().backward();
      std::vector<std::vector<float>> before;
      std::vector<bool> has;
      for (auto& p : cpc.params()) { before.push_back(hostOf(p)); has.push_back(p.isGradAvailable()); }
      EXPECT(has.size() == 5 && has[1] && has[2] && has[3] && has[4]);   // (the mask embedding's gradient comes from the masking's backward alone)
      critOpt.step();
      for (size_t i = 0; i < before.size(); ++i) {
        const std::vector<float> after = hostOf(cpc.params()[i]);
        EXPECT(after.size() % 2 == 1);
        for (float v : after) EXPECT(v == v);
        EXPECT((after != before[i]) == has[i]);
      }
    }
    EXPECT(critOpt.steps() == (uint64_t)steps);
    // the constructor refuses what the kernel would
    int refused = 0;
    try { AdamOptimizer bad(twin, lr, 1.0, beta2, eps, wd); } catch (const std::invalid_argument&) { ++refused; }
    try { AdamOptimizer bad(twin, lr, beta1, beta2, -1e-8, wd); } catch (const std::invalid_argument&) { ++refused; }
    try { AdamOptimizer bad(twin, lr, beta1, beta2, eps, -0.1); } catch (const std::invalid_argument&) { ++refused; }
    EXPECT(refused == 3);
  } catch (const std::exception& e) {
    std::cerr << "adam_caller: " << e.what() << "\n";
    return 1;
  }
  std::cout << "adam caller ok" << std::endl;
  return 0;
}
