// Compiled C++ caller of fl::Residual (include/fl_compat/flashlight.h), built with plain g++ against libw2l_hip.so by
// residual_caller.mk and driven by tests/test_gpu_residual_caller.py.
//
//   residual_caller
//       1. the ResNet-CTC recipe in miniature put together from layer objects -- fl::Residual with add / addShortcut / addScale inside
//          an fl::Sequential -- against the same network built from arch text: same parameter list and initial parameters, and the
//          same emissions, loss and gradients, bit for bit, under CTC in training mode
//       2. the same for a block whose shortcut is a projection (addShortcut(from, to, projection))
//       3. what the pipeline does not build throws std::invalid_argument when the Sequential plans: a shortcut that does not start at
//          the block's input or does not end at its output, a second shortcut, a block without one, and a block whose output differs
//          from its shortcut's in shape
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <string>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

#define EXPECT(c) do { if (!(c)) { std::cerr << "residual_caller: " #c " failed (line " << __LINE__ << ")\n"; return 1; } } while (0)

static std::vector<float> hostOf(const af::array& a) {
  std::vector<float> h((size_t)a.elements());
  a.host(h.data());
  return h;
}
static std::vector<float> hostOf(const Variable& v) { return hostOf(v.array()); }

static uint32_t g_rng = 2468u;
static float uniform() {   // (-1, 1)
  g_rng = g_rng * 1664525u + 1013904223u;
  return (float)((g_rng >> 8) + 0.5) / 8388608.f - 1.f;
}

static const int kFeat = 8, kLabel = 11, kB = 3, kT = 37, kL = 4;

struct Pass {
  std::vector<float> emission, loss;
  std::vector<std::vector<float>> grads;
};

// one training forward / backward under CTC; `from`: a network that must have the same parameters
static int runPass(const std::shared_ptr<Sequential>& net, const std::shared_ptr<Sequential>& from, Pass& out) {
  net->train();
  const std::vector<Variable> params = net->params();
  if (from) {
    const std::vector<Variable> src = from->params();
    EXPECT(src.size() == params.size());
    // the same parameter list, and -- both networks draw their initial values the same way -- the same parameters
    for (size_t i = 0; i < params.size(); ++i) {
      EXPECT(src[i].dims() == params[i].dims());
      EXPECT(hostOf(src[i]) == hostOf(params[i]));
    }
  }
  g_rng = 97531u;
  std::vector<float> x((size_t)kB * kFeat * kT);
  for (auto& v : x) v = uniform();
  std::vector<int> tgt((size_t)kB * kL);
  for (auto& t : tgt) t = (int)((uniform() + 1.f) * 0.5f * (kLabel - 1));
  Variable input = fl::input(af::array(af::dim4(kT, kFeat, 1, kB), x.data()));
  Variable target(af::array(af::dim4(kL, kB), tgt.data()), false);
  auto criterion = std::make_shared<CTCLoss>(getCriterionScaleMode("target", true));
  auto output = net->forward({input, fl::noGrad(af::constant(kT, af::dim4(1, kB)))}).front();
  auto loss = criterion->forward({output, target}).front();
  for (auto& p : net->params()) p.zeroGrad();
  loss.backward();
  out.emission = hostOf(output);
  out.loss = hostOf(loss);
  out.grads.clear();
  for (auto& p : net->params()) {
    EXPECT(p.isGradAvailable());
    out.grads.push_back(hostOf(p.grad()));
  }
  for (float v : out.loss) EXPECT(v == v && v > 0.f);
  return 0;
}

static int samePass(const Pass& a, const Pass& b) {
  EXPECT(a.emission == b.emission);
  EXPECT(a.loss == b.loss);
  EXPECT(a.grads.size() == b.grads.size());
  for (size_t i = 0; i < a.grads.size(); ++i) EXPECT(a.grads[i] == b.grads[i]);
  bool moved = false;
  for (auto& g : a.grads) for (float v : g) moved = moved || v != 0.f;
  EXPECT(moved);
  return 0;
}

static void addPost(Sequential& s) {
  s.add(ReLU());
  s.add(Dropout(0.0));
  s.add(LayerNorm(std::vector<int>{0, 1, 2}));
}

// what must throw std::invalid_argument when the Sequential plans
static bool refusedAtPlan(const std::function<void(Residual&)>& fill, int outChannels = 16) {
  Sequential s;
  s.add(View(af::dim4(-1, 1, kFeat, 0)));
  s.add(Conv2D(kFeat, 16, 3, 1, 1, 1, -1, 0));
  Residual r;
  r.add(Conv2D(16, outChannels, 3, 1, 1, 1, -1, 0));
  r.add(ReLU());
  fill(r);
  s.add(r);
  s.add(Conv2D(outChannels, kLabel, 1, 1, 1, 1, -1, 0));
  s.add(Reorder(2, 0, 3, 1));
  try {
    (void)s.params();
  } catch (const std::invalid_argument& e) {
    return std::string(e.what()).find("RES") != std::string::npos;
  }
  return false;
}

int main() {
  try {
    // 1. the recipe in miniature
    const std::string conv = "C 16 16 3 1 -1 1\n", post = "R\nDO 0\nLN 0 1 2\n";
    const std::string text = "V -1 1 NFEAT 0\nC NFEAT 16 3 2 -1 1\n" + post + "RES 9 1 1\n" + conv + post + conv + post + conv + "SKIP 0 10 0.70711\n" + post +
                             "M 2 1 2 1\nC 16 NLABEL 1 1 -1 1\nRO 2 0 3 1\n";
    auto fromText = buildSequentialModuleFromText(text, kFeat, kLabel);
    auto built = std::make_shared<Sequential>();
    built->add(View(af::dim4(-1, 1, kFeat, 0)));
    built->add(Conv2D(kFeat, 16, 3, 1, 2, 1, -1, 0));
    addPost(*built);
    {
      auto res = std::make_shared<Residual>();
      for (int i = 0; i < 3; ++i) {
        res->add(Conv2D(16, 16, 3, 1, 1, 1, -1, 0));
        if (i < 2) { res->add(ReLU()); res->add(Dropout(0.0)); res->add(LayerNorm(std::vector<int>{0, 1, 2})); }
      }
      res->addShortcut(0, 10);
      res->addScale(10, 0.70711f);
      EXPECT(res->prettyString().find("Residual [RES 9 1 1 | C2 16 16 3 1 1 1 -1 0 | R | ") == 0);
      EXPECT(res->prettyString().find(" | SKIP 0 10 0.7071") != std::string::npos);
      built->add(res);
    }
    addPost(*built);
    built->add(Pool2D(2, 1, 2, 1));
    built->add(Conv2D(16, kLabel, 1, 1, 1, 1, -1, 0));
    built->add(Reorder(2, 0, 3, 1));
    EXPECT(built->prettyString().find("Residual") != std::string::npos);
    Pass a, b;
    if (runPass(fromText, nullptr, a)) return 1;
    if (runPass(built, fromText, b)) return 1;
    EXPECT(a.grads.size() >= 2 + 2 * 3 + 2 + 4);   // front conv, three block convs, output conv; four LayerNorms
    if (samePass(a, b)) return 1;

    // 2. a projection on the shortcut
    const std::string textL = "V -1 1 NFEAT 0\nC NFEAT 16 3 1 -1 1\nRES 4 1 1\nC 16 24 3 1 -1 1\nR\nDO 0\nC 24 24 3 1 -1 1\nSKIPL 0 5 1 0.7071\nC 16 24 1 1 -1 1\nR\n"
                              "C 24 NLABEL 1 1 -1 1\nRO 2 0 3 1\n";
    auto fromTextL = buildSequentialModuleFromText(textL, kFeat, kLabel);
    auto builtL = std::make_shared<Sequential>();
    builtL->add(View(af::dim4(-1, 1, kFeat, 0)));
    builtL->add(Conv2D(kFeat, 16, 3, 1, 1, 1, -1, 0));
    {
      Residual res;
      res.add(Conv2D(16, 24, 3, 1, 1, 1, -1, 0));
      res.add(ReLU());
      res.add(Dropout(0.0));
      res.add(Conv2D(24, 24, 3, 1, 1, 1, -1, 0));
      res.addShortcut(0, 5, Conv2D(16, 24, 1, 1, 1, 1, -1, 0));
      res.addScale(5, 0.7071f);
      builtL->add(res);
    }
    builtL->add(ReLU());
    builtL->add(Conv2D(24, kLabel, 1, 1, 1, 1, -1, 0));
    builtL->add(Reorder(2, 0, 3, 1));
    if (runPass(fromTextL, nullptr, a)) return 1;
    if (runPass(builtL, fromTextL, b)) return 1;
    EXPECT(a.grads.size() == 10);
    if (samePass(a, b)) return 1;

    // 3. refused when the Sequential plans
    EXPECT(refusedAtPlan([](Residual& r) { r.addShortcut(1, 3); }));
    EXPECT(refusedAtPlan([](Residual& r) { r.addShortcut(0, 2); }));
    EXPECT(refusedAtPlan([](Residual& r) { r.addShortcut(0, 3); r.addShortcut(0, 3); }));
    EXPECT(refusedAtPlan([](Residual&) {}));
    EXPECT(refusedAtPlan([](Residual& r) { r.addShortcut(0, 3); }, 24));                                       // 24 channels against the input's 16
    EXPECT(!refusedAtPlan([](Residual& r) { r.addShortcut(0, 3, Conv2D(16, 24, 1, 1, 1, 1, -1, 0)); }, 24));   // ... and with the projection that fits
    EXPECT(!refusedAtPlan([](Residual& r) { r.addShortcut(0, 3); }));
    int refused = 0;
    try { Residual r; r.addScale(1, 0.5f); } catch (const std::invalid_argument&) { ++refused; }               // no shortcut lands there
    try { Residual r; r.add(Residual()); } catch (const std::invalid_argument&) { ++refused; }
    EXPECT(refused == 2);
  } catch (const std::exception& e) {
    std::cerr << "residual_caller: " << e.what() << "\n";
    return 1;
  }
  std::cout << "residual caller ok" << std::endl;
  return 0;
}
