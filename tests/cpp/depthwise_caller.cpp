// Compiled C++ caller of fl::Conv2D with groups and of fl::Swish (include/fl_compat/flashlight.h), built with plain g++ against
// libw2l_hip.so by depthwise_caller.mk and driven by tests/test_gpu_depthwise_net.py and tests/test_depthwise_host.py.
//
//   depthwise_caller refusals   (no GPU) the arch lines the two layer objects write, and std::invalid_argument for groups that are
//                               neither 1 nor nIn == nOut and for a second axis
//   depthwise_caller            the same, then a network of layer objects -- a depthwise fl::Conv2D(8, 8, 3, 1, 1, 1, -1, 0, 1, 1, true, 8)
//                               and fl::Swish between two convolutions -- against the network built from the same lines as arch
//                               text: the same parameters and, on one input, the same output, bit for bit
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

#define EXPECT(c) do { if (!(c)) { std::cerr << "depthwise_caller: " #c " failed (line " << __LINE__ << ")\n"; return 1; } } while (0)

static std::vector<float> hostOf(const af::array& a) {
  std::vector<float> h((size_t)a.elements());
  a.host(h.data());
  return h;
}

static bool refused(int nIn, int nOut, int wy, int groups) {
  try { Conv2D c(nIn, nOut, 3, wy, 1, 1, -1, 0, 1, 1, true, groups); } catch (const std::invalid_argument&) { return true; }
  return false;
}

int main(int argc, char** argv) {
  try {
    EXPECT(Conv2D(8, 8, 3, 1, 1, 1, -1, 0, 1, 1, true, 8).archLine() == "C 8 8 3 1 -1 1 1 8");
    EXPECT(Conv2D(8, 8, 3, 1, 1, 1, -1, 0).archLine() == "C2 8 8 3 1 1 1 -1 0");
    EXPECT(Swish().archLine() == "SH" && Swish(0.5).archLine() == "SH 0.5");
    EXPECT(refused(8, 8, 1, 4) && refused(8, 8, 1, 2) && refused(8, 16, 1, 8) && refused(16, 8, 1, 8) && refused(8, 8, 3, 8));
    EXPECT(!refused(8, 8, 1, 8) && !refused(8, 8, 1, 1));
    if (argc > 1 && !std::strcmp(argv[1], "refusals")) {
      std::cout << "depthwise refusals ok" << std::endl;
      return 0;
    }
    const int nFeat = 8, nLabel = 11, B = 2, T = 12;
    auto fromText = buildSequentialModuleFromText("V -1 1 NFEAT 0\nC NFEAT 8 3 1 -1 1\nC 8 8 3 1 -1 1 1 8\nSH\nC 8 NLABEL 1 1 -1 1\nRO 2 0 3 1\n", nFeat, nLabel);
    auto built = std::make_shared<Sequential>();
    built->add(View(af::dim4(-1, 1, nFeat, 0)));
    built->add(Conv2D(nFeat, 8, 3, 1, 1, 1, -1, 0));
    built->add(Conv2D(8, 8, 3, 1, 1, 1, -1, 0, 1, 1, true, 8));
    built->add(Swish());
    built->add(Conv2D(8, nLabel, 1, 1, 1, 1, -1, 0));
    built->add(Reorder(2, 0, 3, 1));
    std::vector<float> x((size_t)B * nFeat * T);
    for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((i * 37) % 101) / 50.f - 1.f;
    std::vector<std::vector<float>> out;
    for (auto& net : {fromText, built}) {
      const auto params = net->params();
      EXPECT(params.size() == 6 && params[2].array().elements() == 3 * 8);   // the depthwise weight is (kw, 1, 1, C)
      out.push_back(hostOf(params[2].array()));
      Variable input = fl::input(af::array(af::dim4(T, nFeat, 1, B), x.data()));
      out.push_back(hostOf(net->forward({input, fl::noGrad(af::constant(T, af::dim4(1, B)))}).front().array()));
    }
    EXPECT(out[0] == out[2] && out[1] == out[3] && out[1].size() == (size_t)B * T * nLabel);
    bool moved = false;
    for (float v : out[1]) moved = moved || v != 0.f;
    EXPECT(moved);
  } catch (const std::exception& e) {
    std::cerr << "depthwise_caller: " << e.what() << "\n";
    return 1;
  }
  std::cout << "depthwise caller ok" << std::endl;
  return 0;
}
