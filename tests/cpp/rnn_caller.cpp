// Compiled C++ caller of fl::RNN (include/fl_compat/flashlight.h), built with plain g++ against libw2l_hip.so by rnn_caller.mk and
// driven by tests/test_gpu_rnn.py, which repeats the step through the C ABI's Python wrapper and compares bit for bit.
//
//   rnn_caller <out.bin>   the arch lines the layer object writes, for every mode; then an fl::Sequential of layer objects --
//                          Reorder, a bidirectional two-layer fl::RNN(8, 5, 2, RnnMode::GRU, true), Reorder -- against the same lines as
//                          arch text (same parameters, same output), and one CTC step on it.
//       out: float x[B][8][T] | params[n] | output[B][T][10] | loss[B] | parameter gradient[n]     (B = 2, T = 9; int32 target 1 2 / 3 -1)
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

#define EXPECT(c) do { if (!(c)) { std::cerr << "rnn_caller: " #c " failed (line " << __LINE__ << ")\n"; return 1; } } while (0)

static std::vector<float> hostOf(const af::array& a) {
  std::vector<float> h((size_t)a.elements());
  a.host(h.data());
  return h;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::cerr << "usage: rnn_caller <out.bin>\n"; return 2; }
  try {
    EXPECT(RNN(8, 5, 2, RnnMode::GRU, true).archLine() == "GRU 8 5 2 1 0");
    EXPECT(RNN(8, 5, 1, RnnMode::LSTM, false, 0.25f).archLine() == "LSTM 8 5 1 0 0.25");
    EXPECT(RNN(8, 5, 1, RnnMode::RELU).archLine() == "RNN 8 5 1 0 0" && RNN(8, 5, 1, RnnMode::TANH).archLine() == "RNN 8 5 1 0 0 TANH");
    const int nFeat = 8, nLabel = 10, B = 2, T = 9, L = 2;
    auto fromText = buildSequentialModuleFromText("RO 1 3 0 2\nGRU 8 5 2 1 0\nRO 0 2 1 3\n", nFeat, nLabel);
    auto built = std::make_shared<Sequential>();
    built->setInputFeatures(nFeat);   // no leading fl::View to read NFEAT from
    built->add(Reorder(1, 3, 0, 2));
    built->add(RNN(nFeat, 5, 2, RnnMode::GRU, true));
    built->add(Reorder(0, 2, 1, 3));
    std::vector<float> x((size_t)B * nFeat * T);
    for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((i * 37) % 101) / 50.f - 1.f;
    const int tgt[B * L] = {1, 2, 3, -1};
    std::vector<std::vector<float>> first;
    std::vector<float> out = x;
    for (auto& net : {fromText, built}) {
      net->train();
      const auto params = net->params();
      EXPECT(params.size() == 1);
      Variable input = fl::input(af::array(af::dim4(T, nFeat, 1, B), x.data()));
      auto output = net->forward({input, fl::noGrad(af::constant(T, af::dim4(1, B)))}).front();
      std::vector<std::vector<float>> got = {hostOf(params[0].array()), hostOf(output.array())};
      if (first.empty()) { first = got; continue; }
      EXPECT(got == first && got[1].size() == (size_t)B * T * nLabel);
      CTCLoss criterion(getCriterionScaleMode("target", true));
      auto loss = criterion.forward({output, Variable(af::array(af::dim4(L, B), tgt), false)}).front();
      loss.backward();
      EXPECT(params[0].isGradAvailable());
      got.push_back(hostOf(loss.array()));
      got.push_back(hostOf(params[0].grad().array()));
      for (auto& g : got) out.insert(out.end(), g.begin(), g.end());
    }
    FILE* o = fopen(argv[1], "wb");
    if (!o) { perror(argv[1]); return 2; }
    fwrite(out.data(), 4, out.size(), o);
    fclose(o);
  } catch (const std::exception& e) {
    std::cerr << "rnn_caller: " << e.what() << "\n";
    return 1;
  }
  std::cout << "rnn caller ok" << std::endl;
  return 0;
}
