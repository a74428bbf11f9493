// cpc_sampler_test.cpp -- fl_compat/cpc.h printed for its Python twin (wav2letter_amd/cpc.py; compiled with plain g++ and run by
// tests/test_cpc_host.py).  Stand-alone: nothing of the device, no library.
//   cpc_sampler_test sample B T maskProb maskLength nNegative seed [frames...]   M and K, then one line of maskIndex and one of the
//                                                                            byte mask per utterance, then one line of negatives
//                                                                            per (b, m); a refusal prints "refused: <message>"
//   cpc_sampler_test negatives B M nNegative seed                            the negatives alone
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/fl_compat/cpc.h"

using namespace fl::pkg::speech;

static void printNeg(const std::vector<int>& neg, int B, int M, int K) {
  for (int r = 0; r < B * M; ++r) {
    for (int k = 0; k < K; ++k) std::cout << (k ? " " : "") << neg[(size_t)r * K + k];
    std::cout << "\n";
  }
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  try {
    if (cmd == "sample" && argc >= 8) {
      const int B = std::atoi(argv[2]), T = std::atoi(argv[3]);
      const double prob = std::atof(argv[4]);
      const int len = std::atoi(argv[5]), nNeg = std::atoi(argv[6]);
      const uint64_t seed = std::strtoull(argv[7], nullptr, 10);
      std::vector<int> frames;
      for (int i = 8; i < argc; ++i) frames.push_back(std::atoi(argv[i]));
      if (!frames.empty() && (int)frames.size() != B) {
        std::cerr << "one frame count per utterance\n";
        return 2;
      }
      const CpcSample s = cpcSample(B, T, prob, len, nNeg, frames.empty() ? nullptr : frames.data(), seed);
      std::cout << s.M << " " << s.K << "\n";
      for (int b = 0; b < B; ++b) {
        for (int m = 0; m < s.M; ++m) std::cout << (m ? " " : "") << s.maskIndex[(size_t)b * s.M + m];
        std::cout << "\n";
        for (int t = 0; t < T; ++t) std::cout << (int)s.mask[(size_t)b * T + t];
        std::cout << "\n";
      }
      printNeg(s.neg, B, s.M, s.K);
      return 0;
    }
    if (cmd == "negatives" && argc == 6) {
      const int B = std::atoi(argv[2]), M = std::atoi(argv[3]), nNeg = std::atoi(argv[4]);
      CpcRng rng;
      rng.state = std::strtoull(argv[5], nullptr, 10);
      const std::vector<int> neg = cpcNegatives(rng, B, M, nNeg);
      printNeg(neg, B, M, std::min(nNeg, M));
      return 0;
    }
  } catch (const std::invalid_argument& e) {
    std::cout << "refused: " << e.what() << "\n";
    return 0;
  }
  std::cerr << "usage: cpc_sampler_test sample B T maskProb maskLength nNegative seed [frames...] | negatives B M nNegative seed\n";
  return 2;
}
