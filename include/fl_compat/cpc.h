// fl_compat/cpc.h -- which frames the CPC criterion masks and which negatives every masked frame is scored against (header only,
// nothing of the device; Python twin: wav2letter_amd/cpc.py; tests: tests/cpp/cpc_sampler_test.cpp compiled with g++ by
// tests/test_cpc_host.py).  Restated from recipes/joint_training_vox_populi/cpc/CPCCriterion.cpp:
//
//   span mask       :98-113   per utterance floor(maskProb T) start frames, uniform in [0, T) with replacement; a start s marks
//                             s, s+1, s-1, s+2, s-2, ... for maskLength frames in all (delta_i = +-(i + 1) / 2, + for odd i); frames
//                             outside [0, T) are dropped, nothing wraps around
//   equal counts    :118-128  M = the smallest marked count of the batch; every utterance keeps a uniformly random subset of M of
//                             its marked frames -> maskIndex [B][M], strictly ascending per row, and the [B][T] byte mask
//   negatives       :139-158  K = min(nNegative, M); masked position m (an index into the utterance's masked list) draws each of
//                             its K negatives from the positions of the same list that are neither m nor a list neighbour, with
//                             the reference's index arithmetic at nBuff = 1:
//                                 lo = min(M, m + 2), hi = max(M, M - 1 + m), j = (lo + draw % (hi - lo)) % M
//                             m = 0 excludes {0, 1}, m = M - 1 excludes {M - 2, M - 1}, any other m excludes {m - 1, m, m + 1}; hi - lo is
//                             M - 2 or M - 3, so M >= 4 is required (the reference divides by zero below that) -> neg [B][M][K]
//
// Extension: `frames` (may be null) restricts the starts and the spans of utterance b to [0, frames[b]), so padding is never masked;
// the number of starts stays floor(maskProb T).  Null is the reference's behaviour (it masks padding frames too).
//
// Random draws.  ArrayFire's random stream cannot be reproduced, so the draws are this project's: ONE splitmix64 stream (the
// generator of fl_compat/ipl.h) seeded with `seed`, consumed in this order:
//   1. for b ascending: floor(maskProb T) starts, each next % n_b (n_b = frames[b] or T)
//   2. for b ascending: a Fisher-Yates shuffle of the utterance's ascending marked list from the back (for i = size - 1 down to 1:
//      j = next % (i + 1), swap); the first M entries are kept and sorted
//   3. for b, m, k ascending: one draw per negative
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

namespace fl {
namespace pkg {
namespace speech {

struct CpcRng {
  uint64_t state = 0;
  uint64_t next() {
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

struct CpcSample {
  int B = 0, T = 0, M = 0, K = 0;
  std::vector<uint8_t> mask;   // [B][T], 1 = masked
  std::vector<int> maskIndex;  // [B][M], strictly ascending per row
  std::vector<int> neg;        // [B][M][K], positions of the utterance's masked list
};

// the frames start s marks: s, s+1, s-1, s+2, s-2, ... (maskLength of them) clipped to [0, n)
inline void cpcMarkSpan(std::vector<uint8_t>& row, int s, int maskLength, int n) {
  for (int i = 0; i < maskLength; ++i) {
    const int d = (i + 1) / 2;
    const int t = (i & 1) ? s + d : s - d;
    if (t >= 0 && t < n) row[(size_t)t] = 1;
  }
}

// the K negatives of every masked position; M >= 4
inline std::vector<int> cpcNegatives(CpcRng& rng, int B, int M, int nNegative) {
  if (M < 4) throw std::invalid_argument("CPC: negative sampling needs M >= 4 masked frames per utterance, got M = " + std::to_string(M));
  if (nNegative < 1) throw std::invalid_argument("CPC: nNegative must be positive");
  const int K = std::min(nNegative, M);
  std::vector<int> neg((size_t)B * M * K);
  size_t o = 0;
  for (int b = 0; b < B; ++b)
    for (int m = 0; m < M; ++m) {
      const int lo = std::min(M, m + 2), hi = std::max(M, M - 1 + m);
      for (int k = 0; k < K; ++k) neg[o++] = (int)(((uint64_t)lo + rng.next() % (uint64_t)(hi - lo)) % (uint64_t)M);
    }
  return neg;
}

inline CpcSample cpcSample(int B, int T, double maskProb, int maskLength, int nNegative, const int* frames, uint64_t seed) {
  if (B < 1 || T < 1) throw std::invalid_argument("CPC: B and T must be positive");
  if (!(maskProb >= 0.0) || maskLength < 1) throw std::invalid_argument("CPC: maskProb must not be negative and maskLength must be positive");
  CpcRng rng;
  rng.state = seed;
  CpcSample out;
  out.B = B;
  out.T = T;
  const long numMask = (long)std::floor(maskProb * (double)T);
  std::vector<std::vector<uint8_t>> marked((size_t)B, std::vector<uint8_t>((size_t)T, 0));
  for (int b = 0; b < B; ++b) {
    const int n = frames ? frames[b] : T;
    if (n < 1 || n > T) throw std::invalid_argument("CPC: frames[" + std::to_string(b) + "] = " + std::to_string(n) + " is outside 1 .. T");
    for (long i = 0; i < numMask; ++i) cpcMarkSpan(marked[(size_t)b], (int)(rng.next() % (uint64_t)n), maskLength, n);
  }
  std::vector<std::vector<int>> lists((size_t)B);
  int M = T;
  for (int b = 0; b < B; ++b) {
    for (int t = 0; t < T; ++t)
      if (marked[(size_t)b][(size_t)t]) lists[(size_t)b].push_back(t);
    M = std::min(M, (int)lists[(size_t)b].size());
  }
  if (M < 4) throw std::invalid_argument("CPC: negative sampling needs M >= 4 masked frames per utterance, got M = " + std::to_string(M));
  out.M = M;
  out.mask.assign((size_t)B * T, 0);
  out.maskIndex.resize((size_t)B * M);
  for (int b = 0; b < B; ++b) {
    std::vector<int>& v = lists[(size_t)b];
    for (size_t i = v.size(); i-- > 1;) std::swap(v[i], v[(size_t)(rng.next() % (uint64_t)(i + 1))]);
    v.resize((size_t)M);
    std::sort(v.begin(), v.end());
    for (int m = 0; m < M; ++m) {
      out.maskIndex[(size_t)b * M + m] = v[(size_t)m];
      out.mask[(size_t)b * T + v[(size_t)m]] = 1;
    }
  }
  out.neg = cpcNegatives(rng, B, M, nNegative);
  out.K = std::min(nNegative, M);
  return out;
}

}  // namespace speech
}  // namespace pkg
}  // namespace fl
