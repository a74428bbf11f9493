// Compiled C++ caller of fl::pkg::speech::WideStreamingDecoder (include/fl_compat/flashlight.h), built with plain g++ against
// libw2l_hip.so and driven by tests/test_gpu_beam_stream_wide.py, which writes the inputs (and the ARPA file), runs this binary
// and compares its hypotheses after every step with the C ABI's and the Python front end's.  The file format is
// beam_stream_caller.cpp's.
//
//   beam_stream_wide_caller <in.bin> <out.bin> [<tokens file> <arpa>]        (with the two files: the token-LM variant)
//       in : int32 S maxChunk maxFrames N W K M Lmax logAdd normalize steps | float threshold lmWeight eosScore |
//            per step: int32 n[S] start[S] | float em[S][maxChunk][N]
//       out: after every step: int32 labels[S][M][Lmax] | int32 lengths[S][M] | float scores[S][M] | with an LM float lmScores[S][M]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <vector>

#include "fl_compat/flashlight.h"
#include "fl_compat/lm.h"

using namespace fl;
using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 3 && argc != 5) { std::cerr << "usage: beam_stream_wide_caller <in.bin> <out.bin> [<tokens file> <arpa>]\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int S = hd[0], C = hd[1], maxFrames = hd[2], N = hd[3], W = hd[4], K = hd[5], M = hd[6], Lmax = hd[7], steps = hd[10];
  const float* fl3 = (const float*)(hd + 11);
  const char* p = (const char*)(fl3 + 3);

  std::unique_ptr<NGramLM> lm;
  if (argc == 5) {
    std::vector<std::string> tokens;
    std::ifstream tf(argv[3]);
    for (std::string line; std::getline(tf, line);)
      if (!line.empty()) tokens.push_back(line);
    lm.reset(new NGramLM(NGramLM::fromArpa(argv[4], tokens)));
  }
  BeamSearchOptions opt;
  opt.beamSize = W;
  opt.beamSizeToken = K;
  opt.beamThreshold = fl3[0];
  opt.logAdd = hd[8] != 0;
  opt.normalize = hd[9];
  opt.nbest = M;
  opt.maxLen = Lmax;
  if (lm) {
    opt.lm = lm.get();
    opt.lmWeight = fl3[1];
    opt.eosScore = fl3[2];
  }
  WideStreamingDecoder dec(S, C, maxFrames, N, opt);
  StreamingDecoder& base = dec;   // the methods are StreamingDecoder's
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  std::vector<int> fed(S, 0);
  for (int i = 0; i < steps; ++i) {
    const int* c = (const int*)p;
    std::vector<int> cnt(c, c + S), st(c + S, c + 2 * S);
    const float* x = (const float*)(c + 2 * S);
    p = (const char*)(x + (size_t)S * C * N);
    dec.step(af::array(af::dim4(N, C, S), x), cnt, st);
    for (int s = 0; s < S; ++s) {
      fed[s] = (st[s] ? 0 : fed[s]) + cnt[s];
      if (dec.frames(s) != fed[s]) { std::cerr << "frames(" << s << ")\n"; return 1; }
    }
    auto r = dec.result();
    if (r.labels.dims(0) != Lmax || r.labels.dims(1) != M || r.labels.dims(2) != S || r.lengths.dims(0) != M || r.lengths.dims(1) != S ||
        r.scores.dims(0) != M || r.scores.dims(1) != S || r.lmScores.isempty() != !lm || !r.words.isempty()) {
      std::cerr << "result dims\n";
      return 1;
    }
    std::vector<int> lab((size_t)S * M * Lmax), len((size_t)S * M);
    std::vector<float> sc((size_t)S * M), ls((size_t)S * M);
    r.labels.host(lab.data());
    r.lengths.host(len.data());
    r.scores.host(sc.data());
    fwrite(lab.data(), 4, lab.size(), out);
    fwrite(len.data(), 4, len.size(), out);
    fwrite(sc.data(), 4, sc.size(), out);
    if (lm) {
      r.lmScores.host(ls.data());
      fwrite(ls.data(), 4, ls.size(), out);
    }
  }
  fclose(out);
  if (p != buf.data() + n) { std::cerr << "input not consumed\n"; return 1; }
  // error behaviour: std::runtime_error for a beam above 1024 (and, on the narrow class, still for options.wide and a beam of
  // 65); options.wide is ignored here; std::invalid_argument for a chunk above maxChunk, for frames on a closed slot and for a
  // frame past maxFrames
  int refused = 0;
  BeamSearchOptions wide = opt;
  wide.wide = true;
  wide.nbest = 1;
  try { StreamingDecoder d2(S, C, maxFrames, N, wide); } catch (const std::invalid_argument&) {} catch (const std::runtime_error&) { ++refused; }
  try { WideStreamingDecoder d2w(S, C, maxFrames, N, wide); ++refused; } catch (const std::exception&) {}   // accepted: counts when it does NOT throw
  BeamSearchOptions big = opt;
  big.beamSize = 1025;
  big.nbest = 1;
  try { WideStreamingDecoder d3(S, C, maxFrames, N, big); } catch (const std::invalid_argument&) {} catch (const std::runtime_error&) { ++refused; }
  big.beamSize = 65;
  try { StreamingDecoder d3n(S, C, maxFrames, N, big); } catch (const std::invalid_argument&) {} catch (const std::runtime_error&) { ++refused; }
  try { WideStreamingDecoder d3w(S, C, maxFrames, N, big); ++refused; } catch (const std::exception&) {}    // 65 is a wide beam
  af::array em(af::dim4(N, C, S), std::vector<float>((size_t)S * C * N, 0.f).data());
  try { dec.step(em, std::vector<int>(S, C + 1), std::vector<int>(S, 1)); } catch (const std::invalid_argument&) { ++refused; }
  base.reset(0);
  if (base.frames(0) != 0) { std::cerr << "reset\n"; return 1; }
  try { dec.step(em, std::vector<int>(S, 1), {}); } catch (const std::invalid_argument&) { ++refused; }
  try {
    WideStreamingDecoder d4(1, C, 1, N, opt);
    d4.step(af::array(af::dim4(N, C, 1), std::vector<float>((size_t)C * N, 0.f).data()), {1}, {1});
    d4.step(af::array(af::dim4(N, C, 1), std::vector<float>((size_t)C * N, 0.f).data()), {1}, {});
  } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("maxFrames = 1") != std::string::npos) ++refused;
  }
  if (refused != 8) { std::cerr << "expected eight outcomes, got " << refused << "\n"; return 1; }
  std::cout << "beam stream wide caller ok" << std::endl;
  return 0;
}
