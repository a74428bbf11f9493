// Compiled C++ caller of fl::pkg::speech::ManyTokenStreamingDecoder (include/fl_compat/flashlight.h), built by
// beam_stream_mt_caller.mk against libw2l_hip.so and driven by tests/test_gpu_beam_stream_mt.py, which writes the inputs (and the
// ARPA file), runs this binary and compares its hypotheses after every step with the C ABI's and the Python front end's.  The file
// format is beam_stream_caller.cpp's with the silence pair added.
//
//   beam_stream_mt_caller <in.bin> <out.bin> [<tokens file> <arpa>]        (with the two files: the token-LM variant)
//       in : int32 S maxChunk maxFrames N W K M Lmax logAdd normalize steps silToken | float threshold lmWeight eosScore silScore |
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
  if (argc != 3 && argc != 5) { std::cerr << "usage: beam_stream_mt_caller <in.bin> <out.bin> [<tokens file> <arpa>]\n"; return 2; }
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
  const float* fl3 = (const float*)(hd + 12);
  const char* p = (const char*)(fl3 + 4);

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
  opt.silToken = hd[11];
  opt.silScore = fl3[3];
  opt.manyTokens = (W & 1) != 0;   // ignored: the class is always many-token
  if (lm) {
    opt.lm = lm.get();
    opt.lmWeight = fl3[1];
    opt.eosScore = fl3[2];
  }
  ManyTokenStreamingDecoder dec(S, C, maxFrames, N, opt);
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
  // error behaviour: std::runtime_error for a beam above 8192 and for more than 256 tokens; std::invalid_argument for lmToken,
  // wide and xl, and for a silence score without a silence token; the two older classes keep throwing on manyTokens and on a
  // non-zero silScore (std::invalid_argument) and on 65 tokens (std::runtime_error); commit at a beam above 1024 is a
  // std::runtime_error; a chunk above maxChunk and frames on a closed slot are std::invalid_argument
  int refused = 0;
  BeamSearchOptions o = opt;
  o.nbest = 1;
  o.silToken = -1; o.silScore = 0.f;
  o.lm = nullptr; o.lmWeight = 0.f; o.eosScore = 0.f;   // LM-free: the class counts below differ from the LM's
  auto invalid = [&](auto&& make) { try { make(); } catch (const std::invalid_argument&) { ++refused; } catch (const std::exception&) {} };
  auto runtime = [&](auto&& make) { try { make(); } catch (const std::invalid_argument&) {} catch (const std::runtime_error&) { ++refused; } };
  { BeamSearchOptions b = o; b.beamSize = 8193; runtime([&] { ManyTokenStreamingDecoder d(S, C, maxFrames, N, b); }); }
  { BeamSearchOptions b = o; b.beamSizeToken = 1000; runtime([&] { ManyTokenStreamingDecoder d(S, C, maxFrames, 300, b); }); }
  { BeamSearchOptions b = o; b.lmToken = true; invalid([&] { ManyTokenStreamingDecoder d(S, C, maxFrames, N, b); }); }
  { BeamSearchOptions b = o; b.wide = true; invalid([&] { ManyTokenStreamingDecoder d(S, C, maxFrames, N, b); }); }
  { BeamSearchOptions b = o; b.xl = true; invalid([&] { ManyTokenStreamingDecoder d(S, C, maxFrames, N, b); }); }
  { BeamSearchOptions b = o; b.silScore = 0.5f; invalid([&] { ManyTokenStreamingDecoder d(S, C, maxFrames, N, b); }); }   // no token
  { BeamSearchOptions b = o; b.beamSize = 64; b.beamSizeToken = 8; b.manyTokens = true; invalid([&] { StreamingDecoder d(S, C, maxFrames, N, b); }); }
  { BeamSearchOptions b = o; b.beamSize = 64; b.beamSizeToken = 8; b.manyTokens = true; invalid([&] { WideStreamingDecoder d(S, C, maxFrames, N, b); }); }
  { BeamSearchOptions b = o; b.beamSize = 64; b.beamSizeToken = 8; b.silToken = 0; b.silScore = 0.5f; invalid([&] { StreamingDecoder d(S, C, maxFrames, N, b); }); }
  { BeamSearchOptions b = o; b.beamSize = 64; b.beamSizeToken = 8; b.silToken = 0; b.silScore = 0.5f; invalid([&] { WideStreamingDecoder d(S, C, maxFrames, N, b); }); }
  { BeamSearchOptions b = o; b.beamSize = 64; b.beamSizeToken = 65; runtime([&] { StreamingDecoder d(S, C, maxFrames, 300, b); }); }
  { BeamSearchOptions b = o; b.beamSize = 64; b.beamSizeToken = 65; runtime([&] { WideStreamingDecoder d(S, C, maxFrames, 300, b); }); }
  {
    BeamSearchOptions b = o;
    b.beamSize = 1025;
    ManyTokenStreamingDecoder d(1, C, 2, N, b);
    d.step(af::array(af::dim4(N, C, 1), std::vector<float>((size_t)C * N, 0.f).data()), {1}, {1});
    runtime([&] { d.commit(); });
    if (d.frames(0) != 1) { std::cerr << "frames after a refused commit\n"; return 1; }
  }
  af::array em(af::dim4(N, C, S), std::vector<float>((size_t)S * C * N, 0.f).data());
  invalid([&] { dec.step(em, std::vector<int>(S, C + 1), std::vector<int>(S, 1)); });
  base.reset(0);
  if (base.frames(0) != 0) { std::cerr << "reset\n"; return 1; }
  invalid([&] { dec.step(em, std::vector<int>(S, 1), {}); });
  if (refused != 15) { std::cerr << "expected fifteen refusals, got " << refused << "\n"; return 1; }
  std::cout << "beam stream mt caller ok" << std::endl;
  return 0;
}
