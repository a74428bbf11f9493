// Compiled C++ caller of fl::pkg::speech::StreamingDecoder::commit / committed (include/fl_compat/flashlight.h), built with plain
// g++ against libw2l_hip.so and driven by tests/test_gpu_beam_commit.py, which writes the inputs (and the ARPA file), runs this
// binary and compares the lines it prints with the Python front end's.
//
//   beam_commit_caller <in.bin> <tokens file> <arpa>          (the token-LM variant; a beam above 64 takes WideStreamingDecoder)
//       in : int32 S maxChunk maxFrames N W K Lmax logAdd normalize steps commitEvery | float threshold lmWeight eosScore |
//            per step: int32 n[S] start[S] | float em[S][maxChunk][N]
//       out: after every step (and the commit that follows every commitEvery-th one), one line per slot:
//            "<step> <slot> <live or -> : <committed labels so far> | <labels of the best row's tail>"
#include <cstdio>
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
  if (argc != 4) { std::cerr << "usage: beam_commit_caller <in.bin> <tokens file> <arpa>\n"; return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf((size_t)n);
  if (fread(buf.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
  fclose(f);
  const int* hd = (const int*)buf.data();
  const int S = hd[0], C = hd[1], maxFrames = hd[2], N = hd[3], W = hd[4], K = hd[5], Lmax = hd[6], steps = hd[9], every = hd[10];
  const float* fl3 = (const float*)(hd + 11);
  const char* p = (const char*)(fl3 + 3);

  std::vector<std::string> tokens;
  std::ifstream tf(argv[2]);
  for (std::string line; std::getline(tf, line);)
    if (!line.empty()) tokens.push_back(line);
  NGramLM lm = NGramLM::fromArpa(argv[3], tokens);
  BeamSearchOptions opt;
  opt.beamSize = W;
  opt.beamSizeToken = K;
  opt.beamThreshold = fl3[0];
  opt.logAdd = hd[7] != 0;
  opt.normalize = hd[8];
  opt.nbest = 1;
  opt.maxLen = Lmax;
  opt.lm = &lm;
  opt.lmWeight = fl3[1];
  opt.eosScore = fl3[2];
  std::unique_ptr<StreamingDecoder> dec;
  if (W > 64) dec.reset(new WideStreamingDecoder(S, C, maxFrames, N, opt));
  else dec.reset(new StreamingDecoder(S, C, maxFrames, N, opt));
  std::vector<int> live(S, -1);
  for (int i = 0; i < steps; ++i) {
    const int* c = (const int*)p;
    std::vector<int> cnt(c, c + S), st(c + S, c + 2 * S);
    const float* x = (const float*)(c + 2 * S);
    p = (const char*)(x + (size_t)S * C * N);
    dec->step(af::array(af::dim4(N, C, S), x), cnt, st);
    for (int s = 0; s < S; ++s)
      if (st[s]) live[s] = -1;
    if (i % every == every - 1) {
      const StreamingDecoder::Committed got = dec->commit();
      if ((int)got.labels.size() != S || (int)got.words.size() != S || (int)got.live.size() != S) { std::cerr << "commit sizes\n"; return 1; }
      for (int s = 0; s < S; ++s) {
        if (!got.words[s].empty()) { std::cerr << "words without a lexicon\n"; return 1; }
        live[s] = got.live[s];
      }
    }
    auto r = dec->result();
    std::vector<int> lab((size_t)S * Lmax), len((size_t)S);
    r.labels.host(lab.data());
    r.lengths.host(len.data());
    for (int s = 0; s < S; ++s) {
      std::cout << i << " " << s << " ";
      if (live[s] < 0) std::cout << "-";
      else std::cout << live[s];
      std::cout << " :";
      const auto done = dec->committed(s);
      if (done.first != dec->committedLabels(s) || !done.second.empty()) { std::cerr << "committed\n"; return 1; }
      for (int l : done.first) std::cout << " " << l;
      std::cout << " |";
      for (int j = 0; j < len[s] && j < Lmax; ++j) std::cout << " " << lab[(size_t)s * Lmax + j];
      std::cout << "\n";
    }
  }
  if (p != buf.data() + n) { std::cerr << "input not consumed\n"; return 1; }
  // error behaviour: a flag vector of the wrong size, a slot that does not exist; a reset forgets what the slot committed
  int refused = 0;
  try { dec->commit(std::vector<int>(S + 1, 1)); } catch (const std::invalid_argument&) { ++refused; }
  try { dec->committedLabels(S); } catch (const std::invalid_argument&) { ++refused; }
  dec->reset(0);
  if (!dec->committedLabels(0).empty() || dec->frames(0) != 0) { std::cerr << "reset\n"; return 1; }
  const StreamingDecoder::Committed none = dec->commit(std::vector<int>(S, 1));
  if (!none.labels[0].empty() || none.live[0] != 0) { std::cerr << "a closed slot committed\n"; return 1; }
  if (refused != 2) { std::cerr << "expected two refusals, got " << refused << "\n"; return 1; }
  std::cout << "beam commit caller ok" << std::endl;
  return 0;
}
