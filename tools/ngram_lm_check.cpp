// ngram_lm_check -- load ARPA files through the library's own reader and table builder, outside the library: a host-only program
// for sanitizer builds of wav2letter_amd/csrc/host/ngram_lm.cpp (no GPU, no HIP runtime).
//   c++ -std=c++17 -g -fsanitize=address,undefined tools/ngram_lm_check.cpp wav2letter_amd/csrc/host/ngram_lm.cpp -o ngram_lm_check
//   ngram_lm_check <tokens file, one spelling per line> <arpa> [<arpa> ...]
// Every file is loaded with the two-call pattern; a loaded table is walked with every (state, word) pair of a bounded sweep, so
// the scorer's probes and back-off walks run too.  A refusal prints its message and is no error: the exit status is 0 unless a
// call misbehaves (a size that changes between the two calls, a next state outside the table).
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../include/w2l_hip.h"

namespace w2l {
static std::string g_msg;
void setHostError(const std::string& m) { g_msg = m; }
}  // namespace w2l

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <tokens file> <arpa> [<arpa> ...]\n", argv[0]);
    return 2;
  }
  std::vector<std::string> tokens;
  std::ifstream tf(argv[1]);
  for (std::string line; std::getline(tf, line);)
    if (!line.empty()) tokens.push_back(line);
  std::vector<const char*> spell;
  for (auto& t : tokens) spell.push_back(t.c_str());
  int bad = 0;
  for (int a = 2; a < argc; ++a) {
    size_t need = 0;
    int skipped = -1;
    int st = w2l_ngram_lm_from_arpa(argv[a], (int)spell.size(), spell.data(), nullptr, &need, &skipped);
    if (st != W2L_OK) {
      std::printf("%s: refused (%d): %s\n", argv[a], st, w2l::g_msg.c_str());
      continue;
    }
    std::vector<unsigned char> mem(need + 16);
    unsigned char* blob = mem.data() + ((16 - ((uintptr_t)mem.data() & 15)) & 15);
    size_t room = need;
    st = w2l_ngram_lm_from_arpa(argv[a], (int)spell.size(), spell.data(), blob, &room, &skipped);
    if (st != W2L_OK || room != need) {
      std::printf("%s: the second call disagrees with the first (%d, %zu against %zu)\n", argv[a], st, room, need);
      ++bad;
      continue;
    }
    int order = 0, numTokens = 0, numStates = 0, hasBos = 0, hasEos = 0, start = -1;
    w2l_ngram_lm_info(blob, &order, &numTokens, &numStates, &hasBos, &hasEos);
    w2l_ngram_lm_start(blob, &start);
    double sum = 0;
    long scored = 0;
    for (int s = 0; s < numStates && s < 512; ++s)
      for (int w = 0; w <= numTokens + 1; ++w) {
        float p = 0;
        int next = -1;
        if (w2l_ngram_lm_score(blob, s, w, &p, &next) != W2L_OK || next < 0 || next >= numStates) ++bad;
        sum += p;
        ++scored;
      }
    std::printf("%s: order %d, %d tokens, %d states, start %d, bos %d, eos %d, %d skipped, %zu bytes; %ld scores, sum %.6f\n", argv[a],
                order, numTokens, numStates, start, hasBos, hasEos, skipped, need, scored, sum);
  }
  return bad ? 1 : 0;
}
