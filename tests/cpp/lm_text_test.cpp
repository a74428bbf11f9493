// Host-side C++ check of fl_compat/lm.h and the text glue around it (no GPU), built with plain g++ against libw2l_hip.so and driven
// by tests/test_ctc_beam_lm_host.py, which compares every line with the Python NGramLM and text.py.
//
//   lm_text_test <tokens file> <arpa> <wordsep> <word id> ...
//       prints  `info order numTokens numStates start hasBos hasEos skipped`, then for the walk from the start state over the word
//       ids one line `q <log p as %a> <next state>`, `sentence <%a>` for the walk as a label row, `words <the row as words>`
//       (tknLabels2Wrd with the token dictionary of the file), and `refused <message>` for a file the library refuses.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "fl_compat/lm.h"
#include "fl_compat/text.h"

using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc < 4) { std::cerr << "usage: lm_text_test <tokens file> <arpa> <wordsep> <word id> ...\n"; return 2; }
  std::vector<std::string> tokens;
  std::ifstream tf(argv[1]);
  for (std::string line; std::getline(tf, line);)
    if (!line.empty()) tokens.push_back(line);
  try {
    NGramLM lm = NGramLM::fromArpa(argv[2], tokens);
    NGramLM copy = lm;   // copies share the table
    std::printf("info %d %d %d %d %d %d %d\n", copy.order(), copy.numTokens(), copy.numStates(), copy.start(), (int)copy.hasBos(),
                (int)copy.hasEos(), copy.skipped());
    int s = copy.start();
    std::vector<int> row;
    for (int i = 4; i < argc; ++i) {
      const int w = std::atoi(argv[i]);
      auto r = copy.score(s, w);
      std::printf("q %a %d\n", (double)r.first, r.second);
      s = r.second;
      if (w < copy.numTokens()) row.push_back(w);
    }
    std::printf("sentence %a\n", (double)copy.sentence(row));
    fl::lib::text::Dictionary dict(tokens);
    std::string words;
    for (auto& w : tknLabels2Wrd(row, dict, "ctc", "", 0, false, argv[3])) words += (words.empty() ? "" : " ") + w;
    std::printf("words %s\n", words.c_str());
    try { copy.score(copy.numStates(), 0); std::printf("no bounds check\n"); } catch (const std::invalid_argument& e) { std::printf("refused %s\n", e.what()); }
  } catch (const std::invalid_argument& e) {
    std::printf("refused %s\n", e.what());
  } catch (const std::runtime_error& e) {
    std::printf("unsupported %s\n", e.what());
  }
  return 0;
}
