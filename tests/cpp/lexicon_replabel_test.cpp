// include/fl_compat/lexicon.h's replabel packing (Lexicon::fromFile(..., replabel), on packReplabels of fl_compat/text.h) through a
// compiled caller (plain g++ against libw2l_hip.so), driven by tests/test_asg_beam_host.py, which holds every printed line to the
// Python front end (wav2letter_amd.lexicon, replabel=) on the same file.
//
//   lexicon_replabel_test <tokens file> <lexicon file> <silence token or -> <replabel>
//       info <numTokens> <numWords> <numNodes> <silToken> <smeared> <dropped>
//       word <id> <spelling>                          per word, in id order
//       node <id> <hasChildren> <token>:<child> ... | <word id> ...     per node, in id order
//       refused <message>                             a replabel the token dictionary lacks
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "fl_compat/lexicon.h"

using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 5) { std::cerr << "usage: lexicon_replabel_test <tokens> <lexicon> <sil or -> <replabel>\n"; return 2; }
  std::vector<std::string> tokens;
  std::ifstream tf(argv[1]);
  for (std::string line; std::getline(tf, line);)
    if (!line.empty()) tokens.push_back(line);
  const std::string sil = std::string(argv[3]) == "-" ? "" : argv[3];
  try {
    const Lexicon lex = Lexicon::fromFile(argv[2], tokens, nullptr, sil, "none", std::atoi(argv[4]));
    std::printf("info %d %d %d %d %d %zu\n", lex.numTokens(), lex.numWords(), lex.numNodes(), lex.silToken(), (int)lex.smeared(), lex.dropped());
    for (int w = 0; w < lex.numWords(); ++w) std::printf("word %d %s\n", w, lex.words()[(size_t)w].c_str());
    for (int v = 0; v < lex.numNodes(); ++v) {
      const Lexicon::Node nd = lex.node(v);
      std::printf("node %d %d", v, (int)nd.hasChildren);
      for (int t = 0; t < lex.numTokens(); ++t)
        if (lex.child(v, t) >= 0) std::printf(" %d:%d", t, lex.child(v, t));
      std::printf(" |");
      for (int w : nd.words) std::printf(" %d", w);
      std::printf("\n");
    }
  } catch (const std::invalid_argument& e) {
    std::printf("refused %s\n", e.what());
  }
  return 0;
}
