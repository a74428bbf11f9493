// include/fl_compat/lexicon.h through a compiled caller (plain g++ against libw2l_hip.so), driven by
// tests/test_ctc_beam_lex_host.py, which holds every printed line to the Python front end (wav2letter_amd.lexicon) on the same file.
//
//   lexicon_text_test <tokens file> <lexicon file> <silence token or -> [<arpa over the words>]
//       info <numTokens> <numWords> <numNodes> <silToken> <smeared> <dropped>
//       word <id> <spelling>                          per word, in id order
//       node <id> <smear as hexfloat> <hasChildren> <token>:<child> ... | <word id> ...     per node, in id order
//       refused <message>                             a lexicon whose spelling has a token the dictionary lacks
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "fl_compat/lexicon.h"

using namespace fl::pkg::speech;

int main(int argc, char** argv) {
  if (argc != 4 && argc != 5) { std::cerr << "usage: lexicon_text_test <tokens> <lexicon> <sil or -> [<arpa>]\n"; return 2; }
  std::vector<std::string> tokens;
  std::ifstream tf(argv[1]);
  for (std::string line; std::getline(tf, line);)
    if (!line.empty()) tokens.push_back(line);
  const std::string sil = std::string(argv[3]) == "-" ? "" : argv[3];
  try {
    Lexicon lex = Lexicon::fromFile(argv[2], tokens, nullptr, sil, "none");
    std::unique_ptr<NGramLM> lm;
    if (argc == 5) {
      lm.reset(new NGramLM(NGramLM::fromArpa(argv[4], lex.words())));
      lex = Lexicon::fromFile(argv[2], tokens, lm.get(), sil, "max");
    }
    std::printf("info %d %d %d %d %d %zu\n", lex.numTokens(), lex.numWords(), lex.numNodes(), lex.silToken(), (int)lex.smeared(), lex.dropped());
    for (int w = 0; w < lex.numWords(); ++w) std::printf("word %d %s\n", w, lex.words()[(size_t)w].c_str());
    for (int v = 0; v < lex.numNodes(); ++v) {
      const Lexicon::Node nd = lex.node(v);
      std::printf("node %d %a %d", v, (double)nd.smear, (int)nd.hasChildren);
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
