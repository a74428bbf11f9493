// CPU test of the decoded-label host logic of include/fl_compat/text.h (compiled with g++ by tests/test_ctc_beam_host.py): the
// worked examples of that Python file on the C++ names, so the two stay one specification.
#include <cassert>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/fl_compat/text.h"

using namespace fl::pkg::speech;
using fl::lib::text::Dictionary;
using Strs = std::vector<std::string>;

int main() {
  Strs letters = {"|", "'"};
  for (char c = 'a'; c <= 'z'; ++c) letters.push_back(std::string(1, c));
  {  // a doubled letter survives: the labels are already collapsed
    Dictionary d = createTokenDict(Dictionary(letters), "ctc", 0);
    auto i = [&](const char* s) { return d.getIndex(s); };
    std::vector<int> row = {i("h"), i("e"), i("l"), i("l"), i("o"), i("|"), i("b"), i("e"), i("e"), i("|"), -1, -1};
    assert((tknLabels2Ltr(row, d, "ctc", "", 0, false, "|") == Strs{"h", "e", "l", "l", "o", "|", "b", "e", "e"}));
    assert((tknLabels2Wrd(row, d, "ctc", "", 0, false, "|") == Strs{"hello", "bee"}));
    // the per-frame helper would collapse it
    assert((tkn2Wrd(tknPrediction2Ltr(row, d, "ctc", "", 0, false, "|"), "|") == Strs{"helo", "be"}));
    // leading separator, surround token, empty row, padding only
    std::vector<int> lead = {i("|"), i("a"), i("|"), i("|"), i("a"), i("a")};
    assert((tknLabels2Wrd(lead, d, "ctc", "", 0, false, "|") == Strs{"a", "aa"}));
    assert((tknLabels2Ltr(lead, d, "ctc", "|", 0, false, "|") == Strs{"a", "|", "|", "a", "a"}));
    assert(tknLabels2Ltr({}, d, "ctc", "", 0, false, "|").empty() && tknLabels2Wrd({-1, -1}, d, "ctc", "", 0, false, "|").empty());
  }
  {  // word pieces: pieces split into letters, the separator starts a word
    Dictionary d = createTokenDict(Dictionary(Strs{"_the", "_c", "at", "_cat", "s", "_", "t", "h", "e", "c", "a"}), "ctc", 0);
    auto i = [&](const char* s) { return d.getIndex(s); };
    std::vector<int> row = {i("_the"), i("_cat"), i("s"), i("_"), i("e"), i("a"), i("t"), i("t"), -1};
    assert((tknLabels2Ltr(row, d, "ctc", "", 0, true, "_") ==
            Strs{"t", "h", "e", "_", "c", "a", "t", "s", "_", "e", "a", "t", "t"}));
    assert((tknLabels2Wrd(row, d, "ctc", "", 0, true, "_") == Strs{"the", "cats", "eatt"}));
  }
  printf("decode text ok\n");
  return 0;
}
