// CPU test of the forced-alignment host logic of include/fl_compat/text.h (compiled with g++ by tests/test_ctc_align_host.py): the
// worked examples of that Python file on the C++ names, so the two stay one specification.
#include <cassert>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/fl_compat/text.h"

using namespace fl::pkg::speech;
using fl::lib::text::Dictionary;
using Spans = std::vector<std::pair<int, int>>;

static std::vector<std::string> names(const std::vector<int>& v, const Dictionary& d) {
  std::vector<std::string> out;
  for (int i : v) out.push_back(d.getEntry(i));
  return out;
}
static bool seg(const WordSegment& s, double begin, double length, const std::string& word) {
  return std::fabs(s.begin - begin) < 1e-9 && std::fabs(s.length - length) < 1e-9 && s.word == word;
}
template <class F>
static bool throwsInvalid(F f) {
  try { f(); } catch (const std::invalid_argument&) { return true; }
  return false;
}

int main() {
  std::vector<std::string> letters = {"|", "'"};
  for (char c = 'a'; c <= 'z'; ++c) letters.push_back(std::string(1, c));

  {  // CTC letters with the word separator
    Dictionary d = createTokenDict(Dictionary(letters), "ctc", 0);
    auto lex = fl::lib::text::loadWordsFromLines({"hi\th i |", "aa\ta a |"});
    std::vector<std::string> words = {"hi", "aa"};
    auto tgt = targetIndices(words, lex, d, "ctc", 0, "|");
    assert((names(tgt, d) == std::vector<std::string>{"h", "i", "|", "a", "a", "|"}));
    auto widx = targetWordIndex(words, lex, d, "ctc", 0, "|");
    assert((widx == std::vector<int>{0, 0, -1, 1, 1, -1}));
    auto i = [&](const char* s) { return d.getIndex(s); };
    const int b = d.getIndex(kBlankToken);
    std::vector<int> path = {b, i("h"), i("h"), i("i"), i("|"), b, i("a"), b, i("a"), b, i("|"), b};
    auto spans = alignmentTokenSpans(path, tgt, b);
    assert((spans == Spans{{1, 2}, {3, 3}, {4, 4}, {6, 6}, {8, 8}, {10, 10}}));
    auto segs = wordSegments(spans, widx, words, 12, 0.08);
    assert(segs.size() == 5 && seg(segs[0], 0.0, 0.08, "$") && seg(segs[1], 0.08, 0.24, "hi") && seg(segs[2], 0.32, 0.16, "$") &&
           seg(segs[3], 0.48, 0.24, "aa") && seg(segs[4], 0.72, 0.24, "$"));
    assert(formatAlignmentLine("utt-1", segs) ==
           "utt-1\tID A 0.00 0.08 $\\nID A 0.08 0.24 hi\\nID A 0.32 0.16 $\\nID A 0.48 0.24 aa\\nID A 0.72 0.24 $\n");
    std::vector<int> wrong(path.begin(), path.begin() + 6);
    wrong.resize(12, b);
    assert(throwsInvalid([&] { alignmentTokenSpans(wrong, tgt, b); }));
    assert(throwsInvalid([&] { alignmentTokenSpans(std::vector<int>(12, -1), tgt, b); }));   // an infeasible row
    tgt.resize(9, -1);                                                                       // batch padding is ignored
    assert(alignmentTokenSpans(path, tgt, b) == spans);
  }
  {  // speech from frame 0: a zero-length `$` first; words that touch: no silence between them
    Dictionary d = createTokenDict(Dictionary(letters), "ctc", 0);
    auto lex = fl::lib::text::loadWordsFromLines({"a\ta |", "b\tb |"});
    std::vector<std::string> words = {"a", "b"};
    auto tgt = targetIndices(words, lex, d, "ctc", 0, "|");
    auto widx = targetWordIndex(words, lex, d, "ctc", 0, "|");
    assert((widx == std::vector<int>{0, -1, 1, -1}));
    auto i = [&](const char* s) { return d.getIndex(s); };
    const int b = d.getIndex(kBlankToken);
    auto segs = wordSegments(alignmentTokenSpans({i("a"), i("|"), i("b"), i("b"), i("|")}, tgt, b), widx, words, 5, 0.5);
    assert(segs.size() == 5 && seg(segs[0], 0.0, 0.0, "$") && seg(segs[1], 0.0, 0.5, "a") && seg(segs[2], 0.5, 0.5, "$") &&
           seg(segs[3], 1.0, 1.0, "b") && seg(segs[4], 2.0, 0.5, "$"));
    auto segs2 = wordSegments(alignmentTokenSpans({i("a"), i("b"), b}, {i("a"), i("b")}, b), {0, 1}, words, 3, 1.0);
    assert(segs2.size() == 4 && seg(segs2[0], 0.0, 0.0, "$") && seg(segs2[1], 0.0, 1.0, "a") && seg(segs2[2], 1.0, 1.0, "b") &&
           seg(segs2[3], 2.0, 1.0, "$"));
  }
  {  // ASG with replabels and the surround token; an ASG path has no blank
    Dictionary d = createTokenDict(Dictionary(letters), "asg", 2);
    auto lex = fl::lib::text::loadWordsFromLines({"hello\th e l l o |", "aaa\ta a a |"});
    std::vector<std::string> words = {"hello", "aaa"};
    auto plain = targetWordIndex(words, lex, d, "asg", 2, "|");
    assert((names(targetIndices(words, lex, d, "asg", 2, "|"), d) == std::vector<std::string>{"h", "e", "l", "<1>", "o", "|", "a", "<2>", "|"}));
    assert((plain == std::vector<int>{0, 0, 0, 0, 0, -1, 1, 1, -1}));
    // with the surround token the last separator and the surround are one run: the second becomes a replabel of no word
    auto widx = targetWordIndex(words, lex, d, "asg", 2, "|", "|");
    assert((widx == std::vector<int>{-1, 0, 0, 0, 0, 0, -1, 1, 1, -1, -1}));
    std::vector<std::string> toks = {"|", "h", "e", "l", "<1>", "o", "|", "a", "<2>", "|", "<1>"};
    std::vector<int> reps = {2, 1, 1, 2, 1, 1, 3, 1, 2, 1, 1}, tgt, path;
    for (size_t k = 0; k < toks.size(); ++k) {
      tgt.push_back(d.getIndex(toks[k]));
      path.insert(path.end(), (size_t)reps[k], tgt.back());
    }
    auto spans = alignmentTokenSpans(path, tgt);
    assert(spans.front() == std::make_pair(0, 1) && spans.back() == std::make_pair(15, 15));
    auto segs = wordSegments(spans, widx, words, 16, 0.1);
    assert(segs.size() == 5 && seg(segs[0], 0.0, 0.2, "$") && seg(segs[1], 0.2, 0.6, "hello") && seg(segs[2], 0.8, 0.3, "$") &&
           seg(segs[3], 1.1, 0.3, "aaa") && seg(segs[4], 1.4, 0.2, "$"));
    std::vector<int> rotated(path.begin() + 1, path.end());
    rotated.push_back(path[0]);
    assert(throwsInvalid([&] { alignmentTokenSpans(rotated, tgt); }));
    // a run longer than replabel + 1 restarts (a a a a -> a <2> a): the word index follows the packing
    auto lex4 = fl::lib::text::loadWordsFromLines({"aaaa\ta a a a |", "a\ta |"});
    assert((names(targetIndices({"aaaa"}, lex4, d, "asg", 2, "|"), d) == std::vector<std::string>{"a", "<2>", "a", "|"}));
    assert((targetWordIndex({"aaaa"}, lex4, d, "asg", 2, "|") == std::vector<int>{0, 0, 0, -1}));
    assert((names(targetIndices({"a", "aaaa", "a"}, lex4, d, "asg", 2, "|"), d) ==
            std::vector<std::string>{"a", "|", "a", "<2>", "a", "|", "a", "|"}));
    assert((targetWordIndex({"a", "aaaa", "a"}, lex4, d, "asg", 2, "|") == std::vector<int>{0, -1, 1, 1, 1, -1, 2, -1}));
  }
  {  // word pieces: every piece belongs to the word it was generated for, the spelled separator of an out-of-lexicon word included
    std::vector<std::string> pieces = {"_the", "_c", "at", "_cat", "s", "_", "t", "h", "e", "c", "a"};
    Dictionary d = createTokenDict(Dictionary(pieces), "ctc", 0);
    auto lex = fl::lib::text::loadWordsFromLines({"the _the", "cats _cat s", "cat _c at"});
    std::vector<std::string> words = {"the", "cats", "eat"};
    auto widx = targetWordIndex(words, lex, d, "ctc", 0, "_", "", true, true, false);
    assert((widx == std::vector<int>{0, 1, 1, 2, 2, 2, 2}));
    auto i = [&](const char* s) { return d.getIndex(s); };
    const int b = d.getIndex(kBlankToken);
    std::vector<int> tgt = {i("_the"), i("_cat"), i("s"), i("_"), i("e"), i("a"), i("t")};
    std::vector<int> path = {b, b, i("_the"), b, i("_cat"), i("_cat"), i("s"), b, i("_"), i("e"), i("a"), i("t"), i("t"), b};
    auto segs = wordSegments(alignmentTokenSpans(path, tgt, b), widx, words, 14, 0.04);
    assert(segs.size() == 7 && seg(segs[0], 0.0, 0.08, "$") && seg(segs[1], 0.08, 0.04, "the") && seg(segs[2], 0.12, 0.04, "$") &&
           seg(segs[3], 0.16, 0.12, "cats") && seg(segs[4], 0.28, 0.04, "$") && seg(segs[5], 0.32, 0.2, "eat") &&
           seg(segs[6], 0.52, 0.04, "$"));
    double t = 0.0;   // ordered, no overlap, covers [0, frames * seconds per frame]
    for (auto& s : segs) { assert(std::fabs(s.begin - t) < 1e-9 && s.length >= 0); t = s.begin + s.length; }
    assert(std::fabs(t - 14 * 0.04) < 1e-9);
  }
  printf("align text ok\n");
  return 0;
}
