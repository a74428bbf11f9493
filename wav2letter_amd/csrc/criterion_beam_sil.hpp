// criterion_beam_sil.hpp -- the five beam searches with a silence score (w2l_*_beam_search*_sil; contract: include/w2l_hip.h).
// Included at the end of criterion_ctc.hip after the three families' headers.  There is no kernel here: the score is two fields of
// CtcBeamWs (sil, silScore), read at two places -- where ctc_beam_rows writes tokLp, after selection and ranking, and where a stay
// reads lp[e] from the row (beam_stay_front, the wide and xl scans' stays) -- through beam_sil_lp, so the extension, the stay and the
// stay's recomputed merge term see one value.  The compare is on a per-thread class against a kernel argument (the xl scan: against
// two words of its LDS scratch, criterion_beam_xl.hpp) and the add is predicated: no barrier is added and none becomes divergent.  This file is the host side: the checks the silence arguments add,
// the route to the sibling when there is no score (the sibling's kernels and bytes, no + 0), the dispatch over the families, which
// calls each sibling's body (*_do) with a BeamSil, and the one search that changes its scan:
//   the narrow LM-free CTC search.  ctc_beam_scan never materialises extensions: it relies on lp_k + tot being non-increasing in k,
//   which a biased tokLp breaks.  With a silence score the search runs ctc_beam_lm_scan<., ., BeamCtc> with lm == NULL, as the ASG
//   LM-free search and the LM-free session do, and ctc_beam_lm_finish without lmScores; its workspace is the LM variant's.
#pragma once

namespace w2l {

// what the silence arguments add to a sibling's refusals; tokens: N - 1 with a blank, N without
static int beam_sil_check(int family, int tokens, int silToken, float silScore) {
  if (family < 0 || family > 2) return W2L_EINVAL;
  if (!(fabsf(silScore) < INFINITY)) return W2L_EINVAL;
  if (silToken < -1 || silToken >= tokens) return W2L_EINVAL;
  return W2L_OK;
}

static bool beam_sil_none(int silToken, float silScore) { return silToken < 0 || silScore == 0.f; }

static size_t beam_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken, int variant, bool noBlank) {
  if (family == 0) return ctc_beam_workspace_size(B, T, N, beam, beamToken, variant, noBlank);
  if (family == 1) return beam_wide_workspace_size(B, T, N, beam, beamToken, variant, noBlank);
  if (family == 2) return beam_xl_workspace_size(B, T, N, beam, beamToken, variant, noBlank);
  return 0;
}

// w2l_ctc_beam_search's checks, then the token scan without an LM
static int ctc_beam_search_sil_narrow(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
                                      float threshold, int logAdd, int normalize, int nbest, int maxLen, int* labels, int* lengths,
                                      float* scores, void* workspace, w2l_stream_t stream, BeamSil sil) {
  int K = 0;
  if (const int rc = ctc_beam_check(B, T, N, input, beam, beamToken, threshold, nbest, maxLen, labels, lengths, scores, workspace, &K))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  CtcBeamWs ws{};
  if (const int rc = ctc_beam_begin(&ws, kBeamLm, B, T, N, input, frames, beam, K, normalize, workspace, s, false, sil)) return rc;
  ctc_beam_fused_scan(beam, K, logAdd, [&](auto la, auto th) {
    hipLaunchKernelGGL((ctc_beam_lm_scan<decltype(la)::value, decltype(th)::value>), dim3((unsigned)B), dim3(decltype(th)::value), 0, s,
                       T, N, beam, threshold, input, frames, ws, nullptr, 0.f, nullptr, BeamTrans{});
  });
  W2L_LAUNCH_CHECK();
  // without an end term the re-ranking is the identity: the entries come in score order, ties by rank
  hipLaunchKernelGGL(ctc_beam_lm_finish, dim3((unsigned)B), dim3(64), 0, s, nbest, maxLen, N, ws, nullptr, 0.f, 0.f, 0, labels,
                     lengths, scores, nullptr);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

}  // namespace w2l

W2L_API size_t w2l_ctc_beam_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_sil_workspace_size(family, B, T, N, beam, beamToken, w2l::kBeamLm, false);
}
W2L_API size_t w2l_ctc_beam_lm_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_sil_workspace_size(family, B, T, N, beam, beamToken, w2l::kBeamLm, false);
}
W2L_API size_t w2l_ctc_beam_lex_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_sil_workspace_size(family, B, T, N, beam, beamToken, w2l::kBeamLex, false);
}
W2L_API size_t w2l_asg_beam_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_sil_workspace_size(family, B, T, N, beam, beamToken, w2l::kBeamLm, true);
}
W2L_API size_t w2l_asg_beam_lex_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_sil_workspace_size(family, B, T, N, beam, beamToken, w2l::kBeamLex, true);
}

// ARGS: the sibling's argument list as it is passed on.  No score: the sibling's entry point itself.
#define W2L_SIL_DISPATCH(TOKENS, NAME, ...)                                                       \
  using namespace w2l;                                                                            \
  if (const int rc = beam_sil_check(family, TOKENS, silToken, silScore)) return rc;               \
  if (beam_sil_none(silToken, silScore))                                                          \
    return family == 0 ? w2l_##NAME(__VA_ARGS__)                                                  \
                       : family == 1 ? w2l_##NAME##_wide(__VA_ARGS__) : w2l_##NAME##_xl(__VA_ARGS__); \
  const BeamSil sil{silToken, silScore}

W2L_API int w2l_ctc_beam_search_sil(int family, int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
                                    float threshold, int logAdd, int normalize, int nbest, int maxLen, int* labels, int* lengths,
                                    float* scores, void* workspace, w2l_stream_t stream, int silToken, float silScore) {
  W2L_SIL_DISPATCH(N - 1, ctc_beam_search, B, T, N, input, frames, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen,
                   labels, lengths, scores, workspace, stream);
  if (family == 0)
    return ctc_beam_search_sil_narrow(B, T, N, input, frames, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, labels,
                                      lengths, scores, workspace, stream, sil);
  if (family == 1)
    return ctc_beam_search_wide_do(B, T, N, input, frames, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, labels,
                                   lengths, scores, workspace, stream, sil);
  return ctc_beam_search_xl_do(B, T, N, input, frames, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, labels, lengths,
                               scores, workspace, stream, sil);
}

W2L_API int w2l_ctc_beam_search_lm_sil(int family, int B, int T, int N, const float* input, const int* frames, int beam,
                                       int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen,
                                       const void* lm, int lmHasEos, float lmWeight, const float* classScore, float eosScore,
                                       int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
                                       w2l_stream_t stream, int silToken, float silScore) {
#define W2L_SIL_ARGS \
  B, T, N, input, frames, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, lm, lmHasEos, lmWeight, classScore, eosScore, \
      labels, lengths, scores, lmScores, workspace, stream
  W2L_SIL_DISPATCH(N - 1, ctc_beam_search_lm, W2L_SIL_ARGS);
  if (family == 0) return ctc_beam_search_lm_do(W2L_SIL_ARGS, sil);
  if (family == 1) return ctc_beam_search_lm_wide_do(W2L_SIL_ARGS, sil);
  return ctc_beam_search_lm_xl_do(W2L_SIL_ARGS, sil);
#undef W2L_SIL_ARGS
}

W2L_API int w2l_ctc_beam_search_lex_sil(int family, int B, int T, int N, const float* input, const int* frames, int beam,
                                        int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen,
                                        const void* lm, int lmHasEos, float lmWeight, const void* lexicon, float wordScore,
                                        float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
                                        int* words, int* wordCounts, void* workspace, w2l_stream_t stream, int silToken,
                                        float silScore) {
#define W2L_SIL_ARGS \
  B, T, N, input, frames, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, lm, lmHasEos, lmWeight, lexicon, wordScore, \
      eosScore, labels, lengths, scores, lmScores, maxWords, words, wordCounts, workspace, stream
  W2L_SIL_DISPATCH(N - 1, ctc_beam_search_lex, W2L_SIL_ARGS);
  if (family == 0) return ctc_beam_search_lex_do(W2L_SIL_ARGS, sil);
  if (family == 1) return ctc_beam_search_lex_wide_do(W2L_SIL_ARGS, sil);
  return ctc_beam_search_lex_xl_do(W2L_SIL_ARGS, sil);
#undef W2L_SIL_ARGS
}

W2L_API int w2l_asg_beam_search_sil(int family, int B, int T, int N, const float* input, const int* frames, const float* trans,
                                    int beam, int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen,
                                    const void* lm, int lmHasEos, float lmWeight, const float* classScore, float eosScore,
                                    int* labels, int* lengths, float* scores, float* lmScores, void* workspace, w2l_stream_t stream,
                                    int silToken, float silScore) {
#define W2L_SIL_ARGS \
  B, T, N, input, frames, trans, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, lm, lmHasEos, lmWeight, classScore, \
      eosScore, labels, lengths, scores, lmScores, workspace, stream
  W2L_SIL_DISPATCH(N, asg_beam_search, W2L_SIL_ARGS);
  if (family == 0) return asg_beam_search_do(W2L_SIL_ARGS, sil);
  if (family == 1) return asg_beam_search_wide_do(W2L_SIL_ARGS, sil);
  return asg_beam_search_xl_do(W2L_SIL_ARGS, sil);
#undef W2L_SIL_ARGS
}

W2L_API int w2l_asg_beam_search_lex_sil(int family, int B, int T, int N, const float* input, const int* frames, const float* trans,
                                        int beam, int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen,
                                        const void* lm, int lmHasEos, float lmWeight, const void* lexicon, float wordScore,
                                        float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
                                        int* words, int* wordCounts, void* workspace, w2l_stream_t stream, int silToken,
                                        float silScore) {
#define W2L_SIL_ARGS \
  B, T, N, input, frames, trans, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, lm, lmHasEos, lmWeight, lexicon, \
      wordScore, eosScore, labels, lengths, scores, lmScores, maxWords, words, wordCounts, workspace, stream
  W2L_SIL_DISPATCH(N, asg_beam_search_lex, W2L_SIL_ARGS);
  if (family == 0) return asg_beam_search_lex_do(W2L_SIL_ARGS, sil);
  if (family == 1) return asg_beam_search_lex_wide_do(W2L_SIL_ARGS, sil);
  return asg_beam_search_lex_xl_do(W2L_SIL_ARGS, sil);
#undef W2L_SIL_ARGS
}
#undef W2L_SIL_DISPATCH
