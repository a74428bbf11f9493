// criterion_beam_mt.hpp -- the five many-token beam searches (w2l_*_beam_search*_mt; contract: include/w2l_hip.h): the
// xl searches with up to kBeamMtMax = 256 frame tokens, the --beamsizetoken the reference's word-piece recipes ask for (100, 150).
// Included at the end of criterion_ctc.hip after criterion_beam_xl.hpp and criterion_beam_sil.hpp.  There is no kernel here: the
// scan is beam_xl_scan<., ., ., kMt = true> (criterion_beam_xl.hpp), which differs from the xl scan in what a token count above 64
// touches -- 256 LDS slots of frame tokens, gone masks of ceil(K / 64) words, 8 bits of k in the tie key -- and the row pass and the
// finish are the xl searches' as they stand (ctc_beam_rows ranks up to 256 per-thread maxima and makes no use of kBeamMax;
// beam_xl_finish does not see K).  This file is the host side: the checks the silence arguments add, in front of the xl twin's own,
// and the call of the twin's body (*_xl_do) with mt set.  No silence score: BeamSil{}, whose token matches no class, so no + 0 is
// executed.  Nothing is routed to another family: K <= 64 runs the many-token scan too, and returns the xl twin's bytes.
#pragma once

namespace w2l {

static BeamSil beam_mt_sil(int silToken, float silScore) {
  return beam_sil_none(silToken, silScore) ? BeamSil{} : BeamSil{silToken, silScore};
}

}  // namespace w2l

W2L_API size_t w2l_ctc_beam_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_xl_workspace_size(B, T, N, beam, beamToken, w2l::kBeamLm, false, true);
}
W2L_API size_t w2l_ctc_beam_lm_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_xl_workspace_size(B, T, N, beam, beamToken, w2l::kBeamLm, false, true);
}
W2L_API size_t w2l_ctc_beam_lex_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_xl_workspace_size(B, T, N, beam, beamToken, w2l::kBeamLex, false, true);
}
W2L_API size_t w2l_asg_beam_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_xl_workspace_size(B, T, N, beam, beamToken, w2l::kBeamLm, true, true);
}
W2L_API size_t w2l_asg_beam_lex_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_xl_workspace_size(B, T, N, beam, beamToken, w2l::kBeamLex, true, true);
}

W2L_API int w2l_ctc_beam_search_mt(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
                                   float threshold, int logAdd, int normalize, int nbest, int maxLen, int* labels, int* lengths,
                                   float* scores, void* workspace, w2l_stream_t stream, int silToken, float silScore) {
  using namespace w2l;
  if (const int rc = beam_sil_check(2, N - 1, silToken, silScore)) return rc;
  return ctc_beam_search_xl_do(B, T, N, input, frames, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, labels, lengths,
                               scores, workspace, stream, beam_mt_sil(silToken, silScore), true);
}

W2L_API int w2l_ctc_beam_search_lm_mt(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
                                      float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm,
                                      int lmHasEos, float lmWeight, const float* classScore, float eosScore, int* labels,
                                      int* lengths, float* scores, float* lmScores, void* workspace, w2l_stream_t stream,
                                      int silToken, float silScore) {
  using namespace w2l;
  if (const int rc = beam_sil_check(2, N - 1, silToken, silScore)) return rc;
  return ctc_beam_search_lm_xl_do(B, T, N, input, frames, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, lm, lmHasEos,
                                  lmWeight, classScore, eosScore, labels, lengths, scores, lmScores, workspace, stream,
                                  beam_mt_sil(silToken, silScore), true);
}

W2L_API int w2l_ctc_beam_search_lex_mt(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
                                       float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm,
                                       int lmHasEos, float lmWeight, const void* lexicon, float wordScore, float eosScore,
                                       int* labels, int* lengths, float* scores, float* lmScores, int maxWords, int* words,
                                       int* wordCounts, void* workspace, w2l_stream_t stream, int silToken, float silScore) {
  using namespace w2l;
  if (const int rc = beam_sil_check(2, N - 1, silToken, silScore)) return rc;
  return ctc_beam_search_lex_xl_do(B, T, N, input, frames, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, lm, lmHasEos,
                                   lmWeight, lexicon, wordScore, eosScore, labels, lengths, scores, lmScores, maxWords, words,
                                   wordCounts, workspace, stream, beam_mt_sil(silToken, silScore), true);
}

W2L_API int w2l_asg_beam_search_mt(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
                                   int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm,
                                   int lmHasEos, float lmWeight, const float* classScore, float eosScore, int* labels, int* lengths,
                                   float* scores, float* lmScores, void* workspace, w2l_stream_t stream, int silToken,
                                   float silScore) {
  using namespace w2l;
  if (const int rc = beam_sil_check(2, N, silToken, silScore)) return rc;
  return asg_beam_search_xl_do(B, T, N, input, frames, trans, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, lm,
                               lmHasEos, lmWeight, classScore, eosScore, labels, lengths, scores, lmScores, workspace, stream,
                               beam_mt_sil(silToken, silScore), true);
}

W2L_API int w2l_asg_beam_search_lex_mt(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
                                       int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen,
                                       const void* lm, int lmHasEos, float lmWeight, const void* lexicon, float wordScore,
                                       float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
                                       int* words, int* wordCounts, void* workspace, w2l_stream_t stream, int silToken,
                                       float silScore) {
  using namespace w2l;
  if (const int rc = beam_sil_check(2, N, silToken, silScore)) return rc;
  return asg_beam_search_lex_xl_do(B, T, N, input, frames, trans, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, lm,
                                   lmHasEos, lmWeight, lexicon, wordScore, eosScore, labels, lengths, scores, lmScores, maxWords,
                                   words, wordCounts, workspace, stream, beam_mt_sil(silToken, silScore), true);
}
