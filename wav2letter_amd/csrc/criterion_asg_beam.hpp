// criterion_asg_beam.hpp -- w2l_asg_beam_search and w2l_asg_beam_search_lex: the beam searches of an ASG model (contract:
// include/w2l_hip.h).  Included at the end of criterion_ctc.hip after the three CTC beam headers.  An ASG lattice is the CTC one
// with three changes -- no blank, one transition term per step, no token after itself -- and all three are the policy BeamAsg of
// the two workgroup scans: ctc_beam_lm_scan<., ., BeamAsg> (lexicon-free; a null LM means none) and ctc_beam_lex_scan<., .,
// BeamAsg>.  In the scans' terms an ASG entry's value p is pnb = tot with pb = -inf; the empty prefix is pb = tot = 0 as in CTC.
// The one-wavefront lazy scan of the LM-free CTC search does not apply: A[c][e] depends on (entry, token), so lp_k + p is not
// monotone in k, the reason the LM scan materialises every pair.  Rows: ctc_beam_rows<., true> (every class a token, K up to N).
// Finishes: ctc_beam_lm_finish and ctc_beam_lex_finish as they are (with a null LM the EOS term is off and the LM sums are 0).
//   The transition matrix.  A pair's term A[c][e] is a gather.  When N * N * 4 bytes <= kAsgTransLds (32 KiB: N <= 90, the letter
//   models' 30 x 30 is 3.6 KB) the workgroup copies the matrix into dynamic LDS once, before the first frame; else every pair does
//   one dependent 4-byte load from global memory (N = 9998: 400 MB, L2 and HBM), in flight together with the LM and lexicon
//   lookups of the frame.  The budget: the lexicon scan's own LDS is 10 KB, the LM scan's 5.5 KB; 32 KiB more keeps a 256-thread
//   workgroup at 42 KB, so three of them still fit the 160 KiB of a CU beside one another, and a 1024-thread one (16 of a CU's 32
//   wavefronts) at two per CU: the matrix never lowers the occupancy the scans have without it.  Both paths do the same fp32
//   operations on the same values.  libw2l_hip_probe.so: W2L_ASG_BEAM_TRANS=global forces the gather (the A/B of tools/).
#pragma once
#include <cstring>

namespace w2l {

constexpr size_t kAsgTransLds = 32 * 1024;

struct BeamAsg {
  static constexpr bool kNoBlank = true;
  // the matrix the scan reads: LDS after a copy by the whole workgroup (the scan's first barrier publishes it), or global memory
  __device__ static __forceinline__ const float* stage(const BeamTrans& tr, int N) {
    extern __shared__ float sAsgTrans[];
    if (!tr.lds) return tr.a;
    for (int i = threadIdx.x; i < N * N; i += blockDim.x) sAsgTrans[i] = tr.a[i];
    return sAsgTrans;
  }
  __device__ static __forceinline__ bool none(int c, int e) { return c == e; }   // a repeated letter is a replabel's work
  // (p + A[c][e]) + lp[c]: two fp32 adds in w2l_viterbi_compute's order; from the empty prefix lp[c] alone
  __device__ static __forceinline__ float ext(float lpc, int c, int e, float, float tot, const float* A, int N) {
    if (c == e) return -INFINITY;
    return e < 0 ? lpc : (tot + A[(size_t)c * N + e]) + lpc;
  }
  __device__ static __forceinline__ void stay(float lpe, int e, float, float pnb, float, const float* A, int N, float* spb,
                                              float* spnb) {
    *spb = -INFINITY;
    *spnb = e >= 0 ? (pnb + A[(size_t)e * N + e]) + lpe : -INFINITY;
  }
};

static BeamTrans asg_beam_trans(const float* trans, int N, size_t* ldsBytes) {
  const size_t bytes = (size_t)N * N * sizeof(float);
  bool lds = bytes <= kAsgTransLds;
  if (const char* v = tune_env("W2L_ASG_BEAM_TRANS")) lds = lds && strcmp(v, "global") != 0;
  *ldsBytes = lds ? bytes : 0;
  return BeamTrans{trans, lds ? 1 : 0};
}

}  // namespace w2l

W2L_API size_t w2l_asg_beam_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::ctc_beam_workspace_size(B, T, N, beam, beamToken, w2l::kBeamLm, true);
}

W2L_API size_t w2l_asg_beam_lex_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::ctc_beam_workspace_size(B, T, N, beam, beamToken, w2l::kBeamLex, true);
}

namespace w2l {
// w2l_asg_beam_search with a silence class and score (BeamSil{}: none, the entry point below; else criterion_beam_sil.hpp)
static int asg_beam_search_do(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
                                int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm,
                                int lmHasEos, float lmWeight, const float* classScore, float eosScore, int* labels, int* lengths,
                                float* scores, float* lmScores, void* workspace, w2l_stream_t stream, BeamSil sil) {
  if (!lmScores || !trans) return W2L_EINVAL;
  if (!(fabsf(lmWeight) < INFINITY) || !(fabsf(eosScore) < INFINITY)) return W2L_EINVAL;
  if (!lmHasEos && eosScore != 0.f) return W2L_EINVAL;
  if (!lm && (lmHasEos || classScore)) return W2L_EINVAL;
  int K = 0;
  if (const int rc = ctc_beam_check(B, T, N, input, beam, beamToken, threshold, nbest, maxLen, labels, lengths, scores, workspace, &K,
                                    true))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  CtcBeamWs ws{};
  if (const int rc = ctc_beam_begin(&ws, kBeamLm, B, T, N, input, frames, beam, K, normalize, workspace, s, true, sil)) return rc;
  size_t lds = 0;
  const BeamTrans tr = asg_beam_trans(trans, N, &lds);
  ctc_beam_fused_scan(beam, K, logAdd, [&](auto la, auto th) {
    hipLaunchKernelGGL((ctc_beam_lm_scan<decltype(la)::value, decltype(th)::value, BeamAsg>), dim3((unsigned)B),
                       dim3(decltype(th)::value), lds, s, T, N, beam, threshold, input, frames, ws, lm, lmWeight, classScore, tr);
  });
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_beam_lm_finish, dim3((unsigned)B), dim3(64), 0, s, nbest, maxLen, N + 1, ws, lm, lmWeight, eosScore,
                     lmHasEos ? 1 : 0, labels, lengths, scores, lmScores);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
}  // namespace w2l

W2L_API int w2l_asg_beam_search(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
                                int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm,
                                int lmHasEos, float lmWeight, const float* classScore, float eosScore, int* labels, int* lengths,
                                float* scores, float* lmScores, void* workspace, w2l_stream_t stream) {
  return w2l::asg_beam_search_do(B, T, N, input, frames, trans, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen, lm,
      lmHasEos, lmWeight, classScore, eosScore, labels, lengths, scores, lmScores, workspace, stream, w2l::BeamSil{});
}

namespace w2l {
// w2l_asg_beam_search_lex with a silence class and score (BeamSil{}: none, the entry point below; else criterion_beam_sil.hpp)
static int asg_beam_search_lex_do(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
                                    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen,
                                    const void* lm, int lmHasEos, float lmWeight, const void* lexicon, float wordScore,
                                    float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
                                    int* words, int* wordCounts, void* workspace, w2l_stream_t stream, BeamSil sil) {
  if (!lmScores || !lm || !lexicon || !words || !wordCounts || maxWords < 1 || !trans) return W2L_EINVAL;
  if (!(fabsf(lmWeight) < INFINITY) || !(fabsf(eosScore) < INFINITY) || !(fabsf(wordScore) < INFINITY)) return W2L_EINVAL;
  if (!lmHasEos && eosScore != 0.f) return W2L_EINVAL;
  int K = 0;
  if (const int rc = ctc_beam_check(B, T, N, input, beam, beamToken, threshold, nbest, maxLen, labels, lengths, scores, workspace, &K,
                                    true))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  CtcBeamWs ws{};
  if (const int rc = ctc_beam_begin(&ws, kBeamLex, B, T, N, input, frames, beam, K, normalize, workspace, s, true, sil)) return rc;
  size_t lds = 0;
  const BeamTrans tr = asg_beam_trans(trans, N, &lds);
  ctc_beam_fused_scan(beam, K, logAdd, [&](auto la, auto th) {
    hipLaunchKernelGGL((ctc_beam_lex_scan<decltype(la)::value, decltype(th)::value, BeamAsg>), dim3((unsigned)B),
                       dim3(decltype(th)::value), lds, s, T, N, beam, threshold, input, frames, ws, lexicon, lm, lmWeight, wordScore,
                       tr);
  });
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_beam_lex_finish, dim3((unsigned)B), dim3(64), 0, s, nbest, maxLen, maxWords, ws, lexicon, lm, lmWeight,
                     eosScore, lmHasEos ? 1 : 0, labels, lengths, scores, lmScores, words, wordCounts);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
}  // namespace w2l

W2L_API int w2l_asg_beam_search_lex(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
                                    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen,
                                    const void* lm, int lmHasEos, float lmWeight, const void* lexicon, float wordScore,
                                    float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
                                    int* words, int* wordCounts, void* workspace, w2l_stream_t stream) {
  return w2l::asg_beam_search_lex_do(B, T, N, input, frames, trans, beam, beamToken, threshold, logAdd, normalize, nbest, maxLen,
      lm, lmHasEos, lmWeight, lexicon, wordScore, eosScore, labels, lengths, scores, lmScores, maxWords, words, wordCounts,
      workspace, stream, w2l::BeamSil{});
}
