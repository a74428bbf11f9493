// criterion_beam_entry.hpp -- the host side of every whole-utterance beam search (contract: include/w2l_hip.h).  Included at the end
// of criterion_ctc.hip after the kernels' headers; there is no kernel here.  A call, whichever of the named entry points or the
// descriptor call it came through, is one BeamReq (criterion_ctc_beam.hpp) and takes one route:
//   beam_search          the refusals in the contract's order -- the silence arguments', the search's own (beam_req_check), the
//                        shared ones against the family's limits (beam_common_check) -- then the family's run.  A request without a
//                        silence score runs with BeamSil{}, whose token matches no class: the sibling's kernels and bytes, no + 0.
//   beam_narrow_run      W, K <= 64.  The plain CTC search without a silence score is the one-wavefront lazy scan (ctc_beam_scan,
//                        ctc_beam_finish).  It relies on lp_k + tot being non-increasing in k, which a biased tokLp breaks: with a
//                        silence score the search runs ctc_beam_lm_scan<., ., BeamCtc> with lm == NULL, as the ASG search without an
//                        LM does, and ctc_beam_lm_finish without lmScores, on the LM variant's workspace.
//   beam_wide_run, beam_xl_run   criterion_beam_wide.hpp, criterion_beam_xl.hpp; the many-token family is the xl run with mt set
//                        (K <= 64 runs the many-token scan too, and returns the xl twin's bytes).
//   beam_workspace_size  the same map for the workspace sizes.
// The named entry points are one statement each: fill the request, name the family.
#pragma once

namespace w2l {

constexpr int kBeamFamilyMax[4] = {kBeamMax, kBeamWideMax, kBeamXlMax, kBeamXlMax};   // W, by family
constexpr int kBeamFamilyTokens[4] = {kBeamMax, kBeamMax, kBeamMax, kBeamMtMax};      // K, by family

// the family argument of the *_sil and *_lextok entry points, which name no many-token family: anything else is no family
static int beam_sil_family(int family, int last = kFamXl) { return family >= kFamNarrow && family <= last ? family : -1; }

// variant: what the workspace holds beyond the plain search's (CtcBeamVariant).  0: a call the search refuses.  The many-token
// layout depends on T * W as the call refuses it.
static size_t beam_workspace_size(int family, int variant, bool asg, int B, int T, int N, int beam, int beamToken) {
  if (family < kFamNarrow || family > kFamMt || B <= 0 || T <= 0 || N < 2 || beam <= 0 || beamToken <= 0) return 0;
  const int K = ctc_beam_clip(asg ? N : N - 1, beamToken);
  if (beam > kBeamFamilyMax[family] || K > kBeamFamilyTokens[family]) return 0;
  if (family == kFamMt && (size_t)T * beam > ((size_t)1 << 29)) return 0;
  if (family == kFamNarrow) return ctc_beam_layout(nullptr, nullptr, B, T, beam, K, variant);
  if (family == kFamWide) return beam_wide_layout(nullptr, nullptr, B, T, beam, K, variant);
  return beam_xl_layout(nullptr, nullptr, B, T, beam, K, variant, family == kFamMt);
}

// One narrow search after its checks: rows, scan, finish.  K: the clipped beamToken
static int beam_narrow_run(const BeamReq& q, int K) {
  const bool lazy = q.kind == kSearchPlain && q.sil.token < 0;
  const dim3 grid((unsigned)q.B);
  hipStream_t s = q.stream;
  CtcBeamWs ws{};
  ctc_beam_layout(&ws, q.workspace, q.B, q.T, q.beam, K, lazy ? kBeamPlain : q.lex() ? kBeamLex : kBeamLm);
  if (const int rc = beam_rows_launch(q, &ws)) return rc;
  if (lazy) {
    if (q.logAdd) hipLaunchKernelGGL(ctc_beam_scan<true>, grid, dim3(64), 0, s, q.T, q.N, q.beam, q.threshold, q.input, q.frames, ws);
    else hipLaunchKernelGGL(ctc_beam_scan<false>, grid, dim3(64), 0, s, q.T, q.N, q.beam, q.threshold, q.input, q.frames, ws);
    W2L_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_beam_finish, grid, dim3(64), 0, s, q.nbest, q.maxLen, ws, q.labels, q.lengths, q.scores);
    W2L_LAUNCH_CHECK();
    return W2L_OK;
  }
  size_t lds = 0;
  const BeamTrans tr = q.asg ? asg_beam_trans(q.trans, q.N, &lds) : BeamTrans{};
  ctc_beam_fused_scan(q.beam, K, q.logAdd, [&](auto la, auto th) {
    constexpr bool kLa = decltype(la)::value;
    constexpr int kTh = decltype(th)::value;
    auto scan = [&](auto pol) {
      using Pol = decltype(pol);
      if (q.kind == kSearchLextok)
        hipLaunchKernelGGL((beam_lextok_scan<kLa, kTh, Pol>), grid, dim3(kTh), lds, s, q.T, q.N, q.beam, q.threshold, q.input, q.frames,
                           ws, q.lexicon, q.lm, q.lmWeight, q.wordScore, tr);
      else if (q.kind == kSearchLex)
        hipLaunchKernelGGL((ctc_beam_lex_scan<kLa, kTh, Pol>), grid, dim3(kTh), lds, s, q.T, q.N, q.beam, q.threshold, q.input, q.frames,
                           ws, q.lexicon, q.lm, q.lmWeight, q.wordScore, tr);
      else
        hipLaunchKernelGGL((ctc_beam_lm_scan<kLa, kTh, Pol>), grid, dim3(kTh), lds, s, q.T, q.N, q.beam, q.threshold, q.input, q.frames,
                           ws, q.lm, q.lmWeight, q.classScore, tr);
    };
    if (q.asg) scan(BeamAsg{});
    else scan(BeamCtc{});
  });
  W2L_LAUNCH_CHECK();
  const int useEos = q.lmHasEos ? 1 : 0;
  if (q.lex())
    hipLaunchKernelGGL(ctc_beam_lex_finish, grid, dim3(64), 0, s, q.nbest, q.maxLen, q.maxWords, ws, q.lexicon, q.lm, q.lmWeight,
                       q.eosScore, useEos, q.labels, q.lengths, q.scores, q.lmScores, q.words, q.wordCounts);
  else   // without an end term the re-ranking is the identity: the entries come in score order, ties by rank
    hipLaunchKernelGGL(ctc_beam_lm_finish, grid, dim3(64), 0, s, q.nbest, q.maxLen, q.asg ? q.N + 1 : q.N, ws, q.lm, q.lmWeight,
                       q.eosScore, useEos, q.labels, q.lengths, q.scores, q.lmScores);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

// The one route from a request to a kernel family.  The token LM under a lexicon has the narrow and wide families only: beyond
// them every W2L_EINVAL still comes first, then W2L_EUNSUPPORTED.
static int beam_search(const BeamReq& q, int family) {
  if (family < kFamNarrow || family > kFamMt) return W2L_EINVAL;
  if (const int rc = beam_sil_check(q)) return rc;
  if (const int rc = beam_req_check(q)) return rc;
  int K = 0;
  const int rc = beam_common_check(q, kBeamFamilyMax[family], kBeamFamilyTokens[family], &K);
  if (q.kind == kSearchLextok && family > kFamWide) return rc == W2L_EINVAL ? rc : W2L_EUNSUPPORTED;
  if (rc) return rc;
  BeamReq r = q;
  if (beam_sil_none(q.sil)) r.sil = BeamSil{};
  if (family == kFamNarrow) return beam_narrow_run(r, K);
  if (family == kFamWide) return beam_wide_run(r, K);
  return beam_xl_run(r, K, family == kFamMt);
}

}  // namespace w2l

// ---- the named entry points: (ctc | asg) x (plain, lm, lex) x (narrow, wide, xl, sil, mt), and the two lextok ones

W2L_API size_t w2l_ctc_beam_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamNarrow, w2l::kBeamPlain, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, int* labels, int* lengths, float* scores, void* workspace,
    w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchPlain, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .labels = labels, .lengths = lengths, .scores = scores, .workspace = workspace, .stream = (hipStream_t)stream},
      w2l::kFamNarrow);
}

W2L_API size_t w2l_ctc_beam_wide_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamWide, w2l::kBeamLm, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_wide(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, int* labels, int* lengths, float* scores, void* workspace,
    w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchPlain, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .labels = labels, .lengths = lengths, .scores = scores, .workspace = workspace, .stream = (hipStream_t)stream},
      w2l::kFamWide);
}

W2L_API size_t w2l_ctc_beam_xl_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamXl, w2l::kBeamLm, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_xl(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, int* labels, int* lengths, float* scores, void* workspace,
    w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchPlain, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .labels = labels, .lengths = lengths, .scores = scores, .workspace = workspace, .stream = (hipStream_t)stream}, w2l::kFamXl);
}

W2L_API size_t w2l_ctc_beam_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::beam_sil_family(family), w2l::kBeamLm, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_sil(int family, int B, int T, int N, const float* input, const int* frames, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, int* labels, int* lengths, float* scores,
    void* workspace, w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchPlain, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .labels = labels, .lengths = lengths, .scores = scores, .workspace = workspace, .stream = (hipStream_t)stream,
      .sil = {silToken, silScore}}, w2l::beam_sil_family(family));
}

W2L_API size_t w2l_ctc_beam_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamMt, w2l::kBeamLm, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_mt(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, int* labels, int* lengths, float* scores, void* workspace,
    w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchPlain, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .labels = labels, .lengths = lengths, .scores = scores, .workspace = workspace, .stream = (hipStream_t)stream,
      .sil = {silToken, silScore}}, w2l::kFamMt);
}

W2L_API size_t w2l_ctc_beam_lm_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamNarrow, w2l::kBeamLm, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lm(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
    w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore, .eosScore = eosScore, .labels = labels,
      .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace, .stream = (hipStream_t)stream},
      w2l::kFamNarrow);
}

W2L_API size_t w2l_ctc_beam_lm_wide_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamWide, w2l::kBeamLm, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lm_wide(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
    w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore, .eosScore = eosScore, .labels = labels,
      .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace, .stream = (hipStream_t)stream},
      w2l::kFamWide);
}

W2L_API size_t w2l_ctc_beam_lm_xl_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamXl, w2l::kBeamLm, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lm_xl(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
    w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore, .eosScore = eosScore, .labels = labels,
      .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace, .stream = (hipStream_t)stream},
      w2l::kFamXl);
}

W2L_API size_t w2l_ctc_beam_lm_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::beam_sil_family(family), w2l::kBeamLm, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lm_sil(int family, int B, int T, int N, const float* input, const int* frames, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
    w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore, .eosScore = eosScore, .labels = labels,
      .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace, .stream = (hipStream_t)stream,
      .sil = {silToken, silScore}}, w2l::beam_sil_family(family));
}

W2L_API size_t w2l_ctc_beam_lm_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamMt, w2l::kBeamLm, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lm_mt(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
    w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore, .eosScore = eosScore, .labels = labels,
      .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace, .stream = (hipStream_t)stream,
      .sil = {silToken, silScore}}, w2l::kFamMt);
}

W2L_API size_t w2l_ctc_beam_lex_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamNarrow, w2l::kBeamLex, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lex(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon, .wordScore = wordScore, .eosScore = eosScore,
      .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .maxWords = maxWords, .words = words,
      .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream}, w2l::kFamNarrow);
}

W2L_API size_t w2l_ctc_beam_lex_wide_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamWide, w2l::kBeamLex, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lex_wide(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon, .wordScore = wordScore, .eosScore = eosScore,
      .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .maxWords = maxWords, .words = words,
      .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream}, w2l::kFamWide);
}

W2L_API size_t w2l_ctc_beam_lex_xl_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamXl, w2l::kBeamLex, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lex_xl(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon, .wordScore = wordScore, .eosScore = eosScore,
      .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .maxWords = maxWords, .words = words,
      .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream}, w2l::kFamXl);
}

W2L_API size_t w2l_ctc_beam_lex_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::beam_sil_family(family), w2l::kBeamLex, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lex_sil(int family, int B, int T, int N, const float* input, const int* frames, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon, .wordScore = wordScore, .eosScore = eosScore,
      .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .maxWords = maxWords, .words = words,
      .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream, .sil = {silToken, silScore}},
      w2l::beam_sil_family(family));
}

W2L_API size_t w2l_ctc_beam_lex_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamMt, w2l::kBeamLex, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lex_mt(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
    float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon, .wordScore = wordScore, .eosScore = eosScore,
      .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .maxWords = maxWords, .words = words,
      .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream, .sil = {silToken, silScore}}, w2l::kFamMt);
}

W2L_API size_t w2l_asg_beam_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamNarrow, w2l::kBeamLm, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
    w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore,
      .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace,
      .stream = (hipStream_t)stream}, w2l::kFamNarrow);
}

W2L_API size_t w2l_asg_beam_wide_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamWide, w2l::kBeamLm, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_wide(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
    w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore,
      .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace,
      .stream = (hipStream_t)stream}, w2l::kFamWide);
}

W2L_API size_t w2l_asg_beam_xl_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamXl, w2l::kBeamLm, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_xl(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
    w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore,
      .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace,
      .stream = (hipStream_t)stream}, w2l::kFamXl);
}

W2L_API size_t w2l_asg_beam_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::beam_sil_family(family), w2l::kBeamLm, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_sil(int family, int B, int T, int N, const float* input, const int* frames, const float* trans,
    int beam, int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos,
    float lmWeight, const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores,
    void* workspace, w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore,
      .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace,
      .stream = (hipStream_t)stream, .sil = {silToken, silScore}}, w2l::beam_sil_family(family));
}

W2L_API size_t w2l_asg_beam_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamMt, w2l::kBeamLm, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_mt(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const float* classScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, void* workspace,
    w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLm, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .classScore = classScore,
      .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .workspace = workspace,
      .stream = (hipStream_t)stream, .sil = {silToken, silScore}}, w2l::kFamMt);
}

W2L_API size_t w2l_asg_beam_lex_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamNarrow, w2l::kBeamLex, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_lex(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon,
      .wordScore = wordScore, .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores,
      .maxWords = maxWords, .words = words, .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream},
      w2l::kFamNarrow);
}

W2L_API size_t w2l_asg_beam_lex_wide_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamWide, w2l::kBeamLex, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_lex_wide(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon,
      .wordScore = wordScore, .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores,
      .maxWords = maxWords, .words = words, .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream},
      w2l::kFamWide);
}

W2L_API size_t w2l_asg_beam_lex_xl_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamXl, w2l::kBeamLex, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_lex_xl(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon,
      .wordScore = wordScore, .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores,
      .maxWords = maxWords, .words = words, .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream},
      w2l::kFamXl);
}

W2L_API size_t w2l_asg_beam_lex_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::beam_sil_family(family), w2l::kBeamLex, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_lex_sil(int family, int B, int T, int N, const float* input, const int* frames, const float* trans,
    int beam, int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos,
    float lmWeight, const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores,
    float* lmScores, int maxWords, int* words, int* wordCounts, void* workspace, w2l_stream_t stream, int silToken,
    float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon,
      .wordScore = wordScore, .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores,
      .maxWords = maxWords, .words = words, .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream,
      .sil = {silToken, silScore}}, w2l::beam_sil_family(family));
}

W2L_API size_t w2l_asg_beam_lex_mt_workspace_size(int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::kFamMt, w2l::kBeamLex, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_lex_mt(int B, int T, int N, const float* input, const int* frames, const float* trans, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLex, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon,
      .wordScore = wordScore, .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores,
      .maxWords = maxWords, .words = words, .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream,
      .sil = {silToken, silScore}}, w2l::kFamMt);
}

W2L_API size_t w2l_ctc_beam_lextok_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::beam_sil_family(family, w2l::kFamWide), w2l::kBeamLex, false, B, T, N, beam, beamToken);
}

W2L_API int w2l_ctc_beam_search_lextok(int family, int B, int T, int N, const float* input, const int* frames, int beam,
    int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos, float lmWeight,
    const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores, float* lmScores, int maxWords,
    int* words, int* wordCounts, void* workspace, w2l_stream_t stream, int silToken, float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLextok, .B = B, .T = T, .N = N, .input = input, .frames = frames, .beam = beam,
      .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize, .nbest = nbest, .maxLen = maxLen,
      .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon, .wordScore = wordScore, .eosScore = eosScore,
      .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores, .maxWords = maxWords, .words = words,
      .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream, .sil = {silToken, silScore}},
      w2l::beam_sil_family(family));
}

W2L_API size_t w2l_asg_beam_lextok_workspace_size(int family, int B, int T, int N, int beam, int beamToken) {
  return w2l::beam_workspace_size(w2l::beam_sil_family(family, w2l::kFamWide), w2l::kBeamLex, true, B, T, N, beam, beamToken);
}

W2L_API int w2l_asg_beam_search_lextok(int family, int B, int T, int N, const float* input, const int* frames, const float* trans,
    int beam, int beamToken, float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos,
    float lmWeight, const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths, float* scores,
    float* lmScores, int maxWords, int* words, int* wordCounts, void* workspace, w2l_stream_t stream, int silToken,
    float silScore) {
  return w2l::beam_search({.kind = w2l::kSearchLextok, .asg = true, .B = B, .T = T, .N = N, .input = input, .frames = frames,
      .trans = trans, .beam = beam, .beamToken = beamToken, .threshold = threshold, .logAdd = logAdd, .normalize = normalize,
      .nbest = nbest, .maxLen = maxLen, .lm = lm, .lmHasEos = lmHasEos, .lmWeight = lmWeight, .lexicon = lexicon,
      .wordScore = wordScore, .eosScore = eosScore, .labels = labels, .lengths = lengths, .scores = scores, .lmScores = lmScores,
      .maxWords = maxWords, .words = words, .wordCounts = wordCounts, .workspace = workspace, .stream = (hipStream_t)stream,
      .sil = {silToken, silScore}}, w2l::beam_sil_family(family));
}

// ---- the descriptor call

namespace w2l {

static bool beam_desc_ok(const w2l_beam_search_desc* d) {
  return d && d->family >= W2L_BEAM_NARROW && d->family <= W2L_BEAM_MT && d->kind >= W2L_SEARCH_PLAIN && d->kind <= W2L_SEARCH_LEXTOK;
}

// the request a descriptor names, or false: an enumerator out of range, or a field set that the chosen search does not take
static bool beam_desc_req(const w2l_beam_search_desc* d, BeamReq* q) {
  if (!beam_desc_ok(d)) return false;
  const bool asg = d->trans != nullptr, lex = d->kind >= W2L_SEARCH_LEX;
  if (d->kind == W2L_SEARCH_PLAIN && (d->lm || d->lmHasEos || d->lmWeight != 0.f || d->eosScore != 0.f || (!asg && d->lmScores)))
    return false;
  if (!lex && (d->lexicon || d->wordScore != 0.f || d->maxWords || d->words || d->wordCounts)) return false;
  if ((lex || d->kind == W2L_SEARCH_PLAIN) && d->classScore) return false;
  *q = BeamReq{.kind = asg && d->kind == W2L_SEARCH_PLAIN ? (int)kSearchLm : d->kind, .asg = asg, .B = d->B, .T = d->T, .N = d->N,
               .input = d->input, .frames = d->frames, .trans = d->trans, .beam = d->beam, .beamToken = d->beamToken,
               .threshold = d->threshold, .logAdd = d->logAdd, .normalize = d->normalize, .nbest = d->nbest, .maxLen = d->maxLen,
               .lm = d->lm, .lmHasEos = d->lmHasEos, .lmWeight = d->lmWeight, .classScore = d->classScore, .lexicon = d->lexicon,
               .wordScore = d->wordScore, .eosScore = d->eosScore, .labels = d->labels, .lengths = d->lengths, .scores = d->scores,
               .lmScores = d->lmScores, .maxWords = d->maxWords, .words = d->words, .wordCounts = d->wordCounts,
               .sil = {d->silToken, d->silScore}};
  return true;
}

}  // namespace w2l

// like the named size functions, a function of the route and the shape alone
W2L_API size_t w2l_beam_search_workspace_size(const w2l_beam_search_desc* d) {
  if (!w2l::beam_desc_ok(d) || (d->kind == W2L_SEARCH_LEXTOK && d->family > W2L_BEAM_WIDE)) return 0;
  return w2l::beam_workspace_size(d->family, d->kind >= W2L_SEARCH_LEX ? w2l::kBeamLex : w2l::kBeamLm, d->trans != nullptr, d->B, d->T,
                                  d->N, d->beam, d->beamToken);
}

W2L_API int w2l_beam_search(const w2l_beam_search_desc* d, void* workspace, w2l_stream_t stream) {
  w2l::BeamReq q;
  if (!w2l::beam_desc_req(d, &q)) return W2L_EINVAL;
  q.workspace = workspace;
  q.stream = (hipStream_t)stream;
  return w2l::beam_search(q, d->family);
}
