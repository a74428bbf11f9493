// criterion_beam_stream.hpp -- w2l_beam_session_*: the CTC beam searches made incremental (contract: include/w2l_hip.h).  Included at
// the end of criterion_ctc.hip after the searches it continues.  A session has S slots; a slot holds the search of one utterance in
// progress: its beam and its prefix table stay in a caller-supplied state buffer between steps, so a step costs its own frames
// alone and a result can be asked for after any of them.  What a result is, is stated by the whole searches: the same device
// helpers in the same order (the scan and finish BODIES of criterion_ctc_beam_lm.hpp / _lex.hpp are the whole searches' own, with
// kResume set), so hypotheses, scores and ranks are theirs bit for bit whatever the chunking.
//   step    ctc_beam_rows<., false, true> over [S][maxChunk] rows (rows at or beyond the slot's count return at once; a count of 0
//           is no rows) into the chunk-sized lse / lpb / tokLp / tokC area, then ONE scan launch, a workgroup per slot:
//           beam_stream_lm_scan (LM-free: lm == null, and token LM) or beam_stream_lex_scan.  A slot with no frames and no start
//           exits at once.  Starting slots have their table cleared on the stream first (one memset per run of adjacent slots).
//   result  beam_stream_finish<lex>: the whole searches' finish bodies over the stored beams; reads state only.
// The per-slot counts and start flags are host arithmetic; they reach the device with one async copy from pinned memory (a ring
// of kBeamRing tables, as the streaming forward's count table does).  Nothing here synchronises or allocates after bind.
// State buffer (every part 256-byte aligned; w2l_beam_session_state_bytes):
//   cnt[S], base[S], flag[S] int   this call's table: frames of this step, frames before it, start / open flags
//   lse, lpb  [S][maxChunk] fp32;  tokLp fp32, tokC int [S][maxChunk][K]         the row pass of this step
//   table     [S][ctc_beam_cap(maxFrames, W)] u64                                 a slot's prefix trie, for its whole utterance
//   n [S] int;  node, tot, state, acc, u, par, e, lab, pb, pnb, su [S][64]        the beams (11 arrays of 4-byte entries)
// THE WIDE SESSION (w2l_beam_session_create_wide; beam up to kBeamWideMax) is the same protocol, bookkeeping and row
// pass over the wide kernels of criterion_beam_wide.hpp: beam_stream_wide_scan is beam_wide_scan's body with kResume set, one
// workgroup of 1024 threads per slot, and beam_stream_wide_finish is beam_wide_finish's body under the open flag and a BeamWalk.
// Its state (w2l_beam_session_wide_state_bytes), every part 256-byte aligned:
//   cnt, base, flag; lse, lpb, tokLp, tokC; table      as above, the table with cap = ctc_beam_cap(maxFrames, W)
//   cand      [S][W K slots + W] u64, slots = 7 with a lexicon, else 1            the candidate keys of ONE frame: scratch, not carried
//   n [S] int;  node, tot, state, acc, par, e, pb, pnb [S][W]; with a lexicon also u, lab [S][W]   the beams (8 or 10 arrays)
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

namespace w2l {

void setHostError(const std::string& m);   // w2l_host_last_error's message (host/trainer.cpp)

constexpr int kBeamRing = 4;   // count tables in flight (pinned): a call reuses one only after the copy out of it has run

struct BeamSessionLayout {
  int* ctl;   // cnt[S], base[S], flag[S]
  CtcBeamWs ws;
  BeamCarry cy;
};

static size_t beam_session_layout(BeamSessionLayout* L, void* state, int S, int maxChunk, int maxFrames, int W, int K) {
  const size_t rows = (size_t)S * maxChunk, cap = ctc_beam_cap(maxFrames, W), ent = align_up((size_t)S * kBeamMax * 4, 256);
  char* p = (char*)state;
  char* const p0 = p;
  auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
  int* ctl = (int*)take((size_t)3 * S * sizeof(int));
  float* lse = (float*)take(rows * sizeof(float));
  float* lpb = (float*)take(rows * sizeof(float));
  float* tokLp = (float*)take(rows * K * sizeof(float));
  int* tokC = (int*)take(rows * K * sizeof(int));
  u64* table = (u64*)take((size_t)S * cap * sizeof(u64));
  int* n = (int*)take((size_t)S * sizeof(int));
  char* arr[11];
  for (int i = 0; i < 11; ++i) arr[i] = take(ent);
  if (L) {
    L->ctl = ctl;
    L->ws = CtcBeamWs{lse, lpb, tokLp, tokC, table, (int*)arr[0], (float*)arr[1], n, (int*)arr[2], (float*)arr[3], (int*)arr[4], K,
                      (unsigned)cap};
    L->cy = BeamCarry{ctl, ctl + 2 * S, (int*)arr[5], (int*)arr[6], (int*)arr[7], (float*)arr[8], (float*)arr[9], (float*)arr[10]};
  }
  return (size_t)(p - p0);
}

struct BeamWideSessionLayout {
  int* ctl;
  BeamWideWs ww;
  BeamWideCarry cy;
};

static size_t beam_session_wide_layout(BeamWideSessionLayout* L, void* state, int S, int maxChunk, int maxFrames, int W, int K,
                                       bool lex) {
  const size_t rows = (size_t)S * maxChunk, cap = ctc_beam_cap(maxFrames, W), ent = align_up((size_t)S * W * 4, 256);
  const size_t candCap = (size_t)W * K * (lex ? 7 : 1) + (size_t)W;
  char* p = (char*)state;
  char* const p0 = p;
  auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
  int* ctl = (int*)take((size_t)3 * S * sizeof(int));
  float* lse = (float*)take(rows * sizeof(float));
  float* lpb = (float*)take(rows * sizeof(float));
  float* tokLp = (float*)take(rows * K * sizeof(float));
  int* tokC = (int*)take(rows * K * sizeof(int));
  u64* table = (u64*)take((size_t)S * cap * sizeof(u64));
  u64* cand = (u64*)take((size_t)S * candCap * sizeof(u64));
  int* n = (int*)take((size_t)S * sizeof(int));
  char* arr[10] = {};
  for (int i = 0; i < (lex ? 10 : 8); ++i) arr[i] = take(ent);
  if (L) {
    L->ctl = ctl;
    L->ww.c = CtcBeamWs{lse, lpb, tokLp, tokC, table, (int*)arr[0], (float*)arr[1], n, (int*)arr[2], (float*)arr[3], (int*)arr[8], K,
                        (unsigned)cap};
    L->ww.cand = cand; L->ww.candCap = candCap; L->ww.W = W;
    L->cy = BeamWideCarry{ctl, ctl + 2 * S, (int*)arr[4], (int*)arr[5], (int*)arr[9], (float*)arr[6], (float*)arr[7]};
  }
  return (size_t)(p - p0);
}

// THE MANY-TOKEN SESSION (w2l_beam_session_create_mt; beam up to kBeamXlMax, beamToken up to kBeamMtMax, a silence score; DESIGN
// 3.30): the same protocol, bookkeeping and row pass over the kernels of criterion_beam_xl.hpp.  The xl scan keeps both halves of
// its beam in memory, so the stored beam is the halves themselves, with (cur, n) beside them.  State, every part 256-byte aligned:
//   cnt, base, flag; lse, lpb, tokLp, tokC; table; cand   as the wide session's
//   gone      [S][slots][W][ceil(K / 64)] u64;  stay [S][2][W] fp32                one frame's scratch, not carried
//   curn      [S][2] int: the current half and its entry count
//   beam      [S][2][kF][W] 4-byte words, kF = 9 with a lexicon, else 8
//   finNode, finTot [S][W]; finN [S]; finState, finAcc [S][W]; with a lexicon finU [S][W]   what the finish reads
struct BeamMtSessionLayout {
  int* ctl;
  BeamXlWs xw;
  BeamXlCarry cy;
};

static size_t beam_session_mt_layout(BeamMtSessionLayout* L, void* state, int S, int maxChunk, int maxFrames, int W, int K, bool lex,
                                     BeamSil sil) {
  const size_t rows = (size_t)S * maxChunk, cap = ctc_beam_cap(maxFrames, W), ent = align_up((size_t)S * W * 4, 256);
  const size_t slots = lex ? 7 : 1, candCap = (size_t)W * K * slots + (size_t)W;
  char* p = (char*)state;
  char* const p0 = p;
  auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
  int* ctl = (int*)take((size_t)3 * S * sizeof(int));
  float* lse = (float*)take(rows * sizeof(float));
  float* lpb = (float*)take(rows * sizeof(float));
  float* tokLp = (float*)take(rows * K * sizeof(float));
  int* tokC = (int*)take(rows * K * sizeof(int));
  u64* table = (u64*)take((size_t)S * cap * sizeof(u64));
  u64* cand = (u64*)take((size_t)S * candCap * sizeof(u64));
  u64* gone = (u64*)take((size_t)S * slots * W * beam_mt_words(K) * sizeof(u64));
  float* stay = (float*)take((size_t)S * 2 * W * sizeof(float));
  int* curn = (int*)take((size_t)S * 2 * sizeof(int));
  int* beam = (int*)take((size_t)S * 2 * (lex ? 9 : 8) * W * 4);
  int* finNode = (int*)take(ent);
  float* finTot = (float*)take(ent);
  int* finN = (int*)take((size_t)S * sizeof(int));
  int* finState = (int*)take(ent);
  float* finAcc = (float*)take(ent);
  int* finU = lex ? (int*)take(ent) : nullptr;
  if (L) {
    L->ctl = ctl;
    L->xw.w.c = CtcBeamWs{lse, lpb, tokLp, tokC, table, finNode, finTot, finN, finState, finAcc, finU, K, (unsigned)cap, sil.token,
                          sil.score};
    L->xw.w.cand = cand; L->xw.w.candCap = candCap; L->xw.w.W = W;
    L->xw.beam = beam; L->xw.gone = gone; L->xw.stay = stay; L->xw.hashN = 2 * beam_xl_pow2(W);
    L->cy = BeamXlCarry{ctl, ctl + 2 * S, curn};
  }
  return (size_t)(p - p0);
}

// the session's kernels: the xl scan with kMt and kResume, the xl finish with kOpen, a BeamXlCarry behind their arguments
template <bool kLogAdd, bool kLex>
constexpr auto beam_stream_mt_scan = beam_xl_scan<kLogAdd, BeamCtc, kLex, true, true, BeamXlCarry>;
template <bool kLex>
constexpr auto beam_stream_mt_finish = beam_xl_finish<kLex, true, BeamXlCarry>;

template <bool kLogAdd, bool kLex>
__global__ __launch_bounds__(kWideThreads) void beam_stream_wide_scan(int T, int N, int W, float threshold,
                                                                      const float* __restrict__ x, BeamWideWs ww,
                                                                      const void* __restrict__ lex, const void* __restrict__ lm,
                                                                      float lmWeight, const float* __restrict__ classScore,
                                                                      float wordScore, BeamWideCarry cy) {
  beam_wide_scan_body<kLogAdd, BeamCtc, kLex, true>(T, N, W, threshold, x, nullptr, ww, lex, lm, lmWeight, classScore, wordScore,
                                                    BeamTrans{}, cy);
}

// as beam_stream_finish below: cy.cnt[slot] bounds the walks, cy.flag[slot] bit 1 says the slot is open
template <bool kLex>
__global__ __launch_bounds__(kWideThreads) void beam_stream_wide_finish(int M, int Lmax, int maxWords, int eosWord, BeamWideWs ww,
                                                                        BeamWideCarry cy, const void* __restrict__ lex,
                                                                        const void* __restrict__ lm, float lmWeight, float eosScore,
                                                                        int useEos, int* __restrict__ labels,
                                                                        int* __restrict__ lengths, float* __restrict__ scores,
                                                                        float* __restrict__ lmScores, int* __restrict__ words,
                                                                        int* __restrict__ wordCounts) {
  const int b = blockIdx.x;
  const int n = (cy.flag[b] & 2) ? min(max(ww.c.finN[b], 0), min(ww.W, kWideThreads)) : 0;
  BeamWalk g;
  g.capm = ww.c.cap - 1;
  g.steps = max(cy.cnt[b], 0);
  beam_wide_finish_body<kLex>(b, n, g, M, Lmax, maxWords, eosWord, ww, lex, lm, lmWeight, eosScore, useEos, labels, lengths, scores,
                              lmScores, words, wordCounts);
}

template <bool kLogAdd, int kThreads>
__global__ __launch_bounds__(kThreads) void beam_stream_lm_scan(int T, int N, int W, float threshold, const float* __restrict__ x,
                                                                CtcBeamWs ws, const void* __restrict__ lm, float lmWeight,
                                                                const float* __restrict__ classScore, BeamCarry cy) {
  beam_lm_scan_body<kLogAdd, kThreads, BeamCtc, true>(T, N, W, threshold, x, nullptr, ws, lm, lmWeight, classScore, BeamTrans{}, cy);
}

template <bool kLogAdd, int kThreads>
__global__ __launch_bounds__(kThreads) void beam_stream_lex_scan(int T, int N, int W, float threshold, const float* __restrict__ x,
                                                                 CtcBeamWs ws, const void* __restrict__ lex,
                                                                 const void* __restrict__ lm, float lmWeight, float wordScore,
                                                                 BeamCarry cy) {
  beam_lex_scan_body<kLogAdd, kThreads, BeamCtc, true>(T, N, W, threshold, x, nullptr, ws, lex, lm, lmWeight, wordScore, BeamTrans{}, cy);
}

// cy.cnt[slot]: the frames the slot has had (no prefix is longer); cy.flag[slot] bit 1: the slot is open.  A closed or never
// started slot has no entries: empty rows.
template <bool kLex>
__global__ __launch_bounds__(64) void beam_stream_finish(int M, int Lmax, int maxWords, int eosWord, CtcBeamWs ws, BeamCarry cy,
                                                         const void* __restrict__ lex, const void* __restrict__ lm, float lmWeight,
                                                         float eosScore, int useEos, int* __restrict__ labels,
                                                         int* __restrict__ lengths, float* __restrict__ scores,
                                                         float* __restrict__ lmScores, int* __restrict__ words,
                                                         int* __restrict__ wordCounts) {
  const int b = blockIdx.x;
  const int n = (cy.flag[b] & 2) ? min(max(ws.finN[b], 0), kBeamMax) : 0;
  BeamWalk g;
  g.capm = ws.cap - 1;
  g.steps = max(cy.cnt[b], 0);
  if constexpr (kLex)
    beam_lex_finish_body(b, n, g, M, Lmax, maxWords, ws, lex, lm, lmWeight, eosScore, useEos, labels, lengths, scores, lmScores, words,
                         wordCounts);
  else
    beam_lm_finish_body(b, n, g, M, Lmax, eosWord, ws, lm, lmWeight, eosScore, useEos, labels, lengths, scores, lmScores);
}

struct BeamSession {
  w2l_beam_session_desc d{};
  int K = 0;
  size_t stateBytes = 0, cap = 0;
  std::vector<int> frames;    // per slot: emission frames fed since its start
  std::vector<char> active;   // per slot: started and not reset
  // w2l_beam_session_commit (criterion_beam_commit.hpp); all 0 for a slot that has not committed since its start
  std::vector<int> doneLabels, doneWords;   // per slot: labels and words committed since its start
  std::vector<int> live;                    // per slot: nodes of its table after its last commit
  std::vector<int> credit;                  // per slot: frames the last commit gave back: frames then - ceil(live / beam)
  int* commitOut = nullptr;                 // pinned [S][4]: a commit's counts
  BeamSessionLayout L{};
  bool wide = false;          // w2l_beam_session_create_wide: the wide kernels over WL
  BeamWideSessionLayout WL{};
  bool mt = false;            // w2l_beam_session_create_mt: the many-token kernels over ML
  BeamMtSessionLayout ML{};
  BeamSil sil;                // the many-token session's; BeamSil{} when there is no silence score
  bool bound = false;
  int* pinned[kBeamRing] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev[kBeamRing] = {nullptr, nullptr, nullptr, nullptr};
  bool evUsed[kBeamRing] = {false, false, false, false};
  int ring = 0;
  ~BeamSession() {
    for (int r = 0; r < kBeamRing; ++r) {
      if (ev[r]) (void)hipEventDestroy(ev[r]);
      if (pinned[r]) (void)hipHostFree(pinned[r]);
    }
    if (commitOut) (void)hipHostFree(commitOut);
  }
};

static int beam_session_fail(int rc, const std::string& m) {
  setHostError(m);
  return rc;
}

enum BeamSessionKind { kSessNarrow = 0, kSessWide = 1, kSessMt = 2 };

// the state a session's row pass writes and its finish reads, and its control ints
static const CtcBeamWs& beam_session_ws(const BeamSession& s) { return s.mt ? s.ML.xw.w.c : s.wide ? s.WL.ww.c : s.L.ws; }
static int* beam_session_ctl(const BeamSession& s) { return s.mt ? s.ML.ctl : s.wide ? s.WL.ctl : s.L.ctl; }

// the descriptor against the whole searches' argument rules; *K = the clipped beamToken
static int beam_session_check(const w2l_beam_session_desc* d, int* K, int kind = kSessNarrow) {
  const bool wide = kind == kSessWide;
  if (!d) return beam_session_fail(W2L_EINVAL, "beam session: null descriptor");
  if (d->slots <= 0 || d->slots > 65535 || d->maxChunk <= 0 || d->maxFrames <= 0 || d->N < 2 || d->beam <= 0 || d->beamToken <= 0 ||
      !(d->threshold >= 0.f))
    return beam_session_fail(W2L_EINVAL, "beam session: slots (1..65535), maxChunk, maxFrames, beam, beamToken must be positive, N >= 2, "
                                         "threshold >= 0");
  if (d->variant != W2L_BEAM_PLAIN && d->variant != W2L_BEAM_LM && d->variant != W2L_BEAM_LEX)
    return beam_session_fail(W2L_EUNSUPPORTED, "beam session: unknown variant " + std::to_string(d->variant));
  if (d->variant == W2L_BEAM_PLAIN) {
    if (d->lm || d->lexicon || d->classScore || d->lmHasEos || d->lmWeight != 0.f || d->eosScore != 0.f || d->wordScore != 0.f)
      return beam_session_fail(W2L_EINVAL, "beam session: the LM-free variant takes no LM, lexicon or score arguments");
  } else {
    if (!d->lm) return beam_session_fail(W2L_EINVAL, "beam session: this variant needs an LM table");
    if (!(fabsf(d->lmWeight) < INFINITY) || !(fabsf(d->eosScore) < INFINITY) || (!d->lmHasEos && d->eosScore != 0.f))
      return beam_session_fail(W2L_EINVAL, "beam session: lmWeight and eosScore must be finite, eosScore 0 without EOS");
    if (d->variant == W2L_BEAM_LM && (d->lexicon || d->wordScore != 0.f))
      return beam_session_fail(W2L_EINVAL, "beam session: the token-LM variant takes no lexicon or wordScore");
    if (d->variant == W2L_BEAM_LEX && (!d->lexicon || d->classScore || !(fabsf(d->wordScore) < INFINITY)))
      return beam_session_fail(W2L_EINVAL, "beam session: the lexicon variant needs a lexicon table, a finite wordScore, no classScore");
  }
  *K = ctc_beam_clip(d->N - 1, d->beamToken);
  if (kind == kSessMt && (d->beam > kBeamXlMax || *K > kBeamMtMax))
    return beam_session_fail(W2L_EUNSUPPORTED, "many-token beam session: beam above 8192 or beamToken (clipped to N - 1) above 256");
  if (wide && (d->beam > kBeamWideMax || *K > kBeamMax))
    return beam_session_fail(W2L_EUNSUPPORTED, "wide beam session: beam above 1024 or beamToken (clipped to N - 1) above 64");
  if (kind == kSessNarrow && (d->beam > kBeamMax || *K > kBeamMax))
    return beam_session_fail(W2L_EUNSUPPORTED, "beam session: beam and beamToken above 64 (the wide searches) are not incremental "
                                               "here; w2l_beam_session_create_wide takes a beam up to 1024");
  if ((size_t)d->maxFrames * d->beam > ((size_t)1 << 29))
    return beam_session_fail(W2L_EUNSUPPORTED, "beam session: maxFrames * beam above 2^29 (node ids are ints)");
  return W2L_OK;
}

// One step's bookkeeping: validates everything first; fills the table (cnt[S], base[S], flag[S]; may be null) and returns the counts
// after the step in `after` without committing them.
static int beam_session_advance(const BeamSession& s, const int* n, const int* start, int* table, std::vector<int>& after,
                                std::vector<char>& activeAfter) {
  if (!n) return beam_session_fail(W2L_EINVAL, "beam session step: null frame counts");
  const int S = s.d.slots;
  for (int i = 0; i < S; ++i) {
    const bool st = start && start[i];
    if (n[i] < 0 || n[i] > s.d.maxChunk)
      return beam_session_fail(W2L_EINVAL, "beam session step: slot " + std::to_string(i) + " was given " + std::to_string(n[i]) +
                                               " frames, outside 0.." + std::to_string(s.d.maxChunk));
    if (!st && !s.active[i] && n[i] > 0)
      return beam_session_fail(W2L_EINVAL, "beam session step: slot " + std::to_string(i) + " is fed before it was started");
    if (!st && (s.credit[i] > 0 || s.live[i] > 0) && s.frames[i] - s.credit[i] + n[i] > s.d.maxFrames)   // a slot that has committed: its budget
      return beam_session_fail(W2L_EINVAL, "beam session step: slot " + std::to_string(i) + " would pass its budget of maxFrames = " +
                                               std::to_string(s.d.maxFrames) + " frames (" + std::to_string(s.live[i]) +
                                               " nodes kept by its last commit count as " +
                                               std::to_string((s.live[i] + s.d.beam - 1) / s.d.beam) + ", " +
                                               std::to_string(s.frames[i] - s.credit[i] - (s.live[i] + s.d.beam - 1) / s.d.beam) +
                                               " fed since, " + std::to_string(n[i]) + " given); commit again or start the slot anew");
    if ((st ? 0 : s.frames[i] - s.credit[i]) + n[i] > s.d.maxFrames)
      return beam_session_fail(W2L_EINVAL, "beam session step: slot " + std::to_string(i) + " would pass maxFrames = " +
                                               std::to_string(s.d.maxFrames) + " (" + std::to_string(st ? 0 : s.frames[i]) + " fed, " +
                                               std::to_string(n[i]) + " given)");
  }
  after = s.frames;
  activeAfter = s.active;
  for (int i = 0; i < S; ++i) {
    const bool st = start && start[i];
    if (st) { after[i] = 0; activeAfter[i] = 1; }
    if (table) { table[i] = n[i]; table[S + i] = after[i]; table[2 * S + i] = st ? 1 : 0; }
    after[i] += n[i];
  }
  return W2L_OK;
}

// f(std::bool_constant<logAdd>, std::bool_constant<lexicon>) for the session's instantiation of the wide or many-token scan
template <class F>
static int beam_session_wide_kernel(const BeamSession& s, F&& f) {
  const bool lex = s.d.variant == W2L_BEAM_LEX;
  if (lex) return s.d.logAdd ? f(std::true_type{}, std::true_type{}) : f(std::false_type{}, std::true_type{});
  return s.d.logAdd ? f(std::true_type{}, std::false_type{}) : f(std::false_type{}, std::false_type{});
}

// the next pinned table of the ring, free to write
// after a step's counts are taken over: a slot that started has committed nothing
static void beam_session_started(BeamSession& s, const int* start) {
  for (int i = 0; start && i < s.d.slots; ++i)
    if (start[i]) s.doneLabels[i] = s.doneWords[i] = s.live[i] = s.credit[i] = 0;
}

static int beam_session_table(BeamSession& s, int** table) {
  const int r = s.ring;
  if (s.evUsed[r]) W2L_HIP_CHECK(hipEventSynchronize(s.ev[r]));   // the copy of kBeamRing calls ago: long done
  *table = s.pinned[r];
  return W2L_OK;
}
static int beam_session_send(BeamSession& s, hipStream_t st) {
  const int r = s.ring;
  W2L_HIP_CHECK(hipMemcpyAsync(beam_session_ctl(s), s.pinned[r], (size_t)3 * s.d.slots * sizeof(int), hipMemcpyHostToDevice, st));
  W2L_HIP_CHECK(hipEventRecord(s.ev[r], st));
  s.evUsed[r] = true;
  s.ring = (r + 1) % kBeamRing;
  return W2L_OK;
}

}  // namespace w2l

W2L_API size_t w2l_beam_session_state_bytes(const w2l_beam_session_desc* desc) {
  using namespace w2l;
  int K = 0;
  if (beam_session_check(desc, &K)) return 0;
  return beam_session_layout(nullptr, nullptr, desc->slots, desc->maxChunk, desc->maxFrames, desc->beam, K);
}

W2L_API size_t w2l_beam_session_wide_state_bytes(const w2l_beam_session_desc* desc) {
  using namespace w2l;
  int K = 0;
  if (beam_session_check(desc, &K, kSessWide)) return 0;
  return beam_session_wide_layout(nullptr, nullptr, desc->slots, desc->maxChunk, desc->maxFrames, desc->beam, K,
                                  desc->variant == W2L_BEAM_LEX);
}

W2L_API size_t w2l_beam_session_mt_state_bytes(const w2l_beam_session_desc* desc) {
  using namespace w2l;
  int K = 0;
  if (beam_session_check(desc, &K, kSessMt)) return 0;
  return beam_session_mt_layout(nullptr, nullptr, desc->slots, desc->maxChunk, desc->maxFrames, desc->beam, K,
                                desc->variant == W2L_BEAM_LEX, BeamSil{});
}

namespace w2l {
static int beam_session_make(const w2l_beam_session_desc* desc, void** session, int kind, BeamSil sil = BeamSil{}) {
  if (!session) return beam_session_fail(W2L_EINVAL, "beam session: null session pointer");
  *session = nullptr;
  if (kind == kSessMt && desc && (!beam_finite(sil.score) || sil.token < -1 || sil.token >= desc->N - 1))
    return beam_session_fail(W2L_EINVAL, "many-token beam session: silScore must be finite, silToken -1 (none) or a token class "
                                         "(0 .. N - 2)");
  int K = 0;
  if (const int rc = beam_session_check(desc, &K, kind)) return rc;
  const bool wide = kind == kSessWide, mt = kind == kSessMt, lex = desc->variant == W2L_BEAM_LEX;
  BeamSession* s = new BeamSession();
  s->d = *desc;
  s->K = K;
  s->wide = wide;
  s->mt = mt;
  s->sil = beam_sil_none(sil) ? BeamSil{} : sil;   // no silence score: a token that matches no class, no + 0
  s->cap = ctc_beam_cap(desc->maxFrames, desc->beam);
  s->stateBytes = mt ? beam_session_mt_layout(nullptr, nullptr, desc->slots, desc->maxChunk, desc->maxFrames, desc->beam, K, lex, s->sil)
                  : wide ? beam_session_wide_layout(nullptr, nullptr, desc->slots, desc->maxChunk, desc->maxFrames, desc->beam, K, lex)
                         : beam_session_layout(nullptr, nullptr, desc->slots, desc->maxChunk, desc->maxFrames, desc->beam, K);
  s->frames.assign(desc->slots, 0);
  s->active.assign(desc->slots, 0);
  s->doneLabels.assign(desc->slots, 0);
  s->doneWords.assign(desc->slots, 0);
  s->live.assign(desc->slots, 0);
  s->credit.assign(desc->slots, 0);
  *session = s;
  return W2L_OK;
}
}  // namespace w2l

W2L_API int w2l_beam_session_create(const w2l_beam_session_desc* desc, void** session) {
  return w2l::beam_session_make(desc, session, w2l::kSessNarrow);
}
W2L_API int w2l_beam_session_create_wide(const w2l_beam_session_desc* desc, void** session) {
  return w2l::beam_session_make(desc, session, w2l::kSessWide);
}
W2L_API int w2l_beam_session_create_mt(const w2l_beam_session_desc* desc, int silToken, float silScore, void** session) {
  return w2l::beam_session_make(desc, session, w2l::kSessMt, w2l::BeamSil{silToken, silScore});
}

W2L_API void w2l_beam_session_destroy(void* session) { delete (w2l::BeamSession*)session; }

W2L_API int w2l_beam_session_bind(void* session, void* state, size_t bytes) {
  using namespace w2l;
  if (!session) return beam_session_fail(W2L_EINVAL, "beam session bind: null session");
  BeamSession& s = *(BeamSession*)session;
  if (!state || ((uintptr_t)state & 255))
    return beam_session_fail(W2L_EINVAL, "beam session bind: the state buffer must be a 256-byte aligned device pointer");
  if (bytes < s.stateBytes)
    return beam_session_fail(W2L_EINVAL, s.mt     ? "beam session bind: the state buffer is smaller than w2l_beam_session_mt_state_bytes"
                                         : s.wide ? "beam session bind: the state buffer is smaller than w2l_beam_session_wide_state_bytes"
                                                  : "beam session bind: the state buffer is smaller than w2l_beam_session_state_bytes");
  const size_t tb = align_up((size_t)3 * s.d.slots * sizeof(int), 256);
  for (int r = 0; r < kBeamRing; ++r) {
    if (!s.pinned[r]) W2L_HIP_CHECK(hipHostMalloc((void**)&s.pinned[r], tb, hipHostMallocDefault));
    if (!s.ev[r]) W2L_HIP_CHECK(hipEventCreateWithFlags(&s.ev[r], hipEventDisableTiming));
  }
  if (!s.commitOut) W2L_HIP_CHECK(hipHostMalloc((void**)&s.commitOut, (size_t)4 * s.d.slots * sizeof(int), hipHostMallocDefault));
  if (s.wide) {   // the scan's 64 or 72 KiB of dynamic LDS are asked for here, so a step is launches alone
    const int rc = beam_session_wide_kernel(s, [&](auto la, auto lx) -> int {
      constexpr bool kLa = decltype(la)::value, kLx = decltype(lx)::value;
      W2L_HIP_CHECK(hipFuncSetAttribute((const void*)beam_stream_wide_scan<kLa, kLx>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)WideLds<kLx>::bytes));
      return W2L_OK;
    });
    if (rc) return rc;
  }
  if (s.mt) {   // the scan's hash and the finish's keys (up to 131 and 128 KiB of dynamic LDS) are asked for here too
    const int rc = beam_session_wide_kernel(s, [&](auto la, auto lx) -> int {
      constexpr bool kLa = decltype(la)::value, kLx = decltype(lx)::value;
      W2L_HIP_CHECK(hipFuncSetAttribute((const void*)beam_stream_mt_scan<kLa, kLx>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)kMtScanLdsMax));
      W2L_HIP_CHECK(hipFuncSetAttribute((const void*)beam_stream_mt_finish<kLx>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)kXlFinishLdsMax));
      return W2L_OK;
    });
    if (rc) return rc;
    beam_session_mt_layout(&s.ML, state, s.d.slots, s.d.maxChunk, s.d.maxFrames, s.d.beam, s.K, s.d.variant == W2L_BEAM_LEX, s.sil);
  } else if (s.wide) beam_session_wide_layout(&s.WL, state, s.d.slots, s.d.maxChunk, s.d.maxFrames, s.d.beam, s.K, s.d.variant == W2L_BEAM_LEX);
  else beam_session_layout(&s.L, state, s.d.slots, s.d.maxChunk, s.d.maxFrames, s.d.beam, s.K);
  s.bound = true;
  // another buffer holds no slot's search
  std::fill(s.frames.begin(), s.frames.end(), 0);
  std::fill(s.active.begin(), s.active.end(), 0);
  for (std::vector<int>* v : {&s.doneLabels, &s.doneWords, &s.live, &s.credit}) std::fill(v->begin(), v->end(), 0);
  return W2L_OK;
}

W2L_API int w2l_beam_session_counts(void* session, const int* h_n, const int* h_start) {
  using namespace w2l;
  if (!session) return beam_session_fail(W2L_EINVAL, "beam session counts: null session");
  BeamSession& s = *(BeamSession*)session;
  std::vector<int> fa;
  std::vector<char> aa;
  if (const int rc = beam_session_advance(s, h_n, h_start, nullptr, fa, aa)) return rc;
  s.frames.swap(fa);
  s.active.swap(aa);
  beam_session_started(s, h_start);
  return W2L_OK;
}

W2L_API int w2l_beam_session_step(void* session, const float* emissions, const int* h_n, const int* h_start, w2l_stream_t stream) {
  using namespace w2l;
  if (!session) return beam_session_fail(W2L_EINVAL, "beam session step: null session");
  BeamSession& s = *(BeamSession*)session;
  if (!s.bound) return beam_session_fail(W2L_EINVAL, "beam session step: no state bound (w2l_beam_session_bind first)");
  std::vector<int> fa;
  std::vector<char> aa;
  if (const int rc = beam_session_advance(s, h_n, h_start, nullptr, fa, aa)) return rc;
  const int S = s.d.slots, C = s.d.maxChunk, N = s.d.N, W = s.d.beam, K = s.K;
  bool frames = false, starts = false;
  for (int i = 0; i < S; ++i) {
    frames = frames || h_n[i] > 0;
    starts = starts || (h_start && h_start[i]);
  }
  if (frames && !emissions) return beam_session_fail(W2L_EINVAL, "beam session step: null emissions");
  if (frames || starts) {
    hipStream_t st = (hipStream_t)stream;
    int* table = nullptr;
    if (const int rc = beam_session_table(s, &table)) return rc;
    (void)beam_session_advance(s, h_n, h_start, table, fa, aa);
    if (const int rc = beam_session_send(s, st)) return rc;
    for (int i = 0; i < S;) {   // a starting slot's table is cleared before its frames: one memset per run of adjacent slots
      if (!(h_start && h_start[i])) { ++i; continue; }
      int j = i + 1;
      while (j < S && h_start[j]) ++j;
      W2L_HIP_CHECK(hipMemsetAsync(beam_session_ws(s).table + (size_t)i * s.cap, 0,
                                   (size_t)(j - i) * s.cap * sizeof(u64), st));
      i = j;
    }
    const CtcBeamWs& ws = beam_session_ws(s);
    const int* cnt = beam_session_ctl(s);
    if (frames) {
      const unsigned rows = (unsigned)((size_t)S * C);
      if (N > kRowThreads * kRowMaxPer)
        hipLaunchKernelGGL((ctc_beam_rows<true, false, true>), dim3(rows), dim3(kRowThreads), 0, st, C, N, s.d.normalize, emissions,
                           cnt, ws);
      else
        hipLaunchKernelGGL((ctc_beam_rows<false, false, true>), dim3(rows), dim3(kRowThreads), 0, st, C, N, s.d.normalize, emissions,
                           cnt, ws);
      W2L_LAUNCH_CHECK();
    }
    if (s.mt) {
      beam_session_wide_kernel(s, [&](auto la, auto lx) -> int {
        constexpr bool kLa = decltype(la)::value, kLx = decltype(lx)::value;
        hipLaunchKernelGGL((beam_stream_mt_scan<kLa, kLx>), dim3((unsigned)S), dim3(kXlThreads),
                           (size_t)s.ML.xw.hashN * 8 + MtLds::bytes, st, C, N, W, s.d.threshold, emissions, (const int*)nullptr, s.ML.xw, s.d.lexicon, s.d.lm,
                           s.d.lmWeight, s.d.classScore, s.d.wordScore, BeamTrans{nullptr, 0}, s.ML.cy);
        return W2L_OK;
      });
    } else if (s.wide) {
      beam_session_wide_kernel(s, [&](auto la, auto lx) -> int {
        constexpr bool kLa = decltype(la)::value, kLx = decltype(lx)::value;
        hipLaunchKernelGGL((beam_stream_wide_scan<kLa, kLx>), dim3((unsigned)S), dim3(kWideThreads), WideLds<kLx>::bytes, st, C, N, W,
                           s.d.threshold, emissions, s.WL.ww, s.d.lexicon, s.d.lm, s.d.lmWeight, s.d.classScore, s.d.wordScore,
                           s.WL.cy);
        return W2L_OK;
      });
    } else {
      ctc_beam_fused_scan(W, K, s.d.logAdd, [&](auto la, auto th) {
        if (s.d.variant == W2L_BEAM_LEX)
          hipLaunchKernelGGL((beam_stream_lex_scan<decltype(la)::value, decltype(th)::value>), dim3((unsigned)S),
                             dim3(decltype(th)::value), 0, st, C, N, W, s.d.threshold, emissions, ws, s.d.lexicon, s.d.lm, s.d.lmWeight,
                             s.d.wordScore, s.L.cy);
        else
          hipLaunchKernelGGL((beam_stream_lm_scan<decltype(la)::value, decltype(th)::value>), dim3((unsigned)S),
                             dim3(decltype(th)::value), 0, st, C, N, W, s.d.threshold, emissions, ws, s.d.lm, s.d.lmWeight,
                             s.d.classScore, s.L.cy);
      });
    }
    W2L_LAUNCH_CHECK();
  }
  s.frames.swap(fa);
  s.active.swap(aa);
  beam_session_started(s, h_start);
  return W2L_OK;
}

W2L_API int w2l_beam_session_result(void* session, int nbest, int maxLen, int* labels, int* lengths, float* scores, float* lmScores,
                                    int maxWords, int* words, int* wordCounts, w2l_stream_t stream) {
  using namespace w2l;
  if (!session) return beam_session_fail(W2L_EINVAL, "beam session result: null session");
  BeamSession& s = *(BeamSession*)session;
  if (!s.bound) return beam_session_fail(W2L_EINVAL, "beam session result: no state bound (w2l_beam_session_bind first)");
  if (nbest < 1 || nbest > s.d.beam || maxLen <= 0)
    return beam_session_fail(W2L_EINVAL, "beam session result: nbest outside 1..beam or maxLen < 1");
  if (!labels || !lengths || !scores || !lmScores) return beam_session_fail(W2L_EINVAL, "beam session result: null output");
  const bool lex = s.d.variant == W2L_BEAM_LEX;
  if (lex && (!words || !wordCounts || maxWords < 1))
    return beam_session_fail(W2L_EINVAL, "beam session result: the lexicon variant writes words and wordCounts (maxWords >= 1)");
  hipStream_t st = (hipStream_t)stream;
  const int S = s.d.slots;
  int* table = nullptr;
  if (const int rc = beam_session_table(s, &table)) return rc;
  for (int i = 0; i < S; ++i) { table[i] = s.frames[i]; table[S + i] = 0; table[2 * S + i] = s.active[i] ? 2 : 0; }
  if (const int rc = beam_session_send(s, st)) return rc;
  const int useEos = s.d.lmHasEos ? 1 : 0;
  const size_t mtLds = (size_t)beam_xl_pow2(s.d.beam) * 8 + (size_t)s.d.beam * 8 + 8;   // beam_xl_finish's keys, scores, LM sums
  if (s.mt && lex)
    hipLaunchKernelGGL(beam_stream_mt_finish<true>, dim3((unsigned)S), dim3(kXlThreads), mtLds, st, nbest, maxLen, maxWords, 0, s.ML.xw,
                       s.d.lexicon, s.d.lm, s.d.lmWeight, s.d.eosScore, useEos, labels, lengths, scores, lmScores, words, wordCounts,
                       s.ML.cy);
  else if (s.mt)
    hipLaunchKernelGGL(beam_stream_mt_finish<false>, dim3((unsigned)S), dim3(kXlThreads), mtLds, st, nbest, maxLen, 0, s.d.N, s.ML.xw,
                       (const void*)nullptr, s.d.lm, s.d.lmWeight, s.d.eosScore, useEos, labels, lengths, scores, lmScores,
                       (int*)nullptr, (int*)nullptr, s.ML.cy);
  else if (s.wide && lex)
    hipLaunchKernelGGL(beam_stream_wide_finish<true>, dim3((unsigned)S), dim3(kWideThreads), 0, st, nbest, maxLen, maxWords, 0, s.WL.ww,
                       s.WL.cy, s.d.lexicon, s.d.lm, s.d.lmWeight, s.d.eosScore, useEos, labels, lengths, scores, lmScores, words,
                       wordCounts);
  else if (s.wide)
    hipLaunchKernelGGL(beam_stream_wide_finish<false>, dim3((unsigned)S), dim3(kWideThreads), 0, st, nbest, maxLen, 0, s.d.N, s.WL.ww,
                       s.WL.cy, nullptr, s.d.lm, s.d.lmWeight, s.d.eosScore, useEos, labels, lengths, scores, lmScores, nullptr, nullptr);
  else if (lex)
    hipLaunchKernelGGL(beam_stream_finish<true>, dim3((unsigned)S), dim3(64), 0, st, nbest, maxLen, maxWords, s.d.N, s.L.ws, s.L.cy,
                       s.d.lexicon, s.d.lm, s.d.lmWeight, s.d.eosScore, useEos, labels, lengths, scores, lmScores, words, wordCounts);
  else
    hipLaunchKernelGGL(beam_stream_finish<false>, dim3((unsigned)S), dim3(64), 0, st, nbest, maxLen, 0, s.d.N, s.L.ws, s.L.cy, nullptr,
                       s.d.lm, s.d.lmWeight, s.d.eosScore, useEos, labels, lengths, scores, lmScores, nullptr, nullptr);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_beam_session_frames(void* session, int slot, int* h_frames) {
  using namespace w2l;
  if (!session || !h_frames) return beam_session_fail(W2L_EINVAL, "beam session frames: null argument");
  BeamSession& s = *(BeamSession*)session;
  if (slot < 0 || slot >= s.d.slots) return beam_session_fail(W2L_EINVAL, "beam session frames: no such slot");
  *h_frames = s.frames[slot];
  return W2L_OK;
}

W2L_API int w2l_beam_session_reset(void* session, int slot) {
  using namespace w2l;
  if (!session) return beam_session_fail(W2L_EINVAL, "beam session reset: null session");
  BeamSession& s = *(BeamSession*)session;
  if (slot < 0 || slot >= s.d.slots) return beam_session_fail(W2L_EINVAL, "beam session reset: no such slot");
  s.frames[slot] = 0;
  s.active[slot] = 0;
  s.doneLabels[slot] = s.doneWords[slot] = s.live[slot] = s.credit[slot] = 0;
  return W2L_OK;
}
