// criterion_ctc_beam_lex.hpp -- w2l_ctc_beam_search_lex: the CTC prefix beam search restricted to the spellings of a lexicon and
// scored by a word-level back-off n-gram LM whose score is smeared down the lexicon trie (contract: include/w2l_hip.h; the lexicon
// table: lexicon.hpp; the LM table and its score rule: ngram_lm.hpp).  Included at the end of criterion_ctc.hip after
// criterion_ctc_beam_lm.hpp: the row kernel (ctc_beam_rows), the prefix table, (+), the workspace layout and the selection rounds
// are the LM search's.
//   ctc_beam_lex_scan    one workgroup of 256 or 1024 threads per utterance.  A hypothesis is a node of the prefix table whose edge
//                        label is (lexicon node reached by the token << 3) | slot -- slot 0: the token moves into the lexicon trie
//                        (or is the silence loop at the root, lexicon node 0), slot 1 + i: it completes word i of that node -- so
//                        two hypotheses that spell the same tokens with other words or word boundaries are two nodes.  Pair (r, k)
//                        = (beam entry, frame token) belongs to thread (r K + k) mod threads, at most kLmPer pairs per thread.
//                        Pass 1: the edge lookup child(u_r, c_k) and the node's record for every pair, all in flight together,
//                        while thread j < n recomputes the one candidate that spells entry j and merges it into stay(j).  Pass 2:
//                        a pair has up to 7 candidates, too many to keep: the thread keeps the best unconsumed one (key, LM
//                        successor, LM log-probability) and a 7-bit mask of the consumed ones; the LM lookups of all pairs are in
//                        flight together.  Selection rounds as in ctc_beam_lm_scan; the owner of a round's winner marks it consumed
//                        and recomputes the pair's next candidate.
//   ctc_beam_lex_finish  one wavefront per utterance, lane r = surviving entry r: entries inside a word are dropped, the
//                        end-of-sentence term, the re-ranking, then labels, words (from the prefix table's labels and the lexicon's
//                        node records), counts and scores of the rows below M.
#pragma once
#include "lexicon.hpp"

namespace w2l {

struct CtcBeamLexWs {
  CtcBeamLmWs l;
  int* finU;   // [B][64] lexicon node of the final entry of rank r
};

static size_t ctc_beam_lex_layout(CtcBeamLexWs* w, void* ws, int B, int T, int W, int K) {
  const size_t base = ctc_beam_lm_layout(w ? &w->l : nullptr, ws, B, T, W, K);   // a multiple of 256
  if (w) w->finU = (int*)((char*)ws + base);
  return base + align_up((size_t)B * kBeamMax * 4, 256);
}

// total descending, r ascending, stay before extension, k ascending, slot ascending
__device__ __forceinline__ unsigned long long beam_lex_key(float total, int r, int ext, int k, int slot) {
  return ((unsigned long long)beam_ord(total) << 32) |
         (unsigned long long)(0xffffffffu - (unsigned)((r << 10) | (ext << 9) | (k << 3) | slot));
}

// a = (lp[c] + base) + (lmWeight * (smear[v] - su)); a completed word: a + ((lmWeight * (q - smear[v])) + wordScore); one fp32
// operation each, in this order
__device__ __forceinline__ float beam_lex_a(float lpc, float base, float lmWeight, float smv, float su) {
  return (lpc + base) + (lmWeight * (smv - su));
}
__device__ __forceinline__ float beam_lex_word(float a, float lmWeight, float q, float smv, float wordScore) {
  return a + ((lmWeight * (q - smv)) + wordScore);
}

// the best candidate of a pair that is not in its consumed mask (meta = nw | hasChildren << 3 | consumed << 4): 0 when none is left
__device__ __forceinline__ void beam_lex_best(const NgramView& lv, const LexView& xv, int v, float a, float smv, unsigned meta, int st,
                                              float lmWeight, float wordScore, int r, int k, unsigned long long* key, int* nst,
                                              float* lq) {
  typedef unsigned long long u64;
  const unsigned done = meta >> 4;
  u64 best = 0ull;
  int bn = 0;
  float bq = 0.f;
  if (((meta >> 3) & 1u) && !(done & 1u)) best = beam_lex_key(a, r, 1, k, 0);
  const int nw = (int)(meta & 7u);
  if (nw > 0 && (done >> 1) != (1u << nw) - 1u) {
    const LexNode& nd = lex_node(xv, v);
    for (int i = 0; i < nw; ++i)
      if (!((done >> (1 + i)) & 1u)) {
        int ns;
        const float q = ngram_q(lv, st, nd.words[i], &ns);
        const u64 kk = beam_lex_key(beam_lex_word(a, lmWeight, q, smv, wordScore), r, 1, k, 1 + i);
        if (kk > best) { best = kk; bn = ns; bq = q; }
      }
  }
  *key = best; *nst = bn; *lq = bq;
}

template <bool kLogAdd, int kThreads>
__global__ __launch_bounds__(kThreads) void ctc_beam_lex_scan(int T, int N, int W, float threshold, const float* __restrict__ x,
                                                              const int* __restrict__ frames, CtcBeamLexWs wsx,
                                                              const void* __restrict__ lex, const void* __restrict__ lm,
                                                              float lmWeight, float wordScore) {
  typedef unsigned long long u64;
  constexpr int kWaves = kThreads / 64;
  // the beam of this frame and the next one: prefix-table node, parent's node, last token, the label of the last extension, lexicon
  // node, its smear (0 at the root), LM state, pb, pnb, tot, unweighted LM sum
  __shared__ int sNode[2][64], sPar[2][64], sE[2][64], sLab[2][64], sU[2][64], sSt[2][64];
  __shared__ float sSu[2][64], sPb[2][64], sPnb[2][64], sTot[2][64], sAcc[2][64];
  __shared__ u64 sGone[7][64];   // per slot and beam entry: frame tokens whose candidate merged into another entry
  __shared__ int sTc[64];
  __shared__ float sTl[64];
  __shared__ u64 sRed[2][kWaves];
  const CtcBeamWs& ws = wsx.l.b;
  const int b = blockIdx.x, tid = threadIdx.x, K = ws.K;
  const int F = align_frames(frames, b, T);
  const float* xb = x + (size_t)b * T * N;
  u64* tab = ws.table + (size_t)b * ws.cap;
  const unsigned capm = ws.cap - 1;
  const size_t row0 = (size_t)b * T;
  const NgramView lv = ngram_view(lm);
  const LexView xv = lex_view(lex);

  int cur = 0, n = 1;
  if (tid < 64) {
    sNode[0][tid] = tid == 0 ? 0 : -2; sPar[0][tid] = -1; sE[0][tid] = -1; sLab[0][tid] = -1; sU[0][tid] = 0; sSu[0][tid] = 0.f;
    sPb[0][tid] = tid == 0 ? 0.f : -INFINITY; sPnb[0][tid] = -INFINITY; sTot[0][tid] = tid == 0 ? 0.f : -INFINITY;
    sSt[0][tid] = (int)((const NgramHeader*)lm)->start; sAcc[0][tid] = 0.f;
  }
  for (int t = 0; t < F && n > 0; ++t) {
    const size_t row = row0 + t;
    if (tid < 64) {
      sTc[tid] = tid < K ? ws.tokC[row * K + tid] : -2;
      sTl[tid] = tid < K ? ws.tokLp[row * K + tid] : -INFINITY;
    }
    for (int i = tid; i < 7 * 64; i += kThreads) (&sGone[0][0])[i] = 0ull;
    const float lpb = ws.lpb[row], lse = ws.lse[row];
    __syncthreads();
    const int nxt = cur ^ 1, total = n * K;

    // pass 1: every pair's lexicon edge and node record
    int pv[kLmPer];          // the lexicon node the token reaches; 0: the silence loop at the root; -1: no candidate
    float pa[kLmPer];        // a (the silence loop: lp + base)
    float psm[kLmPer];       // smear[v]
    unsigned pmeta[kLmPer];  // nw | hasChildren << 3 | consumed << 4
#pragma unroll
    for (int i = 0; i < kLmPer; ++i) {
      pv[i] = -1; pa[i] = -INFINITY; psm[i] = 0.f; pmeta[i] = 0u;
      const int idx = tid + kThreads * i;
      if (idx < total) {
        const int r = idx / K, k = idx - r * K, c = sTc[k], u = sU[cur][r];
        const float base = c == sE[cur][r] ? sPb[cur][r] : sTot[cur][r];
        if (c == xv.silToken && u == 0) {
          pv[i] = 0; pa[i] = sTl[k] + base; pmeta[i] = 8u;
        } else {
          const int v = lex_child(xv, u, c);
          if (v > 0) {
            const LexNode& nd = lex_node(xv, v);
            pv[i] = v; psm[i] = nd.smear; pmeta[i] = (unsigned)lex_nw(nd) | (lex_has_children(nd) ? 8u : 0u);
            pa[i] = beam_lex_a(sTl[k], base, lmWeight, psm[i], sSu[cur][r]);
          }
        }
      }
    }
    // stay(tid), with the candidate that spells this entry merged in
    u64 stayKey = 0ull;
    float spb = -INFINITY, spnb = -INFINITY, stot = -INFINITY;
    if (tid < n) {
      const int e = sE[cur][tid], par = sPar[cur][tid], lab = sLab[cur][tid];
      int kj = -1, pr = -1;
      for (int k = 0; k < K; ++k) kj = sTc[k] == e ? k : kj;
      for (int r = 0; r < n; ++r) pr = sNode[cur][r] == par ? r : pr;
      spb = lpb + sTot[cur][tid];
      if (e >= 0) spnb = (xb[(size_t)t * N + e] - lse) + sPnb[cur][tid];   // lp[e] comes from the row whether or not e is a frame token
      if (pr >= 0 && kj >= 0 && lab >= 0) {
        const int vj = lab >> 3, slot = lab & 7;
        const float base = e == sE[cur][pr] ? sPb[cur][pr] : sTot[cur][pr];
        float v;
        if (vj == 0) {
          v = sTl[kj] + base;
        } else {
          const LexNode& nd = lex_node(xv, vj);
          const float smv = nd.smear;
          v = beam_lex_a(sTl[kj], base, lmWeight, smv, sSu[cur][pr]);
          if (slot > 0) {
            int unused;
            const float qm = ngram_q(lv, sSt[cur][pr], nd.words[min(slot - 1, kLexMaxWords - 1)], &unused);
            v = beam_lex_word(v, lmWeight, qm, smv, wordScore);
          }
        }
        spnb = beam_oplus<kLogAdd>(spnb, v);
        atomicOr(&sGone[min(slot, 6)][pr], 1ull << kj);
      }
      stot = beam_oplus<kLogAdd>(spb, spnb);
      stayKey = beam_lex_key(stot, tid, 0, 0, 0);
    }
    __syncthreads();
    // pass 2: every pair's best candidate among those that did not merge
    u64 key[kLmPer];
    int nst[kLmPer];
    float lq[kLmPer];
    u64 local = stayKey;
#pragma unroll
    for (int i = 0; i < kLmPer; ++i) {
      key[i] = 0ull; nst[i] = 0; lq[i] = 0.f;
      const int idx = tid + kThreads * i;
      if (idx < total && pv[i] >= 0) {
        const int r = idx / K, k = idx - r * K;
        unsigned done = 0u;
#pragma unroll
        for (int s = 0; s < 7; ++s) done |= (unsigned)((sGone[s][r] >> k) & 1ull) << s;
        pmeta[i] |= done << 4;
        beam_lex_best(lv, xv, pv[i], pa[i], psm[i], pmeta[i], sSt[cur][r], lmWeight, wordScore, r, k, &key[i], &nst[i], &lq[i]);
      }
      local = key[i] > local ? key[i] : local;
    }

    int q = 0;
    float best = 0.f;
    while (q < W) {
      const u64 wm = wave_max_u64(local);
      if ((tid & 63) == 0) sRed[q & 1][tid >> 6] = wm;
      __syncthreads();
      u64 wk = sRed[q & 1][0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) wk = sRed[q & 1][w] > wk ? sRed[q & 1][w] : wk;
      if (wk == 0ull) break;
      const float wtot = beam_unord((unsigned)(wk >> 32));
      if (q == 0) best = wtot;
      if (wtot == -INFINITY || wtot < best - threshold) break;   // candidates come in descending order: the rest fails too
      const unsigned tie = 0xffffffffu - (unsigned)wk;
      const int wr = (int)(tie >> 10), wext = (int)((tie >> 9) & 1u), wkk = (int)((tie >> 3) & 63u), wslot = (int)(tie & 7u);
      bool mine = false;
      if (!wext) {
        if (tid == wr) {
          sNode[nxt][q] = sNode[cur][tid]; sPar[nxt][q] = sPar[cur][tid]; sE[nxt][q] = sE[cur][tid]; sLab[nxt][q] = sLab[cur][tid];
          sU[nxt][q] = sU[cur][tid]; sSu[nxt][q] = sSu[cur][tid]; sSt[nxt][q] = sSt[cur][tid]; sAcc[nxt][q] = sAcc[cur][tid];
          sPb[nxt][q] = spb; sPnb[nxt][q] = spnb; sTot[nxt][q] = stot;
          stayKey = 0ull;
          mine = true;
        }
      } else {
        const int idx = wr * K + wkk;
        if (tid == idx % kThreads) {
          const int at = idx / kThreads;
          int v = 0, ns = 0;
          float a = 0.f, smv = 0.f, q1 = 0.f;
          unsigned meta = 0u;
#pragma unroll
          for (int i = 0; i < kLmPer; ++i)
            if (i == at) { v = pv[i]; a = pa[i]; smv = psm[i]; meta = pmeta[i]; ns = nst[i]; q1 = lq[i]; }
          const bool word = wslot > 0;
          sNode[nxt][q] = -1; sPar[nxt][q] = sNode[cur][wr]; sE[nxt][q] = sTc[wkk]; sLab[nxt][q] = (v << 3) | wslot;
          sU[nxt][q] = word ? 0 : v; sSu[nxt][q] = (word || v == 0) ? 0.f : smv;
          sSt[nxt][q] = word ? ns : sSt[cur][wr]; sAcc[nxt][q] = word ? sAcc[cur][wr] + q1 : sAcc[cur][wr];
          sPb[nxt][q] = -INFINITY; sPnb[nxt][q] = wtot; sTot[nxt][q] = wtot;
          meta |= 1u << (4 + wslot);
          u64 nk;
          beam_lex_best(lv, xv, v, a, smv, meta, sSt[cur][wr], lmWeight, wordScore, wr, wkk, &nk, &ns, &q1);
#pragma unroll
          for (int i = 0; i < kLmPer; ++i)
            if (i == at) { pmeta[i] = meta; key[i] = nk; nst[i] = ns; lq[i] = q1; }
          mine = true;
        }
      }
      if (mine) {
        local = stayKey;
#pragma unroll
        for (int i = 0; i < kLmPer; ++i) local = key[i] > local ? key[i] : local;
      }
      ++q;
    }
    __syncthreads();
    n = q;
    if (tid < n && sNode[nxt][tid] == -1) {   // a new hypothesis: find or make its node of the prefix table
      const u64 edge = ((u64)(unsigned)sPar[nxt][tid] << 32) | (u64)(unsigned)(sLab[nxt][tid] + 1);
      unsigned h = beam_hash(edge) & capm;
      for (unsigned probe = 0; probe <= capm; ++probe) {   // load factor <= 1/2: a free slot ends the chain long before
        const u64 old = atomicCAS(&tab[h], 0ull, edge);
        if (old == 0ull || old == edge) break;
        h = (h + 1) & capm;
      }
      sNode[nxt][tid] = (int)h + 1;
    }
    __syncthreads();
    cur = nxt;
  }
  if (tid < 64) {
    const bool live = tid < n;
    ws.finNode[b * kBeamMax + tid] = live ? sNode[cur][tid] : -1;
    ws.finTot[b * kBeamMax + tid] = live ? sTot[cur][tid] : -INFINITY;
    wsx.l.finState[b * kBeamMax + tid] = live ? sSt[cur][tid] : 0;
    wsx.l.finAcc[b * kBeamMax + tid] = live ? sAcc[cur][tid] : -INFINITY;
    wsx.finU[b * kBeamMax + tid] = live ? sU[cur][tid] : -1;
    if (tid == 0) ws.finN[b] = n;
  }
}

__global__ __launch_bounds__(64) void ctc_beam_lex_finish(int M, int Lmax, int maxWords, CtcBeamLexWs wsx, const void* __restrict__ lex,
                                                          const void* __restrict__ lm, float lmWeight, float eosScore, int useEos,
                                                          int* __restrict__ labels, int* __restrict__ lengths,
                                                          float* __restrict__ scores, float* __restrict__ lmScores,
                                                          int* __restrict__ words, int* __restrict__ wordCounts) {
  typedef unsigned long long u64;
  __shared__ float sScore[64];
  __shared__ int sAlive[64];
  const CtcBeamWs& ws = wsx.l.b;
  const int b = blockIdx.x, r = threadIdx.x;
  const u64* tab = ws.table + (size_t)b * ws.cap;
  const LexView xv = lex_view(lex);
  const int n = ws.finN[b];
  const bool alive = r < n && wsx.finU[b * kBeamMax + r] == 0;   // only finished words count at the end
  float score = -INFINITY, acc = -INFINITY;
  if (alive) {
    score = ws.finTot[b * kBeamMax + r];
    acc = wsx.l.finAcc[b * kBeamMax + r];
    if (useEos) {
      const NgramView lv = ngram_view(lm);
      int unused;
      const float qe = ngram_q(lv, wsx.l.finState[b * kBeamMax + r], (int)((const NgramHeader*)lm)->numTokens + 1, &unused);
      score = score + ((lmWeight * qe) + eosScore);
      acc = acc + qe;
    }
  }
  sScore[r] = score;
  sAlive[r] = alive ? 1 : 0;
  __syncthreads();
  int na = 0, m = 0, deadBefore = 0;
  for (int o = 0; o < 64; ++o) {
    na += sAlive[o];
    m += (sAlive[o] && (sScore[o] > score || (sScore[o] == score && o < r))) ? 1 : 0;
    deadBefore += (!sAlive[o] && o < r) ? 1 : 0;
  }
  if (!alive) m = na + deadBefore;   // rows na .. M-1 are the empty ones: the other lanes, in lane order
  if (m >= M) return;
  int* lab = labels + ((size_t)b * M + m) * Lmax;
  int* wrd = words + ((size_t)b * M + m) * maxWords;
  int len = 0, nwords = 0;
  if (alive) {
    const int node = ws.finNode[b * kBeamMax + r];
    for (int p = node; p > 0;) {
      const u64 edge = tab[p - 1];
      ++len;
      nwords += (((unsigned)edge - 1u) & 7u) ? 1 : 0;
      p = (int)(edge >> 32);
    }
    int i = len - 1, j = nwords - 1;
    for (int p = node; p > 0; --i) {
      const u64 edge = tab[p - 1];
      const unsigned l = (unsigned)edge - 1u;
      const int v = (int)(l >> 3), slot = (int)(l & 7u);
      const LexNode& nd = lex_node(xv, v);
      if (i < Lmax) lab[i] = v == 0 ? xv.silToken : nd.tok;
      if (slot > 0) {
        if (j < maxWords) wrd[j] = nd.words[min(slot - 1, kLexMaxWords - 1)];
        --j;
      }
      p = (int)(edge >> 32);
    }
  }
  for (int i = min(len, Lmax); i < Lmax; ++i) lab[i] = -1;
  for (int j = min(nwords, maxWords); j < maxWords; ++j) wrd[j] = -1;
  lengths[(size_t)b * M + m] = alive ? len : -1;
  wordCounts[(size_t)b * M + m] = alive ? nwords : -1;
  scores[(size_t)b * M + m] = score;
  lmScores[(size_t)b * M + m] = acc;
}

}  // namespace w2l

W2L_API size_t w2l_ctc_beam_lex_workspace_size(int B, int T, int N, int beam, int beamToken) {
  if (B <= 0 || T <= 0 || N < 2 || beam <= 0 || beamToken <= 0) return 0;
  const int K = w2l::ctc_beam_clip(N, beamToken);
  if (beam > w2l::kBeamMax || K > w2l::kBeamMax) return 0;
  return w2l::ctc_beam_lex_layout(nullptr, nullptr, B, T, beam, K);
}

W2L_API int w2l_ctc_beam_search_lex(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
                                    float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos,
                                    float lmWeight, const void* lexicon, float wordScore, float eosScore, int* labels, int* lengths,
                                    float* scores, float* lmScores, int maxWords, int* words, int* wordCounts, void* workspace,
                                    w2l_stream_t stream) {
  using namespace w2l;
  if (B <= 0 || T <= 0 || N < 2 || !input || !labels || !lengths || !scores || !lmScores || !workspace || !lm) return W2L_EINVAL;
  if (!lexicon || !words || !wordCounts || maxWords < 1) return W2L_EINVAL;
  if (beam <= 0 || beamToken <= 0 || nbest <= 0 || nbest > beam || maxLen <= 0) return W2L_EINVAL;
  if (!(threshold >= 0.f)) return W2L_EINVAL;   // NaN or negative
  if (!(fabsf(lmWeight) < INFINITY) || !(fabsf(eosScore) < INFINITY) || !(fabsf(wordScore) < INFINITY)) return W2L_EINVAL;
  if (!lmHasEos && eosScore != 0.f) return W2L_EINVAL;
  const int K = ctc_beam_clip(N, beamToken);
  if (beam > kBeamMax || K > kBeamMax) return W2L_EUNSUPPORTED;
  if ((size_t)T * beam > ((size_t)1 << 29)) return W2L_EUNSUPPORTED;   // node ids are ints
  hipStream_t s = (hipStream_t)stream;
  CtcBeamLexWs ws{};
  ctc_beam_lex_layout(&ws, workspace, B, T, beam, K);
  W2L_HIP_CHECK(hipMemsetAsync(ws.l.b.table, 0, (size_t)B * ws.l.b.cap * sizeof(unsigned long long), s));
  const unsigned rows = (unsigned)((size_t)B * T);
  if (N <= kRowThreads * kRowMaxPer)
    hipLaunchKernelGGL(ctc_beam_rows<false>, dim3(rows), dim3(kRowThreads), 0, s, T, N, normalize, input, frames, ws.l.b);
  else
    hipLaunchKernelGGL(ctc_beam_rows<true>, dim3(rows), dim3(kRowThreads), 0, s, T, N, normalize, input, frames, ws.l.b);
  W2L_LAUNCH_CHECK();
  const bool wide = beam * K > 256 * kLmPer;
#define W2L_LEX_SCAN(LA, TH)                                                                                                    \
  hipLaunchKernelGGL((ctc_beam_lex_scan<LA, TH>), dim3((unsigned)B), dim3(TH), 0, s, T, N, beam, threshold, input, frames, ws, lexicon, \
                     lm, lmWeight, wordScore)
  if (logAdd) { if (wide) W2L_LEX_SCAN(true, 1024); else W2L_LEX_SCAN(true, 256); }
  else { if (wide) W2L_LEX_SCAN(false, 1024); else W2L_LEX_SCAN(false, 256); }
#undef W2L_LEX_SCAN
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_beam_lex_finish, dim3((unsigned)B), dim3(64), 0, s, nbest, maxLen, maxWords, ws, lexicon, lm, lmWeight,
                     eosScore, lmHasEos ? 1 : 0, labels, lengths, scores, lmScores, words, wordCounts);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
