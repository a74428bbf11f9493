// criterion_ctc_beam_lex.hpp -- w2l_ctc_beam_search_lex: the CTC prefix beam search restricted to the spellings of a lexicon and
// scored by a word-level back-off n-gram LM whose score is smeared down the lexicon trie (contract: include/w2l_hip.h; the lexicon
// table: lexicon.hpp; the LM table and its score rule: ngram_lm.hpp).  Included at the end of criterion_ctc.hip after
// criterion_ctc_beam_lm.hpp.  criterion_ctc_beam.hpp owns the row kernel (ctc_beam_rows), the workspace, the prefix table, the keys,
// (+), the entry-point plumbing and the parts of a workgroup scan and of a finish shared with the token-LM search (frame load,
// front of a stay, selection round, final store; chain length, end-of-sentence term, re-rank).  This file keeps what is particular
// to the lexicon: the totals of its candidates (beam_lex_a, beam_lex_word), a pair's best-of-seven with its consumed mask
// (beam_lex_best), the two passes of a frame, and the finish's walk that rebuilds tokens and words from labels and node records.
// The lattice is a policy (BeamCtc, the default; BeamAsg of criterion_asg_beam.hpp).
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

// a = a0 + (lmWeight * (smear[v] - su)), a0 the policy's acoustic sum (CTC: lp[c] + base); a completed word:
// a + ((lmWeight * (q - smear[v])) + wordScore); one fp32 operation each, in this order
__device__ __forceinline__ float beam_lex_a(float a0, float lmWeight, float smv, float su) {
  return a0 + (lmWeight * (smv - su));
}
__device__ __forceinline__ float beam_lex_word(float a, float lmWeight, float q, float smv, float wordScore) {
  return a + ((lmWeight * (q - smv)) + wordScore);
}

// a token LM under the lexicon (criterion_beam_lextok.hpp, the wide scan's kTok): a = a0 + (lmWeight * q), q the token's
// log-probability; a completed word: a + wordScore
__device__ __forceinline__ float beam_lextok_a(float a0, float lmWeight, float q) { return a0 + (lmWeight * q); }

// the best candidate of a pair that is not in its consumed mask (meta = nw | hasChildren << 3 | consumed << 4): 0 when none is left
__device__ __forceinline__ void beam_lex_best(const NgramView& lv, const LexView& xv, int v, float a, float smv, unsigned meta, int st,
                                              float lmWeight, float wordScore, int r, int k, u64* key, int* nst,
                                              float* lq) {
  const unsigned done = meta >> 4;
  u64 best = 0ull;
  int bn = 0;
  float bq = 0.f;
  if (((meta >> 3) & 1u) && !(done & 1u)) best = beam_key(a, r, 1, k, 0);
  const int nw = (int)(meta & 7u);
  if (nw > 0 && (done >> 1) != (1u << nw) - 1u) {
    const LexNode& nd = lex_node(xv, v);
    for (int i = 0; i < nw; ++i)
      if (!((done >> (1 + i)) & 1u)) {
        int ns;
        const float q = ngram_q(lv, st, nd.words[i], &ns);
        const u64 kk = beam_key(beam_lex_word(a, lmWeight, q, smv, wordScore), r, 1, k, 1 + i);
        if (kk > best) { best = kk; bn = ns; bq = q; }
      }
  }
  *key = best; *nst = bn; *lq = bq;
}

// kResume: utterance b is a slot of a beam session (beam_lm_scan_body, criterion_beam_stream.hpp)
template <bool kLogAdd, int kThreads, class Pol, bool kResume>
__device__ __forceinline__ void beam_lex_scan_body(int T, int N, int W, float threshold, const float* __restrict__ x,
                                                   const int* __restrict__ frames, const CtcBeamWs& ws,
                                                   const void* __restrict__ lex, const void* __restrict__ lm, float lmWeight,
                                                   float wordScore, BeamTrans tr, const BeamCarry& cy) {
  constexpr int kWaves = kThreads / 64;
  // the beam of this frame and the next one: prefix-table node, parent's node, last token, the label of the last extension, lexicon
  // node, its smear (0 at the root), LM state, pb, pnb, tot, unweighted LM sum
  __shared__ int sNode[2][64], sPar[2][64], sE[2][64], sLab[2][64], sU[2][64], sSt[2][64];
  __shared__ float sSu[2][64], sPb[2][64], sPnb[2][64], sTot[2][64], sAcc[2][64];
  __shared__ u64 sGone[7][64];   // per slot and beam entry: frame tokens whose candidate merged into another entry
  __shared__ int sTc[64];
  __shared__ float sTl[64];
  __shared__ u64 sRed[2][kWaves];
  const int b = blockIdx.x, tid = threadIdx.x, K = ws.K;
  int F;
  bool fresh = true;
  if constexpr (kResume) {
    if (!beam_carry_begin(cy, b, T, &F, &fresh)) return;
  } else {
    F = align_frames(frames, b, T);
  }
  const float* xb = x + (size_t)b * T * N;
  u64* tab = ws.table + (size_t)b * ws.cap;
  const unsigned capm = ws.cap - 1;
  const size_t row0 = (size_t)b * T;
  const NgramView lv = ngram_view(lm);
  const LexView xv = lex_view(lex);
  const float* A = Pol::stage(tr, N);

  int cur = 0, n = 1;
  if (!fresh) {
    n = beam_carry_load(cy, ws, b, N, sNode[0], sPar[0], sE[0], sPb[0], sPnb[0], sTot[0], sSt[0], sAcc[0], sLab[0], sU[0], sSu[0]);
  } else if (tid < 64) {
    sNode[0][tid] = tid == 0 ? 0 : -2; sPar[0][tid] = -1; sE[0][tid] = -1; sLab[0][tid] = -1; sU[0][tid] = 0; sSu[0][tid] = 0.f;
    sPb[0][tid] = tid == 0 ? 0.f : -INFINITY; sPnb[0][tid] = -INFINITY; sTot[0][tid] = tid == 0 ? 0.f : -INFINITY;
    sSt[0][tid] = (int)((const NgramHeader*)lm)->start; sAcc[0][tid] = 0.f;
  }
  if constexpr (kResume) __syncthreads();   // F may be 0: the store below reads what other threads wrote
  for (int t = 0; t < F && n > 0; ++t) {
    const size_t row = row0 + t;
    beam_load_frame(ws, row, sTc, sTl);
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
        const float a0 = Pol::ext(sTl[k], c, sE[cur][r], sPb[cur][r], sTot[cur][r], A, N);
        if (Pol::none(c, sE[cur][r])) {   // no candidates
        } else if (c == xv.silToken && u == 0) {
          pv[i] = 0; pa[i] = a0; pmeta[i] = 8u;
        } else {
          const int v = lex_child(xv, u, c);
          if (v > 0) {
            const LexNode& nd = lex_node(xv, v);
            pv[i] = v; psm[i] = nd.smear; pmeta[i] = (unsigned)lex_nw(nd) | (lex_has_children(nd) ? 8u : 0u);
            pa[i] = beam_lex_a(a0, lmWeight, psm[i], sSu[cur][r]);
          }
        }
      }
    }
    // stay(tid), with the candidate that spells this entry merged in
    u64 stayKey = 0ull;
    float spb = -INFINITY, spnb = -INFINITY, stot = -INFINITY;
    if (tid < n) {
      const BeamStay s = beam_stay_front<Pol>(n, K, sTc, sTl, sNode[cur], sPar[cur], sE[cur], sPb[cur], sPnb[cur], sTot[cur],
                                              xb + (size_t)t * N, lpb, lse, A, N, ws.sil, ws.silScore);
      const int lab = sLab[cur][tid];
      spb = s.spb; spnb = s.spnb;
      if (s.merge && lab >= 0) {
        const int vj = lab >> 3, slot = lab & 7;
        float v;
        if (vj == 0) {
          v = s.a;
        } else {
          const LexNode& nd = lex_node(xv, vj);
          const float smv = nd.smear;
          v = beam_lex_a(s.a, lmWeight, smv, sSu[cur][s.pr]);
          if (slot > 0) {
            int unused;
            const float qm = ngram_q(lv, sSt[cur][s.pr], nd.words[min(slot - 1, kLexMaxWords - 1)], &unused);
            v = beam_lex_word(v, lmWeight, qm, smv, wordScore);
          }
        }
        spnb = beam_oplus<kLogAdd>(spnb, v);
        atomicOr(&sGone[min(slot, 6)][s.pr], 1ull << s.kj);
      }
      stot = beam_oplus<kLogAdd>(spb, spnb);
      stayKey = beam_key(stot, tid, 0, 0);
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
      BeamWin w;
      if (!beam_select_round<kWaves>(local, q, sRed, threshold, &best, &w)) break;
      bool mine = false;
      if (!w.ext) {
        if (tid == w.r) {
          sNode[nxt][q] = sNode[cur][tid]; sPar[nxt][q] = sPar[cur][tid]; sE[nxt][q] = sE[cur][tid]; sLab[nxt][q] = sLab[cur][tid];
          sU[nxt][q] = sU[cur][tid]; sSu[nxt][q] = sSu[cur][tid]; sSt[nxt][q] = sSt[cur][tid]; sAcc[nxt][q] = sAcc[cur][tid];
          sPb[nxt][q] = spb; sPnb[nxt][q] = spnb; sTot[nxt][q] = stot;
          stayKey = 0ull;
          mine = true;
        }
      } else {
        const int idx = w.r * K + w.k;
        if (tid == idx % kThreads) {
          const int at = idx / kThreads;
          int v = 0, ns = 0;
          float a = 0.f, smv = 0.f, q1 = 0.f;
          unsigned meta = 0u;
#pragma unroll
          for (int i = 0; i < kLmPer; ++i)
            if (i == at) { v = pv[i]; a = pa[i]; smv = psm[i]; meta = pmeta[i]; ns = nst[i]; q1 = lq[i]; }
          const bool word = w.slot > 0;
          sNode[nxt][q] = -1; sPar[nxt][q] = sNode[cur][w.r]; sE[nxt][q] = sTc[w.k]; sLab[nxt][q] = (v << 3) | w.slot;
          sU[nxt][q] = word ? 0 : v; sSu[nxt][q] = (word || v == 0) ? 0.f : smv;
          sSt[nxt][q] = word ? ns : sSt[cur][w.r]; sAcc[nxt][q] = word ? sAcc[cur][w.r] + q1 : sAcc[cur][w.r];
          sPb[nxt][q] = -INFINITY; sPnb[nxt][q] = w.tot; sTot[nxt][q] = w.tot;
          meta |= 1u << (4 + w.slot);
          u64 nk;
          beam_lex_best(lv, xv, v, a, smv, meta, sSt[cur][w.r], lmWeight, wordScore, w.r, w.k, &nk, &ns, &q1);
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
    if (tid < n && sNode[nxt][tid] == -1) sNode[nxt][tid] = beam_node(tab, capm, sPar[nxt][tid], sLab[nxt][tid]);   // a new hypothesis
    __syncthreads();
    cur = nxt;
  }
  beam_store_final(ws, b, n, sNode[cur], sTot[cur], sSt[cur], sAcc[cur], sU[cur]);
  if constexpr (kResume) beam_carry_store(cy, b, n, sPar[cur], sE[cur], sPb[cur], sPnb[cur], sLab[cur], sSu[cur]);
}

template <bool kLogAdd, int kThreads, class Pol = BeamCtc>
__global__ __launch_bounds__(kThreads) void ctc_beam_lex_scan(int T, int N, int W, float threshold, const float* __restrict__ x,
                                                              const int* __restrict__ frames, CtcBeamWs ws,
                                                              const void* __restrict__ lex, const void* __restrict__ lm,
                                                              float lmWeight, float wordScore, BeamTrans tr) {
  beam_lex_scan_body<kLogAdd, kThreads, Pol, false>(T, N, W, threshold, x, frames, ws, lex, lm, lmWeight, wordScore, tr, BeamCarry{});
}

// n: the final entries of utterance b; g: what bounds the walks up the prefix table (BeamWalk{}: nothing does)
__device__ __forceinline__ void beam_lex_finish_body(int b, int n, BeamWalk g, int M, int Lmax, int maxWords, const CtcBeamWs& ws,
                                                     const void* __restrict__ lex, const void* __restrict__ lm, float lmWeight,
                                                     float eosScore, int useEos, int* __restrict__ labels,
                                                     int* __restrict__ lengths, float* __restrict__ scores,
                                                     float* __restrict__ lmScores, int* __restrict__ words,
                                                     int* __restrict__ wordCounts) {
  __shared__ float sScore[64];
  const int r = threadIdx.x;
  const u64* tab = ws.table + (size_t)b * ws.cap;
  const LexView xv = lex_view(lex);
  const bool alive = r < n && ws.finU[b * kBeamMax + r] == 0;   // only finished words count at the end
  float score = -INFINITY, acc = -INFINITY;
  if (alive) {
    score = ws.finTot[b * kBeamMax + r];
    acc = ws.finAcc[b * kBeamMax + r];
    if (useEos)
      beam_eos(lm, ws.finState[b * kBeamMax + r], (int)((const NgramHeader*)lm)->numTokens + 1, lmWeight, eosScore, &score, &acc);
  }
  const int m = beam_rerank(score, alive, sScore);
  if (m >= M) return;
  int* lab = labels + ((size_t)b * M + m) * Lmax;
  int* wrd = words + ((size_t)b * M + m) * maxWords;
  int len = 0, nwords = 0;
  if (alive) {
    const int node = ws.finNode[b * kBeamMax + r];
    len = beam_chain_len(tab, node, &nwords, g);
    int i = len - 1, j = nwords - 1;
    for (int p = node; i >= 0 && beam_walk_ok(g, p); --i) {
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

__global__ __launch_bounds__(64) void ctc_beam_lex_finish(int M, int Lmax, int maxWords, CtcBeamWs ws, const void* __restrict__ lex,
                                                          const void* __restrict__ lm, float lmWeight, float eosScore, int useEos,
                                                          int* __restrict__ labels, int* __restrict__ lengths,
                                                          float* __restrict__ scores, float* __restrict__ lmScores,
                                                          int* __restrict__ words, int* __restrict__ wordCounts) {
  beam_lex_finish_body(blockIdx.x, ws.finN[blockIdx.x], BeamWalk{}, M, Lmax, maxWords, ws, lex, lm, lmWeight, eosScore, useEos, labels,
                       lengths, scores, lmScores, words, wordCounts);
}

}  // namespace w2l
