// criterion_beam_lextok.hpp -- w2l_ctc_beam_search_lextok and w2l_asg_beam_search_lextok: the beam searches restricted to the
// spellings of a lexicon and scored by a TOKEN-level back-off n-gram LM (contract: include/w2l_hip.h; the reference's
// --uselexicon=true --decodertype=tkn).  Included at the end of criterion_ctc.hip after criterion_beam_xl.hpp; the
// host side (checks, launches, entry points) is criterion_beam_entry.hpp's beam_narrow_run and criterion_beam_wide.hpp's beam_wide_run.  The lexicon search
// (criterion_ctc_beam_lex.hpp) owns the state -- prefix-table labels (lexicon node << 3) | slot, the sil / in / word slots, the
// root-only end -- and its finishes serve as they are: they rebuild tokens and words from labels and node records, and their
// end-of-sentence term reads word numTokens + 1 of whatever blob it is given.  What changes is where the LM enters: every token
// that moves along a trie edge adds lmWeight * q(s, c) and advances the LM state, a completed word adds wordScore alone, and the
// trie's smear values are never read.
//   beam_lextok_scan   one workgroup of 256 or 1024 threads per utterance, the pair-to-thread mapping of ctc_beam_lex_scan.  Pass 1
//                      issues, for every pair (r, k) that is not the silence loop at the root, the LM lookup q(s_r, c_k) AND the
//                      trie edge child(u_r, c_k) with the node's record, all in flight together.  The LM lookup is issued before
//                      the edge resolves, also for the pairs the lexicon then blocks: its chain (probe, back-off walk) is as long
//                      as the edge's (probe, node record), so waiting for the edge first would make the frame two round trips
//                      instead of one; a blocked pair's lookup costs bandwidth the frame does not lack and its value is dropped.
//                      A pair's up to seven candidates share one a = a0 + lmWeight * q: slot 0 is a, every word slot a + wordScore,
//                      so the best unconsumed candidate is a function of (a, meta) alone (beam_lextok_best) and selection rounds do
//                      no loads at all -- neither LM nor node record.
//   wide               beam_wide_scan<., ., true, true>: the kTok hooks of criterion_beam_wide.hpp.  There the LM lookup waits for
//                      the edge: 1024 threads walk up to 65536 pairs of a frame, so the scan is bound by the number of lookups
//                      and not by one pair's latency, and a lookup for every blocked pair made it slower than the word search
//                      (592 against 509 us per frame at N = 9998, K = 64, W = 1000, where most pairs are blocked).
// The xl family is not built: W2L_EUNSUPPORTED.
#pragma once

namespace w2l {

// a = a0 + (lmWeight * q), a0 the policy's acoustic sum (CTC: lp[c] + base); a completed word: a + wordScore; one fp32 operation
// each, in this order: beam_lextok_a of criterion_ctc_beam_lex.hpp

// the best candidate of a pair that is not in its consumed mask (meta = nw | hasChildren << 3 | consumed << 4): 0 when none is
// left.  The word candidates tie on the total and are ordered by slot: the first unconsumed one is their best.
__device__ __forceinline__ u64 beam_lextok_best(float a, unsigned meta, float wordScore, int r, int k) {
  const unsigned done = meta >> 4;
  u64 best = 0ull;
  if (((meta >> 3) & 1u) && !(done & 1u)) best = beam_key(a, r, 1, k, 0);
  const unsigned left = ~(done >> 1) & ((1u << (meta & 7u)) - 1u);
  if (left) {
    const u64 kk = beam_key(a + wordScore, r, 1, k, __ffs((int)left));
    best = kk > best ? kk : best;
  }
  return best;
}

template <bool kLogAdd, int kThreads, class Pol>
__global__ __launch_bounds__(kThreads) void beam_lextok_scan(int T, int N, int W, float threshold, const float* __restrict__ x,
                                                             const int* __restrict__ frames, CtcBeamWs ws,
                                                             const void* __restrict__ lex, const void* __restrict__ lm,
                                                             float lmWeight, float wordScore, BeamTrans tr) {
  constexpr int kWaves = kThreads / 64;
  // the beam of this frame and the next one: prefix-table node, parent's node, last token, the label of the last extension, lexicon
  // node, LM state, pb, pnb, tot, unweighted LM sum
  __shared__ int sNode[2][64], sPar[2][64], sE[2][64], sLab[2][64], sU[2][64], sSt[2][64];
  __shared__ float sPb[2][64], sPnb[2][64], sTot[2][64], sAcc[2][64];
  __shared__ u64 sGone[7][64];   // per slot and beam entry: frame tokens whose candidate merged into another entry
  __shared__ int sTc[64];
  __shared__ float sTl[64];
  __shared__ u64 sRed[2][kWaves];
  const int b = blockIdx.x, tid = threadIdx.x, K = ws.K;
  const int F = align_frames(frames, b, T);
  const float* xb = x + (size_t)b * T * N;
  u64* tab = ws.table + (size_t)b * ws.cap;
  const unsigned capm = ws.cap - 1;
  const size_t row0 = (size_t)b * T;
  const NgramView lv = ngram_view(lm);
  const LexView xv = lex_view(lex);
  const float* A = Pol::stage(tr, N);

  int cur = 0, n = 1;
  if (tid < 64) {
    sNode[0][tid] = tid == 0 ? 0 : -2; sPar[0][tid] = -1; sE[0][tid] = -1; sLab[0][tid] = -1; sU[0][tid] = 0;
    sPb[0][tid] = tid == 0 ? 0.f : -INFINITY; sPnb[0][tid] = -INFINITY; sTot[0][tid] = tid == 0 ? 0.f : -INFINITY;
    sSt[0][tid] = (int)((const NgramHeader*)lm)->start; sAcc[0][tid] = 0.f;
  }
  for (int t = 0; t < F && n > 0; ++t) {
    const size_t row = row0 + t;
    beam_load_frame(ws, row, sTc, sTl);
    for (int i = tid; i < 7 * 64; i += kThreads) (&sGone[0][0])[i] = 0ull;
    const float lpb = ws.lpb[row], lse = ws.lse[row];
    __syncthreads();
    const int nxt = cur ^ 1, total = n * K;

    // pass 1: every pair's LM lookup, lexicon edge and node record
    int pv[kLmPer];          // the lexicon node the token reaches; 0: the silence loop at the root; -1: no candidate
    float pa[kLmPer];        // a (the silence loop: the acoustic sum alone)
    unsigned pmeta[kLmPer];  // nw | hasChildren << 3 | consumed << 4
    int pns[kLmPer];         // the LM successor
    float pq[kLmPer];        // the LM log-probability
#pragma unroll
    for (int i = 0; i < kLmPer; ++i) {
      pv[i] = -1; pa[i] = -INFINITY; pmeta[i] = 0u; pns[i] = 0; pq[i] = 0.f;
      const int idx = tid + kThreads * i;
      if (idx < total) {
        const int r = idx / K, k = idx - r * K, c = sTc[k], u = sU[cur][r];
        const float a0 = Pol::ext(sTl[k], c, sE[cur][r], sPb[cur][r], sTot[cur][r], A, N);
        if (Pol::none(c, sE[cur][r])) {   // no candidates
        } else if (c == xv.silToken && u == 0) {
          pv[i] = 0; pa[i] = a0; pmeta[i] = 8u; pns[i] = sSt[cur][r];
        } else {
          pq[i] = ngram_q(lv, sSt[cur][r], c, &pns[i]);
          const int v = lex_child(xv, u, c);
          if (v > 0) {
            const LexNode& nd = lex_node(xv, v);
            pv[i] = v; pmeta[i] = (unsigned)lex_nw(nd) | (lex_has_children(nd) ? 8u : 0u);
            pa[i] = beam_lextok_a(a0, lmWeight, pq[i]);
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
        float v = s.a;
        if (vj != 0) {
          int unused;
          v = beam_lextok_a(v, lmWeight, ngram_q(lv, sSt[cur][s.pr], s.e, &unused));
          if (slot > 0) v = v + wordScore;
        }
        spnb = beam_oplus<kLogAdd>(spnb, v);
        atomicOr(&sGone[min(slot, 6)][s.pr], 1ull << s.kj);
      }
      stot = beam_oplus<kLogAdd>(spb, spnb);
      stayKey = beam_key(stot, tid, 0, 0);
    }
    __syncthreads();
    // pass 2: every pair's best candidate among those that did not merge; arithmetic only
    u64 key[kLmPer];
    u64 local = stayKey;
#pragma unroll
    for (int i = 0; i < kLmPer; ++i) {
      key[i] = 0ull;
      const int idx = tid + kThreads * i;
      if (idx < total && pv[i] >= 0) {
        const int r = idx / K, k = idx - r * K;
        unsigned done = 0u;
#pragma unroll
        for (int s = 0; s < 7; ++s) done |= (unsigned)((sGone[s][r] >> k) & 1ull) << s;
        pmeta[i] |= done << 4;
        key[i] = beam_lextok_best(pa[i], pmeta[i], wordScore, r, k);
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
          sU[nxt][q] = sU[cur][tid]; sSt[nxt][q] = sSt[cur][tid]; sAcc[nxt][q] = sAcc[cur][tid];
          sPb[nxt][q] = spb; sPnb[nxt][q] = spnb; sTot[nxt][q] = stot;
          stayKey = 0ull;
          mine = true;
        }
      } else {
        const int idx = w.r * K + w.k;
        if (tid == idx % kThreads) {
          const int at = idx / kThreads;
          int v = 0, ns = 0;
          float a = 0.f, q1 = 0.f;
          unsigned meta = 0u;
#pragma unroll
          for (int i = 0; i < kLmPer; ++i)
            if (i == at) { v = pv[i]; a = pa[i]; meta = pmeta[i]; ns = pns[i]; q1 = pq[i]; }
          sNode[nxt][q] = -1; sPar[nxt][q] = sNode[cur][w.r]; sE[nxt][q] = sTc[w.k]; sLab[nxt][q] = (v << 3) | w.slot;
          sU[nxt][q] = w.slot > 0 ? 0 : v;
          sSt[nxt][q] = ns; sAcc[nxt][q] = v == 0 ? sAcc[cur][w.r] : sAcc[cur][w.r] + q1;
          sPb[nxt][q] = -INFINITY; sPnb[nxt][q] = w.tot; sTot[nxt][q] = w.tot;
          meta |= 1u << (4 + w.slot);
          const u64 nk = beam_lextok_best(a, meta, wordScore, w.r, w.k);
#pragma unroll
          for (int i = 0; i < kLmPer; ++i)
            if (i == at) { pmeta[i] = meta; key[i] = nk; }
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
}

}  // namespace w2l
