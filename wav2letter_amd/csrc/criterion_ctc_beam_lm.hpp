// criterion_ctc_beam_lm.hpp -- w2l_ctc_beam_search_lm: the CTC prefix beam search fused with a token-level back-off n-gram LM
// (contract: include/w2l_hip.h; the LM table and its score rule: ngram_lm.hpp).  Included at the end of criterion_ctc.hip after
// criterion_ctc_beam.hpp, whose row kernel (ctc_beam_rows: frame tokens by the acoustic lp alone), workspace, prefix table, keys, (+)
// and entry-point plumbing it reuses, and which owns the parts of a workgroup scan and of a finish that this search shares with the
// lexicon search (frame load, front of a stay, selection round, final store; chain walk, end-of-sentence term, re-rank).  This file
// keeps what is particular to the token LM: the total of an extension (beam_lm_ext) and the bookkeeping of all n * K of them.
// The lattice is a policy (BeamCtc, the default; BeamAsg of criterion_asg_beam.hpp, which also runs this scan without an LM).
//   ctc_beam_lm_scan    one workgroup of 256 or 1024 threads per utterance.  The LM term depends on (prefix, token), so lp_k + tot
//                       + g is NOT monotone in k and the LM-free scan's lazy per-lane selection does not hold: every one of the
//                       n * K extension totals of a frame is made.  Extension (r, k) belongs to thread (r K + k) mod threads, at
//                       most kLmPer of them per thread, and stays in that thread's registers with its selection key, its LM
//                       successor state and its LM log-probability: the table lookups (chains of dependent 16-byte loads, latency
//                       bound) of a frame are all in flight together.  The beam itself (node, parent, last label, pb, pnb, tot,
//                       LM state, unweighted LM sum of the prefix) is double-buffered in LDS.  Thread j < n also owns stay(j): it
//                       finds the extension that spells its prefix (parent node, last label), recomputes that one total with the
//                       same operations, adds it to its pnb' and marks it gone.  Selection: each thread keeps the largest of its
//                       keys; a round is a block-wide 64-bit max (wave max, one LDS word per wave, ONE barrier: the words are
//                       double-buffered by round parity), the owner of the winner writes the entry of rank q and rescans its
//                       registers.  Rounds stop at W, at -inf and at the threshold line: keys come in descending order.
//   ctc_beam_lm_finish  one wavefront per utterance, lane r = surviving entry r: the end-of-sentence term, the re-ranking by
//                       (score descending, previous rank ascending) as a count over the other lanes, then labels, length, score
//                       and the unweighted LM score of the rows below M.
#pragma once

namespace w2l {

// pnb' of an extension: a + g, a the policy's acoustic sum (CTC: lp[c] + base), g = (lmWeight * q) + classScore[c]; one fp32
// operation each, in this order
__device__ __forceinline__ float beam_lm_ext(float a, float lmWeight, float q, const float* __restrict__ classScore, int c) {
  float g = lmWeight * q;
  if (classScore) g = g + classScore[c];
  return a + g;
}

// lm may be null, which means no LM: no g term, q = 0, state 0 (the ASG LM-free search, the LM-free session, and the LM-free CTC
// search with a silence score, whose biased tokLp the lazy scan of criterion_ctc_beam.hpp cannot take).
// kResume (criterion_beam_stream.hpp): utterance b is a slot of a beam session: its frame count (0: none) and start flag come from
// cy.cnt / cy.flag, the beam from the session's state unless the slot starts, and every array of the beam goes back there after
// the frames.  ctc_beam_lm_scan below is the body with kResume off: the whole search.
template <bool kLogAdd, int kThreads, class Pol, bool kResume>
__device__ __forceinline__ void beam_lm_scan_body(int T, int N, int W, float threshold, const float* __restrict__ x,
                                                  const int* __restrict__ frames, const CtcBeamWs& ws, const void* __restrict__ lm,
                                                  float lmWeight, const float* __restrict__ classScore, BeamTrans tr,
                                                  const BeamCarry& cy) {
  constexpr int kWaves = kThreads / 64;
  __shared__ int sNode[2][64], sPar[2][64], sE[2][64], sSt[2][64];   // the beam of this frame and the next one
  __shared__ float sPb[2][64], sPnb[2][64], sTot[2][64], sAcc[2][64];
  __shared__ u64 sGone[64];   // per beam entry: frame tokens whose extension merged into another entry
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
  const bool useLm = lm != nullptr;
  const NgramView lv = useLm ? ngram_view(lm) : NgramView{};
  const float* A = Pol::stage(tr, N);

  int cur = 0, n = 1;
  if (!fresh) {
    n = beam_carry_load(cy, ws, b, N, sNode[0], sPar[0], sE[0], sPb[0], sPnb[0], sTot[0], sSt[0], sAcc[0], nullptr, nullptr, nullptr);
  } else if (tid < 64) {
    sNode[0][tid] = tid == 0 ? 0 : -2; sPar[0][tid] = -1; sE[0][tid] = -1;
    sPb[0][tid] = tid == 0 ? 0.f : -INFINITY; sPnb[0][tid] = -INFINITY; sTot[0][tid] = tid == 0 ? 0.f : -INFINITY;
    sSt[0][tid] = useLm ? (int)((const NgramHeader*)lm)->start : 0; sAcc[0][tid] = 0.f;
  }
  if constexpr (kResume) __syncthreads();   // F may be 0: the store below reads what other threads wrote
  for (int t = 0; t < F && n > 0; ++t) {
    const size_t row = row0 + t;
    beam_load_frame(ws, row, sTc, sTl);
    if (tid < 64) sGone[tid] = 0;
    const float lpb = ws.lpb[row], lse = ws.lse[row];
    __syncthreads();
    const int nxt = cur ^ 1, total = n * K;

    // every extension of the frame: total, key, LM successor, LM log-probability
    u64 key[kLmPer];
    int nst[kLmPer];
    float lq[kLmPer];
#pragma unroll
    for (int i = 0; i < kLmPer; ++i) {
      key[i] = 0ull; nst[i] = 0; lq[i] = 0.f;
      const int idx = tid + kThreads * i;
      if (idx < total) {
        const int r = idx / K, k = idx - r * K, c = sTc[k];
        if (!Pol::none(c, sE[cur][r])) {
          float v = Pol::ext(sTl[k], c, sE[cur][r], sPb[cur][r], sTot[cur][r], A, N);
          if (useLm) {
            lq[i] = ngram_q(lv, sSt[cur][r], c, &nst[i]);
            v = beam_lm_ext(v, lmWeight, lq[i], classScore, c);
          }
          key[i] = beam_key(v, r, 1, k);
        }
      }
    }
    // stay(tid), with the extension that spells this entry merged in
    u64 stayKey = 0ull;
    float spb = -INFINITY, spnb = -INFINITY, stot = -INFINITY;
    if (tid < n) {
      const BeamStay s = beam_stay_front<Pol>(n, K, sTc, sTl, sNode[cur], sPar[cur], sE[cur], sPb[cur], sPnb[cur], sTot[cur],
                                              xb + (size_t)t * N, lpb, lse, A, N, ws.sil, ws.silScore);
      spb = s.spb; spnb = s.spnb;
      if (s.merge) {
        float v = s.a;
        if (useLm) {
          int unused;
          const float qm = ngram_q(lv, sSt[cur][s.pr], s.e, &unused);
          v = beam_lm_ext(v, lmWeight, qm, classScore, s.e);
        }
        spnb = beam_oplus<kLogAdd>(spnb, v);
        atomicOr(&sGone[s.pr], 1ull << s.kj);
      }
      stot = beam_oplus<kLogAdd>(spb, spnb);
      stayKey = beam_key(stot, tid, 0, 0);
    }
    __syncthreads();
    u64 local = stayKey;
#pragma unroll
    for (int i = 0; i < kLmPer; ++i) {
      const int idx = tid + kThreads * i;
      if (idx < total) {
        const int r = idx / K, k = idx - r * K;
        if ((sGone[r] >> k) & 1ull) key[i] = 0ull;
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
          sNode[nxt][q] = sNode[cur][tid]; sPar[nxt][q] = sPar[cur][tid]; sE[nxt][q] = sE[cur][tid];
          sSt[nxt][q] = sSt[cur][tid]; sAcc[nxt][q] = sAcc[cur][tid];
          sPb[nxt][q] = spb; sPnb[nxt][q] = spnb; sTot[nxt][q] = stot;
          stayKey = 0ull;
          mine = true;
        }
      } else {
        const int idx = w.r * K + w.k;
        if (tid == idx % kThreads) {
          const int slot = idx / kThreads;
#pragma unroll
          for (int i = 0; i < kLmPer; ++i)
            if (i == slot) {
              sNode[nxt][q] = -1; sPar[nxt][q] = sNode[cur][w.r]; sE[nxt][q] = sTc[w.k];
              sSt[nxt][q] = nst[i]; sAcc[nxt][q] = sAcc[cur][w.r] + lq[i];
              sPb[nxt][q] = -INFINITY; sPnb[nxt][q] = w.tot; sTot[nxt][q] = w.tot;
              key[i] = 0ull;
            }
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
    if (tid < n && sNode[nxt][tid] == -1) sNode[nxt][tid] = beam_node(tab, capm, sPar[nxt][tid], sE[nxt][tid]);   // a new prefix
    __syncthreads();
    cur = nxt;
  }
  beam_store_final(ws, b, n, sNode[cur], sTot[cur], sSt[cur], sAcc[cur], nullptr);
  if constexpr (kResume) beam_carry_store(cy, b, n, sPar[cur], sE[cur], sPb[cur], sPnb[cur], nullptr, nullptr);
}

template <bool kLogAdd, int kThreads, class Pol = BeamCtc>
__global__ __launch_bounds__(kThreads) void ctc_beam_lm_scan(int T, int N, int W, float threshold,
                                                             const float* __restrict__ x, const int* __restrict__ frames,
                                                             CtcBeamWs ws, const void* __restrict__ lm, float lmWeight,
                                                             const float* __restrict__ classScore, BeamTrans tr) {
  beam_lm_scan_body<kLogAdd, kThreads, Pol, false>(T, N, W, threshold, x, frames, ws, lm, lmWeight, classScore, tr, BeamCarry{});
}

// n: the final entries of utterance b; g: what bounds the walks up the prefix table (BeamWalk{}: nothing does)
__device__ __forceinline__ void beam_lm_finish_body(int b, int n, BeamWalk g, int M, int Lmax, int eosWord, const CtcBeamWs& ws,
                                                    const void* __restrict__ lm, float lmWeight, float eosScore, int useEos,
                                                    int* __restrict__ labels, int* __restrict__ lengths,
                                                    float* __restrict__ scores, float* __restrict__ lmScores) {
  __shared__ float sScore[64];
  const int r = threadIdx.x;
  const u64* tab = ws.table + (size_t)b * ws.cap;
  const bool live = r < n;
  float score = -INFINITY, acc = -INFINITY;
  if (live) {
    score = ws.finTot[b * kBeamMax + r];
    acc = ws.finAcc[b * kBeamMax + r];
    if (useEos) beam_eos(lm, ws.finState[b * kBeamMax + r], eosWord, lmWeight, eosScore, &score, &acc);
  }
  const int m = beam_rerank(score, live, sScore);   // rows n .. M-1 are the empty ones
  if (m >= M) return;
  const int len = beam_write_labels(tab, live, ws.finNode + b * kBeamMax + r, Lmax, labels + ((size_t)b * M + m) * Lmax, g);
  lengths[(size_t)b * M + m] = live ? len : -1;
  scores[(size_t)b * M + m] = score;
  if (lmScores) lmScores[(size_t)b * M + m] = acc;   // null: the LM-free CTC search, which has no such output
}

__global__ __launch_bounds__(64) void ctc_beam_lm_finish(int M, int Lmax, int eosWord, CtcBeamWs ws, const void* __restrict__ lm,
                                                         float lmWeight, float eosScore, int useEos, int* __restrict__ labels,
                                                         int* __restrict__ lengths, float* __restrict__ scores,
                                                         float* __restrict__ lmScores) {
  beam_lm_finish_body(blockIdx.x, ws.finN[blockIdx.x], BeamWalk{}, M, Lmax, eosWord, ws, lm, lmWeight, eosScore, useEos, labels,
                      lengths, scores, lmScores);
}

}  // namespace w2l
