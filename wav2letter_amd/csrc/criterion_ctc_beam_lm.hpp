// criterion_ctc_beam_lm.hpp -- w2l_ctc_beam_search_lm: the CTC prefix beam search fused with a token-level back-off n-gram LM
// (contract: include/w2l_hip.h; the LM table and its score rule: ngram_lm.hpp).  Included at the end of criterion_ctc.hip after
// criterion_ctc_beam.hpp, whose row kernel (ctc_beam_rows: frame tokens by the acoustic lp alone), trie, keys and (+) it reuses.
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
#include "ngram_lm.hpp"

namespace w2l {

constexpr int kLmPer = 4;   // extensions a thread owns: threads * kLmPer >= W * K

struct CtcBeamLmWs {
  CtcBeamWs b;
  int* finState;    // [B][64] LM state of the final entry of rank r
  float* finAcc;    // [B][64] sum of q over its labels, in label order
};

static size_t ctc_beam_lm_layout(CtcBeamLmWs* w, void* ws, int B, int T, int W, int K) {
  const size_t base = ctc_beam_layout(w ? &w->b : nullptr, ws, B, T, W, K);   // a multiple of 256
  const size_t fin = align_up((size_t)B * kBeamMax * 4, 256);
  if (w) {
    w->finState = (int*)((char*)ws + base);
    w->finAcc = (float*)((char*)ws + base + fin);
  }
  return base + 2 * fin;
}

// pnb' of an extension: (lp[c] + base) + g, g = (lmWeight * q) + classScore[c]; one fp32 operation each, in this order
__device__ __forceinline__ float beam_lm_ext(float lpc, float base, float lmWeight, float q, const float* __restrict__ classScore, int c) {
  float g = lmWeight * q;
  if (classScore) g = g + classScore[c];
  return (lpc + base) + g;
}

template <bool kLogAdd, int kThreads>
__global__ __launch_bounds__(kThreads) void ctc_beam_lm_scan(int T, int N, int W, float threshold,
                                                             const float* __restrict__ x, const int* __restrict__ frames,
                                                             CtcBeamLmWs wsl, const void* __restrict__ lm, float lmWeight,
                                                             const float* __restrict__ classScore) {
  typedef unsigned long long u64;
  constexpr int kWaves = kThreads / 64;
  __shared__ int sNode[2][64], sPar[2][64], sE[2][64], sSt[2][64];   // the beam of this frame and the next one
  __shared__ float sPb[2][64], sPnb[2][64], sTot[2][64], sAcc[2][64];
  __shared__ u64 sGone[64];   // per beam entry: frame tokens whose extension merged into another entry
  __shared__ int sTc[64];
  __shared__ float sTl[64];
  __shared__ u64 sRed[2][kWaves];
  const CtcBeamWs& ws = wsl.b;
  const int b = blockIdx.x, tid = threadIdx.x, K = ws.K;
  const int F = align_frames(frames, b, T);
  const float* xb = x + (size_t)b * T * N;
  u64* tab = ws.table + (size_t)b * ws.cap;
  const unsigned capm = ws.cap - 1;
  const size_t row0 = (size_t)b * T;
  const NgramView lv = ngram_view(lm);

  int cur = 0, n = 1;
  if (tid < 64) {
    sNode[0][tid] = tid == 0 ? 0 : -2; sPar[0][tid] = -1; sE[0][tid] = -1;
    sPb[0][tid] = tid == 0 ? 0.f : -INFINITY; sPnb[0][tid] = -INFINITY; sTot[0][tid] = tid == 0 ? 0.f : -INFINITY;
    sSt[0][tid] = (int)((const NgramHeader*)lm)->start; sAcc[0][tid] = 0.f;
  }
  for (int t = 0; t < F && n > 0; ++t) {
    const size_t row = row0 + t;
    if (tid < 64) {
      sTc[tid] = tid < K ? ws.tokC[row * K + tid] : -2;
      sTl[tid] = tid < K ? ws.tokLp[row * K + tid] : -INFINITY;
      sGone[tid] = 0;
    }
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
        lq[i] = ngram_q(lv, sSt[cur][r], c, &nst[i]);
        const float v = beam_lm_ext(sTl[k], c == sE[cur][r] ? sPb[cur][r] : sTot[cur][r], lmWeight, lq[i], classScore, c);
        key[i] = beam_key(v, r, 1, k);
      }
    }
    // stay(tid), with the extension that spells this entry merged in
    u64 stayKey = 0ull;
    float spb = -INFINITY, spnb = -INFINITY, stot = -INFINITY;
    if (tid < n) {
      const int e = sE[cur][tid], par = sPar[cur][tid];
      int kj = -1, pr = -1;
      for (int k = 0; k < K; ++k) kj = sTc[k] == e ? k : kj;
      for (int r = 0; r < n; ++r) pr = sNode[cur][r] == par ? r : pr;
      spb = lpb + sTot[cur][tid];
      if (e >= 0) spnb = (xb[(size_t)t * N + e] - lse) + sPnb[cur][tid];   // lp[e] comes from the row whether or not e is a frame token
      if (pr >= 0 && kj >= 0) {
        int unused;
        const float qm = ngram_q(lv, sSt[cur][pr], e, &unused);
        const float v = beam_lm_ext(sTl[kj], e == sE[cur][pr] ? sPb[cur][pr] : sTot[cur][pr], lmWeight, qm, classScore, e);
        spnb = beam_oplus<kLogAdd>(spnb, v);
        atomicOr(&sGone[pr], 1ull << kj);
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
      const int wr = (int)(tie >> 7), wext = (int)((tie >> 6) & 1u), wkk = (int)(tie & 63u);
      bool mine = false;
      if (!wext) {
        if (tid == wr) {
          sNode[nxt][q] = sNode[cur][tid]; sPar[nxt][q] = sPar[cur][tid]; sE[nxt][q] = sE[cur][tid];
          sSt[nxt][q] = sSt[cur][tid]; sAcc[nxt][q] = sAcc[cur][tid];
          sPb[nxt][q] = spb; sPnb[nxt][q] = spnb; sTot[nxt][q] = stot;
          stayKey = 0ull;
          mine = true;
        }
      } else {
        const int idx = wr * K + wkk;
        if (tid == idx % kThreads) {
          const int slot = idx / kThreads;
#pragma unroll
          for (int i = 0; i < kLmPer; ++i)
            if (i == slot) {
              sNode[nxt][q] = -1; sPar[nxt][q] = sNode[cur][wr]; sE[nxt][q] = sTc[wkk];
              sSt[nxt][q] = nst[i]; sAcc[nxt][q] = sAcc[cur][wr] + lq[i];
              sPb[nxt][q] = -INFINITY; sPnb[nxt][q] = wtot; sTot[nxt][q] = wtot;
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
    if (tid < n && sNode[nxt][tid] == -1) {   // a new prefix: find or make its trie node
      const u64 edge = ((u64)(unsigned)sPar[nxt][tid] << 32) | (u64)(unsigned)(sE[nxt][tid] + 1);
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
    wsl.finState[b * kBeamMax + tid] = live ? sSt[cur][tid] : 0;
    wsl.finAcc[b * kBeamMax + tid] = live ? sAcc[cur][tid] : -INFINITY;
    if (tid == 0) ws.finN[b] = n;
  }
}

__global__ __launch_bounds__(64) void ctc_beam_lm_finish(int M, int Lmax, int eosWord, CtcBeamLmWs wsl, const void* __restrict__ lm,
                                                         float lmWeight, float eosScore, int useEos, int* __restrict__ labels,
                                                         int* __restrict__ lengths, float* __restrict__ scores,
                                                         float* __restrict__ lmScores) {
  typedef unsigned long long u64;
  __shared__ float sScore[64];
  const CtcBeamWs& ws = wsl.b;
  const int b = blockIdx.x, r = threadIdx.x;
  const u64* tab = ws.table + (size_t)b * ws.cap;
  const int n = ws.finN[b];
  const bool live = r < n;
  float score = -INFINITY, acc = -INFINITY;
  if (live) {
    score = ws.finTot[b * kBeamMax + r];
    acc = wsl.finAcc[b * kBeamMax + r];
    if (useEos) {
      const NgramView lv = ngram_view(lm);
      int unused;
      const float qe = ngram_q(lv, wsl.finState[b * kBeamMax + r], eosWord, &unused);
      score = score + ((lmWeight * qe) + eosScore);
      acc = acc + qe;
    }
  }
  sScore[r] = score;
  __syncthreads();
  int m = r;   // rows n .. M-1 are the empty ones: the ranks of the live entries are a permutation of 0 .. n-1
  if (live) {
    m = 0;
    for (int o = 0; o < n; ++o) m += (sScore[o] > score || (sScore[o] == score && o < r)) ? 1 : 0;
  }
  if (m >= M) return;
  int* lab = labels + ((size_t)b * M + m) * Lmax;
  int len = 0;
  if (live) {
    const int node = ws.finNode[b * kBeamMax + r];
    for (int p = node; p > 0; p = (int)(tab[p - 1] >> 32)) ++len;
    int i = len - 1;
    for (int p = node; p > 0; --i) {
      const u64 edge = tab[p - 1];
      if (i < Lmax) lab[i] = (int)(unsigned)edge - 1;
      p = (int)(edge >> 32);
    }
  }
  for (int i = min(len, Lmax); i < Lmax; ++i) lab[i] = -1;
  lengths[(size_t)b * M + m] = live ? len : -1;
  scores[(size_t)b * M + m] = score;
  lmScores[(size_t)b * M + m] = acc;
}

}  // namespace w2l

W2L_API size_t w2l_ctc_beam_lm_workspace_size(int B, int T, int N, int beam, int beamToken) {
  if (B <= 0 || T <= 0 || N < 2 || beam <= 0 || beamToken <= 0) return 0;
  const int K = w2l::ctc_beam_clip(N, beamToken);
  if (beam > w2l::kBeamMax || K > w2l::kBeamMax) return 0;
  return w2l::ctc_beam_lm_layout(nullptr, nullptr, B, T, beam, K);
}

W2L_API int w2l_ctc_beam_search_lm(int B, int T, int N, const float* input, const int* frames, int beam, int beamToken,
                                   float threshold, int logAdd, int normalize, int nbest, int maxLen, const void* lm, int lmHasEos,
                                   float lmWeight, const float* classScore, float eosScore, int* labels, int* lengths,
                                   float* scores, float* lmScores, void* workspace, w2l_stream_t stream) {
  using namespace w2l;
  if (B <= 0 || T <= 0 || N < 2 || !input || !labels || !lengths || !scores || !lmScores || !workspace || !lm) return W2L_EINVAL;
  if (beam <= 0 || beamToken <= 0 || nbest <= 0 || nbest > beam || maxLen <= 0) return W2L_EINVAL;
  if (!(threshold >= 0.f)) return W2L_EINVAL;   // NaN or negative
  if (!(fabsf(lmWeight) < INFINITY) || !(fabsf(eosScore) < INFINITY)) return W2L_EINVAL;
  if (!lmHasEos && eosScore != 0.f) return W2L_EINVAL;
  const int K = ctc_beam_clip(N, beamToken);
  if (beam > kBeamMax || K > kBeamMax) return W2L_EUNSUPPORTED;
  if ((size_t)T * beam > ((size_t)1 << 29)) return W2L_EUNSUPPORTED;   // node ids are ints
  hipStream_t s = (hipStream_t)stream;
  CtcBeamLmWs ws{};
  ctc_beam_lm_layout(&ws, workspace, B, T, beam, K);
  W2L_HIP_CHECK(hipMemsetAsync(ws.b.table, 0, (size_t)B * ws.b.cap * sizeof(unsigned long long), s));
  const unsigned rows = (unsigned)((size_t)B * T);
  if (N <= kRowThreads * kRowMaxPer)
    hipLaunchKernelGGL(ctc_beam_rows<false>, dim3(rows), dim3(kRowThreads), 0, s, T, N, normalize, input, frames, ws.b);
  else
    hipLaunchKernelGGL(ctc_beam_rows<true>, dim3(rows), dim3(kRowThreads), 0, s, T, N, normalize, input, frames, ws.b);
  W2L_LAUNCH_CHECK();
  const bool wide = beam * K > 256 * kLmPer;
#define W2L_LM_SCAN(LA, TH)                                                                                                   \
  hipLaunchKernelGGL((ctc_beam_lm_scan<LA, TH>), dim3((unsigned)B), dim3(TH), 0, s, T, N, beam, threshold, input, frames, ws, lm, \
                     lmWeight, classScore)
  if (logAdd) { if (wide) W2L_LM_SCAN(true, 1024); else W2L_LM_SCAN(true, 256); }
  else { if (wide) W2L_LM_SCAN(false, 1024); else W2L_LM_SCAN(false, 256); }
#undef W2L_LM_SCAN
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_beam_lm_finish, dim3((unsigned)B), dim3(64), 0, s, nbest, maxLen, N, ws, lm, lmWeight, eosScore,
                     lmHasEos ? 1 : 0, labels, lengths, scores, lmScores);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
