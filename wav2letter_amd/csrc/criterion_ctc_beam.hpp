// criterion_ctc_beam.hpp -- w2l_ctc_beam_search: LM-free CTC prefix beam search with n-best output (contract: include/w2l_hip.h).
// Included at the end of criterion_ctc.hip (one translation unit: the row loader, the block reductions and align_frames are that
// file's and criterion_ctc_align.hpp's).
//   ctc_beam_rows    one workgroup per emission row (rows at or beyond frames[b] return at once): lse (normalize only), lp[blank]
//                    and the K best non-blank (class, lp) pairs in the contract's order, written compactly.  The row is read once
//                    into registers (ctc_rows_lse's loader).  An element's 64-bit key is (lp as an order-preserving integer, ~class),
//                    so keys are unique and "lp descending, class ascending" is one integer compare.  Selection: the K-th largest of
//                    the 256 per-thread maxima is a lower bound of the K-th largest key; the elements at or above it (about K of them
//                    whatever the ties; more only when few threads own all large values) go to LDS and are ranked there.  More than
//                    kBeamCandCap of them: K rounds of block-wide arg-max extraction instead.  N > 256 * kRowMaxPer: the same
//                    algorithm re-reading the row from memory.
//   ctc_beam_scan    one wavefront per utterance, lane r = beam entry of rank r.  Prefixes are nodes of a trie kept as an open-
//                    addressing hash table (key = parent node, label; node id = slot + 1; root = 0) in the workspace, so one prefix
//                    has one node whatever its history and the merge test is an integer compare of (parent node, label).  A lane's
//                    extensions are never materialised: lp_k + tot is non-increasing in k, so a lane's best candidate is the best of
//                    its stay, its own-label extension (the one that adds pb instead of tot) and the first unconsumed regular
//                    extension; a selection round is a 64-bit wave max of (total, ~(rank, kind, k)) and an O(1) update of the winner.
//                    Extensions merged into a beam entry are bits of a per-lane mask.  No waiting between workgroups, no flags.
//   ctc_beam_finish  one thread per (utterance, output rank): walks the parent chain, writes labels, length, score.
// This file also owns what the three searches share, so that a rule of the contract is written once: the workspace (CtcBeamWs,
// ctc_beam_layout), the tie key, its decoder and the stops of a selection (beam_key, beam_pick), the prefix table's find-or-make
// (beam_node); for the workgroup scans of criterion_ctc_beam_lm.hpp and criterion_ctc_beam_lex.hpp beam_load_frame, beam_stay_front,
// beam_select_round and beam_store_final; for the finishes beam_chain_len, beam_write_labels, beam_eos and beam_rerank; for the
// host side (criterion_beam_entry.hpp and the wide and xl runs) BeamReq with beam_sil_check, beam_req_check, beam_common_check and
// beam_rows_launch, and ctc_beam_fused_scan; for the beam session of criterion_beam_stream.hpp, which
// resumes the two workgroup scans from a stored beam, BeamCarry with beam_carry_begin / _load / _store and the bound of a walk up
// the prefix table (BeamWalk).  The other two files keep what is particular to their search.
// What the lattice is -- the acoustic sum of a stay and of an extension -- is a policy of the two workgroup scans: BeamCtc here,
// BeamAsg in criterion_asg_beam.hpp (no blank, a transition matrix, no token after itself), which also uses ctc_beam_rows<., true>.
// The LM-free search itself uses neither the LM table (ngram_lm.hpp is here for beam_eos) nor kLmPer (the workgroup scans').
#pragma once
#include "ngram_lm.hpp"

namespace w2l {

typedef unsigned long long u64;

constexpr int kBeamMax = 64;          // W and K: one lane per entry, one mask bit per frame token
constexpr int kBeamWideMax = 1024;    // W of the wide searches (criterion_beam_wide.hpp); their K stays <= kBeamMax
constexpr int kBeamCandCap = 1024;    // LDS candidates of the row pass
constexpr int kLmPer = 4;             // (entry, token) pairs a thread of a workgroup scan owns: threads * kLmPer >= W * K

struct BeamSil { int token = -1; float score = 0.f; };   // a search's silence class and score; the default: none

enum CtcBeamVariant { kBeamPlain = 0, kBeamLm = 1, kBeamLex = 2 };   // each one's workspace is the one before plus its own buffers

struct CtcBeamWs {
  float* lse;                  // [B][T]  0 when not normalising
  float* lpb;                  // [B][T]  lp[blank]
  float* tokLp;                // [B][T][K]
  int* tokC;                   // [B][T][K]
  u64* table;   // [B][cap] trie edges: (parent node << 32) | (label + 1), 0 = free
  int* finNode;                // [B][64] node of the final entry of rank r
  float* finTot;               // [B][64]
  int* finN;                   // [B]
  int* finState;               // [B][64] LM state of the final entry of rank r                (null: kBeamPlain)
  float* finAcc;               // [B][64] sum of q over its labels, in label order             (null: kBeamPlain)
  int* finU;                   // [B][64] lexicon node of the final entry of rank r            (null: but for kBeamLex)
  int K;
  unsigned cap;
  int sil = -1;                // the silence class (BeamReq::sil, the *_sil entry points'); -1: none
  float silScore = 0.f;        // added to lp[sil] after the frame tokens are chosen: beam_sil_lp
};

// The silence score of the contract: lp[c] of class c as every later use reads it.  One fp32 add, and none when c is not the silence
// class (sil = -1 matches no class: the searches without a silence score execute no + 0).
__device__ __forceinline__ float beam_sil_lp(float lp, int c, int sil, float silScore) { return c == sil ? lp + silScore : lp; }

static size_t ctc_beam_cap(int T, int W) {
  const size_t need = 2 * (size_t)T * W;   // at most T * W nodes are ever made: load factor <= 1/2
  size_t c = 64;
  while (c < need) c <<= 1;
  return c;
}

static size_t ctc_beam_layout(CtcBeamWs* w, void* ws, int B, int T, int W, int K, int variant) {
  const size_t rows = (size_t)B * T, cap = ctc_beam_cap(T, W);
  char* p = (char*)ws;
  char* const p0 = p;
  float* lse = (float*)p; p += align_up(rows * sizeof(float), 256);
  float* lpb = (float*)p; p += align_up(rows * sizeof(float), 256);
  float* tokLp = (float*)p; p += align_up(rows * K * sizeof(float), 256);
  int* tokC = (int*)p; p += align_up(rows * K * sizeof(int), 256);
  u64* table = (u64*)p; p += align_up((size_t)B * cap * sizeof(u64), 256);
  int* finNode = (int*)p; p += align_up((size_t)B * kBeamMax * sizeof(int), 256);
  float* finTot = (float*)p; p += align_up((size_t)B * kBeamMax * sizeof(float), 256);
  int* finN = (int*)p; p += align_up((size_t)B * sizeof(int), 256);
  const size_t fin = align_up((size_t)B * kBeamMax * 4, 256);
  int* finState = nullptr; float* finAcc = nullptr; int* finU = nullptr;
  if (variant >= kBeamLm) { finState = (int*)p; p += fin; finAcc = (float*)p; p += fin; }
  if (variant >= kBeamLex) { finU = (int*)p; p += fin; }
  if (w) *w = CtcBeamWs{lse, lpb, tokLp, tokC, table, finNode, finTot, finN, finState, finAcc, finU, K, (unsigned)cap};
  return (size_t)(p - p0);
}

// fp32 -> unsigned, order-preserving; -0 and +0 map to one value (they compare equal)
__device__ __forceinline__ unsigned beam_ord(float f) {
  const unsigned u = __float_as_uint(f + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float beam_unord(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  // every lane holds the maximum: say so to the compiler (scalar compares and branches downstream)
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 block_max_u64(u64 v, u64* sm) {
  v = wave_max_u64(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 r = sm[0];
#pragma unroll
  for (int k = 1; k < kRowThreads / 64; ++k) r = sm[k] > r ? sm[k] : r;
  __syncthreads();
  return r;
}

// kNoBlank (the ASG searches of criterion_asg_beam.hpp): every class is a token, K may reach N, lpb is -inf
// kCounts (the beam session of criterion_beam_stream.hpp): frames[b] is a count as it stands, and 0 means no rows; frames[B + b]
// is the utterance's frame index of the slot's first row.  The order in which a row's exponentials are summed follows from where
// the row begins modulo 16 bytes (row_split), so lse is a function of the row's values AND that phase.  A session's rows lie
// wherever the chunking put them; they are split as the whole search splits frame t of an utterance that begins at a 16-byte
// boundary, phase (t N) mod 4, and loaded without an alignment promise: lse has the whole search's bits under any chunking.
template <bool kBig, bool kNoBlank = false, bool kCounts = false>
__global__ __launch_bounds__(kRowThreads) void ctc_beam_rows(int T, int N, int normalize,
                                                             const float* __restrict__ x,
                                                             const int* __restrict__ frames, CtcBeamWs ws) {
  __shared__ float sm[8];
  __shared__ u64 sKey[kRowThreads];
  __shared__ u64 sCand[kBeamCandCap];
  __shared__ u64 sRed[kRowThreads / 64];
  __shared__ u64 sTau;
  __shared__ unsigned sCnt;
  const size_t r = blockIdx.x;  // row = b*T + t
  const int b = (int)(r / T);
  if ((int)(r - (size_t)b * T) >= (kCounts ? min(frames[b], T) : align_frames(frames, b, T))) return;
  const float* row = x + r * N;
  const int tid = threadIdx.x, K = ws.K, blank = kNoBlank ? -1 : N - 1;
  int phase = 0;
  if constexpr (kCounts) phase = (int)(((size_t)(frames[gridDim.x / T + b] + (int)(r - (size_t)b * T)) * (size_t)N) & 3);

  // the row in registers, every load issued before the first use (ctc_rows_lse_body's loader)
  constexpr int kPer = kBig ? 1 : kRowMaxPer / 4;
  float4 v[kPer];
  float hv = 0.f;
  int hidx = -1;
  RowSplit sp{};
  if constexpr (!kBig) {
    sp = kCounts ? row_split_at(phase, N) : row_split(row, N);
    const float4* body = (const float4*)(row + sp.nh);
    if (sp.nbody4 > 0) {
      const int lastc = sp.nbody4 - 1;
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        if constexpr (kCounts) __builtin_memcpy(&v[k], row + sp.nh + 4 * min(tid + kRowThreads * k, lastc), sizeof(float4));
        else v[k] = body[min(tid + kRowThreads * k, lastc)];
      }
    }
    if (tid < sp.nh) hidx = tid;
    else if (tid >= 64 && tid - 64 < sp.ntail) hidx = sp.nh + 4 * sp.nbody4 + (tid - 64);
    if (hidx >= 0) hv = row[hidx];
  }
  auto each = [&](auto&& f) {   // f(value, class) for every element this thread owns
    if constexpr (kBig) {
      for (int n = tid; n < N; n += kRowThreads) f(row[n], n);
    } else {
#pragma unroll
      for (int k = 0; k < kPer; ++k)
        if (tid + kRowThreads * k < sp.nbody4) {
          const int i0 = sp.nh + 4 * (tid + kRowThreads * k);
          f(v[k].x, i0); f(v[k].y, i0 + 1); f(v[k].z, i0 + 2); f(v[k].w, i0 + 3);
        }
      if (hidx >= 0) f(hv, hidx);
    }
  };

  float lse = 0.f;
  if (normalize) {
    float m = -INFINITY;
    each([&](float a, int) { m = fmaxf(m, a); });
    m = block_reduce_max(m, sm);
    float s = 0.f;
    each([&](float a, int) { s += __expf(a - m); });
    s = block_reduce_sum(s, sm);
    lse = m + __logf(s);
  }
  auto key = [&](float a, int i) -> u64 {   // larger = earlier in the contract's order; blank is no token
    return i == blank ? 0ull : ((u64)beam_ord(a - lse) << 32) | (u64)(0xffffffffu - (unsigned)i);
  };

  u64 tm = 0;
  each([&](float a, int i) { const u64 k = key(a, i); tm = k > tm ? k : tm; });
  sKey[tid] = tm;
  if (tid == 0) {
    sTau = 1;   // fewer than K threads own a token: every token is a candidate
    sCnt = 0;
    ws.lse[r] = lse;
    ws.lpb[r] = kNoBlank ? -INFINITY : row[max(blank, 0)] - lse;
  }
  __syncthreads();
  int rank = 0;
  for (int j = 0; j < kRowThreads; ++j) rank += sKey[j] > tm ? 1 : 0;
  if (tm != 0 && rank == K - 1) sTau = tm;   // keys are unique: one writer
  __syncthreads();
  const u64 tau = sTau;
  each([&](float a, int i) {
    const u64 k = key(a, i);
    if (k >= tau) {
      const unsigned pos = atomicAdd(&sCnt, 1u);
      if (pos < (unsigned)kBeamCandCap) sCand[pos] = k;
    }
  });
  __syncthreads();
  const int cnt = (int)sCnt;   // >= K: the K thread maxima at or above tau are among them
  float* oLp = ws.tokLp + r * K;
  int* oC = ws.tokC + r * K;
  if (cnt <= kBeamCandCap) {
    for (int i = tid; i < cnt; i += kRowThreads) {
      const u64 ki = sCand[i];
      int rk = 0;
      for (int j = 0; j < cnt; ++j) rk += sCand[j] > ki ? 1 : 0;
      if (rk < K) {   // the list is in acoustic order; the silence score comes after selection and ranking
        const int c = (int)(0xffffffffu - (unsigned)ki);
        oLp[rk] = beam_sil_lp(beam_unord((unsigned)(ki >> 32)), c, ws.sil, ws.silScore);
        oC[rk] = c;
      }
    }
  } else {   // the large values sit with few threads: K rounds of block-wide extraction
    u64 last = ~0ull;
    for (int q = 0; q < K; ++q) {
      u64 lm = 0;
      each([&](float a, int i) { const u64 k = key(a, i); lm = (k < last && k > lm) ? k : lm; });
      const u64 w = block_max_u64(lm, sRed);
      if (tid == 0) {
        const int c = (int)(0xffffffffu - (unsigned)w);
        oLp[q] = beam_sil_lp(beam_unord((unsigned)(w >> 32)), c, ws.sil, ws.silScore);
        oC[q] = c;
      }
      last = w;
    }
  }
}

template <bool kLogAdd>
__device__ __forceinline__ float beam_oplus(float a, float b) {
  const float m = fmaxf(a, b);
  if constexpr (!kLogAdd) return m;
  return m == -INFINITY ? m : m + log1pf(expf(fminf(a, b) - m));
}

// The selection key of a candidate, larger = earlier: total descending, rank r ascending, stay before extension, k ascending, slot
// ascending (the lexicon search's 3 bits; 0 elsewhere, and then the order is total, r, stay first, k: what a word without slot
// bits would encode).  0 is no candidate.
__device__ __forceinline__ u64 beam_key(float total, int r, int ext, int k, int slot = 0) {
  return ((u64)beam_ord(total) << 32) |
         (u64)(0xffffffffu - (unsigned)((r << 10) | (ext << 9) | (k << 3) | slot));
}

struct BeamWin { u64 key; float tot; int r, ext, k, slot; };   // a round's winner

// The winner of round q from the largest key of the round, or false: no candidate left, -inf, or below the threshold line under
// the frame's best total (round 0's).  Candidates come in descending order: the rest fails too.  One condition, no early return:
// the scans' round loops branch once on it; when it is false *w and *best mean nothing (wk = 0 decodes to a NaN total), and every
// caller ends the frame's rounds.
__device__ __forceinline__ bool beam_pick(u64 wk, int q, float threshold, float* best, BeamWin* w) {
  const float wtot = beam_unord((unsigned)(wk >> 32));
  if (q == 0) *best = wtot;
  const unsigned tie = 0xffffffffu - (unsigned)wk;
  w->key = wk; w->tot = wtot;
  w->r = (int)(tie >> 10); w->ext = (int)((tie >> 9) & 1u); w->k = (int)((tie >> 3) & 63u); w->slot = (int)(tie & 7u);
  return wk != 0ull && wtot != -INFINITY && !(wtot < *best - threshold);
}

__device__ __forceinline__ unsigned beam_hash(u64 z) {   // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (unsigned)(z ^ (z >> 31));
}

// Find or make the node of the prefix table for (parent node, label): node id = slot + 1.  At most T * W nodes are ever made and
// the table has twice as many slots, so a free slot ends the chain long before the bound; a damaged table cannot spin a wavefront.
__device__ __forceinline__ int beam_node(u64* tab, unsigned capm, int par, int label) {
  const u64 edge = ((u64)(unsigned)par << 32) | (u64)(unsigned)(label + 1);
  unsigned h = beam_hash(edge) & capm;
  for (unsigned probe = 0; probe <= capm; ++probe) {
    const u64 old = atomicCAS(&tab[h], 0ull, edge);
    if (old == 0ull || old == edge) break;
    h = (h + 1) & capm;
  }
  return (int)h + 1;
}

template <bool kLogAdd>
__global__ __launch_bounds__(64) void ctc_beam_scan(int T, int N, int W, float threshold,
                                                    const float* __restrict__ x,
                                                    const int* __restrict__ frames, CtcBeamWs ws) {
  __shared__ u64 sGone[64];   // per beam entry: frame tokens whose extension merged into another entry
  __shared__ int sTc[64];
  __shared__ float sTl[64];
  __shared__ int sNode[64], sPar[64], sE[64];   // the next beam, written by the winners in rank order
  __shared__ float sPb[64], sPnb[64];
  const int b = blockIdx.x, lane = threadIdx.x, K = ws.K;
  const int F = align_frames(frames, b, T);
  const float* xb = x + (size_t)b * T * N;
  u64* tab = ws.table + (size_t)b * ws.cap;
  const unsigned capm = ws.cap - 1;
  const u64 maskK = K >= 64 ? ~0ull : ((1ull << K) - 1);
  const size_t row0 = (size_t)b * T;

  // entry of rank `lane`: its node, its parent's node, its last label (-1: the empty prefix), pb, pnb
  int n = 1;
  int node = lane == 0 ? 0 : -2, par = -1, e = -1;
  float pb = lane == 0 ? 0.f : -INFINITY, pnb = -INFINITY;

  int tcN = lane < K ? ws.tokC[row0 * K + lane] : -2;
  float tlN = lane < K ? ws.tokLp[row0 * K + lane] : -INFINITY;
  float lpbN = ws.lpb[row0], lseN = ws.lse[row0];
  for (int t = 0; t < F && n > 0; ++t) {
    const int tc = tcN;
    const float tl = tlN, lpb = lpbN, lse = lseN;
    const float xg = xb[(size_t)t * N + max(e, 0)];   // lp[e] comes from the row whether or not e is a frame token
    {
      const size_t rn = row0 + min(t + 1, F - 1);
      tcN = lane < K ? ws.tokC[rn * K + lane] : -2;
      tlN = lane < K ? ws.tokLp[rn * K + lane] : -INFINITY;
      lpbN = ws.lpb[rn];
      lseN = ws.lse[rn];
    }
    sTc[lane] = tc;
    sTl[lane] = tl;
    sGone[lane] = 0;
    const bool active = lane < n;
    int kj = -1;   // the frame token equal to this entry's last label
    for (int k = 0; k < K; ++k) kj = __builtin_amdgcn_readlane(tc, k) == e ? k : kj;
    int pr = -1;   // the rank of this entry's parent prefix, if it is in the beam
    for (int r = 0; r < n; ++r) pr = __builtin_amdgcn_readlane(node, r) == par ? r : pr;

    const float tot = beam_oplus<kLogAdd>(pb, pnb);
    const float spb = lpb + tot;
    float spnb = e >= 0 ? (xg - lse) + pnb : -INFINITY;
    const int prc = max(pr, 0), kjc = max(kj, 0);
    const int e_p = __shfl(e, prc);
    const float pb_p = __shfl(pb, prc), tot_p = __shfl(tot, prc);
    const float lpk = __shfl(tl, kjc);
    __syncthreads();
    if (active && pr >= 0 && kj >= 0) {   // ext(pr, kj) spells this entry: its pnb' joins this stay, the extension disappears
      atomicOr(&sGone[pr], 1ull << kj);
      spnb = beam_oplus<kLogAdd>(spnb, lpk + (e == e_p ? pb_p : tot_p));
    }
    __syncthreads();
    const float stot = beam_oplus<kLogAdd>(spb, spnb);
    u64 avail = active ? (maskK & ~sGone[lane]) : 0ull;   // the regular extensions not yet taken, in k order
    u64 stayKey = active ? beam_key(stot, lane, 0, 0) : 0ull;
    u64 specKey = 0ull;   // the extension by the entry's own last label adds pb, not tot: out of the monotone sequence
    if (kj >= 0 && ((avail >> kj) & 1ull)) {
      specKey = beam_key(lpk + pb, lane, 1, kj);
      avail &= ~(1ull << kj);
    }

    int q = 0;
    float best = 0.f;
    while (q < W) {
      const int kn = avail ? __ffsll((long long)avail) - 1 : -1;
      const u64 regKey = kn >= 0 ? beam_key(sTl[max(kn, 0)] + tot, lane, 1, kn) : 0ull;
      u64 lk = stayKey > specKey ? stayKey : specKey;
      lk = regKey > lk ? regKey : lk;
      BeamWin w;
      if (!beam_pick(wave_max_u64(lk), q, threshold, &best, &w)) break;
      if (lane == w.r) {
        if (!w.ext) {
          sNode[q] = node; sPar[q] = par; sE[q] = e; sPb[q] = spb; sPnb[q] = spnb;
          stayKey = 0ull;
        } else {
          sNode[q] = -1; sPar[q] = node; sE[q] = sTc[w.k]; sPb[q] = -INFINITY; sPnb[q] = w.tot;
          if (specKey == w.key) specKey = 0ull;
          else avail &= avail - 1;
        }
      }
      ++q;
    }
    __syncthreads();
    n = __builtin_amdgcn_readfirstlane(q);
    if (lane < n) {
      node = sNode[lane]; par = sPar[lane]; e = sE[lane]; pb = sPb[lane]; pnb = sPnb[lane];
      if (node == -1) node = beam_node(tab, capm, par, e);   // a new prefix
    } else {
      node = -2; par = -1; e = -1; pb = -INFINITY; pnb = -INFINITY;
    }
    __syncthreads();
  }
  ws.finNode[b * kBeamMax + lane] = lane < n ? node : -1;
  ws.finTot[b * kBeamMax + lane] = beam_oplus<kLogAdd>(pb, pnb);
  if (lane == 0) ws.finN[b] = n;
}

// ---- the two workgroup scans (ctc_beam_lm_scan, ctc_beam_lex_scan): one workgroup per utterance, the beam double-buffered in LDS

// the frame tokens of `row`, by the first wavefront; the caller's barrier publishes them
__device__ __forceinline__ void beam_load_frame(const CtcBeamWs& ws, size_t row, int* sTc, float* sTl) {
  const int tid = threadIdx.x, K = ws.K;
  if (tid < 64) {
    sTc[tid] = tid < K ? ws.tokC[row * K + tid] : -2;
    sTl[tid] = tid < K ? ws.tokLp[row * K + tid] : -INFINITY;
  }
}

// The front of stay(j), j = threadIdx.x < n, from the current beam (the arrays of this frame's half): pb' = lp[blank] + tot, pnb' =
// lp[e] + pnb before any merge, and the extension that spells entry j, if the frame has it: ext(pr, kj) with pr the rank of the
// parent prefix and kj the frame token equal to the last label e; its total starts from the acoustic sum `a` (CTC: lp[e] + pb of the
// parent when the parent ends in e too, else + its tot).  The search adds its own terms to a, adds that to spnb and marks the
// extension gone.
// The policy Pol says what the lattice is: BeamCtc below; BeamAsg (criterion_asg_beam.hpp) has no blank and a transition matrix A.
struct BeamTrans { const float* a; int lds; };   // A [N][N], to x from; lds: stage it in LDS.  BeamCtc: all 0
struct BeamCtc {
  static constexpr bool kNoBlank = false;
  __device__ static __forceinline__ const float* stage(const BeamTrans&, int) { return nullptr; }
  __device__ static __forceinline__ bool none(int, int) { return false; }   // has (token c, entry ending in e) no candidates?
  // the acoustic sum of the extension by c of an entry (e, pb, tot)
  __device__ static __forceinline__ float ext(float lpc, int c, int e, float pb, float tot, const float*, int) {
    return lpc + (c == e ? pb : tot);
  }
  __device__ static __forceinline__ void stay(float lpe, int e, float lpb, float pnb, float tot, const float*, int, float* spb,
                                              float* spnb) {
    *spb = lpb + tot;
    *spnb = e >= 0 ? lpe + pnb : -INFINITY;
  }
};

struct BeamStay { int e, kj, pr; bool merge; float spb, spnb, a; };   // merge: the frame has ext(pr, kj); a: its acoustic sum
template <class Pol = BeamCtc>
__device__ __forceinline__ BeamStay beam_stay_front(int n, int K, const int* sTc, const float* sTl, const int* sNode,
                                                    const int* sPar, const int* sE, const float* sPb, const float* sPnb,
                                                    const float* sTot, const float* xrow, float lpb, float lse,
                                                    const float* A = nullptr, int N = 0, int sil = -1, float silScore = 0.f) {
  const int j = threadIdx.x;
  BeamStay s;
  s.e = sE[j];
  const int par = sPar[j];
  s.kj = -1; s.pr = -1;
  for (int k = 0; k < K; ++k) s.kj = sTc[k] == s.e ? k : s.kj;
  for (int r = 0; r < n; ++r) s.pr = sNode[r] == par ? r : s.pr;
  // lp[e] comes from the row whether or not e is a frame token; with the silence score the extensions' tokLp carries
  Pol::stay(s.e >= 0 ? beam_sil_lp(xrow[s.e] - lse, s.e, sil, silScore) : 0.f, s.e, lpb, sPnb[j], sTot[j], A, N, &s.spb, &s.spnb);
  s.merge = s.pr >= 0 && s.kj >= 0;
  s.a = 0.f;
  if (s.merge) s.a = Pol::ext(sTl[s.kj], s.e, sE[s.pr], sPb[s.pr], sTot[s.pr], A, N);
  return s;
}

// One selection round: the block-wide 64-bit max of every thread's largest key (wave max, one LDS word per wave, ONE barrier: the
// words are double-buffered by round parity), then beam_pick.  Every thread gets the same answer.
template <int kWaves>
__device__ __forceinline__ bool beam_select_round(u64 local, int q, u64 (*sRed)[kWaves],
                                                  float threshold, float* best, BeamWin* w) {
  const int tid = threadIdx.x;
  const u64 wm = wave_max_u64(local);
  if ((tid & 63) == 0) sRed[q & 1][tid >> 6] = wm;
  __syncthreads();
  u64 wk = sRed[q & 1][0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) wk = sRed[q & 1][i] > wk ? sRed[q & 1][i] : wk;
  return beam_pick(wk, q, threshold, best, w);
}

// the final entries of utterance b, from the beam's arrays after the last frame (sU: the lexicon search's, else null)
__device__ __forceinline__ void beam_store_final(const CtcBeamWs& ws, int b, int n, const int* sNode, const float* sTot,
                                                 const int* sSt, const float* sAcc, const int* sU) {
  const int tid = threadIdx.x;
  if (tid >= 64) return;
  const bool live = tid < n;
  ws.finNode[b * kBeamMax + tid] = live ? sNode[tid] : -1;
  ws.finTot[b * kBeamMax + tid] = live ? sTot[tid] : -INFINITY;
  ws.finState[b * kBeamMax + tid] = live ? sSt[tid] : 0;
  ws.finAcc[b * kBeamMax + tid] = live ? sAcc[tid] : -INFINITY;
  if (sU) ws.finU[b * kBeamMax + tid] = live ? sU[tid] : -1;
  if (tid == 0) ws.finN[b] = n;
}

// ---- a beam that outlives the launch (the beam session of criterion_beam_stream.hpp; the scan bodies' kResume)
// The arrays the finishes read anyway -- node, tot, LM state, LM sum, lexicon node, n: the fin* of CtcBeamWs, [slot][64] -- are
// the stored beam's; BeamCarry adds what only the next frame needs.  pb and pnb are stored apart from tot: the extension by an
// entry's own last label adds pb alone.  cnt[slot]: the slot's frames of this step; flag[slot] bit 0: it starts from the empty
// prefix.  (cnt is followed by the slots' frame indices, ctc_beam_rows<., ., true>'s.)
struct BeamCarry {
  const int *cnt, *flag;
  int *par, *e, *lab;      // [S][64]; lab: the lexicon scan's
  float *pb, *pnb, *su;    // [S][64]; su: the lexicon scan's
};

// a slot's frames of this step and whether it starts; false: nothing to do
__device__ __forceinline__ bool beam_carry_begin(const BeamCarry& cy, int b, int T, int* F, bool* fresh) {
  *F = min(max(cy.cnt[b], 0), T);
  *fresh = (cy.flag[b] & 1) != 0;
  return *F > 0 || *fresh;
}

// The stored beam into the arrays of half 0; returns n.  What indexes memory is held to its range here (n to 64, the last label
// to the row, node ids to the table); LM states and lexicon nodes are clamped where they are used (ngram_q, lex_child, lex_node).
// The caller's barrier publishes the arrays.
__device__ __forceinline__ int beam_carry_load(const BeamCarry& cy, const CtcBeamWs& ws, int b, int N, int* sNode, int* sPar, int* sE,
                                               float* sPb, float* sPnb, float* sTot, int* sSt, float* sAcc, int* sLab, int* sU,
                                               float* sSu) {
  const int tid = threadIdx.x, n = min(max(ws.finN[b], 0), kBeamMax);
  if (tid < 64) {
    const int i = b * kBeamMax + tid;
    const bool live = tid < n;
    const int node = ws.finNode[i], e = cy.e[i];
    sNode[tid] = live ? ((unsigned)node <= ws.cap ? node : 0) : -2;
    sPar[tid] = live ? cy.par[i] : -1;
    sE[tid] = live && e >= 0 && e < N ? e : -1;
    sPb[tid] = live ? cy.pb[i] : -INFINITY;
    sPnb[tid] = live ? cy.pnb[i] : -INFINITY;
    sTot[tid] = live ? ws.finTot[i] : -INFINITY;
    sSt[tid] = live ? ws.finState[i] : 0;
    sAcc[tid] = live ? ws.finAcc[i] : 0.f;
    if (sLab) {
      sLab[tid] = live ? cy.lab[i] : -1;
      sU[tid] = live ? ws.finU[i] : 0;
      sSu[tid] = live ? cy.su[i] : 0.f;
    }
  }
  return n;
}

// what beam_store_final does not store (sLab: the lexicon scan's, else null)
__device__ __forceinline__ void beam_carry_store(const BeamCarry& cy, int b, int n, const int* sPar, const int* sE, const float* sPb,
                                                 const float* sPnb, const int* sLab, const float* sSu) {
  const int tid = threadIdx.x;
  if (tid >= 64 || tid >= n) return;
  const int i = b * kBeamMax + tid;
  cy.par[i] = sPar[tid]; cy.e[i] = sE[tid]; cy.pb[i] = sPb[tid]; cy.pnb[i] = sPnb[tid];
  if (sLab) { cy.lab[i] = sLab[tid]; cy.su[i] = sSu[tid]; }
}

// ---- the finishes

// What bounds a walk up the prefix table.  A whole search made the table in the same call and trusts it (the default: no bound).  A
// beam session reads node ids from a state buffer that lives between calls: a walk stays inside the table (capm) and ends after
// as many labels as the slot has had frames (steps), so a damaged state gives wrong labels, never a spin or a read outside.
struct BeamWalk { unsigned capm = ~0u; int steps = 0x7fffffff; };
__device__ __forceinline__ bool beam_walk_ok(const BeamWalk& g, int p) { return p > 0 && (unsigned)(p - 1) <= g.capm; }

// labels of the prefix that ends at `node`; with nwords, also how many of them carry a slot (the lexicon search's completed words)
__device__ __forceinline__ int beam_chain_len(const u64* tab, int node, int* nwords = nullptr, BeamWalk g = BeamWalk{}) {
  int len = 0, nw = 0;
  for (int p = node; len < g.steps && beam_walk_ok(g, p);) {
    const u64 edge = tab[p - 1];
    ++len;
    nw += (((unsigned)edge - 1u) & 7u) ? 1 : 0;
    p = (int)(edge >> 32);
  }
  if (nwords) *nwords = nw;
  return len;
}

// the labels of a live row (its prefix table's labels are the tokens) or none, padded with -1 to Lmax: the row's length
__device__ __forceinline__ int beam_write_labels(const u64* tab, bool live, const int* finNode, int Lmax, int* lab,
                                                 BeamWalk g = BeamWalk{}) {
  int len = 0;
  if (live) {
    const int node = *finNode;
    len = beam_chain_len(tab, node, nullptr, g);
    int i = len - 1;
    for (int p = node; i >= 0 && beam_walk_ok(g, p); --i) {
      const u64 edge = tab[p - 1];
      if (i < Lmax) lab[i] = (int)(unsigned)edge - 1;
      p = (int)(edge >> 32);
    }
  }
  for (int i = min(len, Lmax); i < Lmax; ++i) lab[i] = -1;
  return len;
}

// the end-of-sentence term: score + ((lmWeight * qe) + eosScore), one fp32 operation each, in this order; acc + qe
__device__ __forceinline__ void beam_eos(const void* __restrict__ lm, int state, int eosWord, float lmWeight, float eosScore,
                                         float* score, float* acc) {
  const NgramView lv = ngram_view(lm);
  int unused;
  const float qe = ngram_q(lv, state, eosWord, &unused);
  *score = *score + ((lmWeight * qe) + eosScore);
  *acc = *acc + qe;
}

// The output row of lane r = threadIdx.x of a one-wavefront finish: the alive lanes by (score descending, lane ascending), then
// the others -- the empty rows -- in lane order.  Every lane of the wavefront calls it.
__device__ __forceinline__ int beam_rerank(float score, bool alive, float* sScore) {
  const int r = threadIdx.x;
  const u64 am = __ballot(alive);
  sScore[r] = score;
  __syncthreads();
  if (!alive) return __popcll(am) + __popcll(~am & ((1ull << r) - 1ull));
  int m = 0;
  for (u64 rest = am; rest; rest &= rest - 1) {
    const int o = __ffsll((long long)rest) - 1;
    m += (sScore[o] > score || (sScore[o] == score && o < r)) ? 1 : 0;
  }
  return m;
}

__global__ __launch_bounds__(64) void ctc_beam_finish(int M, int Lmax, CtcBeamWs ws, int* __restrict__ labels,
                                                      int* __restrict__ lengths, float* __restrict__ scores) {
  const int b = blockIdx.x, m = threadIdx.x;
  if (m >= M) return;
  const u64* tab = ws.table + (size_t)b * ws.cap;
  int* lab = labels + ((size_t)b * M + m) * Lmax;
  const bool live = m < ws.finN[b];
  const int len = beam_write_labels(tab, live, ws.finNode + b * kBeamMax + m, Lmax, lab);
  lengths[(size_t)b * M + m] = live ? len : -1;
  scores[(size_t)b * M + m] = live ? ws.finTot[b * kBeamMax + m] : -INFINITY;
}

// tokens = the classes that are tokens: N - 1 with a blank, N without (noBlank)
static int ctc_beam_clip(int tokens, int beamToken) { return beamToken < tokens ? beamToken : tokens; }

// ---- the host side of a whole search: one request, its checks, the row pass.  The route from a request to a kernel family, the
// narrow family's run and every entry point are criterion_beam_entry.hpp's; the wide and xl runs are their headers'.

enum BeamKind { kSearchPlain = 0, kSearchLm = 1, kSearchLex = 2, kSearchLextok = 3 };   // w2l_beam_search_kind's values
enum BeamFamily { kFamNarrow = 0, kFamWide = 1, kFamXl = 2, kFamMt = 3 };               // w2l_beam_family's values

// Everything a search call carries; never crosses into device code.  asg: every class a token and `trans` required (an entry
// point's name says so, not the pointer).  kind: the ASG token search is kSearchLm with or without an LM; kSearchPlain is CTC's.
struct BeamReq {
  int kind = kSearchPlain;
  bool asg = false;
  int B = 0, T = 0, N = 0;
  const float* input = nullptr;
  const int* frames = nullptr;
  const float* trans = nullptr;
  int beam = 0, beamToken = 0;
  float threshold = 0.f;
  int logAdd = 0, normalize = 0, nbest = 0, maxLen = 0;
  const void* lm = nullptr;
  int lmHasEos = 0;
  float lmWeight = 0.f;
  const float* classScore = nullptr;
  const void* lexicon = nullptr;
  float wordScore = 0.f;
  float eosScore = 0.f;
  int* labels = nullptr;
  int* lengths = nullptr;
  float* scores = nullptr;
  float* lmScores = nullptr;
  int maxWords = 0;
  int* words = nullptr;
  int* wordCounts = nullptr;
  void* workspace = nullptr;
  hipStream_t stream = nullptr;
  BeamSil sil;

  int tokens() const { return asg ? N : N - 1; }   // the classes that are tokens
  bool lex() const { return kind >= kSearchLex; }
};

static bool beam_finite(float v) { return fabsf(v) < INFINITY; }

// what the silence arguments add to a search's refusals
static int beam_sil_check(const BeamReq& q) {
  if (!beam_finite(q.sil.score) || q.sil.token < -1 || q.sil.token >= q.tokens()) return W2L_EINVAL;
  return W2L_OK;
}

// no silence score: the search runs with BeamSil{}, whose token matches no class -- the sibling's kernels and bytes, no + 0
static bool beam_sil_none(const BeamSil& sil) { return sil.token < 0 || sil.score == 0.f; }

// a search's own refusals, all W2L_EINVAL; the plain CTC search has none
static int beam_req_check(const BeamReq& q) {
  if (q.asg && !q.trans) return W2L_EINVAL;
  if (q.kind == kSearchPlain) return W2L_OK;
  if (!q.lmScores || (!q.lm && !(q.asg && q.kind == kSearchLm))) return W2L_EINVAL;
  if (q.lex() && (!q.lexicon || !q.words || !q.wordCounts || q.maxWords < 1)) return W2L_EINVAL;
  if (!beam_finite(q.lmWeight) || !beam_finite(q.eosScore) || (q.lex() && !beam_finite(q.wordScore))) return W2L_EINVAL;
  if (!q.lmHasEos && q.eosScore != 0.f) return W2L_EINVAL;
  if (!q.lm && (q.lmHasEos || q.classScore)) return W2L_EINVAL;   // the ASG token search without an LM
  return W2L_OK;
}

// The arguments every search shares, against a family's limits; *K = the clipped beamToken.  Every W2L_EINVAL comes before
// W2L_EUNSUPPORTED, and the silence arguments' and the search's own checks (all W2L_EINVAL) run before this one, so the code for a
// bad argument does not depend on which one is first.
static int beam_common_check(const BeamReq& q, int maxBeam, int maxTokens, int* K) {
  if (q.B <= 0 || q.T <= 0 || q.N < 2 || !q.input || !q.labels || !q.lengths || !q.scores || !q.workspace) return W2L_EINVAL;
  if (q.beam <= 0 || q.beamToken <= 0 || q.nbest <= 0 || q.nbest > q.beam || q.maxLen <= 0) return W2L_EINVAL;
  if (!(q.threshold >= 0.f)) return W2L_EINVAL;   // NaN or negative
  *K = ctc_beam_clip(q.tokens(), q.beamToken);
  if (q.beam > maxBeam || *K > maxTokens) return W2L_EUNSUPPORTED;
  if ((size_t)q.T * q.beam > ((size_t)1 << 29)) return W2L_EUNSUPPORTED;   // node ids are ints
  return W2L_OK;
}

// the start of a run after the workspace is laid out: the silence score, an empty prefix table, the frame tokens of every row
static int beam_rows_launch(const BeamReq& q, CtcBeamWs* ws) {
  ws->sil = q.sil.token; ws->silScore = q.sil.score;
  W2L_HIP_CHECK(hipMemsetAsync(ws->table, 0, (size_t)q.B * ws->cap * sizeof(u64), q.stream));
  const dim3 rows((unsigned)((size_t)q.B * q.T)), threads(kRowThreads);
  const bool big = q.N > kRowThreads * kRowMaxPer;
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, rows, threads, 0, q.stream, q.T, q.N, q.normalize, q.input, q.frames, *ws); };
  if (q.asg && big) launch(ctc_beam_rows<true, true>);
  else if (q.asg) launch(ctc_beam_rows<false, true>);
  else if (!big) launch(ctc_beam_rows<false>);
  else launch(ctc_beam_rows<true>);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

// The dispatch of a workgroup scan kernel<logAdd, threads>, one workgroup per utterance: 256 threads while they own every (entry,
// token) pair, else 1024.  launch(logAdd, threads) gets the two as std::integral_constant types and starts that instantiation.
template <class Launch>
static void ctc_beam_fused_scan(int W, int K, int logAdd, Launch&& launch) {
  const bool wide = W * K > 256 * kLmPer;
  if (logAdd && wide) launch(std::true_type{}, std::integral_constant<int, 1024>{});
  else if (logAdd) launch(std::true_type{}, std::integral_constant<int, 256>{});
  else if (wide) launch(std::false_type{}, std::integral_constant<int, 1024>{});
  else launch(std::false_type{}, std::integral_constant<int, 256>{});
}

}  // namespace w2l
