// criterion_beam_wide.hpp -- the five wide beam searches (w2l_*_beam_search*_wide): the contracts of the CTC and ASG beam searches
// (include/w2l_hip.h) with a beam of up to kBeamWideMax = 1024 entries.  Included at the end of criterion_ctc.hip after the narrow
// searches' headers, whose row kernel (ctc_beam_rows), prefix table (beam_node, ctc_beam_cap), keys (beam_key, beam_ord), (+)
// (beam_oplus), lattice policies (BeamCtc, BeamAsg), LM and lexicon terms (beam_lm_ext, beam_lex_a, beam_lex_word), end-of-sentence
// term (beam_eos) and chain walk (beam_chain_len, beam_write_labels) it reuses as they are.  New here: a scan whose selection is
// parallel, and a finish for up to 1024 rows.
//   beam_wide_scan<logAdd, Pol, lex>  one workgroup of 1024 threads per utterance; the beam of this frame and the next one (8 fields
//                      of 4 bytes per entry, 9 with a lexicon) in dynamic LDS, 64 or 72 KiB.  `lm` may be null under both policies:
//                      the LM-free CTC search is the token scan without an LM.  A frame:
//     stays       the ranks of the current entries' nodes go into an LDS hash (2048 slots, bounded probes); thread j < n owns
//                 stay(j): it finds its parent's rank there, recomputes the one extension that spells its prefix with the narrow
//                 scans' operation sequence, adds it to its pnb' and sets that extension's bit in the gone masks (one 64-bit word
//                 per entry, and per slot with a lexicon).
//     candidates  every stay and every extension that did not merge, and is not -inf, is written as its 64-bit key into the
//                 utterance's candidate list in the workspace (the position: one LDS counter).  The list holds W * K * 7 + W keys
//                 with a lexicon, W * K + W without: the worst case, so no candidate is ever dropped.  Only the key is kept; the
//                 LM successor, the LM log-probability and the lexicon node of a winner are looked up again from its (rank, token,
//                 slot) -- the same loads, the same values -- by the thread that writes the new entry.
//     selection   keys are unique, so the W best are those at or above the W-th largest key: an MSB-first radix select, 8 bits a
//                 pass with a 256-bin LDS histogram, which ends as soon as the bin that holds the W-th key is taken whole.  The
//                 survivors -- at or above that key, not under the threshold line of the frame's best total -- are at most W; they
//                 are gathered into LDS and sorted there (bitonic, descending), so an entry's rank is a function of the keys alone,
//                 never of the order in which atomics arrived.
//     next beam   thread q < m decodes the key of rank q and writes entry q; a new prefix gets its node from the prefix table.
//                 No waiting between workgroups, no flags, no spin loops; every probe loop is bounded by its table's capacity; every
//                 barrier is reached by all 1024 threads, and every loop with a barrier inside runs on counts read from LDS after a
//                 barrier, the same in every thread.
//   beam_wide_finish<lex>  one workgroup of 1024 threads per utterance, thread r = final entry r: the lexicon's root-only rule, the
//                      end-of-sentence term, the re-ranking by (score descending, previous rank ascending) as a sort of 64-bit keys
//                      in LDS, then thread m < M writes row m.
// Both are device BODIES (beam_wide_scan_body with a kResume flag, beam_wide_finish_body with the entry count and the walk bounds
// as arguments); the kernels above instantiate them for a whole search, criterion_beam_stream.hpp for a slot of a wide beam
// session, whose beam lives in a state buffer between launches (BeamWideCarry).
#pragma once

namespace w2l {

constexpr int kWideThreads = 1024;
constexpr int kWideHash = 2048;                // slots of the node -> rank hash: load factor <= 1/2
constexpr size_t kWideTransLds = 8 * 1024;     // the ASG matrix is staged in LDS up to this size (N <= 45), else gathered

struct BeamWideWs {
  CtcBeamWs c;       // lse, lpb, tokLp, tokC, table, fin* (fin* with W entries per utterance, not kBeamMax), K, cap
  u64* cand;         // [B][candCap] the candidate keys of the frame
  size_t candCap;    // W * K * slots + W
  int W;
};

static size_t beam_wide_layout(BeamWideWs* w, void* ws, int B, int T, int W, int K, int variant) {
  const size_t rows = (size_t)B * T, cap = ctc_beam_cap(T, W);
  const size_t candCap = (size_t)W * K * (variant == kBeamLex ? 7 : 1) + (size_t)W;
  char* p = (char*)ws;
  char* const p0 = p;
  float* lse = (float*)p; p += align_up(rows * sizeof(float), 256);
  float* lpb = (float*)p; p += align_up(rows * sizeof(float), 256);
  float* tokLp = (float*)p; p += align_up(rows * K * sizeof(float), 256);
  int* tokC = (int*)p; p += align_up(rows * K * sizeof(int), 256);
  u64* table = (u64*)p; p += align_up((size_t)B * cap * sizeof(u64), 256);
  u64* cand = (u64*)p; p += align_up((size_t)B * candCap * sizeof(u64), 256);
  const size_t fin = align_up((size_t)B * W * 4, 256);
  int* finNode = (int*)p; p += fin;
  float* finTot = (float*)p; p += fin;
  int* finN = (int*)p; p += align_up((size_t)B * sizeof(int), 256);
  int* finState = (int*)p; p += fin;
  float* finAcc = (float*)p; p += fin;
  int* finU = nullptr;
  if (variant == kBeamLex) { finU = (int*)p; p += fin; }
  if (w) {
    w->c = CtcBeamWs{lse, lpb, tokLp, tokC, table, finNode, finTot, finN, finState, finAcc, finU, K, (unsigned)cap};
    w->cand = cand; w->candCap = candCap; w->W = W;
  }
  return (size_t)(p - p0);
}

// the dynamic LDS of beam_wide_scan after the staged transition matrix, in bytes
template <bool kLex>
struct WideLds {
  static constexpr int kFields = kLex ? 9 : 8;
  static constexpr int kSlots = kLex ? 7 : 1;
  static constexpr size_t beam = 0;                                                  // [2][kFields][1024] 4-byte words
  static constexpr size_t scr = beam + (size_t)2 * kFields * kWideThreads * 4;      // 16 KiB: hash; then spb, spnb | sort keys
  static constexpr size_t gone = scr + (size_t)kWideHash * 8;                        // [kSlots][1024] u64
  static constexpr size_t tc = gone + (size_t)kSlots * kWideThreads * 8;            // [64] int
  static constexpr size_t tl = tc + 64 * 4;                                          // [64] float
  static constexpr size_t hist = tl + 64 * 4;                                        // [256] unsigned
  static constexpr size_t red = hist + 256 * 4;                                      // [16] u64
  static constexpr size_t misc = red + 16 * 8;                                       // [8] unsigned
  static constexpr size_t bytes = misc + 8 * 4;
};

// s[0 .. n2) descending, n2 a power of two <= 1024; every thread of the workgroup calls it; ends with a barrier
__device__ __forceinline__ void beam_wide_sort(u64* s, int n2) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int o = tid ^ j;
      if (tid < n2 && o > tid) {
        const u64 a = s[tid], c = s[o];
        const bool desc = (tid & k) == 0;
        if (desc ? a < c : a > c) { s[tid] = c; s[o] = a; }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ int beam_wide_pow2(int m) {
  int n2 = 2;
  while (n2 < m) n2 <<= 1;
  return n2;
}

// the lexicon node an entry stands at, from the label of its last extension: (node << 3) | slot, -1 for the empty prefix
__device__ __forceinline__ int beam_wide_u(int lab) { return (lab < 0 || (lab & 7)) ? 0 : (lab >> 3); }

// ---- a wide beam that outlives the launch (the wide beam session of criterion_beam_stream.hpp; the scan body's kResume)
// As BeamCarry for the narrow scans: the fin* arrays of the workspace ([slot][W]: node, tot, LM state, LM sum, lexicon node, n) are
// the stored beam's; BeamWideCarry adds what only the next frame needs.  pb and pnb are stored apart from tot: the extension by an
// entry's own last label adds pb alone.  Rank order is array order.  cnt[slot]: the slot's frames of this step; flag[slot] bit 0: it
// starts from the empty prefix.  (cnt is followed by the slots' frame indices, ctc_beam_rows<., ., true>'s.)
struct BeamWideCarry {
  const int *cnt, *flag;
  int *par, *e, *lab;   // [S][W]; lab: the lexicon scan's
  float *pb, *pnb;      // [S][W]
};

// kResume (criterion_beam_stream.hpp): utterance b is a slot of a wide beam session: its frame count (0: none) and start flag come
// from cy.cnt / cy.flag -- the same in every thread, read before the first barrier, so the workgroup leaves or stays as one --, the
// beam from the session's state unless the slot starts, and every field goes back there after the frames.  What indexes memory is
// held to its range where it is loaded (n to W, node ids to the table, the last token to the row); LM states and lexicon nodes
// are clamped where they are used (ngram_q, lex_child, lex_node).  beam_wide_scan below is the body with kResume off.
// kTok (with kLex; criterion_beam_lextok.hpp): `lm` is a token LM under the lexicon: a token that moves along a trie edge adds
// lmWeight * q(s, c) and advances the LM state, a completed word adds wordScore alone, the smear values are not read.
template <bool kLogAdd, class Pol, bool kLex, bool kResume, bool kTok = false>
__device__ __forceinline__ void beam_wide_scan_body(int T, int N, int W, float threshold, const float* __restrict__ x,
                                                    const int* __restrict__ frames, const BeamWideWs& ww,
                                                    const void* __restrict__ lex, const void* __restrict__ lm, float lmWeight,
                                                    const float* __restrict__ classScore, float wordScore, BeamTrans tr,
                                                    const BeamWideCarry& cy) {
  using L = WideLds<kLex>;
  constexpr int kF = L::kFields, kTh = kWideThreads;
  extern __shared__ float sAsgTrans[];   // BeamAsg::stage's array: the staged matrix comes first
  char* const base = (char*)sAsgTrans + (tr.lds ? (((size_t)N * N * sizeof(float) + 15) & ~(size_t)15) : 0);
  int* const sBeam = (int*)(base + L::beam);
  u64* const sScr = (u64*)(base + L::scr);
  float* const sSpb = (float*)sScr;             // after the stays: pb' and pnb' of stay(j)
  float* const sSpnb = sSpb + kTh;
  u64* const sSort = sScr + kTh;                // the survivors' keys
  u64* const sGone = (u64*)(base + L::gone);
  int* const sTc = (int*)(base + L::tc);
  float* const sTl = (float*)(base + L::tl);
  unsigned* const sHist = (unsigned*)(base + L::hist);
  u64* const sRed = (u64*)(base + L::red);
  unsigned* const sMisc = (unsigned*)(base + L::misc);   // 0: candidates, 1: survivors, 2: bin, 3: keys above it, 4: keys in it

  const CtcBeamWs& ws = ww.c;
  const int b = blockIdx.x, tid = threadIdx.x, K = ws.K;
  int F;
  bool fresh = true;
  if constexpr (kResume) {
    F = min(max(cy.cnt[b], 0), T);
    fresh = (cy.flag[b] & 1) != 0;
    if (F == 0 && !fresh) return;   // the whole workgroup, before any barrier
  } else {
    F = align_frames(frames, b, T);
  }
  const float* xb = x + (size_t)b * T * N;
  u64* tab = ws.table + (size_t)b * ws.cap;
  const unsigned capm = ws.cap - 1;
  const size_t row0 = (size_t)b * T;
  u64* cand = ww.cand + (size_t)b * ww.candCap;
  const unsigned candCap = (unsigned)ww.candCap;
  const bool useLm = kLex || lm != nullptr;
  const NgramView lv = useLm ? ngram_view(lm) : NgramView{};
  LexView xv{};
  if constexpr (kLex) xv = lex_view(lex);
  const float* A = Pol::stage(tr, N);

  // field f of half h of the beam: 0 node, 1 parent's node, 2 last token, 3 LM state, 4 pb, 5 pnb, 6 tot, 7 unweighted LM sum,
  // 8 (lexicon) the label of the last extension
  auto fi = [&](int h, int f) { return sBeam + (h * kF + f) * kTh; };
  auto ff = [&](int h, int f) { return (float*)(sBeam + (h * kF + f) * kTh); };

  int cur = 0, n = 1;
  if (!fresh) {   // kResume alone; thread j loads entry j, the first frame's barrier publishes it
    n = min(max(ws.finN[b], 0), min(W, kTh));
    if (tid < n) {
      const size_t o = (size_t)b * ww.W + tid;
      const int node = ws.finNode[o], e = cy.e[o];
      fi(0, 0)[tid] = (unsigned)node <= ws.cap ? node : 0; fi(0, 1)[tid] = cy.par[o]; fi(0, 2)[tid] = e >= 0 && e < N - 1 ? e : -1;
      fi(0, 3)[tid] = ws.finState[o];
      ff(0, 4)[tid] = cy.pb[o]; ff(0, 5)[tid] = cy.pnb[o]; ff(0, 6)[tid] = ws.finTot[o]; ff(0, 7)[tid] = ws.finAcc[o];
      if constexpr (kLex) fi(0, 8)[tid] = cy.lab[o];
    }
  } else if (tid == 0) {
    fi(0, 0)[0] = 0; fi(0, 1)[0] = -1; fi(0, 2)[0] = -1; fi(0, 3)[0] = useLm ? (int)((const NgramHeader*)lm)->start : 0;
    ff(0, 4)[0] = 0.f; ff(0, 5)[0] = -INFINITY; ff(0, 6)[0] = 0.f; ff(0, 7)[0] = 0.f;
    if constexpr (kLex) fi(0, 8)[0] = -1;
  }
  for (int t = 0; t < F && n > 0; ++t) {
    const size_t row = row0 + t;
    const int nxt = cur ^ 1;
    const int *cNode = fi(cur, 0), *cPar = fi(cur, 1), *cE = fi(cur, 2), *cSt = fi(cur, 3);
    const float *cPb = ff(cur, 4), *cPnb = ff(cur, 5), *cTot = ff(cur, 6), *cAcc = ff(cur, 7);
    const int* cLab = kLex ? fi(cur, 8) : nullptr;

    beam_load_frame(ws, row, sTc, sTl);
    if (tid < n)
      for (int s = 0; s < L::kSlots; ++s) sGone[s * kTh + tid] = 0ull;
    sScr[tid] = 0ull; sScr[tid + kTh] = 0ull;
    if (tid < 2) sMisc[tid] = 0u;
    const float lpb = ws.lpb[row], lse = ws.lse[row];
    __syncthreads();
    // the rank of every current node
    if (tid < n) {
      const unsigned nd1 = (unsigned)cNode[tid] + 1u;
      const u64 rec = ((u64)nd1 << 32) | (u64)(unsigned)tid;
      unsigned h = beam_hash(nd1) & (kWideHash - 1);
      for (int probe = 0; probe < kWideHash; ++probe) {
        if (atomicCAS(&sScr[h], 0ull, rec) == 0ull) break;
        h = (h + 1) & (kWideHash - 1);
      }
    }
    __syncthreads();
    // stay(tid), with the extension that spells this entry merged in
    u64 stayKey = 0ull;
    float spb = -INFINITY, spnb = -INFINITY;
    if (tid < n) {
      const int e = cE[tid], par = cPar[tid];
      int kj = -1, pr = -1;
      for (int k = 0; k < K; ++k) kj = sTc[k] == e ? k : kj;
      if (par >= 0) {
        const unsigned pd1 = (unsigned)par + 1u;
        unsigned h = beam_hash(pd1) & (kWideHash - 1);
        for (int probe = 0; probe < kWideHash; ++probe) {
          const u64 rec = sScr[h];
          if (rec == 0ull) break;
          if ((unsigned)(rec >> 32) == pd1) { pr = (int)(unsigned)rec; break; }
          h = (h + 1) & (kWideHash - 1);
        }
      }
      Pol::stay(e >= 0 ? beam_sil_lp(xb[(size_t)t * N + e] - lse, e, ws.sil, ws.silScore) : 0.f, e, lpb, cPnb[tid], cTot[tid], A, N,
                &spb, &spnb);
      if (pr >= 0 && kj >= 0) {
        float v = Pol::ext(sTl[kj], e, cE[pr], cPb[pr], cTot[pr], A, N);
        if constexpr (!kLex) {
          if (useLm) {
            int unused;
            const float qm = ngram_q(lv, cSt[pr], e, &unused);
            v = beam_lm_ext(v, lmWeight, qm, classScore, e);
          }
          spnb = beam_oplus<kLogAdd>(spnb, v);
          atomicOr(&sGone[pr], 1ull << kj);
        } else {
          const int lab = cLab[tid];
          if (lab >= 0) {
            const int vj = lab >> 3, slot = lab & 7;
            if constexpr (kTok) {
              if (vj != 0) {
                int unused;
                v = beam_lextok_a(v, lmWeight, ngram_q(lv, cSt[pr], e, &unused));
                if (slot > 0) v = v + wordScore;
              }
            } else if (vj != 0) {
              const LexNode& nd = lex_node(xv, vj);
              const float smv = nd.smear;
              const int up = beam_wide_u(cLab[pr]);
              v = beam_lex_a(v, lmWeight, smv, up == 0 ? 0.f : lex_node(xv, up).smear);
              if (slot > 0) {
                int unused;
                const float qm = ngram_q(lv, cSt[pr], nd.words[min(slot - 1, kLexMaxWords - 1)], &unused);
                v = beam_lex_word(v, lmWeight, qm, smv, wordScore);
              }
            }
            spnb = beam_oplus<kLogAdd>(spnb, v);
            atomicOr(&sGone[min(slot, 6) * kTh + pr], 1ull << kj);
          }
        }
      }
      stayKey = beam_key(beam_oplus<kLogAdd>(spb, spnb), tid, 0, 0);
    }
    __syncthreads();   // the hash is read, the gone masks are complete
    if (tid < n) { sSpb[tid] = spb; sSpnb[tid] = spnb; }

    // every candidate of the frame that is not -inf: its key into the list
    u64 local = 0ull;
    auto put = [&](u64 key) {
      if ((unsigned)(key >> 32) == beam_ord(-INFINITY)) return;
      const unsigned pos = atomicAdd(&sMisc[0], 1u);
      if (pos < candCap) cand[pos] = key;
      local = key > local ? key : local;
    };
    if (stayKey) put(stayKey);
    const int total = n * K;
    for (int idx = tid; idx < total; idx += kTh) {
      const int r = idx / K, k = idx - r * K, c = sTc[k], e = cE[r];
      if (Pol::none(c, e)) continue;
      const float a0 = Pol::ext(sTl[k], c, e, cPb[r], cTot[r], A, N);
      if constexpr (!kLex) {
        if ((sGone[r] >> k) & 1ull) continue;
        float v = a0;
        if (useLm) {
          int unused;
          const float q = ngram_q(lv, cSt[r], c, &unused);
          v = beam_lm_ext(v, lmWeight, q, classScore, c);
        }
        put(beam_key(v, r, 1, k));
      } else {
        const int u = beam_wide_u(cLab[r]);
        if (c == xv.silToken && u == 0) {
          if (!((sGone[r] >> k) & 1ull)) put(beam_key(a0, r, 1, k, 0));
        } else if constexpr (kTok) {   // one LM lookup per pair that has an edge: this scan is bound by its lookups, not their latency
          const int v = lex_child(xv, u, c);
          if (v > 0) {
            const LexNode& nd = lex_node(xv, v);
            int unused;
            const float a = beam_lextok_a(a0, lmWeight, ngram_q(lv, cSt[r], c, &unused));
            if (lex_has_children(nd) && !((sGone[r] >> k) & 1ull)) put(beam_key(a, r, 1, k, 0));
            const int nw = lex_nw(nd);
            for (int i = 0; i < nw; ++i)
              if (!((sGone[(1 + i) * kTh + r] >> k) & 1ull)) put(beam_key(a + wordScore, r, 1, k, 1 + i));
          }
        } else {
          const int v = lex_child(xv, u, c);
          if (v > 0) {
            const LexNode& nd = lex_node(xv, v);
            const float smv = nd.smear;
            const float a = beam_lex_a(a0, lmWeight, smv, u == 0 ? 0.f : lex_node(xv, u).smear);
            if (lex_has_children(nd) && !((sGone[r] >> k) & 1ull)) put(beam_key(a, r, 1, k, 0));
            const int nw = lex_nw(nd);
            for (int i = 0; i < nw; ++i)
              if (!((sGone[(1 + i) * kTh + r] >> k) & 1ull)) {
                int unused;
                const float q = ngram_q(lv, cSt[r], nd.words[i], &unused);
                put(beam_key(beam_lex_word(a, lmWeight, q, smv, wordScore), r, 1, k, 1 + i));
              }
          }
        }
      }
    }
    {
      const u64 wm = wave_max_u64(local);
      if ((tid & 63) == 0) sRed[tid >> 6] = wm;
    }
    __syncthreads();   // the list, its count and the waves' maxima
    const int cnt = (int)min(sMisc[0], candCap);
    u64 bestKey = sRed[0];
#pragma unroll
    for (int i = 1; i < kTh / 64; ++i) bestKey = sRed[i] > bestKey ? sRed[i] : bestKey;
    const float best = beam_unord((unsigned)(bestKey >> 32));   // cnt == 0: not used

    // the W-th largest key (1 when there are no more than W): MSB-first radix select
    u64 tau = 1ull;
    if (cnt > W) {
      u64 prefix = 0ull;
      unsigned want = (unsigned)W;
      for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (tid < 256) sHist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < cnt; i += kTh) {
          const u64 key = cand[i];
          if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sHist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 256) {
          unsigned above = 0u;
          for (int j = tid + 1; j < 256; ++j) above += sHist[j];
          const unsigned mine = sHist[tid];
          if (above < want && above + mine >= want) { sMisc[2] = (unsigned)tid; sMisc[3] = above; sMisc[4] = mine; }
        }
        __syncthreads();
        prefix |= (u64)sMisc[2] << shift;
        want -= sMisc[3];
        if (want == sMisc[4]) break;   // the bin is taken whole: every key at or above the prefix, and no other
      }
      tau = prefix;
    }
    // the survivors, then their ranks
    for (int i = tid; i < cnt; i += kTh) {
      const u64 key = cand[i];
      if (key >= tau && !(beam_unord((unsigned)(key >> 32)) < best - threshold)) {
        const unsigned pos = atomicAdd(&sMisc[1], 1u);
        if (pos < (unsigned)kTh) sSort[pos] = key;
      }
    }
    __syncthreads();
    const int m = (int)min(sMisc[1], (unsigned)W);
    const int n2 = beam_wide_pow2(m);
    if (tid >= m && tid < n2) sSort[tid] = 0ull;
    __syncthreads();
    beam_wide_sort(sSort, n2);

    // entry tid of the next beam
    if (tid < m) {
      const u64 key = sSort[tid];
      const unsigned tie = 0xffffffffu - (unsigned)key;
      const int r = min((int)(tie >> 10), kTh - 1), ext = (int)((tie >> 9) & 1u), k = (int)((tie >> 3) & 63u), slot = (int)(tie & 7u);
      if (!ext) {
        const float pb = sSpb[r], pnb = sSpnb[r];
        fi(nxt, 0)[tid] = cNode[r]; fi(nxt, 1)[tid] = cPar[r]; fi(nxt, 2)[tid] = cE[r]; fi(nxt, 3)[tid] = cSt[r];
        ff(nxt, 4)[tid] = pb; ff(nxt, 5)[tid] = pnb; ff(nxt, 6)[tid] = beam_oplus<kLogAdd>(pb, pnb); ff(nxt, 7)[tid] = cAcc[r];
        if constexpr (kLex) fi(nxt, 8)[tid] = cLab[r];
      } else {
        const float tot = beam_unord((unsigned)(key >> 32));
        const int c = sTc[k];
        int st = cSt[r], label = c;
        float acc = cAcc[r];
        if constexpr (!kLex) {
          st = 0;
          float q = 0.f;
          if (useLm) q = ngram_q(lv, cSt[r], c, &st);
          acc = acc + q;
        } else {
          const int u = beam_wide_u(cLab[r]);
          const int v = (c == xv.silToken && u == 0) ? 0 : max(lex_child(xv, u, c), 0);
          label = (v << 3) | slot;
          if constexpr (kTok) {
            if (v != 0) {
              const float q = ngram_q(lv, cSt[r], c, &st);
              acc = acc + q;
            }
          } else if (slot > 0) {
            const float q = ngram_q(lv, cSt[r], lex_node(xv, v).words[min(slot - 1, kLexMaxWords - 1)], &st);
            acc = acc + q;
          }
          fi(nxt, 8)[tid] = label;
        }
        const int par = cNode[r];
        fi(nxt, 0)[tid] = beam_node(tab, capm, par, label);   // a new prefix
        fi(nxt, 1)[tid] = par; fi(nxt, 2)[tid] = c; fi(nxt, 3)[tid] = st;
        ff(nxt, 4)[tid] = -INFINITY; ff(nxt, 5)[tid] = tot; ff(nxt, 6)[tid] = tot; ff(nxt, 7)[tid] = acc;
      }
    }
    __syncthreads();
    n = m;
    cur = nxt;
  }
  // the final entries
  {
    const bool live = tid < n;
    if (tid < W) {
      const size_t o = (size_t)b * ww.W + tid;
      ws.finNode[o] = live ? fi(cur, 0)[tid] : -1;
      ws.finTot[o] = live ? ff(cur, 6)[tid] : -INFINITY;
      ws.finState[o] = live ? fi(cur, 3)[tid] : 0;
      ws.finAcc[o] = live ? ff(cur, 7)[tid] : -INFINITY;
      if constexpr (kLex) ws.finU[o] = live ? beam_wide_u(fi(cur, 8)[tid]) : -1;
    }
    if (tid == 0) ws.finN[b] = n;
    if constexpr (kResume) {   // what the fin* arrays do not hold; thread j stores the entry it wrote (or loaded) itself
      if (live) {
        const size_t o = (size_t)b * ww.W + tid;
        cy.par[o] = fi(cur, 1)[tid]; cy.e[o] = fi(cur, 2)[tid]; cy.pb[o] = ff(cur, 4)[tid]; cy.pnb[o] = ff(cur, 5)[tid];
        if constexpr (kLex) cy.lab[o] = fi(cur, 8)[tid];
      }
    }
  }
}

template <bool kLogAdd, class Pol, bool kLex, bool kTok = false>
__global__ __launch_bounds__(kWideThreads) void beam_wide_scan(int T, int N, int W, float threshold,
                                                               const float* __restrict__ x, const int* __restrict__ frames,
                                                               BeamWideWs ww, const void* __restrict__ lex,
                                                               const void* __restrict__ lm, float lmWeight,
                                                               const float* __restrict__ classScore, float wordScore, BeamTrans tr) {
  beam_wide_scan_body<kLogAdd, Pol, kLex, false, kTok>(T, N, W, threshold, x, frames, ww, lex, lm, lmWeight, classScore, wordScore,
                                                       tr, BeamWideCarry{});
}

// eosWord: the LM's index of the end of a sentence (the token searches'; the lexicon search takes it from the LM's header);
// lmScores null: the LM-free CTC search, which has no such output
// n: the final entries of utterance b, the same in every thread; g: what bounds the walks up the prefix table (BeamWalk{}: nothing)
template <bool kLex>
__device__ __forceinline__ void beam_wide_finish_body(int b, int n, BeamWalk g, int M, int Lmax, int maxWords, int eosWord,
                                                      const BeamWideWs& ww, const void* __restrict__ lex,
                                                      const void* __restrict__ lm, float lmWeight, float eosScore, int useEos,
                                                      int* __restrict__ labels, int* __restrict__ lengths,
                                                      float* __restrict__ scores, float* __restrict__ lmScores,
                                                      int* __restrict__ words, int* __restrict__ wordCounts) {
  __shared__ u64 sKey[kWideThreads];
  __shared__ float sScore[kWideThreads], sAcc[kWideThreads];
  const CtcBeamWs& ws = ww.c;
  const int r = threadIdx.x;
  const u64* tab = ws.table + (size_t)b * ws.cap;
  const size_t o = (size_t)b * ww.W + min(r, ww.W - 1);
  const bool alive = r < n && (!kLex || ws.finU[o] == 0);   // with a lexicon only finished words count at the end
  float score = -INFINITY, acc = -INFINITY;
  if (alive) {
    score = ws.finTot[o];
    acc = ws.finAcc[o];
    if (useEos) {
      const int ew = kLex ? (int)((const NgramHeader*)lm)->numTokens + 1 : eosWord;
      beam_eos(lm, ws.finState[o], ew, lmWeight, eosScore, &score, &acc);
    }
  }
  sScore[r] = score; sAcc[r] = acc;
  sKey[r] = alive ? ((u64)beam_ord(score) << 32) | (u64)(0xffffffffu - (unsigned)r) : 0ull;
  const int nAlive = __syncthreads_count(alive);
  beam_wide_sort(sKey, beam_wide_pow2(n));   // the keys beyond n are 0 and stay where they are
  const int m = r;
  if (m >= M) return;
  const bool live = m < nAlive;
  const int src = live ? (int)(0xffffffffu - (unsigned)sKey[m]) : 0;
  const size_t row = (size_t)b * M + m;
  int* lab = labels + row * Lmax;
  int len = 0, nwords = 0;
  if constexpr (!kLex) {
    len = beam_write_labels(tab, live, ws.finNode + (size_t)b * ww.W + src, Lmax, lab, g);
  } else {
    const LexView xv = lex_view(lex);
    int* wrd = words + row * maxWords;
    if (live) {
      const int node = ws.finNode[(size_t)b * ww.W + src];
      len = beam_chain_len(tab, node, &nwords, g);
      int i = len - 1, j = nwords - 1;
      for (int p = node; i >= 0 && beam_walk_ok(g, p); --i) {   // len labels: the walk above counted them under the same bound
        const u64 edge = tab[p - 1];
        const unsigned l = (unsigned)edge - 1u;
        const int v = (int)(l >> 3), slot = (int)(l & 7u);
        const LexNode& nd = lex_node(xv, v);
        if (i < Lmax) lab[i] = v == 0 ? xv.silToken : nd.tok;
        if (slot > 0) {
          if (j >= 0 && j < maxWords) wrd[j] = nd.words[min(slot - 1, kLexMaxWords - 1)];
          --j;
        }
        p = (int)(edge >> 32);
      }
    }
    for (int i = min(len, Lmax); i < Lmax; ++i) lab[i] = -1;
    for (int j = min(nwords, maxWords); j < maxWords; ++j) wrd[j] = -1;
    wordCounts[row] = live ? nwords : -1;
  }
  lengths[row] = live ? len : -1;
  scores[row] = live ? sScore[src] : -INFINITY;
  if (lmScores) lmScores[row] = live ? sAcc[src] : -INFINITY;
}

template <bool kLex>
__global__ __launch_bounds__(kWideThreads) void beam_wide_finish(int M, int Lmax, int maxWords, int eosWord, BeamWideWs ww,
                                                                 const void* __restrict__ lex, const void* __restrict__ lm,
                                                                 float lmWeight, float eosScore, int useEos,
                                                                 int* __restrict__ labels, int* __restrict__ lengths,
                                                                 float* __restrict__ scores, float* __restrict__ lmScores,
                                                                 int* __restrict__ words, int* __restrict__ wordCounts) {
  beam_wide_finish_body<kLex>(blockIdx.x, ww.c.finN[blockIdx.x], BeamWalk{}, M, Lmax, maxWords, eosWord, ww, lex, lm, lmWeight,
                              eosScore, useEos, labels, lengths, scores, lmScores, words, wordCounts);
}

template <bool kLogAdd, class Pol, bool kLex, bool kTok = false>
static int beam_wide_launch(int B, int T, int N, float threshold, const float* input, const int* frames, const BeamWideWs& ww,
                            const void* lex, const void* lm, float lmWeight, const float* classScore, float wordScore,
                            const BeamTrans& tr, size_t transBytes, hipStream_t s) {
  const size_t shmem = align_up(transBytes, 16) + WideLds<kLex>::bytes;
  static bool attr[64] = {};
  if (first_on_device(attr))
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)beam_wide_scan<kLogAdd, Pol, kLex, kTok>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(align_up(kWideTransLds, 16) + WideLds<kLex>::bytes)));
  hipLaunchKernelGGL((beam_wide_scan<kLogAdd, Pol, kLex, kTok>), dim3((unsigned)B), dim3(kWideThreads), shmem, s, T, N, ww.W, threshold,
                     input, frames, ww, lex, lm, lmWeight, classScore, wordScore, tr);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

// One wide search after its checks: rows, scan, finish.  K: the clipped beamToken.  kSearchLextok: lm is a token LM under the
// lexicon (criterion_beam_lextok.hpp)
static int beam_wide_run(const BeamReq& q, int K) {
  const bool tok = q.kind == kSearchLextok;
  const int N = q.N;
  BeamWideWs ww{};
  beam_wide_layout(&ww, q.workspace, q.B, q.T, q.beam, K, q.lex() ? kBeamLex : kBeamLm);
  if (const int rc = beam_rows_launch(q, &ww.c)) return rc;

  const size_t transBytes = q.asg && (size_t)N * N * sizeof(float) <= kWideTransLds ? (size_t)N * N * sizeof(float) : 0;
  const BeamTrans tr{q.trans, transBytes ? 1 : 0};
  const int rc = beam_scan_dispatch(q.logAdd, q.asg, q.lex(), [&](auto la, auto pol, auto lx) {
    constexpr bool kLa = decltype(la)::value, kLex = decltype(lx)::value;
    using Pol = decltype(pol);
    if constexpr (kLex)
      if (tok)
        return beam_wide_launch<kLa, Pol, true, true>(q.B, q.T, N, q.threshold, q.input, q.frames, ww, q.lexicon, q.lm, q.lmWeight,
                                                      nullptr, q.wordScore, tr, transBytes, q.stream);
    return beam_wide_launch<kLa, Pol, kLex>(q.B, q.T, N, q.threshold, q.input, q.frames, ww, q.lexicon, q.lm, q.lmWeight, q.classScore,
                                            q.wordScore, tr, transBytes, q.stream);
  });
  if (rc) return rc;
  const int useEos = q.lm && q.lmHasEos ? 1 : 0;
  const dim3 grid((unsigned)q.B), threads(kWideThreads);
  if (q.lex())
    hipLaunchKernelGGL(beam_wide_finish<true>, grid, threads, 0, q.stream, q.nbest, q.maxLen, q.maxWords, 0, ww, q.lexicon, q.lm,
                       q.lmWeight, q.eosScore, useEos, q.labels, q.lengths, q.scores, q.lmScores, q.words, q.wordCounts);
  else
    hipLaunchKernelGGL(beam_wide_finish<false>, grid, threads, 0, q.stream, q.nbest, q.maxLen, 0, q.asg ? N + 1 : N, ww, nullptr, q.lm,
                       q.lmWeight, q.eosScore, useEos, q.labels, q.lengths, q.scores, q.lmScores, nullptr, nullptr);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

}  // namespace w2l
