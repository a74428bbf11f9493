// criterion_beam_xl.hpp -- the five xl beam searches (w2l_*_beam_search*_xl): the contracts of the CTC and ASG beam searches
// (include/w2l_hip.h) with a beam of up to kBeamXlMax = 8192 entries, the widths the reference's recipes ask for (1500, 2500, 5000,
// 8000).  Included at the end of criterion_ctc.hip.  The algorithm is criterion_beam_wide.hpp's, frame by frame and operation by
// operation -- stays with the merged extension, the candidate list of 64-bit keys, the MSB-first radix select, the sorted survivors,
// the next beam -- on the same device helpers (ctc_beam_rows, beam_node, beam_key, beam_oplus, BeamCtc / BeamAsg, beam_lm_ext,
// beam_lex_a, beam_lex_word, beam_eos, beam_chain_len, beam_write_labels), so at every W both families take the outputs are the
// same bits.  What differs is where the state lives and who owns it:
//   ownership   one workgroup of 1024 threads per utterance; thread tid owns entries tid, tid + 1024, ... of the beam.
//   the beam    both halves, 8 fields of 4 bytes per entry (9 with a lexicon), [2][kFields][W] words per utterance in the
//               WORKSPACE, with the gone masks ([slots][W] u64) and pb' / pnb' of the stays ([2][W] float).  At W = 8192 that is
//               0.6 - 1.1 MiB per utterance: L2-resident.  It is written with plain stores and read with plain loads after a
//               __syncthreads(), as the wide scan's candidate list is: one workgroup, one CU, one L1.  The gone masks are the
//               exception: they are set by 64-bit global atomics, which act at L2, so they are read back with device-scope atomic
//               loads, which go there too.
//   LDS         the node -> rank hash, 2 * pow2(W) slots of 8 bytes (128 KiB at W = 8192; dynamic LDS, one workgroup per CU).  It
//               is dead once the stays are done, and the survivors' sort (pow2(m) <= pow2(W) keys: half of it) takes its place,
//               as the wide scan reuses its sScr.  The frame tokens, the histogram and the counters are 2 KiB more.  The ASG
//               transition matrix is not staged: it is gathered from global memory (BeamTrans.lds = 0), the whole budget is the
//               hash's.
//   atomics     hash CAS, histogram and counters: LDS atomics; gone masks: global 64-bit OR; prefix table: beam_node's global CAS.
//   sort        bitonic over pow2(m) keys, n2 / 2 compare-exchanges a step, strided over the threads.
// No waiting between workgroups, no flags, no spin loops; every probe loop is bounded by its table's capacity; every barrier is
// reached by all 1024 threads, and every loop with a barrier inside runs on counts read from LDS after a barrier, the same in
// every thread.
//   kMt                  the many-token searches (w2l_*_beam_search*_mt) are this scan with K up
//                        to kBeamMtMax = 256: 256 LDS slots of frame tokens, gone masks of ceil(K / 64) words per (slot, entry),
//                        a tie key with 8 bits of k.  Every difference is an `if constexpr (kMt)`; !kMt is the xl scan, whose
//                        instructions must not change.
//   kResume, kOpen       the many-token beam session (criterion_beam_stream.hpp) is this scan with kMt and kResume and
//                        this finish with kOpen, a BeamXlCarry behind their arguments (a parameter pack, empty for a whole search:
//                        the whole searches' kernels keep their argument lists and their instructions).
//   beam_xl_finish<lex>  one workgroup per utterance, strided over the final entries and then over the output rows; keys, scores
//                        and LM sums in dynamic LDS (16 bytes per entry of pow2(W)).
#pragma once

namespace w2l {

constexpr int kBeamXlMax = 8192;      // W of the xl searches; their K stays <= kBeamMax
constexpr int kBeamMtMax = 256;       // K of the many-token searches (beam_xl_run with mt): this scan with kMt, W as here
constexpr int kXlThreads = 1024;

struct BeamXlWs {
  BeamWideWs w;      // the wide family's workspace: rows, table, candidate list, fin* (W entries per utterance)
  int* beam;         // [B][2][kFields][W]
  u64* gone;         // [B][slots][W]; the many-token scan: [B][slots][W][ceil(K / 64)]
  float* stay;       // [B][2][W]: pb', pnb' of stay(j)
  int hashN;         // 2 * pow2(W): slots of the LDS hash
};

__host__ __device__ __forceinline__ int beam_xl_pow2(int m) {
  int n2 = 2;
  while (n2 < m) n2 <<= 1;
  return n2;
}

// words of a gone mask: one bit per frame token
__host__ __device__ __forceinline__ int beam_mt_words(int K) { return (K + 63) >> 6; }

static size_t beam_xl_layout(BeamXlWs* x, void* ws, int B, int T, int W, int K, int variant, bool mt = false) {
  const bool lex = variant == kBeamLex;
  const size_t words = mt ? (size_t)beam_mt_words(K) : 1;
  char* p = (char*)ws;
  char* const p0 = p;
  p += align_up(beam_wide_layout(x ? &x->w : nullptr, ws, B, T, W, K, variant), 256);
  int* beam = (int*)p; p += align_up((size_t)B * 2 * (lex ? 9 : 8) * W * 4, 256);
  u64* gone = (u64*)p; p += align_up((size_t)B * (lex ? 7 : 1) * W * words * 8, 256);
  float* stay = (float*)p; p += align_up((size_t)B * 2 * W * 4, 256);
  if (x) { x->beam = beam; x->gone = gone; x->stay = stay; x->hashN = 2 * beam_xl_pow2(W); }
  return (size_t)(p - p0);
}

// the dynamic LDS of beam_xl_scan after the hash (hashN u64), in bytes; kTok: the frame tokens it holds
template <int kTok>
struct XlLdsT {
  static constexpr size_t tc = 0;                     // [kTok] int
  static constexpr size_t tl = tc + kTok * 4;         // [kTok] float
  static constexpr size_t hist = tl + kTok * 4;       // [256] unsigned
  static constexpr size_t red = hist + 256 * 4;       // [16] u64
  static constexpr size_t misc = red + 16 * 8;        // [8] unsigned
  static constexpr size_t bytes = misc + 8 * 4;
};
using XlLds = XlLdsT<kBeamMax>;
using MtLds = XlLdsT<kBeamMtMax>;

// s[0 .. n2) descending, n2 a power of two <= 8192; every thread of the workgroup calls it; ends with a barrier
__device__ __forceinline__ void beam_xl_sort(u64* s, int n2) {
  const int half = n2 >> 1;
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = threadIdx.x; p < half; p += kXlThreads) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), o = i | j;
        const u64 a = s[i], c = s[o];
        const bool desc = (i & k) == 0;
        if (desc ? a < c : a > c) { s[i] = c; s[o] = a; }
      }
      __syncthreads();
    }
}

// a gone mask as the atomics at L2 left it
__device__ __forceinline__ u64 beam_xl_mask(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- what the many-token scan (kMt: K <= kBeamMtMax) does differently; !kMt is the xl scan as it was
// The selection key with 8 bits of k: total, then ~(r << 12 | ext << 11 | k << 3 | slot), 25 bits for r < 8192: beam_key's order.
template <bool kMt>
__device__ __forceinline__ u64 beam_xl_key(float total, int r, int ext, int k, int slot = 0) {
  if constexpr (!kMt) return beam_key(total, r, ext, k, slot);
  else return ((u64)beam_ord(total) << 32) | (u64)(0xffffffffu - (unsigned)((r << 12) | (ext << 11) | (k << 3) | slot));
}
// the gone-mask word of (slot, entry r) that holds token k's bit, and the bit; mw: words per mask (1 when !kMt)
template <bool kMt>
__device__ __forceinline__ u64* beam_xl_gone(u64* gGone, int slot, int W, int r, int k, int mw) {
  if constexpr (!kMt) return &gGone[(size_t)slot * W + r];
  else return &gGone[((size_t)slot * W + r) * mw + (k >> 6)];
}
template <bool kMt>
__device__ __forceinline__ u64 beam_xl_bit(int k) { return 1ull << (kMt ? (k & 63) : k); }
// the frame tokens of `row`: beam_load_frame with kBeamMtMax slots
__device__ __forceinline__ void beam_mt_load_frame(const CtcBeamWs& ws, size_t row, int* sTc, float* sTl) {
  const int tid = threadIdx.x, K = ws.K;
  if (tid < kBeamMtMax) {
    sTc[tid] = tid < K ? ws.tokC[row * K + tid] : -2;
    sTl[tid] = tid < K ? ws.tokLp[row * K + tid] : -INFINITY;
  }
}

// ---- an xl beam that outlives the launch (the many-token beam session of criterion_beam_stream.hpp; kResume below)
// Both halves of the beam already live in memory, so a slot's stored beam IS its halves: what a resume adds is which half is
// current and how many entries it has.  cnt[slot]: the slot's frames of this step; flag[slot] bit 0: it starts from the empty
// prefix, bit 1 (the finish): it is open; curn[slot]: (cur, n).  (cnt is followed by the slots' frame indices,
// ctc_beam_rows<., ., true>'s.)
struct BeamXlCarry {
  const int *cnt, *flag;
  int* curn;   // [S][2]
};
template <class C>
__device__ __forceinline__ const C& beam_xl_carry(const C& c) { return c; }

// kResume, with one more kernel argument, a BeamXlCarry (the pack Cy; a whole search has none, and its kernel is what it was before
// there was a kResume, instruction for instruction): utterance b is a slot of a many-token beam session: its frame count (0: none)
// and start flag come from cy.cnt / cy.flag -- the same in every thread, read before the first barrier, so the workgroup leaves or
// stays as one --, cur and n from cy.curn unless the slot starts, and both go back there after the frames: they wait in memory, not
// in scalars of their own across the frame loop.  What indexes memory is held to its range before the first frame (n
// to W, node ids to the table, the last token to the row: thread j mends the entries it owns in place, the first frame's barrier
// publishes them); LM states and lexicon nodes are clamped where they are used (ngram_q, lex_child, lex_node).
template <bool kLogAdd, class Pol, bool kLex, bool kMt = false, bool kResume = false, class... Cy>
__global__ __launch_bounds__(kXlThreads) void beam_xl_scan(int T, int N, int W, float threshold, const float* __restrict__ x,
                                                           const int* __restrict__ frames, BeamXlWs xw,
                                                           const void* __restrict__ lex, const void* __restrict__ lm,
                                                           float lmWeight, const float* __restrict__ classScore, float wordScore,
                                                           BeamTrans tr, Cy... cy) {
  constexpr int kF = kLex ? 9 : 8, kSlots = kLex ? 7 : 1, kTh = kXlThreads;
  using Lds = XlLdsT<kMt ? kBeamMtMax : kBeamMax>;
  extern __shared__ float sAsgTrans[];   // BeamAsg::stage's array; nothing is staged here (tr.lds = 0)
  const int hashN = xw.hashN;
  u64* const sHash = (u64*)sAsgTrans;
  u64* const sSort = sHash;               // the survivors' keys, once the hash is dead
  char* const base = (char*)(sHash + hashN);
  int* const sTc = (int*)(base + Lds::tc);
  float* const sTl = (float*)(base + Lds::tl);
  unsigned* const sHist = (unsigned*)(base + Lds::hist);
  u64* const sRed = (u64*)(base + Lds::red);
  unsigned* const sMisc = (unsigned*)(base + Lds::misc);   // 0: candidates, 1: survivors, 2: bin, 3: keys above it, 4: keys in it,
                                                             // 5, 6: the silence class and score (below)

  const BeamWideWs& ww = xw.w;
  const CtcBeamWs& ws = ww.c;
  const int b = blockIdx.x, tid = threadIdx.x, K = ws.K;
  int F0;
  bool fresh = true;
  if constexpr (kResume) {
    const BeamXlCarry& c = beam_xl_carry(cy...);
    F0 = min(max(c.cnt[b], 0), T);
    fresh = (c.flag[b] & 1) != 0;
    if (F0 == 0 && !fresh) return;   // the whole workgroup, before any barrier
  } else {
    F0 = align_frames(frames, b, T);
  }
  const int F = F0;
  const float* xb = x + (size_t)b * T * N;
  u64* tab = ws.table + (size_t)b * ws.cap;
  const unsigned capm = ws.cap - 1;
  const unsigned hm = (unsigned)hashN - 1u;
  const size_t row0 = (size_t)b * T;
  u64* cand = ww.cand + (size_t)b * ww.candCap;
  const unsigned candCap = (unsigned)ww.candCap;
  int* const gBeam = xw.beam + (size_t)b * 2 * kF * W;
  const int mw = kMt ? beam_mt_words(K) : 1;   // words per gone mask
  u64* const gGone = xw.gone + (size_t)b * kSlots * W * mw;
  float* const gSpb = xw.stay + (size_t)b * 2 * W;
  float* const gSpnb = gSpb + W;
  const bool useLm = kLex || lm != nullptr;
  const NgramView lv = useLm ? ngram_view(lm) : NgramView{};
  LexView xv{};
  if constexpr (kLex) xv = lex_view(lex);
  const float* A = Pol::stage(tr, N);

  // field f of half h of the beam: 0 node, 1 parent's node, 2 last token, 3 LM state, 4 pb, 5 pnb, 6 tot, 7 unweighted LM sum,
  // 8 (lexicon) the label of the last extension
  auto fi = [&](int h, int f) { return gBeam + ((size_t)h * kF + f) * W; };
  auto ff = [&](int h, int f) { return (float*)(gBeam + ((size_t)h * kF + f) * W); };

  int cur = 0, n = 1;
  if constexpr (kResume) {
    if (!fresh) {
      const BeamXlCarry& c = beam_xl_carry(cy...);
      cur = c.curn[2 * b] & 1;
      n = min(max(c.curn[2 * b + 1], 0), W);
      for (int j = tid; j < n; j += kTh) {
        const int node = fi(cur, 0)[j], e = fi(cur, 2)[j];
        if ((unsigned)node > ws.cap) fi(cur, 0)[j] = 0;
        if (e < -1 || e >= N - 1) fi(cur, 2)[j] = -1;
      }
    }
  }
  if (tid == 0) {
    // The silence class and score wait in LDS for the stays, which read them where they use them.  As two more scalar kernel
    // arguments alive across the frame loop they cost this kernel, which stands at its scalar-register limit, more spilled scalars
    // in the loop (3 to 5 % of a CTC search at W = 1024).  The first frame's barrier publishes them.
    sMisc[5] = (unsigned)ws.sil; sMisc[6] = __float_as_uint(ws.silScore);
    if (!kResume || fresh) {
      fi(0, 0)[0] = 0; fi(0, 1)[0] = -1; fi(0, 2)[0] = -1; fi(0, 3)[0] = useLm ? (int)((const NgramHeader*)lm)->start : 0;
      ff(0, 4)[0] = 0.f; ff(0, 5)[0] = -INFINITY; ff(0, 6)[0] = 0.f; ff(0, 7)[0] = 0.f;
      if constexpr (kLex) fi(0, 8)[0] = -1;
    }
  }
  for (int t = 0; t < F && n > 0; ++t) {
    const size_t row = row0 + t;
    const int nxt = cur ^ 1;
    const int *cNode = fi(cur, 0), *cPar = fi(cur, 1), *cE = fi(cur, 2), *cSt = fi(cur, 3);
    const float *cPb = ff(cur, 4), *cPnb = ff(cur, 5), *cTot = ff(cur, 6), *cAcc = ff(cur, 7);
    const int* cLab = kLex ? fi(cur, 8) : nullptr;

    if constexpr (kMt) beam_mt_load_frame(ws, row, sTc, sTl);
    else beam_load_frame(ws, row, sTc, sTl);
    if constexpr (kMt) {
      for (int i = tid; i < n * mw; i += kTh)
        for (int s = 0; s < kSlots; ++s) gGone[(size_t)s * W * mw + i] = 0ull;
    } else {
      for (int j = tid; j < n; j += kTh)
        for (int s = 0; s < kSlots; ++s) gGone[(size_t)s * W + j] = 0ull;
    }
    for (int i = tid; i < hashN; i += kTh) sHash[i] = 0ull;
    if (tid < 2) sMisc[tid] = 0u;
    const float lpb = ws.lpb[row], lse = ws.lse[row];
    __syncthreads();
    // the rank of every current node
    for (int j = tid; j < n; j += kTh) {
      const unsigned nd1 = (unsigned)cNode[j] + 1u;
      const u64 rec = ((u64)nd1 << 32) | (u64)(unsigned)j;
      unsigned h = beam_hash(nd1) & hm;
      for (int probe = 0; probe < hashN; ++probe) {
        if (atomicCAS(&sHash[h], 0ull, rec) == 0ull) break;
        h = (h + 1) & hm;
      }
    }
    __syncthreads();

    // every candidate of the frame that is not -inf: its key into the list
    u64 local = 0ull;
    auto put = [&](u64 key) {
      if ((unsigned)(key >> 32) == beam_ord(-INFINITY)) return;
      const unsigned pos = atomicAdd(&sMisc[0], 1u);
      if (pos < candCap) cand[pos] = key;
      local = key > local ? key : local;
    };
    // stay(j), with the extension that spells this entry merged in
    for (int j = tid; j < n; j += kTh) {
      float spb = -INFINITY, spnb = -INFINITY;
      const int e = cE[j], par = cPar[j];
      int kj = -1, pr = -1;
      for (int k = 0; k < K; ++k) kj = sTc[k] == e ? k : kj;
      if (par >= 0) {
        const unsigned pd1 = (unsigned)par + 1u;
        unsigned h = beam_hash(pd1) & hm;
        for (int probe = 0; probe < hashN; ++probe) {
          const u64 rec = sHash[h];
          if (rec == 0ull) break;
          if ((unsigned)(rec >> 32) == pd1) { pr = (int)(unsigned)rec; break; }
          h = (h + 1) & hm;
        }
      }
      Pol::stay(e >= 0 ? beam_sil_lp(xb[(size_t)t * N + e] - lse, e, (int)sMisc[5], __uint_as_float(sMisc[6])) : 0.f, e, lpb, cPnb[j],
                cTot[j], A, N, &spb, &spnb);
      if (pr >= 0 && kj >= 0) {
        float v = Pol::ext(sTl[kj], e, cE[pr], cPb[pr], cTot[pr], A, N);
        if constexpr (!kLex) {
          if (useLm) {
            int unused;
            const float qm = ngram_q(lv, cSt[pr], e, &unused);
            v = beam_lm_ext(v, lmWeight, qm, classScore, e);
          }
          spnb = beam_oplus<kLogAdd>(spnb, v);
          atomicOr(beam_xl_gone<kMt>(gGone, 0, W, pr, kj, mw), beam_xl_bit<kMt>(kj));
        } else {
          const int lab = cLab[j];
          if (lab >= 0) {
            const int vj = lab >> 3, slot = lab & 7;
            if (vj != 0) {
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
            atomicOr(beam_xl_gone<kMt>(gGone, min(slot, 6), W, pr, kj, mw), beam_xl_bit<kMt>(kj));
          }
        }
      }
      gSpb[j] = spb; gSpnb[j] = spnb;
      put(beam_xl_key<kMt>(beam_oplus<kLogAdd>(spb, spnb), j, 0, 0));
    }
    __syncthreads();   // the hash is read, the gone masks are complete

    // is the extension of entry r by frame token k gone in `slot`?
    auto gone = [&](int slot, int r, int k) -> bool {
      if constexpr (kMt) return (beam_xl_mask(beam_xl_gone<true>(gGone, slot, W, r, k, mw)) >> (k & 63)) & 1ull;
      else return (beam_xl_mask(&gGone[(size_t)slot * W + r]) >> k) & 1ull;
    };
    const int total = n * K;
    for (int idx = tid; idx < total; idx += kTh) {
      const int r = idx / K, k = idx - r * K, c = sTc[k], e = cE[r];
      if (Pol::none(c, e)) continue;
      const float a0 = Pol::ext(sTl[k], c, e, cPb[r], cTot[r], A, N);
      if constexpr (!kLex) {
        if (gone(0, r, k)) continue;
        float v = a0;
        if (useLm) {
          int unused;
          const float q = ngram_q(lv, cSt[r], c, &unused);
          v = beam_lm_ext(v, lmWeight, q, classScore, c);
        }
        put(beam_xl_key<kMt>(v, r, 1, k));
      } else {
        const int u = beam_wide_u(cLab[r]);
        if (c == xv.silToken && u == 0) {
          if (!gone(0, r, k)) put(beam_xl_key<kMt>(a0, r, 1, k, 0));
        } else {
          const int v = lex_child(xv, u, c);
          if (v > 0) {
            const LexNode& nd = lex_node(xv, v);
            const float smv = nd.smear;
            const float a = beam_lex_a(a0, lmWeight, smv, u == 0 ? 0.f : lex_node(xv, u).smear);
            if (lex_has_children(nd) && !gone(0, r, k)) put(beam_xl_key<kMt>(a, r, 1, k, 0));
            const int nw = lex_nw(nd);
            for (int i = 0; i < nw; ++i)
              if (!gone(1 + i, r, k)) {
                int unused;
                const float q = ngram_q(lv, cSt[r], nd.words[i], &unused);
                put(beam_xl_key<kMt>(beam_lex_word(a, lmWeight, q, smv, wordScore), r, 1, k, 1 + i));
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
        if (pos < (unsigned)W) sSort[pos] = key;
      }
    }
    __syncthreads();
    const int m = (int)min(sMisc[1], (unsigned)W);
    const int n2 = beam_xl_pow2(m);
    for (int i = m + tid; i < n2; i += kTh) sSort[i] = 0ull;
    __syncthreads();
    beam_xl_sort(sSort, n2);

    // entry q of the next beam
    for (int q = tid; q < m; q += kTh) {
      const u64 key = sSort[q];
      const unsigned tie = 0xffffffffu - (unsigned)key;
      const int r = min((int)(tie >> (kMt ? 12 : 10)), W - 1), ext = (int)((tie >> (kMt ? 11 : 9)) & 1u),
                k = (int)((tie >> 3) & (kMt ? 255u : 63u)), slot = (int)(tie & 7u);
      if (!ext) {
        const float pb = gSpb[r], pnb = gSpnb[r];
        fi(nxt, 0)[q] = cNode[r]; fi(nxt, 1)[q] = cPar[r]; fi(nxt, 2)[q] = cE[r]; fi(nxt, 3)[q] = cSt[r];
        ff(nxt, 4)[q] = pb; ff(nxt, 5)[q] = pnb; ff(nxt, 6)[q] = beam_oplus<kLogAdd>(pb, pnb); ff(nxt, 7)[q] = cAcc[r];
        if constexpr (kLex) fi(nxt, 8)[q] = cLab[r];
      } else {
        const float tot = beam_unord((unsigned)(key >> 32));
        const int c = sTc[k];
        int st = cSt[r], label = c;
        float acc = cAcc[r];
        if constexpr (!kLex) {
          st = 0;
          float q1 = 0.f;
          if (useLm) q1 = ngram_q(lv, cSt[r], c, &st);
          acc = acc + q1;
        } else {
          const int u = beam_wide_u(cLab[r]);
          const int v = (c == xv.silToken && u == 0) ? 0 : max(lex_child(xv, u, c), 0);
          label = (v << 3) | slot;
          if (slot > 0) {
            const float q1 = ngram_q(lv, cSt[r], lex_node(xv, v).words[min(slot - 1, kLexMaxWords - 1)], &st);
            acc = acc + q1;
          }
          fi(nxt, 8)[q] = label;
        }
        const int par = cNode[r];
        fi(nxt, 0)[q] = beam_node(tab, capm, par, label);   // a new prefix
        fi(nxt, 1)[q] = par; fi(nxt, 2)[q] = c; fi(nxt, 3)[q] = st;
        ff(nxt, 4)[q] = -INFINITY; ff(nxt, 5)[q] = tot; ff(nxt, 6)[q] = tot; ff(nxt, 7)[q] = acc;
      }
    }
    __syncthreads();
    n = m;
    cur = nxt;
  }
  // the final entries (the barrier above, or none before a first frame that never ran: then thread 0 reads its own entry 0)
  for (int j = tid; j < W; j += kTh) {
    const bool live = j < n;
    const size_t o = (size_t)b * ww.W + j;
    ws.finNode[o] = live ? fi(cur, 0)[j] : -1;
    ws.finTot[o] = live ? ff(cur, 6)[j] : -INFINITY;
    ws.finState[o] = live ? fi(cur, 3)[j] : 0;
    ws.finAcc[o] = live ? ff(cur, 7)[j] : -INFINITY;
    if constexpr (kLex) ws.finU[o] = live ? beam_wide_u(fi(cur, 8)[j]) : -1;
  }
  if (tid == 0) ws.finN[b] = n;
  if constexpr (kResume) {
    if (tid == 0) {
      const BeamXlCarry& c = beam_xl_carry(cy...);
      c.curn[2 * b] = cur; c.curn[2 * b + 1] = n;
    }
  }
}

// beam_wide_finish with thread r owning final entries r, r + 1024, ... and rows m, m + 1024, ...; dynamic LDS: pow2(W) keys, then
// W scores, W LM sums and the count of the entries that count at the end
// kOpen, with one more kernel argument, a BeamXlCarry (the many-token beam session's result): cy.flag[slot] bit 1 says the slot is
// open -- a closed or never started slot has no entries: empty rows --, cy.cnt[slot] is the frames it has had (no prefix is longer)
// and bounds the walks up the table with the table's size.  A whole search's kernel is what it was before there was a kOpen.
template <bool kLex, bool kOpen = false, class... Cy>
__global__ __launch_bounds__(kXlThreads) void beam_xl_finish(int M, int Lmax, int maxWords, int eosWord, BeamXlWs xw,
                                                             const void* __restrict__ lex, const void* __restrict__ lm,
                                                             float lmWeight, float eosScore, int useEos,
                                                             int* __restrict__ labels, int* __restrict__ lengths,
                                                             float* __restrict__ scores, float* __restrict__ lmScores,
                                                             int* __restrict__ words, int* __restrict__ wordCounts, Cy... cy) {
  extern __shared__ float sAsgTrans[];   // the only LDS of the kernel: the keys come first, 8-byte aligned at offset 0
  const BeamWideWs& ww = xw.w;
  const CtcBeamWs& ws = ww.c;
  const int b = blockIdx.x, tid = threadIdx.x, W = ww.W;
  int n0 = min(max(ws.finN[b], 0), W);
  if constexpr (kOpen) {
    if (!(beam_xl_carry(cy...).flag[b] & 2)) n0 = 0;
  }
  const int n = n0;
  const int n2 = beam_xl_pow2(n);
  u64* const sKey = (u64*)sAsgTrans;
  float* const sScore = (float*)(sKey + beam_xl_pow2(W));
  float* const sAcc = sScore + W;
  unsigned* const sAlive = (unsigned*)(sAcc + W);
  const u64* tab = ws.table + (size_t)b * ws.cap;
  BeamWalk g0{};
  if constexpr (kOpen) {
    g0.capm = ws.cap - 1;
    g0.steps = max(beam_xl_carry(cy...).cnt[b], 0);
  }
  const BeamWalk g = g0;
  if (tid == 0) *sAlive = 0u;
  __syncthreads();
  unsigned mine = 0u;
  for (int r = tid; r < n2; r += kXlThreads) {
    const size_t o = (size_t)b * W + min(r, W - 1);
    const bool alive = r < n && (!kLex || ws.finU[o] == 0);   // with a lexicon only finished words count at the end
    float score = -INFINITY, acc = -INFINITY;
    if (alive) {
      score = ws.finTot[o];
      acc = ws.finAcc[o];
      if (useEos) {
        const int ew = kLex ? (int)((const NgramHeader*)lm)->numTokens + 1 : eosWord;
        beam_eos(lm, ws.finState[o], ew, lmWeight, eosScore, &score, &acc);
      }
      ++mine;
    }
    if (r < W) { sScore[r] = score; sAcc[r] = acc; }
    sKey[r] = alive ? ((u64)beam_ord(score) << 32) | (u64)(0xffffffffu - (unsigned)r) : 0ull;
  }
  if (mine) atomicAdd(sAlive, mine);
  __syncthreads();
  const int nAlive = (int)*sAlive;
  beam_xl_sort(sKey, n2);
  for (int m = tid; m < M; m += kXlThreads) {
    const bool live = m < nAlive;
    const int src = live ? min((int)(0xffffffffu - (unsigned)sKey[m]), W - 1) : 0;
    const size_t row = (size_t)b * M + m;
    int* lab = labels + row * Lmax;
    int len = 0, nwords = 0;
    if constexpr (!kLex) {
      len = beam_write_labels(tab, live, ws.finNode + (size_t)b * W + src, Lmax, lab, g);
    } else {
      const LexView xv = lex_view(lex);
      int* wrd = words + row * maxWords;
      if (live) {
        const int node = ws.finNode[(size_t)b * W + src];
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
}

constexpr size_t kXlScanLdsMax = (size_t)2 * kBeamXlMax * 8 + XlLds::bytes;   // 128 KiB + 2 KiB
constexpr size_t kMtScanLdsMax = (size_t)2 * kBeamXlMax * 8 + MtLds::bytes;   // 128 KiB + 3.2 KiB
constexpr size_t kXlFinishLdsMax = (size_t)kBeamXlMax * 16 + 8;               // 128 KiB
static_assert(kMtScanLdsMax <= 160 * 1024, "the many-token scan's hash and frame state must fit the CU's LDS");

template <bool kLogAdd, class Pol, bool kLex, bool kMt = false>
static int beam_xl_launch(int B, int T, int N, float threshold, const float* input, const int* frames, const BeamXlWs& xw,
                          const void* lex, const void* lm, float lmWeight, const float* classScore, float wordScore,
                          const BeamTrans& tr, hipStream_t s) {
  const size_t shmem = (size_t)xw.hashN * 8 + (kMt ? MtLds::bytes : XlLds::bytes);
  static bool attr[64] = {};
  if (first_on_device(attr))
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)beam_xl_scan<kLogAdd, Pol, kLex, kMt>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(kMt ? kMtScanLdsMax : kXlScanLdsMax)));
  hipLaunchKernelGGL((beam_xl_scan<kLogAdd, Pol, kLex, kMt>), dim3((unsigned)B), dim3(kXlThreads), shmem, s, T, N, xw.w.W, threshold,
                     input, frames, xw, lex, lm, lmWeight, classScore, wordScore, tr);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

template <bool kLex>
static int beam_xl_finish_launch(int B, int M, int Lmax, int maxWords, int eosWord, const BeamXlWs& xw, const void* lex,
                                 const void* lm, float lmWeight, float eosScore, int useEos, int* labels, int* lengths, float* scores,
                                 float* lmScores, int* words, int* wordCounts, hipStream_t s) {
  const size_t shmem = (size_t)beam_xl_pow2(xw.w.W) * 8 + (size_t)xw.w.W * 8 + 8;
  static bool attr[64] = {};
  if (first_on_device(attr))
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)beam_xl_finish<kLex>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)kXlFinishLdsMax));
  hipLaunchKernelGGL(beam_xl_finish<kLex>, dim3((unsigned)B), dim3(kXlThreads), shmem, s, M, Lmax, maxWords, eosWord, xw, lex, lm,
                     lmWeight, eosScore, useEos, labels, lengths, scores, lmScores, words, wordCounts);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

// One xl search after its checks: rows, scan, finish.  K: the clipped beamToken; mt: the many-token scan
static int beam_xl_run(const BeamReq& q, int K, bool mt) {
  BeamXlWs xw{};
  beam_xl_layout(&xw, q.workspace, q.B, q.T, q.beam, K, q.lex() ? kBeamLex : kBeamLm, mt);
  if (const int rc = beam_rows_launch(q, &xw.w.c)) return rc;

  const BeamTrans tr{q.trans, 0};   // gathered from global memory: the LDS is the hash's
  const int rc = beam_scan_dispatch(q.logAdd, q.asg, q.lex(), [&](auto la, auto pol, auto lx) {
    constexpr bool kLa = decltype(la)::value, kLex = decltype(lx)::value;
    using Pol = decltype(pol);
    if (mt)
      return beam_xl_launch<kLa, Pol, kLex, true>(q.B, q.T, q.N, q.threshold, q.input, q.frames, xw, q.lexicon, q.lm, q.lmWeight,
                                                  q.classScore, q.wordScore, tr, q.stream);
    return beam_xl_launch<kLa, Pol, kLex>(q.B, q.T, q.N, q.threshold, q.input, q.frames, xw, q.lexicon, q.lm, q.lmWeight, q.classScore,
                                          q.wordScore, tr, q.stream);
  });
  if (rc) return rc;
  const int useEos = q.lm && q.lmHasEos ? 1 : 0;
  if (q.lex())
    return beam_xl_finish_launch<true>(q.B, q.nbest, q.maxLen, q.maxWords, 0, xw, q.lexicon, q.lm, q.lmWeight, q.eosScore, useEos,
                                       q.labels, q.lengths, q.scores, q.lmScores, q.words, q.wordCounts, q.stream);
  return beam_xl_finish_launch<false>(q.B, q.nbest, q.maxLen, 0, q.asg ? q.N + 1 : q.N, xw, nullptr, q.lm, q.lmWeight, q.eosScore,
                                      useEos, q.labels, q.lengths, q.scores, q.lmScores, nullptr, nullptr, q.stream);
}

}  // namespace w2l
