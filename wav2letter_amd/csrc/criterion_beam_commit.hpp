// criterion_beam_commit.hpp -- w2l_beam_session_commit: the stable prefix of a beam session's slot handed out, its prefix table
// rebuilt with the nodes that live entries still descend from (contract: include/w2l_hip.h).  Included after
// criterion_beam_stream.hpp, whose sessions (narrow, wide, and many-token up to a beam of 1024) it works on.
// A slot's stored beam is n entries, each at a node of the slot's prefix table.  The deepest node C that is an ancestor-or-self of
// every entry's node spells what no later frame can change: every hypothesis the search will ever return descends from an entry of
// today.  The new root is C's PARENT: C's own label stays in the table, so no live entry sits at node 0 with a real last label, a
// state the scans never see.  Node ids are hash slots and no decision or output depends on them (the session's contract), so the
// rebuilt table, with other ids for the same prefixes, continues the same search bit for bit.
// Per flagged slot, in stream order, against ONE slot's worth of scratch:
//   clear   the scratch table (a memset)
//   walk    beam_commit_walk, ONE workgroup, thread j = entry j (256 threads for a narrow session: 64 entries, and the label padding
//           strides; 1024 for a wide or many-token one: an entry per thread): depths, the cut (the entries level their
//           nodes to the smallest depth, then step up together until all stand on one node), the committed labels and words in
//           root-to-cut order, or the refusal when they do not fit (nothing of the slot changed); then every entry re-inserts its
//           chain below the new root top-down into the scratch table with beam_node (find-or-make: entries that share an ancestor
//           agree on its new id) and rewrites its node and parent ids.
//   copy    beam_commit_copy, a bandwidth pass of many workgroups: the scratch table over the slot's table, counting its nodes
//           (`live`); skipped by a slot that was refused.
// An entry's chain goes up through a stack of maxFrames labels in scratch ([maxFrames][entries], entry-minor).  A chain may be
// longer than that (an entry deep under a cut that is itself an entry, carried over several commits): it is then inserted in
// rounds of maxFrames levels from the top, each round walking up from the entry again.
// Every walk is bounded as the session's finishes are (BeamWalk: inside the table, at most `steps` labels): a damaged state gives
// wrong output, never a spin or an access outside.
#pragma once

namespace w2l {

struct BeamCommit {
  u64* tab;          // the slot's table
  u64* ntab;         // scratch: the rebuilt table, cleared
  unsigned cap;
  int* node;         // the slot's stored node and parent ids, nmax of each
  int* par;
  const int* finN;   // the slot's entry count
  int nmax;          // 64, or the wide or many-token session's beam
  int* stack;        // scratch [D][nmax]
  int D;
  int steps;         // no chain has more labels
  const void* lex;   // the lexicon table (labels and words are decoded from edges), or null: an edge's label is the token
  int maxLen, maxWords;
  int* labels;       // [maxLen] this slot's row
  int* words;        // [maxWords] this slot's row (lexicon only)
  int* out;          // [4] labels committed (or needed), words committed (or needed), live (beam_commit_copy's count), 1 = done
};

__device__ __forceinline__ int beam_commit_up(const u64* tab, const BeamWalk& g, int p) {
  return beam_walk_ok(g, p) ? (int)(tab[p - 1] >> 32) : 0;
}

// The many-token session's one more kernel argument (beam <= 1024: an entry per thread).  a.node / a.par are those of half 0 of the
// slot's beam; the current half is curn[0] on the device (a dead beam stops flipping: the frame count does not tell); a half is
// halfWords ints; finNode, which the session's finish reads, follows the half's node ids.
struct BeamCommitMt {
  const int* curn;
  int halfWords;
  int* finNode;
};
template <class C>
__device__ __forceinline__ const C& beam_commit_mt(const C& c) { return c; }

// Mt: nothing (the narrow and wide sessions, whose kernels are what they were before there was an Mt) or a BeamCommitMt
template <int kThreads, class... Mt>
__global__ __launch_bounds__(kThreads) void beam_commit_walk(BeamCommit a, Mt... mt) {
  __shared__ int sMin, sRef, sDiff, sStop, sWords;
  if constexpr (sizeof...(Mt) > 0) {
    const BeamCommitMt& m = beam_commit_mt(mt...);
    const size_t off = (size_t)(m.curn[0] & 1) * m.halfWords;
    a.node += off;
    a.par += off;
  }
  const int tid = threadIdx.x;
  const int n = min(max(*a.finN, 0), min(a.nmax, kThreads));
  BeamWalk g;
  g.capm = a.cap - 1;
  g.steps = a.steps;
  const bool live = tid < n;
  int node = 0, d = 0;
  if (tid == 0) sMin = 0x7fffffff;
  __syncthreads();
  if (live) {
    node = a.node[tid];
    if ((unsigned)node > a.cap) node = 0;
    d = beam_chain_len(a.tab, node, nullptr, g);
    atomicMin(&sMin, d);
  }
  __syncthreads();
  // the cut: every entry's ancestor at the smallest depth, then up together until they are one node
  int depth = n > 0 ? sMin : 0;
  int p = node;
  if (live)
    for (int k = d - depth; k > 0; --k) p = beam_commit_up(a.tab, g, p);
  for (;;) {
    __syncthreads();
    if (tid == 0) { sRef = p; sDiff = 0; }
    __syncthreads();
    if (live && p != sRef) sDiff = 1;
    __syncthreads();
    if (!sDiff || depth == 0) break;
    if (live) p = beam_commit_up(a.tab, g, p);
    --depth;
  }
  // C = sRef at `depth`; the new root is its parent: depth - 1 labels are committed
  const int nLab = max(depth - 1, 0);
  const LexView xv = a.lex ? lex_view(a.lex) : LexView{};
  if (tid == 0) {
    const int root = depth >= 1 ? beam_commit_up(a.tab, g, sRef) : 0;
    int nw = 0;
    if (a.lex) {
      int q = root;
      for (int k = 0; k < nLab && beam_walk_ok(g, q); ++k) {
        const u64 edge = a.tab[q - 1];
        nw += (((unsigned)edge - 1u) & 7u) ? 1 : 0;
        q = (int)(edge >> 32);
      }
    }
    const bool fits = nLab <= a.maxLen && nw <= a.maxWords;
    a.out[0] = nLab; a.out[1] = nw; a.out[2] = 0; a.out[3] = fits ? 1 : 0;
    sStop = fits ? 0 : 1;
    sWords = nw;
    if (fits) {   // root to new root in order, decoded as the finishes decode an edge
      int q = root, j = nw - 1;
      for (int i = nLab - 1; i >= 0 && beam_walk_ok(g, q); --i) {
        const u64 edge = a.tab[q - 1];
        const unsigned l = (unsigned)edge - 1u;
        if (a.lex) {
          const int v = (int)(l >> 3), slot = (int)(l & 7u);
          const LexNode& nd = lex_node(xv, v);
          a.labels[i] = v == 0 ? xv.silToken : nd.tok;
          if (slot > 0) {
            if (j >= 0) a.words[j] = nd.words[min(slot - 1, kLexMaxWords - 1)];
            --j;
          }
        } else {
          a.labels[i] = (int)l;
        }
        q = (int)(edge >> 32);
      }
    }
  }
  __syncthreads();
  if (sStop) return;   // the whole workgroup: nothing of the slot has changed
  for (int i = nLab + tid; i < a.maxLen; i += kThreads) a.labels[i] = -1;
  if (a.lex)
    for (int j = sWords + tid; j < a.maxWords; j += kThreads) a.words[j] = -1;

  // the chain below the new root, top-down into the scratch table
  const int rel = d - nLab;
  if (live && rel > 0) {
    int np = 0, npar = 0;
    for (int done = 0; done < rel;) {
      const int take = min(a.D, rel - done), skip = rel - done - take;
      int q = node;
      for (int k = 0; k < skip; ++k) q = beam_commit_up(a.tab, g, q);
      for (int k = 0; k < take; ++k) {
        const u64 edge = beam_walk_ok(g, q) ? a.tab[q - 1] : 1ull;
        a.stack[(size_t)k * a.nmax + tid] = (int)(unsigned)edge - 1;
        q = (int)(edge >> 32);
      }
      for (int k = take - 1; k >= 0; --k) {
        npar = np;
        np = beam_node(a.ntab, g.capm, np, a.stack[(size_t)k * a.nmax + tid]);
      }
      done += take;
    }
    a.node[tid] = np;
    a.par[tid] = npar;
    if constexpr (sizeof...(Mt) > 0) beam_commit_mt(mt...).finNode[tid] = np;
  }
}

// the rebuilt table over the slot's own; out[2] += its nodes.  A refused slot (out[3] == 0) keeps its table.
__global__ __launch_bounds__(256) void beam_commit_copy(u64* __restrict__ tab, const u64* __restrict__ ntab, unsigned cap,
                                                        int* __restrict__ out) {
  __shared__ int sCount;
  if (!out[3]) return;
  if (threadIdx.x == 0) sCount = 0;
  __syncthreads();
  int c = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (size_t)gridDim.x * 256) {
    const u64 v = ntab[i];
    tab[i] = v;
    c += v != 0ull ? 1 : 0;
  }
  if (c) atomicAdd(&sCount, c);
  __syncthreads();
  if (threadIdx.x == 0 && sCount) atomicAdd(&out[2], sCount);
}

struct BeamCommitLayout {
  int* out;     // [S][4]
  u64* ntab;    // [cap]
  int* stack;   // [maxFrames][nmax]
};

static size_t beam_commit_layout(BeamCommitLayout* L, void* scratch, const BeamSession& s) {
  const size_t nmax = s.wide || s.mt ? (size_t)s.d.beam : (size_t)kBeamMax;
  char* p = (char*)scratch;
  char* const p0 = p;
  auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
  int* out = (int*)take((size_t)4 * s.d.slots * sizeof(int));
  u64* ntab = (u64*)take(s.cap * sizeof(u64));
  int* stack = (int*)take((size_t)s.d.maxFrames * nmax * sizeof(int));
  if (L) *L = BeamCommitLayout{out, ntab, stack};
  return (size_t)(p - p0);
}

}  // namespace w2l

W2L_API size_t w2l_beam_session_commit_bytes(void* session) {
  using namespace w2l;
  if (!session) return 0;
  const BeamSession& s = *(BeamSession*)session;
  if (s.mt && s.d.beam > kBeamWideMax) return 0;   // the walk is an entry per thread
  return beam_commit_layout(nullptr, nullptr, s);
}

W2L_API int w2l_beam_session_commit(void* session, const int* h_commit, void* scratch, size_t scratchBytes, int maxLen, int* labels,
                                    int maxWords, int* words, int* h_nLabels, int* h_nWords, int* h_live, w2l_stream_t stream) {
  using namespace w2l;
  if (!session) return beam_session_fail(W2L_EINVAL, "beam session commit: null session");
  BeamSession& s = *(BeamSession*)session;
  if (s.mt && s.d.beam > kBeamWideMax)
    return beam_session_fail(W2L_EUNSUPPORTED, "beam session commit: a many-token session commits at a beam up to 1024 (the walk is an "
                                               "entry per thread), this one has " + std::to_string(s.d.beam));
  const size_t need = beam_commit_layout(nullptr, nullptr, s);
  if (!scratch || ((uintptr_t)scratch & 255))
    return beam_session_fail(W2L_EINVAL, "beam session commit: the scratch buffer must be a 256-byte aligned device pointer");
  if (scratchBytes < need)
    return beam_session_fail(W2L_EINVAL, "beam session commit: the scratch buffer is smaller than w2l_beam_session_commit_bytes (" +
                                             std::to_string(scratchBytes) + " < " + std::to_string(need) + ")");
  const bool lex = s.d.variant == W2L_BEAM_LEX;
  if (maxLen < 1) return beam_session_fail(W2L_EINVAL, "beam session commit: maxLen < 1");
  if (!labels) return beam_session_fail(W2L_EINVAL, "beam session commit: null labels");
  if (lex && (!words || maxWords < 1))
    return beam_session_fail(W2L_EINVAL, "beam session commit: the lexicon variant writes words (maxWords >= 1)");
  if (!h_nLabels) return beam_session_fail(W2L_EINVAL, "beam session commit: null h_nLabels");
  if (!s.bound) return beam_session_fail(W2L_EINVAL, "beam session commit: no state bound (w2l_beam_session_bind first)");
  const int S = s.d.slots, nmax = s.wide || s.mt ? s.d.beam : kBeamMax;
  hipStream_t st = (hipStream_t)stream;
  BeamCommitLayout L;
  beam_commit_layout(&L, scratch, s);
  const CtcBeamWs& ws = beam_session_ws(s);
  int* const par = s.wide ? s.WL.cy.par : s.L.cy.par;   // not the many-token session's: its ids are in the halves of its beam
  const int half = (lex ? 9 : 8) * nmax;                 // the many-token session: the ints of a half
  std::vector<char> run(S, 0);
  bool any = false;
  for (int i = 0; i < S; ++i) {
    run[i] = (h_commit ? h_commit[i] != 0 : true) && s.active[i];
    any = any || run[i];
  }
  if (any) {
    W2L_HIP_CHECK(hipMemsetAsync(L.out, 0, (size_t)4 * S * sizeof(int), st));
    const unsigned blocks = (unsigned)std::min<size_t>((s.cap + 2047) / 2048, 2048);
    for (int i = 0; i < S; ++i) {
      if (!run[i]) continue;
      W2L_HIP_CHECK(hipMemsetAsync(L.ntab, 0, s.cap * sizeof(u64), st));
      BeamCommit a;
      a.tab = ws.table + (size_t)i * s.cap; a.ntab = L.ntab; a.cap = (unsigned)s.cap;
      a.node = ws.finNode + (size_t)i * nmax; a.par = par + (size_t)i * nmax; a.finN = ws.finN + i; a.nmax = nmax;
      a.stack = L.stack; a.D = s.d.maxFrames;
      a.steps = (int)std::min<size_t>((size_t)s.frames[i], s.cap / 2);
      a.lex = lex ? s.d.lexicon : nullptr;
      a.maxLen = maxLen; a.maxWords = lex ? maxWords : 0;
      a.labels = labels + (size_t)i * maxLen; a.words = lex ? words + (size_t)i * maxWords : nullptr;
      a.out = L.out + 4 * i;
      if (s.mt) {
        a.node = s.ML.xw.beam + (size_t)i * 2 * half;
        a.par = a.node + nmax;
        hipLaunchKernelGGL((beam_commit_walk<kWideThreads, BeamCommitMt>), dim3(1), dim3(kWideThreads), 0, st, a,
                           BeamCommitMt{s.ML.cy.curn + 2 * i, half, ws.finNode + (size_t)i * nmax});
      } else if (s.wide) hipLaunchKernelGGL(beam_commit_walk<kWideThreads>, dim3(1), dim3(kWideThreads), 0, st, a);
      else hipLaunchKernelGGL(beam_commit_walk<256>, dim3(1), dim3(256), 0, st, a);
      W2L_LAUNCH_CHECK();
      hipLaunchKernelGGL(beam_commit_copy, dim3(blocks), dim3(256), 0, st, a.tab, a.ntab, a.cap, a.out);
      W2L_LAUNCH_CHECK();
    }
    W2L_HIP_CHECK(hipMemcpyAsync(s.commitOut, L.out, (size_t)4 * S * sizeof(int), hipMemcpyDeviceToHost, st));
    W2L_HIP_CHECK(hipStreamSynchronize(st));   // the one session call that waits: counts and live come to the host
  }
  int refused = -1;
  for (int i = 0; i < S; ++i) {
    const int* o = s.commitOut + 4 * i;
    int nl = 0, nw = 0, live = s.live[i];   // a slot that is not committed keeps its count (0 for one that is closed)
    if (run[i]) {
      nl = o[0]; nw = o[1];
      if (o[3]) {
        live = o[2];
        s.doneLabels[i] += nl;
        s.doneWords[i] += nw;
        s.live[i] = live;
        s.credit[i] = s.frames[i] - (live + s.d.beam - 1) / s.d.beam;
      } else if (refused < 0) {
        refused = i;
      }
    }
    h_nLabels[i] = nl;
    if (h_nWords) h_nWords[i] = nw;
    if (h_live) h_live[i] = live;
  }
  if (refused >= 0) {
    const int* o = s.commitOut + 4 * refused;
    return beam_session_fail(W2L_EINVAL, "beam session commit: slot " + std::to_string(refused) + " has " + std::to_string(o[0]) +
                                             " labels and " + std::to_string(o[1]) + " words to commit, maxLen = " +
                                             std::to_string(maxLen) + ", maxWords = " + std::to_string(lex ? maxWords : 0) +
                                             "; the slot is unchanged");
  }
  return W2L_OK;
}

W2L_API int w2l_beam_session_committed(void* session, int slot, int* h_labels, int* h_words) {
  using namespace w2l;
  if (!session) return beam_session_fail(W2L_EINVAL, "beam session committed: null session");
  BeamSession& s = *(BeamSession*)session;
  if (slot < 0 || slot >= s.d.slots) return beam_session_fail(W2L_EINVAL, "beam session committed: no such slot");
  if (h_labels) *h_labels = s.doneLabels[slot];
  if (h_words) *h_words = s.doneWords[slot];
  return W2L_OK;
}
