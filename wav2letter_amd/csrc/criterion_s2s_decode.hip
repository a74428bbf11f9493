// criterion_s2s_decode.hip -- decoding a seq2seq model (DESIGN 3.35 is the contract): a token beam search over the step-by-step decoder
// of the model of DESIGN 3.34 (embedding, GRU cell, one round of attention with o = h + context, output Linear).  fp32 throughout.
//
// Rows are r = b beam + j.  A beam level is a table (score, token, src, peakPrev per row; nSlots, nLive per utterance): src is the
// slot of the previous level whose state the row continues, or -1 for a row that computes nothing (an empty slot, or a hypothesis that
// ended in eos).  Live rows stand in front.  Tables and hidden states are double-buffered: step u reads level u (set u & 1) and the
// states of step u - 1, and writes level u + 1 and the states of step u.  One step is five launches in stream order:
//
//   cell        grid (H / 32, ceil(R / 32)).  32 rows x 32 hidden columns: wave 0 holds the r gate's tile (W_ir x + W_hr h), wave 1 the
//               z gate's, wave 2 W_in x, wave 3 W_hn h, each one v_mfma_f32_32x32x2_f32 accumulator.  The A operands are GATHERED
//               while they are staged (E[token] or the start row; hPrev[src]; 128 columns per chunk), so the beam reorder costs no
//               launch; a lane reads its weight row 16 bytes at a time, once per row tile.  Chunks ascend; expf / tanhf gates.
//   attention   grid (ceil(beam / 32), B).  The training kernel's two products (s2s_attn.hpp) with the score rows in LDS between
//               them; writes o = h + context and the first argmax of alpha, not alpha.
//   vocabulary  grid (ceil(N / 128), ceil(R / 32)).  32 rows x 128 columns, a 32 x 32 accumulator per wave, o and the W slab staged
//               per 32 rows of K.  z = (acc + bias) / temperature goes to LDS, never to memory: a wave per row writes the slab's
//               (max, sum exp) and its min(beamToken, 128) largest (z, token) in order, each element finding its rank by counting.
//   merge       a wave per live row: lse from the slabs' pairs in slab order, and the row's min(beamToken, N) best tokens by
//               popping the heads of the slabs' sorted lists (values staged in LDS when they fit).
//   prune       a workgroup per utterance: finished hypotheses to the completed pool (kept to its best `beam` by a bitonic sort),
//               the nLive x beamToken candidates into LDS, eos score, attention threshold, one bitonic sort by (score descending,
//               parent slot, token), the beam threshold against the best, the next level written with live rows in front, the
//               back-pointer row of the trace table.
//
// A tile whose rows are all dead returns at once.  A row's bits depend on its own operands only: every sum has one order and no tile
// mixes rows, so two calls agree bit for bit and an utterance decodes the same alone or in a batch.  The host launches steps back to
// back and reads one count of unfinished utterances every 8 steps.  A last launch ranks the results and walks the back-pointers.
//
// LM fusion: merge, prune and the last launch have a second instantiation, kLm.  Every row carries the
// n-gram state of its hypothesis and its running unweighted LM score.  The merge wave, once its row's tokens are popped, has lane k look
// up q(state, token k) -- R waves of min(beamToken, N) hash walks each, spread over the chip -- and writes (q, next state) beside the
// candidate; the prune packs the candidate's place in its row into the sort value, adds lmWeight q after the acoustic adds, and writes
// the child's state and LM score into the next level and, for finished hypotheses, into the pool.  The LM-free kernels are the
// kLm = false instantiations with an empty argument pack: their arguments and their instructions do not change.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "ngram_lm.hpp"
#include "s2s_attn.hpp"

namespace w2l {

constexpr int kDecThreads = 256;
constexpr int kDecRt = 32;                        // rows of a tile = M of the MFMA tile
constexpr int kDecSlab = 128;                     // vocabulary columns of a workgroup: 32 per wave
constexpr int kDecKc = 128, kDecLda = kDecKc + 4; // the cell's staged columns of x and h; LDS row stride
constexpr int kDecVk = 32, kDecLdo = 36, kDecLdw = kDecSlab + 4;   // the vocabulary product's chunk of K; LDS row strides of o and W
constexpr int kDecMaxBeam = 128, kDecMaxBt = 64, kDecMaxLen = 512, kDecMaxN = 65536;
constexpr int kDecLists = kDecMaxN / kDecSlab / 64;                // sorted lists a lane of the merge can own
constexpr int kDecMergeLds = 8192;                // list values a merge wave stages in LDS
constexpr int kDecPool = 2 * kDecMaxBeam;         // pool entries in LDS: the kept `beam` and a level's finished hypotheses

struct DecTable { float* score; int *token, *src, *peakPrev, *nSlots, *nLive; };

struct DecStep {
  const float *E, *start, *wih, *whh, *bih, *bhh, *W, *bias, *k, *v, *hPrev;
  const int *keyLen, *src, *token;
  float *h, *o, *partMS, *partVal, *lse, *candVal;
  int *peak, *partTok, *candTok;
  int B, T, H, N, ldenc, ldS, beam, R, nSlab, kk, bt, ldc;
  float scale, temperature;
  bool vecEnc;
};

struct DecPrune {
  DecTable cur, nxt;
  const float *lse, *candVal;
  const int *candTok, *peak;
  float* poolScore;
  int *poolRef, *poolCount, *done, *lastLevel, *trPar, *trTok;
  int B, beam, bt, ldc, eos, u, attThr, n2max;
  float threshold, eosScore;
};

// what the kLm instantiations take beside DecStep / DecPrune: the blob (device memory, read through ngram_view / ngram_q only), the two
// levels' LM columns, a step's (q, next state) per candidate, the pool's LM scores
struct DecLmTable { int* state; float* lmScore; };
struct DecLm {
  const void* blob;
  DecLmTable cur, nxt;
  float *candLm, *poolLm;
  int* candNext;
  float weight;
  int hasEos, eos, eosWord;
};
struct DecLmOut { const float *poolLm, *lm0, *lm1; float* lmScores; };
// merge, prune and the last launch are templates <kLm, Lm...>: the LM-free instantiation has an empty pack, so its arguments and its
// instructions are what they were; the kLm one takes one more argument (DecLm, or DecLmOut in the last launch)
struct DecNoLm {};
__device__ __forceinline__ DecNoLm dec_lm_arg() { return DecNoLm{}; }
template <class T> __device__ __forceinline__ T dec_lm_arg(const T& x) { return x; }

__device__ __forceinline__ float dec_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}
// does any of the tile's rows compute?  (block-uniform)
__device__ __forceinline__ bool dec_tile_live(const int* src, int r0, int rows) {
  const int t = threadIdx.x;
  return __syncthreads_or(t < rows && src[r0 + t] >= 0) != 0;
}
// (ka, va) stands before (kb, vb): the larger key, then the smaller value
__device__ __forceinline__ bool dec_before(float ka, int va, float kb, int vb) { return ka > kb || (ka == kb && va < vb); }

// bitonic sort of n2 = 2^m pairs in LDS, best first; all threads of the workgroup
__device__ __forceinline__ void dec_sort(float* key, int* val, int n2) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < n2; i += kDecThreads) {
        const int p = i ^ j;
        if (p <= i) continue;
        const float ki = key[i], kp = key[p];
        const int vi = val[i], vp = val[p];
        if ((i & k) == 0 ? dec_before(kp, vp, ki, vi) : dec_before(ki, vi, kp, vp)) {
          key[i] = kp; key[p] = ki; val[i] = vp; val[p] = vi;
        }
      }
    }
  __syncthreads();
}

// ---- 1. the GRU cell with gathered operands -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDecThreads) void s2s_dec_cell_k(DecStep a) {
  __shared__ __attribute__((aligned(16))) float sx[kDecRt * kDecLda];
  __shared__ __attribute__((aligned(16))) float sh[kDecRt * kDecLda];
  __shared__ float red[4 * kDecRt * 33];
  __shared__ int sSrc[kDecRt], sTok[kDecRt];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int j0 = blockIdx.x * 32, r0 = blockIdx.y * kDecRt, H = a.H, rows = min(kDecRt, a.R - r0);
  if (!dec_tile_live(a.src, r0, rows)) return;
  if (tid < kDecRt) {   // the row of hPrev a row continues (-1: a dead row) and its token (-1: the start embedding, zero state)
    const int s = tid < rows ? a.src[r0 + tid] : -1;
    sSrc[tid] = s < 0 ? -1 : (r0 + tid) / a.beam * a.beam + s;
    sTok[tid] = tid < rows ? a.token[r0 + tid] : -1;
  }
  __syncthreads();
  const int g = wave < 2 ? wave : 2;
  const size_t wrow = (size_t)(g * H + j0 + li) * H;   // H is a multiple of 32: every column of the tile is a hidden unit
  const bool useX = wave != 3, useH = wave != 2;
  s2s_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < H; k0 += kDecKc) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + i * kDecThreads, r = e >> 5, c = (e & 31) * 4;
      float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vh = vx;
      if (k0 + c < H && sSrc[r] >= 0) {
        const int tok = sTok[r];
        vx = *reinterpret_cast<const float4*>((tok < 0 ? a.start : a.E + (size_t)tok * H) + k0 + c);
        if (tok >= 0) vh = *reinterpret_cast<const float4*>(a.hPrev + (size_t)sSrc[r] * H + k0 + c);
      }
      *reinterpret_cast<float4*>(sx + r * kDecLda + c) = vx;
      *reinterpret_cast<float4*>(sh + r * kDecLda + c) = vh;
    }
    __syncthreads();
#pragma unroll 4
    for (int it = 0; it < kDecKc / 8; ++it) {
      if (k0 + it * 8 >= H) break;   // wave-uniform: H is a multiple of 8
      const int kl = it * 8 + lh * 4, k = k0 + kl;
      if (useX) {
        const float4 x = *reinterpret_cast<const float4*>(sx + li * kDecLda + kl);
        const float4 w = *reinterpret_cast<const float4*>(a.wih + wrow + k);
        S2S_MFMA4(acc, x, w);
      }
      if (useH) {
        const float4 x = *reinterpret_cast<const float4*>(sh + li * kDecLda + kl);
        const float4 w = *reinterpret_cast<const float4*>(a.whh + wrow + k);
        S2S_MFMA4(acc, x, w);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * kDecRt + s2s_tile_row(r, lh)) * 33 + li] = acc[r];
  __syncthreads();
  for (int e = tid; e < kDecRt * 32; e += kDecThreads) {
    const int b = e >> 5, u = e & 31, j = j0 + u;
    if (sSrc[b] < 0) continue;
    const float* p = red + b * 33 + u;
    const float gr = dec_sigmoid((p[0] + a.bih[j]) + a.bhh[j]);
    const float gz = dec_sigmoid((p[kDecRt * 33] + a.bih[H + j]) + a.bhh[H + j]);
    const float hn = p[3 * kDecRt * 33] + a.bhh[2 * H + j];
    const float gn = tanhf((p[2 * kDecRt * 33] + a.bih[2 * H + j]) + gr * hn);
    const float hprev = sTok[b] < 0 ? 0.f : a.hPrev[(size_t)sSrc[b] * H + j];
    a.h[(size_t)(r0 + b) * H + j] = (1.f - gz) * gn + gz * hprev;
  }
}

// ---- 2. attention: 32 queries of one utterance ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kS2sThreads) void s2s_dec_attn_k(DecStep a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int sLive[kS2sQt];
  float* S = lds;
  float* stage = lds + kS2sQt * a.ldS;
  const int b = blockIdx.y, j0 = blockIdx.x * kS2sQt, rows = min(kS2sQt, a.beam - j0), r0 = b * a.beam + j0, H = a.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (!dec_tile_live(a.src, r0, rows)) return;
  if (threadIdx.x < kS2sQt) sLive[threadIdx.x] = threadIdx.x < rows && a.src[r0 + threadIdx.x] >= 0;
  const int kl = a.keyLen[b], klp = (kl + 31) & ~31;
  const float* hq = a.h + (size_t)r0 * H;
  s2s_qk_product(S, a.ldS, stage, hq, H, rows, true, a.k + (size_t)b * a.T * a.ldenc, a.ldenc, kl, a.vecEnc, H);
  for (int r = wave; r < kS2sQt; r += 4) {
    float* row = S + r * a.ldS;
    if (!sLive[r]) {   // a dead row's state means nothing: its score row feeds the product as zeros and nothing is kept of it
      for (int t = lane; t < klp; t += 64) row[t] = 0.f;
      continue;
    }
    float m = -INFINITY;
    for (int t = lane; t < kl; t += 64) { const float s = row[t] * a.scale; row[t] = s; m = fmaxf(m, s); }
    m = wave_max(m);
    float sum = 0.f;
    for (int t = lane; t < kl; t += 64) { const float e = expf(row[t] - m); row[t] = e; sum += e; }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    float best = -1.f;
    int at = INT_MAX;
    for (int t = lane; t < klp; t += 64) {
      const float p = t < kl ? row[t] * inv : 0.f;
      row[t] = p;
      if (t < kl && p > best) { best = p; at = t; }
    }
    const float top = wave_max(best);
    at = wave_min_int(best == top ? at : INT_MAX);   // the first key that holds the largest probability
    if (lane == 0) a.peak[r0 + r] = at;
  }
  __syncthreads();
  float* out = a.o + (size_t)r0 * H;
  s2s_pv_product(S, a.ldS, stage, a.v + (size_t)b * a.T * a.ldenc, a.ldenc, kl, a.vecEnc, H, [&](int r, int c, float x) {
    if (sLive[r]) out[(size_t)r * H + c] = hq[(size_t)r * H + c] + x;
  });
}

// ---- 3. the output product of a slab of the vocabulary, reduced to what the search needs ------------------------------------------
__global__ __launch_bounds__(kDecThreads) void s2s_dec_vocab_k(DecStep a) {
  __shared__ __attribute__((aligned(16))) float so[kDecRt * kDecLdo];
  __shared__ __attribute__((aligned(16))) float sw[kDecVk * kDecLdw];
  __shared__ __attribute__((aligned(16))) float Z[kDecRt * kDecLdw];
  __shared__ int sLive[kDecRt];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int slab = blockIdx.x, c0 = slab * kDecSlab, r0 = blockIdx.y * kDecRt, H = a.H, N = a.N, rows = min(kDecRt, a.R - r0);
  if (!dec_tile_live(a.src, r0, rows)) return;
  if (tid < kDecRt) sLive[tid] = tid < rows && a.src[r0 + tid] >= 0;
  const bool mine = c0 + wave * 32 < N;   // wave-uniform: some of this wave's 32 columns are tokens
  s2s_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < H; k0 += kDecVk) {   // H is a multiple of 32
    __syncthreads();
    {
      const int r = tid >> 3, c = (tid & 7) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (sLive[r]) v = *reinterpret_cast<const float4*>(a.o + (size_t)(r0 + r) * H + k0 + c);
      *reinterpret_cast<float4*>(so + r * kDecLdo + c) = v;
    }
#pragma unroll
    for (int i = 0; i < kDecVk * kDecSlab / kDecThreads; ++i) {
      const int e = tid + i * kDecThreads, kr = e >> 7, c = e & 127;
      sw[kr * kDecLdw + c] = c0 + c < N ? a.W[(size_t)(k0 + kr) * N + c0 + c] : 0.f;   // rows of W [H][N] are not aligned: N is any
    }
    __syncthreads();
    if (!mine) continue;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int kl = it * 8 + lh * 4;
      const float4 x = *reinterpret_cast<const float4*>(so + li * kDecLdo + kl);
      const float* bp = sw + kl * kDecLdw + wave * 32 + li;
      const float4 w = make_float4(bp[0], bp[kDecLdw], bp[2 * kDecLdw], bp[3 * kDecLdw]);
      S2S_MFMA4(acc, x, w);
    }
  }
  {   // the ragged last slab: a column that is no token holds -inf and enters no max, no sum and no list
    const int c = c0 + wave * 32 + li;
    const float bc = c < N ? a.bias[c] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) Z[s2s_tile_row(r, lh) * kDecLdw + wave * 32 + li] = c < N ? (acc[r] + bc) / a.temperature : -INFINITY;
  }
  __syncthreads();
  const int kk = a.kk;
  for (int r = wave; r < kDecRt; r += 4) {
    if (!sLive[r]) continue;
    const float* z = Z + r * kDecLdw;
    const float v0 = z[lane], v1 = z[lane + 64];
    const float m = wave_max(fmaxf(v0, v1));
    const float s = wave_sum(expf(v0 - m) + expf(v1 - m));
    const size_t at = (size_t)(r0 + r) * a.nSlab + slab;
    if (lane == 0) { a.partMS[2 * at] = m; a.partMS[2 * at + 1] = s; }
    // the rank of an element: how many stand before it (the larger value, then the lower column)
    int k0r = 0, k1r = 0;
#pragma unroll 8
    for (int q = 0; q < kDecSlab / 4; ++q) {
      const float4 x = *reinterpret_cast<const float4*>(z + 4 * q);
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int j = 4 * q + t;
        k0r += (xs[t] > v0 || (xs[t] == v0 && j < lane)) ? 1 : 0;
        k1r += (xs[t] > v1 || (xs[t] == v1 && j < lane + 64)) ? 1 : 0;
      }
    }
    if (k0r < kk) { a.partVal[at * kk + k0r] = v0; a.partTok[at * kk + k0r] = c0 + lane < N ? c0 + lane : -1; }
    if (k1r < kk) { a.partVal[at * kk + k1r] = v1; a.partTok[at * kk + k1r] = c0 + lane + 64 < N ? c0 + lane + 64 : -1; }
  }
}

// ---- 3b. a row's slabs into its lse and its best tokens ------------------------------------------------------------------------------
template <bool kLm, class... Lm>
__global__ __launch_bounds__(64) void s2s_dec_merge_k(DecStep a, Lm... lmArg) {
  [[maybe_unused]] const auto lm = dec_lm_arg(lmArg...);
  __shared__ float sv[kDecMergeLds];
  const int r = blockIdx.x, lane = threadIdx.x, nSlab = a.nSlab, kk = a.kk, n = nSlab * kk;
  if (a.src[r] < 0) return;
  const float* gv = a.partVal + (size_t)r * n;
  const int* gt = a.partTok + (size_t)r * n;
  const float* ms = a.partMS + (size_t)r * nSlab * 2;
  float m = -INFINITY;
  for (int s = lane; s < nSlab; s += 64) m = fmaxf(m, ms[2 * s]);
  m = wave_max(m);
  float sum = 0.f;
  for (int s = lane; s < nSlab; s += 64) sum += ms[2 * s + 1] * expf(ms[2 * s] - m);
  sum = wave_sum(sum);
  if (lane == 0) a.lse[r] = m + logf(sum);
  const float* vals = gv;
  if (n <= kDecMergeLds) {
    for (int i = lane; i < n; i += 64) sv[i] = gv[i];
    __syncthreads();
    vals = sv;
  }
  // lane l owns the sorted lists of slabs l, l + 64, ...: hv their heads, pos how many of each are taken
  float hv[kDecLists];
  int pos[kDecLists];
#pragma unroll
  for (int q = 0; q < kDecLists; ++q) {
    const int s = lane + 64 * q;
    pos[q] = 0;
    hv[q] = s < nSlab ? vals[(size_t)s * kk] : -INFINITY;
  }
  float* cv = a.candVal + (size_t)r * a.ldc;
  int* ct = a.candTok + (size_t)r * a.ldc;
  [[maybe_unused]] int myTok = -1;   // kLm: lane i keeps the i-th token
  for (int i = 0; i < a.bt; ++i) {
    float best = -INFINITY;
    int bq = 0;
#pragma unroll
    for (int q = 0; q < kDecLists; ++q)
      if (hv[q] > best) { best = hv[q]; bq = q; }   // among a lane's equal heads the lower slab: the lower token
    const float top = wave_max(best);
    if (top == -INFINITY) {   // fewer tokens than asked for: cannot happen with bt <= N, kept for a row of NaN or -inf
      if (lane == 0) { cv[i] = -INFINITY; ct[i] = -1; }
      continue;
    }
    const bool tied = best == top;
    const size_t head = (size_t)(lane + 64 * bq) * kk;
    int p = 0;
#pragma unroll
    for (int q = 0; q < kDecLists; ++q) p = q == bq ? pos[q] : p;
    unsigned long long who = __ballot(tied);
    if (__popcll(who) > 1) {   // equal values in two lanes: the lower token
      const int tok = tied ? gt[head + p] : INT_MAX;
      const int low = wave_min_int(tok);
      who = __ballot(tied && tok == low);
    }
    if constexpr (kLm) {
      const int win = __ffsll((long long)who) - 1;
      const int t = __shfl(lane == win ? gt[head + p] : -1, win);
      if (lane == i) myTok = t;
    }
    if (lane == __ffsll((long long)who) - 1) {
      cv[i] = top;
      ct[i] = gt[head + p];
      const float next = p + 1 < kk ? vals[head + p + 1] : -INFINITY;
#pragma unroll
      for (int q = 0; q < kDecLists; ++q)
        if (q == bq) { pos[q] = p + 1; hv[q] = next; }
    }
  }
  for (int i = a.bt + lane; i < a.ldc; i += 64) { cv[i] = -INFINITY; ct[i] = -1; }
  if constexpr (kLm) {   // lane k scores the k-th token in the row's LM state; eos is the LM's EOS word, or nothing in a model without one
    const NgramView v = ngram_view(lm.blob);
    if (lane < a.bt) {
      const bool isEos = myTok == lm.eos;
      float q = 0.f;
      int next = 0;
      if (myTok >= 0 && (!isEos || lm.hasEos)) q = ngram_q(v, lm.cur.state[r], isEos ? lm.eosWord : myTok, &next);
      lm.candLm[(size_t)r * a.ldc + lane] = q;
      lm.candNext[(size_t)r * a.ldc + lane] = next;
    }
  }
}

// ---- 4. the next beam level of an utterance ------------------------------------------------------------------------------------------
// kLm: the sort value is (parent slot << 22) | (token << 6) | the candidate's place in its row -- the same order, since a row holds a
// token once -- and pLm [kDecPool] stands behind flag
template <bool kLm, class... Lm>
__global__ __launch_bounds__(kDecThreads) void s2s_dec_prune_k(DecPrune a, Lm... lmArg) {
  [[maybe_unused]] const auto lm = dec_lm_arg(lmArg...);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* key = lds;
  int* val = reinterpret_cast<int*>(lds + a.n2max);
  float* pKey = lds + 2 * a.n2max;
  int* pVal = reinterpret_cast<int*>(pKey + kDecPool);
  int* pRef = pVal + kDecPool;
  int* flag = pRef + kDecPool;   // [kDecMaxBeam]
  [[maybe_unused]] float* pLm = reinterpret_cast<float*>(flag + kDecMaxBeam);
  const int b = blockIdx.x, tid = threadIdx.x, beam = a.beam, base = b * beam;
  if (a.done[b]) return;
  const int n = a.cur.nSlots[b], nLive = a.cur.nLive[b], nEos = n - nLive;
  // the hypotheses of this level that ended in eos (they stand behind the live ones) move to the completed pool
  if (nEos > 0) {
    const int cap = 2 * beam, pc = a.poolCount[b], all = pc + nEos;   // pc <= beam, nEos <= beam
    if (tid < kDecPool) {
      float s = -INFINITY;
      int ref = -1;
      if (tid < pc) { s = a.poolScore[(size_t)b * cap + tid]; ref = a.poolRef[(size_t)b * cap + tid]; }
      else if (tid < all) { const int j = nLive + tid - pc; s = a.cur.score[base + j]; ref = (a.u << 8) | j; }
      pKey[tid] = s; pRef[tid] = ref; pVal[tid] = tid < all ? tid : INT_MAX;
      if constexpr (kLm) pLm[tid] = tid < pc ? lm.poolLm[(size_t)b * cap + tid] : tid < all ? lm.cur.lmScore[base + nLive + tid - pc] : 0.f;
    }
    __syncthreads();
    if (all >= beam) dec_sort(pKey, pVal, kDecPool);   // the best `beam`; among equals the earlier entry
    const int keep = min(all, beam);
    if (tid < keep) { a.poolScore[(size_t)b * cap + tid] = pKey[tid]; a.poolRef[(size_t)b * cap + tid] = pRef[min(pVal[tid], kDecPool - 1)]; }
    if constexpr (kLm)
      if (tid < keep) lm.poolLm[(size_t)b * cap + tid] = pLm[min(pVal[tid], kDecPool - 1)];
    if (tid == 0) a.poolCount[b] = keep;
  }
  if (nLive == 0) {   // nobody proposes: this utterance's search is over; its last levels stay as they are
    for (int j = tid; j < beam; j += kDecThreads) a.nxt.src[base + j] = -1;
    if (tid == 0) { a.nxt.nLive[b] = 0; a.done[b] = 1; }
    return;
  }
  const int bt = a.bt, nc = nLive * bt;
  int n2 = 1;
  while (n2 < nc) n2 <<= 1;
  for (int i = tid; i < n2; i += kDecThreads) {
    float s = -INFINITY;
    int v = INT_MAX;
    if (i < nc) {
      const int j = i / bt, c = i - j * bt, r = base + j, tok = a.candTok[(size_t)r * a.ldc + c], pp = a.cur.peakPrev[r];
      const bool blocked = a.attThr >= 0 && pp >= 0 && abs(a.peak[r] - pp) > a.attThr;
      if (tok >= 0 && !blocked) {
        s = a.cur.score[r] + (a.candVal[(size_t)r * a.ldc + c] - a.lse[r]);
        if (tok == a.eos) s += a.eosScore;
        v = (j << 16) | tok;
        if constexpr (kLm) {
          if (tok != a.eos || lm.hasEos) s = s + lm.weight * lm.candLm[(size_t)r * a.ldc + c];
          v = (j << 22) | (tok << 6) | c;
        }
      }
    }
    key[i] = s; val[i] = v;
  }
  dec_sort(key, val, n2);
  const float best = key[0];
  const bool keep = tid < min(beam, n2) && key[tid] > -INFINITY && key[tid] >= best - a.threshold;
  const int tok = keep ? (kLm ? (val[tid] >> 6) & 0xffff : val[tid] & 0xffff) : 0, par = keep ? (val[tid] >> (kLm ? 22 : 16)) : 0;
  const bool ends = keep && tok == a.eos;
  if (tid < kDecMaxBeam) flag[tid] = keep ? (ends ? 2 : 1) : 0;
  __syncthreads();
  int nNew = 0, nLiveNew = 0, before = 0;   // kept slots; live ones among them; of my own kind before me
  for (int j = 0; j < beam; ++j) {
    const int f = flag[j];
    nNew += f != 0;
    nLiveNew += f == 1;
    if (j < tid) before += ends ? f == 2 : f == 1;
  }
  if (keep) {   // live rows in front, finished ones behind, each kind in the order of the sort
    const int slot = ends ? nLiveNew + before : before;
    const size_t tr = ((size_t)a.u * a.B + b) * beam + slot;
    a.nxt.score[base + slot] = key[tid];
    a.nxt.token[base + slot] = tok;
    a.nxt.src[base + slot] = ends ? -1 : par;
    a.nxt.peakPrev[base + slot] = a.peak[base + par];
    a.trPar[tr] = par;
    a.trTok[tr] = tok;
    if constexpr (kLm) {   // the child's LM state and its unweighted LM score, one fp32 add per token (q is 0 where no term was added)
      const size_t at = (size_t)(base + par) * a.ldc + (val[tid] & 63);
      lm.nxt.state[base + slot] = lm.candNext[at];
      lm.nxt.lmScore[base + slot] = lm.cur.lmScore[base + par] + lm.candLm[at];
    }
  }
  for (int j = nNew + tid; j < beam; j += kDecThreads) a.nxt.src[base + j] = -1;
  if (tid == 0) {
    a.nxt.nSlots[b] = nNew;
    a.nxt.nLive[b] = nLiveNew;
    if (nNew > 0) a.lastLevel[b] = a.u + 1;
  }
}

// level 0: the empty hypothesis in slot 0 of every utterance
__global__ void s2s_dec_init_k(DecTable t0, DecTable t1, int* poolCount, int* done, int* lastLevel, int beam, int R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int b = r / beam, j = r - b * beam;
  t0.score[r] = 0.f; t0.token[r] = -1; t0.src[r] = j == 0 ? 0 : -1; t0.peakPrev[r] = -1;
  t1.src[r] = -1;
  if (j == 0) {
    t0.nSlots[b] = 1; t0.nLive[b] = 1; t1.nSlots[b] = 0; t1.nLive[b] = 0;
    poolCount[b] = 0; done[b] = 0; lastLevel[b] = 0;
  }
}

// level 0 of the LM columns: the root holds the blob's start state and an LM score of 0
__global__ void s2s_dec_lm_init_k(const void* blob, DecLmTable t0, int beam, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  t0.state[b * beam] = (int)((const NgramHeader*)blob)->start;
  t0.lmScore[b * beam] = 0.f;
}

__global__ __launch_bounds__(kDecThreads) void s2s_dec_count_k(const int* done, int* liveUtts, int B) {
  int c = 0;
  for (int b = threadIdx.x; b < B; b += kDecThreads) c += done[b] == 0;
  const int any = __syncthreads_count(c > 0);   // only "is anybody left" matters to the host
  if (threadIdx.x == 0) *liveUtts = any;
}

// ---- 5. the results: the best nbest of the pool (or of the last level that holds anything), their tokens by the back-pointers ----
template <bool kLm, class... Lm>
__global__ __launch_bounds__(kDecThreads) void s2s_dec_trace_k(DecTable t0, DecTable t1, const float* poolScore, const int* poolRef, const int* poolCount,
                                                               const int* lastLevel, const int* trPar, const int* trTok, int* tokens, int* lengths,
                                                               float* scores, int B, int beam, int maxLen, int nbest, Lm... lmArg) {
  [[maybe_unused]] const auto lo = dec_lm_arg(lmArg...);
  __shared__ float sc[kDecPool];
  __shared__ int ref[kDecPool];
  const int b = blockIdx.x, tid = threadIdx.x, pc = poolCount[b];
  int cnt;
  [[maybe_unused]] float lmv = 0.f;   // kLm: the unweighted LM score of this thread's hypothesis
  if (pc > 0) {
    cnt = min(pc, kDecPool);
    if (tid < cnt) { sc[tid] = poolScore[(size_t)b * 2 * beam + tid]; ref[tid] = poolRef[(size_t)b * 2 * beam + tid]; }
    if constexpr (kLm)
      if (tid < cnt) lmv = lo.poolLm[(size_t)b * 2 * beam + tid];
  } else {
    const int L = lastLevel[b];
    const DecTable& t = (L & 1) ? t1 : t0;
    cnt = min(t.nSlots[b], beam);
    if (tid < cnt) { sc[tid] = t.score[b * beam + tid]; ref[tid] = (L << 8) | tid; }
    if constexpr (kLm)
      if (tid < cnt) lmv = ((L & 1) ? lo.lm1 : lo.lm0)[b * beam + tid];
  }
  __syncthreads();
  if (tid < cnt) {
    int rank = 0;
    for (int k = 0; k < cnt; ++k) rank += dec_before(sc[k], k, sc[tid], tid);
    if (rank < nbest) {
      const size_t out = (size_t)b * nbest + rank;
      const int L = ref[tid] >> 8;
      int j = ref[tid] & 255;
      scores[out] = sc[tid];
      if constexpr (kLm) lo.lmScores[out] = lmv;
      lengths[out] = L;
      int* row = tokens + out * maxLen;
      for (int l = L; l >= 1; --l) {
        const size_t at = ((size_t)(l - 1) * B + b) * beam + j;
        row[l - 1] = trTok[at];
        j = trPar[at];
      }
      for (int l = L; l < maxLen; ++l) row[l] = -1;
    }
  }
  if (tid >= cnt && tid < nbest) {   // fewer hypotheses than asked for
    const size_t out = (size_t)b * nbest + tid;
    scores[out] = -INFINITY;
    if constexpr (kLm) lo.lmScores[out] = -INFINITY;
    lengths[out] = 0;
    for (int l = 0; l < maxLen; ++l) tokens[out * maxLen + l] = -1;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// lm: the check of w2l_s2s_decode_lm, which honours lmWeight and wants it and eosScore finite
static int dec_check(const w2l_s2s_decode_desc* d, bool lm = false) {
  if (!d || d->B < 1 || d->T < 1 || d->H < 1 || d->N < 2 || d->ldenc < d->H || d->eos < 0 || d->eos >= d->N || d->beam < 1 || d->beamToken < 1 ||
      d->maxLen < 1 || d->nbest < 1 || d->nbest > d->beam || !(d->temperature > 0.f) || !(d->threshold >= 0.f) || !(d->eosScore == d->eosScore))
    return W2L_EINVAL;
  if (lm && (!std::isfinite(d->lmWeight) || !std::isfinite(d->eosScore))) return W2L_EINVAL;
  if (!lm && d->lmWeight != 0.f) return W2L_EUNSUPPORTED;   // LM fusion is w2l_s2s_decode_lm's
  if (d->beam > kDecMaxBeam || d->beamToken > kDecMaxBt || d->maxLen > kDecMaxLen || d->H % 32 || d->H > kS2sMaxH || d->T > kS2sMaxT ||
      d->B > kS2sMaxB || d->N > kDecMaxN)
    return W2L_EUNSUPPORTED;
  return W2L_OK;
}

struct DecWs {
  size_t keyLen, tab[2][6], hbuf[2], o, peak, partMS, partVal, partTok, lse, candVal, candTok, poolScore, poolRef, poolCount, done, lastLevel,
      liveUtts, trPar, trTok, lmState[2], lmScore[2], candLm, candNext, poolLm, total;
  int R, nSlab, kk, bt, n2max;
};
static DecWs dec_ws(const w2l_s2s_decode_desc& d, bool lm = false) {
  DecWs w{};
  w.R = d.B * d.beam;
  w.nSlab = (d.N + kDecSlab - 1) / kDecSlab;
  w.kk = std::min(d.beamToken, kDecSlab);
  w.bt = std::min(d.beamToken, d.N);
  w.n2max = 1;
  while (w.n2max < d.beam * w.bt) w.n2max <<= 1;
  size_t at = 0;
  auto take = [&](size_t elems) { const size_t o = at; at += align_up(elems * 4, 256); return o; };
  const size_t R = w.R, B = d.B;
  w.keyLen = take(B);
  for (int s = 0; s < 2; ++s) {
    for (int i = 0; i < 4; ++i) w.tab[s][i] = take(R);
    w.tab[s][4] = take(B); w.tab[s][5] = take(B);
  }
  w.hbuf[0] = take(R * d.H); w.hbuf[1] = take(R * d.H); w.o = take(R * d.H); w.peak = take(R);
  w.partMS = take(R * w.nSlab * 2); w.partVal = take(R * w.nSlab * w.kk); w.partTok = take(R * w.nSlab * w.kk);
  w.lse = take(R); w.candVal = take(R * d.beamToken); w.candTok = take(R * d.beamToken);
  w.poolScore = take(2 * R); w.poolRef = take(2 * R); w.poolCount = take(B); w.done = take(B); w.lastLevel = take(B); w.liveUtts = take(1);
  w.trPar = take((size_t)d.maxLen * R); w.trTok = take((size_t)d.maxLen * R);
  if (lm) {   // behind everything else: the LM-free layout is a prefix of this one
    for (int s = 0; s < 2; ++s) { w.lmState[s] = take(R); w.lmScore[s] = take(R); }
    w.candLm = take(R * d.beamToken); w.candNext = take(R * d.beamToken); w.poolLm = take(2 * R);
  }
  w.total = at;
  return w;
}
static DecTable dec_table(char* ws, const DecWs& w, int s) {
  return DecTable{(float*)(ws + w.tab[s][0]), (int*)(ws + w.tab[s][1]), (int*)(ws + w.tab[s][2]), (int*)(ws + w.tab[s][3]),
                  (int*)(ws + w.tab[s][4]), (int*)(ws + w.tab[s][5])};
}

static DecStep dec_step_args(const w2l_s2s_decode_desc& d, const DecWs& w, char* ws, const float* E, const float* start, const float* rnn,
                             const float* W, const float* bias, const float* k, const float* v) {
  DecStep a{};
  const size_t H = d.H;
  a.E = E; a.start = start; a.W = W; a.bias = bias; a.k = k; a.v = v;
  a.wih = rnn; a.whh = rnn + 3 * H * H; a.bih = rnn + 6 * H * H; a.bhh = rnn + 6 * H * H + 3 * H;   // the GRU's flat parameter, I = H
  a.keyLen = (const int*)(ws + w.keyLen);
  a.partMS = (float*)(ws + w.partMS); a.partVal = (float*)(ws + w.partVal); a.partTok = (int*)(ws + w.partTok);
  a.B = d.B; a.T = d.T; a.H = d.H; a.N = d.N; a.ldenc = d.ldenc; a.ldS = s2s_lds_stride(d.T); a.beam = d.beam; a.R = w.R;
  a.nSlab = w.nSlab; a.kk = w.kk; a.bt = w.bt; a.ldc = d.beamToken;
  a.scale = (float)(1.0 / sqrt((double)d.H));
  a.temperature = d.temperature;
  a.vecEnc = d.ldenc % 4 == 0 && s2s_aligned(k, v);
  return a;
}

// the cell, attention, vocabulary and merge launches of one step; lm: the merge that also scores its tokens
static int dec_launch_step(const DecStep& a, hipStream_t s, const DecLm* lm = nullptr) {
  static bool seen[64] = {};
  if (first_on_device(seen))
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)s2s_dec_attn_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s2s_lds_bytes(kS2sMaxT)));
  const int tiles = (a.R + kDecRt - 1) / kDecRt;
  s2s_dec_cell_k<<<dim3(a.H / 32, tiles), kDecThreads, 0, s>>>(a);
  W2L_LAUNCH_CHECK();
  s2s_dec_attn_k<<<dim3((a.beam + kS2sQt - 1) / kS2sQt, a.B), kS2sThreads, s2s_lds_bytes(a.T), s>>>(a);
  W2L_LAUNCH_CHECK();
  s2s_dec_vocab_k<<<dim3(a.nSlab, tiles), kDecThreads, 0, s>>>(a);
  W2L_LAUNCH_CHECK();
  if (lm) s2s_dec_merge_k<true><<<a.R, 64, 0, s>>>(a, *lm);
  else s2s_dec_merge_k<false><<<a.R, 64, 0, s>>>(a);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

static int dec_common_check(const w2l_s2s_decode_desc* d, const float* E, const float* start, const float* rnn, const float* W, const float* bias,
                            const float* k, const float* v, const int* keyLen, void* workspace, size_t workspaceBytes, bool lm = false) {
  const int st = dec_check(d, lm);
  if (st != W2L_OK) return st;
  if (!E || !start || !rnn || !W || !bias || !k || !v || !keyLen || !workspace || !s2s_aligned(E, start, rnn, workspace) ||
      workspaceBytes < dec_ws(*d, lm).total)
    return W2L_EINVAL;
  for (int b = 0; b < d->B; ++b)
    if (keyLen[b] < 1 || keyLen[b] > d->T) return W2L_EINVAL;
  return W2L_OK;
}

#define DEC_OK(expr) do { const int _st = (expr); if (_st != W2L_OK) return _st; } while (0)

}  // namespace w2l

using namespace w2l;

W2L_API size_t w2l_s2s_decode_workspace_size(const w2l_s2s_decode_desc* d) {
  if (dec_check(d) != W2L_OK) return 0;
  return dec_ws(*d).total;
}

W2L_API int w2l_s2s_decode_step(const w2l_s2s_decode_desc* d, const float* E, const float* start, const float* rnn, const float* W,
                                const float* bias, const float* k, const float* v, const int* keyLen, const int* parent, const int* token,
                                const float* hPrev, float* h, float* o, int* peak, float* lse, float* candVal, int* candTok, void* workspace,
                                size_t workspaceBytes, w2l_stream_t stream) {
  DEC_OK(dec_common_check(d, E, start, rnn, W, bias, k, v, keyLen, workspace, workspaceBytes));
  if (!parent || !token || !h || !o || !peak || !lse || !candVal || !candTok || !s2s_aligned(h, o, hPrev)) return W2L_EINVAL;
  const DecWs w = dec_ws(*d);
  for (int r = 0; r < w.R; ++r) {
    if (parent[r] >= d->beam || token[r] < -1 || token[r] >= d->N) return W2L_EINVAL;
    if (parent[r] >= 0 && token[r] >= 0 && !hPrev) return W2L_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const DecTable t = dec_table(ws, w, 0);
  W2L_HIP_CHECK(hipMemcpyAsync(ws + w.keyLen, keyLen, (size_t)d->B * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipMemcpyAsync(t.src, parent, (size_t)w.R * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipMemcpyAsync(t.token, token, (size_t)w.R * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipStreamSynchronize(s));   // the host arrays are the caller's again when this call returns
  DecStep a = dec_step_args(*d, w, ws, E, start, rnn, W, bias, k, v);
  a.src = t.src; a.token = t.token; a.hPrev = hPrev; a.h = h; a.o = o; a.peak = peak; a.lse = lse; a.candVal = candVal; a.candTok = candTok;
  return dec_launch_step(a, s);
}

// the whole search; lm: the blob and lmScores of w2l_s2s_decode_lm, whose merge, prune and last launch are the kLm instantiations
struct DecLmCall { const void* blob; int hasEos; float* lmScores; };

static int dec_search(const w2l_s2s_decode_desc* d, const float* E, const float* start, const float* rnn, const float* W, const float* bias,
                      const float* k, const float* v, const int* keyLen, int* tokens, int* lengths, float* scores, void* workspace, hipStream_t s,
                      const DecLmCall* lm) {
  const DecWs w = dec_ws(*d, lm != nullptr);
  char* ws = (char*)workspace;
  const DecTable tab[2] = {dec_table(ws, w, 0), dec_table(ws, w, 1)};
  float* hbuf[2] = {(float*)(ws + w.hbuf[0]), (float*)(ws + w.hbuf[1])};
  const size_t pruneLds = (2 * (size_t)w.n2max + (lm ? 4 : 3) * kDecPool + kDecMaxBeam) * sizeof(float);
  static bool seen[64] = {};
  if (first_on_device(seen)) {
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)s2s_dec_prune_k<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)((2 * 8192 + 3 * kDecPool + kDecMaxBeam) * sizeof(float))));
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)s2s_dec_prune_k<true, DecLm>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)((2 * 8192 + 4 * kDecPool + kDecMaxBeam) * sizeof(float))));
  }
  W2L_HIP_CHECK(hipMemcpyAsync(ws + w.keyLen, keyLen, (size_t)d->B * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipStreamSynchronize(s));   // before any launch: keyLen is the caller's again, as after the step entry
  DecStep a = dec_step_args(*d, w, ws, E, start, rnn, W, bias, k, v);
  a.o = (float*)(ws + w.o); a.peak = (int*)(ws + w.peak); a.lse = (float*)(ws + w.lse);
  a.candVal = (float*)(ws + w.candVal); a.candTok = (int*)(ws + w.candTok);
  DecPrune p{};
  p.lse = a.lse; p.candVal = a.candVal; p.candTok = a.candTok; p.peak = a.peak;
  p.poolScore = (float*)(ws + w.poolScore); p.poolRef = (int*)(ws + w.poolRef); p.poolCount = (int*)(ws + w.poolCount);
  p.done = (int*)(ws + w.done); p.lastLevel = (int*)(ws + w.lastLevel); p.trPar = (int*)(ws + w.trPar); p.trTok = (int*)(ws + w.trTok);
  p.B = d->B; p.beam = d->beam; p.bt = w.bt; p.ldc = d->beamToken; p.eos = d->eos; p.attThr = d->attentionThreshold; p.n2max = w.n2max;
  p.threshold = d->threshold; p.eosScore = d->eosScore;
  DecLm m{};
  DecLmTable ltab[2] = {};
  if (lm) {
    for (int i = 0; i < 2; ++i) ltab[i] = DecLmTable{(int*)(ws + w.lmState[i]), (float*)(ws + w.lmScore[i])};
    m.blob = lm->blob; m.candLm = (float*)(ws + w.candLm); m.candNext = (int*)(ws + w.candNext); m.poolLm = (float*)(ws + w.poolLm);
    m.weight = d->lmWeight; m.hasEos = lm->hasEos; m.eos = d->eos; m.eosWord = d->N + 1;   // the words of a blob for N tokens: N is BOS, N + 1 EOS
  }
  int* liveUtts = (int*)(ws + w.liveUtts);
  s2s_dec_init_k<<<(w.R + 255) / 256, 256, 0, s>>>(tab[0], tab[1], p.poolCount, p.done, p.lastLevel, d->beam, w.R);
  W2L_LAUNCH_CHECK();
  if (lm) {
    s2s_dec_lm_init_k<<<(d->B + 255) / 256, 256, 0, s>>>(m.blob, ltab[0], d->beam, d->B);
    W2L_LAUNCH_CHECK();
  }
  for (int u = 0; u < d->maxLen; ++u) {
    const int cur = u & 1;
    a.src = tab[cur].src; a.token = tab[cur].token; a.hPrev = hbuf[cur ^ 1]; a.h = hbuf[cur];
    m.cur = ltab[cur]; m.nxt = ltab[cur ^ 1];
    DEC_OK(dec_launch_step(a, s, lm ? &m : nullptr));
    p.cur = tab[cur]; p.nxt = tab[cur ^ 1]; p.u = u;
    if (lm) s2s_dec_prune_k<true><<<d->B, kDecThreads, pruneLds, s>>>(p, m);
    else s2s_dec_prune_k<false><<<d->B, kDecThreads, pruneLds, s>>>(p);
    W2L_LAUNCH_CHECK();
    if ((u & 7) == 7 && u + 1 < d->maxLen) {   // is anybody still searching?  one blocking 4-byte copy every 8 steps
      int live = 1;
      s2s_dec_count_k<<<1, kDecThreads, 0, s>>>(p.done, liveUtts, d->B);
      W2L_LAUNCH_CHECK();
      W2L_HIP_CHECK(hipMemcpyAsync(&live, liveUtts, sizeof(int), hipMemcpyDeviceToHost, s));
      W2L_HIP_CHECK(hipStreamSynchronize(s));
      if (!live) break;
    }
  }
  if (lm)
    s2s_dec_trace_k<true><<<d->B, kDecThreads, 0, s>>>(tab[0], tab[1], p.poolScore, p.poolRef, p.poolCount, p.lastLevel, p.trPar, p.trTok, tokens,
                                                   lengths, scores, d->B, d->beam, d->maxLen, d->nbest,
                                                   DecLmOut{m.poolLm, ltab[0].lmScore, ltab[1].lmScore, lm->lmScores});
  else
    s2s_dec_trace_k<false><<<d->B, kDecThreads, 0, s>>>(tab[0], tab[1], p.poolScore, p.poolRef, p.poolCount, p.lastLevel, p.trPar, p.trTok, tokens, lengths,
                                                scores, d->B, d->beam, d->maxLen, d->nbest);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_s2s_decode(const w2l_s2s_decode_desc* d, const float* E, const float* start, const float* rnn, const float* W, const float* bias,
                           const float* k, const float* v, const int* keyLen, int* tokens, int* lengths, float* scores, void* workspace,
                           size_t workspaceBytes, w2l_stream_t stream) {
  DEC_OK(dec_common_check(d, E, start, rnn, W, bias, k, v, keyLen, workspace, workspaceBytes));
  if (!tokens || !lengths || !scores) return W2L_EINVAL;
  return dec_search(d, E, start, rnn, W, bias, k, v, keyLen, tokens, lengths, scores, workspace, (hipStream_t)stream, nullptr);
}

W2L_API size_t w2l_s2s_decode_lm_workspace_size(const w2l_s2s_decode_desc* d) {
  if (dec_check(d, true) != W2L_OK) return 0;
  return dec_ws(*d, true).total;
}

W2L_API int w2l_s2s_decode_lm(const w2l_s2s_decode_desc* d, const float* E, const float* start, const float* rnn, const float* W, const float* bias,
                              const float* k, const float* v, const int* keyLen, int* tokens, int* lengths, float* scores, float* lmScores,
                              void* workspace, size_t workspaceBytes, w2l_stream_t stream, const void* lm, int lmHasEos) {
  DEC_OK(dec_common_check(d, E, start, rnn, W, bias, k, v, keyLen, workspace, workspaceBytes, true));
  if (!tokens || !lengths || !scores || !lmScores || !lm || (lmHasEos != 0 && lmHasEos != 1)) return W2L_EINVAL;
  const DecLmCall call{lm, lmHasEos, lmScores};
  return dec_search(d, E, start, rnn, W, bias, k, v, keyLen, tokens, lengths, scores, workspace, (hipStream_t)stream, &call);
}
