// attention_causal.hip -- fused causal multi-head self-attention with a relative-position term, fp32, forward and backward: the hot piece
// of the Transformer decoder criterion (DESIGN 3.37 is the contract; include/w2l_hip.h the ABI).
//
//   s[i][j] = scale (q_i . k_j + q_i . E[j - i + n0])  for j <= i,   P = softmax_j s,   Pd = dropout(P),   ctx_i = sum_j Pd[i][j] v_j
//
// Every kernel runs 256 threads on v_mfma_f32_32x32x2_f32 and is built on ONE tile routine, ac_scores: for a 32-query tile i0 and a
// 32-key tile j0 of one (utterance, head) it streams the head's d columns through LDS in chunks of 32 and gives every wave one product:
//   wave 0     S = Q K^T                                              -> sS [32][32]
//   waves 1, 2 R = Q Es^T, Es the 63 table rows j0 - i0 - 31 + n0 ..   -> sR [32][64]; rel[ii][jj] = R[ii][jj - ii + 31] (read skewed)
//   wave 3     dPd = dctx V^T (backward only)                          -> sP [32][32]
// Key tiles above the diagonal are never visited; the diagonal tile is masked where the scores are read.
//
//   forward    grid (ceil(U / 32), Hd, B).  Key tiles 0 .. i0 / 32 in order with an online softmax: 8 lanes share a row (4 scores
//              each), running max and sum in their registers; the dropped probabilities go back to sS and are the A operand of
//              ctx += Pd V, V staged 32 keys x up to 128 columns (two rounds for d = 256), wave w owning 32 columns per round.
//   backward   ac_grad_tile recomputes P = exp(s - lse) and forms Pd and dS = scale P (mult dPd - D) in LDS, D_i = sum_j Pd dPd.
//     query side   per query tile, key tiles ascending: a first pass over them forms D, the second dq += dS K + skew(dS) Es (32 + 63 staged rows).
//     key side     per key tile, query tiles at or below it ascending: dk += dS^T Q, dv += Pd^T dctx.
//     table side   per 32 distances w = i - j, query tiles ascending and the two key tiles that hold j = i - w: dEp[w] += G Q with
//                  G[w][i] = dS[i][i - w]; per-(utterance, head) partials, then a fixed-order sum over (b, h).
// No atomics; every sum has one order; what an utterance receives does not depend on B.
#include <initializer_list>

#include "common.hpp"

namespace w2l {

typedef float ac_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kAcThreads = 256, kAcT = 32;
constexpr int kAcLd = 36;                   // LDS row stride of a 32-column chunk or tile
constexpr int kAcLdR = 68;                  // of the position strip
constexpr int kAcWide = 128, kAcLdW = 132;  // columns per round of the wide stage; its row stride
constexpr int kAcMaxD = 256, kAcMaxC = 1024, kAcMaxU = 512, kAcMaxB = 1024;
// LDS map, in floats
constexpr int kAcA = 0, kAcB = kAcA + kAcT * kAcLd, kAcA2 = kAcB + kAcT * kAcLd, kAcB2 = kAcA2 + kAcT * kAcLd, kAcE = kAcB2 + kAcT * kAcLd;
constexpr int kAcS = kAcE + 64 * kAcLd, kAcR = kAcS + kAcT * kAcLd, kAcP = kAcR + kAcT * kAcLdR, kAcD = kAcP + kAcT * kAcLd;
constexpr int kAcVec = kAcD + kAcT * kAcLd, kAcW = kAcVec + 4 * kAcT;
static inline size_t ac_lds_bytes(int wideRows) { return (size_t)(kAcW + wideRows * kAcLdW) * sizeof(float); }

struct AttnCausal {
  const float *q, *k, *v, *E, *dctx, *lseIn;
  const int* len;
  float *ctx, *lse, *dq, *dk, *dv, *dE, *dEp, *Dw;
  int B, Hd, U, d, ld, ldc, n0;
  float scale, keepScale;
  uint32_t thr, seed, stream;
};

#define AC_ZERO16 {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}
__device__ __forceinline__ int ac_tile_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }
__device__ __forceinline__ float4 ac_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void ac_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// the sum / max over the 8 lanes that share a score row: a butterfly, so all 8 hold the same bits
__device__ __forceinline__ float ac_row_sum(float v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); return v; }
__device__ __forceinline__ float ac_row_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1)); v = fmaxf(v, __shfl_xor(v, 2)); v = fmaxf(v, __shfl_xor(v, 4));
  return v;
}
__device__ __forceinline__ float ac_mult(const AttnCausal& a, int bh, int i, int j) {
  if (!a.thr) return 1.f;
  return keep_elem(((uint64_t)bh * a.U + i) * a.U + j, a.seed, a.stream, a.thr) ? a.keepScale : 0.f;
}

// acc += A B over kk reduction steps: lane (li, lh) supplies fa(li, k) and fb(k, li) for k = 2 s + lh
template <class FA, class FB>
__device__ __forceinline__ void ac_mma(ac_f32x16& acc, int kk, int li, int lh, FA fa, FB fb) {
  for (int k = lh; k < kk; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa(li, k), fb(k, li), acc, 0, 0, 0);
}

// rows [r0, r0 + n) x 128-column round c0 of the wide stage from a [..][ldsrc] array whose row `first + r` must lie in [0, limit)
__device__ __forceinline__ void ac_stage_wide(float* sW, int r0, int n, const float* src, size_t ldsrc, int first, int limit, int c0, int d) {
  const int w4 = min(kAcWide, d - c0) >> 2;
  for (int e = threadIdx.x; e < n * w4; e += kAcThreads) {
    const int r = e / w4, c = (e - r * w4) * 4, g = first + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src && g >= 0 && g < limit) v = ac_ld4(src + (size_t)g * ldsrc + c0 + c);
    ac_st4(sW + (r0 + r) * kAcLdW + c, v);
  }
}

// the tile products described at the top; ends with a barrier.  qb, kb, vb, gb: row 0 of the (utterance, head) in q, k, v, dctx.
// Rows at or past lim = len[b] are staged as zeros: nothing is ever read of the padded rows of an operand.
template <bool BWD>
__device__ __forceinline__ void ac_scores(const AttnCausal& a, float* lds, const float* qb, const float* kb, const float* vb, const float* gb,
                                          int i0, int j0, int lim) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int r = tid >> 3, c = (tid & 7) * 4, w0 = j0 - i0 - 31 + a.n0;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  ac_f32x16 acc = AC_ZERO16;
  for (int c0 = 0; c0 < a.d; c0 += 32) {
    __syncthreads();
    ac_st4(lds + kAcA + r * kAcLd + c, i0 + r < lim ? ac_ld4(qb + (size_t)(i0 + r) * a.ld + c0 + c) : z4);
    ac_st4(lds + kAcB + r * kAcLd + c, j0 + r < lim ? ac_ld4(kb + (size_t)(j0 + r) * a.ld + c0 + c) : z4);
    if (BWD) {
      ac_st4(lds + kAcA2 + r * kAcLd + c, i0 + r < lim ? ac_ld4(gb + (size_t)(i0 + r) * a.ldc + c0 + c) : z4);
      ac_st4(lds + kAcB2 + r * kAcLd + c, j0 + r < lim ? ac_ld4(vb + (size_t)(j0 + r) * a.ld + c0 + c) : z4);
    }
    if (a.E) {
#pragma unroll
      for (int rr = r; rr < 64; rr += 32) {
        const int w = w0 + rr;   // table row; rr == 63 is the unused 64th row of the strip
        ac_st4(lds + kAcE + rr * kAcLd + c, (rr < 63 && w >= 0 && w <= 2 * a.n0) ? ac_ld4(a.E + (size_t)w * a.d + c0 + c) : z4);
      }
    }
    __syncthreads();
    const float* sa = lds + (wave == 3 ? kAcA2 : kAcA);
    const float* sb = lds + (wave == 0 ? kAcB : wave == 3 ? kAcB2 : kAcE + (wave - 1) * 32 * kAcLd);
    if (wave == 0 || (wave == 3 ? BWD : a.E != nullptr))
      ac_mma(acc, 32, li, lh, [&](int row, int k) { return sa[row * kAcLd + k]; }, [&](int k, int col) { return sb[col * kAcLd + k]; });
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int row = ac_tile_row(t, lh);
    if (wave == 0) lds[kAcS + row * kAcLd + li] = acc[t];
    else if (wave == 3) { if (BWD) lds[kAcP + row * kAcLd + li] = acc[t]; }
    else if (a.E) lds[kAcR + row * kAcLdR + (wave - 1) * 32 + li] = acc[t];
  }
  __syncthreads();
}

// the score of (row r, column jj) of the tile the last ac_scores left: scaled, -inf above the diagonal
__device__ __forceinline__ float ac_score(const AttnCausal& a, const float* lds, int r, int jj, int i, int j) {
  float x = lds[kAcS + r * kAcLd + jj];
  if (a.E) x += lds[kAcR + r * kAcLdR + jj - r + 31];
  return j <= i ? x * a.scale : -INFINITY;
}

__global__ __launch_bounds__(kAcThreads) void attn_causal_fwd_k(AttnCausal a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * kAcT, U = a.U, d = a.d, bh = b * a.Hd + h;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int len = a.len[b], rows = min(kAcT, U - i0);
  float* ctx = a.ctx + ((size_t)b * U + i0) * a.ldc + h * d;
  float* lse = a.lse + (size_t)bh * U + i0;
  if (i0 >= len) {   // block-uniform: a tile of padded queries writes its zeros and leaves
    for (int e = tid; e < rows * (d >> 2); e += kAcThreads) ac_st4(ctx + (size_t)(e / (d >> 2)) * a.ldc + (e % (d >> 2)) * 4, make_float4(0.f, 0.f, 0.f, 0.f));
    if (tid < rows) lse[tid] = 0.f;
    return;
  }
  const float* qb = a.q + (size_t)b * U * a.ld + h * d;
  const float* kb = a.k + (size_t)b * U * a.ld + h * d;
  const float* vb = a.v + (size_t)b * U * a.ld + h * d;
  const int r = tid >> 3, cb = (tid & 7) * 4, i = i0 + r;
  float* sW = lds + kAcW;
  float* sAl = lds + kAcVec;
  float m = -INFINITY, l = 0.f;
  ac_f32x16 acc[2] = {AC_ZERO16, AC_ZERO16};
  for (int j0 = 0; j0 <= i0; j0 += kAcT) {
    ac_scores<false>(a, lds, qb, kb, vb, nullptr, i0, j0, len);
    float s[4], mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[e] = ac_score(a, lds, r, cb + e, i, j0 + cb + e); mx = fmaxf(mx, s[e]); }
    const float mn = fmaxf(m, ac_row_max(mx));   // finite from the first tile on: key 0 is never masked
    const float al = expf(m - mn);
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p = expf(s[e] - mn);
      sum += p;
      lds[kAcS + r * kAcLd + cb + e] = p * ac_mult(a, bh, i, j0 + cb + e);
    }
    l = l * al + ac_row_sum(sum);
    m = mn;
    if ((tid & 7) == 0) sAl[r] = al;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int c0 = n * kAcWide;
      if (c0 >= d) break;
      if (n) __syncthreads();
      ac_stage_wide(sW, 0, kAcT, vb, a.ld, j0, len, c0, d);
      __syncthreads();
      if (c0 + wave * 32 < d) {
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[n][t] *= sAl[ac_tile_row(t, lh)];
        ac_mma(acc[n], 32, li, lh, [&](int row, int k) { return lds[kAcS + row * kAcLd + k]; },
               [&](int k, int col) { return sW[k * kAcLdW + wave * 32 + col]; });
      }
    }
  }
  __syncthreads();
  if ((tid & 7) == 0) {
    sAl[r] = l;
    if (i < U) lse[r] = i < len ? m + logf(l) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int cw = n * kAcWide + wave * 32;
    if (cw >= d) continue;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int row = ac_tile_row(t, lh);
      if (i0 + row < U) ctx[(size_t)row * a.ldc + cw + li] = i0 + row < len ? acc[n][t] / sAl[row] : 0.f;
    }
  }
}

// Pd -> sP and dS -> sD of tile (i0, j0); sLse, sDv: lse and D of the 32 queries.  Ends with a barrier.
__device__ __forceinline__ void ac_grad_tile(const AttnCausal& a, float* lds, const float* qb, const float* kb, const float* vb, const float* gb,
                                             int bh, int i0, int j0, int len) {
  ac_scores<true>(a, lds, qb, kb, vb, gb, i0, j0, len);
  const int tid = threadIdx.x, r = tid >> 3, cb = (tid & 7) * 4, i = i0 + r;
  const float lse = lds[kAcVec + r], D = lds[kAcVec + kAcT + r];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int jj = cb + e, j = j0 + jj;
    const bool valid = j <= i && i < len;
    float pd = 0.f, ds = 0.f;
    if (valid) {
      const float p = expf(ac_score(a, lds, r, jj, i, j) - lse), mult = ac_mult(a, bh, i, j);
      pd = p * mult;
      ds = a.scale * p * (lds[kAcP + r * kAcLd + jj] * mult - D);
    }
    lds[kAcP + r * kAcLd + jj] = pd;
    lds[kAcD + r * kAcLd + jj] = ds;
  }
  __syncthreads();
}

// lse and D of query tile i0 into LDS (0 for the rows at or past len)
__device__ __forceinline__ void ac_load_rows(const AttnCausal& a, float* lds, int bh, int i0, int len) {
  const int tid = threadIdx.x;
  if (tid < 2 * kAcT) {
    const int r = tid & 31, i = i0 + r;
    const float* src = tid < kAcT ? a.lseIn : a.Dw;
    lds[kAcVec + tid] = i < len ? src[(size_t)bh * a.U + i] : 0.f;
  }
}

__device__ __forceinline__ void ac_zero_rows(float* dst, size_t ld, int rows, int d) {
  for (int e = threadIdx.x; e < rows * (d >> 2); e += kAcThreads) ac_st4(dst + (size_t)(e / (d >> 2)) * ld + (e % (d >> 2)) * 4, make_float4(0.f, 0.f, 0.f, 0.f));
}

__global__ __launch_bounds__(kAcThreads) void attn_causal_bwd_q_k(AttnCausal a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * kAcT, U = a.U, d = a.d, bh = b * a.Hd + h;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int len = a.len[b], rows = min(kAcT, U - i0);
  float* dq = a.dq + ((size_t)b * U + i0) * a.ld + h * d;
  if (i0 >= len) {
    ac_zero_rows(dq, a.ld, rows, d);
    if (tid < rows) a.Dw[(size_t)bh * U + i0 + tid] = 0.f;
    return;
  }
  const float* qb = a.q + (size_t)b * U * a.ld + h * d;
  const float* kb = a.k + (size_t)b * U * a.ld + h * d;
  const float* vb = a.v + (size_t)b * U * a.ld + h * d;
  const float* gb = a.dctx + (size_t)b * U * a.ldc + h * d;
  {   // first pass: D_i = sum_j Pd[i][j] dPd[i][j], key tiles ascending, from the very products the second pass forms again (so that a
      // row with a single key gets dS = 0 exactly)
    const int r = tid >> 3, cb = (tid & 7) * 4, i = i0 + r;
    if (tid < kAcT) lds[kAcVec + tid] = i0 + tid < len ? a.lseIn[(size_t)bh * U + i0 + tid] : 0.f;
    float D = 0.f;
    for (int j0 = 0; j0 <= i0; j0 += kAcT) {
      ac_scores<true>(a, lds, qb, kb, vb, gb, i0, j0, len);
      const float lse = lds[kAcVec + r];
      float part = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int jj = cb + e, j = j0 + jj;
        if (j <= i && i < len) part += expf(ac_score(a, lds, r, jj, i, j) - lse) * ac_mult(a, bh, i, j) * lds[kAcP + r * kAcLd + jj];
      }
      D += ac_row_sum(part);
    }
    if ((tid & 7) == 0) {
      lds[kAcVec + kAcT + r] = D;
      if (i < U) a.Dw[(size_t)bh * U + i] = D;
    }
  }
  float* sW = lds + kAcW;
  ac_f32x16 acc[2] = {AC_ZERO16, AC_ZERO16};
  for (int j0 = 0; j0 <= i0; j0 += kAcT) {
    ac_grad_tile(a, lds, qb, kb, vb, gb, bh, i0, j0, len);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int c0 = n * kAcWide;
      if (c0 >= d) break;
      if (n) __syncthreads();
      ac_stage_wide(sW, 0, kAcT, kb, a.ld, j0, len, c0, d);
      if (a.E) ac_stage_wide(sW, kAcT, 63, a.E, a.d, j0 - i0 - 31 + a.n0, 2 * a.n0 + 1, c0, d);
      __syncthreads();
      if (c0 + wave * 32 >= d) continue;
      ac_mma(acc[n], 32, li, lh, [&](int row, int k) { return lds[kAcD + row * kAcLd + k]; },
             [&](int k, int col) { return sW[k * kAcLdW + wave * 32 + col]; });
      if (a.E)   // strip column k holds table row j - i + n0 for jj = k + ii - 31
        ac_mma(acc[n], 64, li, lh, [&](int row, int k) { const int jj = k + row - 31; return (jj >= 0 && jj < 32) ? lds[kAcD + row * kAcLd + jj] : 0.f; },
               [&](int k, int col) { return k < 63 ? sW[(kAcT + k) * kAcLdW + wave * 32 + col] : 0.f; });
    }
  }
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int cw = n * kAcWide + wave * 32;
    if (cw >= d) continue;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int row = ac_tile_row(t, lh);
      if (i0 + row < U) dq[(size_t)row * a.ld + cw + li] = i0 + row < len ? acc[n][t] : 0.f;
    }
  }
}

__global__ __launch_bounds__(kAcThreads) void attn_causal_bwd_kv_k(AttnCausal a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.z, h = blockIdx.y, j0 = blockIdx.x * kAcT, U = a.U, d = a.d, bh = b * a.Hd + h;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int len = a.len[b], rows = min(kAcT, U - j0);
  float* dk = a.dk + ((size_t)b * U + j0) * a.ld + h * d;
  float* dv = a.dv + ((size_t)b * U + j0) * a.ld + h * d;
  if (j0 >= len) {
    ac_zero_rows(dk, a.ld, rows, d);
    ac_zero_rows(dv, a.ld, rows, d);
    return;
  }
  const float* qb = a.q + (size_t)b * U * a.ld + h * d;
  const float* kb = a.k + (size_t)b * U * a.ld + h * d;
  const float* vb = a.v + (size_t)b * U * a.ld + h * d;
  const float* gb = a.dctx + (size_t)b * U * a.ldc + h * d;
  float* sW = lds + kAcW;
  ac_f32x16 ak[2] = {AC_ZERO16, AC_ZERO16}, av[2] = {AC_ZERO16, AC_ZERO16};
  for (int i0 = j0; i0 < len; i0 += kAcT) {
    __syncthreads();
    ac_load_rows(a, lds, bh, i0, len);
    ac_grad_tile(a, lds, qb, kb, vb, gb, bh, i0, j0, len);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int c0 = n * kAcWide;
      if (c0 >= d) break;
      if (n) __syncthreads();
      ac_stage_wide(sW, 0, kAcT, qb, a.ld, i0, len, c0, d);
      ac_stage_wide(sW, kAcT, kAcT, gb, a.ldc, i0, len, c0, d);
      __syncthreads();
      if (c0 + wave * 32 >= d) continue;
      ac_mma(ak[n], 32, li, lh, [&](int row, int k) { return lds[kAcD + k * kAcLd + row]; },
             [&](int k, int col) { return sW[k * kAcLdW + wave * 32 + col]; });
      ac_mma(av[n], 32, li, lh, [&](int row, int k) { return lds[kAcP + k * kAcLd + row]; },
             [&](int k, int col) { return sW[(kAcT + k) * kAcLdW + wave * 32 + col]; });
    }
  }
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int cw = n * kAcWide + wave * 32;
    if (cw >= d) continue;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int row = ac_tile_row(t, lh);
      if (j0 + row >= U) continue;
      const bool live = j0 + row < len;
      dk[(size_t)row * a.ld + cw + li] = live ? ak[n][t] : 0.f;
      dv[(size_t)row * a.ld + cw + li] = live ? av[n][t] : 0.f;
    }
  }
}

// dEp[bh][w][c] = sum over i of dS[i][i - w] q_i[c] for the 32 distances w = w0 .. w0 + 31
__global__ __launch_bounds__(kAcThreads) void attn_causal_bwd_e_k(AttnCausal a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.z, h = blockIdx.y, w0 = blockIdx.x * kAcT, U = a.U, d = a.d, bh = b * a.Hd + h;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int len = a.len[b], rows = min(kAcT, U - w0);
  float* dEp = a.dEp + ((size_t)bh * U + w0) * d;
  if (w0 >= len) {
    ac_zero_rows(dEp, d, rows, d);
    return;
  }
  const float* qb = a.q + (size_t)b * U * a.ld + h * d;
  const float* kb = a.k + (size_t)b * U * a.ld + h * d;
  const float* vb = a.v + (size_t)b * U * a.ld + h * d;
  const float* gb = a.dctx + (size_t)b * U * a.ldc + h * d;
  float* sW = lds + kAcW;
  ac_f32x16 acc[2] = {AC_ZERO16, AC_ZERO16};
  for (int i0 = w0; i0 < len; i0 += kAcT) {
    for (int j0 = i0 - w0 - kAcT; j0 <= i0 - w0; j0 += kAcT) {   // the two key tiles that hold j = i - w
      if (j0 < 0) continue;
      __syncthreads();
      ac_load_rows(a, lds, bh, i0, len);
      ac_grad_tile(a, lds, qb, kb, vb, gb, bh, i0, j0, len);
      const int off = i0 - w0 - j0;   // jj = ii - ww + off
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int c0 = n * kAcWide;
        if (c0 >= d) break;
        if (n) __syncthreads();
        ac_stage_wide(sW, 0, kAcT, qb, a.ld, i0, len, c0, d);
        __syncthreads();
        if (c0 + wave * 32 >= d) continue;
        ac_mma(acc[n], 32, li, lh, [&](int row, int k) { const int jj = k - row + off; return (jj >= 0 && jj < 32) ? lds[kAcD + k * kAcLd + jj] : 0.f; },
               [&](int k, int col) { return sW[k * kAcLdW + wave * 32 + col]; });
      }
    }
  }
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int cw = n * kAcWide + wave * 32;
    if (cw >= d) continue;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int row = ac_tile_row(t, lh);
      if (w0 + row < U) dEp[(size_t)row * d + cw + li] = acc[n][t];
    }
  }
}

// dE[t][c] = the sum over (b, h) ascending of dEp[bh][n0 - t][c]; 0 for the table rows no (i, j) reaches
__global__ __launch_bounds__(kAcThreads) void attn_causal_bwd_e_sum_k(AttnCausal a) {
  const int n = (2 * a.n0 + 1) * a.d, e = blockIdx.x * kAcThreads + threadIdx.x;
  if (e >= n) return;
  const int t = e / a.d, c = e - t * a.d, w = a.n0 - t;
  float s = 0.f;
  if (w >= 0 && w < a.U)
    for (int bh = 0; bh < a.B * a.Hd; ++bh) s += a.dEp[((size_t)bh * a.U + w) * a.d + c];
  a.dE[e] = s;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
static inline size_t ac_bytes(size_t n) { return align_up(n * 4, 256); }

static int ac_check(const w2l_attn_causal_desc* d) {
  if (!d || d->B < 1 || d->Hd < 1 || d->U < 1 || d->d < 1 || d->n0 < 0 || !(d->scale == d->scale) || !(d->dropP >= 0.0 && d->dropP < 1.0))
    return W2L_EINVAL;
  if (d->d % 32 || d->d > kAcMaxD || (long long)d->Hd * d->d > kAcMaxC || d->U > kAcMaxU || d->B > kAcMaxB) return W2L_EUNSUPPORTED;
  if (d->ld < d->Hd * d->d || d->ldc < d->Hd * d->d) return W2L_EINVAL;
  if (d->ld % 4 || d->ldc % 4) return W2L_EUNSUPPORTED;
  return W2L_OK;
}
static bool ac_aligned(std::initializer_list<const void*> ps) {
  uintptr_t x = 0;
  for (const void* p : ps) x |= (uintptr_t)p;
  return (x & 15) == 0;
}
static int ac_len_check(const w2l_attn_causal_desc* d, const int* len) {
  for (int b = 0; b < d->B; ++b)
    if (len[b] < 1 || len[b] > d->U) return W2L_EINVAL;
  return W2L_OK;
}
static AttnCausal ac_args(const w2l_attn_causal_desc* d, const float* q, const float* k, const float* v, const float* E, const void* ws) {
  AttnCausal a{};
  a.q = q; a.k = k; a.v = v; a.E = E; a.len = (const int*)ws;
  a.B = d->B; a.Hd = d->Hd; a.U = d->U; a.d = d->d; a.ld = d->ld; a.ldc = d->ldc; a.n0 = d->n0;
  a.scale = d->scale; a.thr = dropout_threshold(d->dropP); a.keepScale = (float)(1.0 / (1.0 - d->dropP));
  a.seed = d->dropSeed; a.stream = d->dropStream;
  return a;
}
template <class K>
static int ac_opt_in(K kernel, bool (&seen)[64], int wideRows) {
  if (first_on_device(seen)) W2L_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ac_lds_bytes(wideRows)));
  return W2L_OK;
}

#define AC_OK(expr) do { const int _st = (expr); if (_st != W2L_OK) return _st; } while (0)

}  // namespace w2l

using namespace w2l;

// workspace: len [B] ints; backward adds D [B Hd][U] and the table partials [B Hd][U][d]
W2L_API size_t w2l_attn_causal_workspace_size(const w2l_attn_causal_desc* d, int backward) {
  if (ac_check(d) != W2L_OK) return 0;
  const size_t bh = (size_t)d->B * d->Hd;
  return ac_bytes(d->B) + (backward ? ac_bytes(bh * d->U) + ac_bytes(bh * d->U * d->d) : 0);
}

W2L_API int w2l_attn_causal_forward(const w2l_attn_causal_desc* d, const float* q, const float* k, const float* v, const float* E, const int* len,
                                    float* ctx, float* lse, void* workspace, size_t workspaceBytes, w2l_stream_t stream) {
  AC_OK(ac_check(d));
  if (!q || !k || !v || !len || !ctx || !lse || !workspace || workspaceBytes < w2l_attn_causal_workspace_size(d, 0)) return W2L_EINVAL;
  if (!ac_aligned({q, k, v, E, ctx})) return W2L_EUNSUPPORTED;
  AC_OK(ac_len_check(d, len));
  hipStream_t s = (hipStream_t)stream;
  static bool seen[64] = {};
  AC_OK(ac_opt_in(attn_causal_fwd_k, seen, kAcT));
  W2L_HIP_CHECK(hipMemcpyAsync(workspace, len, (size_t)d->B * sizeof(int), hipMemcpyHostToDevice, s));
  AttnCausal a = ac_args(d, q, k, v, E, workspace);
  a.ctx = ctx; a.lse = lse;
  attn_causal_fwd_k<<<dim3((d->U + kAcT - 1) / kAcT, d->Hd, d->B), kAcThreads, ac_lds_bytes(kAcT), s>>>(a);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_attn_causal_backward(const w2l_attn_causal_desc* d, const float* q, const float* k, const float* v, const float* E, const int* len,
                                     const float* lse, const float* dctx, float* dq, float* dk, float* dv, float* dE,
                                     void* workspace, size_t workspaceBytes, w2l_stream_t stream) {
  AC_OK(ac_check(d));
  if (!q || !k || !v || !len || !lse || !dctx || !dq || !dk || !dv || (E && !dE) || !workspace ||
      workspaceBytes < w2l_attn_causal_workspace_size(d, 1))
    return W2L_EINVAL;
  if (!ac_aligned({q, k, v, E, dctx, dq, dk, dv, workspace})) return W2L_EUNSUPPORTED;
  AC_OK(ac_len_check(d, len));
  hipStream_t s = (hipStream_t)stream;
  static bool seenQ[64] = {}, seenKv[64] = {}, seenE[64] = {};
  AC_OK(ac_opt_in(attn_causal_bwd_q_k, seenQ, kAcT + 63));
  AC_OK(ac_opt_in(attn_causal_bwd_kv_k, seenKv, 2 * kAcT));
  AC_OK(ac_opt_in(attn_causal_bwd_e_k, seenE, kAcT));
  W2L_HIP_CHECK(hipMemcpyAsync(workspace, len, (size_t)d->B * sizeof(int), hipMemcpyHostToDevice, s));
  AttnCausal a = ac_args(d, q, k, v, E, workspace);
  a.lseIn = lse; a.dctx = dctx; a.dq = dq; a.dk = dk; a.dv = dv; a.dE = dE;
  a.Dw = (float*)((char*)workspace + ac_bytes(d->B));
  a.dEp = (float*)((char*)a.Dw + ac_bytes((size_t)d->B * d->Hd * d->U));
  const dim3 grid((d->U + kAcT - 1) / kAcT, d->Hd, d->B);
  attn_causal_bwd_q_k<<<grid, kAcThreads, ac_lds_bytes(kAcT + 63), s>>>(a);
  W2L_LAUNCH_CHECK();
  attn_causal_bwd_kv_k<<<grid, kAcThreads, ac_lds_bytes(2 * kAcT), s>>>(a);
  W2L_LAUNCH_CHECK();
  if (E) {
    attn_causal_bwd_e_k<<<grid, kAcThreads, ac_lds_bytes(kAcT), s>>>(a);
    W2L_LAUNCH_CHECK();
    attn_causal_bwd_e_sum_k<<<dim3(((2 * d->n0 + 1) * d->d + kAcThreads - 1) / kAcThreads), kAcThreads, 0, s>>>(a);
    W2L_LAUNCH_CHECK();
  }
  return W2L_OK;
}
