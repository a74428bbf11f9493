// criterion_s2s.hip -- the three kernels groups the teacher-forced seq2seq criterion needs beside the GRU and the Linear products
// (DESIGN 3.34 is the contract): encoder-decoder attention, label-smoothed cross entropy, token embedding.  fp32 throughout.
//
//   attention forward   grid (ceil(U / 32), B), 256 threads.  A workgroup owns 32 queries of ONE utterance and keeps their score rows
//                       S [32][T] in LDS from the first product to the second:
//                         1. S = h k^T on v_mfma_f32_32x32x2_f32: keys stream through LDS in chunks of 128 (wave w owns keys
//                            32 w .. 32 w + 31 of the chunk), the reduction over H in chunks of 32 columns; only keys < keyLen[b];
//                         2. a wave per row: scale, window term from (u, t, keyLen, tgtLen), max, expf, sum (one order), alpha to LDS and
//                            to the result; keys >= keyLen[b] never enter a max or a sum and get probability exactly 0;
//                         3. ctx = alpha v: values stream through LDS in chunks of 32 keys x 128 columns (wave w owns 32 columns), alpha
//                            is the A operand straight from the score rows.
//   attention backward  launch 1, the same ownership and the same two products: dP = dout v^T into LDS, dS = alpha (dP - sum alpha dP)
//                       / sqrt(H) per row (kept in LDS and written to the workspace), dh = dS k.  Launch 2: grid (ceil(T / 32),
//                       ceil(H / 128), B), a workgroup owns 32 KEYS of one utterance and 128 columns and sums over all U in ascending
//                       order: dk = dS^T h, dv = alpha^T dout.  No atomics; dk == dv (content attention) receives the sum.
//   cross entropy       a workgroup per row of z: one pass with an online max / sum and the plain sum of the row, 16 bytes per lane
//                       with a scalar head and tail where the row's phase needs them; per-utterance sums by one thread in row order.
//   embedding           forward: a row gather.  backward: positions grouped by token on the host (a stable counting sort), a workgroup
//                       per row of dE adds its positions in position order; rows nobody names are written as 0.
//
// Every sum has one order, so two calls give the same bits, and nothing an utterance receives depends on B.
// Lengths and tokens are HOST arrays: they are checked before the first launch and copied into the workspace.
#include <algorithm>
#include <vector>

#include "s2s_attn.hpp"

namespace w2l {

constexpr int kS2sMaxU = 512;
constexpr int kXentMaxN = 65536, kS2sMaxRows = kS2sMaxB * kS2sMaxU, kEmbMaxH = 4096;

struct S2sAttn {
  const float *h, *k, *v, *alphaIn, *dout, *dalpha;
  const int *keyLen, *tgtLen;
  float *out, *alpha, *dS, *dh, *dk, *dv;
  int B, U, T, H, ldenc, ldS, window, addQuery;
  float scale, inv2s2;
  bool vecEnc;
};

__global__ __launch_bounds__(kS2sThreads) void s2s_attn_fwd_k(S2sAttn a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* S = lds;
  float* stage = lds + kS2sQt * a.ldS;
  const int b = blockIdx.y, u0 = blockIdx.x * kS2sQt, rows = min(kS2sQt, a.U - u0), H = a.H, T = a.T;
  const int kl = a.keyLen[b], tl = a.tgtLen[b], klp = (kl + 31) & ~31;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* hq = a.h + ((size_t)b * a.U + u0) * H;
  s2s_qk_product(S, a.ldS, stage, hq, H, rows, true, a.k + (size_t)b * T * a.ldenc, a.ldenc, kl, a.vecEnc, H);
  for (int r = wave; r < rows; r += 4) {
    float* row = S + r * a.ldS;
    const int u = u0 + r;
    const bool win = a.window && u < tl;
    const float c = (float)u * (float)kl / (float)tl;
    float m = -INFINITY;
    for (int t = lane; t < kl; t += 64) {
      float s = row[t] * a.scale;
      if (win) { const float d = (float)t - c; s -= d * d * a.inv2s2; }
      row[t] = s;
      m = fmaxf(m, s);
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int t = lane; t < kl; t += 64) { const float e = expf(row[t] - m); row[t] = e; sum += e; }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    float* ao = a.alpha + ((size_t)b * a.U + u) * T;
    for (int t = lane; t < max(T, klp); t += 64) {
      const float p = t < kl ? row[t] * inv : 0.f;
      if (t < klp) row[t] = p;
      if (t < T) ao[t] = p;
    }
  }
  for (int r = rows + wave; r < kS2sQt; r += 4)   // queries past U: their rows feed the product, nothing is kept of them
    for (int t = lane; t < klp; t += 64) S[r * a.ldS + t] = 0.f;
  __syncthreads();
  float* out = a.out + ((size_t)b * a.U + u0) * H;
  const bool addq = a.addQuery != 0;
  s2s_pv_product(S, a.ldS, stage, a.v + (size_t)b * T * a.ldenc, a.ldenc, kl, a.vecEnc, H, [&](int r, int c, float x) {
    if (r < rows) out[(size_t)r * H + c] = addq ? hq[(size_t)r * H + c] + x : x;
  });
}

__global__ __launch_bounds__(kS2sThreads) void s2s_attn_bwd_q_k(S2sAttn a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* S = lds;
  float* stage = lds + kS2sQt * a.ldS;
  const int b = blockIdx.y, u0 = blockIdx.x * kS2sQt, rows = min(kS2sQt, a.U - u0), H = a.H, T = a.T;
  const int kl = a.keyLen[b], klp = (kl + 31) & ~31;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* dq = a.dout + ((size_t)b * a.U + u0) * H;
  s2s_qk_product(S, a.ldS, stage, dq, H, rows, true, a.v + (size_t)b * T * a.ldenc, a.ldenc, kl, a.vecEnc, H);
  for (int r = wave; r < kS2sQt; r += 4) {
    float* row = S + r * a.ldS;
    if (r >= rows) {
      for (int t = lane; t < klp; t += 64) row[t] = 0.f;
      continue;
    }
    const size_t at = ((size_t)b * a.U + u0 + r) * T;
    const float* al = a.alphaIn + at;
    float dot = 0.f;
    for (int t = lane; t < kl; t += 64) {
      float dp = row[t];
      if (a.dalpha) dp += a.dalpha[at + t];
      row[t] = dp;
      dot += al[t] * dp;
    }
    dot = wave_sum(dot);
    for (int t = lane; t < max(T, klp); t += 64) {
      const float ds = t < kl ? al[t] * (row[t] - dot) * a.scale : 0.f;
      if (t < klp) row[t] = ds;
      if (t < T) a.dS[at + t] = ds;
    }
  }
  __syncthreads();
  float* dh = a.dh + ((size_t)b * a.U + u0) * H;
  const bool addq = a.addQuery != 0;
  s2s_pv_product(S, a.ldS, stage, a.k + (size_t)b * T * a.ldenc, a.ldenc, kl, a.vecEnc, H, [&](int r, int c, float x) {
    if (r < rows) dh[(size_t)r * H + c] = addq ? dq[(size_t)r * H + c] + x : x;
  });
}

// dk[t][c] = sum_u dS[u][t] h[u][c], dv[t][c] = sum_u alpha[u][t] dout[u][c]: 32 keys x 128 columns of one utterance, u ascending
__global__ __launch_bounds__(kS2sThreads) void s2s_attn_bwd_kv_k(S2sAttn a) {
  __shared__ __attribute__((aligned(16))) float sA[2][kS2sQt * kS2sLdc];   // [u][t]: dS, alpha
  __shared__ __attribute__((aligned(16))) float sB[2][kS2sQt * kS2sLdv];   // [u][c]: h, dout
  const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 128, H = a.H, T = a.T, U = a.U;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int kl = a.keyLen[b], cw = c0 + wave * 32;
  s2s_f32x16 ak = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, av = ak;
  if (t0 < kl) {   // block-uniform: a chunk of masked keys receives zeros
    const float* src[2] = {a.h + (size_t)b * U * H, a.dout + (size_t)b * U * H};
    const float* pa[2] = {a.dS + (size_t)b * U * T, a.alphaIn + (size_t)b * U * T};
    for (int u0 = 0; u0 < U; u0 += 32) {
      __syncthreads();
#pragma unroll
      for (int w = 0; w < 2; ++w) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + i * kS2sThreads, r = e >> 5, c = e & 31;
          sA[w][r * kS2sLdc + c] = (u0 + r < U && t0 + c < T) ? pa[w][(size_t)(u0 + r) * T + t0 + c] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + i * kS2sThreads, r = e >> 5, c = (e & 31) * 4;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (u0 + r < U && c0 + c < H) v = *reinterpret_cast<const float4*>(src[w] + (size_t)(u0 + r) * H + c0 + c);
          *reinterpret_cast<float4*>(&sB[w][r * kS2sLdv + c]) = v;
        }
      }
      __syncthreads();
      if (cw >= H) continue;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int kk = it * 8 + lh * 4;
        const float* p0 = &sA[0][kk * kS2sLdc + li];
        const float* p1 = &sA[1][kk * kS2sLdc + li];
        const float* q0 = &sB[0][kk * kS2sLdv + wave * 32 + li];
        const float* q1 = &sB[1][kk * kS2sLdv + wave * 32 + li];
        const float4 a0 = make_float4(p0[0], p0[kS2sLdc], p0[2 * kS2sLdc], p0[3 * kS2sLdc]);
        const float4 a1 = make_float4(p1[0], p1[kS2sLdc], p1[2 * kS2sLdc], p1[3 * kS2sLdc]);
        const float4 b0 = make_float4(q0[0], q0[kS2sLdv], q0[2 * kS2sLdv], q0[3 * kS2sLdv]);
        const float4 b1 = make_float4(q1[0], q1[kS2sLdv], q1[2 * kS2sLdv], q1[3 * kS2sLdv]);
        S2S_MFMA4(ak, a0, b0);
        S2S_MFMA4(av, a1, b1);
      }
    }
  }
  if (cw >= H) return;
  const bool joint = a.dk == a.dv;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = t0 + s2s_tile_row(r, lh);
    if (t >= T) continue;
    const size_t at = ((size_t)b * T + t) * a.ldenc + cw + li;
    if (joint) a.dk[at] = ak[r] + av[r];
    else { a.dk[at] = ak[r]; a.dv[at] = av[r]; }
  }
}

// ---- cross entropy ----------------------------------------------------------------------------------------------------------------------
// online softmax statistics of a part of a row: max m, sum of exp(x - m), plain sum
struct XentAcc { float m, s, z; };
__device__ __forceinline__ void xent_add4(XentAcc& a, float4 x) {
  const float m4 = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
  if (m4 > a.m) { a.s *= expf(a.m - m4); a.m = m4; }
  a.s += (expf(x.x - a.m) + expf(x.y - a.m)) + (expf(x.z - a.m) + expf(x.w - a.m));
  a.z += (x.x + x.y) + (x.z + x.w);
}
__device__ __forceinline__ void xent_add1(XentAcc& a, float x) {
  if (x > a.m) { a.s *= expf(a.m - x); a.m = x; }
  a.s += expf(x - a.m);
  a.z += x;
}
// a part that saw nothing has m = -inf, s = 0: it must not produce -inf - -inf
__device__ __forceinline__ XentAcc xent_merge(XentAcc a, XentAcc b) {
  const float m = fmaxf(a.m, b.m);
  XentAcc r;
  r.m = m;
  r.s = (a.s > 0.f ? a.s * expf(a.m - m) : 0.f) + (b.s > 0.f ? b.s * expf(b.m - m) : 0.f);
  r.z = a.z + b.z;
  return r;
}

// the elements of a row that lie before its first 16-byte boundary (at most 3, at most N)
__device__ __forceinline__ int xent_head(const float* row, int N) { return min(N, (int)((4 - (((uintptr_t)row >> 2) & 3)) & 3)); }

__global__ __launch_bounds__(kS2sThreads) void xent_fwd_k(const float* z, const int* target, float* lse, float* rowLoss, int N, float eps) {
  __shared__ XentAcc part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t m = blockIdx.x;
  const float* row = z + m * N;
  const int head = xent_head(row, N), nv = (N - head) >> 2, tail = head + nv * 4;
  XentAcc a{-INFINITY, 0.f, 0.f};
  if (tid < head) xent_add1(a, row[tid]);
  const float4* body = reinterpret_cast<const float4*>(row + head);
  for (int i = tid; i < nv; i += kS2sThreads) xent_add4(a, body[i]);
  if (tail + tid < N) xent_add1(a, row[tail + tid]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    XentAcc o{__shfl_down(a.m, off), __shfl_down(a.s, off), __shfl_down(a.z, off)};
    a = xent_merge(a, o);
  }
  if (lane == 0) part[wave] = a;
  __syncthreads();
  if (tid == 0) {
    a = xent_merge(xent_merge(part[0], part[1]), xent_merge(part[2], part[3]));
    const float l = a.m + logf(a.s);
    lse[m] = l;
    const int y = target[m];
    // (1 - eps) (lse - z_y) - (eps / N) (sum_c z_c - N lse)
    rowLoss[m] = y < 0 ? 0.f : (float)((1.0 - (double)eps) * ((double)l - (double)row[y]) - (double)eps / N * ((double)a.z - (double)N * (double)l));
  }
}

__global__ void xent_utt_k(const float* rowLoss, const int* uttStart, float* loss, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int m = uttStart[b]; m < uttStart[b + 1]; ++m) s += (double)rowLoss[m];
  loss[b] = (float)s;
}

__global__ __launch_bounds__(kS2sThreads) void xent_bwd_k(const float* z, const float* lse, const int* target, const int* rowUtt, const float* g,
                                                          float* dz, int N, float eps) {
  const int tid = threadIdx.x;
  const size_t m = blockIdx.x;
  const float* row = z + m * N;
  float* out = dz + m * N;
  const int y = target[m];
  const bool valid = y >= 0;
  const float gm = valid ? g[rowUtt[m]] : 0.f, l = lse[m], sm = eps / (float)N, hit = 1.f - eps;
  auto one = [&](float x, int c) { return valid ? gm * ((expf(x - l) - (c == y ? hit : 0.f)) - sm) : 0.f; };
  const bool same = (((uintptr_t)row ^ (uintptr_t)out) & 15) == 0;   // one phase: both rows take 16 bytes per lane
  const int head = same ? xent_head(row, N) : N, nv = (N - head) >> 2, tail = head + nv * 4;
  for (int c = tid; c < head; c += kS2sThreads) out[c] = one(row[c], c);
  const float4* body = reinterpret_cast<const float4*>(row + head);
  float4* obody = reinterpret_cast<float4*>(out + head);
  for (int i = tid; i < nv; i += kS2sThreads) {
    const float4 x = body[i];
    const int c = head + 4 * i;
    obody[i] = make_float4(one(x.x, c), one(x.y, c + 1), one(x.z, c + 2), one(x.w, c + 3));
  }
  if (tail + tid < N) out[tail + tid] = one(row[tail + tid], tail + tid);
}

// ---- embedding ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kS2sThreads) void emb_fwd_k(const int* tokens, const float* E, const float* start, float* x, int H, bool vec) {
  const size_t m = blockIdx.x;
  const int tok = tokens[m];
  const float* src = tok < 0 ? start : E + (size_t)tok * H;
  float* dst = x + m * H;
  if (vec) {
    for (int c = threadIdx.x; c < (H >> 2); c += kS2sThreads) reinterpret_cast<float4*>(dst)[c] = reinterpret_cast<const float4*>(src)[c];
  } else {
    for (int c = threadIdx.x; c < H; c += kS2sThreads) dst[c] = src[c];
  }
}

// row r < N of dE, row N = the start embedding: the positions perm[rowStart[r] .. rowStart[r + 1]) in ascending order
__global__ __launch_bounds__(kS2sThreads) void emb_bwd_k(const int* rowStart, const int* perm, const float* dx, float* dE, float* dstart, int N, int H) {
  const int r = blockIdx.x, lo = rowStart[r], hi = rowStart[r + 1];
  float* dst = r < N ? dE + (size_t)r * H : dstart;
  for (int c = threadIdx.x; c < H; c += kS2sThreads) {
    float s = 0.f;
    for (int i = lo; i < hi; ++i) s += dx[(size_t)perm[i] * H + c];
    dst[c] = s;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
static inline size_t s2s_ints(size_t n) { return align_up(n * sizeof(int), 256); }

static int s2s_attn_check(const w2l_s2s_attn_desc* d) {
  if (!d || d->B < 1 || d->U < 1 || d->T < 1 || d->H < 1 || d->ldenc < d->H || !(d->windowStd == d->windowStd)) return W2L_EINVAL;
  if (d->H % 32 || d->H > kS2sMaxH || d->T > kS2sMaxT || d->U > kS2sMaxU || d->B > kS2sMaxB) return W2L_EUNSUPPORTED;
  return W2L_OK;
}
static int s2s_len_check(const w2l_s2s_attn_desc* d, const int* keyLen, const int* tgtLen) {
  for (int b = 0; b < d->B; ++b)
    if (keyLen[b] < 1 || keyLen[b] > d->T || tgtLen[b] < 1 || tgtLen[b] > d->U) return W2L_EINVAL;
  return W2L_OK;
}

static S2sAttn s2s_attn_args(const w2l_s2s_attn_desc* d, const float* h, const float* k, const float* v, const int* lens) {
  S2sAttn a{};
  a.h = h; a.k = k; a.v = v; a.keyLen = lens; a.tgtLen = lens + d->B;
  a.B = d->B; a.U = d->U; a.T = d->T; a.H = d->H; a.ldenc = d->ldenc; a.ldS = s2s_lds_stride(d->T);
  a.window = d->windowStd > 0.f; a.addQuery = d->addQuery;
  a.scale = (float)(1.0 / sqrt((double)d->H));
  a.inv2s2 = a.window ? (float)(1.0 / (2.0 * (double)d->windowStd * (double)d->windowStd)) : 0.f;
  a.vecEnc = d->ldenc % 4 == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0;
  return a;
}

static int s2s_upload_lens(const w2l_s2s_attn_desc* d, const int* keyLen, const int* tgtLen, void* ws, hipStream_t s) {
  W2L_HIP_CHECK(hipMemcpyAsync(ws, keyLen, (size_t)d->B * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipMemcpyAsync((int*)ws + d->B, tgtLen, (size_t)d->B * sizeof(int), hipMemcpyHostToDevice, s));
  return W2L_OK;
}

template <class K>
static int s2s_lds_opt_in(K kernel, bool (&seen)[64]) {   // the score rows of T = 1024 pass 64 KiB
  if (first_on_device(seen)) W2L_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s2s_lds_bytes(kS2sMaxT)));
  return W2L_OK;
}

// rowUtt of every row and the first row of every utterance; 0 ok
static int xent_rows(int M, int N, int B, const int* target, const int* rowUtt, std::vector<int>& utt, std::vector<int>& start) {
  utt.resize(M);
  start.assign(B + 1, 0);
  if (!rowUtt && M % B) return W2L_EINVAL;
  int prev = 0;
  for (int m = 0; m < M; ++m) {
    if (target[m] < -1 || target[m] >= N) return W2L_EINVAL;
    const int b = rowUtt ? rowUtt[m] : m / (M / B);
    if (b < prev || b >= B) return W2L_EINVAL;   // rows of an utterance are contiguous, utterances ascending
    utt[m] = prev = b;
    ++start[b + 1];
  }
  for (int b = 0; b < B; ++b) start[b + 1] += start[b];
  return W2L_OK;
}
static int xent_check(int M, int N, int B) {
  if (M < 1 || N < 1 || B < 1) return W2L_EINVAL;
  if (N > kXentMaxN || M > kS2sMaxRows || B > kS2sMaxB) return W2L_EUNSUPPORTED;
  return W2L_OK;
}
// workspace: target [M], rowUtt [M], uttStart [B + 1] ints, rowLoss [M] floats
struct XentWs { size_t target, utt, start, rowLoss, total; };
static XentWs xent_ws(int M, int B) {
  XentWs w;
  w.target = 0; w.utt = s2s_ints(M); w.start = w.utt + s2s_ints(M); w.rowLoss = w.start + s2s_ints(B + 1);
  w.total = w.rowLoss + s2s_ints(M);
  return w;
}

static int emb_check(int M, int N, int H) {
  if (M < 1 || N < 1 || H < 1) return W2L_EINVAL;
  if (N > kXentMaxN || M > kS2sMaxRows || H > kEmbMaxH) return W2L_EUNSUPPORTED;
  return W2L_OK;
}
static int emb_tokens_check(int M, int N, const int* tokens) {
  for (int m = 0; m < M; ++m)
    if (tokens[m] < -1 || tokens[m] >= N) return W2L_EINVAL;
  return W2L_OK;
}
// workspace: tokens [M], rowStart [N + 2], perm [M] ints
struct EmbWs { size_t tokens, rowStart, perm, total; };
static EmbWs emb_ws(int M, int N) {
  EmbWs w;
  w.tokens = 0; w.rowStart = s2s_ints(M); w.perm = w.rowStart + s2s_ints((size_t)N + 2); w.total = w.perm + s2s_ints(M);
  return w;
}

#define S2S_OK(expr) do { const int _st = (expr); if (_st != W2L_OK) return _st; } while (0)

}  // namespace w2l

using namespace w2l;

W2L_API size_t w2l_s2s_attn_workspace_size(const w2l_s2s_attn_desc* d, int backward) {
  if (s2s_attn_check(d) != W2L_OK) return 0;
  return s2s_ints(2 * (size_t)d->B) + (backward ? align_up((size_t)d->B * d->U * d->T * sizeof(float), 256) : 0);
}

W2L_API int w2l_s2s_attn_forward(const w2l_s2s_attn_desc* d, const float* h, const float* k, const float* v, const int* keyLen, const int* tgtLen,
                                 float* out, float* alpha, void* workspace, size_t workspaceBytes, w2l_stream_t stream) {
  S2S_OK(s2s_attn_check(d));
  if (!h || !k || !v || !keyLen || !tgtLen || !out || !alpha || !workspace || workspaceBytes < w2l_s2s_attn_workspace_size(d, 0) ||
      !s2s_aligned(h, out))
    return W2L_EINVAL;
  S2S_OK(s2s_len_check(d, keyLen, tgtLen));
  hipStream_t s = (hipStream_t)stream;
  static bool seen[64] = {};
  const size_t lds = s2s_lds_bytes(d->T);
  S2S_OK(s2s_lds_opt_in(s2s_attn_fwd_k, seen));
  S2S_OK(s2s_upload_lens(d, keyLen, tgtLen, workspace, s));
  S2sAttn a = s2s_attn_args(d, h, k, v, (const int*)workspace);
  a.out = out; a.alpha = alpha;
  s2s_attn_fwd_k<<<dim3((d->U + kS2sQt - 1) / kS2sQt, d->B), kS2sThreads, lds, s>>>(a);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_s2s_attn_backward(const w2l_s2s_attn_desc* d, const float* h, const float* k, const float* v, const int* keyLen, const int* tgtLen,
                                  const float* alpha, const float* dout, const float* dalpha, float* dh, float* dk, float* dv, void* workspace,
                                  size_t workspaceBytes, w2l_stream_t stream) {
  S2S_OK(s2s_attn_check(d));
  if (!h || !k || !v || !keyLen || !tgtLen || !alpha || !dout || !dh || !dk || !dv || !workspace ||
      workspaceBytes < w2l_s2s_attn_workspace_size(d, 1) || !s2s_aligned(h, dout, dh, workspace))
    return W2L_EINVAL;
  S2S_OK(s2s_len_check(d, keyLen, tgtLen));
  hipStream_t s = (hipStream_t)stream;
  static bool seen[64] = {};
  const size_t lds = s2s_lds_bytes(d->T);
  S2S_OK(s2s_lds_opt_in(s2s_attn_bwd_q_k, seen));
  S2S_OK(s2s_upload_lens(d, keyLen, tgtLen, workspace, s));
  S2sAttn a = s2s_attn_args(d, h, k, v, (const int*)workspace);
  a.alphaIn = alpha; a.dout = dout; a.dalpha = dalpha; a.dh = dh; a.dk = dk; a.dv = dv;
  a.dS = (float*)((char*)workspace + s2s_ints(2 * (size_t)d->B));
  s2s_attn_bwd_q_k<<<dim3((d->U + kS2sQt - 1) / kS2sQt, d->B), kS2sThreads, lds, s>>>(a);
  W2L_LAUNCH_CHECK();
  s2s_attn_bwd_kv_k<<<dim3((d->T + 31) / 32, (d->H + 127) / 128, d->B), kS2sThreads, 0, s>>>(a);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API size_t w2l_s2s_xent_workspace_size(int M, int B) {
  if (M < 1 || B < 1 || M > kS2sMaxRows || B > kS2sMaxB) return 0;
  return xent_ws(M, B).total;
}

W2L_API int w2l_s2s_xent_forward(int M, int N, int B, const float* z, const int* target, const int* rowUtt, float eps, float* lse, float* loss,
                                 void* workspace, size_t workspaceBytes, w2l_stream_t stream) {
  S2S_OK(xent_check(M, N, B));
  if (!z || !target || !lse || !loss || !workspace || !(eps >= 0.f && eps < 1.f) || workspaceBytes < xent_ws(M, B).total) return W2L_EINVAL;
  std::vector<int> utt, start;
  S2S_OK(xent_rows(M, N, B, target, rowUtt, utt, start));
  hipStream_t s = (hipStream_t)stream;
  const XentWs w = xent_ws(M, B);
  char* ws = (char*)workspace;
  W2L_HIP_CHECK(hipMemcpyAsync(ws + w.target, target, (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipMemcpyAsync(ws + w.utt, utt.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipMemcpyAsync(ws + w.start, start.data(), (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipStreamSynchronize(s));   // the two vectors above die with this call
  xent_fwd_k<<<M, kS2sThreads, 0, s>>>(z, (const int*)(ws + w.target), lse, (float*)(ws + w.rowLoss), N, eps);
  W2L_LAUNCH_CHECK();
  xent_utt_k<<<(B + 63) / 64, 64, 0, s>>>((const float*)(ws + w.rowLoss), (const int*)(ws + w.start), loss, B);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_s2s_xent_backward(int M, int N, int B, const float* z, const float* lse, const int* target, const int* rowUtt, float eps,
                                  const float* g, float* dz, void* workspace, size_t workspaceBytes, w2l_stream_t stream) {
  S2S_OK(xent_check(M, N, B));
  if (!z || !lse || !target || !g || !dz || !workspace || !(eps >= 0.f && eps < 1.f) || workspaceBytes < xent_ws(M, B).total) return W2L_EINVAL;
  std::vector<int> utt, start;
  S2S_OK(xent_rows(M, N, B, target, rowUtt, utt, start));
  hipStream_t s = (hipStream_t)stream;
  const XentWs w = xent_ws(M, B);
  char* ws = (char*)workspace;
  W2L_HIP_CHECK(hipMemcpyAsync(ws + w.target, target, (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipMemcpyAsync(ws + w.utt, utt.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipStreamSynchronize(s));
  xent_bwd_k<<<M, kS2sThreads, 0, s>>>(z, lse, (const int*)(ws + w.target), (const int*)(ws + w.utt), g, dz, N, eps);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API size_t w2l_embedding_workspace_size(int M, int N) {
  if (M < 1 || N < 1 || M > kS2sMaxRows || N > kXentMaxN) return 0;
  return emb_ws(M, N).total;
}

W2L_API int w2l_embedding_forward(int M, int N, int H, const int* tokens, const float* E, const float* start, float* x, void* workspace,
                                  size_t workspaceBytes, w2l_stream_t stream) {
  S2S_OK(emb_check(M, N, H));
  if (!tokens || !E || !start || !x || !workspace || workspaceBytes < emb_ws(M, N).total) return W2L_EINVAL;
  S2S_OK(emb_tokens_check(M, N, tokens));
  hipStream_t s = (hipStream_t)stream;
  W2L_HIP_CHECK(hipMemcpyAsync(workspace, tokens, (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  const bool vec = H % 4 == 0 && (((uintptr_t)E | (uintptr_t)start | (uintptr_t)x) & 15) == 0;
  emb_fwd_k<<<M, kS2sThreads, 0, s>>>((const int*)workspace, E, start, x, H, vec);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_embedding_backward(int M, int N, int H, const int* tokens, const float* dx, float* dE, float* dstart, void* workspace,
                                   size_t workspaceBytes, w2l_stream_t stream) {
  S2S_OK(emb_check(M, N, H));
  if (!tokens || !dx || !dE || !dstart || !workspace || workspaceBytes < emb_ws(M, N).total) return W2L_EINVAL;
  S2S_OK(emb_tokens_check(M, N, tokens));
  // positions grouped by row (token, or N for the start embedding), ascending inside a row: a stable counting sort
  std::vector<int> rowStart((size_t)N + 2, 0), perm(M);
  for (int m = 0; m < M; ++m) ++rowStart[(tokens[m] < 0 ? N : tokens[m]) + 1];
  for (int r = 0; r <= N; ++r) rowStart[r + 1] += rowStart[r];
  std::vector<int> at(rowStart.begin(), rowStart.end() - 1);
  for (int m = 0; m < M; ++m) perm[at[tokens[m] < 0 ? N : tokens[m]]++] = m;
  hipStream_t s = (hipStream_t)stream;
  const EmbWs w = emb_ws(M, N);
  char* ws = (char*)workspace;
  W2L_HIP_CHECK(hipMemcpyAsync(ws + w.rowStart, rowStart.data(), rowStart.size() * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipMemcpyAsync(ws + w.perm, perm.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  W2L_HIP_CHECK(hipStreamSynchronize(s));   // the two vectors above die with this call
  emb_bwd_k<<<N + 1, kS2sThreads, 0, s>>>((const int*)(ws + w.rowStart), (const int*)(ws + w.perm), dx, dE, dstart, N, H);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
