// criterion_cpc.hip -- the CPC contrastive criterion: span mask with a learned embedding, two projections into a common
// space, InfoNCE of every masked frame against negatives drawn from the other masked frames of its utterance.
//
// Reference: recipes/joint_training_vox_populi/cpc/CPCCriterion.cpp:85-223.  The contract is in include/w2l_hip.h; which frames are
// masked and which negatives are drawn is host logic (include/fl_compat/cpc.h), the device sees maskIndex [B][M] and neg [B][M][K].
//
// THE SHAPE: dense, deterministic, no atomics.  With R = B M masked rows:
//   forward   cpc_gather_k      the masked rows of enc and ctx -> xe [R][Ce], xc [R][Cc]
//             2 products        p = xe We^T + be, a = xc Wc^T + bc                       (w2l_gemm_f32, all utterances in one product)
//             cpc_normalize_k   one wave per row: row / |row| in place, 1 / |row| kept for the backward pass
//             B products        S_b = a_b p_b^T   [M][M]: every anchor against every candidate of its utterance
//             cpc_rows_k<0>     one workgroup per (b, m): the K + 1 logits S_b[m][m] / tau, S_b[m][neg] / tau, log-sum-exp, the row's term
//             cpc_loss_k        one workgroup per utterance: the M terms in a fixed order / M
//   backward  cpc_rows_k<1>     the same logits again; the coefficient row G[m][:] is built in LDS -- zero-filled, softmax_0 - 1 on
//                               column m, softmax_k on column neg[m][k], added in k order by ONE lane so that repeated negatives add
//                               in a fixed order -- scaled by g[b] / (M tau) and written to G_b (S_b stays: a second backward call
//                               on the same workspace gives the same bits)
//             2 B products      da_b = G_b p_b, dp_b = G_b^T a_b
//             cpc_normalize_bwd_k  one wave per row: dx = (dy - y <dy, y>) / |x|
//             4 products + 2 column sums   dxe = dp We, dWe = dp^T xe, dbe = sum_r dp; the same for the context side
//             cpc_scatter_k     one workgroup per frame (b, t): a binary search of t in maskIndex[b]; the frame's gradient row or zeros
// A fused gather-dot kernel would read K + 1 rows of D floats per anchor (R (K + 1) D loads, 40 x the dense block's traffic at the
// recipe's K = 100, D = 256) and its backward would have to add several anchors' terms into one candidate's row: atomics or a sort.
// The dense block turns both into products the MFMA kernels already do, and the sparsity into a row kernel that touches K + 1 floats.
//
// The products follow w2l_set_matmul_precision like every w2l_gemm_f32 call (fp32 unless the caller switched the process to bf16).
#include "common.hpp"

#include <cmath>
#include <string>

namespace w2l {
void setHostError(const std::string& m);   // w2l_host_last_error's message (host/trainer.cpp)

constexpr int kCpcThreads = 256;
constexpr int kCpcWaves = kCpcThreads / kWave;
constexpr int kCpcMaskChunk = 64;          // rows per partial sum of the mask embedding's gradient
constexpr size_t kCpcLdsFloats = 16000;    // cpc_rows_k<1>: M + 2 (K + 1) floats of LDS, below the 64 KiB a kernel gets without opt-in

struct CpcWs {
  size_t xe, xc, p, a, rinv, S, terms, G, dp, da, dxe, dxc, total;   // offsets in floats
};

static size_t cpc_take(size_t& at, size_t floats) {
  const size_t o = at;
  at += align_up(floats, 64);   // 256-byte regions: every operand of a product is 16-byte aligned
  return o;
}

// p and a are ONE region of 2 R rows, as are dp and da and the inverse norms: the row kernels walk both sides in one launch
static bool cpc_layout(int B, int T, int Ce, int Cc, int D, int M, int K, CpcWs& w) {
  if (B < 1 || T < 1 || Ce < 1 || Cc < 1 || D < 1 || M < 1 || M > T || K < 1 || K > M) return false;
  const size_t R = (size_t)B * M, big = (size_t)1 << 31;
  if ((size_t)M + 2 * ((size_t)K + 1) > kCpcLdsFloats) return false;
  if (R * Ce >= big || R * Cc >= big || 2 * R * D >= big || R * M >= big || (size_t)B * T >= big) return false;   // int dims of the products
  size_t at = 0;
  w.xe = cpc_take(at, R * Ce);
  w.xc = cpc_take(at, R * Cc);
  w.p = cpc_take(at, R * D);
  w.a = cpc_take(at, R * D);
  w.rinv = cpc_take(at, 2 * R);
  w.S = cpc_take(at, R * M);
  w.terms = cpc_take(at, R);
  w.G = cpc_take(at, R * M);
  w.dp = cpc_take(at, R * D);
  w.da = cpc_take(at, R * D);
  w.dxe = cpc_take(at, R * Ce);
  w.dxc = cpc_take(at, R * Cc);
  w.total = at;
  return true;
}

// ---- block reductions in a fixed order: DPP inside a wave, the four wave results through LDS, the same sum in every thread
__device__ __forceinline__ float cpc_block_max(float v, float* sm) {
  v = wave_max(v);
  __syncthreads();   // sm may still be read from the previous reduction
  if (lane_id() == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}
__device__ __forceinline__ float cpc_block_sum(float v, float* sm) {
  v = wave_sum(v);
  __syncthreads();
  if (lane_id() == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__device__ __forceinline__ int cpc_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one workgroup per masked row r = b M + m: xe[r] = enc[b][maskIndex[r]], xc[r] = ctx[b][maskIndex[r]] (an index outside [0, T) is
// outside the contract: the row is zeros, nothing outside the operands is read)
__global__ __launch_bounds__(kCpcThreads) void cpc_gather_k(const float* __restrict__ enc, const float* __restrict__ ctx,
                                                          const int* __restrict__ maskIndex, int T, int Ce, int Cc, int M,
                                                          float* __restrict__ xe, float* __restrict__ xc) {
  const size_t r = blockIdx.x;
  const int b = (int)(r / (size_t)M), t = maskIndex[r];
  const bool ok = t >= 0 && t < T;
  const size_t row = (size_t)b * T + (ok ? t : 0);
  for (int c = threadIdx.x; c < Ce; c += kCpcThreads) xe[r * Ce + c] = ok ? enc[row * Ce + c] : 0.f;
  for (int c = threadIdx.x; c < Cc; c += kCpcThreads) xc[r * Cc + c] = ok ? ctx[row * Cc + c] : 0.f;
}

// one wave per row of x [rows][D]: x /= |x| (no epsilon, as the reference: a zero row is outside the contract), rinv = 1 / |x|
__global__ __launch_bounds__(kCpcThreads) void cpc_normalize_k(float* __restrict__ x, float* __restrict__ rinv, size_t rows, int D) {
  const size_t r = (size_t)blockIdx.x * kCpcWaves + (threadIdx.x >> 6);
  if (r >= rows) return;   // wave-uniform: the DPP reduction below runs with all 64 lanes
  float* xr = x + r * D;
  float ss = 0.f;
  for (int d = lane_id(); d < D; d += kWave) ss += xr[d] * xr[d];
  const float n = sqrtf(wave_sum(ss));
  for (int d = lane_id(); d < D; d += kWave) xr[d] = xr[d] / n;
  if (lane_id() == 0) rinv[r] = 1.0f / n;
}

// y = x / |x|: dx = (dy - y <dy, y>) / |x|, in place on dy
__global__ __launch_bounds__(kCpcThreads) void cpc_normalize_bwd_k(const float* __restrict__ y, const float* __restrict__ rinv,
                                                                 float* __restrict__ dy, size_t rows, int D) {
  const size_t r = (size_t)blockIdx.x * kCpcWaves + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* yr = y + r * D;
  float* gr = dy + r * D;
  float dot = 0.f;
  for (int d = lane_id(); d < D; d += kWave) dot += gr[d] * yr[d];
  dot = wave_sum(dot);
  const float ri = rinv[r];
  for (int d = lane_id(); d < D; d += kWave) gr[d] = (gr[d] - yr[d] * dot) * ri;
}

// the column of logit k of row m: 0 is the positive (column m), 1 + k the negative neg[k] (clamped into [0, M): a value outside is
// outside the contract, nothing outside S is read)
__device__ __forceinline__ int cpc_col(const int* __restrict__ neg, int k, int m, int M) {
  return k == 0 ? m : cpc_clampi(neg[k - 1], 0, M - 1);
}

// one workgroup per (b, m).  BWD = 0: terms[r] = logsumexp_k s_k - s_0.  BWD = 1: G[r][:] as described at the top of the file.
template <int BWD>
__global__ __launch_bounds__(kCpcThreads) void cpc_rows_k(const float* __restrict__ S, const int* __restrict__ neg, int M, int K, float tau,
                                                        float* __restrict__ terms, const float* __restrict__ g, float* __restrict__ G) {
  extern __shared__ float lds[];   // BWD: row [M], coef [K + 1], col [K + 1]
  __shared__ float sm[kCpcWaves];
  const size_t r = blockIdx.x;
  const int b = (int)(r / (size_t)M), m = (int)(r % (size_t)M), tid = threadIdx.x;
  const float* Sr = S + r * M;
  const int* nr = neg + r * K;
  float mx = -INFINITY;
  for (int k = tid; k <= K; k += kCpcThreads) mx = fmaxf(mx, Sr[cpc_col(nr, k, m, M)] / tau);
  mx = cpc_block_max(mx, sm);
  float se = 0.f;
  for (int k = tid; k <= K; k += kCpcThreads) se += expf(Sr[cpc_col(nr, k, m, M)] / tau - mx);
  se = cpc_block_sum(se, sm);
  if (!BWD) {
    if (tid == 0) terms[r] = (mx + logf(se)) - Sr[m] / tau;
    return;
  }
  float* row = lds;
  float* coef = lds + M;
  int* col = (int*)(lds + M + K + 1);
  for (int j = tid; j < M; j += kCpcThreads) row[j] = 0.f;
  for (int k = tid; k <= K; k += kCpcThreads) {
    const int j = cpc_col(nr, k, m, M);
    col[k] = j;
    coef[k] = expf(Sr[j] / tau - mx) / se - (k == 0 ? 1.0f : 0.0f);
  }
  __syncthreads();
  if (tid == 0)
    for (int k = 0; k <= K; ++k) row[col[k]] += coef[k];   // one lane, k ascending: repeats add in a fixed order
  __syncthreads();
  const float scale = g[b] / ((float)M * tau);
  float* Gr = G + r * M;
  for (int j = tid; j < M; j += kCpcThreads) Gr[j] = row[j] * scale;
}

// one workgroup per utterance: thread i adds terms i, i + 256, ... upward, the 256 partial sums fold in a fixed tree
__global__ __launch_bounds__(kCpcThreads) void cpc_loss_k(const float* __restrict__ terms, int M, float* __restrict__ loss) {
  __shared__ float sm[kCpcThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (int m = tid; m < M; m += kCpcThreads) s += terms[(size_t)b * M + m];
  sm[tid] = s;
  __syncthreads();
  for (int h = kCpcThreads / 2; h > 0; h >>= 1) {
    if (tid < h) sm[tid] += sm[tid + h];
    __syncthreads();
  }
  if (tid == 0) loss[b] = sm[0] / (float)M;
}

// one workgroup per frame (b, t): masked frames take their gradient row, every other frame is written as zeros
__global__ __launch_bounds__(kCpcThreads) void cpc_scatter_k(const float* __restrict__ dxe, const float* __restrict__ dxc,
                                                           const int* __restrict__ maskIndex, int T, int Ce, int Cc, int M,
                                                           float* __restrict__ denc, float* __restrict__ dctx) {
  const size_t f = blockIdx.x;
  const int b = (int)(f / (size_t)T), t = (int)(f % (size_t)T);
  const int* idx = maskIndex + (size_t)b * M;
  int lo = 0, hi = M;   // the first position whose index is >= t (the row is strictly ascending)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (idx[mid] < t) lo = mid + 1; else hi = mid;
  }
  const bool hit = lo < M && idx[lo] == t;
  const size_t r = (size_t)b * M + (hit ? lo : 0);
  for (int c = threadIdx.x; c < Ce; c += kCpcThreads) denc[f * Ce + c] = hit ? dxe[r * Ce + c] : 0.f;
  for (int c = threadIdx.x; c < Cc; c += kCpcThreads) dctx[f * Cc + c] = hit ? dxc[r * Cc + c] : 0.f;
}

// y[b][t][:] = mask[b][t] ? emb : x[b][t][:], one workgroup per frame
__global__ __launch_bounds__(kCpcThreads) void cpc_apply_mask_k(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ emb, int C, float* __restrict__ y) {
  const size_t f = blockIdx.x;
  const bool m = mask[f] != 0;
  for (int c = threadIdx.x; c < C; c += kCpcThreads) y[f * C + c] = m ? emb[c] : x[f * C + c];
}

// grid (chunks of kCpcMaskChunk frames, tiles of 256 channels): dx = mask ? 0 : dy, part[chunk][c] = the chunk's masked dy rows added
// upward
__global__ __launch_bounds__(kCpcThreads) void cpc_mask_bwd_k(const float* __restrict__ dy, const uint8_t* __restrict__ mask, size_t frames,
                                                            int C, float* __restrict__ dx, float* __restrict__ part) {
  const int c = blockIdx.y * kCpcThreads + threadIdx.x;
  if (c >= C) return;
  const size_t f0 = (size_t)blockIdx.x * kCpcMaskChunk;
  const size_t f1 = f0 + kCpcMaskChunk < frames ? f0 + kCpcMaskChunk : frames;
  float s = 0.f;
  for (size_t f = f0; f < f1; ++f) {
    const float v = dy[f * C + c];
    const bool m = mask[f] != 0;
    dx[f * C + c] = m ? 0.f : v;
    if (m) s += v;
  }
  part[(size_t)blockIdx.x * C + c] = s;
}

// demb[c] = the chunks' partial sums added upward
__global__ __launch_bounds__(kCpcThreads) void cpc_mask_fold_k(const float* __restrict__ part, int chunks, int C, float* __restrict__ demb) {
  const int c = blockIdx.x * kCpcThreads + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int i = 0; i < chunks; ++i) s += part[(size_t)i * C + c];
  demb[c] = s;
}

static int cpc_refuse(int status, const std::string& m) {
  setHostError(m);
  return status;
}

// the refusals the forward and the backward call share; W2L_OK: `w` is the workspace's layout
static int cpc_check(int B, int T, int Ce, int Cc, int D, int M, int K, float tau, const void* workspace, CpcWs& w) {
  if (B < 1 || T < 1 || Ce < 1 || Cc < 1) return cpc_refuse(W2L_EINVAL, "cpc: B, T, Ce and Cc must be positive");
  if (D < 1) return cpc_refuse(W2L_EINVAL, "cpc: D must be positive");
  if (M < 1 || M > T) return cpc_refuse(W2L_EINVAL, "cpc: M = " + std::to_string(M) + " is outside 1 .. T");
  if (K < 1 || K > M) return cpc_refuse(W2L_EINVAL, "cpc: K = " + std::to_string(K) + " is outside 1 .. M");
  if (!(tau > 0.f) || !std::isfinite(tau)) return cpc_refuse(W2L_EINVAL, "cpc: the temperature must be positive and finite");
  if (!workspace) return cpc_refuse(W2L_EINVAL, "cpc: null pointer (workspace)");
  if ((uintptr_t)workspace & 15) return cpc_refuse(W2L_EINVAL, "cpc: the workspace must be 16-byte aligned");
  if (!cpc_layout(B, T, Ce, Cc, D, M, K, w))
    return cpc_refuse(W2L_EUNSUPPORTED, "cpc: M + 2 (K + 1) is above " + std::to_string(kCpcLdsFloats) + ", or an operand has 2^31 elements or more");
  return W2L_OK;
}

}  // namespace w2l

using namespace w2l;

#define CPC_TRY(expr)               \
  do {                              \
    const int _st = (expr);         \
    if (_st != W2L_OK) return _st;  \
  } while (0)

W2L_API size_t w2l_cpc_workspace_size(int B, int T, int Ce, int Cc, int D, int M, int K) {
  CpcWs w;
  if (!cpc_layout(B, T, Ce, Cc, D, M, K, w)) return 0;
  return w.total * sizeof(float);
}

W2L_API size_t w2l_cpc_mask_workspace_size(int B, int T, int C) {
  if (B < 1 || T < 1 || C < 1) return 0;
  const size_t chunks = ((size_t)B * T + kCpcMaskChunk - 1) / kCpcMaskChunk;
  return chunks * (size_t)C * sizeof(float);
}

W2L_API int w2l_cpc_forward(int B, int T, int Ce, int Cc, int D, int M, int K, float tau, const float* enc, const float* ctx,
                            const int* maskIndex, const int* neg, const float* We, const float* be, const float* Wc, const float* bc,
                            float* loss, void* workspace, w2l_stream_t stream) {
  if (!enc || !ctx || !maskIndex || !neg || !We || !be || !Wc || !bc || !loss)
    return cpc_refuse(W2L_EINVAL, "cpc forward: null pointer");
  CpcWs w;
  CPC_TRY(cpc_check(B, T, Ce, Cc, D, M, K, tau, workspace, w));
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int R = B * M;
  hipLaunchKernelGGL(cpc_gather_k, dim3((unsigned)R), dim3(kCpcThreads), 0, s, enc, ctx, maskIndex, T, Ce, Cc, M, ws + w.xe, ws + w.xc);
  W2L_LAUNCH_CHECK();
  CPC_TRY(w2l_gemm_f32(R, D, Ce, ws + w.xe, Ce, 1, We, Ce, 1, ws + w.p, D, be, 0, 1, stream));
  CPC_TRY(w2l_gemm_f32(R, D, Cc, ws + w.xc, Cc, 1, Wc, Cc, 1, ws + w.a, D, bc, 0, 1, stream));
  const unsigned rowGrid = (unsigned)((R + kCpcWaves - 1) / kCpcWaves);
  hipLaunchKernelGGL(cpc_normalize_k, dim3(rowGrid), dim3(kCpcThreads), 0, s, ws + w.p, ws + w.rinv, (size_t)R, D);
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(cpc_normalize_k, dim3(rowGrid), dim3(kCpcThreads), 0, s, ws + w.a, ws + w.rinv + R, (size_t)R, D);
  W2L_LAUNCH_CHECK();
  for (int b = 0; b < B; ++b) {
    const size_t o = (size_t)b * M;
    CPC_TRY(w2l_gemm_f32(M, M, D, ws + w.a + o * D, D, 1, ws + w.p + o * D, D, 1, ws + w.S + o * M, M, nullptr, 0, 1, stream));
  }
  hipLaunchKernelGGL(cpc_rows_k<0>, dim3((unsigned)R), dim3(kCpcThreads), 0, s, ws + w.S, neg, M, K, tau, ws + w.terms, (const float*)nullptr,
                     (float*)nullptr);
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(cpc_loss_k, dim3((unsigned)B), dim3(kCpcThreads), 0, s, ws + w.terms, M, loss);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_cpc_backward(int B, int T, int Ce, int Cc, int D, int M, int K, float tau, const int* maskIndex, const int* neg,
                             const float* We, const float* Wc, const float* g, float* denc, float* dctx, float* dWe, float* dbe,
                             float* dWc, float* dbc, void* workspace, w2l_stream_t stream) {
  if (!maskIndex || !neg || !We || !Wc || !g || !denc || !dctx || !dWe || !dbe || !dWc || !dbc)
    return cpc_refuse(W2L_EINVAL, "cpc backward: null pointer");
  CpcWs w;
  CPC_TRY(cpc_check(B, T, Ce, Cc, D, M, K, tau, workspace, w));
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int R = B * M;
  const size_t lds = ((size_t)M + 2 * ((size_t)K + 1)) * sizeof(float);
  hipLaunchKernelGGL(cpc_rows_k<1>, dim3((unsigned)R), dim3(kCpcThreads), lds, s, ws + w.S, neg, M, K, tau, (float*)nullptr, g, ws + w.G);
  W2L_LAUNCH_CHECK();
  for (int b = 0; b < B; ++b) {
    const size_t o = (size_t)b * M;
    // da_b [M][D] = G_b [M][M] p_b [M][D];  dp_b [M][D] = G_b^T a_b
    CPC_TRY(w2l_gemm_f32(M, D, M, ws + w.G + o * M, M, 1, ws + w.p + o * D, D, 0, ws + w.da + o * D, D, nullptr, 0, 1, stream));
    CPC_TRY(w2l_gemm_f32(M, D, M, ws + w.G + o * M, M, 0, ws + w.a + o * D, D, 0, ws + w.dp + o * D, D, nullptr, 0, 1, stream));
  }
  const unsigned rowGrid = (unsigned)((R + kCpcWaves - 1) / kCpcWaves);
  hipLaunchKernelGGL(cpc_normalize_bwd_k, dim3(rowGrid), dim3(kCpcThreads), 0, s, ws + w.p, ws + w.rinv, ws + w.dp, (size_t)R, D);
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(cpc_normalize_bwd_k, dim3(rowGrid), dim3(kCpcThreads), 0, s, ws + w.a, ws + w.rinv + R, ws + w.da, (size_t)R, D);
  W2L_LAUNCH_CHECK();
  // dxe [R][Ce] = dp [R][D] We [D][Ce];  dWe [D][Ce] = dp^T xe;  dbe [D] = the column sums of dp
  CPC_TRY(w2l_gemm_f32(R, Ce, D, ws + w.dp, D, 1, We, Ce, 0, ws + w.dxe, Ce, nullptr, 0, 1, stream));
  CPC_TRY(w2l_gemm_f32(D, Ce, R, ws + w.dp, D, 0, ws + w.xe, Ce, 0, dWe, Ce, nullptr, 0, 1, stream));
  CPC_TRY(w2l_colsum(ws + w.dp, dbe, (size_t)R, D, stream));
  CPC_TRY(w2l_gemm_f32(R, Cc, D, ws + w.da, D, 1, Wc, Cc, 0, ws + w.dxc, Cc, nullptr, 0, 1, stream));
  CPC_TRY(w2l_gemm_f32(D, Cc, R, ws + w.da, D, 0, ws + w.xc, Cc, 0, dWc, Cc, nullptr, 0, 1, stream));
  CPC_TRY(w2l_colsum(ws + w.da, dbc, (size_t)R, D, stream));
  hipLaunchKernelGGL(cpc_scatter_k, dim3((unsigned)((size_t)B * T)), dim3(kCpcThreads), 0, s, ws + w.dxe, ws + w.dxc, maskIndex, T, Ce, Cc, M,
                     denc, dctx);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_cpc_apply_mask(int B, int T, int C, const float* x, const unsigned char* mask, const float* emb, float* y,
                               w2l_stream_t stream) {
  if (B < 1 || T < 1 || C < 1) return cpc_refuse(W2L_EINVAL, "cpc mask: B, T and C must be positive");
  if (!x || !mask || !emb || !y) return cpc_refuse(W2L_EINVAL, "cpc mask: null pointer");
  if ((size_t)B * T >= ((size_t)1 << 31)) return cpc_refuse(W2L_EUNSUPPORTED, "cpc mask: B T is 2^31 or more");
  hipLaunchKernelGGL(cpc_apply_mask_k, dim3((unsigned)((size_t)B * T)), dim3(kCpcThreads), 0, (hipStream_t)stream, x, mask, emb, C, y);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_cpc_apply_mask_backward(int B, int T, int C, const float* dy, const unsigned char* mask, float* dx, float* demb,
                                        void* workspace, w2l_stream_t stream) {
  if (B < 1 || T < 1 || C < 1) return cpc_refuse(W2L_EINVAL, "cpc mask backward: B, T and C must be positive");
  if (!dy || !mask || !dx || !demb || !workspace) return cpc_refuse(W2L_EINVAL, "cpc mask backward: null pointer");
  if ((size_t)B * T >= ((size_t)1 << 31)) return cpc_refuse(W2L_EUNSUPPORTED, "cpc mask backward: B T is 2^31 or more");
  const size_t frames = (size_t)B * T;
  const int chunks = (int)((frames + kCpcMaskChunk - 1) / kCpcMaskChunk), tiles = (C + kCpcThreads - 1) / kCpcThreads;
  if (tiles > 65535) return cpc_refuse(W2L_EUNSUPPORTED, "cpc mask backward: C is above 65535 x 256");
  hipLaunchKernelGGL(cpc_mask_bwd_k, dim3((unsigned)chunks, (unsigned)tiles), dim3(kCpcThreads), 0, (hipStream_t)stream, dy, mask, frames, C,
                     dx, (float*)workspace);
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(cpc_mask_fold_k, dim3((unsigned)tiles), dim3(kCpcThreads), 0, (hipStream_t)stream, (const float*)workspace, chunks, C, demb);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
