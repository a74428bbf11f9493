// local_norm.hip -- LocalNorm, the windowed feature normalisation of the streaming recipe, batch and streaming form.
//
// Reference: recipes/streaming_convnets/inference/inference/module/nn/LocalNorm.cpp keeps the sum and the sum of squares of every
// frame, normalises frame t with ONE mean and deviation over all features of frames t - L .. t and replaces a deviation at or
// below 1e-5 by 1.  The contract here (include/w2l_hip.h) is that window with an optional right context R, in double:
//
//   1. frame sums    s_u = sum_f x[f][u], q_u = sum_f x[f][u]^2, f ascending
//   2. window sums   S = sum_{u = lo..hi} s_u, Q likewise, u ascending, summed DIRECTLY (no differences of prefix sums: their
//                    roundings would depend on where the utterance began, and a frame's result must be a function of its window)
//   3. moments       mean = S / cnt, var = max(Q / cnt - mean^2, 0), sd = sqrt(var), sd <= 1e-5f -> 1
//   4. output        y = (x - (float)mean) * (float)(1 / sd), one fp32 subtract and one fp32 multiply
//
// Features are [rows][F][ld] with time fastest, so FRAMES SIT ON LANES: the F loads of a frame are one coalesced row of the wave
// each, a lane walks its own frame's features upward and nothing is reduced across lanes, waves or workgroups.  The four steps are
// the four device functions below; both forms call them, which is what makes the session equal the batch call bit for bit:
//
//   batch    local_norm_sums_k   one thread per frame: step 1 -> workspace [B][T] of (s, q)
//            local_norm_apply_k  one thread per frame: steps 2-4 (the sums are complete before the first store: y may be x)
//   session  norm_stream_k       one workgroup per slot, one launch per step: step 1 of the slot's new frames into the slot's ring
//                                (the last L frames stay where they are: the ring holds L + maxChunk pairs), a barrier, steps 2-4
//
// Loads and stores of steps 1 and 4 go in blocks of kLnBlock: all loads of a block are issued before the first use / store (a
// rolled load -> store loop keeps one access per lane in flight, stores count in vmcnt: DESIGN 7 (iv)).
#include "common.hpp"

#include <string>

namespace w2l {
void setHostError(const std::string& m);   // w2l_host_last_error's message (host/trainer.cpp)

constexpr int kLnThreads = 256;
constexpr int kLnBlock = 8;

// step 1 for the frame whose feature 0 is at x, features ld floats apart
__device__ __forceinline__ double2 ln_frame_sums(const float* __restrict__ x, int F, size_t ld) {
  double s = 0.0, q = 0.0;
  int f = 0;
  for (; f + kLnBlock <= F; f += kLnBlock) {
    float v[kLnBlock];
#pragma unroll
    for (int u = 0; u < kLnBlock; ++u) v[u] = x[(size_t)(f + u) * ld];
#pragma unroll
    for (int u = 0; u < kLnBlock; ++u) {
      const double d = (double)v[u];
      s += d;
      q += d * d;
    }
  }
  for (; f < F; ++f) {
    const double d = (double)x[(size_t)f * ld];
    s += d;
    q += d * d;
  }
  return make_double2(s, q);
}

// step 2: the sum of `count` pairs from sq[first] upward; RING: the index wraps at cap
template <bool RING>
__device__ __forceinline__ double2 ln_window_sums(const double2* __restrict__ sq, int first, int count, int cap) {
  double S = 0.0, Q = 0.0;
  int i = first;
#pragma unroll 4
  for (int k = 0; k < count; ++k) {
    const double2 v = sq[i];
    S += v.x;
    Q += v.y;
    ++i;
    if (RING && i == cap) i = 0;
  }
  return make_double2(S, Q);
}

// step 3: m = (float)mean, r = (float)(1 / sd) of a window of `frames` frames
__device__ __forceinline__ void ln_moments(double2 SQ, int frames, int F, float& m, float& r) {
  const double cnt = (double)frames * (double)F;
  const double mean = SQ.x / cnt;
  double var = SQ.y / cnt - mean * mean;
  if (var < 0.0) var = 0.0;
  double sd = sqrt(var);
  if (sd <= (double)1e-5f) sd = 1.0;
  m = (float)mean;
  r = (float)(1.0 / sd);
}

// step 4 for one frame
__device__ __forceinline__ void ln_apply(const float* x, size_t ldx, float* y, size_t ldy, int F, float m, float r) {
  int f = 0;
  for (; f + kLnBlock <= F; f += kLnBlock) {
    float v[kLnBlock];
#pragma unroll
    for (int u = 0; u < kLnBlock; ++u) v[u] = x[(size_t)(f + u) * ldx];
#pragma unroll
    for (int u = 0; u < kLnBlock; ++u) y[(size_t)(f + u) * ldy] = (v[u] - m) * r;
  }
  for (; f < F; ++f) y[(size_t)f * ldy] = (x[(size_t)f * ldx] - m) * r;
}

__device__ __forceinline__ int ln_frames_of(const int* __restrict__ frames, int b, int T) {
  return frames ? min(max(frames[b], 0), T) : T;
}

// grid = B x tiles of kLnThreads frames (flat: B is not bounded by the grid's y limit)
__global__ __launch_bounds__(kLnThreads) void local_norm_sums_k(const float* __restrict__ x, size_t ldx, int F, int T, int tiles,
                                                              const int* __restrict__ frames, double2* __restrict__ ws) {
  const int b = blockIdx.x / tiles, t = (blockIdx.x % tiles) * kLnThreads + threadIdx.x;
  if (t >= ln_frames_of(frames, b, T)) return;
  ws[(size_t)b * T + t] = ln_frame_sums(x + (size_t)b * F * ldx + t, F, ldx);
}

// x and y may be the same array: a thread reads and writes its own frame only, the sums it reads are the first launch's
__global__ __launch_bounds__(kLnThreads) void local_norm_apply_k(const float* x, size_t ldx, float* y, size_t ldy, int F, int T, int tiles,
                                                               const int* __restrict__ frames, int left, int right,
                                                               const double2* __restrict__ ws) {
  const int b = blockIdx.x / tiles, t = (blockIdx.x % tiles) * kLnThreads + threadIdx.x;
  const int n = ln_frames_of(frames, b, T);
  if (t >= n) return;
  const int lo = t > left ? t - left : 0;                  // left, right <= 65535: no overflow
  const int hi = right < n - 1 - t ? t + right : n - 1;
  float m, r;
  ln_moments(ln_window_sums<false>(ws + (size_t)b * T, lo, hi - lo + 1, 0), hi - lo + 1, F, m, r);
  ln_apply(x + (size_t)b * F * ldx + t, ldx, y + (size_t)b * F * ldy + t, ldy, F, m, r);
}

// tab[s] = {ring position of the slot's first new frame, new frames, min(frames so far, L), unused}: host arithmetic.  One workgroup
// per slot: the new frames' pairs go into the ring behind the old ones (cap = L + maxChunk: none of the last L is overwritten), then
// frame j's window is the min(L, have + j) + 1 pairs that end at its own.
__global__ __launch_bounds__(kLnThreads) void norm_stream_k(const float* x, size_t ld, float* y, size_t ldy, int F, int L, int cap,
                                                          const int* __restrict__ tab, double2* ring) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const int pos = tab[4 * s], n = tab[4 * s + 1], have = tab[4 * s + 2];
  if (n <= 0 || n > cap - L || pos < 0 || pos >= cap || have < 0 || have > L) return;   // nothing to do / not a table the host wrote
  double2* rg = ring + (size_t)s * cap;
  const float* xs = x + (size_t)s * F * ld;
  float* ys = y + (size_t)s * F * ldy;
  for (int j = tid; j < n; j += kLnThreads) {
    int i = pos + j;
    if (i >= cap) i -= cap;
    rg[i] = ln_frame_sums(xs + j, F, ld);
  }
  __syncthreads();   // the pairs written above are read by the other threads of this workgroup
  for (int j = tid; j < n; j += kLnThreads) {
    const int w = min(L, have + j) + 1;
    int first = pos + j - (w - 1);
    if (first < 0) first += cap;
    if (first >= cap) first -= cap;
    float m, r;
    ln_moments(ln_window_sums<true>(rg, first, w, cap), w, F, m, r);
    ln_apply(xs + j, ld, ys + j, ldy, F, m, r);
  }
}

// the session step's launch (host/norm_stream.cpp validates)
int norm_stream_launch(const float* x, size_t ld, float* y, size_t ldy, int F, int L, int cap, const int* tab, void* ring, int slots,
                       hipStream_t stream) {
  hipLaunchKernelGGL(norm_stream_k, dim3((unsigned)slots), dim3(kLnThreads), 0, stream, x, ld, y, ldy, F, L, cap, tab, (double2*)ring);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

static int ln_refuse(int status, const std::string& m) {
  setHostError(m);
  return status;
}

}  // namespace w2l

using namespace w2l;

W2L_API size_t w2l_local_norm_workspace_size(int B, int T) {
  if (B < 1 || T < 1) return 0;
  return (size_t)B * (size_t)T * 2 * sizeof(double);
}

W2L_API int w2l_local_norm(int B, int F, int T, size_t ldx, const float* x, const int* frames, int left, int right, size_t ldy, float* y,
                           void* workspace, w2l_stream_t stream) {
  if (B < 1 || F < 1 || T < 1) return ln_refuse(W2L_EINVAL, "local norm: B, F and T must be positive");
  if (left < 0 || right < 0) return ln_refuse(W2L_EINVAL, "local norm: the context sizes left and right must not be negative");
  if (ldx < (size_t)T || ldy < (size_t)T) return ln_refuse(W2L_EINVAL, "local norm: ldx and ldy must be at least T");
  if (!x || !y || !workspace) return ln_refuse(W2L_EINVAL, "local norm: null pointer (x, y or workspace)");
  if ((uintptr_t)workspace & 15) return ln_refuse(W2L_EINVAL, "local norm: the workspace must be 16-byte aligned");
  if ((long long)left + right + 1 > 65536)
    return ln_refuse(W2L_EUNSUPPORTED, "local norm: a window of left + right + 1 = " + std::to_string((long long)left + right + 1) + " frames is above 65536");
  if (F > 4096) return ln_refuse(W2L_EUNSUPPORTED, "local norm: F " + std::to_string(F) + " is above 4096");
  // in place means the same array: any other overlap would let one frame's store land under another frame's load
  if (!((const float*)y == x && ldy == ldx)) {
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (((size_t)B * F - 1) * ldx + T) * sizeof(float);
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (((size_t)B * F - 1) * ldy + T) * sizeof(float);
    if (x0 < y1 && y0 < x1) return ln_refuse(W2L_EINVAL, "local norm: x and y overlap partially (in place needs y == x and ldy == ldx)");
  }
  const int tiles = (T + kLnThreads - 1) / kLnThreads;
  if ((long long)B * tiles > 0x7fffffffLL) return ln_refuse(W2L_EUNSUPPORTED, "local norm: B x ceil(T / 256) is above 2^31 - 1");
  const dim3 grid((unsigned)((long long)B * tiles));
  hipLaunchKernelGGL(local_norm_sums_k, grid, dim3(kLnThreads), 0, (hipStream_t)stream, x, ldx, F, T, tiles, frames, (double2*)workspace);
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(local_norm_apply_k, grid, dim3(kLnThreads), 0, (hipStream_t)stream, x, ldx, y, ldy, F, T, tiles, frames, left, right,
                     (const double2*)workspace);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
