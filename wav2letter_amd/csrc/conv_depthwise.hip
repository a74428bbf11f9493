// conv_depthwise.hip -- depthwise kw x 1 convolutions over time (fl::Conv2D with groups == nIn == nOut; arch line
// `C c c kw 1 pad 1 bias c`, cpc/SequentialBuilder.cpp:203-252): the convolution of the Conformer's conv module.
//
//   forward          y[b][t][h][c]  = bias[c] + sum_k w[k][c] x[b][t - padl + k][h][c]
//   backward data    dx[b][t][h][c] = sum_k w[kw-1-k][c] dy[b][t - (kw-1-padl) + k][h][c]      (the same kernel, filter reversed)
//   backward filter  dw[k][c] = sum_{b,t,h} dy[b][t][h][c] x[b][t - padl + k][h][c],   dbias[c] = sum dy
//
// x [B][T][H][C], y / dy [B][To][H][C], w [kw][C], stride 1.  Nothing here is a matrix product -- at kw = 31 an element costs
// 62 flops against 8 bytes of traffic -- so there is no MFMA and no bf16 form; the work is organised around the memory system:
//
//   * a frame is F = H C contiguous floats and a column f of it carries channel f % C, so H needs no code of its own;
//   * lanes sit on columns: a workgroup of 256 threads owns (utterance, chunk of 32 output frames -- 16 above kw = 32 --, tile of 256 columns) and
//     every global access of a wave is whole contiguous rows;
//   * the chunk and its kw - 1 halo frames are staged in LDS once, as float4 rows where the frames are 16-byte aligned (F % 4 == 0
//     and an aligned base) and column by column otherwise; frames outside the utterance and columns beyond F are zeros there, so
//     the inner loops carry no bounds checks.  All of a thread's staging loads are independent of each other: the bulk of the
//     traffic is in flight at once, and a second workgroup on the CU computes meanwhile (at most 63 KiB of LDS up to kw = 32, 79 KiB above: two fit a CU's 160 KiB);
//   * a lane keeps its column's kw taps in registers for the launch and produces runs of kDwRun consecutive frames from a register
//     window of kDwRun + kw - 1 staged values, read from LDS with consecutive lanes on consecutive words (conflict-free): a staged
//     value is read (kDwRun + kw - 1) / kDwRun times, not kw times;
//   * an output is ONE chain of fmaf over k ascending that starts at the bias: its bits depend on its own window only, not on
//     where a chunk boundary fell (a zero-filled tap adds an exact zero);
//   * the loops are unrolled for kw classes 8 / 16 / 32 / 64; inside a class the taps k >= kw are skipped by a wave-uniform test.
//
// The filter gradient is the same walk with kw + 1 accumulators per lane (the last is the bias gradient): the (utterance, chunk)
// items of a column tile are cut into S contiguous segments, a workgroup walks one segment and leaves its sums in
// part[s][kw + 1][F]; a second launch adds the S partials of every (k, c), and the H columns of a channel, in a fixed order in
// double.  No atomics: two runs give the same bits.
#include <algorithm>

#include "common.hpp"

namespace w2l {

constexpr int kDwThreads = 256;     // = columns of a tile
constexpr int kDwChunk = 32;        // output frames of a workgroup ...
constexpr int kDwChunkWide = 16;    // ... and above kw = 32, where 32 frames and the halo would leave a CU's LDS to ONE workgroup
static inline int dw_chunk(int kw) { return kw > 32 ? kDwChunkWide : kDwChunk; }   // both multiples of kDwRun
constexpr int kDwRun = 8;           // consecutive output frames from one register window
constexpr int kDwMaxKw = 64;
constexpr int kDwMaxSegments = 128;   // the reduce reads S (kw + 1) F floats: 8 MiB at kw = 31, F = 512

// frames [f0, f0 + nf) of one utterance `in` [Tin][F], columns [c0, c0 + 256) -> lds[nf][256]; zeros outside the utterance / frame
__device__ __forceinline__ void dw_stage(float* lds, const float* __restrict__ in, int Tin, int F, int f0, int nf, int c0, int vec) {
  const int tid = threadIdx.x;
  if (vec) {   // a wave loads one 1 KiB row
    const int q = tid & 63, col = c0 + 4 * q;
    const bool colOk = col < F;   // F % 4 == 0: a float4 is inside or outside as a whole
#pragma unroll 4
    for (int j = tid >> 6; j < nf; j += kDwThreads / 64) {
      const int t = f0 + j;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (colOk && t >= 0 && t < Tin) v = *(const float4*)(in + (size_t)t * F + col);
      *(float4*)(lds + j * kDwThreads + 4 * q) = v;
    }
  } else {
    const int col = c0 + tid;
#pragma unroll 8
    for (int j = 0; j < nf; ++j) {
      const int t = f0 + j;
      float v = 0.f;
      if (col < F && t >= 0 && t < Tin) v = in[(size_t)t * F + col];
      lds[j * kDwThreads + tid] = v;
    }
  }
}

// the register window of a run that starts at staged frame r0
template <int KWC>
__device__ __forceinline__ void dw_window(const float* lds, int r0, int kw, float (&win)[kDwRun + KWC - 1]) {
#pragma unroll
  for (int j = 0; j < kDwRun + KWC - 1; ++j) win[j] = j < kDwRun + kw - 1 ? lds[(r0 + j) * kDwThreads + threadIdx.x] : 0.f;
}

// out[b][t][f] = bias[f % C] + sum_k tap_k in[b][t - padl + k][f],  tap_k = w[k] (forward) or w[kw - 1 - k] (`reverse`: data gradient)
template <int KWC>
__global__ __launch_bounds__(kDwThreads) void dw_conv_k(const float* __restrict__ in, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out, int Tin, int Tout, int F,
                                                        int C, int kw, int padl, int reverse, int vec, int chunk) {
  extern __shared__ float lds[];   // [chunk + kw - 1][256]
  const int tid = threadIdx.x, c0 = blockIdx.x * kDwThreads, t0 = blockIdx.y * chunk, b = blockIdx.z;
  const int col = c0 + tid;
  const bool live = col < F;
  const int ch = live ? col % C : 0;
  float tap[KWC];
#pragma unroll
  for (int k = 0; k < KWC; ++k) tap[k] = (live && k < kw) ? w[(size_t)(reverse ? kw - 1 - k : k) * C + ch] : 0.f;
  const float init = (bias && live) ? bias[ch] : 0.f;
  dw_stage(lds, in + (size_t)b * Tin * F, Tin, F, t0 - padl, chunk + kw - 1, c0, vec);
  __syncthreads();
  if (!live) return;
  const int nOut = min(chunk, Tout - t0);
  float* o = out + ((size_t)b * Tout + t0) * F + col;
#pragma unroll 1
  for (int r0 = 0; r0 < nOut; r0 += kDwRun) {
    float win[kDwRun + KWC - 1];
    dw_window<KWC>(lds, r0, kw, win);
    float acc[kDwRun];
#pragma unroll
    for (int r = 0; r < kDwRun; ++r) acc[r] = init;
#pragma unroll
    for (int k = 0; k < KWC; ++k) {
      if (k < kw) {
#pragma unroll
        for (int r = 0; r < kDwRun; ++r) acc[r] = fmaf(tap[k], win[k + r], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kDwRun; ++r)
      if (r0 + r < nOut) o[(size_t)(r0 + r) * F] = acc[r];
  }
}

// part[s][k][f] = sum over the items of segment s of dy[b][t][f] x[b][t - padl + k][f]  (k < kw),  part[s][kw][f] = sum dy
template <int KWC>
__global__ __launch_bounds__(kDwThreads) void dw_filter_k(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
                                                          int T, int To, int F, int kw, int padl, int chunks, int items, int S, int vec, int chunk) {
  extern __shared__ float lds[];   // [chunk + kw - 1][256]
  const int tid = threadIdx.x, c0 = blockIdx.x * kDwThreads, s = blockIdx.y;
  const int col = c0 + tid;
  const bool live = col < F;
  float acc[KWC], accB = 0.f;
#pragma unroll
  for (int k = 0; k < KWC; ++k) acc[k] = 0.f;
  const int i0 = (int)((long long)s * items / S), i1 = (int)((long long)(s + 1) * items / S);
#pragma unroll 1
  for (int it = i0; it < i1; ++it) {
    const int b = it / chunks, t0 = (it - b * chunks) * chunk;
    dw_stage(lds, x + (size_t)b * T * F, T, F, t0 - padl, chunk + kw - 1, c0, vec);
    __syncthreads();
    if (live) {
      const int nOut = min(chunk, To - t0);
      const float* g = dy + ((size_t)b * To + t0) * F + col;
#pragma unroll 1
      for (int r0 = 0; r0 < nOut; r0 += kDwRun) {
        float d[kDwRun];
#pragma unroll
        for (int r = 0; r < kDwRun; ++r) d[r] = r0 + r < nOut ? g[(size_t)(r0 + r) * F] : 0.f;
        float win[kDwRun + KWC - 1];
        dw_window<KWC>(lds, r0, kw, win);
#pragma unroll
        for (int k = 0; k < KWC; ++k) {
          if (k < kw) {
#pragma unroll
            for (int r = 0; r < kDwRun; ++r) acc[k] = fmaf(d[r], win[k + r], acc[k]);
          }
        }
#pragma unroll
        for (int r = 0; r < kDwRun; ++r) accB += d[r];
      }
    }
    __syncthreads();   // the next item's staging overwrites the window
  }
  if (!live) return;
  float* p = part + (size_t)s * (kw + 1) * F + col;
#pragma unroll
  for (int k = 0; k < KWC; ++k)
    if (k < kw) p[(size_t)k * F] = acc[k];
  p[(size_t)kw * F] = accB;
}

// dw[k][c] = sum over the S H partials part[s][k][h C + c], in double; row kw is the bias gradient.  A workgroup owns 64 consecutive
// (k, c) and its four waves every fourth partial each, four loads in flight per lane (one lane walking all S partials alone waits
// for S round trips to memory: 50 us at S = 128); the four sums meet in LDS and are added in wave order -- a fixed order throughout.
constexpr int kDwReduceCols = 64, kDwReduceWays = kDwThreads / kDwReduceCols, kDwReduceBatch = 4;
__global__ __launch_bounds__(kDwThreads) void dw_filter_reduce_k(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ dbias,
                                                                 int S, int H, int C, int kw) {
  __shared__ double red[kDwReduceWays][kDwReduceCols];
  const int lane = threadIdx.x & (kDwReduceCols - 1), way = threadIdx.x / kDwReduceCols;
  const int idx = blockIdx.x * kDwReduceCols + lane;
  const bool live = idx < (kw + 1) * C;
  const int k = live ? idx / C : 0, c = live ? idx - k * C : 0;
  const size_t F = (size_t)H * C, rowStride = (size_t)(kw + 1) * F;
  const int n = S * H;   // partial j: segment j / H, row j % H
  double sum = 0.0;
  if (live) {
    for (int j0 = way; j0 < n; j0 += kDwReduceWays * kDwReduceBatch) {
      float v[kDwReduceBatch];
#pragma unroll
      for (int u = 0; u < kDwReduceBatch; ++u) {
        const int j = j0 + u * kDwReduceWays;
        v[u] = j < n ? part[(size_t)(j / H) * rowStride + (size_t)k * F + (size_t)(j % H) * C + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kDwReduceBatch; ++u) sum += (double)v[u];
    }
  }
  red[way][lane] = sum;
  __syncthreads();
  if (!live || way) return;
#pragma unroll
  for (int q = 1; q < kDwReduceWays; ++q) sum += red[q][lane];
  if (k < kw) dw[idx] = (float)sum;
  else if (dbias) dbias[c] = (float)sum;
}

struct DwGeom {
  int To, F, tiles, chunk, chunks, items, S;
  size_t ldsBytes;
};

// W2L_OK and the geometry, or the refusal
static int dw_geom(const w2l_conv_desc* d, DwGeom& g) {
  if (!d || d->B < 1 || d->T < 1 || d->H < 1 || d->Cin < 1 || d->Cout < 1 || d->kw < 1 || d->stride < 1 || d->padl < 0 || d->padr < 0) return W2L_EINVAL;
  if (d->Cin != d->Cout || d->stride != 1 || d->kw > kDwMaxKw) return W2L_EUNSUPPORTED;
  const long long To = (long long)d->T + d->padl + d->padr - d->kw + 1, F = (long long)d->H * d->Cin;
  if (To < 1) return W2L_EINVAL;
  const long long frames = std::max<long long>(To, d->T);
  g.chunk = dw_chunk(d->kw);
  const long long chunks = (frames + g.chunk - 1) / g.chunk;   // of the longer side: forward walks To, the data gradient T
  if (F > (1 << 24) || chunks > 65535 || d->B > 65535 || (long long)d->padl + d->padr + d->kw > (1 << 24)) return W2L_EUNSUPPORTED;
  g.To = (int)To; g.F = (int)F;
  g.tiles = (int)((F + kDwThreads - 1) / kDwThreads);
  g.chunks = (int)((To + g.chunk - 1) / g.chunk);
  if ((long long)d->B * g.chunks > 0x7fffffffLL) return W2L_EUNSUPPORTED;
  g.items = d->B * g.chunks;
  // segments of the filter gradient: two workgroups per CU (512 / tiles), never more than kDwMaxSegments.  A workgroup stages,
  // waits and computes in turn, so the CU needs several to have loads in flight under the arithmetic; against that, a segment's
  // partials are as many bytes as half an item's operands, written once and read once (measured: DESIGN 3.30)
  g.S = std::min(g.items, std::max(1, std::min(kDwMaxSegments, 512 / g.tiles)));
  g.ldsBytes = (size_t)(g.chunk + d->kw - 1) * kDwThreads * sizeof(float);
  return W2L_OK;
}

static inline int dw_vec(const void* p, int F) { return (F % 4 == 0 && ((uintptr_t)p & 15) == 0) ? 1 : 0; }

template <int KWC>
static int dw_conv_launch(const float* in, const float* w, const float* bias, float* out, int B, int Tin, int Tout, const DwGeom& g, int C, int kw,
                          int padl, int reverse, hipStream_t s) {
  static bool attr[64] = {};
  if (KWC > 32 && first_on_device(attr))   // more than 64 KiB of LDS
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)dw_conv_k<KWC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)((dw_chunk(KWC) + KWC - 1) * kDwThreads * sizeof(float))));
  const dim3 grid((unsigned)g.tiles, (unsigned)((Tout + g.chunk - 1) / g.chunk), (unsigned)B);
  hipLaunchKernelGGL(dw_conv_k<KWC>, grid, dim3(kDwThreads), g.ldsBytes, s, in, w, bias, out, Tin, Tout, g.F, C, kw, padl, reverse, dw_vec(in, g.F),
                     g.chunk);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

static int dw_conv(const float* in, const float* w, const float* bias, float* out, int B, int Tin, int Tout, const DwGeom& g, int C, int kw, int padl,
                   int reverse, hipStream_t s) {
  if (kw <= 8) return dw_conv_launch<8>(in, w, bias, out, B, Tin, Tout, g, C, kw, padl, reverse, s);
  if (kw <= 16) return dw_conv_launch<16>(in, w, bias, out, B, Tin, Tout, g, C, kw, padl, reverse, s);
  if (kw <= 32) return dw_conv_launch<32>(in, w, bias, out, B, Tin, Tout, g, C, kw, padl, reverse, s);
  return dw_conv_launch<64>(in, w, bias, out, B, Tin, Tout, g, C, kw, padl, reverse, s);
}

template <int KWC>
static int dw_filter_launch(const w2l_conv_desc* d, const DwGeom& g, const float* x, const float* dy, float* part, hipStream_t s) {
  static bool attr[64] = {};
  if (KWC > 32 && first_on_device(attr))
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)dw_filter_k<KWC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)((dw_chunk(KWC) + KWC - 1) * kDwThreads * sizeof(float))));
  hipLaunchKernelGGL(dw_filter_k<KWC>, dim3((unsigned)g.tiles, (unsigned)g.S), dim3(kDwThreads), g.ldsBytes, s, x, dy, part, d->T, g.To, g.F, d->kw,
                     d->padl, g.chunks, g.items, g.S, dw_vec(x, g.F), g.chunk);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

}  // namespace w2l

using namespace w2l;

W2L_API int w2l_conv_depthwise_forward(const w2l_conv_desc* d, const float* x, const float* w, const float* bias, float* y, w2l_stream_t stream) {
  DwGeom g;
  const int st = dw_geom(d, g);
  if (st != W2L_OK) return st;
  if (!x || !w || !y) return W2L_EINVAL;
  return dw_conv(x, w, bias, y, d->B, d->T, g.To, g, d->Cin, d->kw, d->padl, 0, (hipStream_t)stream);
}

W2L_API int w2l_conv_depthwise_backward_data(const w2l_conv_desc* d, const float* dy, const float* w, float* dx, w2l_stream_t stream) {
  DwGeom g;
  const int st = dw_geom(d, g);
  if (st != W2L_OK) return st;
  if (!dy || !w || !dx || dx == dy) return W2L_EINVAL;
  return dw_conv(dy, w, nullptr, dx, d->B, g.To, d->T, g, d->Cin, d->kw, d->kw - 1 - d->padl, 1, (hipStream_t)stream);
}

W2L_API size_t w2l_conv_depthwise_workspace_floats(const w2l_conv_desc* d) {
  DwGeom g;
  if (dw_geom(d, g) != W2L_OK) return 0;
  return (size_t)g.S * (d->kw + 1) * g.F;
}

W2L_API int w2l_conv_depthwise_backward_filter(const w2l_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias, float* workspace,
                                               w2l_stream_t stream) {
  DwGeom g;
  int st = dw_geom(d, g);
  if (st != W2L_OK) return st;
  if (!x || !dy || !dw || !workspace) return W2L_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (d->kw <= 8) st = dw_filter_launch<8>(d, g, x, dy, workspace, s);
  else if (d->kw <= 16) st = dw_filter_launch<16>(d, g, x, dy, workspace, s);
  else if (d->kw <= 32) st = dw_filter_launch<32>(d, g, x, dy, workspace, s);
  else st = dw_filter_launch<64>(d, g, x, dy, workspace, s);
  if (st != W2L_OK) return st;
  const int n = (d->kw + 1) * d->Cin;
  hipLaunchKernelGGL(dw_filter_reduce_k, dim3((unsigned)((n + kDwReduceCols - 1) / kDwReduceCols)), dim3(kDwThreads), 0, s, workspace, dw, dbias, g.S, d->H,
                     d->Cin, d->kw);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
