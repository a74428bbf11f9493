// conv_bf16.hip -- the WIDE-channel time convolution (fl::Conv2D kw x 1 at H == 1: the `C cin cout kw s pad` lines of the conv_glu
// recipes, recipes/conv_glu/librispeech/network.arch -- 200 .. 908 input channels, kw 13 .. 29 --, of the lexicon-free recipe and
// of the Transformer recipes' three-layer front end) with bf16 operands: the second level of the mixed-precision mode
// (w2l_trainer_set_mixed_precision_convs).  x / dy and the weights are rounded to bf16 (nearest even), the products run on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation, bias / ReLU / addend and every result are fp32.
//
// conv.hip phrases this convolution as a GEMM on OVERLAPPING rows -- in the frame-major layout the unfolded row of output frame
// (b, to) is kw * C contiguous elements of x -- and runs it on the fp32 LDS-DMA engine.  Here the same three products run on the
// bf16 LDS-DMA engine of gemm_bf16g.hpp (launch128h: 128 x 128 / 256 x 256 tiles, k-major operands in place, aligned K split
// with an in-order slab reduction), on two IMAGES the passes write first:
//
//   x image   [B][Tp][CPi] bf16: the activation with padl zero frames in front of and padr (+ stride - 1 at most) behind every
//             utterance -- the time padding is data, no index arithmetic -- and the channels padded with zeros to CPi = a
//             multiple of 8, so that every frame starts on a 16-byte boundary (the 16-byte LDS-DMA pieces and the k-major
//             fragment reads need that; the recipe's 242 / 321 / 353 / 565 / 621 / 683 / 751 channels do not give it);
//   dy image  [kw - 1 zero frames][B][Tp][CPo] bf16: dy[b][to] at frame stride * to of utterance b, zeros everywhere else.
//
//   forward   y[(b, to)][co] = X[row (b Tp / s + to), ld = s CPi][k = tap CPi + ci] . Wf[co][k]        K = kw CPi
//   bwd-data  dx[(b, t')][ci] = D[row b Tp + t', ld = CPo][k = j CPo + co] . Wb[ci][k], Wb tap j = w[kw - 1 - j]^T   K = kw CPo
//             (t' = ti + padl; with stride 2 the zero frames between the dy frames make it the stride-1 product: half of its
//             multiplies meet zeros -- the price of one code path; the recipes have a handful of kw 3 / 7 lines at stride 2)
//   bwd-filt  dw[(tap, ci)][co] = sum_r X[r][tap CPi + ci] . D[r][co]: ONE product over K = B Tp - (kw - 1) frames with BOTH
//             operands k-major and read in place -- the A operand on overlapping rows again, the kw CPi elements that start at
//             frame r (a tap is a shift by whole 16-byte aligned frames; a shift inside a transposed image would not be).  The
//             zero frames of the dy image kill the terms that straddle two utterances.
//   dbias     column sums of the dy image (the ROUNDED dy, as in the TDS family), fixed order.
// The epilogue's row remap (GemmOut::rowPin) drops the GEMM rows that are no output frame.  The K tail of a row (K rounded up to
// 64) reads the following frames against zero weights; past the image the buffer range returns zeros.
// Deterministic: no atomics on results, the K split of the filter products adds its slabs in chunk order.
//
// What the images cost: x is read (4 bytes) and written (2 bytes) once per pass that needs it -- forward and filter gradient --,
// dy likewise for backward-data and the filter gradient: 6 bytes per element and pass against 2 kw Cout flops per element of x.
#include "gemm.hpp"

namespace w2l {

typedef __bf16 cb_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float cb_f32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t cb_pack2(float a, float b) {   // round to nearest even (v_cvt_pk_bf16_f32)
  const cb_f32x2_t p = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(p, cb_bf16x2_t));
}

constexpr int kCbMaxChan = 8192;
constexpr int kCbColsumParts = 256;

struct CbGeom {
  int s, To, Tp, CPi, CPo;
  int Kf, Kfp, Kb, Kbp;        // reduction lengths of forward / backward-data, and rounded up to the 64-k tile
  size_t xElems, dyElems;      // image sizes in bf16 elements (the dy image with its kw - 1 front frames)
  size_t wElems;               // one weight image buffer
  size_t csFloats;             // column-sum partials
};

static inline size_t cb_up8(size_t v) { return (v + 7) & ~(size_t)7; }

// 0: bad descriptor (W2L_EINVAL), 1: no kernel for this geometry (W2L_EUNSUPPORTED), 2: accepted
static int cb_geometry(const w2l_conv_desc* d, CbGeom& g) {
  if (!d || d->B <= 0 || d->T <= 0 || d->H <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->kw <= 0 || d->stride <= 0 || d->padl < 0 ||
      d->padr < 0)
    return 0;
  const long long n = (long long)d->T + d->padl + d->padr - d->kw;
  if (n < 0) return 0;
  if (d->H != 1 || (d->stride != 1 && d->stride != 2) || d->Cin < 32 || d->Cin > kCbMaxChan || d->Cout > kCbMaxChan ||
      d->kw > 64)
    return 1;
  const long long tp0 = (long long)d->T + d->padl + d->padr;
  const long long tp = (tp0 + d->stride - 1) / d->stride * d->stride;
  g.s = d->stride;
  g.To = (int)(n / d->stride) + 1;
  g.CPi = (d->Cin + 7) & ~7;
  g.CPo = (d->Cout + 7) & ~7;
  g.Kf = d->kw * g.CPi; g.Kfp = (g.Kf + 63) / 64 * 64;
  g.Kb = d->kw * g.CPo; g.Kbp = (g.Kb + 63) / 64 * 64;
  const long long rows = (long long)d->B * tp;
  const long long xB = rows * g.CPi * 2, dyB = (rows + d->kw - 1) * g.CPo * 2;
  const long long wf = (long long)d->Cout * g.Kfp, wb = (long long)d->Cin * g.Kbp;
  // every operand is addressed through a 32-bit buffer range
  if (rows >= (1ll << 30) || xB >= 0x7fffffffll || dyB >= 0x7fffffffll || wf * 2 >= 0x7fffffffll || wb * 2 >= 0x7fffffffll) return 1;
  g.Tp = (int)tp;
  g.xElems = (size_t)rows * g.CPi;
  g.dyElems = (size_t)(rows + d->kw - 1) * g.CPo;
  g.wElems = cb_up8((size_t)(wf > wb ? wf : wb));
  g.csFloats = (size_t)kCbColsumParts * g.CPo;
  return 2;
}

// ---- images ---------------------------------------------------------------------------------------------------------
// dst [B][Tdst][CP] bf16 <- src [B][Tsrc][C] fp32: frame t' of an utterance holds source frame (t' - off) / step where that is a
// whole number in [0, Tsrc), zeros otherwise; channels C .. CP are zeros.  A thread writes one 16-byte chunk (8 channels).
template <bool VEC4>
__global__ __launch_bounds__(256) void cb_image_k(const float* __restrict__ src, uint16_t* __restrict__ dst, int Tsrc, int Tdst, int C, int CP,
                                                  int off, int step, size_t chunks) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= chunks) return;
  const int nC = CP >> 3;
  const size_t f = e / (size_t)nC;
  const int c0 = (int)(e - f * nC) * 8;
  const size_t b = f / (size_t)Tdst;
  const int t = (int)(f - b * Tdst) - off;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
  if (t >= 0 && t % step == 0 && t / step < Tsrc) {
    const float* p = src + ((size_t)b * Tsrc + (size_t)(t / step)) * C + c0;
    if (VEC4) {   // C % 4 == 0 and a 16-byte aligned tensor
      if (c0 < C) { const float4 a = *(const float4*)p; v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
      if (c0 + 4 < C) { const float4 a = *(const float4*)(p + 4); v[4] = a.x; v[5] = a.y; v[6] = a.z; v[7] = a.w; }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (c0 + i < C) v[i] = p[i];
    }
  }
  *(uint4*)(dst + e * 8) = make_uint4(cb_pack2(v[0], v[1]), cb_pack2(v[2], v[3]), cb_pack2(v[4], v[5]), cb_pack2(v[6], v[7]));
}

static int cb_image(const float* src, uint16_t* dst, int B, int Tsrc, int Tdst, int C, int CP, int off, int step, hipStream_t s) {
  const size_t chunks = (size_t)B * Tdst * (CP / 8);
  const unsigned grid = (unsigned)((chunks + 255) / 256);
  if (C % 4 == 0 && (((uintptr_t)src) & 15) == 0) hipLaunchKernelGGL(cb_image_k<true>, dim3(grid), dim3(256), 0, s, src, dst, Tsrc, Tdst, C, CP, off, step, chunks);
  else hipLaunchKernelGGL(cb_image_k<false>, dim3(grid), dim3(256), 0, s, src, dst, Tsrc, Tdst, C, CP, off, step, chunks);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

// forward weight image  img[co][j CP + ci] = w[j][ci][co] (zeros at ci >= Cin and k >= kw CP): a transposition, 32 x 32 tiles
// through LDS -- reads run along co, writes along k
__global__ __launch_bounds__(256) void cb_wprep_fwd_k(const float* __restrict__ w, int kw, int Cin, int Cout, int CP, int Kp,
                                                      uint16_t* __restrict__ img) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int k0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = k0 + ty + 8 * r, n = n0 + tx;
    const int j = k / CP, c = k - j * CP;
    float v = 0.f;
    if (j < kw && c < Cin && n < Cout) v = w[((size_t)j * Cin + c) * Cout + n];
    tile[ty + 8 * r][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + ty + 8 * r, k = k0 + tx;
    if (n < Cout && k < Kp) img[(size_t)n * Kp + k] = (uint16_t)(cb_pack2(tile[tx][ty + 8 * r], 0.f) & 0xffffu);
  }
}

// backward-data weight image  img[ci][j CP + co] = w[kw - 1 - j][ci][co]: co is contiguous on both sides
__global__ __launch_bounds__(256) void cb_wprep_bwd_k(const float* __restrict__ w, int kw, int Cin, int Cout, int CP, int Kp,
                                                      uint16_t* __restrict__ img) {
  const int k = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (k >= Kp) return;
  const int j = k / CP, c = k - j * CP;
  float v = 0.f;
  if (j < kw && c < Cout) v = w[((size_t)(kw - 1 - j) * Cin + n) * Cout + c];
  img[(size_t)n * Kp + k] = (uint16_t)(cb_pack2(v, 0.f) & 0xffffu);
}

// column sums of a bf16 image [rows][CP]: part p = blockIdx.x adds its rows, blockIdx.y picks 256 of a row's 16-byte chunks (thread =
// one chunk of every RPP-th row, then the RPP row lanes in lane order); cb_colsum_finish_k adds the parts in part order
__global__ __launch_bounds__(256) void cb_colsum_part_k(const uint16_t* __restrict__ img, float* __restrict__ partial, size_t rows, int CP,
                                                        size_t rowsPerPart) {
  __shared__ float sm[256][9];
  const int c0 = blockIdx.y * 256, nAll = CP >> 3;
  const int nC = nAll - c0 < 256 ? nAll - c0 : 256, RPP = 256 / nC;
  const int tid = threadIdx.x, ch = c0 + tid % nC, rl = tid / nC;
  size_t r0 = (size_t)blockIdx.x * rowsPerPart, r1 = r0 + rowsPerPart;
  if (r1 > rows) r1 = rows;
  float a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = 0.f;
  if (rl < RPP)
    for (size_t r = r0 + rl; r < r1; r += RPP) {
      const uint4 q = *(const uint4*)(img + r * CP + 8 * ch);
      const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[2 * i] += __builtin_bit_cast(float, u[i] << 16);
        a[2 * i + 1] += __builtin_bit_cast(float, u[i] & 0xffff0000u);
      }
    }
#pragma unroll
  for (int i = 0; i < 8; ++i) sm[tid][i] = a[i];
  __syncthreads();
  if (tid < nC) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float t = 0.f;
      for (int q = 0; q < RPP; ++q) t += sm[q * nC + tid][i];
      partial[(size_t)blockIdx.x * CP + 8 * (c0 + tid) + i] = t;
    }
  }
}

__global__ __launch_bounds__(256) void cb_colsum_finish_k(const float* __restrict__ partial, int parts, int CP, int N, float* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float t = 0.f;
  for (int p = 0; p < parts; ++p) t += partial[(size_t)p * CP + n];
  out[n] = t;
}

struct CbScratch {
  uint16_t* x;     // x image
  uint16_t* dy;    // dy image (front frames included)
  float* cs;       // column-sum partials
};
static inline CbScratch cb_scratch(const CbGeom& g, uint16_t* scratch) {
  CbScratch r;
  r.x = scratch;
  r.dy = scratch + cb_up8(g.xElems);
  r.cs = (float*)(r.dy + cb_up8(g.dyElems));
  return r;
}

static int cb_dy_image(const w2l_conv_desc* d, const CbGeom& g, const float* dy, uint16_t* img, hipStream_t s) {
  const size_t front = (size_t)(d->kw - 1) * g.CPo;
  if (front) W2L_HIP_CHECK(hipMemsetAsync(img, 0, front * sizeof(uint16_t), s));
  return cb_image(dy, img + front, d->B, g.To, g.Tp, d->Cout, g.CPo, 0, g.s, s);
}

}  // namespace w2l

using namespace w2l;

// bf16 elements of ONE weight image buffer (the forward image [Cout][kw CPi] or the backward-data image [Cin][kw CPo], rows
// rounded up to 64 k, whichever is larger); 0: the geometry has no kernel here -- stay on w2l_conv_*.  Host arithmetic.
W2L_API size_t w2l_conv_bf16_image_elems(const w2l_conv_desc* d) {
  CbGeom g;
  return cb_geometry(d, g) == 2 ? g.wElems : 0;
}

// bf16 elements of the caller-owned scratch the three passes write their activation / gradient images to (16-byte aligned; its
// contents mean nothing between calls).  Host arithmetic.
W2L_API size_t w2l_conv_bf16_scratch_elems(const w2l_conv_desc* d) {
  CbGeom g;
  if (cb_geometry(d, g) != 2) return 0;
  return cb_up8(g.xElems) + cb_up8(g.dyElems) + 2 * g.csFloats;
}

#define CB_GEOMETRY(d, g)                                  \
  CbGeom g;                                                \
  {                                                        \
    const int _k = cb_geometry(d, g);                      \
    if (_k != 2) return _k ? W2L_EUNSUPPORTED : W2L_EINVAL; \
  }

// once per step: the two weight images of w [kw][Cin][Cout] (fp32 master weights, or the result of w2l_weightnorm_forward)
W2L_API int w2l_conv_bf16_prepare(const w2l_conv_desc* d, const float* w, uint16_t* imgForward, uint16_t* imgBackward, w2l_stream_t stream) {
  if (!d || !w || (!imgForward && !imgBackward)) return W2L_EINVAL;
  CB_GEOMETRY(d, g)
  if ((((uintptr_t)imgForward) | ((uintptr_t)imgBackward)) & 15) return W2L_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (imgForward)
    hipLaunchKernelGGL(cb_wprep_fwd_k, dim3((unsigned)(g.Kfp / 32), (unsigned)((d->Cout + 31) / 32)), dim3(256), 0, s, w, d->kw, d->Cin, d->Cout,
                       g.CPi, g.Kfp, imgForward);
  if (imgBackward)
    hipLaunchKernelGGL(cb_wprep_bwd_k, dim3((unsigned)((g.Kbp + 255) / 256), (unsigned)d->Cin), dim3(256), 0, s, w, d->kw, d->Cin, d->Cout, g.CPo,
                       g.Kbp, imgBackward);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

// y [B][To][1][Cout] = (relu)(conv(bf16(x), imgForward) + bias)
W2L_API int w2l_conv_bf16_forward(const w2l_conv_desc* d, const float* x, const uint16_t* imgForward, const float* bias, float* y, int relu,
                                  uint16_t* scratch, w2l_stream_t stream) {
  if (!d || !x || !imgForward || !y || !scratch) return W2L_EINVAL;
  CB_GEOMETRY(d, g)
  if ((((uintptr_t)imgForward) | ((uintptr_t)scratch)) & 15) return W2L_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const CbScratch sc = cb_scratch(g, scratch);
  int st = cb_image(x, sc.x, d->B, d->T, g.Tp, d->Cin, g.CPi, d->padl, 1, s);
  if (st) return st;
  const int Tps = g.Tp / g.s;
  GemmOut o{y, bias, d->B * Tps, d->Cout, g.Kf, d->Cout, 0};
  gemm_set_row_remap(o, Tps, g.To, 0);
  const int epi = (bias ? EPI_BIAS : 0) | (relu ? EPI_RELU : 0);
  return gemm_bf16_images(sc.x, g.s * g.CPi, 2ull * g.xElems, imgForward, g.Kfp, 0, o, epi, s);
}

// dx [B][T][1][Cin] = (add +) conv^T(bf16(dy), imgBackward)
W2L_API int w2l_conv_bf16_backward_data(const w2l_conv_desc* d, const float* dy, const uint16_t* imgBackward, const float* add, float* dx,
                                        uint16_t* scratch, w2l_stream_t stream) {
  if (!d || !dy || !imgBackward || !dx || !scratch) return W2L_EINVAL;
  CB_GEOMETRY(d, g)
  if ((((uintptr_t)imgBackward) | ((uintptr_t)scratch)) & 15) return W2L_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const CbScratch sc = cb_scratch(g, scratch);
  int st = cb_dy_image(d, g, dy, sc.dy, s);
  if (st) return st;
  GemmOut o{dx, nullptr, d->B * g.Tp, d->Cin, g.Kb, d->Cin, 0};
  gemm_set_row_remap(o, g.Tp, d->T, d->padl);
  int epi = 0;
  if (add) { o.addend = add; epi |= EPI_ACCUM; }
  return gemm_bf16_images(sc.dy, g.CPo, 2ull * g.dyElems, imgBackward, g.Kbp, 0, o, epi, s);
}

// dw [kw][Cin][Cout] = x (*) dy on the rounded operands; dbias [Cout] (may be null): the column sums of the ROUNDED dy
W2L_API int w2l_conv_bf16_backward_filter_bias(const w2l_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                               uint16_t* scratch, w2l_stream_t stream) {
  if (!d || !x || !dy || !dw || !scratch) return W2L_EINVAL;
  CB_GEOMETRY(d, g)
  if (((uintptr_t)scratch) & 15) return W2L_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const CbScratch sc = cb_scratch(g, scratch);
  int st = cb_image(x, sc.x, d->B, d->T, g.Tp, d->Cin, g.CPi, d->padl, 1, s);
  if (st) return st;
  st = cb_dy_image(d, g, dy, sc.dy, s);
  if (st) return st;
  const uint16_t* D = sc.dy + (size_t)(d->kw - 1) * g.CPo;   // the image proper, behind the front frames of backward-data
  const size_t rows = (size_t)d->B * g.Tp;
  // ONE product for all taps: rows of the result = (tap, padded ci) = the kw CPi consecutive elements that start at frame r of the
  // x image -- a k-major A operand on overlapping rows.  The last kw - 1 frames r hold no dy (zeros): K stops before them, so every
  // read stays inside the image.  The row remap drops the padded channels: row (tap, ci) -> dw row tap Cin + ci.
  GemmOut o{dw, nullptr, d->kw * g.CPi, d->Cout, (int)(rows - (size_t)(d->kw - 1)), d->Cout, 0};
  if (g.CPi != d->Cin) gemm_set_row_remap(o, g.CPi, d->Cin, 0);
  st = gemm_bf16_images(sc.x, g.CPi, 2ull * g.xElems, D, g.CPo, 0, o, 0, s, true, true);
  if (st) return st;
  if (dbias) {
    size_t rpp = (rows + kCbColsumParts - 1) / kCbColsumParts;
    if (rpp < 16) rpp = 16;
    const int parts = (int)((rows + rpp - 1) / rpp);
    hipLaunchKernelGGL(cb_colsum_part_k, dim3((unsigned)parts, (unsigned)((g.CPo / 8 + 255) / 256)), dim3(256), 0, s, D, sc.cs, rows, g.CPo, rpp);
    hipLaunchKernelGGL(cb_colsum_finish_k, dim3((unsigned)((d->Cout + 255) / 256)), dim3(256), 0, s, sc.cs, parts, g.CPo, d->Cout, dbias);
    W2L_LAUNCH_CHECK();
  }
  return W2L_OK;
}
