// stream.hip -- the hand-over kernel of the chunked streaming forward (host/stream.cpp).
//
// A layer with a time extent (Conv2D, TDS block) runs as a VALID convolution over a rectangular window [S][W][F] per step; the
// slots are ragged (each sits at its own phase of its own utterance), so a per-slot count entry says what the row holds:
//   window[s] = carry[s][0 .. nCarry)  ++  new[s][0 .. nNew)  ++  zeros up to W
// (zeros: the right padding of an utterance that finishes in this step, then the fill -- nothing a product reads is ever
// uninitialised).  The SAME launch stores what the layer will not have consumed after this step, window[s][consumed .. nIn), as
// the next step's carry -- the counts are host arithmetic, known before the layer runs -- and, for a TDS block, the window frames
// that line up with the convolution's outputs (its residual operand, [S][To][F]).  The carry is double-buffered: a thread reads
// the old one and writes the new one, no thread reads what another wrote, and a slot that is idle in this step has its carry
// copied across.
//
// One thread moves one 16-byte vector (frame sizes that are a multiple of 4 floats: every layout of the recipes) or one float.
// Each thread issues its one load first and then up to three independent stores of the loaded value: there is no store -> load
// chain inside the kernel.
#include "common.hpp"

namespace w2l {

template <typename V>
__global__ __launch_bounds__(256) void stream_window_k(const V* __restrict__ src, int srcRows, const V* __restrict__ carryIn,
                                                       V* __restrict__ carryOut, int carryCap, V* __restrict__ win, int W,
                                                       V* __restrict__ res, int resShift, int To, const int4* __restrict__ tab, int FV) {
  const int s = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= W * FV) return;
  const int j = idx / FV, f = idx - j * FV;
  const int4 t = tab[s];   // x: carry frames (bit 30: they are the zero frames ahead of an utterance), y: new, z: nIn, w: consumed
  const int nc = t.x & 0x3fffffff;
  const bool zeroCarry = (t.x >> 30) & 1;
  V v{};
  if (j < nc) {
    if (!zeroCarry && j < carryCap) v = carryIn[((size_t)s * carryCap + j) * FV + f];
  } else if (j < nc + t.y && j - nc < srcRows) {
    v = src[((size_t)s * srcRows + (j - nc)) * FV + f];
  }
  win[((size_t)s * W + j) * FV + f] = v;
  if (res && j >= resShift && j - resShift < To) res[((size_t)s * To + (j - resShift)) * FV + f] = v;
  if (j >= t.w && j < t.z && j - t.w < carryCap) carryOut[((size_t)s * carryCap + (j - t.w)) * FV + f] = v;
}

}  // namespace w2l

using namespace w2l;

// src [S][srcRows][F]: the producer's frames of this step (row s: nNew[s] of them); carryIn / carryOut [S][carryCap][F] (carryCap
// may be 0: both may be null then); win [S][W][F]; res [S][To][F] or null; tab: S device entries (see the kernel).  The caller
// guarantees per slot nCarry <= carryCap, nNew <= srcRows, nIn <= W and nIn - consumed <= carryCap (host/stream.cpp checks).
W2L_API int w2l_stream_window(const float* src, int srcRows, const float* carryIn, float* carryOut, int carryCap, float* win, int W,
                              float* res, int resShift, int To, const int* tab, int S, int F, w2l_stream_t stream) {
  if (!src || !win || !tab || S <= 0 || F <= 0 || W <= 0 || srcRows <= 0 || carryCap < 0) return W2L_EINVAL;
  if (carryCap > 0 && (!carryIn || !carryOut || carryIn == carryOut)) return W2L_EINVAL;
  if (res && (resShift < 0 || To <= 0 || resShift + To > W)) return W2L_EINVAL;
  if ((size_t)W * F > (size_t)1 << 30 || S > 65535) return W2L_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  auto aligned = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (F % 4 == 0 && aligned(src) && aligned(carryIn) && aligned(carryOut) && aligned(win) && aligned(res)) {
    const int FV = F / 4;
    dim3 grid((unsigned)((W * FV + 255) / 256), (unsigned)S);
    hipLaunchKernelGGL(stream_window_k<float4>, grid, dim3(256), 0, s, (const float4*)src, srcRows, (const float4*)carryIn,
                       (float4*)carryOut, carryCap, (float4*)win, W, (float4*)res, resShift, To, (const int4*)tab, FV);
  } else {
    dim3 grid((unsigned)((W * F + 255) / 256), (unsigned)S);
    hipLaunchKernelGGL(stream_window_k<float>, grid, dim3(256), 0, s, src, srcRows, carryIn, carryOut, carryCap, win, W, res, resShift,
                       To, (const int4*)tab, F);
  }
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
