// feat_stream.hip -- the streaming log-mel front end in ONE launch per step: PCM chunks of S slots -> MFSC frames.
//
// Reference: recipes/streaming_convnets/inference/inference/module/feature/LogMelFeature.cpp buffers samples, produces
// numFrames(buffered) frames, consumes numFrames x stride samples and keeps the rest.  The arithmetic is features.hip's and
// features.py's: the frame's linear part (pre-emphasis, Hamming window, DFT) is the table G [N][2 nbins], the filterbank the
// table H [ldSpec][F]; here both products, the magnitude between them and the log behind them run in one workgroup per tile of
// kFeatRows frames, with everything between the samples and the log in LDS and registers.
//
//   grid (frame tiles, slots), 512 threads = 8 waves.  tab[s] = {carry samples, new samples, frames, flags}: host arithmetic.
//   1. window   = carry[s] ++ pcm[s][0..n) restricted to the tile's samples [t0 St, t0 St + R St + N - St), zero beyond the slot's
//                 count, int16 scaled by 1/32768 on the way.  LDS, one pad float every 32 (frame stride 160 = 5 x 32 would put the
//                 16 rows of an A fragment into one bank).
//   2. spectrum = [R x N] . [N x 2 nbins] on v_mfma_f32_16x16x4_f32: A = overlapping rows of the window (leading dimension St), G
//                 from global memory (L2 resident).  A wave owns column tiles w, w + 8, w + 16 and for each the real AND the
//                 imaginary tile, so one A fragment feeds up to six independent accumulators and re / im meet in registers.
//                 Operands are loaded a block of 4 k-steps ahead of the products that use them (feat_spectrum).
//   3. |.|        sqrtf(re^2 + im^2) (usePower: the square) -> LDS spectrum tile [R][ldS], zero at and beyond nbins.
//   4. mel      = [R x nbins] . [nbins x F] the same way, H from global memory, one column tile of 16 filters per wave.
//   5. logf(fmaxf(., floor)) -> out[s][f][t0 + r]: a lane holds 4 consecutive frames of one filter, a filter's 16 frames are one
//                 64-byte run.  Columns at or beyond the slot's frame count are not written.
//   The workgroup of tile 0 also writes the slot's next carry into the OTHER carry buffer (the slot's other tiles still read the
//   old one); which of the two is current is a bit of the slot's table entry, flipped by the host when the slot had work.
//
// A frame's result depends on its own N samples only: every output element is one accumulator whose k runs upward in steps of 4,
// no K split, no reduction across lanes or waves, and the row of the tile a frame lands in only selects lanes.  That is what makes
// the features independent of how the audio was chunked, bit for bit.
#include "common.hpp"

namespace w2l {

constexpr int kFeatRows = 16;      // frames per tile (the M of the 16x16x4 MFMA)
constexpr int kFeatThreads = 512;  // 8 waves
constexpr int kFeatWaves = kFeatThreads / 64;
constexpr int kFeatColTiles = 3;   // spectrum column tiles per wave: 8 x 3 x 16 = 384 >= 257 bins
constexpr int kFeatBlock = 4;      // k-steps of the spectrum product whose operands are loaded together, one block ahead
constexpr int kFeatMelBlock = 8;   // the same for the mel product, not ahead (one column tile per wave: a block is 16 loads)

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int feat_pad(int j) { return j + (j >> 5); }

template <typename T>
__device__ __forceinline__ float feat_sample(const T* p);
template <>
__device__ __forceinline__ float feat_sample<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float feat_sample<int16_t>(const int16_t* p) { return (float)*p * (1.0f / 32768.0f); }

// sample g of the slot's buffer carry ++ new; 0 at and beyond `have`
template <typename T>
__device__ __forceinline__ float feat_buffered(const float* carry, const T* pcm, int nc, int have, int g) {
  if (g >= have) return 0.f;
  return g < nc ? carry[g] : feat_sample<T>(pcm + (g - nc));
}

// The spectrum product of one wave: NT column tiles (real and imaginary), k upward in steps of 4.  The loads of a block of
// kFeatBlock k-steps (one window value and 2 NT values of G each) are issued before the previous block's products run, so the
// latency of G is paid once per block and hidden behind a block of MFMAs, not once per k-step; the order of the products per
// accumulator is the plain loop's.
template <int NT>
struct FeatFrag {
  float a[kFeatBlock], br[kFeatBlock][NT], bi[kFeatBlock][NT];
};

// GUARD: the block may reach beyond the frame (k >= N reads a valid address and counts as zero) and beyond the last k-step
template <int NT, bool GUARD>
__device__ __forceinline__ void feat_load(FeatFrag<NT>& f, const float* __restrict__ win, int a0, const float* __restrict__ G, int q,
                                          int N, int nb, const int (&col)[NT], int blk) {
#pragma unroll
  for (int u = 0; u < kFeatBlock; ++u) {
    const int k = 4 * (blk * kFeatBlock + u) + q;
    const bool in = !GUARD || k < N;
    const int kc = in ? k : N - 1;
    const float a = win[feat_pad(a0 + kc)];
    f.a[u] = in ? a : 0.f;
    const float* g = G + (size_t)kc * 2 * nb;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      const float br = g[col[c]], bi = g[nb + col[c]];
      f.br[u][c] = in ? br : 0.f;
      f.bi[u][c] = in ? bi : 0.f;
    }
  }
}

template <int NT>
__device__ __forceinline__ void feat_mma(const FeatFrag<NT>& f, f32x4 (&re)[kFeatColTiles], f32x4 (&im)[kFeatColTiles], int steps) {
#pragma unroll
  for (int u = 0; u < kFeatBlock; ++u)
    if (u < steps) {   // uniform
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        re[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[u], f.br[u][c], re[c], 0, 0, 0);
        im[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[u], f.bi[u][c], im[c], 0, 0, 0);
      }
    }
}

template <int NT>
__device__ __forceinline__ void feat_spectrum(const float* __restrict__ win, const float* __restrict__ G, int N, int St, int nb, int wave,
                                              int r16, int q, f32x4 (&re)[kFeatColTiles], f32x4 (&im)[kFeatColTiles]) {
  int col[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) col[c] = min((wave + kFeatWaves * c) * 16 + r16, nb - 1);   // columns beyond nbins repeat the last one and are dropped
  const int a0 = r16 * St;
  const int K4 = (N + 3) / 4;
  const int nblk = N / 4 / kFeatBlock;   // blocks of k-steps that lie inside the frame with all four k
  const int tail = K4 - nblk * kFeatBlock;   // k-steps of the last, guarded block (0 .. kFeatBlock)
  FeatFrag<NT> f0, f1;
  if (nblk > 0) feat_load<NT, false>(f0, win, a0, G, q, N, nb, col, 0);
  for (int blk = 0; blk < nblk; blk += 2) {
    if (blk + 1 < nblk) feat_load<NT, false>(f1, win, a0, G, q, N, nb, col, blk + 1);
    else if (tail) feat_load<NT, true>(f1, win, a0, G, q, N, nb, col, nblk);
    feat_mma<NT>(f0, re, im, kFeatBlock);
    if (blk + 1 < nblk) {
      if (blk + 2 < nblk) feat_load<NT, false>(f0, win, a0, G, q, N, nb, col, blk + 2);
      else if (tail) feat_load<NT, true>(f0, win, a0, G, q, N, nb, col, nblk);
      feat_mma<NT>(f1, re, im, kFeatBlock);
    }
  }
  // the guarded block was loaded into f1 after an odd number of whole blocks, into f0 after an even number (or none)
  if (tail) {
    if (nblk == 0) feat_load<NT, true>(f0, win, a0, G, q, N, nb, col, 0);
    if (nblk & 1) feat_mma<NT>(f1, re, im, tail);
    else feat_mma<NT>(f0, re, im, tail);
  }
}

template <typename T>
__global__ __launch_bounds__(kFeatThreads) void feat_stream_k(const T* __restrict__ pcm, int maxSamples, const int* __restrict__ tab,
                                                              float* __restrict__ carry0, float* __restrict__ carry1, int carryLd,
                                                              const float* __restrict__ G, const float* __restrict__ H,
                                                              float* __restrict__ out, int maxOut, int N, int St, int nb,
                                                              int F, int usePower, float floorv, int ldS) {
  extern __shared__ float lds[];
  const int s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int nc = tab[4 * s], n = tab[4 * s + 1], nOut = tab[4 * s + 2], flags = tab[4 * s + 3];
  const int t0 = tile * kFeatRows;
  if (!(flags & 2) || (t0 >= nOut && tile > 0)) return;   // the slot had no work / the tile lies beyond its frames
  const int have = nc + n;
  const float* cin = ((flags & 1) ? carry1 : carry0) + (size_t)s * carryLd;
  const T* x = pcm + (size_t)s * maxSamples;
  if (tile == 0) {   // the next carry: what the step's frames do not consume (always fewer than N samples)
    float* cout = ((flags & 1) ? carry0 : carry1) + (size_t)s * carryLd;
    const int consumed = nOut * St;
    for (int i = tid; i < have - consumed; i += kFeatThreads) cout[i] = feat_buffered<T>(cin, x, nc, have, consumed + i);
    if (nOut == 0) return;
  }
  const int W = kFeatRows * St + N - St;
  float* win = lds;
  float* spec = lds + feat_pad(W) + 1;
  for (int j = tid; j < W; j += kFeatThreads) win[feat_pad(j)] = feat_buffered<T>(cin, x, nc, have, t0 * St + j);
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int nbT = (nb + 15) / 16;
  // ---- spectrum: re and im accumulators of up to kFeatColTiles column tiles per wave
  if (wave < nbT) {
    f32x4 re[kFeatColTiles], im[kFeatColTiles];
#pragma unroll
    for (int c = 0; c < kFeatColTiles; ++c) {
      re[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      im[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // wave-uniform: how many column tiles this wave owns
    if (wave + 2 * kFeatWaves < nbT) feat_spectrum<3>(win, G, N, St, nb, wave, r16, q, re, im);
    else if (wave + kFeatWaves < nbT) feat_spectrum<2>(win, G, N, St, nb, wave, r16, q, re, im);
    else feat_spectrum<1>(win, G, N, St, nb, wave, r16, q, re, im);
    // accumulator element i of a lane: row 4 q + i, column r16 of the tile
#pragma unroll
    for (int c = 0; c < kFeatColTiles; ++c) {
      const int ct = wave + kFeatWaves * c;
      if (ct < nbT) {
        const int cc = ct * 16 + r16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float pw = re[c][i] * re[c][i] + im[c][i] * im[c][i];
          spec[(4 * q + i) * ldS + cc] = cc < nb ? (usePower ? pw : sqrtf(pw)) : 0.f;
        }
      }
    }
  }
  __syncthreads();

  // ---- mel: one column tile of 16 filters per wave, then the log and the store
  if (wave * 16 < F) {
    const int f = wave * 16 + r16, fc = min(f, F - 1);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    // blocks of kFeatMelBlock k-steps with every load issued before the first product; k at or beyond nbins reads the tile's zero
    // columns (4 K4 <= 16 nbT) against a zero instead of H
    const int K4 = (nb + 3) / 4;
    for (int k0 = 0; k0 < K4; k0 += kFeatMelBlock) {
      float a[kFeatMelBlock], b[kFeatMelBlock];
#pragma unroll
      for (int u = 0; u < kFeatMelBlock; ++u) {
        const int k = 4 * (k0 + u) + q;
        a[u] = spec[r16 * ldS + min(k, ldS - 1)];
        b[u] = k < nb ? H[(size_t)k * F + fc] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kFeatMelBlock; ++u)
        if (k0 + u < K4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc, 0, 0, 0);
    }
    if (f < F) {
      float* o = out + ((size_t)s * F + f) * maxOut + t0 + 4 * q;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (t0 + 4 * q + i < nOut) o[i] = logf(fmaxf(acc[i], floorv));
    }
  }
}

}  // namespace w2l

using namespace w2l;

W2L_API int w2l_feat_stream_tile_rows(void) { return kFeatRows; }

W2L_API int w2l_feat_stream_frames(const w2l_feat_desc* d, const float* G, const float* H, const void* pcm, int pcmType, int maxSamples,
                                   const int* tab, float* carry0, float* carry1, int carryLd, float* out, int maxOut, int slots,
                                   w2l_stream_t stream) {
  if (!d || !G || !H || !pcm || !tab || !carry0 || !carry1 || !out) return W2L_EINVAL;
  const int N = d->frameSize, St = d->frameStride, nb = d->nbins, F = d->numFilters;
  if (St < 1 || N < St || nb < 1 || d->ldSpec < nb || F < 1 || !(d->melFloor > 0.f)) return W2L_EINVAL;
  if (slots < 1 || slots > 65535 || maxSamples < 1 || maxOut < 1 || carryLd < N - 1) return W2L_EINVAL;
  if (pcmType != W2L_PCM_F32 && pcmType != W2L_PCM_S16) return W2L_EINVAL;
  if (N > 512 || nb > 16 * kFeatWaves * kFeatColTiles || nb > 257 || F > 16 * kFeatWaves) return W2L_EUNSUPPORTED;
  const int W = kFeatRows * St + N - St;
  const int ldS = (nb + 15) / 16 * 16 + 1;
  const size_t ldsBytes = ((size_t)(W + (W >> 5)) + 1 + (size_t)kFeatRows * ldS) * sizeof(float);   // <= 33.8 + 17.5 KiB
  const dim3 grid((unsigned)((maxOut + kFeatRows - 1) / kFeatRows), (unsigned)slots);
  if (pcmType == W2L_PCM_S16)
    hipLaunchKernelGGL(feat_stream_k<int16_t>, grid, dim3(kFeatThreads), ldsBytes, (hipStream_t)stream, (const int16_t*)pcm, maxSamples,
                       tab, carry0, carry1, carryLd, G, H, out, maxOut, N, St, nb, F, d->usePower, d->melFloor, ldS);
  else
    hipLaunchKernelGGL(feat_stream_k<float>, grid, dim3(kFeatThreads), ldsBytes, (hipStream_t)stream, (const float*)pcm, maxSamples, tab,
                       carry0, carry1, carryLd, G, H, out, maxOut, N, St, nb, F, d->usePower, d->melFloor, ldS);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
