// gemm_split.hpp -- split-bf16 GEMM ("3xBF16", "fast fp32"): fp32 operands, results and accumulation, the multiply on three
// v_mfma_f32_32x32x16_bf16 products per fp32 product.  Every operand element is split in registers on its way into LDS,
//   hi = rne_bf16(x),   lo = rne_bf16(x - float(hi))        (the subtraction is exact in fp32; a padding zero gives hi = lo = 0)
// and a . b is taken as a_lo . b_hi + a_hi . b_lo + a_hi . b_hi -- accumulated in THAT order, small terms first, into one fp32
// accumulator per 16-k step; lo . lo (below 2^-18 |a||b|) is never computed.  x - hi - lo is at most 2^-18 |x|, so an element of C
// is within (2^-16 + K 2^-23) (|A| |B|)[m][n] of the exact product: two orders of magnitude tighter than a bf16 product, about
// three times looser than the fp32 MFMA chain.  Contract: finite operands below 2^127 in magnitude --
// hi rounds to infinity above the largest finite bf16 and the result is then not finite.
//
// Tile 128 x 128 x 32, 4 waves x (2 x 2) 32x32 accumulators, the staging contract of gemm_bf16.hpp: any layout (k-contiguous or
// k-rows), any alignment (vector or scalar loads), any K, the next K tile's global loads in flight under the current tile's MFMAs,
// gemm128_epilogue at the end (bias / ReLU / dropout / mask / addend / accumulate).  LDS holds hi and lo of an operand tile as two
// PLANES, each the [row][32 k] image of gemm_bf16.hpp (64-byte pitch, 16-byte chunks XOR-swizzled by the row): the stores keep the
// shapes whose bank behaviour is known (8-byte stores from a k-contiguous source, packed (k, k+1) dwords from a k-row source) and
// every fragment read stays a conflict-free ds_read_b128 -- hi and lo side by side in one row would double the pitch to 128 bytes
// and put rows 2 apart on the same banks.  128 x 32 x 2 B x 2 planes x 2 operands x 2 stages = 64 KiB: two workgroups per CU.
// Per wave and K tile: 16 fragment reads, 24 MFMAs.  A 256 x 128 tile would halve the reads per MFMA but needs 96 KiB of LDS, one
// workgroup per CU: not built.
//
// Long reductions with few tiles (the weight gradients) are cut over blockIdx.z into partial slabs in the stream's scratch
// (sk_scratch) that a second launch adds in slice order: no atomics, the same bits every run.
//
// This header is compiled in a translation unit of its own (gemm_split.hip) without packed fp32 arithmetic, like conv_depthwise.hip
// and rnn.hip: the split's subtraction must be the exact scalar one.
#pragma once
#include "gemm.hpp"

namespace w2l {
namespace split {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kRowDw = 16;                        // dwords per LDS row: 32 bf16, no padding
constexpr int kPlaneDw = 128 * kRowDw;            // one plane (hi or lo) of one operand tile
constexpr int kStageDw = 4 * kPlaneDw;            // A hi, A lo, B hi, B lo
constexpr size_t kLdsBytes = 2 * (size_t)kStageDw * 4;   // two stages = 64 KiB

__device__ __forceinline__ uint32_t pack2(float a, float b) {
  const f32x2 v = {a, b};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);   // v_cvt_pk_bf16_f32: round to nearest even
  return __builtin_bit_cast(uint32_t, h);
}
// (a, b) -> packed hi pair, packed lo pair
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pack2(a, b);
  lo = pack2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}
// chunk c (8 k) of row i sits at chunk position c ^ ((i >> 2) & 3): gemm_bf16.hpp's bf_chunk
__device__ __forceinline__ int chunk(int row, int c) { return c ^ ((row >> 2) & 3); }

// Operand op(k, i): KC = true: element at p[i*ld + k] (k contiguous), false: p[k*ld + i] ("k-rows").  vec: float4-able.
// Thread map of the [32 k][128 i] tile, 16 floats per thread -- KC: 4 k at 4 (tid & 7), rows (tid >> 3) + 32 j;
// k-rows: 4 i at 4 (tid & 31), the k pairs (tid >> 5) and (tid >> 5) + 8.  Nothing outside [0, extent) x [0, K) is read.
template <bool KC>
struct Op {
  const float* p;
  int ld, extent, K;
  bool vec;
  __device__ __forceinline__ void load(float (&r)[16], int i0, int k0, int tid) const {
    if (KC) {
      const int gk = k0 + 4 * (tid & 7);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int gi = i0 + (tid >> 3) + 32 * j;
        const float* src = p + (size_t)(gi < extent ? gi : extent - 1) * ld + gk;
        if (vec && gi < extent && gk + 3 < K) {
          const float4 v = *(const float4*)src;
          r[4 * j] = v.x; r[4 * j + 1] = v.y; r[4 * j + 2] = v.z; r[4 * j + 3] = v.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) r[4 * j + e] = (gi < extent && gk + e < K) ? src[e] : 0.f;
        }
      }
    } else {
      const int gi = i0 + 4 * (tid & 31), kp = tid >> 5;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int gk = k0 + 2 * (kp + 8 * j) + h;
          const float* src = p + (size_t)(gk < K ? gk : K - 1) * ld + gi;
          float* d = &r[8 * j + 4 * h];
          if (vec && gk < K && gi + 3 < extent) {
            const float4 v = *(const float4*)src;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = (gk < K && gi + e < extent) ? src[e] : 0.f;
          }
        }
    }
  }
  // split and store: `hi` is the operand's hi plane of one stage, its lo plane follows it
  __device__ __forceinline__ void store(uint32_t* hi, const float (&r)[16], int tid) const {
    uint32_t* lo = hi + kPlaneDw;
    if (KC) {
      const int kq = tid & 7;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = (tid >> 3) + 32 * j;
        const int at = row * kRowDw + 4 * chunk(row, kq >> 1) + 2 * (kq & 1);
        uint2 h, l;
        split2(r[4 * j], r[4 * j + 1], h.x, l.x);
        split2(r[4 * j + 2], r[4 * j + 3], h.y, l.y);
        *(uint2*)(hi + at) = h;
        *(uint2*)(lo + at) = l;
      }
    } else {
      const int iq = tid & 31, kp = tid >> 5;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int kpair = kp + 8 * j;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 4 * iq + e;
          const int at = row * kRowDw + 4 * chunk(row, kpair >> 2) + (kpair & 3);
          uint32_t h, l;
          split2(r[8 * j + e], r[8 * j + 4 + e], h, l);
          hi[at] = h;
          lo[at] = l;
        }
      }
    }
  }
};

#define W2L_SPLIT_MFMA(c, a, b) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

// grid (tilesN, tilesM, splitK); splitK > 1: partial[z][M][N] (plain row-major fp32), no epilogue
template <bool AKC, bool BKC>
__global__ __launch_bounds__(256, 2) void gemm128_split_kernel(Op<AKC> aop, Op<BKC> bop, GemmOut out, int ktPer, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smemRaw[];
  uint32_t* smem = (uint32_t*)smemRaw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int li = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.y * 128, n0 = blockIdx.x * 128;
  const int ktAll = (out.K + 31) / 32;
  const int ktBegin = blockIdx.z * ktPer;
  int ktEnd = ktBegin + ktPer;
  if (ktEnd > ktAll) ktEnd = ktAll;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float ra[16], rb[16];
  if (ktBegin < ktEnd) {
    aop.load(ra, m0, ktBegin * 32, tid);
    bop.load(rb, n0, ktBegin * 32, tid);
    aop.store(smem, ra, tid);
    bop.store(smem + 2 * kPlaneDw, rb, tid);
  }
  __syncthreads();
  // fragment offsets (dwords) inside a plane: rows wm + li (+32) of A, wn + li (+32) of B, logical chunk 2 ks + lh
  int fa[2][2], fb[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int rowA = wm + li + 32 * i, rowB = wn + li + 32 * i;
      fa[i][ks] = rowA * kRowDw + 4 * chunk(rowA, 2 * ks + lh);
      fb[i][ks] = 2 * kPlaneDw + rowB * kRowDw + 4 * chunk(rowB, 2 * ks + lh);
    }
  for (int kt = ktBegin; kt < ktEnd; ++kt) {
    const int cur = (kt - ktBegin) & 1;
    const bool more = kt + 1 < ktEnd;
    if (more) {
      aop.load(ra, m0, (kt + 1) * 32, tid);
      bop.load(rb, n0, (kt + 1) * 32, tid);
    }
    const uint32_t* st = smem + cur * kStageDw;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ah[i] = *(const bf16x8*)(st + fa[i][ks]);
        al[i] = *(const bf16x8*)(st + fa[i][ks] + kPlaneDw);
        bh[i] = *(const bf16x8*)(st + fb[i][ks]);
        bl[i] = *(const bf16x8*)(st + fb[i][ks] + kPlaneDw);
      }
      // the fixed order per accumulator: a_lo b_hi, then a_hi b_lo, then a_hi b_hi; the four accumulators take a term one after
      // the other, so that no MFMA waits for the one issued just before it
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) W2L_SPLIT_MFMA(acc[i][j], al[i], bh[j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) W2L_SPLIT_MFMA(acc[i][j], ah[i], bl[j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) W2L_SPLIT_MFMA(acc[i][j], ah[i], bh[j]);
    }
    if (more) {
      uint32_t* nx = smem + (cur ^ 1) * kStageDw;
      aop.store(nx, ra, tid);
      bop.store(nx + 2 * kPlaneDw, rb, tid);
    }
    __syncthreads();
  }
  if (!partial) {
    gemm128_epilogue(out, m0, n0, acc);
  } else {
    float* dst = partial + (size_t)blockIdx.z * out.M * out.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + j * 32 + li;
        if (n >= out.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (m < out.M) dst[(size_t)m * out.N + n] = acc[i][j][r];
        }
      }
  }
}
#undef W2L_SPLIT_MFMA

// C[m][n] = sum_z partial[z][m][n], slices added in order
static __global__ __launch_bounds__(256) void gemm_split_sum_k(const float* __restrict__ partial, int S, size_t MN, int N, float* __restrict__ C, int ldc) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < MN; e += (size_t)gridDim.x * 256) {
    float s = 0.f;
    for (int z = 0; z < S; ++z) s += partial[(size_t)z * MN + e];
    const size_t m = e / N, n = e - m * N;
    C[m * ldc + n] = s;
  }
}

template <bool AKC, bool BKC>
inline int launch128(const Op<AKC>& a, const Op<BKC>& b, GemmOut o, int epi, hipStream_t s) {
  o.epi = epi;
  const int tilesM = (o.M + 127) / 128, tilesN = (o.N + 127) / 128, tiles = tilesM * tilesN;
  const int ktAll = (o.K + 31) / 32;
  int splitK = 1;
  float* partial = nullptr;
  // few tiles, long reduction, no epilogue (the weight gradients): cut K so that about two workgroups per CU are busy
  if (o.epi == 0 && !o.rowPin && tiles < 256 && ktAll >= 64) {
    splitK = (512 + tiles - 1) / tiles;
    if (splitK > ktAll / 16) splitK = ktAll / 16;
    if (splitK > 16) splitK = 16;
    if (splitK > 1 && (size_t)splitK * o.M * o.N * sizeof(float) <= kSkScratchBytes) partial = sk_scratch(s, kSkScratchBytes);
    if (!partial) splitK = 1;
  }
  const int ktPer = (ktAll + splitK - 1) / splitK;
  splitK = (ktAll + ktPer - 1) / ktPer;
  static const bool attr = hipFuncSetAttribute((const void*)gemm128_split_kernel<AKC, BKC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)kLdsBytes) == hipSuccess;
  if (!attr) return W2L_EHIP;
  prof_begin(s, 2.0 * o.M * (double)o.N * o.K, PROF_GEMM_BF16);   // (counted with the other bf16-MFMA products)
  hipLaunchKernelGGL((gemm128_split_kernel<AKC, BKC>), dim3((unsigned)tilesN, (unsigned)tilesM, (unsigned)splitK), dim3(256), kLdsBytes, s,
                     a, b, o, ktPer, splitK > 1 ? partial : nullptr);
  if (splitK > 1) {
    const size_t MN = (size_t)o.M * o.N;
    const unsigned grid = (unsigned)((MN + 255) / 256 > 2048 ? 2048 : (MN + 255) / 256);
    hipLaunchKernelGGL(gemm_split_sum_k, dim3(grid), dim3(256), 0, s, partial, splitK, MN, o.N, o.C, o.ldc);
  }
  prof_end(s);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

}  // namespace split
}  // namespace w2l
