// gemm_smallm.hip -- w2l_gemm_bf16_smallm: C[M][N] = A[M][K] . B[N][K]^T on bf16 operand images with fp32 accumulation, for the
// few rows (M = slots x a few frames) of a streaming step (host/stream.cpp).  The 128 x 128 and 256 x 256 tiles of w2l_gemm_bf16 are
// made for M in the thousands: at M = 144 a 1200-column product is 20 tiles on 256 CUs.
//
// Shape of the work.  The weight image B [N][ldb] is cut into slabs of 16 rows (32 from N = 4096 up); one workgroup takes one slab,
// the WHOLE reduction and ALL rows of A: wave w holds the accumulators of the 32-row tiles w * MT .. w * MT + MT - 1 of C (MT <= 4,
// at most 8 waves: 1024 rows, the cap).  Every wave reads the slab's weight fragments itself -- the first read of a cache line comes
// from HBM, the other waves of the workgroup hit the cache -- so each weight byte leaves HBM once per call whatever M is.  Operand
// fragments come straight from global memory into the registers of v_mfma_f32_32x32x16_bf16 (lane l: row l & 31, the 8 bf16 at
// k = 16 s + 8 (l >> 5)); the four loads of a 64-k step consume whole 128-byte lines of every row.  In a 16-row slab the upper 16
// columns of the MFMA repeat the lower ones (same addresses: no traffic) and are dropped; the MFMA rate is nowhere near the bound.
//
// K IS NOT SPLIT, and the k order is the natural one.  Element (m, n) is ONE chain of MFMAs over k = 0, 16, 32, ... from a zero
// accumulator -- exactly the chain of gemm128h_kernel / gemm256h_kernel (gemm_bf16g.hpp) wherever w2l_gemm_bf16 does not split K
// itself (K < 4096: every product of the streaming recipe), followed by the same epilogue arithmetic.  So the result has the BITS of
// w2l_gemm_bf16, and a mixed-precision session on this kernel equals the trainer's own forward bit for bit.  That is not a nicety:
// a first version split K over workgroups (partial sums added in chunk order by a second kernel) and was 5000 times inside the
// fp32 error bound -- and the session on it missed the whole-recipe bar by a factor of 6 (1.2e-2 against 2e-3 of the largest
// emission).  Every bf16 rounding of an activation is a discontinuity; a 1e-7 difference in a sum flips a rounding here and there,
// each flip is a 4e-3 difference in one operand, which flips many more roundings in the next block, and after 18 TDS blocks the
// difference has grown to the size of the bf16 noise itself (the mixed-precision and the fp32 forward differ by 2.2e-2 on that
// network).  Any summation order but the trainer's ends there; occupancy comes from narrow slabs instead of a K split.
//
// Row independence, bit for bit: the position of row m inside its tile does not enter the arithmetic of the MFMA and no value of
// another row is ever added to it, so row m of C depends on row m of A and on B only, whatever M is and whatever the other rows
// hold (NaN included).  No workspace, no atomics, one launch.
#include "common.hpp"

namespace w2l {
namespace {

typedef __bf16 sm_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sm_bf16x2 __attribute__((ext_vector_type(2)));
typedef float sm_f32x2 __attribute__((ext_vector_type(2)));
typedef float sm_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSmallMCap = 1024;     // rows: 8 waves x 4 tiles of 32
constexpr int kSmallMWaves = 8;
constexpr int kSmallMWideN = 4096;   // from here on 32-row slabs fill the chip; below, 16-row slabs double the workgroups

inline int smallm_slab(int N) { return N >= kSmallMWideN ? 32 : 16; }

struct SmallMOut {
  float* C;
  const float* bias;
  const float* addend;
  uint16_t* img;
  size_t ldImg;
  int ldc, relu, M, N;
};

__device__ __forceinline__ uint16_t smallm_bf16(float v) {
  const sm_f32x2 p = {v, 0.f};
  const uint32_t bits = __builtin_bit_cast(uint32_t, __builtin_convertvector(p, sm_bf16x2));   // v_cvt_pk_bf16_f32: nearest even
  return (uint16_t)(bits & 0xffffu);
}

// v = sum (+ bias[n]) (ReLU) (+ addend[m][n]) -> C[m][n] and / or the bf16 row image; m < M and n < N checked by the caller
__device__ __forceinline__ void smallm_store(const SmallMOut& o, int m, int n, float v) {
  v += o.bias ? o.bias[n] : 0.f;   // (always an addition, as gemm128_epilogue: the bits of w2l_gemm_bf16, -0 included)
  if (o.relu) v = fmaxf(v, 0.f);
  if (o.addend) v += o.addend[(size_t)m * o.ldc + n];
  if (o.C) o.C[(size_t)m * o.ldc + n] = v;
  if (o.img) o.img[(size_t)m * o.ldImg + n] = smallm_bf16(v);
}

// grid (slabs of `sw` = 16 or 32 weight rows), block 64 x waves; wave w: tiles w * MT .. + MT - 1 of 32 rows.  Rows past M and
// weight rows past N are read from the last valid row (in bounds) and never stored.  k64: 64-k steps in all; lda, ldb >= 64 * k64.
template <int MT>
__global__ __launch_bounds__(64 * kSmallMWaves) void gemm_bf16_smallm_kernel(const uint16_t* __restrict__ A, int lda,
                                                                             const uint16_t* __restrict__ B, int ldb, int k64, int sw,
                                                                             SmallMOut o) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * sw, lc = li & (sw - 1);   // MFMA column li holds weight row n0 + lc
  const int kb = 0, ke = k64;

  const int nrow = n0 + lc < o.N ? n0 + lc : o.N - 1;
  const uint4* bp = (const uint4*)(B + (size_t)nrow * ldb + 8 * lh);
  const uint4* ap[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = (wave * MT + t) * 32 + li;
    ap[t] = (const uint4*)(A + (size_t)(m < o.M ? m : o.M - 1) * lda + 8 * lh);
  }

  sm_f32x16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // one 64-k step = 8 uint4 per row (128 bytes); MFMA j of the step takes k = 16 j + 8 lh .. + 7: this lane's uint4 8 k + 2 j (its
  // pointer already carries the 8 lh elements).  The chain is serial in k, the LOADS need not be: D steps of fragments are in
  // flight per wave (a ring of register stages, refilled as soon as a stage's MFMAs are issued) -- with one step in flight every
  // 64 k cost a full trip to HBM and the kernel ran at the speed of w2l_gemm_bf16.  A stage past the end re-reads the
  // last step (in bounds) and is never multiplied.
  constexpr int D = MT == 1 ? 6 : MT == 2 ? 3 : 2;
  uint4 b[D][4], a[D][MT][4];
  auto fill = [&](int d, int k) {
    const size_t at = (size_t)(k < ke ? k : ke - 1) * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) b[d][j] = bp[at + 2 * j];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[d][t][j] = ap[t][at + 2 * j];
  };
#pragma unroll
  for (int d = 0; d < D; ++d) fill(d, kb + d);
  for (int k = kb; k < ke; k += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (k + d < ke) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const sm_bf16x8 fb = __builtin_bit_cast(sm_bf16x8, b[d][j]);
#pragma unroll
          for (int t = 0; t < MT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(sm_bf16x8, a[d][t][j]), fb, acc[t], 0, 0, 0);
        }
      }
      fill(d, k + d + D);
    }
  }

  // D layout of the 32x32 MFMA: column on the lane (li), row (r & 3) + 8 (r >> 2) + 4 lh in register r
  const int n = n0 + li;
  if (li >= sw || n >= o.N) return;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = (wave * MT + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (m >= o.M) continue;
      smallm_store(o, m, n, acc[t][r]);
    }
}

}  // namespace
}  // namespace w2l

using namespace w2l;

W2L_API int w2l_gemm_bf16_smallm_max_m(void) { return kSmallMCap; }

// pure host.  The kernel needs no workspace today (one launch, no partial sums); the query and the two arguments stay in the entry
// point so that a variant that needs one does not change the ABI
W2L_API size_t w2l_gemm_bf16_smallm_workspace_bytes(int M, int N, int K) {
  (void)M; (void)N; (void)K;
  return 0;
}

W2L_API int w2l_gemm_bf16_smallm(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc,
                                 const float* bias, int relu, const float* addend, const w2l_bf16_image_sink* image, void* workspace,
                                 size_t workspaceBytes, w2l_stream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || !A || !B) return W2L_EINVAL;
  const int kp = (K + 63) / 64 * 64;
  if (lda < K || ldb < K) return W2L_EINVAL;
  if (lda < kp || ldb < kp || (lda & 7) || (ldb & 7) || ((uintptr_t)A & 15) || ((uintptr_t)B & 15)) return W2L_EINVAL;
  if (image && image->transposed) return W2L_EINVAL;   // the row image only: what the next forward product reads
  uint16_t* img = image ? image->rowMajor : nullptr;
  if (!C && !img) return W2L_EINVAL;
  if (ldc < N || (img && image->ldRows < (size_t)N)) return W2L_EINVAL;
  if (M > kSmallMCap) return W2L_EUNSUPPORTED;
  // probe library: the caller's fall-back (w2l_gemm_bf16) for every product, for A/B runs of a bf16 streaming session
  static const bool off = tune_env("W2L_SMALLM_OFF") != nullptr;
  if (off) return W2L_EUNSUPPORTED;
  (void)workspace; (void)workspaceBytes;

  hipStream_t s = (hipStream_t)stream;
  SmallMOut o{C, bias, addend, img, img ? image->ldRows : 0, ldc, relu ? 1 : 0, M, N};
  const int tiles = (M + 31) / 32;
  const int mt = (tiles + kSmallMWaves - 1) / kSmallMWaves;   // 1 .. 4
  const int waves = (tiles + mt - 1) / mt;
  const int sw = smallm_slab(N);
  const dim3 grid((unsigned)((N + sw - 1) / sw)), block(64u * (unsigned)waves);
  const int k64 = kp / 64;
  switch (mt) {
    case 1: hipLaunchKernelGGL(gemm_bf16_smallm_kernel<1>, grid, block, 0, s, A, lda, B, ldb, k64, sw, o); break;
    case 2: hipLaunchKernelGGL(gemm_bf16_smallm_kernel<2>, grid, block, 0, s, A, lda, B, ldb, k64, sw, o); break;
    case 3: hipLaunchKernelGGL(gemm_bf16_smallm_kernel<3>, grid, block, 0, s, A, lda, B, ldb, k64, sw, o); break;
    default: hipLaunchKernelGGL(gemm_bf16_smallm_kernel<4>, grid, block, 0, s, A, lda, B, ldb, k64, sw, o); break;
  }
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
