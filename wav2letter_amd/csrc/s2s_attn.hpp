// s2s_attn.hpp -- the device routines of the seq2seq attention products, shared by the training kernels (criterion_s2s.hip)
// and the decoder's step kernel (criterion_s2s_decode.hip): 32 queries of one utterance against that utterance's keys and
// values on v_mfma_f32_32x32x2_f32, the score rows staying in LDS between the two products.
#pragma once
#include "common.hpp"

namespace w2l {

typedef float s2s_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kS2sThreads = 256;
constexpr int kS2sQt = 32;                 // queries of a workgroup = M of the MFMA tile
constexpr int kS2sKt = 128;                // keys per score chunk: 32 per wave
constexpr int kS2sHc = 32, kS2sLdc = 36;   // columns of H per staged chunk of the score product; LDS row stride
constexpr int kS2sVt = 32, kS2sLdv = 132;  // keys per staged chunk of the context product (128 columns wide); LDS row stride
constexpr int kS2sStage = (kS2sQt + kS2sKt) * kS2sLdc > kS2sVt * kS2sLdv ? (kS2sQt + kS2sKt) * kS2sLdc : kS2sVt * kS2sLdv;
constexpr int kS2sMaxH = 1024, kS2sMaxT = 1024, kS2sMaxB = 1024;

__device__ __forceinline__ float4 s2s_ld4(const float* p, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ int s2s_tile_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

#define S2S_MFMA4(acc, a, b)                                             \
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);    \
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);    \
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);    \
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0)

// S[r][t] = A[r][0 .. H) . Bm[t][0 .. H) for r < 32 and t < roundup(nK, 128); rows of A past `rows` and keys past nK count as zero
__device__ __forceinline__ void s2s_qk_product(float* S, int ldS, float* stage, const float* A, size_t lda, int rows, bool vecA, const float* Bm,
                                               size_t ldb, int nK, bool vecB, int H) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  float* sa = stage;
  float* sb = stage + kS2sQt * kS2sLdc;
  for (int t0 = 0; t0 < nK; t0 += kS2sKt) {
    s2s_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < H; c0 += kS2sHc) {
      __syncthreads();
      {
        const int r = tid >> 3, c = (tid & 7) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows) v = s2s_ld4(A + (size_t)r * lda + c0 + c, vecA);
        *reinterpret_cast<float4*>(sa + r * kS2sLdc + c) = v;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = tid + i * kS2sThreads, r = e >> 3, c = (e & 7) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 + r < nK) v = s2s_ld4(Bm + (size_t)(t0 + r) * ldb + c0 + c, vecB);
        *reinterpret_cast<float4*>(sb + r * kS2sLdc + c) = v;
      }
      __syncthreads();
      if (t0 + wave * 32 >= nK) continue;   // wave-uniform: this wave's keys are all masked
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int kl = it * 8 + lh * 4;
        const float4 a = *reinterpret_cast<const float4*>(sa + li * kS2sLdc + kl);
        const float4 b = *reinterpret_cast<const float4*>(sb + (wave * 32 + li) * kS2sLdc + kl);
        S2S_MFMA4(acc, a, b);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) S[s2s_tile_row(r, lh) * ldS + t0 + wave * 32 + li] = acc[r];
  }
  __syncthreads();
}

// epi(r, c, sum_t S[r][t] Vm[t][c]) for r < 32, c < H; S holds zeros from nK to the next multiple of 32
template <class Epi>
__device__ __forceinline__ void s2s_pv_product(const float* S, int ldS, float* stage, const float* Vm, size_t ldv, int nK, bool vecV, int H, Epi epi) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  for (int c0 = 0; c0 < H; c0 += 128) {
    s2s_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int cw = c0 + wave * 32;   // H is a multiple of 32: a wave's 32 columns lie inside H or outside, never across
    for (int t0 = 0; t0 < nK; t0 += kS2sVt) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = tid + i * kS2sThreads, r = e >> 5, c = (e & 31) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 + r < nK && c0 + c < H) v = s2s_ld4(Vm + (size_t)(t0 + r) * ldv + c0 + c, vecV);
        *reinterpret_cast<float4*>(stage + r * kS2sLdv + c) = v;
      }
      __syncthreads();
      if (cw >= H) continue;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int kl = it * 8 + lh * 4;
        const float4 a = *reinterpret_cast<const float4*>(S + li * ldS + t0 + kl);
        const float* bp = stage + kl * kS2sLdv + wave * 32 + li;
        const float4 b = make_float4(bp[0], bp[kS2sLdv], bp[2 * kS2sLdv], bp[3 * kS2sLdv]);
        S2S_MFMA4(acc, a, b);
      }
    }
    if (cw < H) {
#pragma unroll
      for (int r = 0; r < 16; ++r) epi(s2s_tile_row(r, lh), cw + li, acc[r]);
    }
  }
}

static inline int s2s_lds_stride(int T) { return (T + 127) / 128 * 128 + 4; }
static inline size_t s2s_lds_bytes(int T) { return ((size_t)kS2sQt * s2s_lds_stride(T) + kS2sStage) * sizeof(float); }
static inline bool s2s_aligned(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

}  // namespace w2l
