// criterion_asg_dpp.hpp -- 32 x 32 matrix-vector products on DPP row rotations, and the ViterbiPath kernels built on them, for
// N <= 31 states (the ASG letter sets: N = 30 for LibriSpeech, recipes/conv_glu/librispeech/train.cfg); included by criterion_fcc.hip.
// The FullConnectionCriterion scans that use the same products are in criterion_asg_mitm.hpp.
//
// Replaces Flashlight's fl::lib::{cpu,cuda}::ViterbiPath<float> (un-vendored; call site recipes/slimIPL/src/Train.cpp:838; math
// SURVEY.md App. B.3; CPU restatement oracle/criterion_oracle.c).
//
// A frame of these scans is a 32 x 32 matrix-vector product whose result feeds the next frame: T dependent steps, so what counts
// is the number of instructions ONE wave must issue per frame.  Broadcasting every state through v_readlane into an SGPR operand
// (fcc_fwd_small, viterbi_small: the N = 32 .. 64 kernels of criterion_fcc.hip) is 32 + 16 instructions.  Here the product runs on
// DPP row rotations: the 64 lanes are 4 rows of 16; every row holds one 16-state half of the vector and computes, with 16
// `v_fmac_f32_dpp row_ror:n` (rotation and multiply-add in ONE instruction, no broadcast at all), the partial sums of 16 output
// states over the 16 inputs it holds: 4 rows = the 4 blocks of the 32 x 32 matrix.  The two partials of an output state are added
// across rows by ONE v_permlane32_swap (rows 0+2, 1+3) or v_permlane16_swap (rows 0+1, 2+3) -- gfx950 instructions.  A combine
// leaves each half of the result in TWO rows, but not the two rows the same step needs as input, so the steps ALTERNATE between
// two arrangements and two register sets of the matrix:
//   arrangement H: rows hold halves [0,0,1,1]  --step A: rows produce halves [0,1,0,1], permlane32 combine-->  arrangement G
//   arrangement G: rows hold halves [0,1,0,1]  --step B: rows produce halves [0,0,1,1], permlane16 combine-->  arrangement H
// ~21 chain instructions per frame instead of ~60.  The lane <-> source-lane map of `row_ror:n` is CALIBRATED at kernel start (a
// rotation of the lane index), and the two swap instructions are checked on known values: a semantic surprise poisons the result
// (NaN) instead of producing wrong numbers.
// Viterbi: the same rotations with (+, max): 16 v_add_f32_dpp + 8 v_max3_f32 per frame.  Only delta is on the chain; the
// back-pointers psi_t[i] = first argmax_j(delta_{t-1}[j] + A[i][j]) -- same fp32 sums, first maximum wins, as the oracle's
// strict '>' scan -- are recomputed from the stored delta rows by the parallel kernel vit_psi_k and walked by vit_walk_k.
#pragma once
#include "common.hpp"
#include <type_traits>

namespace w2l {

constexpr int kDppChunk = 16;   // frames per prefetch chunk (even: a frame's arrangement depends on its parity only)

template <int N> __device__ __forceinline__ int dpp_ror_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, 0x120 + N, 0xf, 0xf, true);
}

// sum_n E[n] * u[source lane of row_ror:n]  (n = 0: the lane itself); two accumulators
__device__ __forceinline__ float dpp_dot16(float u, const float (&E)[16]) {
  float a0, a1;
  asm("s_nop 1\n\t"
      "v_mul_f32_e32 %0, %2, %3\n\t"
      "v_mul_f32_dpp %1, %2, %4 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %2, %5 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %2, %6 row_ror:3 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %2, %7 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %2, %8 row_ror:5 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %2, %9 row_ror:6 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %2, %10 row_ror:7 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %2, %11 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %2, %12 row_ror:9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %2, %13 row_ror:10 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %2, %14 row_ror:11 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %2, %15 row_ror:12 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %2, %16 row_ror:13 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %2, %17 row_ror:14 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %2, %18 row_ror:15 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 0"
      : "=&v"(a0), "=&v"(a1)
      : "v"(u), "v"(E[0]), "v"(E[1]), "v"(E[2]), "v"(E[3]), "v"(E[4]), "v"(E[5]), "v"(E[6]), "v"(E[7]), "v"(E[8]), "v"(E[9]),
        "v"(E[10]), "v"(E[11]), "v"(E[12]), "v"(E[13]), "v"(E[14]), "v"(E[15]));
  return a0 + a1;
}

// max_n (A[n] + d[source lane of row_ror:n])  -- the (max, +) form of dpp_dot16: 16 adds with the rotation folded in, 8 v_max3
__device__ __forceinline__ float dpp_maxplus16(float d, const float (&A)[16]) {
  float m, t0, t1;
  asm("s_nop 1\n\t"
      "v_add_f32_e32 %0, %3, %4\n\t"
      "v_add_f32_dpp %1, %3, %5 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %3, %6 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_max3_f32 %0, %0, %1, %2\n\t"
      "v_add_f32_dpp %1, %3, %7 row_ror:3 row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %3, %8 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_max3_f32 %0, %0, %1, %2\n\t"
      "v_add_f32_dpp %1, %3, %9 row_ror:5 row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %3, %10 row_ror:6 row_mask:0xf bank_mask:0xf\n\t"
      "v_max3_f32 %0, %0, %1, %2\n\t"
      "v_add_f32_dpp %1, %3, %11 row_ror:7 row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %3, %12 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_max3_f32 %0, %0, %1, %2\n\t"
      "v_add_f32_dpp %1, %3, %13 row_ror:9 row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %3, %14 row_ror:10 row_mask:0xf bank_mask:0xf\n\t"
      "v_max3_f32 %0, %0, %1, %2\n\t"
      "v_add_f32_dpp %1, %3, %15 row_ror:11 row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %3, %16 row_ror:12 row_mask:0xf bank_mask:0xf\n\t"
      "v_max3_f32 %0, %0, %1, %2\n\t"
      "v_add_f32_dpp %1, %3, %17 row_ror:13 row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %3, %18 row_ror:14 row_mask:0xf bank_mask:0xf\n\t"
      "v_max3_f32 %0, %0, %1, %2\n\t"
      "v_add_f32_dpp %1, %3, %19 row_ror:15 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 0\n\t"
      "v_max_f32_e32 %0, %0, %1"
      : "=&v"(m), "=&v"(t0), "=&v"(t1)
      : "v"(d), "v"(A[0]), "v"(A[1]), "v"(A[2]), "v"(A[3]), "v"(A[4]), "v"(A[5]), "v"(A[6]), "v"(A[7]), "v"(A[8]), "v"(A[9]),
        "v"(A[10]), "v"(A[11]), "v"(A[12]), "v"(A[13]), "v"(A[14]), "v"(A[15]));
  return m;
}

// lanes l and l ^ 32 (rows 0+2, 1+3) / l and l ^ 16 (rows 0+1, 2+3): both lanes receive the combination of the two values
__device__ __forceinline__ void swap32(float p, float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(p), __float_as_int(p), false, false);
  a = __int_as_float(r[0]); b = __int_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float p, float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_int(p), __float_as_int(p), false, false);
  a = __int_as_float(r[0]); b = __int_as_float(r[1]);
}
__device__ __forceinline__ float comb_add32(float p) { float a, b; swap32(p, a, b); return a + b; }
__device__ __forceinline__ float comb_add16(float p) { float a, b; swap16(p, a, b); return a + b; }
__device__ __forceinline__ float comb_max32(float p) { float a, b; swap32(p, a, b); return fmaxf(a, b); }
__device__ __forceinline__ float comb_max16(float p) { float a, b; swap16(p, a, b); return fmaxf(a, b); }

// the two arrangements of a 32-vector over the 4 rows of a wave
struct DppGeom {
  int sH, sG;        // the state this lane holds in arrangement H (rows hold halves [0,0,1,1]) / G ([0,1,0,1])
  bool primH, primG; // this lane is the copy that loads / stores the state (every state lives in two lanes)
  bool ok;           // the swap instructions behave as the schedule assumes
};
__device__ __forceinline__ DppGeom dpp_geom(int lane) {
  DppGeom g;
  const int row = lane >> 4, c = lane & 15;
  g.sH = 16 * (row >> 1) + c;
  g.sG = 16 * (row & 1) + c;
  g.primH = (row & 1) == 0;
  g.primG = row < 2;
  const float v = (float)(1 << row);
  const float want32 = (row & 1) ? 10.f : 5.f, want16 = (row >> 1) ? 12.f : 3.f;
  g.ok = __all(comb_add32(v) == want32 && comb_add16(v) == want16);
  return g;
}

// the matrix registers of the two steps.  f(i, j): entry "to i from j" of the operator that is applied (E, E^T, A as the caller
// defines it; i, j in 0..31).  Step A: the lane produces state sG from the inputs of arrangement H; step B: sH from G.
template <class F>
__device__ __forceinline__ void dpp_tables(int lane, const DppGeom& g, F f, float (&TA)[16], float (&TB)[16]) {
  int src[16];
  src[0] = lane;
  src[1] = dpp_ror_i<1>(lane); src[2] = dpp_ror_i<2>(lane); src[3] = dpp_ror_i<3>(lane); src[4] = dpp_ror_i<4>(lane);
  src[5] = dpp_ror_i<5>(lane); src[6] = dpp_ror_i<6>(lane); src[7] = dpp_ror_i<7>(lane); src[8] = dpp_ror_i<8>(lane);
  src[9] = dpp_ror_i<9>(lane); src[10] = dpp_ror_i<10>(lane); src[11] = dpp_ror_i<11>(lane); src[12] = dpp_ror_i<12>(lane);
  src[13] = dpp_ror_i<13>(lane); src[14] = dpp_ror_i<14>(lane); src[15] = dpp_ror_i<15>(lane);
#pragma unroll
  for (int n = 0; n < 16; ++n) {
    const int srow = src[n] >> 4, sc = src[n] & 15;
    TA[n] = f(g.sG, 16 * (srow >> 1) + sc);   // the source lane holds (arrangement H) state 16 (srow >> 1) + sc
    TB[n] = f(g.sH, 16 * (srow & 1) + sc);    // ... (arrangement G) state 16 (srow & 1) + sc
  }
}

// maximum over the lanes that hold the states once: arrangement G -> rows 0, 1; arrangement H -> rows 0, 2 (uniform result)
template <bool ARR_G>
__device__ __forceinline__ float dpp_state_max(float v) {
  asm volatile(
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 0"
      : "+v"(v));
  return fmaxf(readlane(v, 0), readlane(v, ARR_G ? 16 : 32));
}

// ------------------------------------------------------------------------------------------------ Viterbi
__global__ __launch_bounds__(64) void vit_fwd_dpp(int T, int N, const float* __restrict__ x, const float* __restrict__ trans,
                                                  float* __restrict__ deltaAll) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const DppGeom g = dpp_geom(lane);
  const float NEG = -INFINITY;
  float AA[16], AB[16];
  dpp_tables(lane, g, [&](int i, int j) -> float { return (i < N && j < N) ? trans[(size_t)i * N + j] : NEG; }, AA, AB);
  const bool actG = g.sG < N, actH = g.sH < N;
  const float* xb = x + (size_t)b * T * N;
  float* db = deltaAll + (size_t)b * T * N;

  float xc[kDppChunk], xn[kDppChunk];
#pragma unroll
  for (int s = 0; s < kDppChunk; ++s) {
    const bool odd = s & 1;
    const bool act = odd ? actG : actH;
    const int st = odd ? g.sG : g.sH;
    xc[s] = (act && s < T) ? xb[(size_t)s * N + st] : 0.f;
  }
#pragma unroll
  for (int s = 0; s < kDppChunk; ++s) asm volatile("" : "+v"(xc[s]));   // landed before the loop: no pending load at its head
  float d = NEG;
  for (int t0 = 0; t0 < T; t0 += kDppChunk) {
#pragma unroll
    for (int s = 0; s < kDppChunk; ++s) {
      const int tn = t0 + kDppChunk + s;
      const bool odd = s & 1;
      const bool act = odd ? actG : actH;
      const int st = odd ? g.sG : g.sH;
      xn[s] = (act && tn < T) ? xb[(size_t)tn * N + st] : 0.f;
    }
    float ds[kDppChunk];
    auto frames = [&](auto full) {
#pragma unroll
      for (int s = 0; s < kDppChunk; ++s) {
        const int t = t0 + s;
        ds[s] = NEG;
        if (decltype(full)::value || t < T) {
          const bool odd = s & 1;
          const bool act = odd ? actG : actH;
          if (t == 0) {
            d = act ? xc[s] : NEG;
          } else {
            float best;
            if (odd) best = comb_max32(dpp_maxplus16(d, AA));
            else best = comb_max16(dpp_maxplus16(d, AB));
            d = act ? best + xc[s] : NEG;
          }
          ds[s] = d;
        }
      }
    };
    if (t0 + kDppChunk <= T) frames(std::true_type{});
    else frames(std::false_type{});
    // the prefetched chunk is consumed BEFORE the frames' stores are issued: hipcc waits vmcnt(0) at the first use of a loaded
    // register when stores may have been issued behind the load (the counter is shared and in order), i.e. a store round trip
    // per chunk if the stores come first -- this way the loads have had the whole chunk to land and the stores drain meanwhile
#pragma unroll
    for (int s = 0; s < kDppChunk; ++s) asm volatile("" : "+v"(xn[s]));
#pragma unroll
    for (int s = 0; s < kDppChunk; ++s) {
      const int t = t0 + s;
      const bool odd = s & 1;
      const bool st = odd ? (g.primG && actG) : (g.primH && actH);
      const int sx = odd ? g.sG : g.sH;
      if (st && t < T) db[(size_t)t * N + sx] = g.ok ? ds[s] : __builtin_nanf("");
    }
#pragma unroll
    for (int s = 0; s < kDppChunk; ++s) xc[s] = xn[s];
  }
}

// back-pointers from the stored delta rows + the walk, in two parallel kernels (a frame of a serial walk is a dependent LDS
// read: 2000 of them cost more than the whole scan -- vit_bt_k of the first version, 520 us at T = 2000):
//   vit_psi_k   grid (chunks of kVpChunk frames, B): psi_t[i] = first j maximising delta_{t-1}[j] + A[i][j] (fp32 sums, strict '>'
//               upwards in j: the oracle's scan) for the chunk's frames -> psi bytes [B][T][32]; then the chunk's back-pointers
//               are COMPOSED: comp_c[i] = the state at the chunk's first frame - 1 when the path is in state i at its last frame
//               (kVpChunk dependent LDS reads, every chunk of every utterance in parallel);
//   vit_walk_k  one wave per utterance: the end state of every chunk by walking the composed maps (T / kVpChunk dependent
//               steps), then every lane walks ONE chunk from its end state through the psi bytes staged in LDS.
// Serial depth 2 * kVpChunk + T / kVpChunk steps instead of T.
constexpr int kVpChunk = 32;
struct VitBtWs {
  unsigned char* psi;    // [B][T][32]
  unsigned char* comp;   // [B][nChunks][32]
};
__host__ __device__ inline int vit_chunks(int T) { return (T - 1 + kVpChunk - 1) / kVpChunk; }   // frames 1 .. T-1 in chunks
__host__ __device__ inline VitBtWs vit_bt_ws(void* base, int B, int T, int N) {
  VitBtWs w;
  char* p = (char*)base + align_up((size_t)B * T * N * sizeof(float), 256);   // behind the delta rows
  w.psi = (unsigned char*)p; p += align_up((size_t)B * T * 32, 256);
  w.comp = (unsigned char*)p;
  return w;
}
__host__ __device__ inline size_t vit_dpp_ws_bytes(int B, int T, int N) {
  return align_up((size_t)B * T * N * sizeof(float), 256) + align_up((size_t)B * T * 32, 256) +
         align_up((size_t)B * (size_t)(vit_chunks(T) + 1) * 32, 256);
}

// chunk c covers frames t = 1 + c * kVpChunk .. min(T - 1, (c + 1) * kVpChunk)
__global__ __launch_bounds__(64) void vit_psi_k(int T, int N, const float* __restrict__ trans, const float* __restrict__ deltaAll,
                                                VitBtWs ws) {
  __shared__ float sA[32 * 33];
  __shared__ float sD[kVpChunk * 32];          // delta rows t - 1 of the chunk's frames
  __shared__ unsigned char sPsi[kVpChunk * 32];
  const int c = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int tlo = 1 + c * kVpChunk;
  int thi = tlo + kVpChunk - 1;
  if (thi > T - 1) thi = T - 1;
  const int nf = thi - tlo + 1;
  const float* db = deltaAll + (size_t)b * T * N;
  for (int e = lane; e < N * N; e += 64) sA[(e / N) * 33 + (e % N)] = trans[e];
  for (int e = lane; e < nf * N; e += 64) sD[(e / N) * 32 + (e % N)] = db[(size_t)(tlo - 1) * N + e];
  __syncthreads();
  // two frames at a time: lanes 0..31 the even, 32..63 the odd frame of a pair; lane & 31 = state i
  const int i = lane & 31, half = lane >> 5;
  for (int f = half; f < nf; f += 2) {
    if (i < N) {
      const float* dr = sD + f * 32;
      const float* ar = sA + i * 33;
      float best = dr[0] + ar[0];
      int arg = 0;
      for (int j = 1; j < N; ++j) {
        const float v = dr[j] + ar[j];
        if (v > best) { best = v; arg = j; }
      }
      sPsi[f * 32 + i] = (unsigned char)arg;
    }
  }
  __syncthreads();
  unsigned char* pg = ws.psi + ((size_t)b * T + tlo) * 32;
  for (int e = lane; e < nf * 32; e += 64) pg[e] = sPsi[e];
  if (lane < 32) {   // compose from the chunk's last frame down: state at frame tlo - 1 given state `lane` at frame thi
    int cur = lane < N ? lane : 0;
    for (int f = nf - 1; f >= 0; --f) cur = sPsi[f * 32 + cur];
    ws.comp[((size_t)b * (vit_chunks(T) + 1) + c) * 32 + lane] = (unsigned char)cur;
  }
}

// stage = 1: the utterance's psi bytes fit in LDS (T <= ~4800) and are walked there; 0: walked in global memory
__global__ __launch_bounds__(64) void vit_walk_k(int T, int N, int stage, const float* __restrict__ deltaAll, VitBtWs ws,
                                                 int* __restrict__ path) {
  extern __shared__ unsigned char sm[];   // [psi bytes of the utterance [T][32],] comp [nChunks][32], end states [nChunks + 1] ints
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nC = vit_chunks(T);
  const size_t psiBytes = stage ? (size_t)T * 32 : 0;
  unsigned char* sComp = sm + psiBytes;
  int* sEnd = (int*)(sm + ((psiBytes + (size_t)nC * 32 + 15) & ~(size_t)15));
  const unsigned char* sPsi = stage ? sm : ws.psi + (size_t)b * T * 32;
  {   // stage (16 B per lane and load)
    const uint4* src = (const uint4*)(ws.psi + (size_t)b * T * 32);
    uint4* dst = (uint4*)sm;
    if (stage)
      for (int e = lane; e < T * 2; e += 64) dst[e] = src[e];
    const uint4* cs = (const uint4*)(ws.comp + (size_t)b * (nC + 1) * 32);
    uint4* cd = (uint4*)sComp;
    for (int e = lane; e < nC * 2; e += 64) cd[e] = cs[e];
  }
  // final state: first argmax_i delta_{T-1}[i]
  const float* db = deltaAll + (size_t)b * T * N;
  const float v = lane < N ? db[(size_t)(T - 1) * N + lane] : -INFINITY;
  const float m = wave_max(v);
  const unsigned long long eq = __ballot(lane < N && v == m);
  int cur = eq ? __ffsll((long long)eq) - 1 : 0;
  __syncthreads();
  if (lane == 0) {   // end state of chunk c = state at frame min(T - 1, (c + 1) kVpChunk); sEnd[c] for c = nC - 1 .. 0, sEnd[-1] -> frame 0
    for (int c = nC - 1; c >= 0; --c) {
      sEnd[c + 1] = cur;
      cur = sComp[c * 32 + cur];
    }
    sEnd[0] = cur;   // the state at frame 0
  }
  __syncthreads();
  int* pb = path + (size_t)b * T;
  if (lane == 0) pb[0] = sEnd[0];
  for (int c = lane; c < nC; c += 64) {
    const int tlo = 1 + c * kVpChunk;
    int thi = tlo + kVpChunk - 1;
    if (thi > T - 1) thi = T - 1;
    int s = sEnd[c + 1];
    for (int t = thi; t >= tlo; --t) {
      pb[t] = s;
      s = sPsi[(size_t)t * 32 + s];
    }
  }
}

}  // namespace w2l

