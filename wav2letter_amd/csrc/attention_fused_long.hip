// attention_fused_long.hip -- the fused attention core for LONG sequences, 192 < T <= 512, head width 32 / 192 / 256: the same
// results and the same C ABI as attention_fused.hip (forward) and attention_fused_bwd.hip (backward), whose kernels keep every score
// tile of a 32-query block in registers and the whole K / V^T image of an (utterance, head) in LDS -- 270 KB at T = 512, d = 256.
// Here the KEYS STREAM through LDS in chunks of CK = 32 or 64 keys, double buffered, shared by the four query waves of a workgroup:
//
//   attn_long_fwd_k    a wave owns 32 queries and computes S^T = K Q^T tile by tile (the short kernel's layout: a lane holds one
//                      query, 16 keys per tile).  TWO PASSES over the keys: pass 1 streams K only and keeps a running row maximum
//                      and a running sum (rescaled when the maximum moves); pass 2 streams K and V^T, recomputes each score tile --
//                      the same instructions on the same operands, hence the same bits --, writes P = exp(s - max) / sum and Pd
//                      once, and accumulates ctx^T += V^T Pd^T in D / 32 accumulator tiles.  (One pass with a rescale would have to
//                      write unnormalised probabilities and run over the [T][T] matrices in HBM again to normalise P and Pd, a
//                      second kernel's worth of traffic, to save the recomputed score tiles.)  Measured, this forward is SLOWER
//                      than the unfused sequence: host/net.cpp does not route to it, the C ABI serves it.
//                      The relative-position term streams with the tiles: table block e serves tiles e - 1 and e, `prev` is carried.
//   attn_long_bwd_q_k  the query side of the backward pass, again two passes: pass A streams V and sums dot_i = sum_j P dPm, pass B
//                      streams V and K^T, recomputes dP^T, forms dS^T, writes the dS^T / Pd^T / dR^T bf16 images and accumulates
//                      dq^T += K^T dS^T + E^T dR^T; table block e is complete after tile e (the skew of attention_fused_bwd.hip).
//   attn_long_bwd_kv_k the key side: 8 waves x 32 image rows per workgroup; the transposed q / dctx image streams through LDS in
//                      chunks of 64 QUERIES, double buffered; D / 32 accumulator tiles per wave.
//   attn_long_prep_k / attn_long_de_reduce_k   E^T image and the fixed-order sum of the [B H] table-gradient partials.
//
// LDS (bytes): two row images [CK][D + 8] + two transposed images [D][CK + 4] + 4 x 8320 skew scratch:
//   d = 32 (CK 64) 52 224, d = 192 (CK 64) 136 704, d = 256 (CK 32) 103 936; key side 2 x [D][72]: 9 216 / 55 296 / 73 728.
// Pitches as in the short family: row image 16 bytes x odd (ds_read_b128), transposed image = 2 mod 4 dwords (ds_read_b64).
// No atomics; bf16 roundings exactly where the unfused w2l_bgemm_bf16 sequence has them; fp32 accumulation and softmax.
#include "attention_fused.hpp"

namespace w2l {

typedef __bf16 al_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 al_bf16x2 __attribute__((ext_vector_type(2)));
typedef float al_f32x2 __attribute__((ext_vector_type(2)));
typedef float al_f32x4 __attribute__((ext_vector_type(4)));
typedef float al_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint32_t al_pack2(float a, float b) {
  const al_f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, al_bf16x2));
}
__device__ __forceinline__ uint16_t al_bf16(float a) { return (uint16_t)al_pack2(a, 0.f); }
__device__ __forceinline__ al_bf16x8 al_pack8(al_f32x4 a, al_f32x4 b) {
  const uint4 u = make_uint4(al_pack2(a[0], a[1]), al_pack2(a[2], a[3]), al_pack2(b[0], b[1]), al_pack2(b[2], b[3]));
  return __builtin_bit_cast(al_bf16x8, u);
}
// k-step u (0 / 1) of a C-layout tile as an MFMA B operand: k slot e of half lh <-> register 8 u + e
__device__ __forceinline__ al_bf16x8 al_frag(const al_f32x16& t, int u) {
  const al_f32x4 a = {t[8 * u], t[8 * u + 1], t[8 * u + 2], t[8 * u + 3]};
  const al_f32x4 c = {t[8 * u + 4], t[8 * u + 5], t[8 * u + 6], t[8 * u + 7]};
  return al_pack8(a, c);
}
__device__ __forceinline__ al_f32x16 al_zero16() {
  al_f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}
__device__ __forceinline__ al_bf16x8 al_read44(const uint16_t* p) {   // two 8-byte LDS / global reads 8 elements apart
  const uint2 lo = *(const uint2*)p, hi = *(const uint2*)(p + 8);
  return __builtin_bit_cast(al_bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
}

template <int D>
struct AlGeom {
  static constexpr int TC = D == 256 ? 1 : 2;    // key tiles of 32 per chunk
  static constexpr int CK = 32 * TC;             // keys per chunk
  static constexpr int KP = D + 8;               // bf16 pitch of a row image [CK][KP]
  static constexpr int VP = CK + 4;              // bf16 pitch of a transposed image [D][VP]
  static constexpr int KS = D / 16;
  static constexpr int rowBytes = CK * KP * 2, trBytes = D * VP * 2;
  static constexpr int NI = CK * (D / 8) / 256;  // staging items per thread of a 256-thread workgroup, either image
  static constexpr int scratchBytes = 4 * 32 * 65 * 4;
  static constexpr int shmem = 2 * rowBytes + 2 * trBytes + scratchBytes;
  static_assert(NI * 256 == CK * (D / 8) && NI * 256 == (CK / 2) * (D / 4), "a chunk is a whole number of items per thread");
};

template <int D>
struct AlStage { al_f32x4 a[AlGeom<D>::NI], c[AlGeom<D>::NI]; };

// ---- row image of a chunk: keys j0 .. j0 + CK of X (this utterance's rows, this head's columns), rows >= T zero.  The loads are
// unconditional from a clamped row and are issued a chunk ahead; the conversion and the LDS stores follow the MFMAs of the chunk
// in flight
template <int D>
__device__ __forceinline__ void al_load_rows(AlStage<D>& r, const float* X, size_t ld, int j0, int T, int tid) {
#pragma unroll
  for (int u = 0; u < AlGeom<D>::NI; ++u) {
    const int idx = u * 256 + tid;
    const int j = idx / (D / 8), c8 = idx - j * (D / 8);
    const float* src = X + (size_t)(j0 + j < T ? j0 + j : T - 1) * ld + 8 * c8;
    r.a[u] = *(const al_f32x4*)src;
    r.c[u] = *(const al_f32x4*)(src + 4);
  }
}
template <int D>
__device__ __forceinline__ void al_store_rows(const AlStage<D>& r, uint16_t* img, int j0, int T, int tid) {
#pragma unroll
  for (int u = 0; u < AlGeom<D>::NI; ++u) {
    const int idx = u * 256 + tid;
    const int j = idx / (D / 8), c8 = idx - j * (D / 8);
    uint4 v = make_uint4(al_pack2(r.a[u][0], r.a[u][1]), al_pack2(r.a[u][2], r.a[u][3]), al_pack2(r.c[u][0], r.c[u][1]),
                         al_pack2(r.c[u][2], r.c[u][3]));
    if (j0 + j >= T) v = make_uint4(0u, 0u, 0u, 0u);
    *(uint4*)(img + j * AlGeom<D>::KP + 8 * c8) = v;
  }
}
// ---- transposed image [channel][key] of a chunk: thread = (key pair, 4 channels), 8 key pairs x 8 channel quads per wave
// instruction (attention_fused.hip's V^T staging)
template <int D>
__device__ __forceinline__ void al_load_tr(AlStage<D>& r, const float* X, size_t ld, int j0, int T, int tid) {
  constexpr int nCq = D / 32;
#pragma unroll
  for (int u = 0; u < AlGeom<D>::NI; ++u) {
    const int idx = u * 256 + tid;
    const int blk = idx >> 6, l6 = idx & 63;
    const int jg = blk / nCq, cg = blk - jg * nCq;
    const int j = j0 + 2 * (jg * 8 + (l6 & 7)), c4 = cg * 8 + (l6 >> 3);
    r.a[u] = *(const al_f32x4*)(X + (size_t)(j < T ? j : T - 1) * ld + 4 * c4);
    r.c[u] = *(const al_f32x4*)(X + (size_t)(j + 1 < T ? j + 1 : T - 1) * ld + 4 * c4);
  }
}
template <int D>
__device__ __forceinline__ void al_store_tr(const AlStage<D>& r, uint16_t* img, int j0, int T, int tid) {
  constexpr int nCq = D / 32;
#pragma unroll
  for (int u = 0; u < AlGeom<D>::NI; ++u) {
    const int idx = u * 256 + tid;
    const int blk = idx >> 6, l6 = idx & 63;
    const int jg = blk / nCq, cg = blk - jg * nCq;
    const int jl = 2 * (jg * 8 + (l6 & 7)), c4 = cg * 8 + (l6 >> 3);
    const int j = j0 + jl;
#pragma unroll
    for (int x = 0; x < 4; ++x)
      *(uint32_t*)(img + (4 * c4 + x) * AlGeom<D>::VP + jl) = al_pack2(j < T ? r.a[u][x] : 0.f, j + 1 < T ? r.c[u][x] : 0.f);
  }
}

// one 32 x 32 tile X_tile B^T: rows = the 32 image rows at `rows`, B fragments bf[KS]
template <int D>
__device__ __forceinline__ al_f32x16 al_tile(const uint16_t* rows, const al_bf16x8* bf, int li, int lh) {
  al_f32x16 acc = al_zero16();
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    const al_bf16x8 a = *(const al_bf16x8*)(rows + li * AlGeom<D>::KP + 16 * s + 8 * lh);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bf[s], acc, 0, 0, 0);
    if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // at most four k-steps of LDS reads in registers at a time
  }
  return acc;
}

// R^T block: rows = table-window rows w0 .. w0 + 32 (zero outside 0 .. W), columns = this wave's queries
template <int D>
__device__ __forceinline__ al_f32x16 al_pos_block(const float* E, int rlo, int W, int w0, const al_bf16x8* qf, int li, int lh) {
  al_f32x16 cur = al_zero16();
  const int w = w0 + li;
  const bool ok = w >= 0 && w < W;
  const float* src = E + (size_t)(rlo + (ok ? w : 0)) * D + 8 * lh;
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    al_f32x4 a = *(const al_f32x4*)(src + 16 * s), c = *(const al_f32x4*)(src + 16 * s + 4);
    if (!ok) { a = al_f32x4{0.f, 0.f, 0.f, 0.f}; c = a; }
    cur = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_pack8(a, c), qf[s], cur, 0, 0, 0);
    if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // at most four k-steps of table loads in registers at a time
  }
  return cur;
}
// acc[key jj][query li] += R[w = jj - li + 31] of the 64-row window (prev, cur), through the wave's scratch [32 queries][65]
__device__ __forceinline__ void al_skew_add(al_f32x16& acc, const al_f32x16& prev, const al_f32x16& cur, float* rs, int li, int lh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int wr = (r & 3) + 8 * (r >> 2) + 4 * lh;
    rs[li * 65 + wr] = prev[r];
    rs[li * 65 + 32 + wr] = cur[r];
  }
  __builtin_amdgcn_wave_barrier();   // same wave wrote and reads: its LDS operations complete in order
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int jj = (r & 3) + 8 * (r >> 2) + 4 * lh;
    acc[r] += rs[li * 65 + jj - li + 31];
  }
  __builtin_amdgcn_wave_barrier();
}

// ntp: key tiles of 32, rounded up to an even number (8 .. 16); D: head width
template <int D>
__global__ __launch_bounds__(256, 1) void attn_long_fwd_k(AfP p, int ntp, int blocksPerWg) {
  typedef AlGeom<D> G;
  constexpr int KS = G::KS, TC = G::TC, CK = G::CK;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // two K row images, then two V^T images (buffer i of each)
  auto kimg = [&](int i) { return (uint16_t*)(smem + i * G::rowBytes); };
  auto vimg = [&](int i) { return (uint16_t*)(smem + 2 * G::rowBytes + i * G::trBytes); };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* rs = (float*)(smem + 2 * G::rowBytes + 2 * G::trBytes) + wave * (32 * 65);
  const int li = lane & 31, lh = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const int T = p.T;
  const size_t rowBase = (size_t)b * T;
  const int hc = h * D;
  const float* Kb = p.k + rowBase * p.ld + hc;
  const float* Vb = p.v + rowBase * p.ld + hc;
  const int nch = ntp / TC;

  const int qb = blockIdx.x * blocksPerWg + wave;        // query block; waves past the last block only help with the images
  const bool active = wave < blocksPerWg && 32 * qb < T;
  const int i0 = 32 * qb, iq = i0 + li;
  const int iqc = iq < T ? iq : T - 1;
  al_bf16x8 qf[KS];
  {
    const float* src = p.q + (rowBase + iqc) * p.ld + hc + 8 * lh;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = al_pack8(*(const al_f32x4*)(src + 16 * s), *(const al_f32x4*)(src + 16 * s + 4));
  }
  const int kl = p.keyLen ? max(0, min(p.keyLen[b], T)) : T;
  const int wb0 = -i0 - 31 + p.n0 - p.rlo;               // first window row of table block 0 (attention_fused.hip)
  const bool pos = p.E != nullptr;

  // ---- pass 1: row maximum and sum over the chunks that hold valid keys
  const int nch1 = (kl + CK - 1) / CK;
  AlStage<D> sk;
  if (nch1 > 0) {
    al_load_rows<D>(sk, Kb, p.ld, 0, T, tid);
    al_store_rows<D>(sk, kimg(0), 0, T, tid);
  }
  __syncthreads();
  float mx = -INFINITY, sum = 0.f;
  al_f32x16 prev = al_zero16();
  if (active && pos) prev = al_pos_block<D>(p.E, p.rlo, p.W, wb0, qf, li, lh);
  for (int c = 0; c < nch1; ++c) {
    if (c + 1 < nch1) al_load_rows<D>(sk, Kb, p.ld, (c + 1) * CK, T, tid);
    if (active) {
#pragma unroll
      for (int tt = 0; tt < TC; ++tt) {
        const int t = c * TC + tt;
        if (32 * t >= kl) break;                         // (uniform over the workgroup)
        al_f32x16 acc = al_tile<D>(kimg(c & 1) + tt * 32 * G::KP, qf, li, lh);
        if (pos) {
          const al_f32x16 cur = al_pos_block<D>(p.E, p.rlo, p.W, wb0 + 32 * (t + 1), qf, li, lh);
          al_skew_add(acc, prev, cur, rs, li, lh);
          prev = cur;
        }
        float tm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const float v = j < kl ? acc[r] * p.scale : -INFINITY;
          acc[r] = v;
          tm = fmaxf(tm, v);
        }
        const float mn = fmaxf(mx, tm);
        if (mn > -INFINITY) {
          float ts = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) ts += expf(acc[r] - mn);   // (exp(-inf) = 0 for the masked keys)
          sum = sum * expf(mx - mn) + ts;
          mx = mn;
        }
      }
    }
    if (c + 1 < nch1) al_store_rows<D>(sk, kimg((c + 1) & 1), (c + 1) * CK, T, tid);
    __syncthreads();
  }
  // the two half-waves hold the two halves of a query's keys
  float inv = 0.f;
  {
    const float mo = __shfl_xor(mx, 32);
    const float m = fmaxf(mx, mo);
    const float mine = mx > -INFINITY ? sum * expf(mx - m) : 0.f;
    const float tot = mine + __shfl_xor(mine, 32);
    inv = tot > 0.f ? 1.f / tot : 0.f;                   // an utterance with no valid key: zeros (as the unfused kernel)
    mx = m;
  }

  // ---- pass 2: P, Pd and ctx^T = V^T Pd^T
  AlStage<D> sv;
  al_load_rows<D>(sk, Kb, p.ld, 0, T, tid);
  al_load_tr<D>(sv, Vb, p.ld, 0, T, tid);
  al_store_rows<D>(sk, kimg(0), 0, T, tid);
  al_store_tr<D>(sv, vimg(0), 0, T, tid);
  __syncthreads();
  al_f32x16 o[D / 32];
#pragma unroll
  for (int ct = 0; ct < D / 32; ++ct) o[ct] = al_zero16();
  if (active && pos) prev = al_pos_block<D>(p.E, p.rlo, p.W, wb0, qf, li, lh);
  const size_t prow = (((size_t)b * p.H + h) * T + iqc) * T;
  const bool vec = (T & 3) == 0;
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) {
      al_load_rows<D>(sk, Kb, p.ld, (c + 1) * CK, T, tid);
      al_load_tr<D>(sv, Vb, p.ld, (c + 1) * CK, T, tid);
    }
    if (active) {
#pragma unroll 1
      for (int tt = 0; tt < TC; ++tt) {
        const int t = c * TC + tt;
        al_f32x16 acc;
        {
          acc = al_tile<D>(kimg(c & 1) + tt * 32 * G::KP, qf, li, lh);
          __builtin_amdgcn_sched_barrier(0);             // keep the table loads of the next product out of this one's registers
          if (pos) {
            const al_f32x16 cur = al_pos_block<D>(p.E, p.rlo, p.W, wb0 + 32 * (t + 1), qf, li, lh);
            __builtin_amdgcn_sched_barrier(0);
            al_skew_add(acc, prev, cur, rs, li, lh);
            prev = cur;
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int j = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
            acc[r] = j < kl ? expf(acc[r] * p.scale - mx) : 0.f;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int j = 32 * t + 8 * g + 4 * lh;
          al_f32x4 pv, dv;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float pr = acc[4 * g + x] * inv;
            pv[x] = pr;
            float dr = pr;
            if (p.thr) dr = keep_elem(prow + j + x, p.seed, p.stream, p.thr) ? pr * p.keepScale : 0.f;
            dv[x] = dr;
            acc[4 * g + x] = dr;
          }
          if (iq < T && j < T) {
            if (vec) {
              *(al_f32x4*)(p.P + prow + j) = pv;
              if (p.thr) *(al_f32x4*)(p.Pd + prow + j) = dv;
            } else {
#pragma unroll
              for (int x = 0; x < 4; ++x)
                if (j + x < T) {
                  p.P[prow + j + x] = pv[x];
                  if (p.thr) p.Pd[prow + j + x] = dv[x];
                }
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        {
          const al_bf16x8 pf0 = al_frag(acc, 0), pf1 = al_frag(acc, 1);
#pragma unroll
          for (int ct = 0; ct < D / 32; ++ct) {
            const uint16_t* vrow = vimg(c & 1) + (32 * ct + li) * G::VP + 32 * tt + 4 * lh;
            o[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_read44(vrow), pf0, o[ct], 0, 0, 0);
            o[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_read44(vrow + 16), pf1, o[ct], 0, 0, 0);
            if (ct & 1) __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
    if (c + 1 < nch) {
      al_store_rows<D>(sk, kimg((c + 1) & 1), (c + 1) * CK, T, tid);
      al_store_tr<D>(sv, vimg((c + 1) & 1), (c + 1) * CK, T, tid);
    }
    __syncthreads();
  }
  if (active && iq < T) {
#pragma unroll
    for (int ct = 0; ct < D / 32; ++ct) {
      const al_f32x16& oc = o[ct];
      if (p.ctx) {
        float* dst = p.ctx + (rowBase + iq) * p.ldc + hc + 32 * ct + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) *(al_f32x4*)(dst + 8 * g) = al_f32x4{oc[4 * g], oc[4 * g + 1], oc[4 * g + 2], oc[4 * g + 3]};
      }
      if (p.ctxI.rowMajor) {
        uint16_t* dst = p.ctxI.rowMajor + (rowBase + iq) * p.ctxI.ldRows + hc + 32 * ct + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) *(uint2*)(dst + 8 * g) = make_uint2(al_pack2(oc[4 * g], oc[4 * g + 1]), al_pack2(oc[4 * g + 2], oc[4 * g + 3]));
      }
      if (p.ctxI.transposed) {
        uint16_t* dst = p.ctxI.transposed + (size_t)(hc + 32 * ct + 4 * lh) * p.ctxI.ldTrans + rowBase + iq;
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(size_t)((r & 3) + 8 * (r >> 2)) * p.ctxI.ldTrans] = al_bf16(oc[r]);
      }
      __builtin_amdgcn_sched_barrier(0);   // one tile's store addresses at a time
    }
  }
}

// ===================================================================== backward

// One 32 x 32 output tile in the MFMA C layout as fp32 and / or bf16 images (attention_fused_bwd.hip::ab_store_tile)
__device__ __forceinline__ void al_store_tile(const al_f32x16& o, bool ok, size_t row, int col0, int lh, float* f, size_t ldf,
                                              const w2l_bf16_image_sink& im) {
  if (!ok) return;
  if (f) {
    float* dst = f + row * ldf + col0 + 4 * lh;
#pragma unroll
    for (int g = 0; g < 4; ++g) *(al_f32x4*)(dst + 8 * g) = al_f32x4{o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
  }
  if (im.rowMajor) {
    uint16_t* dst = im.rowMajor + row * im.ldRows + col0 + 4 * lh;
#pragma unroll
    for (int g = 0; g < 4; ++g) *(uint2*)(dst + 8 * g) = make_uint2(al_pack2(o[4 * g], o[4 * g + 1]), al_pack2(o[4 * g + 2], o[4 * g + 3]));
  }
  if (im.transposed) {
    uint16_t* dst = im.transposed + (size_t)(col0 + 4 * lh) * im.ldTrans + row;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[(size_t)((r & 3) + 8 * (r >> 2)) * im.ldTrans] = al_bf16(o[r]);
  }
}

// window rows are numbered globally per (utterance, head) as in attention_fused_bwd.hip: query block qb's table block e is global
// block g = e - qb + ntp - 1, 2 ntp blocks of 32
__host__ __device__ __forceinline__ int al_w_origin(int ntp, int n0, int rlo) { return n0 - rlo - 31 - 32 * (ntp - 1); }

template <int D>
__global__ __launch_bounds__(256) void attn_long_prep_k(AbP p, int ntp) {
  const int GW = 64 * ntp;
  const int idx = blockIdx.x * 256 + threadIdx.x;   // (channel quad, window row)
  if (idx >= GW * (D / 4)) return;
  const int wg = idx % GW, c4 = idx / GW;
  const int w = wg + al_w_origin(ntp, p.n0, p.rlo);
  const bool ok = w >= 0 && w < p.W;
  const al_f32x4 e = *(const al_f32x4*)(p.E + (size_t)(p.rlo + (ok ? w : 0)) * D + 4 * c4);
#pragma unroll
  for (int x = 0; x < 4; ++x) p.Et[(size_t)(4 * c4 + x) * GW + wg] = ok ? al_bf16(e[x]) : (uint16_t)0;
}

// the P tile of this lane's query in the C layout (zero outside the matrix)
__device__ __forceinline__ al_f32x16 al_load_p(const float* P, size_t prow, int t, int lh, int T, bool rowIn, bool vec) {
  al_f32x16 pr;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int j = 32 * t + 8 * g + 4 * lh;
    const int jc = j < T ? j : 0;
    al_f32x4 pv;
    if (vec) {
      pv = *(const al_f32x4*)(P + prow + jc);
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x) pv[x] = P[prow + (jc + x < T ? jc + x : T - 1)];
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) pr[4 * g + x] = (rowIn && j + x < T) ? pv[x] : 0.f;
  }
  return pr;
}

template <int D>
__global__ __launch_bounds__(256, 1) void attn_long_bwd_q_k(AbP p, int ntp, int blocksPerWg) {
  typedef AlGeom<D> G;
  constexpr int KS = G::KS, TC = G::TC, CK = G::CK;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // two V row images, then two K^T images (buffer i of each)
  auto vimg = [&](int i) { return (uint16_t*)(smem + i * G::rowBytes); };
  auto kimg = [&](int i) { return (uint16_t*)(smem + 2 * G::rowBytes + i * G::trBytes); };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* rs = (float*)(smem + 2 * G::rowBytes + 2 * G::trBytes) + wave * (32 * 65);
  const int li = lane & 31, lh = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const int T = p.T;
  const size_t rowBase = (size_t)b * T;
  const int hc = h * D;
  const size_t bh = (size_t)b * p.H + h;
  const size_t TP = 32 * (size_t)ntp, GW = 64 * (size_t)ntp;
  const float* Kb = p.k + rowBase * p.ld + hc;
  const float* Vb = p.v + rowBase * p.ld + hc;
  const int nch = ntp / TC;
  const int nchT = (T + CK - 1) / CK;                    // chunks that hold frames

  const int qb = blockIdx.x * blocksPerWg + wave;
  const bool active = wave < blocksPerWg && 32 * qb < T;
  const int i0 = 32 * qb, iq = i0 + li;
  const int iqc = iq < T ? iq : T - 1;
  al_bf16x8 df[KS];
  {
    const float* src = p.dctx + (rowBase + iqc) * p.ldc + hc + 8 * lh;
#pragma unroll
    for (int s = 0; s < KS; ++s) df[s] = al_pack8(*(const al_f32x4*)(src + 16 * s), *(const al_f32x4*)(src + 16 * s + 4));
  }
  const size_t prow = ((bh * T) + iqc) * T;
  const bool vec = (T & 3) == 0;

  // ---- pass A: dot_i = sum_j P[i][j] dPm[i][j]
  AlStage<D> sv;
  al_load_rows<D>(sv, Vb, p.ld, 0, T, tid);
  al_store_rows<D>(sv, vimg(0), 0, T, tid);
  __syncthreads();
  float dot = 0.f;
  for (int c = 0; c < nchT; ++c) {
    if (c + 1 < nchT) al_load_rows<D>(sv, Vb, p.ld, (c + 1) * CK, T, tid);
    if (active) {
#pragma unroll
      for (int tt = 0; tt < TC; ++tt) {
        const int t = c * TC + tt;
        const al_f32x16 pr = al_load_p(p.P, prow, t, lh, T, iq < T, vec);
        const al_f32x16 acc = al_tile<D>(vimg(c & 1) + tt * 32 * G::KP, df, li, lh);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
          float dp = acc[r];
          if (p.thr) dp = keep_elem(prow + j, p.seed, p.stream, p.thr) ? dp * p.keepScale : 0.f;
          dot += pr[r] * dp;
        }
      }
    }
    if (c + 1 < nchT) al_store_rows<D>(sv, vimg((c + 1) & 1), (c + 1) * CK, T, tid);
    __syncthreads();
  }
  dot += __shfl_xor(dot, 32);

  // ---- pass B: dS^T, the three images, dq^T = K^T dS^T + E^T dR^T
  AlStage<D> sk;
  al_load_rows<D>(sv, Vb, p.ld, 0, T, tid);
  al_load_tr<D>(sk, Kb, p.ld, 0, T, tid);
  al_store_rows<D>(sv, vimg(0), 0, T, tid);
  al_store_tr<D>(sk, kimg(0), 0, T, tid);
  __syncthreads();
  al_f32x16 o[D / 32];
#pragma unroll
  for (int ct = 0; ct < D / 32; ++ct) o[ct] = al_zero16();
  al_f32x16 prevUp = al_zero16();
  uint16_t* dStb = p.dSt + bh * TP * TP + i0 + li;
  uint16_t* Pdtb = p.Pdt + bh * TP * TP + i0 + li;
  uint16_t* dRtb = p.E ? p.dRt + bh * GW * TP + i0 + li : nullptr;
  const uint16_t* etb = p.E ? p.Et + 32 * (ntp - 1 - qb) + 4 * lh : nullptr;   // + c GW + 32 e + 16 u (+ 8)
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) {
      al_load_rows<D>(sv, Vb, p.ld, (c + 1) * CK, T, tid);
      al_load_tr<D>(sk, Kb, p.ld, (c + 1) * CK, T, tid);
    }
    if (active) {
#pragma unroll
      for (int tt = 0; tt < TC; ++tt) {
        const int t = c * TC + tt;
        const al_f32x16 pr = al_load_p(p.P, prow, t, lh, T, iq < T, vec);
        al_f32x16 acc = al_tile<D>(vimg(c & 1) + tt * 32 * G::KP, df, li, lh);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
          float pd = pr[r], dp = acc[r];
          if (p.thr) {
            const bool keep = keep_elem(prow + j, p.seed, p.stream, p.thr);
            pd = keep ? pd * p.keepScale : 0.f;
            dp = keep ? dp * p.keepScale : 0.f;
          }
          const float ds = p.scale * pr[r] * (dp - dot);
          acc[r] = ds;
          Pdtb[(size_t)j * TP] = al_bf16(pd);
          dStb[(size_t)j * TP] = al_bf16(ds);
        }
        const al_bf16x8 sf0 = al_frag(acc, 0), sf1 = al_frag(acc, 1);
        al_bf16x8 rf0 = sf0, rf1 = sf0;
        if (p.E) {
          // the skewed copy: tile t holds the window rows w' = jj - li + 31 of blocks e = t (w' < 32) and e = t + 1 (w' >= 32);
          // block t is complete now: from this tile where wr + li >= 31, from tile t - 1 (prevUp) below that
          al_f32x16 blk;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int jj = (r & 3) + 8 * (r >> 2) + 4 * lh;
            rs[li * 65 + jj - li + 31] = acc[r];
          }
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int wr = (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float lo = rs[li * 65 + wr];
            const float up = rs[li * 65 + 32 + wr];
            blk[r] = wr + li >= 31 ? lo : prevUp[r];
            prevUp[r] = up;
          }
          __builtin_amdgcn_wave_barrier();
          const int g = t - qb + ntp - 1;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int wr = (r & 3) + 8 * (r >> 2) + 4 * lh;
            dRtb[(size_t)(32 * g + wr) * TP] = al_bf16(blk[r]);
          }
          rf0 = al_frag(blk, 0);
          rf1 = al_frag(blk, 1);
        }
#pragma unroll
        for (int ct = 0; ct < D / 32; ++ct) {
          const uint16_t* krow = kimg(c & 1) + (32 * ct + li) * G::VP + 32 * tt + 4 * lh;
          o[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_read44(krow), sf0, o[ct], 0, 0, 0);
          o[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_read44(krow + 16), sf1, o[ct], 0, 0, 0);
          if (p.E) {
            const uint16_t* erow = etb + (size_t)(32 * ct + li) * GW + 32 * t;
            o[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_read44(erow), rf0, o[ct], 0, 0, 0);
            o[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_read44(erow + 16), rf1, o[ct], 0, 0, 0);
          }
        }
      }
    }
    if (c + 1 < nch) {
      al_store_rows<D>(sv, vimg((c + 1) & 1), (c + 1) * CK, T, tid);
      al_store_tr<D>(sk, kimg((c + 1) & 1), (c + 1) * CK, T, tid);
    }
    __syncthreads();
  }
  if (active) {
    if (p.E) {
      // the last block, e = ntp: only the upper half of the last tile's window
      al_f32x16 blk;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int wr = (r & 3) + 8 * (r >> 2) + 4 * lh;
        blk[r] = wr + li >= 31 ? 0.f : prevUp[r];
      }
      const int g = 2 * ntp - 1 - qb;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int wr = (r & 3) + 8 * (r >> 2) + 4 * lh;
        dRtb[(size_t)(32 * g + wr) * TP] = al_bf16(blk[r]);
      }
      const al_bf16x8 rf0 = al_frag(blk, 0), rf1 = al_frag(blk, 1);
#pragma unroll
      for (int ct = 0; ct < D / 32; ++ct) {
        const uint16_t* erow = etb + (size_t)(32 * ct + li) * GW + 32 * ntp;
        o[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_read44(erow), rf0, o[ct], 0, 0, 0);
        o[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_read44(erow + 16), rf1, o[ct], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ct = 0; ct < D / 32; ++ct) al_store_tile(o[ct], iq < T, rowBase + iqc, hc + 32 * ct, lh, p.dq, (size_t)p.ld, p.dqI);
  }
}

// The key side.  blockIdx.x selects (role, group of 8 row blocks): role 0 dk = dS^T q, 1 dv = Pd^T dctx, 2 dE partial = dR^T q.
// Wave w owns image rows 32 (8 grp + w) .. + 32; the transposed q / dctx image streams in chunks of 64 queries.
template <int D>
__global__ __launch_bounds__(512) void attn_long_bwd_kv_k(AbP p, int ntp) {
  constexpr int QC = 64, XP = QC + 8;    // bf16 pitch of the transposed chunk: 16 bytes x odd -> conflict-free ds_read_b128
  constexpr int nItems = (QC / 2) * (D / 4);
  constexpr int NI = (nItems + 511) / 512;
  constexpr int nCq = D / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  auto ximg = [&](int i) { return (uint16_t*)smem + i * (D * XP); };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z;
  const int T = p.T;
  const size_t rowBase = (size_t)b * T;
  const int hc = h * D;
  const size_t bh = (size_t)b * p.H + h;
  const size_t TP = 32 * (size_t)ntp, GW = 64 * (size_t)ntp;
  const int nG = (ntp + 7) / 8;
  const int role = (int)blockIdx.x < nG ? 0 : (int)blockIdx.x < 2 * nG ? 1 : 2;
  const int g = 8 * ((int)blockIdx.x - role * nG) + wave;          // this wave's row block
  const bool rowsOk = g < (role < 2 ? ntp : 2 * ntp);
  const float* X = (role == 1 ? p.dctx + rowBase * p.ldc : p.q + rowBase * p.ld) + hc;
  const size_t ldx = role == 1 ? p.ldc : p.ld;
  const uint16_t* rowp = role == 0   ? p.dSt + bh * TP * TP
                         : role == 1 ? p.Pdt + bh * TP * TP
                                     : p.dRt + bh * GW * TP;
  rowp += (size_t)(32 * (rowsOk ? g : 0) + li) * TP + 8 * lh;

  al_f32x4 sa[NI], sc[NI];
  auto load = [&](int i0) {
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      int idx = u * 512 + tid;
      if (idx >= nItems) idx = 0;
      const int blk = idx >> 6, l6 = idx & 63;
      const int jg = blk / nCq, cg = blk - jg * nCq;
      const int i = i0 + 2 * (jg * 8 + (l6 & 7)), c4 = cg * 8 + (l6 >> 3);
      sa[u] = *(const al_f32x4*)(X + (size_t)(i < T ? i : T - 1) * ldx + 4 * c4);
      sc[u] = *(const al_f32x4*)(X + (size_t)(i + 1 < T ? i + 1 : T - 1) * ldx + 4 * c4);
    }
  };
  auto store = [&](uint16_t* img, int i0) {
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int idx = u * 512 + tid;
      const int blk = idx >> 6, l6 = idx & 63;
      const int jg = blk / nCq, cg = blk - jg * nCq;
      const int il = 2 * (jg * 8 + (l6 & 7)), c4 = cg * 8 + (l6 >> 3);
      const int i = i0 + il;
      if (idx < nItems) {
#pragma unroll
        for (int x = 0; x < 4; ++x) *(uint32_t*)(img + (4 * c4 + x) * XP + il) = al_pack2(i < T ? sa[u][x] : 0.f, i + 1 < T ? sc[u][x] : 0.f);
      }
    }
  };

  const int nq = ntp / 2;                // query chunks
  load(0);
  store(ximg(0), 0);
  __syncthreads();
  al_f32x16 o[D / 32];
#pragma unroll
  for (int ct = 0; ct < D / 32; ++ct) o[ct] = al_zero16();
  for (int c = 0; c < nq; ++c) {
    if (c + 1 < nq) load(QC * (c + 1));
    if (rowsOk) {
      // B fragments: 8 consecutive queries of this lane's row per k-step, straight from the global image; zero where the query
      // side wrote nothing (query blocks past T; for dR^T the blocks outside 0 <= e <= ntp)
      al_bf16x8 bf[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int qblk = 2 * c + (s >> 1);
        const int e = g + qblk - (ntp - 1);
        const bool valid = 32 * qblk < T && (role < 2 || (e >= 0 && e <= ntp));
        uint4 ld = *(const uint4*)(rowp + QC * c + 16 * s);   // unconditional (inside the workspace either way)
        if (!valid) ld = make_uint4(0u, 0u, 0u, 0u);
        bf[s] = __builtin_bit_cast(al_bf16x8, ld);
      }
#pragma unroll
      for (int ct = 0; ct < D / 32; ++ct) {
        const uint16_t* xrow = ximg(c & 1) + (32 * ct + li) * XP + 8 * lh;
#pragma unroll
        for (int s = 0; s < 4; ++s) o[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const al_bf16x8*)(xrow + 16 * s), bf[s], o[ct], 0, 0, 0);
      }
    }
    if (c + 1 < nq) store(ximg((c + 1) & 1), QC * (c + 1));
    __syncthreads();
  }
  if (!rowsOk) return;
  const int row = 32 * g + li;
  const w2l_bf16_image_sink none{nullptr, 0, nullptr, 0};
#pragma unroll
  for (int ct = 0; ct < D / 32; ++ct) {
    if (role == 0) al_store_tile(o[ct], row < T, rowBase + (row < T ? row : 0), hc + 32 * ct, lh, p.dk, (size_t)p.ld, p.dkI);
    else if (role == 1) al_store_tile(o[ct], row < T, rowBase + (row < T ? row : 0), hc + 32 * ct, lh, p.dv, (size_t)p.ld, p.dvI);
    else al_store_tile(o[ct], true, bh * GW + row, 32 * ct, lh, p.dEp, (size_t)D, none);
  }
}

// dE[row][c] = sum over (b, h) of the partials in a fixed order; rows outside the window zero
template <int D>
__global__ __launch_bounds__(256) void attn_long_de_reduce_k(AbP p, int ntp) {
  const int GW = 64 * ntp;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int rows = 2 * p.n0 + 1;
  if (idx >= rows * (D / 4)) return;
  const int row = idx / (D / 4), c4 = idx - row * (D / 4);
  const int w = row - p.rlo;
  al_f32x4 s = {0.f, 0.f, 0.f, 0.f};
  const int wg = w - al_w_origin(ntp, p.n0, p.rlo);
  if (w >= 0 && w < p.W && wg >= 0 && wg < GW) {
    const float* src = p.dEp + (size_t)wg * D + 4 * c4;
    const int n = p.B * p.H;
    int i = 0;
    for (; i + 8 <= n; i += 8) {   // eight loads in flight; the order of the additions is fixed
      al_f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *(const al_f32x4*)(src + (size_t)(i + u) * GW * D);
#pragma unroll
      for (int u = 0; u < 8; ++u) { s[0] += v[u][0]; s[1] += v[u][1]; s[2] += v[u][2]; s[3] += v[u][3]; }
    }
    for (; i < n; ++i) {
      const al_f32x4 v = *(const al_f32x4*)(src + (size_t)i * GW * D);
      s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
  }
  *(al_f32x4*)(p.dE + (size_t)row * D + 4 * c4) = s;
}

// ===================================================================== host side

static int al_tiles(int T) { return 2 * ((T + 63) / 64); }   // key / query tiles of 32, rounded up to an even number

// query blocks per workgroup: as few as keeps the grid within one wave of workgroups, at most 4 (the short family's rule)
static int al_blocks_per_wg(int blocks, int H, int B) {
  int bpw = 4;
  while (bpw > 1 && (long long)((blocks + bpw - 2) / (bpw - 1)) * H * B <= 256) --bpw;
  return bpw;
}

bool attn_long_supported(int T, int d) { return T > 192 && T <= 512 && (d == 32 || d == 192 || d == 256); }

template <int D>
static int al_forward(const AfP& p, hipStream_t s) {
  typedef AlGeom<D> G;
  static const bool attr =
      hipFuncSetAttribute((const void*)attn_long_fwd_k<D>, hipFuncAttributeMaxDynamicSharedMemorySize, G::shmem) == hipSuccess;
  if (!attr) return W2L_EHIP;
  const int blocks = (p.T + 31) / 32;
  const int bpw = al_blocks_per_wg(blocks, p.H, p.B);
  hipLaunchKernelGGL((attn_long_fwd_k<D>), dim3((unsigned)((blocks + bpw - 1) / bpw), (unsigned)p.H, (unsigned)p.B), dim3(256), G::shmem, s,
                     p, al_tiles(p.T), bpw);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

int attn_long_forward(const AfP& p, int d, hipStream_t s) {
  if (!attn_long_supported(p.T, d)) return W2L_EUNSUPPORTED;
  return d == 32 ? al_forward<32>(p, s) : d == 192 ? al_forward<192>(p, s) : al_forward<256>(p, s);
}

struct AlWs {
  size_t img, dRt, et, dEp;
  AlWs(size_t BH, int ntp, int d) {
    const size_t TP = 32 * (size_t)ntp, GW = 64 * (size_t)ntp;
    img = align_up(BH * TP * TP * 2, 256);
    dRt = align_up(BH * GW * TP * 2, 256);
    et = align_up((size_t)d * GW * 2, 256);
    dEp = align_up(BH * GW * d * 4, 256);
  }
  size_t total(bool table) const { return 2 * img + (table ? dRt + et + dEp : 0); }
};

size_t attn_long_backward_workspace(int B, int H, int T, int d, bool table) {
  if (B <= 0 || H <= 0 || !attn_long_supported(T, d)) return 0;
  return AlWs((size_t)B * H, al_tiles(T), d).total(table);
}

template <int D>
static int al_backward(AbP p, void* ws, size_t wsBytes, hipStream_t s) {
  typedef AlGeom<D> G;
  const int ntp = al_tiles(p.T);
  const size_t BH = (size_t)p.B * p.H;
  const bool table = p.E != nullptr;
  const AlWs g(BH, ntp, D);
  if (wsBytes < g.total(table)) return W2L_EINVAL;
  unsigned char* w = (unsigned char*)ws;
  p.dSt = (uint16_t*)w; w += g.img;
  p.Pdt = (uint16_t*)w; w += g.img;
  if (table) {
    p.dRt = (uint16_t*)w; w += g.dRt;
    p.Et = (uint16_t*)w; w += g.et;
    p.dEp = (float*)w;
  } else {
    p.dRt = p.Et = nullptr; p.dEp = nullptr;
  }
  constexpr int shmemK = 2 * D * 72 * 2;
  static const bool attr =
      hipFuncSetAttribute((const void*)attn_long_bwd_q_k<D>, hipFuncAttributeMaxDynamicSharedMemorySize, G::shmem) == hipSuccess &&
      hipFuncSetAttribute((const void*)attn_long_bwd_kv_k<D>, hipFuncAttributeMaxDynamicSharedMemorySize, shmemK) == hipSuccess;
  if (!attr) return W2L_EHIP;
  const int blocks = (p.T + 31) / 32;
  const int bpw = al_blocks_per_wg(blocks, p.H, p.B);
  if (table) {
    hipLaunchKernelGGL((attn_long_prep_k<D>), dim3((unsigned)((64 * ntp * (D / 4) + 255) / 256)), dim3(256), 0, s, p, ntp);
    W2L_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((attn_long_bwd_q_k<D>), dim3((unsigned)((blocks + bpw - 1) / bpw), (unsigned)p.H, (unsigned)p.B), dim3(256), G::shmem, s, p,
                     ntp, bpw);
  W2L_LAUNCH_CHECK();
  const int nG = (ntp + 7) / 8, nGe = (2 * ntp + 7) / 8;
  hipLaunchKernelGGL((attn_long_bwd_kv_k<D>), dim3((unsigned)(2 * nG + (table ? nGe : 0)), (unsigned)p.H, (unsigned)p.B), dim3(512), shmemK, s, p,
                     ntp);
  W2L_LAUNCH_CHECK();
  if (table) {
    const int rows = 2 * p.n0 + 1;
    hipLaunchKernelGGL((attn_long_de_reduce_k<D>), dim3((unsigned)((rows * (D / 4) + 255) / 256)), dim3(256), 0, s, p, ntp);
    W2L_LAUNCH_CHECK();
  }
  return W2L_OK;
}

int attn_long_backward(AbP p, int d, void* ws, size_t wsBytes, hipStream_t s) {
  if (!attn_long_supported(p.T, d)) return W2L_EUNSUPPORTED;
  return d == 32 ? al_backward<32>(p, ws, wsBytes, s) : d == 192 ? al_backward<192>(p, ws, wsBytes, s) : al_backward<256>(p, ws, wsBytes, s);
}

}  // namespace w2l
