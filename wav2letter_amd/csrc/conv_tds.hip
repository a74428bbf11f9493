// conv_tds.hip -- the TDS time convolution (fl::Conv2D kw x 1 over (T, H) with few channels:
// C = 10 / 14 / 18, kw = 21, H = 80 mel rows) forward / backward-data / backward-filter.
//
// Reference: fl::TDSBlock's conv (recipes/joint_training_vox_populi/cpc/SequentialBuilder.cpp
// :254-268; arithmetic recipes/streaming_convnets/inference/inference/module/nn/backend/fbgemm/
// Conv1dFbGemm.cpp:104-185) and the C2 sub-sampling convolutions of am_tds_ctc.arch:3-6; cuDNN
// forward / backward-data / backward-filter in the reference.
//
// The generic implicit-GEMM operand of conv.hip gathers one scalar per (row, k) with two
// divisions: at N = C_out = 10 the GEMM is so skinny that this address arithmetic, not the
// matrix pipe, was the bound (16 TF/s, 0.3 TB/s).  Here the convolution is IM2COL-FREE in
// LDS: a workgroup stages the input slab it needs ONCE
//     slab[frame f][h][ci],  f in [t0*stride - padl, ... + (BT-1)*stride + kw)
// (rows of 16*C_in contiguous floats, coalesced float4 loads, halo (BT+kw-1)/BT), and the
// v_mfma_f32_16x16x4_f32 A fragments are read straight out of it:
//     A[(t,h)][(tap,ci)] = slab[(t*stride + tap)*FS + h*C_in + ci]
// = one ds_read_b32 at  rowoff(t,h) + koff(tap,ci)  with koff from a 1 KB LDS table.  The
// 16 rows of an MFMA tile are 16 consecutive mel rows h (stride C_in = 10/14/18 floats:
// conflict-free banks), a wave owns 8 output frames x 16 h.  Output tiles are staged through
// LDS and written as whole contiguous frames.  backward-data (stride 1) is the same kernel
// with tap-flipped, transposed weights; backward-filter keeps the (tap,ci) x co accumulators
// of a PERSISTENT workgroup in registers over many (b, t, h) chunks, gets the bias gradient
// from an extra all-ones row, and ends with a deterministic partial-sum reduction.
//
// MFMA roofline note: N = C_out is padded to 16 (32 for C = 18), so the matrix-pipe ceiling
// of this op is C/16 = 62.5 % / 87.5 % / 56 % of the fp32 peak by construction.
#include <cstdlib>

#include "conv_tds.hpp"

namespace w2l {

constexpr int kTdsBT = 32;   // output frames per workgroup (forward / backward-data)
constexpr int kTdsBTF = 16;  // frames per chunk (backward-filter)
constexpr int kTdsBH = 16;   // mel rows per workgroup = rows of one MFMA tile
constexpr int kTdsMaxXV = 12;  // float4 slab pieces per thread (register-prefetching kernels)
constexpr int kTdsMaxTilesPerWave = 6;  // backward-filter: (K+1)/16 row tiles over 4 waves -> K <= 383

__device__ __forceinline__ void tds_load_slab(const TdsConvP& p, float* slab, int b, int tIn0, int h0, int nf) {
  const int rowLen = kTdsBH * p.Cin;            // floats per slab frame (without pad)
  int hc = p.H - h0;
  if (hc > kTdsBH) hc = kTdsBH;
  const int valid = hc * p.Cin;
  const bool vec = ((p.H * p.Cin) & 3) == 0 && (valid & 3) == 0 && ((h0 * p.Cin) & 3) == 0;
  if (vec) {
    const int q = rowLen >> 2, total = nf * (q + 1);  // + 1: the 4-float pad of each frame is zero-filled
    for (int e = threadIdx.x; e < total; e += 256) {
      const int f = e / (q + 1), o = (e - f * (q + 1)) << 2;
      const int ti = tIn0 + f;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ti >= 0 && ti < p.Tin && o < valid) v = *(const float4*)(p.x + (((size_t)b * p.Tin + ti) * p.H + h0) * p.Cin + o);
      *(float4*)(slab + f * p.FS + o) = v;
    }
  } else {
    const int total = nf * p.FS;
    for (int e = threadIdx.x; e < total; e += 256) {
      const int f = e / p.FS, o = e - f * p.FS;
      const int ti = tIn0 + f;
      float v = 0.f;
      if (ti >= 0 && ti < p.Tin && o < valid) v = p.x[(((size_t)b * p.Tin + ti) * p.H + h0) * p.Cin + o];
      slab[e] = v;
    }
  }
}


// Batched staging: every thread issues up to NV independent loads back to back, THEN stores them -- one
// exposed memory latency per batch instead of one per element (the element-at-a-time loops above wait
// for each load before the next trip: ~9-18 serialized L2/HBM round trips per workgroup).
template <int NV, class LoadF, class StoreF>
__device__ __forceinline__ void tds_batched_copy4(int total, LoadF ld, StoreF st) {
  for (int base = 0; base < total; base += NV * 256) {
    float4 v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int e = base + threadIdx.x + 256 * j;
      v[j] = ld(e < total ? e : total - 1);
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int e = base + threadIdx.x + 256 * j;
      if (e < total) st(e, v[j]);
    }
  }
}
template <int NV, class LoadF, class StoreF>
__device__ __forceinline__ void tds_batched_copy1(int total, LoadF ld, StoreF st) {
  for (int base = 0; base < total; base += NV * 256) {
    float v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int e = base + threadIdx.x + 256 * j;
      v[j] = ld(e < total ? e : total - 1);
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int e = base + threadIdx.x + 256 * j;
      if (e < total) st(e, v[j]);
    }
  }
}

// slab load, float4 pieces in batches (whole 16-row mel block, 16-byte aligned rows: checked by the caller)
__device__ __forceinline__ void tds_load_slab_batched(const TdsConvP& p, float* slab, int b, int tIn0, int h0, int nf) {
  const int q = (kTdsBH * p.Cin) >> 2;  // float4 per frame; + 1 = the zero pad of the frame
  const float* xb = p.x + ((size_t)b * p.Tin * p.H + h0) * p.Cin;
  const int HCi = p.H * p.Cin;
  tds_batched_copy4<8>(nf * (q + 1),
      [&](int e) {
        const int f = e / (q + 1), o = e - f * (q + 1);
        const int ti = tIn0 + f;
        const bool ok = ti >= 0 && ti < p.Tin && o < q;
        const float4 t4 = *(const float4*)(xb + (size_t)(ok ? ti : 0) * HCi + (ok ? (o << 2) : 0));
        return ok ? t4 : make_float4(0.f, 0.f, 0.f, 0.f);
      },
      [&](int e, float4 v) {
        const int f = e / (q + 1), o = e - f * (q + 1);
        *(float4*)(slab + f * p.FS + (o << 2)) = v;
      });
}

// ---------------------------------------------------------------- forward / backward-data
// grid (ceil(H/16), ceil(Tout/32), B), 256 threads.  LDS: slab | weights [Kp][Cout] | koff[Kp]
template <int NT>
__global__ __launch_bounds__(256) void tds_conv_fwd_k(TdsConvP p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int slabFloats = max(p.NF * p.FS, kTdsBT * kTdsBH * p.Cout);
  float* slab = lds;
  float* wS = slab + ((slabFloats + 3) & ~3);
  int* koff = (int*)(wS + ((p.Kp * p.Cout + 3) & ~3));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = blockIdx.x * kTdsBH, t0 = blockIdx.y * kTdsBT, b = blockIdx.z;

  // weights: forward W[(tap,ci)][co]; backward-data W'[(tap',co_w)][ci_w] = W[kw-1-tap'][ci_w][co_w]
  const int wTot = p.Kp * p.Cout, wValid = p.K * p.Cout;
  if (!p.flip && (wValid & 3) == 0 && ((((uintptr_t)p.w) & 15) == 0)) {
    tds_batched_copy4<8>((wTot + 3) >> 2,
        [&](int e) {
          const bool ok = 4 * e < wValid;
          const float4 t4 = *(const float4*)(p.w + (ok ? 4 * e : 0));
          return ok ? t4 : make_float4(0.f, 0.f, 0.f, 0.f);
        },
        [&](int e, float4 v) { *(float4*)(wS + 4 * e) = v; });
  } else {
    tds_batched_copy1<8>(wTot,
        [&](int e) {
          const int kk = e / p.Cout, co = e - kk * p.Cout;
          const bool ok = kk < p.K;
          size_t src = 0;
          if (ok) {
            if (!p.flip) {
              src = (size_t)e;
            } else {
              const int tap = kk / p.Cin, c = kk - tap * p.Cin;  // c indexes CoutW, co indexes CinW
              src = ((size_t)(p.kw - 1 - tap) * p.CinW + co) * p.CoutW + c;
            }
          }
          const float t = p.w[src];
          return ok ? t : 0.f;
        },
        [&](int e, float v) { wS[e] = v; });
  }
  for (int kk = tid; kk < p.Kp; kk += 256) {
    const int tap = kk / p.Cin, c = kk - tap * p.Cin;
    koff[kk] = kk < p.K ? tap * p.FS + c : 0;
  }
  {
    int hc = p.H - h0;
    if (hc > kTdsBH) hc = kTdsBH;
    const bool vec = hc == kTdsBH && ((p.H * p.Cin) & 3) == 0 && ((kTdsBH * p.Cin) & 3) == 0 && ((((uintptr_t)p.x) & 15) == 0);
    if (vec) tds_load_slab_batched(p, slab, b, t0 * p.stride - p.padl, h0, p.NF);
    else tds_load_slab(p, slab, b, t0 * p.stride - p.padl, h0, p.NF);
  }
  __syncthreads();

  const int i = lane & 15, lq = lane >> 4;
  f32x4 acc[8][NT];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[r][nt][q] = 0.f;

  const float* sl = slab + i * p.Cin + (wave * 8 * p.stride) * p.FS;
  const int rstep = p.stride * p.FS;
  const int nk = p.Kp >> 2;
  for (int kq = 0; kq < nk; ++kq) {
    const int kk = 4 * kq + lq;
    const int ko = koff[kk];
    float bf[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bf[nt] = (16 * nt + i < p.Cout) ? wS[kk * p.Cout + 16 * nt + i] : 0.f;
    float a[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) a[r] = sl[r * rstep + ko];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], bf[nt], acc[r][nt], 0, 0, 0);
  }
  __syncthreads();  // all fragment reads done: the slab region becomes the output stage

  // D layout: col = lane & 15 (co within the N tile), row = 4 * (lane >> 4) + q (mel row)
  float* outS = slab;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co = 16 * nt + i;
    if (co < p.Cout) {
      const float bv = p.bias ? p.bias[co] : 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = acc[r][nt][q] + bv;
          if (p.relu) v = fmaxf(v, 0.f);
          outS[((wave * 8 + r) * kTdsBH + 4 * lq + q) * p.Cout + co] = v;
        }
    }
  }
  __syncthreads();
  int hc = p.H - h0;
  if (hc > kTdsBH) hc = kTdsBH;
  const int rowLen = hc * p.Cout;
  int tc = p.Tout - t0;
  if (tc > kTdsBT) tc = kTdsBT;
  const int total = tc * rowLen;
  const size_t gBase = (((size_t)b * p.Tout + t0) * p.H + h0) * p.Cout;
  const size_t gRow = (size_t)p.H * p.Cout;
  const bool vec = (rowLen & 3) == 0 && ((p.H * p.Cout) & 3) == 0 && ((kTdsBH * p.Cout) & 3) == 0 &&
                   ((((uintptr_t)p.y) | ((uintptr_t)p.add)) & 15) == 0;
  if (vec) {
    // whole contiguous frames as float4; the optional addend / accumulate reads are batched like the loads above
    const int rq = rowLen >> 2;
    tds_batched_copy4<8>(tc * rq,
        [&](int e) {
          const int t = e / rq, o = (e - t * rq) << 2;
          const size_t g = gBase + (size_t)t * gRow + o;
          float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
          if (p.add) a = *(const float4*)(p.add + g);
          if (p.accum) {
            const float4 y0 = *(const float4*)(p.y + g);
            a.x += y0.x; a.y += y0.y; a.z += y0.z; a.w += y0.w;
          }
          return a;
        },
        [&](int e, float4 a) {
          const int t = e / rq, o = (e - t * rq) << 2;
          const float4 v = *(const float4*)(outS + t * kTdsBH * p.Cout + o);
          *(float4*)(p.y + gBase + (size_t)t * gRow + o) = make_float4(v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
        });
  } else {
    for (int e = tid; e < total; e += 256) {
      const int t = e / rowLen, o = e - t * rowLen;
      const size_t g = gBase + (size_t)t * gRow + o;
      float v = outS[t * kTdsBH * p.Cout + o];
      if (p.add) v += p.add[g];
      if (p.accum) v += p.y[g];
      p.y[g] = v;
    }
  }
}


// ---------------------------------------------------------------- forward / backward-data, persistent
// tds_conv_fwd_k stages weights + slab, multiplies, writes -- strictly in sequence, once per workgroup,
// so every tile exposes its staging latency (the kernel ran at 2x its MFMA-bound time).  This version
// keeps a workgroup ALIVE over many (b, t-block, h-block) tiles: weights and the koff table are staged
// once, and the float4 pieces of tile i+1's slab are issued into registers (fixed per-thread piece
// descriptors) right before tile i is multiplied, then written to LDS after tile i's output has left it.
// R = output frames per wave (8: 32-frame tiles; 4: 16-frame tiles when the 32-frame slab would not
// leave room for two workgroups per CU).  Requires whole 16-row mel blocks and 16-byte aligned rows.
// CIN > 0: input channels known at compile time (stride 1): the slab frame stride is a constant, the R
// fragment reads of a K step share ONE address VGPR and differ in their immediate offsets.
template <int NT, int R, int CIN>
__global__ __launch_bounds__(256, 2) void tds_conv_fwd2_k(TdsConvP p, int nTiles, int tBlocks, int hBlocks) {
  constexpr int BT = 4 * R;
  const int CP = p.Cout;  // weight row stride; lanes past Cout re-read column Cout-1 (their MFMA columns are never stored)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int slabFloats = max(p.NF * p.FS, BT * kTdsBH * p.Cout);
  float* slab = lds;
  float* wS = slab + ((slabFloats + 3) & ~3);
  int* koff = (int*)(wS + ((p.Kp * CP + 3) & ~3));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ---- once per workgroup: weights, koff, pad zeroing, piece descriptors
  tds_batched_copy1<8>(p.Kp * CP,
      [&](int e) {
        const int kk = e / CP, co = e - kk * CP;
        const bool ok = kk < p.K;
        size_t src = 0;
        if (ok) {
          if (!p.flip) {
            src = (size_t)kk * p.Cout + co;
          } else {
            const int tap = kk / p.Cin, c = kk - tap * p.Cin;  // c indexes CoutW, co indexes CinW
            src = ((size_t)(p.tapOff + p.tapStep * (p.kw - 1 - tap)) * p.CinW + co) * p.CoutW + c;
          }
        }
        const float t = p.w[src];
        return ok ? t : 0.f;
      },
      [&](int e, float v) { wS[e] = v; });
  for (int kk = tid; kk < p.Kp; kk += 256) {
    const int tap = kk / p.Cin, c = kk - tap * p.Cin;
    koff[kk] = kk < p.K ? tap * p.FS + c : 0;
  }
  const int xq = (kTdsBH * p.Cin) >> 2;  // float4 per slab frame
  const int xTotal = p.NF * xq;
  const int HCi = p.H * p.Cin;
  int xf[kTdsMaxXV], xo[kTdsMaxXV];
#pragma unroll
  for (int v = 0; v < kTdsMaxXV; ++v) {
    const int e = tid + 256 * v;
    xf[v] = e < xTotal ? e / xq : -1;
    xo[v] = e < xTotal ? (e - xf[v] * xq) << 2 : 0;
  }
  float4 xr[kTdsMaxXV];
  auto fetch = [&](int tile) {
    const int hb = tile % hBlocks, tb = (tile / hBlocks) % tBlocks, b = tile / (hBlocks * tBlocks);
    const int tIn0 = tb * BT * p.stride - p.padl;
    const float* xb = p.x + ((size_t)b * p.Tin * p.H + hb * kTdsBH) * p.Cin;
#pragma unroll
    for (int v = 0; v < kTdsMaxXV; ++v) {
      const int ti = tIn0 + xf[v];
      const bool ok = xf[v] >= 0 && ti >= 0 && ti < p.Tin;
      const float4 t4 = *(const float4*)(xb + (size_t)(ok ? ti : 0) * HCi + xo[v]);
      xr[v] = ok ? t4 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };

  const int i = lane & 15, lq = lane >> 4;
  const int rstep = CIN ? 16 * CIN + 4 : p.stride * p.FS;
  const int nk = p.Kp >> 2;
  const float* sl = slab + i * p.Cin + (wave * R * p.stride) * p.FS;
  const size_t gRow = (size_t)p.oStep * p.H * p.Cout;
  const int rowLen = kTdsBH * p.Cout, rq = rowLen >> 2;

  float biasv[NT];  // once per workgroup: a load per tile would expose a global round trip in every tile's epilogue
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) biasv[nt] = (p.bias && 16 * nt + i < p.Cout) ? p.bias[16 * nt + i] : 0.f;

  int tile = blockIdx.x;
  if (tile < nTiles) fetch(tile);
  for (; tile < nTiles; tile += gridDim.x) {
    const int hb = tile % hBlocks, tb = (tile / hBlocks) % tBlocks, b = tile / (hBlocks * tBlocks);
    const int h0 = hb * kTdsBH, t0 = tb * BT;
    __syncthreads();  // the previous tile's output has been read out of the slab region
    if (!(p.abl & 2)) {
#pragma unroll
      for (int v = 0; v < kTdsMaxXV; ++v)
        if (xf[v] >= 0) *(float4*)(slab + xf[v] * p.FS + xo[v]) = xr[v];
    }
    __syncthreads();
    const int nxt = tile + gridDim.x;
    if (!(p.abl & 2)) fetch(nxt < nTiles ? nxt : tile);  // in flight behind this tile's MFMAs and output

    f32x4 acc[R][NT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[r][nt][q] = 0.f;
    // K loop, hand-scheduled: two fragment register sets in ping-pong and ONE LDS read slotted behind every
    // MFMA, so the reads of step kq+1 issue while the matrix pipe works on step kq.  (hipcc's own schedule --
    // all reads, wait, all MFMAs -- left the loop at 57 % of its MFMA-bound time even with staging and output
    // ablated: a wave issues in order, and a block of 11 ds_reads in front of 8 MFMAs is ~100 cycles in which
    // its MFMA queue is empty; profiles/r01_run13_conv_fwd_ablation.log.)
    int wcol[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wcol[nt] = 16 * nt + i < p.Cout ? 16 * nt + i : p.Cout - 1;
    const float* wl = wS + lq * CP;
    const int nkLoop = (p.abl & 1) ? 0 : nk;
    float aA[R], bA[NT], aB[R], bB[NT];
    int koN = koff[lq + (nk > 1 ? 4 : 0)];   // table entry of step 1
    {
      const int ko0 = koff[lq];
#pragma unroll
      for (int r = 0; r < R; ++r) aA[r] = sl[r * rstep + ko0];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bA[nt] = wl[wcol[nt]];
#pragma unroll
      for (int r = 0; r < R; ++r) aB[r] = aA[r];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bB[nt] = bA[nt];
    }
    // PMC (profiles/r01_run17_conv_fwd_sq_pmc.csv): 8.6 instructions per MFMA at 4 cycles of issue each against
    // a 32-cycle MFMA -- the loop was instruction-issue bound (MFMA pipe 46 % busy).  Diet: immediate-offset
    // fragment reads (CIN) and ONE lgkmcnt(0) per step instead of a counted wait in front of every MFMA (all of
    // a step's operands were read during the previous step).
    for (int kq = 0; kq < nkLoop; kq += 2) {
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only (vmcnt / expcnt fields at their maxima)
      // ---- step kq on set A; set B <- step kq+1 (clamped: a step past the end re-reads the last one and is not multiplied)
      const int k1 = kq + 1 < nk ? kq + 1 : nk - 1, k2 = kq + 2 < nk ? kq + 2 : nk - 1, k3 = kq + 3 < nk ? kq + 3 : nk - 1;
      const int koB = koN;
      int koA2 = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aA[r], bA[nt], acc[r][nt], 0, 0, 0);
        aB[r] = sl[r * rstep + koB];
        if (r == 0) koA2 = koff[4 * k2 + lq];
        if (r == 1) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) bB[nt] = wl[4 * k1 * CP + wcol[nt]];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (kq + 1 >= nk) break;
      __builtin_amdgcn_s_waitcnt(0xC07F);
      // ---- step kq+1 on set B; set A <- step kq+2
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aB[r], bB[nt], acc[r][nt], 0, 0, 0);
        aA[r] = sl[r * rstep + koA2];
        if (r == 0) koN = koff[4 * k3 + lq];
        if (r == 1) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) bA[nt] = wl[4 * k2 * CP + wcol[nt]];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();  // all fragment reads done: the slab region becomes the output stage

    float* outS = slab;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int co = 16 * nt + i;
      if (co < p.Cout) {
        const float bv = biasv[nt];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float v = acc[r][nt][q] + bv;
            if (p.relu) v = fmaxf(v, 0.f);
            outS[((wave * R + r) * kTdsBH + 4 * lq + q) * p.Cout + co] = v;
          }
      }
    }
    __syncthreads();
    int tc = p.Tout - t0;
    if (tc > BT) tc = BT;
    if (p.abl & 4) tc = 0;
    const size_t gBase = (((size_t)b * p.ToutFull + p.oOff + (size_t)p.oStep * t0) * p.H + h0) * p.Cout;
    tds_batched_copy4<8>(tc * rq,
        [&](int e) {
          const int t = e / rq, o = (e - t * rq) << 2;
          const size_t g = gBase + (size_t)t * gRow + o;
          float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
          if (p.add) a4 = *(const float4*)(p.add + g);
          if (p.accum) {
            const float4 y0 = *(const float4*)(p.y + g);
            a4.x += y0.x; a4.y += y0.y; a4.z += y0.z; a4.w += y0.w;
          }
          return a4;
        },
        [&](int e, float4 a4) {
          const int t = e / rq, o = (e - t * rq) << 2;
          const float4 v = *(const float4*)(outS + t * rowLen + o);
          *(float4*)(p.y + gBase + (size_t)t * gRow + o) = make_float4(v.x + a4.x, v.y + a4.y, v.z + a4.z, v.w + a4.w);
        });
  }
}

// ---------------------------------------------------------------- backward-filter (+ bias gradient)
// persistent grid; chunk = (b, 16 frames, 16 mel rows).  A = x^T: rows (tap,ci) [+ one all-ones row
// for the bias gradient], k = the chunk's 256 (t,h) positions; B = dy [(t,h)][co].
// partial[block][rowTile*16 + row][16*NT]
template <int NT>
__global__ __launch_bounds__(256) void tds_conv_filter_k(TdsConvP p, const float* __restrict__ dy, float* __restrict__ partial,
                                                        int nChunks, int tBlocks, int hBlocks, int rowTiles) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* slab = lds;
  float* dyS = slab + ((p.NF * p.FS + 3) & ~3);  // [256][Cout]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, lq = lane >> 4;

  int ko[kTdsMaxTilesPerWave];
  bool one[kTdsMaxTilesPerWave], val[kTdsMaxTilesPerWave];
#pragma unroll
  for (int tl = 0; tl < kTdsMaxTilesPerWave; ++tl) {
    const int kk = 16 * (wave + 4 * tl) + i;
    const int tap = kk / p.Cin, c = kk - tap * p.Cin;
    val[tl] = kk < p.K;
    one[tl] = kk == p.K;
    ko[tl] = val[tl] ? tap * p.FS + c : 0;
  }
  f32x4 acc[kTdsMaxTilesPerWave][NT];
#pragma unroll
  for (int tl = 0; tl < kTdsMaxTilesPerWave; ++tl)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[tl][nt][q] = 0.f;

  for (int chunk = blockIdx.x; chunk < nChunks; chunk += gridDim.x) {
    const int hb = chunk % hBlocks, tb = (chunk / hBlocks) % tBlocks, b = chunk / (hBlocks * tBlocks);
    const int h0 = hb * kTdsBH, t0 = tb * kTdsBTF;
    __syncthreads();  // previous chunk's fragment reads are done
    tds_load_slab(p, slab, b, t0 * p.stride - p.padl, h0, p.NF);
    int hc = p.H - h0;
    if (hc > kTdsBH) hc = kTdsBH;
    for (int e = tid; e < kTdsBTF * kTdsBH * p.Cout; e += 256) {
      const int m = e / p.Cout, co = e - m * p.Cout;
      const int t = m >> 4, h = m & 15;
      float v = 0.f;
      if (t0 + t < p.Tout && h < hc) v = dy[(((size_t)b * p.Tout + t0 + t) * p.H + h0 + h) * p.Cout + co];
      dyS[e] = v;
    }
    __syncthreads();
    for (int kq = 0; kq < kTdsBTF * kTdsBH / 4; ++kq) {
      const int m = 4 * kq + lq;
      const int rowoff = (m >> 4) * p.stride * p.FS + (m & 15) * p.Cin;
      float bf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bf[nt] = (16 * nt + i < p.Cout) ? dyS[m * p.Cout + 16 * nt + i] : 0.f;
#pragma unroll
      for (int tl = 0; tl < kTdsMaxTilesPerWave; ++tl) {
        if (wave + 4 * tl < rowTiles) {  // wave-uniform
          float a = slab[rowoff + ko[tl]];
          a = one[tl] ? 1.f : (val[tl] ? a : 0.f);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[tl][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bf[nt], acc[tl][nt], 0, 0, 0);
        }
      }
    }
  }
  float* dst = partial + (size_t)blockIdx.x * rowTiles * 16 * (16 * NT);
#pragma unroll
  for (int tl = 0; tl < kTdsMaxTilesPerWave; ++tl) {
    const int tile = wave + 4 * tl;
    if (tile < rowTiles) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[(size_t)(tile * 16 + 4 * lq + q) * (16 * NT) + 16 * nt + i] = acc[tl][nt][q];
    }
  }
}



// Lean K loop of the backward-filter kernel for the TDS convolutions proper (C -> C channels, stride 1, both
// compile-time): one chunk = 16 frames x 16 mel rows = 64 K steps of 4 positions.  The generic loop spent
// ~10 instructions per MFMA (runtime row offsets, a wave-uniform branch and two selects per row tile, a guard
// per column) against the 8 issue slots a 32-cycle MFMA allows; here every LDS read is `base VGPR + immediate`
// (frame stride and channel count are constants), invalid rows / columns are NOT masked (they only feed
// partial rows / columns the reduction never reads), the all-ones row of the bias gradient exists only in
// the last row tile of the wave that owns it, and the row-tile count per wave NTW is a template parameter.
template <int NT, int C, int NTW>
__device__ __forceinline__ void tds_filter_kloop(const float* __restrict__ slab, const float* __restrict__ dyS,
                                                 const int (&abase)[kTdsMaxTilesPerWave], const int (&dbase)[NT],
                                                 bool ownsOne, bool oneLane, f32x4 (&acc)[kTdsMaxTilesPerWave][NT]) {
  constexpr int FS = kTdsBH * C + 4;
  float aA[NTW], bA[NT], aB[NTW], bB[NT];
#pragma unroll
  for (int tl = 0; tl < NTW; ++tl) aA[tl] = slab[abase[tl]];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) bA[nt] = dyS[dbase[nt]];
  if (ownsOne) aA[NTW - 1] = oneLane ? 1.f : aA[NTW - 1];
#pragma unroll
  for (int kq = 0; kq < kTdsBTF * kTdsBH / 4; kq += 2) {
    // position m = 4 kq + lq: frame t = kq / 4, mel row 4 (kq % 4) + lq  (lq is inside abase / dbase)
    constexpr int dummy = 0;
    (void)dummy;
    const int k1 = kq + 1, k2 = kq + 2 < 64 ? kq + 2 : 63;
    const int aoff1 = (k1 >> 2) * FS + 4 * (k1 & 3) * C, doff1 = (16 * (k1 >> 2) + 4 * (k1 & 3)) * C;
    const int aoff2 = (k2 >> 2) * FS + 4 * (k2 & 3) * C, doff2 = (16 * (k2 >> 2) + 4 * (k2 & 3)) * C;
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): set A was read during the previous step
#pragma unroll
    for (int tl = 0; tl < NTW; ++tl) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[tl][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aA[tl], bA[nt], acc[tl][nt], 0, 0, 0);
      aB[tl] = slab[abase[tl] + aoff1];
      if (tl == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bB[nt] = dyS[dbase[nt] + doff1];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ownsOne) aB[NTW - 1] = oneLane ? 1.f : aB[NTW - 1];
    __builtin_amdgcn_s_waitcnt(0xC07F);
#pragma unroll
    for (int tl = 0; tl < NTW; ++tl) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[tl][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aB[tl], bB[nt], acc[tl][nt], 0, 0, 0);
      aA[tl] = slab[abase[tl] + aoff2];
      if (tl == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bA[nt] = dyS[dbase[nt] + doff2];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ownsOne) aA[NTW - 1] = oneLane ? 1.f : aA[NTW - 1];
  }
}

// ---------------------------------------------------------------- backward-filter, pipelined
// Same chunking / fragment scheme as tds_conv_filter_k, but the global -> LDS staging is built for
// latency: every thread owns a FIXED set of float4 pieces of a chunk (slab pieces + dy pieces,
// descriptors in registers), issues all of them for chunk c+1 back to back BEFORE multiplying chunk
// c, and writes them to LDS afterwards.  The first version loaded one element per loop trip with the
// s_waitcnt right behind it: ~16 serialized HBM round trips per chunk (43 us per chunk measured,
// against 3 us of MFMA work).  Requires whole 16-row mel blocks (H % 16 == 0), 16-byte aligned rows.
constexpr int kTdsMaxDV = 5;   // float4 dy pieces per thread

template <int NT, int C>
__global__ __launch_bounds__(256, 2) void tds_conv_filter2_k(TdsConvP p, const float* __restrict__ dy, float* __restrict__ partial,
                                                            int nChunks, int tBlocks, int hBlocks, int rowTiles) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* slab = lds;
  float* dyS = slab + ((p.NF * p.FS + 3) & ~3);  // [256][Cout]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, lq = lane >> 4;

  int ko[kTdsMaxTilesPerWave];
  bool one[kTdsMaxTilesPerWave], val[kTdsMaxTilesPerWave];
#pragma unroll
  for (int tl = 0; tl < kTdsMaxTilesPerWave; ++tl) {
    const int kk = 16 * (wave + 4 * tl) + i;
    const int tap = kk / p.Cin, c = kk - tap * p.Cin;
    val[tl] = kk < p.K;
    one[tl] = kk == p.K;
    ko[tl] = val[tl] ? tap * p.FS + c : 0;
  }
  f32x4 acc[kTdsMaxTilesPerWave][NT];
#pragma unroll
  for (int tl = 0; tl < kTdsMaxTilesPerWave; ++tl)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[tl][nt][q] = 0.f;

  // piece descriptors (chunk-independent): slab piece v -> frame f, float offset o inside the frame
  const int xq = (kTdsBH * p.Cin) >> 2;          // float4 per slab frame
  const int xTotal = p.NF * xq;
  const int dq = (kTdsBH * p.Cout) >> 2;         // float4 per dy frame
  const int dTotal = kTdsBTF * dq;
  const int HCi = p.H * p.Cin, HCo = p.H * p.Cout;
  int xf[kTdsMaxXV], xo[kTdsMaxXV];
#pragma unroll
  for (int v = 0; v < kTdsMaxXV; ++v) {
    const int e = tid + 256 * v;
    xf[v] = e < xTotal ? e / xq : -1;
    xo[v] = e < xTotal ? (e - xf[v] * xq) << 2 : 0;
  }
  int df[kTdsMaxDV], dof[kTdsMaxDV];
#pragma unroll
  for (int v = 0; v < kTdsMaxDV; ++v) {
    const int e = tid + 256 * v;
    df[v] = e < dTotal ? e / dq : -1;
    dof[v] = e < dTotal ? (e - df[v] * dq) << 2 : 0;
  }
  // the 4-float pad of every slab frame is never overwritten: zero it once
  for (int f = tid; f < p.NF; f += 256) *(float4*)(slab + f * p.FS + kTdsBH * p.Cin) = make_float4(0.f, 0.f, 0.f, 0.f);

  // lean-loop constants: fragment base offsets (floats) with the lane's lq folded in, tiles of this wave, and
  // whether this wave's LAST tile carries the all-ones row (row K) of the bias gradient
  int abase[kTdsMaxTilesPerWave], dbase[NT];
#pragma unroll
  for (int tl = 0; tl < kTdsMaxTilesPerWave; ++tl) abase[tl] = ko[tl] + lq * p.Cin;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) dbase[nt] = lq * p.Cout + (16 * nt + i < p.Cout ? 16 * nt + i : p.Cout - 1);
  const int ntw = wave < rowTiles ? (rowTiles - wave + 3) / 4 : 0;
  const bool ownsOne = ntw > 0 && (wave + 4 * (ntw - 1)) == p.K / 16;
  const bool oneLane = i == (p.K & 15);
  (void)abase; (void)dbase; (void)ownsOne; (void)oneLane;

  float4 xr[kTdsMaxXV], dr[kTdsMaxDV];
  auto fetch = [&](int chunk) {
    const int hb = chunk % hBlocks, tb = (chunk / hBlocks) % tBlocks, b = chunk / (hBlocks * tBlocks);
    const int h0 = hb * kTdsBH, t0 = tb * kTdsBTF, tIn0 = t0 * p.stride - p.padl;
    const float* xb = p.x + ((size_t)b * p.Tin * p.H + h0) * p.Cin;
    const float* db = dy + ((size_t)b * p.Tout * p.H + h0) * p.Cout;
#pragma unroll
    for (int v = 0; v < kTdsMaxXV; ++v) {
      const int ti = tIn0 + xf[v];
      const bool ok = xf[v] >= 0 && ti >= 0 && ti < p.Tin;
      // unconditional load from a clamped (valid) address + select: no branch around the load
      const float4 t4 = *(const float4*)(xb + (size_t)(ok ? ti : 0) * HCi + xo[v]);
      xr[v] = ok ? t4 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int v = 0; v < kTdsMaxDV; ++v) {
      const int t = t0 + df[v];
      const bool ok = df[v] >= 0 && t < p.Tout;
      const float4 t4 = *(const float4*)(db + (size_t)(ok ? t : 0) * HCo + dof[v]);
      dr[v] = ok ? t4 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };

  int chunk = blockIdx.x;
  if (chunk < nChunks) fetch(chunk);
  for (; chunk < nChunks; chunk += gridDim.x) {
    __syncthreads();  // previous chunk's fragment reads are done
#pragma unroll
    for (int v = 0; v < kTdsMaxXV; ++v)
      if (xf[v] >= 0) *(float4*)(slab + xf[v] * p.FS + xo[v]) = xr[v];
#pragma unroll
    for (int v = 0; v < kTdsMaxDV; ++v)
      if (df[v] >= 0) *(float4*)(dyS + df[v] * (kTdsBH * p.Cout) + dof[v]) = dr[v];
    __syncthreads();
    const int nxt = chunk + gridDim.x;
    fetch(nxt < nChunks ? nxt : chunk);  // in flight behind this chunk's MFMAs (last trip: harmless re-load)
    if constexpr (C > 0) {
      switch (ntw) {  // wave-uniform
        case 3: tds_filter_kloop<NT, C, 3>(slab, dyS, abase, dbase, ownsOne, oneLane, acc); break;
        case 4: tds_filter_kloop<NT, C, 4>(slab, dyS, abase, dbase, ownsOne, oneLane, acc); break;
        case 5: tds_filter_kloop<NT, C, 5>(slab, dyS, abase, dbase, ownsOne, oneLane, acc); break;
        case 6: tds_filter_kloop<NT, C, 6>(slab, dyS, abase, dbase, ownsOne, oneLane, acc); break;
        default: break;  // (host guarantees 3..6 for the compile-time channel counts)
      }
    } else {
#pragma unroll 4
      for (int kq = 0; kq < kTdsBTF * kTdsBH / 4; ++kq) {
        const int m = 4 * kq + lq;
        const int rowoff = (m >> 4) * p.stride * p.FS + (m & 15) * p.Cin;
        float bf[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bf[nt] = (16 * nt + i < p.Cout) ? dyS[m * p.Cout + 16 * nt + i] : 0.f;
#pragma unroll
        for (int tl = 0; tl < kTdsMaxTilesPerWave; ++tl) {
          if (wave + 4 * tl < rowTiles) {  // wave-uniform
            float a = slab[rowoff + ko[tl]];
            a = one[tl] ? 1.f : (val[tl] ? a : 0.f);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[tl][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bf[nt], acc[tl][nt], 0, 0, 0);
          }
        }
      }
    }
  }
  float* dst = partial + (size_t)blockIdx.x * rowTiles * 16 * (16 * NT);
#pragma unroll
  for (int tl = 0; tl < kTdsMaxTilesPerWave; ++tl) {
    const int tile = wave + 4 * tl;
    if (tile < rowTiles) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[(size_t)(tile * 16 + 4 * lq + q) * (16 * NT) + 16 * nt + i] = acc[tl][nt][q];
    }
  }
}

// dw[kk][co] = sum_g partial[g][kk][co] ; dbias[co] = row K.  One workgroup per output row kk: 16 lanes
// span the columns, 16 lane groups stride over the parts, fixed-order LDS tree (deterministic).
__global__ __launch_bounds__(256) void tds_conv_filter_reduce2_k(const float* __restrict__ partial, int nParts, int rows, int ncp,
                                                                int K, int Cout, float* __restrict__ dw, float* __restrict__ dbias) {
  __shared__ float red[16][32];
  const int kk = blockIdx.x, col = threadIdx.x % ncp, grp = threadIdx.x / ncp, ngrp = 256 / ncp;
  float s = 0.f;
  for (int g = grp; g < nParts; g += ngrp) s += partial[((size_t)g * rows + kk) * ncp + col];
  red[grp][col] = s;
  __syncthreads();
  if (grp == 0 && col < Cout) {
    float t = 0.f;
    for (int g = 0; g < ngrp; ++g) t += red[g][col];
    if (kk < K) dw[(size_t)kk * Cout + col] = t;
    else if (dbias) dbias[col] = t;
  }
}

// dw[kk][co] = sum_g partial[g][kk][co] ; dbias[co] = row K.  64 elements x 16 slices of the partials per block (one thread
// walking all the partials of its element took 126-146 us per call: 2 ms of the streaming recipe's step), slices combined
// in fixed order through LDS: deterministic.
__global__ __launch_bounds__(1024) void tds_conv_filter_reduce_k(const float* __restrict__ partial, int nParts, int rows, int ncp,
                                                                int K, int Cout, float* __restrict__ dw, float* __restrict__ dbias) {
  constexpr int NS = 16;
  __shared__ float red[NS][64];
  const int el = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;
  const bool in = e < (K + 1) * Cout;
  const int kk = in ? e / Cout : 0, co = in ? e - kk * Cout : 0;
  const int per = (nParts + NS - 1) / NS;
  const int g0 = sl * per, g1 = g0 + per < nParts ? g0 + per : nParts;
  const float* src = partial + (size_t)kk * ncp + co;
  const size_t step = (size_t)rows * ncp;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (in) {
    int g = g0;
    for (; g + 4 <= g1; g += 4) {
      s0 += src[(size_t)g * step]; s1 += src[(size_t)(g + 1) * step]; s2 += src[(size_t)(g + 2) * step]; s3 += src[(size_t)(g + 3) * step];
    }
    for (; g < g1; ++g) s0 += src[(size_t)g * step];
  }
  red[sl][el] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (sl == 0 && in) {
    float t = red[0][el];
#pragma unroll
    for (int k = 1; k < NS; ++k) t += red[k][el];
    if (kk < K) dw[e] = t;
    else if (dbias) dbias[co] = t;
  }
}

static inline int tds_out_len(int T, int kw, int stride, int padl, int padr) {
  int n = T + padl + padr - kw;
  return n < 0 ? 0 : n / stride + 1;
}

bool tds_conv_applicable(const w2l_conv_desc* d) {
  return d->Cout <= 32 && d->Cin <= 32 && d->kw * d->Cin + 1 <= 16 * 4 * kTdsMaxTilesPerWave;
}

static TdsConvP make_p(int B, int Tin, int Tout, int H, int Cin, int Cout, int kw, int stride, int padl, int bt) {
  TdsConvP p{};
  p.B = B; p.Tin = Tin; p.Tout = Tout; p.H = H; p.Cin = Cin; p.Cout = Cout; p.kw = kw; p.stride = stride; p.padl = padl;
  p.K = kw * Cin;
  p.Kp = (p.K + 3) & ~3;
  p.FS = kTdsBH * Cin + 4;
  p.NF = (bt - 1) * stride + kw;
  p.tapOff = 0; p.tapStep = 1; p.oOff = 0; p.oStep = 1; p.ToutFull = Tout;
  return p;
}

static size_t fwd_lds_bytes(const TdsConvP& p) {
  size_t slab = (size_t)p.NF * p.FS;
  const size_t outS = (size_t)kTdsBT * kTdsBH * p.Cout;
  if (outS > slab) slab = outS;
  slab = (slab + 3) & ~(size_t)3;
  const size_t ws = ((size_t)p.Kp * p.Cout + 3) & ~(size_t)3;
  return (slab + ws + p.Kp) * sizeof(float);
}

static size_t fwd2_lds_bytes(const TdsConvP& p, int bt) {
  size_t slab = (size_t)p.NF * p.FS;
  const size_t outS = (size_t)bt * kTdsBH * p.Cout;
  if (outS > slab) slab = outS;
  slab = (slab + 3) & ~(size_t)3;
  const size_t ws = ((size_t)p.Kp * p.Cout + 3) & ~(size_t)3;
  return (slab + ws + p.Kp) * sizeof(float);
}

template <int NT, int R, int CIN>
static int launch_fwd2_t(const TdsConvP& p, size_t shmem, hipStream_t s) {
  constexpr int BT = 4 * R;
  const int tBlocks = (p.Tout + BT - 1) / BT, hBlocks = p.H / kTdsBH;
  const int nTiles = p.B * tBlocks * hBlocks;
  const int perCu = 2;  // 174-215 VGPRs: two waves per SIMD
  const int blocks = nTiles < 256 * perCu ? nTiles : 256 * perCu;
  if (shmem > 64 * 1024)
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_fwd2_k<NT, R, CIN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL((tds_conv_fwd2_k<NT, R, CIN>), dim3((unsigned)blocks), dim3(256), shmem, s, p, nTiles, tBlocks, hBlocks);
  return W2L_OK;
}

// persistent register-prefetching kernel when the geometry allows it; `pIn` was built for 32-frame tiles
static bool try_launch_fwd2(const TdsConvP& pIn0, hipStream_t s, int* status, int profKind = PROF_TDSCONV) {
  TdsConvP pIn = pIn0;
  pIn.abl = 0;
  if (pIn.H % kTdsBH || ((pIn.H * pIn.Cin) & 3) || ((pIn.H * pIn.Cout) & 3) || ((kTdsBH * pIn.Cin) & 3) || ((kTdsBH * pIn.Cout) & 3)) return false;
  if ((((uintptr_t)pIn.x | (uintptr_t)pIn.y | (uintptr_t)pIn.add) & 15) != 0) return false;
  for (int bt = 32; bt >= 16; bt >>= 1) {
    TdsConvP p = pIn;
    p.NF = (bt - 1) * p.stride + p.kw;
    const int pieces = (p.NF * ((kTdsBH * p.Cin) >> 2) + 255) / 256;
    const size_t shmem = fwd2_lds_bytes(p, bt);
    if (pieces > kTdsMaxXV || 2 * shmem > 160 * 1024) continue;  // two workgroups per CU or nothing
    const double flops = 2.0 * p.B * p.Tout * (double)p.H * p.K * p.Cout;
    prof_begin(s, flops, profKind);
    int st;
    const int cin = p.stride == 1 ? p.Cin : 0;  // compile-time channel counts of the TDS-CTC recipe; anything else: runtime stride
    if (p.Cout <= 16) {
      if (bt == 32) st = cin == 10 ? launch_fwd2_t<1, 8, 10>(p, shmem, s) : cin == 14 ? launch_fwd2_t<1, 8, 14>(p, shmem, s)
                       : cin == 18 ? launch_fwd2_t<1, 8, 18>(p, shmem, s) : launch_fwd2_t<1, 8, 0>(p, shmem, s);
      else st = cin == 10 ? launch_fwd2_t<1, 4, 10>(p, shmem, s) : cin == 14 ? launch_fwd2_t<1, 4, 14>(p, shmem, s)
                : cin == 18 ? launch_fwd2_t<1, 4, 18>(p, shmem, s) : launch_fwd2_t<1, 4, 0>(p, shmem, s);
    } else {
      if (bt == 32) st = cin == 18 ? launch_fwd2_t<2, 8, 18>(p, shmem, s) : launch_fwd2_t<2, 8, 0>(p, shmem, s);
      else st = cin == 18 ? launch_fwd2_t<2, 4, 18>(p, shmem, s) : launch_fwd2_t<2, 4, 0>(p, shmem, s);
    }
    prof_end(s);
    if (st == W2L_OK && hipGetLastError() != hipSuccess) st = W2L_EHIP;
    *status = st;
    return true;
  }
  return false;
}

static int launch_fwd(const TdsConvP& p, hipStream_t s, int profKind = PROF_TDSCONV) {
  int st2 = W2L_OK;
  // the specialised kernels first (conv_tds_special.hip), then the general ones of this file
  if (tds_c1_fwd_try(p, profKind, s, &st2) || tds_tz_try(p, profKind, s, &st2)) return st2;
  if (try_launch_fwd2(p, s, &st2, profKind)) return st2;
  const size_t shmem = fwd_lds_bytes(p);
  if (shmem > 160 * 1024) return W2L_EUNSUPPORTED;
  dim3 grid((unsigned)((p.H + kTdsBH - 1) / kTdsBH), (unsigned)((p.Tout + kTdsBT - 1) / kTdsBT), (unsigned)p.B);
  const double flops = 2.0 * p.B * p.Tout * (double)p.H * p.K * p.Cout;
  prof_begin(s, flops, profKind);
  if (p.Cout <= 16) {
    if (shmem > 64 * 1024) W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_fwd_k<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(tds_conv_fwd_k<1>, grid, dim3(256), shmem, s, p);
  } else {
    if (shmem > 64 * 1024) W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_fwd_k<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(tds_conv_fwd_k<2>, grid, dim3(256), shmem, s, p);
  }
  prof_end(s);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

int tds_conv_forward(const w2l_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int relu,
                     hipStream_t s) {
  const int To = tds_out_len(d->T, d->kw, d->stride, d->padl, d->padr);
  TdsConvP p = make_p(d->B, d->T, To, d->H, d->Cin, d->Cout, d->kw, d->stride, d->padl, kTdsBT);
  p.x = x; p.w = w; p.bias = bias; p.y = y; p.relu = relu;
  p.CinW = d->Cin; p.CoutW = d->Cout;
  return launch_fwd(p, s);
}

// dx = conv(dy, flipped W^T) with left padding kw-1-padl; dx = add + conv (add may be null).
// stride s > 1: one stride-1 launch per phase f = (ti + padl) mod s.  Only the taps tap = f + s*j reach those input
// frames (ti + padl = s*to + tap), so phase f is a stride-1 correlation of dy with the kw_f = ceil((kw-f)/s) taps
// W[f + s*j], written to every s-th frame of dx: no zero-stuffed dy, no wasted multiplies, each dx frame written once.
int tds_conv_backward_data(const w2l_conv_desc* d, const float* dy, const float* w, float* dx, int accumulate,
                           const float* add, hipStream_t s) {
  const int To = tds_out_len(d->T, d->kw, d->stride, d->padl, d->padr);
  if (d->stride == 1) {
    TdsConvP p = make_p(d->B, To, d->T, d->H, d->Cout, d->Cin, d->kw, 1, d->kw - 1 - d->padl, kTdsBT);
    p.x = dy; p.w = w; p.y = dx; p.accum = accumulate; p.add = add; p.flip = 1;
    p.CinW = d->Cin; p.CoutW = d->Cout;
    return launch_fwd(p, s, PROF_TDS_BWD_DATA);
  }
  const int st = d->stride;
  if (st > d->kw) return W2L_EUNSUPPORTED;  // every phase needs at least one tap
  bool launched = false;   // a phase of this call has run (the geometry is the same for every phase: only the FIRST one can be refused)
  for (int f = 0; f < st; ++f) {
    const int kwf = (d->kw - f + st - 1) / st;
    const int c0 = (((f - d->padl) % st) + st) % st;   // first input frame of the phase
    if (c0 >= d->T) continue;
    const int U = (d->T - c0 + st - 1) / st;           // input frames of the phase
    const int s0 = (c0 + d->padl - f) / st;            // dy frame of tap f at u = 0
    TdsConvP p = make_p(d->B, To, U, d->H, d->Cout, d->Cin, kwf, 1, kwf - 1 - s0, kTdsBT);
    p.x = dy; p.w = w; p.y = dx; p.accum = accumulate; p.add = add; p.flip = 1;
    p.CinW = d->Cin; p.CoutW = d->Cout;
    p.tapOff = f; p.tapStep = st; p.oOff = c0; p.oStep = st; p.ToutFull = d->T;
    int st2 = W2L_OK;
    if (tds_tz_try(p, PROF_TDS_BWD_DATA, s, &st2)) {
      if (st2 != W2L_OK) return st2;
      launched = true;
      continue;
    }
    // (was `f == 0 ? unsupported : error`: with T = 1 and an odd left padding phase 0 has no input frame and is skipped, so the
    //  refusal of a geometry these kernels do not hold came back as an error instead of sending the caller to the generic path:
    //  round 5, test_conv_random_geometries)
    if (!try_launch_fwd2(p, s, &st2, PROF_TDS_BWD_DATA)) return launched ? W2L_EHIP : W2L_EUNSUPPORTED;
    if (st2 != W2L_OK) return st2;
    launched = true;
  }
  return W2L_OK;
}

int tds_conv_backward_filter(const w2l_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                             hipStream_t s) {
  const int To = tds_out_len(d->T, d->kw, d->stride, d->padl, d->padr);
  TdsConvP p = make_p(d->B, d->T, To, d->H, d->Cin, d->Cout, d->kw, d->stride, d->padl, kTdsBTF);
  p.x = x;
  {  // the specialised kernels first (conv_tds_special.hip), then the general ones of this file
    int st2 = W2L_OK;
    if (tds_rsf_try(p, dy, dw, dbias, s, &st2) || tds_c1_filter_try(p, dy, dw, dbias, s, &st2) ||
        tds_tzf_strided_try(p, dy, dw, dbias, s, &st2))
      return st2;
  }
  const int rowTiles = (p.K + 1 + 15) / 16;
  if (rowTiles > 4 * kTdsMaxTilesPerWave) return W2L_EUNSUPPORTED;
  const int NT = d->Cout <= 16 ? 1 : 2;
  const int tBlocks = (To + kTdsBTF - 1) / kTdsBTF, hBlocks = (d->H + kTdsBH - 1) / kTdsBH;
  const int nChunks = d->B * tBlocks * hBlocks;
  int blocks = nChunks < 512 ? nChunks : 512;
  const size_t shmem = ((((size_t)p.NF * p.FS + 3) & ~(size_t)3) + (size_t)kTdsBTF * kTdsBH * p.Cout) * sizeof(float);
  if (shmem > 160 * 1024) return W2L_EUNSUPPORTED;
  const size_t partFloats = (size_t)blocks * rowTiles * 16 * 16 * NT;
  // partial sums live in the library's per-stream scratch (shared with the stream-K slabs: same stream => ordered)
  float* partial = sk_scratch(s, kSkScratchBytes);
  if (!partial || partFloats > (size_t)kSkSlots * 2 * kSlabFloats) return W2L_EUNSUPPORTED;
  const double flops = 2.0 * d->B * To * (double)d->H * p.K * d->Cout;
  // pipelined kernel: whole mel blocks, float4-addressable rows, piece counts within the register budget
  const int xPieces = (p.NF * ((kTdsBH * p.Cin) >> 2) + 255) / 256, dPieces = (kTdsBTF * ((kTdsBH * p.Cout) >> 2) + 255) / 256;
  const bool fast = d->H % kTdsBH == 0 && (d->H * d->Cin) % 4 == 0 && (d->H * d->Cout) % 4 == 0 && (kTdsBH * d->Cin) % 4 == 0 &&
                    (kTdsBH * d->Cout) % 4 == 0 && xPieces <= kTdsMaxXV && dPieces <= kTdsMaxDV &&
                    (((uintptr_t)x | (uintptr_t)dy) & 15) == 0 && !tune_env("W2L_TDS_FILTER_V1");
  prof_begin(s, flops, PROF_TDS_BWD_FILTER);
  if (fast) {
#define W2L_FILTER2(NTv, Cv)                                                                                                    \
  do {                                                                                                                          \
    if (shmem > 64 * 1024)                                                                                                      \
      W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_filter2_k<NTv, Cv>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                        (int)shmem));                                                                           \
    hipLaunchKernelGGL((tds_conv_filter2_k<NTv, Cv>), dim3((unsigned)blocks), dim3(256), shmem, s, p, dy, partial, nChunks,     \
                       tBlocks, hBlocks, rowTiles);                                                                             \
  } while (0)
    // lean K loop for the TDS convolutions proper (C -> C, stride 1, 3..6 row tiles per wave)
    const int cc = (d->Cin == d->Cout && d->stride == 1 && rowTiles >= 12 && !tune_env("W2L_TDS_FILTER_GENERIC")) ? d->Cin : 0;
    if (NT == 1) {
      if (cc == 10) W2L_FILTER2(1, 10);
      else if (cc == 14) W2L_FILTER2(1, 14);
      else W2L_FILTER2(1, 0);
    } else {
      if (cc == 18) W2L_FILTER2(2, 18);
      else W2L_FILTER2(2, 0);
    }
#undef W2L_FILTER2
    hipLaunchKernelGGL(tds_conv_filter_reduce2_k, dim3((unsigned)(p.K + 1)), dim3(256), 0, s, partial, blocks, rowTiles * 16,
                       16 * NT, p.K, d->Cout, dw, dbias);
    prof_end(s);
    W2L_LAUNCH_CHECK();
    return W2L_OK;
  }
  if (NT == 1) {
    if (shmem > 64 * 1024) W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_filter_k<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(tds_conv_filter_k<1>, dim3((unsigned)blocks), dim3(256), shmem, s, p, dy, partial, nChunks, tBlocks, hBlocks, rowTiles);
  } else {
    if (shmem > 64 * 1024) W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_filter_k<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(tds_conv_filter_k<2>, dim3((unsigned)blocks), dim3(256), shmem, s, p, dy, partial, nChunks, tBlocks, hBlocks, rowTiles);
  }
  const int n = (p.K + 1) * d->Cout;
  hipLaunchKernelGGL(tds_conv_filter_reduce_k, dim3((unsigned)((n + 63) / 64)), dim3(1024), 0, s, partial, blocks, rowTiles * 16,
                     16 * NT, p.K, d->Cout, dw, dbias);
  prof_end(s);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

}  // namespace w2l
