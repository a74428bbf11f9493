// gemm_glds.hpp -- persistent fp32 MFMA GEMM with direct-to-LDS operand staging (gfx950).
//
// The second-generation main loop of the fl::Linear GEMMs (see gemm.hip for the reference call sites).
// Same 128x128x32 block tile / 4 waves x (2x2) v_mfma_f32_32x32x2_f32 as gemm128_kernel, but
//   * operand tiles go global -> LDS by `global_load_lds_dwordx4` (LDS-DMA): no staging VGPRs, no
//     ds_write pass, no transposing scalar stores between the MFMAs.  The LDS image is lane-linear
//     per wave-instruction (1 KiB pieces), so the bank-conflict-free layout is produced by permuting
//     the per-lane SOURCE address (XOR swizzle), not by padding;
//   * k-contiguous operands keep k contiguous in LDS ([i][32 k], 128-B rows) and a lane fetches FOUR
//     consecutive k of its row with one ds_read_b128.  The MFMA k-slot assignment inside a group of
//     8 k is  k = 8g + 4*(lane>>5) + q  (q = 0..3 = the four MFMA k-steps of the group) for BOTH
//     operands, which only permutes the order of the k-sum;
//   * the kernel is persistent: 2 workgroups per CU walk a static list of (tile, k-range) segments
//     (whole tiles first, then one stream-K range) and the first K tile of the NEXT segment is
//     already in flight while the current segment's last K tile is multiplied and its epilogue
//     runs -- the per-tile prologue latency (5.6 K-iterations per tile in the first-generation kernel,
//     measured on MI355X) is off the critical path;
//   * tiles are rasterised in groups of 8 tile-columns, N-fastest inside a group, and the worker id
//     is XCD-major, so the 64 workgroups of one XCD work on an 8x8 block of tiles that shares
//     8 + 8 operand panels in that XCD's L2.
// Shapes (line 4 of the dispatch in gemm.hip's header; launch128g): K % 32 == 0 and either 16-byte aligned operand pointers
// and leading dimensions with extents % 4 == 0, or dword-aligned operands below 2 GiB; whatever gemm160_kernel does not take.
// Two instances per operand layout pair:
//   BUF = true   buffer-addressed LDS-DMA (`buffer_load_dwordx4 ... lds`: 32-bit offsets, bounds-checked): both operands below 2 GiB
//   BUF = false  64-bit `global_load_lds` addresses: what runs for (strictly aligned) operands of 2 GiB and more
// Stream-K partial tiles are added inside the launch (g_slab_handover; up to 1024 stream-K tiles), or by gemm128_fixup.
// Also here, shared with gemm_t160.hpp and gemm_bf16g.hpp: GOp, the swizzled piece addressing, g_segment (the persistent
// schedule), gemm128g_epilogue_wide and g_slab_handover.
#pragma once
#include <cstdlib>

#include "gemm.hpp"

namespace w2l {

struct GOp {
  const float* p;
  int ld;
  int extent;  // number of valid i (rows of A / columns of B)
  unsigned bytes = 0;  // size of the operand's address range (buffer-addressed variant; 0 = too large)
};

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int kGStageFloats = 2 * 128 * 32;  // A tile + B tile of one K step

// XCD-major worker id: hardware workgroup b runs on XCD b % 8; give XCD x the 64 consecutive
// logical workers [64x, 64x + 64) of a 512-wide round (bijective for any worker count)
__device__ __forceinline__ int xcd_major(int b, int workers) {
  const int q = workers / 8, r = workers % 8, x = b % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

template <bool KC>
__device__ __forceinline__ void g_init_ptrs(const float* (&q)[4], const GOp& op, int i0, int wave, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (KC) {
      const int r = (wave * 4 + j) * 8 + (lane >> 3);             // tile row 0..127
      const int c = (lane & 7) ^ ((r >> 1) & 7);                  // source chunk of this LDS slot
      int gi = i0 + r;
      if (gi > op.extent - 1) gi = op.extent - 1;
      q[j] = op.p + (size_t)gi * op.ld + 4 * c;
    } else {
      const int kr = (wave * 4 + j) * 2 + (lane >> 5);            // tile k-row 0..31
      int gi = i0 + 4 * (lane & 31);
      if (gi >= op.extent) gi = (op.extent - 1) & ~3;  // a chunk that straddles the row end stays in place (its tail columns are never stored)
      q[j] = op.p + (size_t)kr * op.ld + gi;
    }
  }
}

__device__ __forceinline__ void g_issue(const float* const (&q)[4], size_t off, float* ldsTile, int wave) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    __builtin_amdgcn_global_load_lds((gptr_t)(q[j] + off), (lptr_t)(ldsTile + (wave * 4 + j) * 256), 16, 0, 0);
}

__device__ __forceinline__ void g_issue1(const float* q, size_t off, float* ldsTile, int wave, int j) {
  __builtin_amdgcn_global_load_lds((gptr_t)(q + off), (lptr_t)(ldsTile + (wave * 4 + j) * 256), 16, 0, 0);
}

// ---- buffer-addressed variant (BUF): the operand is described by a 128-bit buffer resource in SGPRs, the
// lane supplies ONE 32-bit byte offset (half the address VGPR traffic of a 64-bit global pointer) and the
// K advance rides in the scalar offset of the instruction -- no per-piece 64-bit VALU add.
template <bool KC>
__device__ __forceinline__ void g_init_offs(uint32_t (&vo)[4], const GOp& op, int i0, int wave, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (KC) {
      const int r = (wave * 4 + j) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ ((r >> 1) & 7);
      int gi = i0 + r;
      if (gi > op.extent - 1) gi = op.extent - 1;
      vo[j] = ((uint32_t)gi * (uint32_t)op.ld + 4u * c) * 4u;
    } else {
      const int kr = (wave * 4 + j) * 2 + (lane >> 5);
      int gi = i0 + 4 * (lane & 31);
      if (gi >= op.extent) gi = (op.extent - 1) & ~3;  // a chunk that straddles the row end stays in place (its tail columns are never stored)
      vo[j] = ((uint32_t)kr * (uint32_t)op.ld + (uint32_t)gi) * 4u;
    }
  }
}
__device__ __forceinline__ void g_issue1_buf(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, uint32_t soff, float* ldsTile, int wave, int j) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)(ldsTile + (wave * 4 + j) * 256), 16, (int)voff, (int)soff, 0, 0);
}

// fragments of one 8-k group for the two 32-row MFMA tiles of this wave
template <bool KC>
__device__ __forceinline__ void g_frag(float (&f)[2][4], const float* tile, int w0, int g, int li, int lh) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (KC) {
      const int r = w0 + 32 * i + li;
      const int c = (2 * g) ^ lh ^ ((li >> 1) & 7);
      const f32x4 v = *(const f32x4*)(tile + r * 32 + 4 * c);
      f[i][0] = v[0]; f[i][1] = v[1]; f[i][2] = v[2]; f[i][3] = v[3];
    } else {
      const float* src = tile + (8 * g + 4 * lh) * 128 + w0 + 32 * i + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) f[i][q] = src[q * 128];
    }
  }
}


// Epilogue with 16-byte stores.  The MFMA C layout gives a lane 16 rows of ONE column, so the direct
// epilogue (gemm128_epilogue) issues 64 global_store_dword per lane and per tile -- store-issue bound: with
// the K loop ablated the TDS fc shapes ran at 117 TF/s against 145 TF/s at 4096^3 (MI355X).  Here each
// wave turns its 64x64 sub-tile through its own 8 KiB slice of the LDS stage that the K loop has just
// released (two 32-row halves): ds_write_b32 in C layout, ds_read_b128 as 4 rows x 16 float4 per
// instruction, then 16 global_store_dwordx4 per lane.  Bias / ReLU / mask / accumulate are applied on
// the float4.  Requires a 16-byte aligned C and ldc % 4 == 0 (host-checked; `wide` false otherwise).
// quad: which 64 x 64 quadrant of the 128 x 128 tile this wave holds (-1: threadIdx.x >> 6); slice: which 8 KiB slice of
// `scratch` it turns its rows through (-1: the same) -- the 256 x 256 kernel runs two 4-wave groups side by side
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 g_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float g_f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t g_pack2(float a, float b) {   // two bf16, round to nearest even (v_cvt_pk_bf16_f32): convert.hip's cv_pack2
  const g_f32x2_t v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, g_bf16x2_t));
}
// IMG (the bf16-operand kernels): out.imgRows / out.imgTrans / out.maskH are honoured (see GemmOut).  The row image leaves with the
// float4 as four bf16 (128-byte row segments per 16 lanes); for the transposed image the finished float4 goes back into its LDS slot
// and, after the half's eight passes, lane c reads column c of the 32 x 64 slice and stores 32 consecutive rows = 64 bytes of
// image row n0 + c (the two halves of a wave complete the 128-byte line in the L2).
template <bool IMG = false>
__device__ __forceinline__ void gemm128g_epilogue_wide(const GemmOut& out, int m0, int n0, const f32x16 (&acc)[2][2],
                                                       float* scratch, const float (&bv)[4], int quad = -1, int slice = -1) {
  const int EPI = out.epi;
  const int lane = threadIdx.x & 63, wave = quad >= 0 ? quad : (int)(threadIdx.x >> 6);
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int li = lane & 31, lh = lane >> 5;
  float* sc = scratch + (slice >= 0 ? slice : wave) * 2048;       // [32 rows][64 cols] of this wave
  const int c4 = 4 * (lane & 15), rq = lane >> 4;
  const int n = n0 + wn + c4;
  const bool fullVec = n + 3 < out.N;
  // (Register budget: 187 - 195 VGPRs with the eight prefetched operand vectors of a half below -- two workgroups leave ~120
  // registers per SIMD lane free, room for a communication kernel's waves to co-reside during the overlapped gradient all-reduce.
  // Round 1 had tried the prefetch for all 16 rows of a wave at once and seen no gain; per half, with clamped instead of predicated
  // addresses, it is worth 10 - 15 us per product that has a mask or an addend: profiles/r06_run26 ... r06_run28_*.)
  const float* accSrc = out.addend ? out.addend : out.C;
  // the mask (or, without one, the addend / accumulate operand) of a half's eight row passes is fetched BEFORE the half's LDS turn,
  // addresses clamped instead of predicated (see t160_epilogue: in the pass loop every pass paid its own memory round trip)
  const bool preMask = (EPI & EPI_MASK) != 0, preAdd = !preMask && (EPI & EPI_ACCUM);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    f32x4 pre[8];
    if (IMG && preMask && out.maskH) {
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        int m;
        const bool ok = gemm_out_row(out, m0 + wm + 32 * i + 4 * p + rq, m) && fullVec;
        const u32x2 u = __builtin_nontemporal_load((const u32x2*)(out.maskH + (ok ? (size_t)m * out.ldMaskH + n : (size_t)0)));
        pre[p][0] = __uint_as_float(u[0] << 16); pre[p][1] = __uint_as_float(u[0] & 0xffff0000u);
        pre[p][2] = __uint_as_float(u[1] << 16); pre[p][3] = __uint_as_float(u[1] & 0xffff0000u);
      }
    } else if (preMask || preAdd) {
      const float* src = preMask ? out.mask : accSrc;
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        int m;
        const bool ok = gemm_out_row(out, m0 + wm + 32 * i + 4 * p + rq, m) && fullVec;
        pre[p] = __builtin_nontemporal_load((const f32x4*)(src + (ok ? (size_t)m * out.ldc + n : (size_t)0)));   // read once: not worth a cache line next to the operand panels
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[((r & 3) + 8 * (r >> 2) + 4 * lh) * 64 + j * 32 + li] = acc[i][j][r];
    // same wave wrote and reads: LDS operations of one wave complete in order, no barrier needed
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int row = 4 * p + rq;
      const f32x4 v4 = *(const f32x4*)(sc + row * 64 + c4);
      int m;
      if (!gemm_out_row(out, m0 + wm + 32 * i + row, m) || n >= out.N) continue;
      float v[4] = {v4[0] + bv[0], v4[1] + bv[1], v4[2] + bv[2], v4[3] + bv[3]};
      float* dst = out.C + (size_t)m * out.ldc + n;
      if (EPI & EPI_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      if (EPI & EPI_DROPOUT) {
        const uint64_t idx = (uint64_t)m * out.ldc + n;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = keep_elem(idx + e, out.dropSeed, out.dropStream, out.dropThr) ? v[e] * out.dropScale : 0.f;
      }
      if (fullVec) {
        if (EPI & EPI_MASK) {
          const f32x4 mk = pre[p];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = mk[e] > 0.f ? v[e] * out.maskScale : 0.f;
        }
        if (EPI & EPI_ACCUM) {
          const f32x4 o = preAdd ? pre[p] : *(const f32x4*)(accSrc + (size_t)m * out.ldc + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += o[e];
        }
        f32x4 w4;
        w4[0] = v[0]; w4[1] = v[1]; w4[2] = v[2]; w4[3] = v[3];
        if (!IMG || out.C) *(f32x4*)dst = w4;
        if (IMG && out.imgRows) {
          u32x2 h;
          h[0] = g_pack2(v[0], v[1]); h[1] = g_pack2(v[2], v[3]);
          *(u32x2*)(out.imgRows + (size_t)m * out.ldImgRows + n) = h;
        }
        if (IMG && out.imgTrans) *(f32x4*)(sc + row * 64 + c4) = w4;   // back into its slot, for the column pass below
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (n + e >= out.N) continue;
          float t = v[e];
          if (EPI & EPI_MASK) t = out.mask[(size_t)m * out.ldc + n + e] > 0.f ? t * out.maskScale : 0.f;
          if (EPI & EPI_ACCUM) t += accSrc[(size_t)m * out.ldc + n + e];
          dst[e] = t;
        }
      }
    }
    if (IMG && out.imgTrans) {   // (host: N % 4 == 0, no row remap -- every stored float4 above was a full one)
      const int nn = n0 + wn + lane, mb = m0 + wm + 32 * i;
      int rv = out.M - mb;
      rv = rv > 32 ? 32 : rv;
      if (nn < out.N && rv > 0) {
        uint32_t pk[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) pk[q] = g_pack2(sc[(2 * q) * 64 + lane], sc[(2 * q + 1) * 64 + lane]);
        uint16_t* d = out.imgTrans + (size_t)nn * out.ldImgTrans + mb;
        if (rv == 32) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            u32x4 t;
            t[0] = pk[4 * q]; t[1] = pk[4 * q + 1]; t[2] = pk[4 * q + 2]; t[3] = pk[4 * q + 3];
            *(u32x4*)(d + 8 * q) = t;
          }
        } else {
          for (int rr = 0; rr < rv; ++rr) d[rr] = (uint16_t)(pk[rr >> 1] >> (16 * (rr & 1)));
        }
      }
    }
    // the second half overwrites the slice only after this wave's reads have returned (in-order LDS queue)
  }
}

struct GSeg {
  int tile, kb, ke, slab;  // slab: index of the partial slab (stream-K ranges), -1 = whole tile
  bool valid;
};

// segment `ord` of logical worker w: whole tiles w, w + workers, ... then the stream-K range w
__device__ __forceinline__ GSeg g_segment(const SkPlan& p, int w, int workers, int ord) {
  GSeg s;
  s.valid = false;
  s.tile = 0; s.kb = 0; s.ke = 0; s.slab = -1;
  if (p.ksplit) {   // aligned K split: unit u = (chunk, tile), chunk-major
    const int u = w + ord * workers;
    if (u >= p.ksplit * p.skTiles) return s;
    const int x = u / p.skTiles;
    s.tile = u - x * p.skTiles;
    s.kb = x * p.kChunk;
    s.ke = s.kb + p.kChunk < p.kTiles ? s.kb + p.kChunk : p.kTiles;
    s.slab = u;
    s.valid = true;
    return s;
  }
  const int nDp = w < p.dpTiles ? (p.dpTiles - w + workers - 1) / workers : 0;
  if (ord < nDp) {
    s.tile = w + ord * workers; s.kb = 0; s.ke = p.kTiles; s.valid = true;
    return s;
  }
  if (w >= p.skBlocks) return s;
  const int o = ord - nDp;
  if (o > 1) return s;
  long long it = sk_begin(p, w);
  const long long itEnd = sk_begin(p, w + 1);
  if (it >= itEnd) return s;
  long long firstEnd = (it / p.kTiles + 1) * (long long)p.kTiles;
  if (firstEnd > itEnd) firstEnd = itEnd;
  if (o == 1) {
    it = firstEnd;
    if (it >= itEnd) return s;
    firstEnd = itEnd;
  }
  s.tile = p.dpTiles + (int)(it / p.kTiles);
  s.kb = (int)(it % p.kTiles);
  s.ke = s.kb + (int)(firstEnd - it);
  s.slab = (s.kb == 0 && s.ke == p.kTiles) ? -1 : w * 2 + o;
  s.valid = true;
  return s;
}

// segment fields as SGPRs: left in VGPRs (the schedule's 64-bit divisions), the K-tile index makes hipcc wrap every
// buffer-addressed LDS-DMA issue in a readfirstlane "waterfall" loop for its scalar offset (8 loops per K tile in the ISA)
__device__ __forceinline__ GSeg g_pin(GSeg s) {
  s.tile = __builtin_amdgcn_readfirstlane(s.tile);
  s.kb = __builtin_amdgcn_readfirstlane(s.kb);
  s.ke = __builtin_amdgcn_readfirstlane(s.ke);
  s.slab = __builtin_amdgcn_readfirstlane(s.slab);
  s.valid = __builtin_amdgcn_readfirstlane((int)s.valid) != 0;
  return s;
}

// Hand-over of the in-kernel slab reduction (replaces the fix-up launch; cdna_hip_programming.md, in-launch split-K reduction
// recipe), called by every thread of a workgroup that has just stored a partial slab of stream-K tile `counter`.  Publish: every
// wave drains its slab stores, one lane releases at agent scope and draws the tile's arrival ticket (handed to the other waves
// through *flag, an LDS word nobody else uses now: the stage the K loop has just released).  The workgroup that draws ticket
// `last` (= arrivals - 1: uniform) is the tile's last arriver: it acquires and returns true -- the caller then adds ALL slabs of
// the tile from memory in range order (its own included: deterministic), runs the ordinary epilogue and re-zeroes the ticket.
// The order and the scopes below are the protocol: do not reorder.
__device__ __forceinline__ bool g_slab_handover(unsigned* counter, int* flag, int last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *flag = (int)__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const int ticket = *flag;
  if (ticket != last) return false;
  if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  __syncthreads();  // (also: every wave has read the ticket before the stage becomes epilogue scratch)
  return true;
}

// BUF: buffer-addressed LDS-DMA (the default); false: 64-bit global_load_lds addresses, for operands of 2 GiB and more
template <bool AKC, bool BKC, bool BUF = false>
__global__ __launch_bounds__(256, 2) void gemm128g_kernel(GOp aop, GOp bop, GemmOut out, SkPlan plan, int workers, int wide) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  // wave id as a SCALAR: LDS-DMA destinations (M0) and piece indices stay on the SALU, no v_readfirstlane per piece
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int li = lane & 31, lh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(xcd_major(blockIdx.x, workers));
  const size_t aStep = AKC ? 32 : (size_t)32 * aop.ld;
  const size_t bStep = BKC ? 32 : (size_t)32 * bop.ld;

  GSeg seg = g_pin(g_segment(plan, w, workers, 0));
  if (!seg.valid) return;
  const float* qa[4];
  const float* qb[4];
  uint32_t va[4], vb[4];
  __amdgpu_buffer_rsrc_t ra, rb;
  if (BUF) {
    ra = __builtin_amdgcn_make_buffer_rsrc((void*)aop.p, 0, (int)aop.bytes, 0x00020000);
    rb = __builtin_amdgcn_make_buffer_rsrc((void*)bop.p, 0, (int)bop.bytes, 0x00020000);
  }
  int bx, by;
  sk_tile_xy(plan, seg.tile, bx, by);
  if (BUF) {
    g_init_offs<AKC>(va, aop, bx * 128, wave, lane);
    g_init_offs<BKC>(vb, bop, by * 128, wave, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      g_issue1_buf(ra, va[j], (uint32_t)(aStep * seg.kb * 4), smem, wave, j);
      g_issue1_buf(rb, vb[j], (uint32_t)(bStep * seg.kb * 4), smem + 4096, wave, j);
    }
  } else {
    g_init_ptrs<AKC>(qa, aop, bx * 128, wave, lane);
    g_init_ptrs<BKC>(qb, bop, by * 128, wave, lane);
    g_issue(qa, aStep * seg.kb, smem, wave);
    g_issue(qb, bStep * seg.kb, smem + 4096, wave);
  }
  int stage = 0;
  __syncthreads();  // (drains the LDS-DMA: vmcnt(0) precedes the barrier)

  for (int ord = 0;; ++ord) {
    const GSeg nxt = g_pin(g_segment(plan, w, workers, ord + 1));
    // bias of this lane's four output columns, fetched at the START of the tile (its latency hides under the K loop)
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (out.epi & EPI_BIAS) {
      const int nb = by * 128 + wn + 4 * (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = nb + e < out.N ? out.bias[nb + e] : 0.f;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    for (int kt = seg.kb; kt < seg.ke; ++kt) {
      const float* As = smem + stage * kGStageFloats;
      const float* Bs = As + 4096;
      float* An = smem + (stage ^ 1) * kGStageFloats;
      float fa[2][2][4], fb[2][2][4];
      g_frag<AKC>(fa[0], As, wm, 0, li, lh);
      g_frag<BKC>(fb[0], Bs, wn, 0, li, lh);
      // What goes to the other stage during this iteration: the next K tile, or the first K tile of
      // the next segment, or (very last iteration of this worker) a harmless re-load of this tile.
      // Every wave has passed the barrier that ended the previous iteration, so nobody reads that stage.
      size_t offA = aStep * kt, offB = bStep * kt;
      if (kt + 1 < seg.ke) {
        offA += aStep; offB += bStep;
      } else if (nxt.valid) {
        int nbx, nby;
        sk_tile_xy(plan, nxt.tile, nbx, nby);
        if (BUF) {
          g_init_offs<AKC>(va, aop, nbx * 128, wave, lane);
          g_init_offs<BKC>(vb, bop, nby * 128, wave, lane);
        } else {
          g_init_ptrs<AKC>(qa, aop, nbx * 128, wave, lane);
          g_init_ptrs<BKC>(qb, bop, nby * 128, wave, lane);
        }
        offA = aStep * nxt.kb; offB = bStep * nxt.kb;
      }
      const uint32_t sOffA = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(offA * 4));
      const uint32_t sOffB = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(offB * 4));
      // 16 k-steps of 4 MFMAs; the 8 LDS-DMA pieces and the fragment reads of the next 8-k group are
      // slotted BETWEEN k-steps (one filler per gap, order pinned) so that their issue cost and latency
      // sit behind MFMA execution instead of in front of it.
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cur = g & 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][0][q], fb[cur][0][q], acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][0][q], fb[cur][1][q], acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][1][q], fb[cur][0][q], acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][1][q], fb[cur][1][q], acc[1][1], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          const int step = 4 * g + q;
          if (q == 0) {
            if (g < 3) {
              g_frag<AKC>(fa[cur ^ 1], As, wm, g + 1, li, lh);
              g_frag<BKC>(fb[cur ^ 1], Bs, wn, g + 1, li, lh);
            }
          } else {
            const int piece = step - 1 - g;  // steps 1,2,3,5,6,7,9,10 -> pieces 0..7
            if (BUF) {
              if (piece < 4) g_issue1_buf(ra, va[piece], sOffA, An, wave, piece);
              else if (piece < 8) g_issue1_buf(rb, vb[piece - 4], sOffB, An + 4096, wave, piece - 4);
            } else {
              if (piece < 4) g_issue1(qa[piece], offA, An, wave, piece);
              else if (piece < 8) g_issue1(qb[piece - 4], offB, An + 4096, wave, piece - 4);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      stage ^= 1;
      __syncthreads();  // the stage just filled has landed (vmcnt(0)) and is visible to all waves
    }

    bool doEpi = seg.slab < 0;  // whole tile: epilogue straight from the accumulators
    int resetTicket = -1;
    if (!doEpi) {
      gemm128_store_partial(plan.slabs + (size_t)seg.slab * kSlabFloats, acc);
      if (plan.counters) {
        // in-kernel slab reduction (g_slab_handover): the tile's last arriver adds its slabs in range order
        const int t = seg.tile - plan.dpTiles;
        int sF, sL;
        sk_tile_ranges(plan, t, sF, sL);
        if (g_slab_handover(plan.counters + t, (int*)(smem + (stage ^ 1) * kGStageFloats), sL - sF)) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
          for (int sr = sF; sr <= sL; ++sr) {
            const int segIdx = t - (int)(sk_begin(plan, sr) / plan.kTiles);  // ranges span <= 2 tiles: 0 or 1
            const f32x4* s4 = (const f32x4*)(plan.slabs + ((size_t)sr * 2 + segIdx) * kSlabFloats);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const f32x4 v = s4[((wave * 4 + i * 2 + j) * 4 + q) * 64 + lane];
                  acc[i][j][4 * q] += v[0]; acc[i][j][4 * q + 1] += v[1]; acc[i][j][4 * q + 2] += v[2]; acc[i][j][4 * q + 3] += v[3];
                }
          }
          doEpi = true;
          resetTicket = t;
        }
      }
    }
    if (doEpi) {
      // `stage` now names the buffer holding the prefetched next K tile; the other one is free
      if (wide) gemm128g_epilogue_wide(out, bx * 128, by * 128, acc, smem + (stage ^ 1) * kGStageFloats, bv);
      else gemm128_epilogue(out, bx * 128, by * 128, acc);
      if (resetTicket >= 0 && tid == 0) __hip_atomic_store(plan.counters + resetTicket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!nxt.valid) break;
    if (wide || plan.counters) __syncthreads();  // the next iteration's LDS-DMA lands in the slices the epilogue / ticket used

    seg = nxt;
    sk_tile_xy(plan, seg.tile, bx, by);
  }
}

inline int launch128g(const GOp& a, bool akc, const GOp& b, bool bkc, GemmOut o, int epi, hipStream_t s) {
  SkPlan plan = make_sk_plan(o.M, o.N, o.K, true);
  plan.grouped = 1;
  if (plan.skBlocks > 0) {
    plan.slabs = sk_scratch(s, kSkScratchBytes);
    if (!plan.slabs) { plan = make_sk_plan(o.M, o.N, o.K, false); plan.grouped = 1; }
    const char* eFix = tune_env("W2L_GEMM_INFIX");  // read per call (tests flip it): 0 = separate fix-up launch
    const int inFix = eFix ? atoi(eFix) : 1;
    if (plan.skBlocks > 0 && inFix && plan.skTiles <= 1024) plan.counters = sk_counters(s);
  }
  int workers = plan.dpTiles < kSkSlots ? plan.dpTiles : kSkSlots;
  if (workers < plan.skBlocks) workers = plan.skBlocks;
  const size_t shmem = 2 * (size_t)kGStageFloats * sizeof(float);
  dim3 grid((unsigned)workers), block(256);
  o.epi = epi;
  prof_begin(s, 2.0 * o.M * (double)o.N * o.K, PROF_GEMM128, o.M, o.N, o.K, 2);
  const int wide = (((uintptr_t)o.C) & 15) == 0 && o.ldc % 4 == 0 && (!o.mask || (((uintptr_t)o.mask) & 15) == 0);
  // buffer-addressed LDS-DMA wherever both operands are below 2 GiB (+8 % at 4096^3, +5-7 % on the TDS fc shapes over 64-bit
  // global addresses, MI355X); the global_load_lds instances take the (strictly aligned) operands beyond that
#define W2L_G128_GO(A, B, BUF) hipLaunchKernelGGL((gemm128g_kernel<A, B, BUF>), grid, block, shmem, s, a, b, o, plan, workers, wide)
  if (a.bytes && b.bytes) {
    if (akc && bkc) W2L_G128_GO(true, true, true);
    else if (akc) W2L_G128_GO(true, false, true);
    else if (bkc) W2L_G128_GO(false, true, true);
    else W2L_G128_GO(false, false, true);
  } else if (akc && bkc) W2L_G128_GO(true, true, false);
  else if (akc) W2L_G128_GO(true, false, false);
  else if (bkc) W2L_G128_GO(false, true, false);
  else W2L_G128_GO(false, false, false);
#undef W2L_G128_GO
  if (plan.skBlocks > 0 && !plan.counters)
    hipLaunchKernelGGL(gemm128_fixup, dim3((unsigned)plan.skTiles * 4), dim3(64), 0, s, o, plan);
  prof_end(s);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

}  // namespace w2l
