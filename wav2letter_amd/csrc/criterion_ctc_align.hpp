// criterion_ctc_align.hpp -- w2l_ctc_align: CTC forced alignment (the best lattice path of a known transcript).
// Included at the end of criterion_ctc.hip (one translation unit: the row pass and ctc_positions_per_lane are that file's).
//
// The max-plus twin of ctc_scan on the RAW emissions: a step is two fp32 compares and ONE fp32 add per lattice position, so the
// path is a pure function of fp32 compares and single adds and a numpy restatement reproduces it bit for bit, ties included
// (stay beats advance beats skip; a later candidate wins only when strictly greater: w2l_fac_viterbi's rule).
//   ctc_rows_lse_only  (score != NULL only) the ctc_rows_lse pass without the label probabilities: lse[b][t]
//   ctc_align_scan     one wavefront per utterance, ctc_positions_per_lane(L) positions per lane, the neighbour lane's two
//                      boundary positions by DPP.  Reads the L_b + 1 label emissions of a frame, nothing else of the row.  Writes
//                      2 back-pointer bits per (t, s), packed per lane into one word (32 bits for P <= 16, 64 for P = 32), and
//                      the end state (-1: infeasible, L_b + R > F).
//   ctc_align_walk     one wavefront per utterance: walks the back-pointers from the end state.  A chunk of kAlignWalkChunk frames
//                      is held in registers in the layout the scan wrote (lane l: its own words), the next chunk loading while
//                      this one is walked; the state is wave-uniform, so a step is a v_readlane and scalar arithmetic -- no memory
//                      or LDS round trip on the chain of F dependent steps.  Writes the STATE of every frame into path.
//   ctc_align_finish   one workgroup per utterance, frames in parallel: state -> label, the blank fill beyond F, -1 rows, and the
//                      path's log-probability sum_t (x[t][path_t] - lse_t) accumulated in double in a fixed order.
// Three kernels rather than one so that a kernel trace tells the scan from the walk.
#pragma once

namespace w2l {

constexpr int kAlignWalkChunk = 32;

template <int P> struct AlignWord { using type = std::conditional_t<(P <= 16), uint32_t, uint64_t>; };

struct CtcAlignWs {
  float* lse;   // [B][T]
  void* bp;     // [B][T][64] back-pointer words
  int* end;     // [B] end state of the best path, -1: infeasible
  int P;
};

__host__ __device__ inline size_t ctc_align_word_bytes(int P) { return P <= 16 ? 4 : 8; }

static CtcAlignWs ctc_align_ws(void* ws, int B, int T, int L) {
  CtcAlignWs w{};
  w.P = ctc_positions_per_lane(L);
  char* p = (char*)ws;
  w.lse = (float*)p; p += align_up((size_t)B * T * sizeof(float), 256);
  w.bp = (void*)p; p += align_up((size_t)B * T * 64 * ctc_align_word_bytes(w.P), 256);
  w.end = (int*)p;
  return w;
}

__device__ __forceinline__ float dpp_up_f32(float v, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

__device__ __forceinline__ int align_frames(const int* __restrict__ frames, int b, int T) {
  return frames ? min(max(frames[b], 1), T) : T;
}

// lse[b][t] alone (ctc_rows_lse_body's VAR 2 returns before the label probabilities: nothing else of CtcWs is touched)
__global__ __launch_bounds__(kRowThreads) void ctc_rows_lse_only(int T, int N, int L,
                                                                 const float* __restrict__ x,
                                                                 const int* __restrict__ target,
                                                                 const int* __restrict__ targetSize,
                                                                 CtcWs ws) {
  ctc_rows_lse_body<2, false>(T, N, L, x, target, targetSize, ws, nullptr);
}
__global__ __launch_bounds__(kRowThreads) void ctc_rows_lse_only_big(int T, int N, int L,
                                                                     const float* __restrict__ x,
                                                                     const int* __restrict__ target,
                                                                     const int* __restrict__ targetSize,
                                                                     CtcWs ws) {
  ctc_rows_lse_big_body<false, false>(T, N, L, x, target, targetSize, ws, nullptr);
}

// D frames of label emissions are prefetched a chunk ahead (ctc_scan's two-buffer scheme), a chunk's back-pointer words are stored
// behind the consumption of the prefetched values.
template <int P, int D>
__global__ __launch_bounds__(64) void ctc_align_scan(int T, int N, int L,
                                                     const float* __restrict__ x,
                                                     const int* __restrict__ target,
                                                     const int* __restrict__ targetSize,
                                                     const int* __restrict__ frames,
                                                     typename AlignWord<P>::type* __restrict__ bp,
                                                     int* __restrict__ end) {
  static_assert(P >= 2, "a lane's two lower neighbours must live in ONE neighbouring lane");
  using W = typename AlignWord<P>::type;
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int Lb = min(max(targetSize[b], 0), L);
  const int S = 2 * Lb + 1;
  const int F = align_frames(frames, b, T);
  const int* y = target + (size_t)b * L;
  const float* xb = x + (size_t)b * T * N;
  W* bpb = bp + (size_t)b * T * 64 + lane;

  int lab[P];     // column of the position's label (clamped into the row: a position beyond the lattice reads a valid float)
  bool skip[P];   // position s may be entered from s - 2
  int reps = 0;   // R: adjacent equal pairs of the target
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int si = lane * P + p;
    const int e0 = (si & 1) ? y[min(si >> 1, max(Lb, 1) - 1)] : (N - 1);
    lab[p] = min(max(e0, 0), N - 1);
    const bool odd3 = (si & 1) && si >= 3 && si < S;
    const int em2 = odd3 ? y[(si - 2) >> 1] : -2;
    skip[p] = odd3 && e0 != em2;
    reps += (odd3 && e0 == em2) ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) reps += __shfl_xor(reps, off);
  if (Lb + reps > F) {   // infeasible: no lattice path; ctc_align_finish writes the -1 row and the -inf score
    if (lane == 0) end[b] = -1;
    return;
  }

  auto loade = [&](float (&dst)[P], int k) {   // label emissions of frame k (a frame beyond F re-reads frame F - 1: no branch)
    const float* row = xb + (size_t)min(k, F - 1) * N;
#pragma unroll
    for (int p = 0; p < P; ++p) dst[p] = row[lab[p]];
  };

  float a[P];
  {
    float e0[P];
    loade(e0, 0);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int si = lane * P + p;
      a[p] = (si < 2 && si < S) ? e0[p] : -INFINITY;
    }
    bpb[0] = (W)0;   // frame 0 has no predecessor: the walk's step there stays
  }

  float ec[D][P], en[D][P];
#pragma unroll
  for (int u = 0; u < D; ++u) loade(ec[u], 1 + u);
#pragma unroll
  for (int u = 0; u < D; ++u)
#pragma unroll
    for (int p = 0; p < P; ++p) asm volatile("" : "+v"(ec[u][p]));   // landed before the loop (see ctc_scan_body)

  auto chunk = [&](float (&ec)[D][P], float (&en)[D][P], const int k0, auto checked) {
    constexpr bool CHECK = decltype(checked)::value;
#pragma unroll
    for (int u = 0; u < D; ++u) loade(en[u], k0 + D + u);
    W sw[D];
#pragma unroll
    for (int u = 0; u < D; ++u) {
      sw[u] = (W)0;
      if (!CHECK || k0 + u < F) {
        const float n1 = dpp_up_f32(a[P - 1], -INFINITY);   // lane - 1's last two positions
        const float n2 = dpp_up_f32(a[P - 2], -INFINITY);
        float na[P];
        W word = (W)0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
          const float adv = p >= 1 ? a[p >= 1 ? p - 1 : 0] : n1;
          const float sk = p >= 2 ? a[p >= 2 ? p - 2 : 0] : (p == 1 ? n1 : n2);
          float best = a[p];   // stay
          unsigned bits = 0;
          if (adv > best) { best = adv; bits = 1; }
          if (skip[p] && sk > best) { best = sk; bits = 2; }
          na[p] = best + ec[u][p];   // ONE fp32 add (the translation unit is compiled with -ffp-contract=off)
          word |= (W)bits << (2 * p);
        }
#pragma unroll
        for (int p = 0; p < P; ++p) a[p] = na[p];
        sw[u] = word;
      }
    }
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int p = 0; p < P; ++p) asm volatile("" : "+v"(en[u][p]));   // consumed BEFORE the chunk's stores are issued
#pragma unroll
    for (int u = 0; u < D; ++u)
      if (!CHECK || k0 + u < F) bpb[(size_t)(k0 + u) * 64] = sw[u];
  };
  int k0 = 1;
  for (; k0 + 3 * D <= F; k0 += 2 * D) {   // two chunks per trip, the two buffers swapping roles
    chunk(ec, en, k0, std::false_type{});
    chunk(en, ec, k0 + D, std::false_type{});
  }
  for (; k0 < F; k0 += D) {
    chunk(ec, en, k0, std::true_type{});
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int p = 0; p < P; ++p) ec[u][p] = en[u][p];
  }

  // end state S - 1, replaced by S - 2 only when strictly greater (the two may sit in two lanes)
  float m1 = -INFINITY, m2 = -INFINITY;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int si = lane * P + p;
    if (si == S - 1) m1 = a[p];
    if (si == S - 2) m2 = a[p];
  }
  const float v1 = __shfl(m1, (S - 1) / P);
  const float v2 = S >= 2 ? __shfl(m2, (S - 2) / P) : -INFINITY;
  if (lane == 0) end[b] = (S >= 2 && v2 > v1) ? S - 2 : S - 1;
}

template <int P>
__global__ __launch_bounds__(64) void ctc_align_walk(int T, const int* __restrict__ frames,
                                                     const typename AlignWord<P>::type* __restrict__ bp,
                                                     const int* __restrict__ end, int* __restrict__ path) {
  using W = typename AlignWord<P>::type;
  constexpr int C = kAlignWalkChunk;
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int F = align_frames(frames, b, T);
  int s = end[b];
  if (s < 0) return;
  s = __builtin_amdgcn_readfirstlane(s);   // wave-uniform: the walk below is scalar arithmetic and v_readlane
  const W* bpb = bp + (size_t)b * T * 64 + lane;
  int* pb = path + (size_t)b * T;
  W wc[C], wn[C];
  auto loadw = [&](W (&dst)[C], int t0) {   // words of frames t0, t0 - 1, ..: frames below 0 re-read frame 0 (word 0: a stay)
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c] = bpb[(size_t)max(t0 - c, 0) * 64];
  };
  loadw(wc, F - 1);
  for (int t0 = F - 1; t0 >= 0; t0 -= C) {
    loadw(wn, t0 - C);
    int st = 0;   // lane c: the state of frame t0 - c
#pragma unroll
    for (int c = 0; c < C; ++c) {
      st = lane == c ? s : st;
      const int ln = (int)((unsigned)s / (unsigned)P), pos = s - ln * P;
      unsigned bits;
      if constexpr (sizeof(W) == 8) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)wc[c], ln);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(wc[c] >> 32), ln);
        bits = (unsigned)((((uint64_t)hi << 32) | lo) >> (2 * pos)) & 3u;
      } else {
        bits = ((unsigned)__builtin_amdgcn_readlane((int)wc[c], ln) >> (2 * pos)) & 3u;
      }
      s = max(s - (int)bits, 0);
    }
    if (lane < C && t0 - lane >= 0) pb[t0 - lane] = st;
#pragma unroll
    for (int c = 0; c < C; ++c) wc[c] = wn[c];
  }
}

__global__ __launch_bounds__(kRowThreads) void ctc_align_finish(int T, int N, int L,
                                                                const float* __restrict__ x,
                                                                const int* __restrict__ target,
                                                                const int* __restrict__ frames,
                                                                const float* __restrict__ lse,
                                                                const int* __restrict__ end,
                                                                int* __restrict__ path, float* __restrict__ score) {
  __shared__ double smd[kRowThreads / 64];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int F = align_frames(frames, b, T);
  const int e = end[b];
  const int* y = target + (size_t)b * L;
  const float* xb = x + (size_t)b * T * N;
  int* pb = path + (size_t)b * T;
  double acc = 0.0;
  for (int t = tid; t < T; t += kRowThreads) {
    int out;
    if (e < 0) out = -1;
    else if (t >= F) out = N - 1;
    else {
      const int st = pb[t];
      out = (st & 1) ? min(max(y[min(st >> 1, L - 1)], 0), N - 1) : N - 1;
      if (score) acc += (double)xb[(size_t)t * N + out] - (double)lse[(size_t)b * T + t];
    }
    pb[t] = out;
  }
  if (!score) return;
  acc = wave_sum_f64(acc);
  if ((tid & 63) == 0) smd[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = smd[0];
#pragma unroll
    for (int w = 1; w < kRowThreads / 64; ++w) s += smd[w];
    score[b] = e < 0 ? -INFINITY : (float)s;
  }
}

}  // namespace w2l

W2L_API size_t w2l_ctc_align_workspace_size(int B, int T, int N, int L) {
  if (B <= 0 || T <= 0 || N <= 0 || L < 0) return 0;
  return w2l::align_up((size_t)B * T * sizeof(float), 256) +
         w2l::align_up((size_t)B * T * 64 * w2l::ctc_align_word_bytes(w2l::ctc_positions_per_lane(L)), 256) +
         w2l::align_up((size_t)B * sizeof(int), 256);
}

W2L_API int w2l_ctc_align(int B, int T, int N, int L, const float* input, const int* target, const int* targetSize,
                          const int* frames, int* path, float* score, void* workspace, w2l_stream_t stream) {
  using namespace w2l;
  if (B <= 0 || T <= 0 || N <= 1 || L <= 0 || !input || !target || !targetSize || !path || !workspace) return W2L_EINVAL;
  if (L > kCtcMaxLabels) return W2L_EUNSUPPORTED;   // as w2l_ctc_forward
  hipStream_t s = (hipStream_t)stream;
  const CtcAlignWs ws = ctc_align_ws(workspace, B, T, L);
  if (score) {   // the only read of whole rows; without score the call reads the label emissions alone
    CtcWs rw{};
    rw.lse = ws.lse;
    const unsigned rows = (unsigned)((size_t)B * T);
    if (N <= kRowThreads * kRowMaxPer)
      hipLaunchKernelGGL(ctc_rows_lse_only, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, rw);
    else
      hipLaunchKernelGGL(ctc_rows_lse_only_big, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, rw);
    W2L_LAUNCH_CHECK();
  }
  const dim3 grid((unsigned)B), blk(64);
#define W2L_ALIGN_CASE(P, D)                                                                                                  \
  case P:                                                                                                                     \
    hipLaunchKernelGGL((ctc_align_scan<P, D>), grid, blk, 0, s, T, N, L, input, target, targetSize, frames,                   \
                       (AlignWord<P>::type*)ws.bp, ws.end);                                                                   \
    W2L_LAUNCH_CHECK();                                                                                                       \
    hipLaunchKernelGGL((ctc_align_walk<P>), grid, blk, 0, s, T, frames, (const AlignWord<P>::type*)ws.bp, ws.end, path);      \
    break;
  switch (ws.P) {   // ctc_scan's (positions per lane, prefetch depth) pairs
    W2L_ALIGN_CASE(2, 16)
    W2L_ALIGN_CASE(3, 10)
    W2L_ALIGN_CASE(4, 8)
    W2L_ALIGN_CASE(5, 6)
    W2L_ALIGN_CASE(6, 5)
    W2L_ALIGN_CASE(8, 4)
    W2L_ALIGN_CASE(16, 2)
    default:
    W2L_ALIGN_CASE(32, 1)
  }
#undef W2L_ALIGN_CASE
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_align_finish, grid, dim3(kRowThreads), 0, s, T, N, L, input, target, frames, ws.lse, ws.end, path, score);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
