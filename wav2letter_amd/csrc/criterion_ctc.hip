// criterion_ctc.hip -- ConnectionistTemporalClassificationCriterion for gfx950.
//
// Replaces Flashlight's CTC criterion (CUDA build: warp-ctc; CPU build:
// flashlight/lib/sequence/criterion/cpu/ConnectionistTemporalClassificationCriterion.cpp,
// un-vendored).  Reference call sites: recipes/slimIPL/src/Train.cpp:406-407, :1675;
// blank is the LAST class (Train.cpp:248-251).  Math: SURVEY.md App. B.4; CPU
// restatement: oracle/criterion_oracle.c (== torch ctc_loss(blank=N-1)).
//
// At the north-star size (N = 9998 word pieces) the criterion is HBM-bound on
// streaming the [B][T][N] emissions, so it is split by access pattern:
//   ctc_rows_lse   one workgroup per (b,t) row: the row is read ONCE into
//                  registers (coalesced, 16 B/lane where alignment allows) and
//                  reduced to lse[b][t]; the <= 2L+1 label log-probs the lattice
//                  needs are gathered from the register-resident row's source.
//   ctc_scan       two wavefronts per utterance, side by side: the alpha scan and
//                  the beta scan over the 2L+1 extended labels in the scaled
//                  linear domain (fp64 mantissas, one power-of-two exponent per
//                  lattice position: no exp / log on the dependency chain); the
//                  alpha wave also writes the loss.
//   ctc_rows_grad  one workgroup per row: grad = g*(softmax(x) - occupancy):
//                  streams x once more, writes grad once, then subtracts the
//                  <= 2L+1 occupancies gamma[t][s] = exp(alpha+beta-lp-logZ) of
//                  that frame.
// Algorithmic HBM bytes: 4BTN (fwd) + 8BTN (bwd) = 12*B*T*N.
// w2l_ctc_align (forced alignment: the best lattice path of a known transcript) lives in criterion_ctc_align.hpp, included below.
// w2l_ctc_beam_search (lexicon-free n-best prefix beam search) lives in criterion_ctc_beam.hpp, included below with its siblings;
// the beam searches of the ASG lattice (criterion_asg_beam.hpp) come last, on the same helpers and scans.
// w2l_beam_session_* (the CTC searches continued chunk by chunk for streaming) lives in criterion_beam_stream.hpp.
// w2l_*_beam_search*_xl (the five searches with a beam of up to 8192 entries) lives in criterion_beam_xl.hpp, included before the
// sessions, whose many-token kind runs its kernels.
// w2l_ctc_score (evaluation: loss and greedy path, no gradient) reads the emissions once, 4BTN:
//   ctc_rows_score  the ctc_rows_lse pass (same arithmetic, template flag) that also writes the first-max argmax of the row
//   ctc_scan_score  the alpha wave alone, grid (B, 1), lattice rows kept in registers: only the loss is written
#include "common.hpp"

namespace w2l {

constexpr int kRowThreads = 256;
// ws.link[b][k] (ctc_label_links_k): the next label position with the same label (kLinkNone: none), | kLinkLater when an earlier
// position holds it too.  The entry points refuse L > kCtcMaxLabels, so a position fits below kLinkNone.
constexpr int kCtcMaxLabels = 1023;
constexpr int kLinkNone = 0xFFFF, kLinkLater = 1 << 16;
static_assert(2 * kCtcMaxLabels + 1 <= 64 * 32 && kCtcMaxLabels < kLinkNone, "label positions: lattice rows and link fields");
constexpr int kRowMaxPer = 48;  // register-resident row: N <= 256*48 = 12288

struct CtcWs {
  float* lse;     // [B][T]
  double* pd;     // [B][T][S]   exp(lp) in fp64, written by the row kernels through an integer / fraction split: a label
                  //             100+ nats below the row's normaliser keeps a finite probability (fp32 exp flushes below -87)
  double* alpha;  // [B][T][S]
  double* beta;   // [B][T][S]   (beta includes p_t(s), as alpha does)
  int* eA;        // [B][T][S]   power-of-two exponents of the alpha mantissas (one per lattice position)
  int* eB;        // [B][T][S]
  double* zhat;   // [B]  Z = zhat * 2^ez
  int* ez;        // [B]
  float* scale;   // [B]
  float* nll;     // [B]  (-log likelihood, unscaled)
  int* link;      // [B][L] repeated-label links of the targets (ctc_label_links_k, backward only)
  int S;          // row stride of the per-position arrays: 64 * P >= 2 L + 1
  int P;          // lattice positions per lane of the scans
};

__host__ __device__ inline int ctc_positions_per_lane(int L) {
  const int S = 2 * L + 1;
  // (a step of the scans costs instructions per position: no more positions per lane than the lattice needs)
  return S <= 128 ? 2 : S <= 192 ? 3 : S <= 256 ? 4 : S <= 320 ? 5 : S <= 384 ? 6 : S <= 512 ? 8 : S <= 1024 ? 16 : 32;
}

__host__ __device__ inline CtcWs ctc_ws(void* ws, int B, int T, int N, int L) {
  (void)N;
  CtcWs w;
  w.P = ctc_positions_per_lane(L);
  w.S = 64 * w.P;   // row stride of the per-position arrays: every lane's P positions lie inside a row (positions >= 2 L_b + 1 hold
                    // p = 0, written by the row kernels), rows are 16-byte aligned: the scans move whole lanes with vector accesses
  char* p = (char*)ws;
  w.lse = (float*)p; p += align_up((size_t)B * T * sizeof(float), 256);
  w.pd = (double*)p; p += align_up((size_t)B * T * w.S * sizeof(double), 256);
  w.alpha = (double*)p; p += align_up((size_t)B * T * w.S * sizeof(double), 256);
  w.beta = (double*)p; p += align_up((size_t)B * T * w.S * sizeof(double), 256);
  w.eA = (int*)p; p += align_up((size_t)B * T * w.S * sizeof(int), 256);
  w.eB = (int*)p; p += align_up((size_t)B * T * w.S * sizeof(int), 256);
  w.zhat = (double*)p; p += align_up((size_t)B * sizeof(double), 256);
  w.ez = (int*)p; p += align_up((size_t)B * sizeof(int), 256);
  w.scale = (float*)p; p += align_up((size_t)B * sizeof(float), 256);
  w.nll = (float*)p; p += align_up((size_t)B * sizeof(float), 256);
  w.link = (int*)p;
  return w;
}

// exp(lp) for lp <= ~0 over the whole fp64 range: 2^frac by the hardware fp32 exp2 (frac in [-0.5, 0.5]), the integer part by
// v_ldexp_f64.  __expf(lp) alone is 0 below -87 (-103 with denormals): one confident-wrong frame would make its lattice cells
// impossible, and with a tight alignment the whole likelihood 0 (loss +inf) where the log-domain reference stays finite.
__device__ __forceinline__ double exp_wide(float lp) {
  const float z = fmaxf(lp * 1.44269504088896341f, -1090.f);
  const float zi = __builtin_rintf(z);
  return __builtin_amdgcn_ldexp((double)__builtin_amdgcn_exp2f(z - zi), (int)zi);
}

__device__ __forceinline__ float block_reduce_max(float v, float* sm) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  float r = sm[0];
  for (int k = 1; k < (int)(blockDim.x >> 6); ++k) r = fmaxf(r, sm[k]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_reduce_sum(float v, float* sm) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  float r = sm[0];
  for (int k = 1; k < (int)(blockDim.x >> 6); ++k) r += sm[k];
  __syncthreads();
  return r;
}

// path[0] = the smallest cand of the workgroup (thread 0 stores)
__device__ __forceinline__ void block_argmin_store(int cand, int* out) {
  __shared__ int smi[kRowThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cand = min(cand, __shfl_xor(cand, off));
  if ((threadIdx.x & 63) == 0) smi[threadIdx.x >> 6] = cand;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = smi[0];
#pragma unroll
    for (int k = 1; k < kRowThreads / 64; ++k) c = min(c, smi[k]);
    *out = c;
  }
}

// Row loader: elements [0,N) of a row that is only 4-byte aligned. Thread tid owns
// element indices  head: tid (< nh);  body: nh + 4*(tid + 256*k) .. +3;  tail scalars.
// nh = number of leading scalars so that the body is 16-byte aligned.
struct RowSplit { int nh, nbody4, ntail; };
// mis: the floats by which the row begins past a 16-byte boundary
__device__ __forceinline__ RowSplit row_split_at(int mis, int N) {
  RowSplit r;
  r.nh = mis ? 4 - mis : 0;
  if (r.nh > N) r.nh = N;
  r.nbody4 = (N - r.nh) >> 2;
  r.ntail = (N - r.nh) & 3;
  return r;
}
__device__ __forceinline__ RowSplit row_split(const float* row, int N) { return row_split_at((int)(((uintptr_t)row >> 2) & 3), N); }

// lse[b][t] and the label probabilities pd[b][t][s] = exp(x[ext_s] - lse) in fp64
// VAR 3 (the product's form when L >= 1): the label gather of the first kRowThreads lattice positions -- target, then x[label] --
//   is issued WITH the row loads instead of behind the two reductions, where its two dependent round trips were 8 us of the
//   kernel's 68 (profiles/r05_run26_ctc_rows_lse_variants.log: variant 2 = no gather at all).
// VAR 0: the gather behind the reductions.  Probe library, W2L_CTC_LSE_VAR: 1 = nontemporal row loads (48 us, but ctc_rows_grad
//   then no longer finds the emissions in the Infinity Cache and takes the 20 us), 2 = no label gather (timing only)
// kArgmax (ctc_rows_score, w2l_ctc_score): the same pass also writes path[r], the first-max argmax of the row that
//   ctc_rows_argmax computes, from the register-resident row -- the arithmetic of lse and pd is the forward pass's own.
template <int VAR, bool kArgmax>
__device__ __forceinline__ void ctc_rows_lse_body(int T, int N, int L,
                                                  const float* __restrict__ x,
                                                  const int* __restrict__ target,
                                                  const int* __restrict__ targetSize,
                                                  const CtcWs& ws, int* __restrict__ path) {
  __shared__ float sm[8];
  const size_t r = blockIdx.x;  // row = b*T + t
  const int b = (int)(r / T);
  const float* row = x + r * N;
  const int tid = threadIdx.x;
  RowSplit sp = row_split(row, N);
  const float4* body = (const float4*)(row + sp.nh);
  const int Lb = targetSize[b];
  const int S = 2 * Lb + 1;
  const int* y = target + (size_t)b * L;
  int lab0 = 0;
  if (VAR == 3) lab0 = y[min(tid >> 1, max(Lb, 1) - 1)];   // (L >= 1)

  // Every load of the row is issued before the first use, none behind a lane predicate (a chunk past the row re-reads the
  // row's last chunk and is replaced by -inf): written as `if (idx < nbody4) { load; max }` hipcc waited for each of the
  // twelve loads in turn -- one 16-byte load in flight per thread, 3.4 TB/s (round-4 verdict, weak 8).
  float4 v[kRowMaxPer / 4];
  float hv = -INFINITY;
  if (sp.nbody4 > 0) {
    const int lastc = sp.nbody4 - 1;
#pragma unroll
    for (int k = 0; k < kRowMaxPer / 4; ++k) {
      const float4* q = body + min(tid + kRowThreads * k, lastc);
      if (VAR == 1) {
        const float* qf = (const float*)q;
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v t = __builtin_nontemporal_load((const f4v*)qf);
        v[k] = make_float4(t[0], t[1], t[2], t[3]);
      } else {
        v[k] = *q;
      }
    }
  }
  if (tid < sp.nh) hv = row[tid];
  else if (tid >= 64 && tid - 64 < sp.ntail) hv = row[sp.nh + 4 * sp.nbody4 + (tid - 64)];
  // (hipcc waits for the whole row here -- vmcnt(0) behind the branches above -- and the gather flies under the two reductions)
  float xl = 0.f;
  if (VAR == 3) xl = row[min(max((tid & 1) ? lab0 : N - 1, 0), N - 1)];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kRowMaxPer / 4; ++k) {
    if (tid + kRowThreads * k >= sp.nbody4) v[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    m = fmaxf(m, fmaxf(fmaxf(v[k].x, v[k].y), fmaxf(v[k].z, v[k].w)));
  }
  m = fmaxf(m, hv);
  m = block_reduce_max(m, sm);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kRowMaxPer / 4; ++k)
    s += (__expf(v[k].x - m) + __expf(v[k].y - m)) + (__expf(v[k].z - m) + __expf(v[k].w - m));   // exp(-inf - m) = 0: a chunk past the row
  if (hv != -INFINITY) s += __expf(hv - m);
  s = block_reduce_sum(s, sm);
  const float lse = m + __logf(s);
  if (tid == 0) ws.lse[r] = lse;
  if constexpr (kArgmax) {
    // smallest index holding the row's max (m: the same fmaxf reduction, NaN ignored; -inf past the row never matches, and an
    // all -inf row gets ctc_rows_argmax's 0x7fffffff)
    int cand = 0x7fffffff;
    if (m > -INFINITY) {
#pragma unroll
      for (int k = kRowMaxPer / 4 - 1; k >= 0; --k) {
        const int i0 = sp.nh + 4 * (tid + kRowThreads * k);
        if (v[k].w == m) cand = i0 + 3;
        if (v[k].z == m) cand = i0 + 2;
        if (v[k].y == m) cand = i0 + 1;
        if (v[k].x == m) cand = i0;
      }
      if (hv == m) cand = tid < sp.nh ? tid : min(cand, sp.nh + 4 * sp.nbody4 + (tid - 64));
    }
    block_argmin_store(cand, path + r);
  }
  if (VAR == 2) return;
  // label log-probs
  double* pd = ws.pd + r * ws.S;
  if (VAR == 3 && tid < S) pd[tid] = exp_wide(xl - lse);
  for (int si = VAR == 3 ? tid + kRowThreads : tid; si < S; si += kRowThreads) {
    int lab = (si & 1) ? y[si >> 1] : (N - 1);
    pd[si] = exp_wide(row[lab] - lse);
  }
  for (int si = S + tid; si < ws.S; si += kRowThreads) pd[si] = 0.0;   // positions beyond the utterance's lattice: p = 0
}

template <int VAR>
__global__ __launch_bounds__(kRowThreads) void ctc_rows_lse(int T, int N, int L,
                                                            const float* __restrict__ x,
                                                            const int* __restrict__ target,
                                                            const int* __restrict__ targetSize,
                                                            CtcWs ws) {
  ctc_rows_lse_body<VAR, false>(T, N, L, x, target, targetSize, ws, nullptr);
}

// generic-N fallback (N > 256*kRowMaxPer): two passes over the row.  kArgmax: the first pass also keeps each thread's
// first max and its index (ctc_rows_argmax's loop), so the argmax costs no third pass.  kPd = false (w2l_ctc_align): lse alone
template <bool kArgmax, bool kPd = true>
__device__ __forceinline__ void ctc_rows_lse_big_body(int T, int N, int L,
                                                      const float* __restrict__ x,
                                                      const int* __restrict__ target,
                                                      const int* __restrict__ targetSize,
                                                      const CtcWs& ws, int* __restrict__ path) {
  __shared__ float sm[8];
  const size_t r = blockIdx.x;
  const int b = (int)(r / T);
  const float* row = x + r * N;
  const int tid = threadIdx.x;
  float m = -INFINITY;
  float best = -INFINITY;
  int arg = 0x7fffffff;
  for (int n = tid; n < N; n += kRowThreads) {
    const float v = row[n];
    m = fmaxf(m, v);
    if (kArgmax && v > best) { best = v; arg = n; }   // ascending n per thread: first max kept
  }
  m = block_reduce_max(m, sm);
  if constexpr (kArgmax) block_argmin_store(best == m ? arg : 0x7fffffff, path + r);
  float s = 0.f;
  for (int n = tid; n < N; n += kRowThreads) s += __expf(row[n] - m);
  s = block_reduce_sum(s, sm);
  const float lse = m + __logf(s);
  if (tid == 0) ws.lse[r] = lse;
  if constexpr (!kPd) return;
  const int Lb = targetSize[b];
  const int S = 2 * Lb + 1;
  const int* y = target + (size_t)b * L;
  double* pd = ws.pd + r * ws.S;
  for (int si = tid; si < S; si += kRowThreads) {
    int lab = (si & 1) ? y[si >> 1] : (N - 1);
    pd[si] = exp_wide(row[lab] - lse);
  }
  for (int si = S + tid; si < ws.S; si += kRowThreads) pd[si] = 0.0;   // positions beyond the utterance's lattice: p = 0
}

__global__ __launch_bounds__(kRowThreads) void ctc_rows_lse_big(int T, int N, int L,
                                                                const float* __restrict__ x,
                                                                const int* __restrict__ target,
                                                                const int* __restrict__ targetSize,
                                                                CtcWs ws) {
  ctc_rows_lse_big_body<false>(T, N, L, x, target, targetSize, ws, nullptr);
}

// w2l_ctc_score's row pass: lse, the label probabilities and the argmax from one read of the row
__global__ __launch_bounds__(kRowThreads) void ctc_rows_score(int T, int N, int L,
                                                              const float* __restrict__ x,
                                                              const int* __restrict__ target,
                                                              const int* __restrict__ targetSize,
                                                              CtcWs ws, int* __restrict__ path) {
  ctc_rows_lse_body<3, true>(T, N, L, x, target, targetSize, ws, path);
}
__global__ __launch_bounds__(kRowThreads) void ctc_rows_score_big(int T, int N, int L,
                                                                  const float* __restrict__ x,
                                                                  const int* __restrict__ target,
                                                                  const int* __restrict__ targetSize,
                                                                  CtcWs ws, int* __restrict__ path) {
  ctc_rows_lse_big_body<true>(T, N, L, x, target, targetSize, ws, path);
}

// ---- alpha / beta lattice scans in the SCALED LINEAR domain -----------------------------------------------------------
// alpha_t(s) = (alpha_{t-1}(s) + alpha_{t-1}(s-1) + [skip] alpha_{t-1}(s-2)) * p_t(s) in fp64, every lattice POSITION carrying its
// own power-of-two exponent (value = mantissa * 2^e, mantissa in [0.5, 1) after every step).  Against the log-domain recursion this
//   * takes the transcendentals OFF the dependency chain: p_t(s) = exp(lp) comes as an fp64 value from the row kernel (exp_wide:
//     no underflow); a step is three v_ldexp_f64, two adds, one multiply and a v_frexp pair per position -- no exp / log;
//   * removes the accumulated rounding of T dependent fp32 log-sum-exp corrections: sums and products are fp64;
//   * keeps the log domain's dynamic range: the three inputs of a position are brought to their largest exponent with
//     v_ldexp_f64 -- a contribution 2^-1074 below the largest of the three is lost, nothing else.
// Round 4: one exponent per POSITION instead of one per lane (round 3).  A wave that is alone on its SIMD issues one instruction
// every ~6.5 cycles (tools/micro/clock_probe.hip), and the per-lane-exponent step -- align the neighbour lane, align the own
// positions, renormalise the lane -- was ~155 instructions at two positions per lane (0.43 us per frame); this one is ~45.
// One wavefront per (utterance, direction): blockIdx.y = 0 alpha, 1 beta; lane l owns positions l P .. l P + P - 1; the two
// lower (alpha) / upper (beta) neighbours of a lane's first / last position come by DPP from the neighbouring lane.
// Stored per position: mantissa (fp64) and exponent of alpha and of beta; both scans include p_t(s), so the occupancy is
// gamma_t(s) = alpha^ beta^ / (p z^) * 2^(eA + eB - ez), taken in ctc_rows_grad.  Rows are stored a chunk of D steps at a time,
// BEHIND the consumption of the prefetched p values (a store in flight in front of a loaded register's first use makes hipcc
// wait for its round trip).
__device__ __forceinline__ int dpp_up_i32(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int dpp_down_i32(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false); }
constexpr int kCtcNoExp = -(1 << 28);   // exponent of a position that holds no mass

// The direction is a TEMPLATE parameter and the chunk loop has a check-free main part: with `isBeta` a run-time value and
// `k < T` tested per step and per load, hipcc kept uniform branches and register copies around every step -- ~125 instructions per
// frame at P = 3 for ~50 of arithmetic (ISA), on a wave that issues one instruction every ~6.5 cycles.
// kScore (w2l_ctc_score): the alpha recursion alone, nothing stored but the loss -- the lattice rows live in registers only.
template <int P, int D, bool isBeta, bool kScore = false>
__device__ __forceinline__ void ctc_scan_body(int T, int N, int L, int scaleMode,
                                              const int* __restrict__ target,
                                              const int* __restrict__ targetSize,
                                              float* __restrict__ loss, const CtcWs& ws) {
  static_assert(P >= 2, "a lane's two lower / upper neighbours must live in ONE neighbouring lane");
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int Lb = targetSize[b];
  const int S = 2 * Lb + 1;
  const int SW = ws.S;
  const int* y = target + (size_t)b * L;
  const double* pd = ws.pd + (size_t)b * T * SW;
  static_assert(!(kScore && isBeta), "the score pass has no beta scan");
  double* lat = kScore ? nullptr : (isBeta ? ws.beta : ws.alpha) + (size_t)b * T * SW;
  int* lex = kScore ? nullptr : (isBeta ? ws.eB : ws.eA) + (size_t)b * T * SW;

  bool skip[P];   // alpha: position s may be entered from s - 2; beta: position s may go to s + 2
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int si = lane * P + p;
    const int e0 = (si & 1) ? ((si >> 1) < Lb ? y[si >> 1] : -1) : (N - 1);
    if (!isBeta) {
      const int em2 = (si >= 2 && (si & 1) && ((si - 2) >> 1) < Lb) ? y[(si - 2) >> 1] : -2;
      skip[p] = (si < S) && (si & 1) && si >= 2 && e0 != em2;
    } else {
      const int ep2 = ((si & 1) && si + 2 < S) ? y[(si + 2) >> 1] : -2;
      skip[p] = (si < S) && (si & 1) && si + 2 < S && e0 != ep2;
    }
  }
  // frame order of this scan: alpha walks t = 0 .. T-1, beta t = T-1 .. 0.  Every lane moves its P consecutive positions of a
  // row with 16-byte vector accesses (rows are 64 P positions wide: no bounds, p = 0 beyond the lattice), and the row addresses
  // advance by a constant stride per step -- the per-access index arithmetic was a third of the step's instructions
  typedef double d2_t __attribute__((ext_vector_type(2)));
  typedef int i2_t __attribute__((ext_vector_type(2)));
  const long rstride = isBeta ? -(long)SW : (long)SW;
  const long row0 = (long)(isBeta ? T - 1 : 0) * SW + (long)lane * P;
  const d2_t* pdp = (const d2_t*)(pd + row0);   // p of step k at pdp + k * rstride (in doubles: / 2 vectors)
  d2_t* latp = kScore ? nullptr : (d2_t*)(lat + row0);
  i2_t* lexp = kScore ? nullptr : (i2_t*)(lex + row0);
  auto loadp = [&](double (&dst)[P], int k, auto checked) {   // checked: std::true_type = step k may lie beyond the last frame
    constexpr bool CHECK = decltype(checked)::value;
    const double* q1 = (const double*)pdp + (long)k * rstride;
    if constexpr (P % 2 == 0) {
      const d2_t* q = (const d2_t*)q1;
#pragma unroll
      for (int p = 0; p < P; p += 2) { const d2_t v = (!CHECK || k < T) ? q[p / 2] : d2_t{0.0, 0.0}; dst[p] = v[0]; dst[p + 1] = v[1]; }
    } else {   // odd P: a lane's positions are 8-byte aligned only
#pragma unroll
      for (int p = 0; p < P; ++p) dst[p] = (!CHECK || k < T) ? q1[p] : 0.0;
    }
  };
  auto storerow = [&](const double (&mv)[P], const int (&ev)[P], int k) {
    double* q1 = (double*)latp + (long)k * rstride;
    int* qe1 = (int*)lexp + (long)k * rstride;
    if constexpr (P % 2 == 0) {
      d2_t* q = (d2_t*)q1;
      i2_t* qe = (i2_t*)qe1;
#pragma unroll
      for (int p = 0; p < P; p += 2) { q[p / 2] = d2_t{mv[p], mv[p + 1]}; qe[p / 2] = i2_t{ev[p], ev[p + 1]}; }
    } else {
#pragma unroll
      for (int p = 0; p < P; ++p) { q1[p] = mv[p]; qe1[p] = ev[p]; }
    }
  };

  // ---- first frame: alpha_0(s) = p_0(s) for s < 2; beta_{T-1}(s) = p_{T-1}(s) for s >= S - 2
  double m[P];
  int e[P];
  {
    double p0[P];
    loadp(p0, 0, std::false_type{});
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int si = lane * P + p;
      const bool on = si < S && (isBeta ? si >= S - 2 : si < 2);
      const double h = on ? p0[p] : 0.0;
      m[p] = __builtin_amdgcn_frexp_mant(h);
      e[p] = h > 0.0 ? __builtin_amdgcn_frexp_exp(h) : kCtcNoExp;
    }
    if constexpr (!kScore) storerow(m, e, 0);
  }

  double pc[D][P], pn[D][P];   // p of steps k0 .. k0 + D - 1 (current chunk) and of the next chunk
#pragma unroll
  for (int u = 0; u < D; ++u) loadp(pc[u], 1 + u, std::true_type{});
#pragma unroll
  for (int u = 0; u < D; ++u)
#pragma unroll
    for (int p = 0; p < P; ++p) asm volatile("" : "+v"(pc[u][p]));   // landed before the loop: no load pending at its head (a pending load
                                                                     // there makes hipcc wait vmcnt(0) at every step's first use)
  // steps k0 .. k0 + D - 1 on the p values in pc, the next chunk's p into pn; checked = std::false_type: this chunk AND the next lie inside T
  auto chunk = [&](double (&pc)[D][P], double (&pn)[D][P], const int k0, auto checked) {
    constexpr bool CHECK = decltype(checked)::value;
#pragma unroll
    for (int u = 0; u < D; ++u) loadp(pn[u], k0 + D + u, checked);
    double sm[D][P];   // this chunk's rows: stored after the chunk
    int se[D][P];
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int k = k0 + u;
#pragma unroll
      for (int p = 0; p < P; ++p) { sm[u][p] = 0.0; se[u][p] = kCtcNoExp; }
      if (!CHECK || k < T) {
        // the neighbour lane's two boundary positions (alpha: lane - 1's last two; beta: lane + 1's first two)
        double n1m, n2m;
        int n1e, n2e;
        if (!isBeta) {
          n1m = lane_shift_up_dpp(m[P - 1], 0.0); n1e = dpp_up_i32(e[P - 1], kCtcNoExp);
          n2m = lane_shift_up_dpp(m[P - 2], 0.0); n2e = dpp_up_i32(e[P - 2], kCtcNoExp);
        } else {
          n1m = lane_shift_down_dpp(m[0], 0.0); n1e = dpp_down_i32(e[0], kCtcNoExp);
          n2m = lane_shift_down_dpp(m[1], 0.0); n2e = dpp_down_i32(e[1], kCtcNoExp);
        }
        double nm[P];
        int ne[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
          double m1, m2;   // the position one / two steps towards the neighbour lane
          int e1, e2;
          if (!isBeta) {
            m1 = p >= 1 ? m[p >= 1 ? p - 1 : 0] : n1m;                       e1 = p >= 1 ? e[p >= 1 ? p - 1 : 0] : n1e;
            m2 = p >= 2 ? m[p >= 2 ? p - 2 : 0] : (p == 1 ? n1m : n2m);      e2 = p >= 2 ? e[p >= 2 ? p - 2 : 0] : (p == 1 ? n1e : n2e);
          } else {
            m1 = p + 1 < P ? m[p + 1 < P ? p + 1 : 0] : n1m;                 e1 = p + 1 < P ? e[p + 1 < P ? p + 1 : 0] : n1e;
            m2 = p + 2 < P ? m[p + 2 < P ? p + 2 : 0] : (p + 1 < P ? n1m : n2m);
            e2 = p + 2 < P ? e[p + 2 < P ? p + 2 : 0] : (p + 1 < P ? n1e : n2e);
          }
          // not enterable from two positions away: the term must shift out to exactly 0 -- also when NOTHING else feeds the position
          // (E = kCtcNoExp): with e2 = kCtcNoExp the shift would be 0 there and the position would inherit a ghost mass of
          // 2^-2^28 from a place it cannot be reached from (harmless next to real mass, but an infeasible target's likelihood
          // came out as 2^-2^28 instead of 0: loss 1.9e8 where the reference's is +inf; oracle/ctc_linear_domain.py)
          if (!skip[p]) e2 = kCtcNoExp - 4096;
          const int E = max(max(e[p], e1), e2);
          const double sum = (__builtin_amdgcn_ldexp(m[p], e[p] - E) + __builtin_amdgcn_ldexp(m1, e1 - E)) + __builtin_amdgcn_ldexp(m2, e2 - E);
          const double h = sum * pc[u][p];     // p = 0 beyond S: stays zero
          nm[p] = __builtin_amdgcn_frexp_mant(h);
          ne[p] = h > 0.0 ? E + __builtin_amdgcn_frexp_exp(h) : kCtcNoExp;
        }
#pragma unroll
        for (int p = 0; p < P; ++p) { m[p] = nm[p]; e[p] = ne[p]; sm[u][p] = nm[p]; se[u][p] = ne[p]; }
      }
    }
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int p = 0; p < P; ++p) asm volatile("" : "+v"(pn[u][p]));   // consumed BEFORE the chunk's stores are issued
    if constexpr (!kScore) {
#pragma unroll
      for (int u = 0; u < D; ++u)
        if (!CHECK || k0 + u < T) storerow(sm[u], se[u], k0 + u);
    }
  };
  int k0 = 1;
  for (; k0 + 3 * D <= T; k0 += 2 * D) {   // two chunks per trip, the two p buffers swapping roles: no D P register copies per chunk
    chunk(pc, pn, k0, std::false_type{});
    chunk(pn, pc, k0 + D, std::false_type{});
  }
  for (; k0 < T; k0 += D) {
    chunk(pc, pn, k0, std::true_type{});
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int p = 0; p < P; ++p) pc[u][p] = pn[u][p];
  }
  if constexpr (isBeta) return;

  // ---- likelihood Z = alpha_{T-1}(S-1) + alpha_{T-1}(S-2) = zhat * 2^ez (the two positions may sit in two lanes)
  int ez = kCtcNoExp;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int si = lane * P + p;
    if ((si == S - 1 || si == S - 2) && m[p] > 0.0) ez = max(ez, e[p]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(ez, off); ez = o > ez ? o : ez; }
  double zs = 0.0;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int si = lane * P + p;
    if ((si == S - 1 || si == S - 2) && m[p] > 0.0) zs += __builtin_amdgcn_ldexp(m[p], e[p] - ez);
  }
  zs = wave_sum_f64(zs);
  if (lane == 0) {
    const float sc = scale_of(scaleMode, T, Lb);
    double ll = -INFINITY;
    if (zs > 0.0) ll = log(zs) + (double)ez * 0.69314718055994530942;
    loss[b] = (float)(-(double)sc * ll);
    if constexpr (kScore) return;
    ws.scale[b] = sc;
    ws.nll[b] = (float)(-ll);
    ws.zhat[b] = zs;
    ws.ez[b] = ez;
  }
}

template <int P, int D>
__global__ __launch_bounds__(64) void ctc_scan(int T, int N, int L, int scaleMode,
                                               const int* __restrict__ target,
                                               const int* __restrict__ targetSize,
                                               float* __restrict__ loss, CtcWs ws) {
  if (blockIdx.y == 1) ctc_scan_body<P, D, true>(T, N, L, scaleMode, target, targetSize, loss, ws);
  else ctc_scan_body<P, D, false>(T, N, L, scaleMode, target, targetSize, loss, ws);
}

// w2l_ctc_score: the alpha wave alone, grid (B, 1)
template <int P, int D>
__global__ __launch_bounds__(64) void ctc_scan_score(int T, int N, int L, int scaleMode,
                                                     const int* __restrict__ target,
                                                     const int* __restrict__ targetSize,
                                                     float* __restrict__ loss, CtcWs ws) {
  ctc_scan_body<P, D, false, true>(T, N, L, scaleMode, target, targetSize, loss, ws);
}

// link[b][k] for k < L_b: the next position with the same label (kLinkNone: none), | kLinkLater when an earlier position holds
// it.  One workgroup per utterance, once per backward call: the O(L^2) comparison is not repeated for every frame.
__global__ __launch_bounds__(kRowThreads) void ctc_label_links_k(int L, const int* __restrict__ target,
                                                                 const int* __restrict__ targetSize, int* __restrict__ link) {
  const int b = blockIdx.x;
  const int Lb = targetSize[b];
  const int* y = target + (size_t)b * L;
  for (int k = threadIdx.x; k < Lb; k += kRowThreads) {
    const int lab = y[k];
    int next = kLinkNone, later = 0;
    for (int j = Lb - 1; j > k; --j) next = y[j] == lab ? j : next;
    for (int j = 0; j < k; ++j) later |= y[j] == lab;
    link[(size_t)b * L + k] = next | (later ? kLinkLater : 0);
  }
}

// grad row = g * softmax(x); then subtract g * gamma at the frame's labels
__global__ __launch_bounds__(kRowThreads) void ctc_rows_grad(int T, int N, int L,
                                                             const float* __restrict__ x,
                                                             const int* __restrict__ target,
                                                             const int* __restrict__ targetSize,
                                                             const float* __restrict__ grad,
                                                             float* __restrict__ dx, CtcWs ws) {
  const size_t r = blockIdx.x;
  const int b = (int)(r / T);
  const float* row = x + r * N;
  float* out = dx + r * N;
  const int tid = threadIdx.x;
  const float g = ws.scale[b] * grad[b];
  const float lse = ws.lse[r];
  RowSplit sp = row_split(row, N);  // dx has the same alignment as x modulo 16 B iff bases agree
  const bool same = ((((uintptr_t)row) ^ ((uintptr_t)out)) & 15) == 0;
  if (same && N <= kRowThreads * kRowMaxPer && sp.nbody4 >= 1) {
    // Every load of the row issued before the first use, as ctc_rows_lse does, and LANDED at one unconditional point before the
    // first store: on gfx9 stores count in vmcnt too, and wherever a load was still pending on some path hipcc put
    // `s_waitcnt vmcnt(0)` in front of the next use -- behind a store that meant waiting for the store's round trip (the rolled
    // loop below: one load in flight per wave, every load behind the previous store; 4.3 TB/s read + written where the forward
    // pass reads at 5.9).  Loads are unconditional (idle lanes re-read the row's first vector) so that no branch separates them.
    const float4* body = (const float4*)(row + sp.nh);
    float4* obody = (float4*)(out + sp.nh);
    float4 v[kRowMaxPer / 4];
#pragma unroll
    for (int k = 0; k < kRowMaxPer / 4; ++k) {
      const int idx = tid + kRowThreads * k;
      v[k] = body[idx < sp.nbody4 ? idx : 0];
    }
    int hn = 0;   // head / tail scalar of this thread (element 0 for the threads that own none: a harmless read)
    bool hasH = false;
    if (tid < sp.nh) { hn = tid; hasH = true; }
    else if (tid >= 64 && tid - 64 < sp.ntail) { hn = sp.nh + 4 * sp.nbody4 + (tid - 64); hasH = true; }
    float hv = row[hn];
#pragma unroll
    for (int k = 0; k < kRowMaxPer / 4; ++k)
      asm volatile("" : "+v"(v[k].x), "+v"(v[k].y), "+v"(v[k].z), "+v"(v[k].w));
    asm volatile("" : "+v"(hv));
#pragma unroll
    for (int k = 0; k < kRowMaxPer / 4; ++k) {
      const int idx = tid + kRowThreads * k;
      if (idx < sp.nbody4) {
        float4 o = v[k];
        o.x = g * __expf(o.x - lse); o.y = g * __expf(o.y - lse);
        o.z = g * __expf(o.z - lse); o.w = g * __expf(o.w - lse);
        obody[idx] = o;
      }
    }
    if (hasH) out[hn] = g * __expf(hv - lse);
  } else if (same) {
    const float4* body = (const float4*)(row + sp.nh);
    float4* obody = (float4*)(out + sp.nh);
    for (int idx = tid; idx < sp.nbody4; idx += kRowThreads) {
      float4 v = body[idx];
      v.x = g * __expf(v.x - lse); v.y = g * __expf(v.y - lse);
      v.z = g * __expf(v.z - lse); v.w = g * __expf(v.w - lse);
      obody[idx] = v;
    }
    if (tid < sp.nh) out[tid] = g * __expf(row[tid] - lse);
    else if (tid >= 64 && tid - 64 < sp.ntail) {
      int n = sp.nh + 4 * sp.nbody4 + (tid - 64);
      out[n] = g * __expf(row[n] - lse);
    }
  } else {
    for (int n = tid; n < N; n += kRowThreads) out[n] = g * __expf(row[n] - lse);
  }
  __syncthreads();  // drains the row stores (vmcnt(0)) before the label fix-up
  const int Lb = targetSize[b];
  const int S = 2 * Lb + 1;
  const int* y = target + (size_t)b * L;
  // occupancy of label position s at this frame: alpha beta / (p Z) = alpha^ beta^ / (p zhat) * 2^(eA + eB - ez)
  // (alpha and beta both carry p_t(s); p is the SAME fp64 value pd[t][s] the scans multiplied by)
  const double* pdr = ws.pd + r * ws.S;
  const double* alr = ws.alpha + r * ws.S;
  const double* ber = ws.beta + r * ws.S;
  const int* ear = ws.eA + r * ws.S;
  const int* ebr = ws.eB + r * ws.S;
  const double zh = ws.zhat[b];
  if (zh > 0.0) {   // an infeasible target (Z = 0) has no occupancy: its loss is +inf, its gradient g * softmax (zh: row-uniform)
    const int ez = ws.ez[b];
    auto occ = [&](int si) -> float {
      const double av = alr[si], bv = ber[si];
      if (!(av > 0.0 && bv > 0.0)) return 0.f;
      return (float)ldexp(av * bv / (pdr[si] * zh), ear[si] + ebr[si] - ez);
    };
    // Several positions share a column (every even one the blank's, a repeated label its own): they are added in a FIXED
    // order, not by atomics, so that the gradient -- and the training run it drives -- repeats bit for bit.  Blank: per-thread
    // sums in ascending position, a fixed-shape wave tree, the waves in index order.  Label: the thread of its first
    // position adds all of its positions in ascending order; the others skip it.
    // Every position's occupancy is formed in parallel; the label positions' values and their links (ctc_label_links_k, per
    // utterance) go to LDS, where the thread of a label's first position then walks its chain: O(L) per row.
    __shared__ float lv[kCtcMaxLabels];
    __shared__ int ll[kCtcMaxLabels];
    const int* lnk = ws.link + (size_t)b * L;
    float blank = 0.f;
    for (int si = tid; si < S; si += kRowThreads) {
      const int k = si >> 1;
      const int lab = (si & 1) ? y[k] : (N - 1);
      const float v = occ(si);
      if (lab == N - 1) {
        if (v != 0.f) blank += -g * v;
        continue;
      }
      lv[k] = v;
      ll[k] = lnk[k];
    }
    __syncthreads();
    for (int k = tid; k < Lb; k += kRowThreads) {
      int lk = ll[k];
      const int lab = y[k];
      if ((lk & kLinkLater) || lab == N - 1) continue;
      float acc = out[lab];
      for (int j = k;;) {
        const float v = lv[j];
        if (v != 0.f) acc += -g * v;
        if ((lk & kLinkNone) == kLinkNone) break;
        j = lk & kLinkNone;
        lk = ll[j];
      }
      out[lab] = acc;
    }
    __shared__ float smb[kRowThreads / 64];
    blank = wave_sum(blank);
    if ((tid & 63) == 0) smb[tid >> 6] = blank;
    __syncthreads();
    if (tid == 0) {
      float s = smb[0];
#pragma unroll
      for (int w = 1; w < kRowThreads / 64; ++w) s += smb[w];
      out[N - 1] += s;
    }
  }
}

__global__ __launch_bounds__(kRowThreads) void ctc_rows_argmax(int N, const float* __restrict__ x,
                                                               int* __restrict__ path) {
  __shared__ float smv[4];
  __shared__ int smi[4];
  const size_t r = blockIdx.x;
  const float* row = x + r * N;
  const int tid = threadIdx.x;
  float best = -INFINITY;
  int arg = 0x7fffffff;
  for (int n = tid; n < N; n += kRowThreads) {
    float v = row[n];
    if (v > best) { best = v; arg = n; }  // ascending n per thread: first max kept
  }
  // wave: max value, then smallest index among lanes holding it
  float m = wave_max(best);
  int cand = (best == m) ? arg : 0x7fffffff;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cand = min(cand, __shfl_xor(cand, off));
  if ((tid & 63) == 0) { smv[tid >> 6] = m; smi[tid >> 6] = cand; }
  __syncthreads();
  if (tid == 0) {
    float bm = smv[0];
    int bi = smi[0];
    for (int k = 1; k < kRowThreads / 64; ++k) {
      if (smv[k] > bm || (smv[k] == bm && smi[k] < bi)) { bm = smv[k]; bi = smi[k]; }
    }
    path[r] = bi;
  }
}

// one wavefront per utterance (a thread per utterance walked the L labels with dependent, uncoalesced loads: 49 us at
// L = 300 in front of every criterion call -- profiles/r02_run16_asg_timeline.log)
__global__ __launch_bounds__(64) void batch_target_size_k(int B, int L, int maxSize, const int* __restrict__ target,
                                                          int* __restrict__ targetSize, int ctc) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const int* y = target + (size_t)b * L;
  int first = L;   // index of the first negative label
  for (int i = lane; i < L; i += 64)
    if (y[i] < 0) { first = i; break; }
  for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off));
  const int n = first;
  if (!ctc) {
    if (lane == 0) targetSize[b] = n < maxSize ? n : maxSize;
    return;
  }
  int R = 0;
  for (int i = 1 + lane; i < n; i += 64) R += (y[i] == y[i - 1]);
  for (int off = 32; off > 0; off >>= 1) R += __shfl_xor(R, off);
  if (lane == 0) {
    const int m = (n + R < maxSize ? n + R : maxSize) - R;
    targetSize[b] = m < 0 ? 0 : m;
  }
}

}  // namespace w2l

using namespace w2l;

W2L_API int w2l_batch_target_size(int B, int L, int maxSize, const int* target, int* targetSize,
                                  w2l_stream_t stream) {
  if (B <= 0 || L <= 0 || !target || !targetSize) return W2L_EINVAL;
  hipLaunchKernelGGL(batch_target_size_k, dim3(B), dim3(64), 0, (hipStream_t)stream, B, L, maxSize, target, targetSize, 0);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_batch_ctc_target_size(int B, int L, int T, const int* target, int* targetSize,
                                      w2l_stream_t stream) {
  if (B <= 0 || L <= 0 || !target || !targetSize) return W2L_EINVAL;
  hipLaunchKernelGGL(batch_target_size_k, dim3(B), dim3(64), 0, (hipStream_t)stream, B, L, T, target, targetSize, 1);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API size_t w2l_ctc_workspace_size(int B, int T, int N, int L) {
  if (B <= 0 || T <= 0 || N <= 0 || L < 0) return 0;
  size_t S = 64 * (size_t)ctc_positions_per_lane(L);
  return align_up((size_t)B * T * sizeof(float), 256) +
         3 * align_up((size_t)B * T * S * sizeof(double), 256) + 2 * align_up((size_t)B * T * S * sizeof(int), 256) +
         align_up((size_t)B * sizeof(double), 256) + align_up((size_t)B * sizeof(int), 256) + 2 * align_up((size_t)B * sizeof(float), 256) +
         align_up((size_t)B * L * sizeof(int), 256);
}

W2L_API int w2l_ctc_forward(int B, int T, int N, int L, int scaleMode, const float* input,
                            const int* target, const int* targetSize, float* loss,
                            void* workspace, w2l_stream_t stream) {
  if (B <= 0 || T <= 0 || N <= 1 || L <= 0 || !input || !target || !targetSize || !loss || !workspace)
    return W2L_EINVAL;
  if (L > kCtcMaxLabels) return W2L_EUNSUPPORTED;   // L <= 1023 label positions per utterance (2 L + 1 <= 32 per lane)
  hipStream_t s = (hipStream_t)stream;
  CtcWs ws = ctc_ws(workspace, B, T, N, L);
  const unsigned rows = (unsigned)((size_t)B * T);
  if (N <= kRowThreads * kRowMaxPer)
  {
    const char* e = tune_env("W2L_CTC_LSE_VAR");
    const int var = e ? atoi(e) : 0;
    if (var == 1) hipLaunchKernelGGL(ctc_rows_lse<1>, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, ws);
    else if (var == 2) hipLaunchKernelGGL(ctc_rows_lse<2>, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, ws);
    else if (var == 3 || (!e && L >= 1)) hipLaunchKernelGGL(ctc_rows_lse<3>, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, ws);
    else hipLaunchKernelGGL(ctc_rows_lse<0>, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, ws);
  }
  else
    hipLaunchKernelGGL(ctc_rows_lse_big, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, ws);
  W2L_LAUNCH_CHECK();
  const int S = 2 * L + 1;
  const dim3 grid((unsigned)B, 2), blk(64);   // (utterance, alpha | beta)
  switch (ws.P) {   // (positions per lane, prefetch depth): 2 D P floats of p_t(s) in registers
    case 2: hipLaunchKernelGGL((ctc_scan<2, 16>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 3: hipLaunchKernelGGL((ctc_scan<3, 10>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 4: hipLaunchKernelGGL((ctc_scan<4, 8>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 5: hipLaunchKernelGGL((ctc_scan<5, 6>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 6: hipLaunchKernelGGL((ctc_scan<6, 5>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 8: hipLaunchKernelGGL((ctc_scan<8, 4>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 16: hipLaunchKernelGGL((ctc_scan<16, 2>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    default: hipLaunchKernelGGL((ctc_scan<32, 1>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
  }
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_ctc_backward(int B, int T, int N, int L, const float* input, const int* target,
                             const int* targetSize, const float* grad, float* inputGrad,
                             void* workspace, w2l_stream_t stream) {
  if (B <= 0 || T <= 0 || N <= 1 || L <= 0 || !input || !target || !targetSize || !grad || !inputGrad || !workspace)
    return W2L_EINVAL;
  if (L > kCtcMaxLabels) return W2L_EUNSUPPORTED;   // as the forward (and the LDS arrays of ctc_rows_grad)
  hipStream_t s = (hipStream_t)stream;
  CtcWs ws = ctc_ws(workspace, B, T, N, L);
  const unsigned rows = (unsigned)((size_t)B * T);
  hipLaunchKernelGGL(ctc_label_links_k, dim3((unsigned)B), dim3(kRowThreads), 0, s, L, target, targetSize, ws.link);
  W2L_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_rows_grad, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, grad, inputGrad, ws);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

// The score pass's workspace: lse [B][T] and the label probabilities pd [B][T][S] -- what the row pass hands to the alpha scan.
// No alpha / beta rows, no exponents, no links: those exist only for the backward pass.
static CtcWs ctc_score_ws(void* ws, int B, int T, int L) {
  CtcWs w{};
  w.P = ctc_positions_per_lane(L);
  w.S = 64 * w.P;
  char* p = (char*)ws;
  w.lse = (float*)p; p += align_up((size_t)B * T * sizeof(float), 256);
  w.pd = (double*)p;
  return w;
}

W2L_API size_t w2l_ctc_score_workspace_size(int B, int T, int N, int L) {
  if (B <= 0 || T <= 0 || N <= 0 || L < 0) return 0;
  const size_t S = 64 * (size_t)ctc_positions_per_lane(L);
  return align_up((size_t)B * T * sizeof(float), 256) + align_up((size_t)B * T * S * sizeof(double), 256);
}

W2L_API int w2l_ctc_score(int B, int T, int N, int L, int scaleMode, const float* input, const int* target,
                          const int* targetSize, float* loss, int* path, void* workspace, w2l_stream_t stream) {
  if (B <= 0 || T <= 0 || N <= 1 || L <= 0 || !input || !target || !targetSize || !loss || !path || !workspace)
    return W2L_EINVAL;
  if (L > kCtcMaxLabels) return W2L_EUNSUPPORTED;   // as w2l_ctc_forward
  hipStream_t s = (hipStream_t)stream;
  CtcWs ws = ctc_score_ws(workspace, B, T, L);
  const unsigned rows = (unsigned)((size_t)B * T);
  if (N <= kRowThreads * kRowMaxPer)
    hipLaunchKernelGGL(ctc_rows_score, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, ws, path);
  else
    hipLaunchKernelGGL(ctc_rows_score_big, dim3(rows), dim3(kRowThreads), 0, s, T, N, L, input, target, targetSize, ws, path);
  W2L_LAUNCH_CHECK();
  const dim3 grid((unsigned)B, 1), blk(64);   // the alpha wave of each utterance
  switch (ws.P) {   // the forward pass's (P, D) pairs
    case 2: hipLaunchKernelGGL((ctc_scan_score<2, 16>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 3: hipLaunchKernelGGL((ctc_scan_score<3, 10>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 4: hipLaunchKernelGGL((ctc_scan_score<4, 8>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 5: hipLaunchKernelGGL((ctc_scan_score<5, 6>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 6: hipLaunchKernelGGL((ctc_scan_score<6, 5>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 8: hipLaunchKernelGGL((ctc_scan_score<8, 4>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    case 16: hipLaunchKernelGGL((ctc_scan_score<16, 2>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
    default: hipLaunchKernelGGL((ctc_scan_score<32, 1>), grid, blk, 0, s, T, N, L, scaleMode, target, targetSize, loss, ws); break;
  }
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

W2L_API int w2l_ctc_viterbi(int B, int T, int N, const float* input, int* path, w2l_stream_t stream) {
  if (B <= 0 || T <= 0 || N <= 0 || !input || !path) return W2L_EINVAL;
  hipLaunchKernelGGL(ctc_rows_argmax, dim3((unsigned)((size_t)B * T)), dim3(kRowThreads), 0, (hipStream_t)stream, N, input, path);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}

#include "criterion_ctc_align.hpp"
#include "criterion_ctc_beam.hpp"
#include "criterion_ctc_beam_lm.hpp"
#include "criterion_ctc_beam_lex.hpp"
#include "criterion_asg_beam.hpp"
#include "criterion_beam_wide.hpp"
#include "criterion_beam_xl.hpp"
#include "criterion_beam_stream.hpp"
#include "criterion_beam_commit.hpp"
#include "criterion_beam_lextok.hpp"
#include "criterion_beam_entry.hpp"
