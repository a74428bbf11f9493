// conv_tds_special.hip -- the launchers of the SPECIALISED fp32 TDS time-convolution kernels: the kernels written for the
// exact layer geometries of the TDS recipes (fl::TDSBlock's Conv2D kw x 1 with C = 10 / 14 / 18, kw = 21, H = 80 mel rows, and
// the sub-sampling layers between the stages; recipes/sota/2019/am_arch/am_tds_ctc.arch:3-37).  conv_tds.hip offers every
// launch (a TdsConvP, conv_tds.hpp) to the tds_*_try functions below in the order written here -- this comment is the one
// place where that order is written down.  A function that returns false has launched nothing, and the launch goes on to
// the next line; the last line of each chain is the general kernels of conv_tds.hip, which take every geometry and
// honour `accum` and `add`.
//
// forward and backward-data (launch_fwd):
//   1. tds_c1_fwd_try       tds_c1_fwd_k (conv_tds_c1.hpp): the one-channel first layer, 1 -> 10 channels, forward only,
//                           kw <= 21, any stride and H, no addend, no accumulate
//   2. tds_tz_try           tds_conv_tz_k (conv_tds_tz.hpp, block-Toeplitz): H % 16 == 0, kw <= 21, no accumulate, 16-byte
//                           aligned tensors, one utterance below 2 GiB, and one of
//                             C -> C with C = 10 / 14 / 18, stride 1: forward (bias, ReLU) and backward-data (addend)
//                             10 -> 14 and 14 -> 18, stride 2: forward
//                             14 -> 10 and 18 -> 14: the two phases of the backward-data pass of those strided layers (every
//                             second tap, every second frame of dx; tds_conv_backward_data offers its phases to this line only)
//   3. conv_tds.hip         tds_conv_fwd2_k (H % 16 == 0, float4-addressable rows), else tds_conv_fwd_k (anything)
// filter gradient (tds_conv_backward_filter):
//   1. tds_rsf_try          C -> C, stride 1, kw <= 21, 16-byte aligned, one utterance below 2 GiB:
//                             tds_conv_tzf_k (conv_tds_tzf.hpp, block-Toeplitz): C = 10 / 14, H % 16 == 0
//                             else tds_conv_rsf3_k (conv_tds_rsf3.hpp, role-swapped, wave-specialised): C = 10 / 18, H % 8 == 0
//   2. tds_c1_filter_try    tds_c1_filter_k (conv_tds_c1.hpp): 1 -> 10 channels, stride 2, kw <= 21
//   3. tds_tzf_strided_try  tds_conv_tzf_k: 10 -> 14 and 14 -> 18, stride 2, H % 16 == 0, kw <= 21
//   4. conv_tds.hip         tds_conv_filter2_k (H % 16 == 0, float4-addressable rows), else tds_conv_filter_k (anything)
//
// Probe library: W2L_TDS_C1_OFF, W2L_TDS_TZ_OFF, W2L_TDS_TZ_C2_OFF (the strided layers and phases only), W2L_TDS_RSF_OFF and
// W2L_TDS_TZF_OFF make the line they name refuse, i.e. they select the general kernels.
#include <cstdlib>
#include <type_traits>

#include "conv_tds.hpp"
#include "conv_tds_tz.hpp"
#include "conv_tds_rsf3.hpp"
#include "conv_tds_tzf.hpp"
#include "conv_tds_c1.hpp"

namespace w2l {

template <int CI, int CO, int R, int NCT, int SIG, int KWM, int ST, bool FWD>
static int tz_launch(TdsTzP p, int abl, hipStream_t s) {
  using Cfg = TzCfg<CI, CO, R, NCT, SIG, KWM, ST>;
  { const char* e = tune_env("W2L_TDS_TZ_DBG"); p.dbg = e ? (long long*)strtoull(e, nullptr, 10) : nullptr; }
  p.hBlocks = p.H / Cfg::HB;
  p.rps = (p.Tout + Cfg::RF - 1) / Cfg::RF;
  const long long rounds = (long long)p.B * p.hBlocks * p.rps;
  if (rounds <= 0 || rounds > (1ll << 30)) return W2L_EUNSUPPORTED;
  p.nRounds = (int)rounds;
  // two workgroups per CU; equal contiguous shares of the round axis
  // 512 = two resident workgroups per CU; where the rounds do not divide by 512 but do by 768 (C = 14: 3840 rounds = 7.5 per
  // workgroup at 512, 5 at 768) the finer cut wins: 79.7 / 76.3 us against 82.6 / 79.2 (profiles/r05_run16_conv_tz.log)
  int wgMax = (p.nRounds % 512 != 0 && p.nRounds % 768 == 0) ? 768 : 512;
  { const char* e = tune_env("W2L_TDS_TZ_WGS"); if (e && atoi(e) > 0) wgMax = atoi(e); }
  const int wgs = p.nRounds < wgMax ? p.nRounds : wgMax;
  p.rpw = (p.nRounds + wgs - 1) / wgs;
  const int blocks = (p.nRounds + p.rpw - 1) / p.rpw;
  constexpr bool DEFER = true;       // (C = 18 has the registers for the second accumulator set since its waves walk their own 22-frame windows)
  constexpr int M0 = FWD ? 0 : 2;    // the two modes of the direction: plain / + ReLU, plain / + addend
#ifdef W2L_PROBE
  if (abl && FWD) {
    bool done = false;
    auto go = [&](auto tag) {
      constexpr int M = decltype(tag)::value;
      if (abl != M || done || !p.relu) return;
      (void)hipFuncSetAttribute((const void*)tds_conv_tz_k<CI, CO, R, NCT, SIG, KWM, ST, 1, DEFER, M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS);
      hipLaunchKernelGGL((tds_conv_tz_k<CI, CO, R, NCT, SIG, KWM, ST, 1, DEFER, M>), dim3((unsigned)blocks), dim3(256), Cfg::LDS, s, p);
      done = true;
    };
    go(std::integral_constant<int, 1>{}); go(std::integral_constant<int, 2>{}); go(std::integral_constant<int, 4>{});
    go(std::integral_constant<int, 8>{}); go(std::integral_constant<int, 14>{}); go(std::integral_constant<int, 12>{});
    if (done) return W2L_OK;
  }
#endif
  static bool attr[64] = {};
  if (first_on_device(attr)) {
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_tz_k<CI, CO, R, NCT, SIG, KWM, ST, M0, DEFER, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS));
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_tz_k<CI, CO, R, NCT, SIG, KWM, ST, M0 + 1, DEFER, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS));
  }
  const bool second = FWD ? p.relu != 0 : p.add != nullptr;
  if (second) hipLaunchKernelGGL((tds_conv_tz_k<CI, CO, R, NCT, SIG, KWM, ST, M0 + 1, DEFER, 0>), dim3((unsigned)blocks), dim3(256), Cfg::LDS, s, p);
  else hipLaunchKernelGGL((tds_conv_tz_k<CI, CO, R, NCT, SIG, KWM, ST, M0, DEFER, 0>), dim3((unsigned)blocks), dim3(256), Cfg::LDS, s, p);
  return W2L_OK;
}

// true + *status when the block-Toeplitz generation (conv_tds_tz.hpp) runs this convolution: the TDS convolutions proper
// (C -> C, stride 1, both directions), the strided sub-sampling layers between the stages (10 -> 14, 14 -> 18, stride 2)
// forward, and the phases of their backward-data pass (every second tap, every second output frame)
bool tds_tz_try(const TdsConvP& q, int profKind, hipStream_t s, int* status) {
  const float *x = q.x, *w = q.w, *bias = q.bias, *add = q.add;
  float* y = q.y;
  const int B = q.B, Tin = q.Tin, Tout = q.Tout, H = q.H, Cin = q.Cin, Cout = q.Cout, kw = q.kw, stride = q.stride, padl = q.padl,
            relu = q.relu, flip = q.flip, tapOff = q.tapOff, tapStep = q.tapStep, oOff = q.oOff, oStep = q.oStep, ToutFull = q.ToutFull;
  if (q.CinW != (flip ? Cout : Cin) || q.CoutW != (flip ? Cin : Cout)) return false;   // the whole weight tensor, not a slice of it
  if (tune_env("W2L_TDS_TZ_OFF") || H % 16 || q.accum || kw < 1) return false;
  if (flip ? (bias || relu || stride != 1) : (add || tapOff || tapStep != 1 || oOff || oStep != 1)) return false;
  if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)add | (uintptr_t)w) & 15) != 0) return false;
  if ((long long)Tin * H * Cin * 4 >= (1ll << 31) || (long long)ToutFull * H * Cout * 4 >= (1ll << 31)) return false;   // one utterance per buffer resource
  TdsTzP p{};
  p.x = x; p.w = w; p.bias = bias; p.add = add; p.y = y;
  p.B = B; p.Tin = Tin; p.Tout = Tout; p.H = H; p.kw = kw; p.padl = padl; p.relu = relu; p.flip = flip;
  p.kwFull = flip ? tapOff + tapStep * (kw - 1) + 1 : kw;
  p.tapOff = tapOff; p.oOff = oOff; p.oStep = oStep; p.ToutFull = ToutFull;
  int abl = 0;
  { const char* e = tune_env("W2L_TDS_RS_ABL"); abl = e ? atoi(e) : 0; }
  int st = W2L_EUNSUPPORTED;
  const bool same = Cin == Cout && stride == 1 && tapStep == 1 && kw <= 21;
  const bool sub = !flip && stride == 2 && kw <= 21 && !tune_env("W2L_TDS_TZ_C2_OFF");
  const bool phase = flip && tapStep == 2 && kw <= 11 && !tune_env("W2L_TDS_TZ_C2_OFF");
  if (!(same && (Cin == 10 || Cin == 14 || Cin == 18)) && !(sub && ((Cin == 10 && Cout == 14) || (Cin == 14 && Cout == 18))) &&
      !(phase && ((Cin == 14 && Cout == 10) || (Cin == 18 && Cout == 14))))
    return false;
  prof_begin(s, 2.0 * B * Tout * (double)H * kw * Cin * Cout, profKind);
  if (same) {
    if (!flip) st = Cin == 10 ? tz_launch<10, 10, 3, 1, 1, 21, 1, true>(p, abl, s) : Cin == 14 ? tz_launch<14, 14, 2, 1, 1, 21, 1, true>(p, abl, s)
                                                                                                  : tz_launch<18, 18, 3, 2, 1, 21, 1, true>(p, abl, s);
    else st = Cin == 10 ? tz_launch<10, 10, 3, 1, 1, 21, 1, false>(p, abl, s) : Cin == 14 ? tz_launch<14, 14, 2, 1, 1, 21, 1, false>(p, abl, s)
                                                                                              : tz_launch<18, 18, 3, 2, 1, 21, 1, false>(p, abl, s);
  } else if (sub) {
    st = Cin == 10 ? tz_launch<10, 14, 2, 1, 2, 21, 1, true>(p, 0, s) : tz_launch<14, 18, 3, 2, 2, 21, 1, true>(p, 0, s);
  } else {
    st = Cin == 14 ? tz_launch<14, 10, 3, 1, 1, 11, 2, false>(p, 0, s) : tz_launch<18, 14, 2, 1, 1, 11, 2, false>(p, 0, s);
  }
  prof_end(s);
  if (st == W2L_EUNSUPPORTED) return false;   // tz_launch refused (round count out of range)
  if (st == W2L_OK && hipGetLastError() != hipSuccess) st = W2L_EHIP;
  *status = st;
  return true;
}

// ================================================================================================ backward-filter
// dW[tap][ci][co] = sum_{b,t,h} X[t + tap - padl][h][ci] * dY[t][h][co],   dbias[co] = sum dY[t][h][co]
// is a GEMM with a huge K = (b, t, h) and a 21*C x C result: with the result on 16-wide tiles of 16x16x4 MFMAs
// (conv_tds.hip) C = 10 / 14 / 18 columns fill 62.5 / 87.5 / 56 % of the lanes and the loop was issue-bound at ~30-47 %.
// Role swap for the filter gradient: split tap = ga*GB + gb and shift BOTH operands along time,
//     D[(ga, ci)][(gb, co)] = sum_{t'} X[t' + ga*GB - padl][ci] * dY[t' - gb][co]          (t' = t + gb)
// rows (ga, ci) = GA*C (+ one all-ones row: its gb = 0 columns are the bias gradient), columns (gb, co) = GB*C, K = time:
//     C = 10: GA = 3, GB = 7 : 1 x 3 tiles of 32x32, 21 taps     68 % of the MFMA lanes carry a wanted product
//     C = 14: GA = 2, GB = 11: 1 x 5 tiles, 22 taps (21 wanted)  80 %
//     C = 18: GA = 7, GB = 3 : 4 x 2 tiles, 21 taps              83 %
// Both operands are read straight out of time-fastest slabs (x[(h, ci)][frame], dy[(h, co)][frame]): a fragment read is
// 32 consecutive floats of one row, the K step is an immediate offset, NRT + NCT ds_read_b32 feed NRT*NCT 64-cycle MFMAs.
// A wave owns one mel row of the workgroup's tile and keeps its NRT x NCT accumulators in registers over ALL its tiles
// (conv_tds_rsf3.hpp); one partial per workgroup goes to the stream scratch, tds_rsf_reduce_k adds the partials in
// workgroup order (deterministic) and scatters into dW / dbias.  The block-Toeplitz filter gradient (conv_tds_tzf.hpp)
// is launched from the same descriptor.
struct TdsRsfP {
  const float* x;   // [B][Tin][H][C]
  const float* dy;  // [B][Tout][H][C]
  int B, Tin, Tout, H, kw, padl;
};

static TdsRsfP make_rsf_p(const TdsConvP& q, const float* dy) {
  TdsRsfP p{};
  p.x = q.x; p.dy = dy; p.B = q.B; p.Tin = q.Tin; p.Tout = q.Tout; p.H = q.H; p.kw = q.kw; p.padl = q.padl;
  return p;
}

// dw / dbias = sum over the workgroups' partials, in workgroup order.  One thread per (element, slice of the partials);
// 64 elements x 16 slices per block (the partials of a slice are independent loads: 16 in flight per thread with 256
// workgroups), slices combined in fixed order through LDS.  (With 4 slices and one load stream per thread this launch
// took 17-20 us, a fifth of the whole filter gradient: profiles/r02_run15_*.)
template <int C, int GA, int GB, int NRT, int NCT>
__global__ __launch_bounds__(1024) void tds_rsf_reduce_k(const float* __restrict__ partial, int nParts, int kw, float* __restrict__ dw,
                                                        float* __restrict__ dbias) {
  constexpr int ACCF = NRT * NCT * 16 * 64, NS = 16;
  __shared__ float red[NS][64];
  const int el = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;   // index in register order: ((rt*NCT + ct)*16 + q)*64 + lane
  float s = 0.f;
  const int per = (nParts + NS - 1) / NS;
  const int g0 = sl * per, g1 = g0 + per < nParts ? g0 + per : nParts;
  if (e < ACCF) {
    int g = g0;
    for (; g + 4 <= g1; g += 4) {
      const float a0 = partial[(size_t)g * ACCF + e], a1 = partial[(size_t)(g + 1) * ACCF + e], a2 = partial[(size_t)(g + 2) * ACCF + e],
                  a3 = partial[(size_t)(g + 3) * ACCF + e];
      s = (((s + a0) + a1) + a2) + a3;
    }
    for (; g < g1; ++g) s += partial[(size_t)g * ACCF + e];
  }
  red[sl][el] = s;
  __syncthreads();
  if (sl == 0 && e < ACCF) {
    float t = red[0][el];
#pragma unroll
    for (int k = 1; k < NS; ++k) t += red[k][el];
    const int lane = e & 63, q = (e >> 6) & 15, tl = e >> 10, rt = tl / NCT, ct = tl - rt * NCT;
    const int m = 32 * rt + 8 * (q >> 2) + 4 * (lane >> 5) + (q & 3), n = 32 * ct + (lane & 31);
    const int gb = n / C, co = n - gb * C;
    if (gb < GB) {
      if (m < GA * C) {
        const int ga = m / C, ci = m - ga * C, tap = ga * GB + gb;
        if (tap < kw) dw[((size_t)tap * C + ci) * C + co] = t;
      } else if (m == GA * C && gb == 0 && dbias) {
        dbias[co] = t;
      }
    }
  }
}

template <int C, int GA, int GB, int HH, int TS>
static int rsf3_launch(const TdsRsfP& q, float* dw, float* dbias, hipStream_t s) {
  using Cfg = Rsf3Cfg<C, GA, GB, HH, TS>;
  if (q.H % HH) return W2L_EUNSUPPORTED;
  if ((long long)q.Tin * q.H * C * 4 >= (1ll << 31) || (long long)q.Tout * q.H * C * 4 >= (1ll << 31)) return W2L_EUNSUPPORTED;   // one utterance per buffer resource
  TdsRsf3P p{};
  p.x = q.x; p.dy = q.dy; p.B = q.B; p.Tin = q.Tin; p.Tout = q.Tout; p.H = q.H; p.kw = q.kw; p.padl = q.padl;
  p.hBlocks = q.H / HH;
  p.nStrips = (q.Tout + GB - 1 + TS - 1) / TS;
  const long long tiles = (long long)q.B * p.nStrips * p.hBlocks;
  if (tiles > (1ll << 30)) return W2L_EUNSUPPORTED;
  p.nTiles = (int)tiles;
  const int blocks = p.nTiles < 256 ? p.nTiles : 256;
  float* partial = sk_scratch(s, kSkScratchBytes);
  if (!partial || (size_t)blocks * Cfg::ACCF * sizeof(float) > kSkScratchBytes) return W2L_EUNSUPPORTED;
  static bool attr[64] = {};
  if (first_on_device(attr)) {
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_rsf3_k<C, GA, GB, HH, TS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS));
  }
  hipLaunchKernelGGL((tds_conv_rsf3_k<C, GA, GB, HH, TS>), dim3((unsigned)blocks), dim3(Cfg::WAVES * 64), Cfg::LDS, s, p, partial);
  hipLaunchKernelGGL((tds_rsf_reduce_k<C, GA, GB, Cfg::NRT, Cfg::NCT>), dim3((unsigned)((Cfg::ACCF + 63) / 64)), dim3(1024), 0, s, partial,
                     blocks, q.kw, dw, dbias);
  return W2L_OK;
}

// block-Toeplitz filter gradient (conv_tds_tzf.hpp)
template <int CI, int CO, int R, int GR, int SIG>
static int tzf_launch(const TdsRsfP& q, float* dw, float* dbias, hipStream_t s) {
  using Cfg = TzfCfg<CI, CO, R, GR, SIG>;
  if (q.H % Cfg::HB) return W2L_EUNSUPPORTED;
  if ((long long)q.Tin * q.H * CI * 4 >= (1ll << 31) || (long long)q.Tout * q.H * CO * 4 >= (1ll << 31)) return W2L_EUNSUPPORTED;   // one utterance per buffer resource
  TdsTzfP p{};
  p.x = q.x; p.dy = q.dy; p.B = q.B; p.Tin = q.Tin; p.Tout = q.Tout; p.H = q.H; p.kw = q.kw; p.padl = q.padl;
  p.hBlocks = q.H / Cfg::HB;
  p.rps = (q.Tout + Cfg::RF - 1) / Cfg::RF;
  const long long rounds = (long long)q.B * p.hBlocks * p.rps;
  if (rounds <= 0 || rounds > (1ll << 30)) return W2L_EUNSUPPORTED;
  p.nRounds = (int)rounds;
  const int wgs = p.nRounds < 256 ? p.nRounds : 256;   // one workgroup per CU
  p.rpw = (p.nRounds + wgs - 1) / wgs;
  const int blocks = (p.nRounds + p.rpw - 1) / p.rpw;
  float* partial = sk_scratch(s, kSkScratchBytes);
  if (!partial || (size_t)blocks * Cfg::ACCF * sizeof(float) > kSkScratchBytes) return W2L_EUNSUPPORTED;
  static bool attr[64] = {};
  if (first_on_device(attr)) {
    W2L_HIP_CHECK(hipFuncSetAttribute((const void*)tds_conv_tzf_k<CI, CO, R, GR, SIG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS));
  }
  hipLaunchKernelGGL((tds_conv_tzf_k<CI, CO, R, GR, SIG>), dim3((unsigned)blocks), dim3(512), Cfg::LDS, s, p, partial);
  hipLaunchKernelGGL((tds_tzf_reduce_k<CI, CO, R, GR, SIG>), dim3((unsigned)((q.kw * CI * CO + CO + 15) / 16)), dim3(1024), 0, s, partial, blocks, q.kw, dw, dbias);
  return W2L_OK;
}

// the one-input-channel first layer of the TDS recipes (conv_tds_c1.hpp): forward, and filter + bias gradient
bool tds_c1_fwd_try(const TdsConvP& q, int profKind, hipStream_t s, int* status) {
  if (q.Cin != 1 || q.flip || q.add || q.accum || q.CinW != 1 || q.CoutW != q.Cout || q.tapStep != 1 || q.oStep != 1) return false;
  const int B = q.B, Tout = q.Tout, H = q.H, Cout = q.Cout, kw = q.kw;
  if (tune_env("W2L_TDS_C1_OFF") || Cout != 10 || kw > 21 || kw < 1 || (((uintptr_t)q.y) & 15) != 0) return false;
  TdsC1P p{};
  p.x = q.x; p.w = q.w; p.bias = q.bias; p.y = q.y; p.B = B; p.Tin = q.Tin; p.Tout = Tout; p.H = H; p.kw = kw; p.stride = q.stride; p.padl = q.padl; p.relu = q.relu;
  const long long total = (long long)B * Tout * H;
  if (total <= 0 || total > (1ll << 31) - 512) return false;
  prof_begin(s, 2.0 * B * Tout * (double)H * kw * Cout, profKind);
  hipLaunchKernelGGL((tds_c1_fwd_k<10, 21>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
  prof_end(s);
  *status = hipGetLastError() == hipSuccess ? W2L_OK : W2L_EHIP;
  return true;
}

bool tds_c1_filter_try(const TdsConvP& q, const float* dy, float* dw, float* dbias, hipStream_t s, int* status) {
  const int B = q.B, Tout = q.Tout, H = q.H, Cout = q.Cout, kw = q.kw;
  if (q.Cin != 1 || tune_env("W2L_TDS_C1_OFF") || Cout != 10 || kw > 21 || kw < 1 || q.stride != 2) return false;   // (the kernel's sliding window is written for stride 2)
  TdsC1P p{};
  p.x = q.x; p.dy = dy; p.B = B; p.Tin = q.Tin; p.Tout = Tout; p.H = H; p.kw = kw; p.stride = q.stride; p.padl = q.padl;
  const long long total = (long long)B * ((Tout + 3) / 4) * H;   // runs of four output frames
  if (total <= 0 || (long long)B * Tout * H > (1ll << 31) - 65536 * 128) return false;
  long long blocks = (total + 127) / 128;
  if (blocks > 512) blocks = 512;
  constexpr int ROW = 21 * 10 + 10;
  float* partial = sk_scratch(s, kSkScratchBytes);
  if (!partial || (size_t)blocks * ROW * sizeof(float) > kSkScratchBytes) return false;
  prof_begin(s, 2.0 * B * Tout * (double)H * kw * Cout, PROF_TDS_BWD_FILTER);
  hipLaunchKernelGGL((tds_c1_filter_k<10, 21>), dim3((unsigned)blocks), dim3(256), 0, s, p, partial);
  hipLaunchKernelGGL((tds_c1_filter_reduce_k<10, 21>), dim3((ROW + 31) / 32), dim3(1024), 0, s, partial, (int)blocks, kw, dw, dbias);
  prof_end(s);
  *status = hipGetLastError() == hipSuccess ? W2L_OK : W2L_EHIP;
  return true;
}

// true + *status when the block-Toeplitz filter gradient runs a strided sub-sampling layer (10 -> 14, 14 -> 18, stride 2)
bool tds_tzf_strided_try(const TdsConvP& q, const float* dy, float* dw, float* dbias, hipStream_t s, int* status) {
  const int H = q.H, Cin = q.Cin, Cout = q.Cout, kw = q.kw;
  if (tune_env("W2L_TDS_TZF_OFF") || tune_env("W2L_TDS_TZ_C2_OFF") || q.stride != 2 || kw > 21 || kw < 1 || H % 16) return false;
  if (!((Cin == 10 && Cout == 14) || (Cin == 14 && Cout == 18))) return false;
  if ((((uintptr_t)q.x | (uintptr_t)dy) & 15) != 0) return false;
  const TdsRsfP p = make_rsf_p(q, dy);
  prof_begin(s, 2.0 * q.B * q.Tout * (double)H * kw * Cin * Cout, PROF_TDS_BWD_FILTER);
  int st = Cin == 10 ? tzf_launch<10, 14, 2, 12, 2>(p, dw, dbias, s) : tzf_launch<14, 18, 1, 12, 2>(p, dw, dbias, s);
  prof_end(s);
  if (st == W2L_EUNSUPPORTED) return false;
  if (st == W2L_OK && hipGetLastError() != hipSuccess) st = W2L_EHIP;
  *status = st;
  return true;
}

// true + *status when the filter gradient of a TDS convolution proper (C -> C, stride 1) runs on the block-Toeplitz kernel
// (conv_tds_tzf.hpp: C = 10 / 14, H % 16 == 0) or else on the wave-specialised role-swapped one (conv_tds_rsf3.hpp:
// C = 10 / 18, H % 8 == 0)
bool tds_rsf_try(const TdsConvP& q, const float* dy, float* dw, float* dbias, hipStream_t s, int* status) {
  const int H = q.H, C = q.Cin, kw = q.kw;
  if (q.stride != 1 || q.Cin != q.Cout || tune_env("W2L_TDS_RSF_OFF")) return false;
  if (!(C == 10 || C == 14 || C == 18) || kw > 21 || kw < 1) return false;
  if ((((uintptr_t)q.x | (uintptr_t)dy) & 15) != 0) return false;
  const bool tzf = !tune_env("W2L_TDS_TZF_OFF") && H % 16 == 0 && (C == 10 || C == 14);
  const bool rsf3 = H % 8 == 0 && C != 14;   // (C = 14 measured 152 us against 103 us of conv_tds.hip's kernel)
  if (!tzf && !rsf3) return false;
  const TdsRsfP p = make_rsf_p(q, dy);
  prof_begin(s, 2.0 * q.B * q.Tout * (double)H * kw * C * C, PROF_TDS_BWD_FILTER);
  int st = W2L_EUNSUPPORTED;
  if (tzf) st = C == 10 ? tzf_launch<10, 10, 3, 16, 1>(p, dw, dbias, s) : tzf_launch<14, 14, 2, 12, 1>(p, dw, dbias, s);
  if (st == W2L_EUNSUPPORTED && rsf3) st = C == 10 ? rsf3_launch<10, 3, 7, 8, 96>(p, dw, dbias, s) : rsf3_launch<18, 7, 3, 4, 96>(p, dw, dbias, s);
  prof_end(s);
  if (st == W2L_EUNSUPPORTED) return false;
  if (st == W2L_OK && hipGetLastError() != hipSuccess) st = W2L_EHIP;
  *status = st;
  return true;
}

}  // namespace w2l
