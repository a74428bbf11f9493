// rnn.hip -- fl::RNN (arch tokens RNN / GRU / LSTM; fl::RnnMode RELU, TANH, LSTM, GRU): stacked, optionally bidirectional recurrent
// layers with cuDNN's equations (DESIGN 3.32 is the contract).  fp32 throughout.
//
// The arithmetic splits in two.  Everything that does not depend on the previous frame is a whole-sequence product on the fp32 MFMA
// GEMM (gemm_f32): the input-side pre-activations X . W_ih^T + b_ih of a layer and direction over all B T rows, and in the backward
// dX, dW_ih, dW_hh and (column sums) the bias gradients.  The recurrence is ONE launch per time step; the launch boundary is the only
// synchronisation between steps (no grid barrier, no cooperative launch, no spinning on flags, no atomics).  Both directions of a
// bidirectional layer share a launch (blockIdx.z; forward at frame s, reverse at T - 1 - s).
//
//   forward step    a workgroup (256 threads = 4 waves) owns a tile of 32 batch rows and a slice of J = 32 / G hidden units, i.e. up to
//                   32 rows of W_hh: one v_mfma_f32_32x32x2_f32 tile (M = batch, N = gate rows).  h_{t-1} [32][H] goes through LDS in
//                   chunks of 128 columns (H is not bounded by LDS); inside a chunk wave w multiplies columns 32 w .. 32 w + 31, a lane
//                   reading its weight row 16 bytes at a time, so the weight slice is streamed exactly once per step.  The four
//                   partial tiles are added through LDS in wave order, then b_hh and the staged pre-activation are added, the gate
//                   functions (expf / tanhf, not the hardware approximations) applied, c updated and h_t written straight to
//                   y[b][t][dir H + j].  In training the gate activations replace the pre-activations in place, c_t (LSTM) and
//                   W_hn h + b_hn (GRU) are kept, and h_{t-1} is kept beside frame t (hp), zero at the first frame of the scan.
//   backward step   the same ownership with J = 32 for every mode: dh_t = dy_t + dgates_{t+1} . W_hh (K = G H over what the previous
//                   launch wrote, W_hh read as rows: coalesced) (+ z_{t+1} dh_{t+1} for the GRU, + the c gradient for the LSTM; both
//                   carried in [B][H] buffers that only their owner touches), then the pointwise gate backward, dgates_t written.
//
// Every sum has ONE order: chunks ascending inside a wave, waves 0..3, so two runs give the same bits, and an output row is a function
// of its own batch row only -- the same bits whatever tile or batch size it ran in.
//
// dW_hh pairs dgates_t with h_{t-1}: with hp kept per frame (zero where the scan starts) it is one product over all B T rows -- the
// rows a shifted view of y would have to skip at every utterance boundary multiply zeros instead.
#include <algorithm>

#include "gemm.hpp"

namespace w2l {

constexpr int kRnnThreads = 256;
constexpr int kRnnBt = 32;        // batch rows of a workgroup = M of the MFMA tile
constexpr int kRnnKc = 128;       // columns of h (dgates) staged per chunk: 32 per wave
constexpr int kRnnLd = kRnnKc + 4;
constexpr int kRnnMaxDim = 4096, kRnnMaxB = 1024, kRnnMaxLayers = 8, kRnnMaxT = 1 << 16;

static inline int rnn_gates(int mode) { return mode == W2L_RNN_LSTM ? 4 : mode == W2L_RNN_GRU ? 3 : 1; }

struct RnnStep {
  const float* whh[2]; const float* bhh[2];
  float* gates[2];      // [B T][G H]: pre-activations in, activations out (training)
  float* cs[2];         // LSTM: c_t [B T][H]
  float* hn[2];         // GRU: W_hn h + b_hn [B T][H]
  float* hp[2];         // training: h_{t-1} beside frame t [B T][H]
  float* y; int ldy;    // [B][T][ldy], direction d at column d H
  // backward
  const float* dy; int lddy;
  float* dgi[2];        // [B T][G H] gradient of the input-side pre-activations
  float* dgh[2];        // GRU: of the hidden-side ones (n gate times r); otherwise == dgi
  float* dhc[2];        // GRU: z dh carried to the previous frame [B][H]
  float* dcc[2];        // LSTM: c gradient carried [B][H]
  int B, T, H, s, train;
};

__device__ __forceinline__ float sigmoidf_acc(float x) { return 1.f / (1.f + expf(-x)); }

// acc (+)= rows[b0 .. b0 + 31][0 .. K) . Wslice: the 32 x 32 tile of this wave's share of the reduction.  FWD: column n of the tile is
// weight row wrow(n) (k contiguous); BWD: column n is weight column j0 + n (rows are k).  src == nullptr: nothing to add.
template <bool FWD>
__device__ __forceinline__ void scan_product(f32x16& acc, float* lds, const float* src, size_t srcStride, int rows, int K, const float* W,
                                             int ldw, int wrow, bool wvalid, bool vec) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  for (int k0 = 0; k0 < K; k0 += kRnnKc) {
    __syncthreads();
    for (int r = tid >> 7; r < kRnnBt; r += 2) {
      const int c = tid & 127;
      lds[r * kRnnLd + c] = (r < rows && k0 + c < K) ? src[(size_t)r * srcStride + k0 + c] : 0.f;
    }
    __syncthreads();
    if (k0 + wave * 32 >= K) continue;   // wave-uniform: this wave's columns lie past the reduction
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int kl = wave * 32 + it * 8 + lh * 4, k = k0 + kl;
      const float4 a = *reinterpret_cast<const float4*>(&lds[li * kRnnLd + kl]);
      float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
      if (FWD) {
        const float* p = W + (size_t)wrow * ldw + k;
        if (wvalid) {
          if (vec) { if (k < K) w = *reinterpret_cast<const float4*>(p); }
          else {
            if (k < K) w.x = p[0];
            if (k + 1 < K) w.y = p[1];
            if (k + 2 < K) w.z = p[2];
            if (k + 3 < K) w.w = p[3];
          }
        }
      } else if (wvalid) {
        const float* p = W + (size_t)k * ldw + wrow;
        if (k < K) w.x = p[0];
        if (k + 1 < K) w.y = p[ldw];
        if (k + 2 < K) w.z = p[2 * (size_t)ldw];
        if (k + 3 < K) w.w = p[3 * (size_t)ldw];
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, acc, 0, 0, 0);
    }
  }
}

// the four waves' tiles into red[w][b][n] (n fastest, row stride 33)
__device__ __forceinline__ void scan_reduce(const f32x16& acc, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * kRnnBt + (r & 3) + 8 * (r >> 2) + 4 * lh) * 33 + li] = acc[r];
  __syncthreads();
}
__device__ __forceinline__ float red_sum(const float* red, int b, int n) {
  return ((red[(0 * kRnnBt + b) * 33 + n] + red[(1 * kRnnBt + b) * 33 + n]) + red[(2 * kRnnBt + b) * 33 + n]) + red[(3 * kRnnBt + b) * 33 + n];
}

template <int MODE>
__global__ __launch_bounds__(kRnnThreads) void rnn_fwd_step_k(RnnStep a) {
  constexpr int G = MODE == W2L_RNN_LSTM ? 4 : MODE == W2L_RNN_GRU ? 3 : 1, J = 32 / G;
  __shared__ __attribute__((aligned(16))) float lds[kRnnBt * kRnnLd];
  __shared__ float red[4 * kRnnBt * 33];
  const int d = blockIdx.z, H = a.H, T = a.T, B = a.B;
  const int j0 = blockIdx.x * J, b0 = blockIdx.y * kRnnBt, rows = min(kRnnBt, B - b0);
  const int t = d ? T - 1 - a.s : a.s, tp = d ? t + 1 : t - 1;
  const bool first = a.s == 0;
  const int li = threadIdx.x & 31;
  // tile column n = g J + jj is weight row g H + j0 + jj
  const int g = li / J, jj = li - g * J;
  const bool wvalid = g < G && j0 + jj < H;
  const int wrow = g * H + j0 + jj;
  const float* W = a.whh[d];
  const bool vec = (H & 3) == 0 && ((uintptr_t)W & 15) == 0;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float* yd = a.y + (size_t)d * H;
  if (!first)   // h_{t-1} of this tile's rows: y[b][tp][d H ..]
    scan_product<true>(acc, lds, yd + ((size_t)b0 * T + tp) * a.ldy, (size_t)T * a.ldy, rows, H, W, H, wrow, wvalid, vec);
  scan_reduce(acc, red);
  const float* bh = a.bhh[d];
  for (int e = threadIdx.x; e < kRnnBt * J; e += kRnnThreads) {
    const int b = e / J, u = e - b * J, j = j0 + u;
    if (b >= rows || j >= H) continue;
    const size_t row = (size_t)(b0 + b) * T + t, rowp = (size_t)(b0 + b) * T + tp;
    float* gt = a.gates[d] + row * (size_t)(G * H);
    const float hprev = first ? 0.f : yd[rowp * a.ldy + j];
    float h;
    if (MODE == W2L_RNN_RELU || MODE == W2L_RNN_TANH) {
      const float v = gt[j] + (red_sum(red, b, u) + bh[j]);
      h = MODE == W2L_RNN_RELU ? fmaxf(v, 0.f) : tanhf(v);
      if (a.train) gt[j] = h;
    } else if (MODE == W2L_RNN_LSTM) {
      const float gi = sigmoidf_acc(gt[j] + (red_sum(red, b, u) + bh[j]));
      const float gf = sigmoidf_acc(gt[H + j] + (red_sum(red, b, J + u) + bh[H + j]));
      const float gg = tanhf(gt[2 * H + j] + (red_sum(red, b, 2 * J + u) + bh[2 * H + j]));
      const float go = sigmoidf_acc(gt[3 * H + j] + (red_sum(red, b, 3 * J + u) + bh[3 * H + j]));
      const float cprev = first ? 0.f : a.cs[d][rowp * H + j];
      const float c = gf * cprev + gi * gg;
      a.cs[d][row * H + j] = c;
      h = go * tanhf(c);
      if (a.train) { gt[j] = gi; gt[H + j] = gf; gt[2 * H + j] = gg; gt[3 * H + j] = go; }
    } else {
      const float gr = sigmoidf_acc(gt[j] + (red_sum(red, b, u) + bh[j]));
      const float gz = sigmoidf_acc(gt[H + j] + (red_sum(red, b, J + u) + bh[H + j]));
      const float hn = red_sum(red, b, 2 * J + u) + bh[2 * H + j];
      const float gn = tanhf(gt[2 * H + j] + gr * hn);
      h = (1.f - gz) * gn + gz * hprev;
      if (a.train) { gt[j] = gr; gt[H + j] = gz; gt[2 * H + j] = gn; a.hn[d][row * H + j] = hn; }
    }
    a.y[row * a.ldy + (size_t)d * H + j] = h;
    if (a.train) a.hp[d][row * H + j] = hprev;
  }
}

template <int MODE>
__global__ __launch_bounds__(kRnnThreads) void rnn_bwd_step_k(RnnStep a) {
  constexpr int G = MODE == W2L_RNN_LSTM ? 4 : MODE == W2L_RNN_GRU ? 3 : 1;
  __shared__ __attribute__((aligned(16))) float lds[kRnnBt * kRnnLd];
  __shared__ float red[4 * kRnnBt * 33];
  const int d = blockIdx.z, H = a.H, T = a.T, B = a.B, GH = G * H;
  const int j0 = blockIdx.x * 32, b0 = blockIdx.y * kRnnBt, rows = min(kRnnBt, B - b0);
  const int s = T - 1 - a.s;                       // scan index of the frame this launch differentiates
  const int t = d ? T - 1 - s : s, tp = d ? t + 1 : t - 1, tn = d ? t - 1 : t + 1;
  const bool first = s == 0, last = s == T - 1;    // no h_{t-1}; no successor
  const int li = threadIdx.x & 31;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (!last)   // dgates of the successor frame, all G H of them
    scan_product<false>(acc, lds, a.dgh[d] + ((size_t)b0 * T + tn) * GH, (size_t)T * GH, rows, GH, a.whh[d], H, j0 + li, j0 + li < H, false);
  scan_reduce(acc, red);
  for (int e = threadIdx.x; e < kRnnBt * 32; e += kRnnThreads) {
    const int b = e >> 5, u = e & 31, j = j0 + u;
    if (b >= rows || j >= H) continue;
    const size_t row = (size_t)(b0 + b) * T + t, rowp = (size_t)(b0 + b) * T + tp, bj = (size_t)(b0 + b) * H + j;
    const float* gt = a.gates[d] + row * (size_t)GH;
    float* di = a.dgi[d] + row * (size_t)GH;
    float dh = a.dy[row * a.lddy + (size_t)d * H + j] + red_sum(red, b, u);
    if (MODE == W2L_RNN_RELU) {
      di[j] = gt[j] > 0.f ? dh : 0.f;
    } else if (MODE == W2L_RNN_TANH) {
      di[j] = dh * (1.f - gt[j] * gt[j]);
    } else if (MODE == W2L_RNN_LSTM) {
      const float gi = gt[j], gf = gt[H + j], gg = gt[2 * H + j], go = gt[3 * H + j];
      const float tc = tanhf(a.cs[d][row * H + j]);
      const float cprev = first ? 0.f : a.cs[d][rowp * H + j];
      float dc = dh * go * (1.f - tc * tc);
      if (!last) dc += a.dcc[d][bj];
      di[j] = dc * gg * gi * (1.f - gi);
      di[H + j] = dc * cprev * gf * (1.f - gf);
      di[2 * H + j] = dc * gi * (1.f - gg * gg);
      di[3 * H + j] = dh * tc * go * (1.f - go);
      a.dcc[d][bj] = dc * gf;
    } else {
      const float gr = gt[j], gz = gt[H + j], gn = gt[2 * H + j], hn = a.hn[d][row * H + j];
      const float hprev = first ? 0.f : a.y[rowp * a.ldy + (size_t)d * H + j];
      if (!last) dh += a.dhc[d][bj];
      const float dn = dh * (1.f - gz) * (1.f - gn * gn);
      const float dz = dh * (hprev - gn) * gz * (1.f - gz);
      const float dr = dn * hn * gr * (1.f - gr);
      float* dg = a.dgh[d] + row * (size_t)GH;
      di[j] = dr; di[H + j] = dz; di[2 * H + j] = dn;
      dg[j] = dr; dg[H + j] = dz; dg[2 * H + j] = dn * gr;
      a.dhc[d][bj] = dh * gz;
    }
  }
}

// ---- host side: parameter and workspace layout ------------------------------------------------------------------------------------
struct RnnLayout {
  int G, HD;
  size_t M;
  // float offsets into the workspace
  size_t act[kRnnMaxLayers], xd[kRnnMaxLayers];   // output of layer l (l < layers - 1); dropped copy of the input of layer l (l > 0)
  size_t gates[kRnnMaxLayers][2], cs[kRnnMaxLayers][2], hn[kRnnMaxLayers][2], hp[kRnnMaxLayers][2];
  size_t dgi[2], dgh[2], dhc[2], dcc[2], dact[2];
  size_t total;
};

static inline size_t rnn_in(const w2l_rnn_desc& d, int l) { return l == 0 ? (size_t)d.I : (size_t)d.H * d.dirs; }

// 0 ok, else the refusal
static int rnn_check(const w2l_rnn_desc* d) {
  if (!d) return W2L_EINVAL;
  if (d->mode < W2L_RNN_RELU || d->mode > W2L_RNN_GRU || d->I < 1 || d->H < 1 || d->layers < 1 || d->dirs < 1 || d->dirs > 2 || d->B < 1 ||
      d->T < 1 || d->ldx < d->I || d->ldy < d->H * d->dirs || !(d->dropP >= 0.0 && d->dropP < 1.0))
    return W2L_EINVAL;
  if (d->I > kRnnMaxDim || d->H > kRnnMaxDim || d->B > kRnnMaxB || d->layers > kRnnMaxLayers || d->T > kRnnMaxT) return W2L_EUNSUPPORTED;
  const unsigned long long M = (unsigned long long)d->B * d->T;
  const unsigned long long widest = std::max<unsigned long long>({4ull * d->H, (unsigned long long)d->ldx, (unsigned long long)d->ldy});
  if (M * widest >= 0x7fffffffull) return W2L_EUNSUPPORTED;   // the products index their operands with ints
  return W2L_OK;
}

static RnnLayout rnn_layout(const w2l_rnn_desc& d) {
  RnnLayout L{};
  L.G = rnn_gates(d.mode); L.HD = d.H * d.dirs; L.M = (size_t)d.B * d.T;
  size_t at = 0;
  auto take = [&](size_t n) { size_t o = at; at += (n + 63) / 64 * 64; return o; };
  const bool train = d.train != 0, lstm = d.mode == W2L_RNN_LSTM, gru = d.mode == W2L_RNN_GRU;
  // evaluation keeps nothing per layer: two activation buffers in turn, one set of scan buffers
  for (int l = 0; l < d.layers; ++l) {
    const bool fresh = train || l < 2;
    if (l < d.layers - 1) L.act[l] = fresh ? take(L.M * L.HD) : L.act[l - 2];
    if (l > 0 && train && d.dropP > 0) L.xd[l] = take(L.M * L.HD);
    for (int k = 0; k < d.dirs; ++k) {
      const bool own = train || l == 0;
      L.gates[l][k] = own ? take(L.M * L.G * d.H) : L.gates[0][k];
      if (lstm) L.cs[l][k] = own ? take(L.M * d.H) : L.cs[0][k];
      if (gru && train) L.hn[l][k] = take(L.M * d.H);
      if (train) L.hp[l][k] = take(L.M * d.H);
    }
  }
  if (train) {
    for (int k = 0; k < d.dirs; ++k) {
      L.dgi[k] = take(L.M * L.G * d.H);
      L.dgh[k] = gru ? take(L.M * L.G * d.H) : L.dgi[k];
      if (gru) L.dhc[k] = take((size_t)d.B * d.H);
      if (lstm) L.dcc[k] = take((size_t)d.B * d.H);
    }
    if (d.layers > 1) { L.dact[0] = take(L.M * L.HD); L.dact[1] = take(L.M * L.HD); }
  }
  L.total = at;
  return L;
}

// parameters of (layer, direction): W_ih [G H][I_l], W_hh [G H][H], b_ih [G H], b_hh [G H]
struct RnnParams { size_t wih, whh, bih, bhh; };
static RnnParams rnn_params(const w2l_rnn_desc& d, int l, int dir) {
  const size_t GH = (size_t)rnn_gates(d.mode) * d.H;
  size_t at = 0;
  for (int i = 0; i < l; ++i) at += d.dirs * GH * (rnn_in(d, i) + d.H + 2);
  at += dir * GH * (rnn_in(d, l) + d.H + 2);
  RnnParams p;
  p.wih = at; p.whh = p.wih + GH * rnn_in(d, l); p.bih = p.whh + GH * d.H; p.bhh = p.bih + GH;
  return p;
}

static inline uint32_t rnn_layer_seed(uint32_t seed, int l) { return seed ^ (0x9E3779B9u * (uint32_t)l); }

template <int MODE>
static int rnn_launch(bool bwd, const RnnStep& a, int dirs, hipStream_t s) {
  constexpr int G = MODE == W2L_RNN_LSTM ? 4 : MODE == W2L_RNN_GRU ? 3 : 1;
  const int J = bwd ? 32 : 32 / G;
  const dim3 grid((a.H + J - 1) / J, (a.B + kRnnBt - 1) / kRnnBt, dirs);
  if (bwd) rnn_bwd_step_k<MODE><<<grid, kRnnThreads, 0, s>>>(a);
  else rnn_fwd_step_k<MODE><<<grid, kRnnThreads, 0, s>>>(a);
  W2L_LAUNCH_CHECK();
  return W2L_OK;
}
static int rnn_step(int mode, bool bwd, const RnnStep& a, int dirs, hipStream_t s) {
  switch (mode) {
    case W2L_RNN_RELU: return rnn_launch<W2L_RNN_RELU>(bwd, a, dirs, s);
    case W2L_RNN_TANH: return rnn_launch<W2L_RNN_TANH>(bwd, a, dirs, s);
    case W2L_RNN_LSTM: return rnn_launch<W2L_RNN_LSTM>(bwd, a, dirs, s);
    default: return rnn_launch<W2L_RNN_GRU>(bwd, a, dirs, s);
  }
}

#define RNN_OK(expr) do { const int _st = (expr); if (_st != W2L_OK) return _st; } while (0)

}  // namespace w2l

using namespace w2l;

W2L_API size_t w2l_rnn_param_count(const w2l_rnn_desc* d) {
  if (!d || d->mode < W2L_RNN_RELU || d->mode > W2L_RNN_GRU || d->I < 1 || d->H < 1 || d->layers < 1 || d->dirs < 1 || d->dirs > 2) return 0;
  const RnnParams p = rnn_params(*d, d->layers, 0);
  return p.wih;
}

W2L_API size_t w2l_rnn_workspace_size(const w2l_rnn_desc* d) {
  if (rnn_check(d) != W2L_OK) return 0;
  return rnn_layout(*d).total * sizeof(float);
}

W2L_API int w2l_rnn_forward(const w2l_rnn_desc* d, const float* x, const float* params, float* y, void* workspace, size_t workspaceBytes,
                            w2l_stream_t stream) {
  RNN_OK(rnn_check(d));
  if (!x || !params || !y || !workspace) return W2L_EINVAL;
  const RnnLayout L = rnn_layout(*d);
  if (workspaceBytes < L.total * sizeof(float)) return W2L_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int H = d->H, GH = L.G * H, M = (int)L.M;
  for (int l = 0; l < d->layers; ++l) {
    const float* in = l == 0 ? x : ws + L.act[l - 1];
    const int ldin = l == 0 ? d->ldx : L.HD, Il = (int)rnn_in(*d, l);
    if (l > 0 && d->train && d->dropP > 0) {
      RNN_OK(w2l_dropout_copy(ws + L.xd[l], in, L.M * L.HD, d->dropP, rnn_layer_seed(d->seed, l), d->rngStream, stream));
      in = ws + L.xd[l];
    }
    RnnStep a{};
    a.y = l == d->layers - 1 ? y : ws + L.act[l];
    a.ldy = l == d->layers - 1 ? d->ldy : L.HD;
    a.B = d->B; a.T = d->T; a.H = H; a.train = d->train != 0;
    for (int k = 0; k < d->dirs; ++k) {
      const RnnParams p = rnn_params(*d, l, k);
      a.whh[k] = params + p.whh; a.bhh[k] = params + p.bhh;
      a.gates[k] = ws + L.gates[l][k]; a.cs[k] = ws + L.cs[l][k]; a.hn[k] = ws + L.hn[l][k]; a.hp[k] = ws + L.hp[l][k];
      // pre-activations of every frame: X [M][I_l] . W_ih^T + b_ih
      RNN_OK(gemm_f32(in, ldin, 1, params + p.wih, Il, 1, GemmOut{a.gates[k], params + p.bih, M, GH, Il, GH, EPI_BIAS}, s));
    }
    for (a.s = 0; a.s < d->T; ++a.s) RNN_OK(rnn_step(d->mode, false, a, d->dirs, s));
  }
  return W2L_OK;
}

W2L_API int w2l_rnn_backward(const w2l_rnn_desc* d, const float* x, const float* params, const float* y, const float* dy, float* dx,
                             float* dparams, void* workspace, size_t workspaceBytes, w2l_stream_t stream) {
  RNN_OK(rnn_check(d));
  if (!x || !params || !y || !dy || !dparams || !workspace || !d->train) return W2L_EINVAL;
  const RnnLayout L = rnn_layout(*d);
  if (workspaceBytes < L.total * sizeof(float)) return W2L_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int H = d->H, GH = L.G * H, M = (int)L.M;
  for (int l = d->layers - 1; l >= 0; --l) {
    const bool top = l == d->layers - 1;
    const float* in = l == 0 ? x : ws + ((d->dropP > 0) ? L.xd[l] : L.act[l - 1]);
    const int ldin = l == 0 ? d->ldx : L.HD, Il = (int)rnn_in(*d, l);
    RnnStep a{};
    a.y = const_cast<float*>(top ? y : ws + L.act[l]);
    a.ldy = top ? d->ldy : L.HD;
    a.dy = top ? dy : ws + L.dact[(d->layers - 1 - l) & 1];
    a.lddy = top ? d->ldy : L.HD;
    a.B = d->B; a.T = d->T; a.H = H; a.train = 1;
    for (int k = 0; k < d->dirs; ++k) {
      const RnnParams p = rnn_params(*d, l, k);
      a.whh[k] = params + p.whh; a.bhh[k] = params + p.bhh;
      a.gates[k] = ws + L.gates[l][k]; a.cs[k] = ws + L.cs[l][k]; a.hn[k] = ws + L.hn[l][k]; a.hp[k] = ws + L.hp[l][k];
      a.dgi[k] = ws + L.dgi[k]; a.dgh[k] = ws + L.dgh[k]; a.dhc[k] = ws + L.dhc[k]; a.dcc[k] = ws + L.dcc[k];
    }
    for (a.s = 0; a.s < d->T; ++a.s) RNN_OK(rnn_step(d->mode, true, a, d->dirs, s));
    float* dIn = l == 0 ? dx : ws + L.dact[(d->layers - l) & 1];
    const int lddin = l == 0 ? d->ldx : L.HD;
    for (int k = 0; k < d->dirs; ++k) {
      const RnnParams p = rnn_params(*d, l, k);
      // dW_ih [G H][I_l] = dgi^T X;  dW_hh [G H][H] = dgh^T hp (hp is zero where the scan starts);  the bias gradients are column sums
      RNN_OK(gemm_f32(a.dgi[k], GH, 0, in, ldin, 0, GemmOut{dparams + p.wih, nullptr, GH, Il, M, Il, 0}, s));
      RNN_OK(gemm_f32(a.dgh[k], GH, 0, a.hp[k], H, 0, GemmOut{dparams + p.whh, nullptr, GH, H, M, H, 0}, s));
      RNN_OK(colsum(a.dgi[k], dparams + p.bih, L.M, GH, s));
      RNN_OK(colsum(a.dgh[k], dparams + p.bhh, L.M, GH, s));
      // dX [M][I_l] = sum over directions dgi . W_ih
      if (dIn) RNN_OK(gemm_f32(a.dgi[k], GH, 1, params + p.wih, Il, 0, GemmOut{dIn, nullptr, M, Il, GH, lddin, k ? EPI_ACCUM : 0}, s));
    }
    if (l > 0 && d->dropP > 0)
      RNN_OK(w2l_dropout_inplace(dIn, L.M * L.HD, d->dropP, rnn_layer_seed(d->seed, l), d->rngStream, stream));
  }
  return W2L_OK;
}
