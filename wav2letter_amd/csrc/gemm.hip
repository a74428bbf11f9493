// gemm.hip -- fp32 MFMA GEMM engine for gfx950 (v_mfma_f32_32x32x2_f32 / 16x16x4_f32).
//
// Replaces the cuBLAS / cuDNN calls behind fl::Linear and fl::Conv2D in the
// reference's training step (fl::linear / fl::conv2d autograd functions,
// un-vendored Flashlight; instantiated by the arch grammar in
// recipes/joint_training_vox_populi/cpc/SequentialBuilder.cpp:203-252, :305-313):
//   forward      Y = X W + b            (A k-contiguous, B k-rows)
//   backward dX  dX = dY W^T            (A k-contiguous, B k-contiguous)
//   backward dW  dW = X^T dY            (A k-rows,       B k-rows)
// and, through the implicit-GEMM operand in conv.hip, the time convolutions.
//
// fp32 in / fp32 accumulate MFMA is bit-for-bit a k-ordered fmaf chain
// (cdna_hip_programming.md section 3), so results are within fp32 round-off of
// the fp64 oracle (parity bar 1e-4).  Peak is 157.3 TFLOP/s.
//
// Dispatch.  gemm_f32 (every w2l_linear_* product, w2l_gemm_f32, the dA product of criterion_fcc_big.hip) sends a product
// C[M][N] = op(A) op(B) to the first line whose conditions hold -- this comment is the one place where the order is written down:
//   1. launch128_bf16   gemm_bf16.hpp     w2l_set_matmul_precision(1) is in force and K >= 32: fp32 operands in memory, bf16 multiply
//   2. (ragged K)                         K % 32 != 0, K >= 256, no bias / epilogue, operands LDS-DMA eligible (dX of the final
//                                         layer, K = 9998): the whole K tiles go through lines 3 - 4, the K % 32 tail through
//                                         line 5, accumulated into C
//   3. launch160        gemm_t160.hpp     K % 32 == 0, operands LDS-DMA eligible and below 2 GiB, N % 4 == 0, C / mask / addend
//                                         16-byte aligned with ldc % 4 == 0, a 128 x 160 or 160 x 128 tiling saves >= 2 % of the
//                                         128 x 128 grid's padded area (t160_choice: every TDS fc shape), <= 1024 stream-K tiles.
//                                         gemm160_kernel; with k-row operands it also delivers GemmOut::colsum (the bias gradient)
//   4. launch128g       gemm_glds.hpp     K % 32 == 0, operands LDS-DMA eligible.  gemm128g_kernel: buffer-addressed instances
//                                         when both operands are below 2 GiB, 64-bit global_load_lds instances otherwise
//   5. launch128        gemm.hpp          everything else: gemm128_kernel, register-staged operands of any alignment, any K
// LDS-DMA eligible (glds_ok / glds_ok_relaxed below): both operands 16-byte aligned with ld % 4 == 0 and extent % 4 == 0 (strict),
// or both dword aligned with extent >= 4 and below 2 GiB (relaxed: N = 9998).  Lines 3 - 5 cut K by the stream-K schedule of
// gemm.hpp (make_sk_plan); 3 and 4 add the partial tiles inside the launch (g_slab_handover), 5 in a fix-up launch.
// Other entries: gemm_glds_raw (conv.hip's overlapping-row operand views: lines 3 - 4 only, else W2L_EUNSUPPORTED); conv.hip's
// implicit-GEMM operands call launch128 / launch_skinny (N <= 32) directly; the bf16-OPERAND products (w2l_gemm_bf16*,
// gemm_bf16_images) go to launch128h of gemm_bf16g.hpp, which picks gemm128h_kernel or gemm256h_kernel per shape.
// Probe library: W2L_GEMM_GLDS=0 sends everything to line 5, W2L_GEMM_T160=0 / 2 / 3 never takes line 3 / takes it whenever
// eligible / with the 160 x 128 tile, W2L_GEMM_INFIX=0 gives line 4 the fix-up launch of line 5 (tests compare the kernels so).
#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

#include "gemm.hpp"
#include "gemm_glds.hpp"
#include "gemm_t160.hpp"
#include "gemm_bf16.hpp"
#include "gemm_bf16g.hpp"

namespace w2l {

GemmProf& gemm_prof() {
  static GemmProf p;
  return p;
}
bool profileEnabled() { return gemm_prof().on; }   // read by host/net.cpp: bracketed launches stay on one stream

// stream-K partial-tile slabs: library-owned, ONE buffer per stream (work on a stream is
// serialised, so launches on the same stream may share it); allocated on first use.
float* sk_scratch(hipStream_t s, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, std::pair<float*, size_t>> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  auto& e = cache[{dev, s}];
  if (e.second < bytes) {
    if (e.first) (void)hipFree(e.first);
    e.first = nullptr;
    e.second = 0;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    e.first = (float*)p;
    e.second = bytes;
  }
  return e.first;
}

// W2L_GEMM_GLDS=0 routes every GEMM through the register-staged first-generation kernel (A/B runs)
static bool glds_enabled() {
  const char* e = tune_env("W2L_GEMM_GLDS");
  return !(e && e[0] == '0');
}

// Eligibility of an operand for the LDS-DMA kernels.  Strict: 16-byte aligned rows whose extent is a multiple of 4.
static inline bool glds_ok(const float* p, int ld, int extent) {
  return (((uintptr_t)p) & 15) == 0 && ld % 4 == 0 && extent % 4 == 0 && extent >= 4;
}
// Relaxed (buffer-addressed instances only, so the operand must also be below 2 GiB): dword-aligned rows are enough for
// `buffer_load_dwordx4 ... lds` (odd leading dimensions included; measured: r01_run45), and the extent of a k-row operand need
// not be a multiple of 4 -- a chunk that straddles a row end brings in the first floats of the next row (zeros past the end of
// the buffer: num_records bounds the resource), which only feed columns >= N that no epilogue stores.  This is what N = 9998
// needs (final fl::Linear of the TDS-CTC recipe, dA of the ASG stress shape).
static inline bool glds_ok_relaxed(const float* p, int extent) {
  return (((uintptr_t)p) & 3) == 0 && extent >= 4;
}

unsigned* sk_counters(hipStream_t s) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, unsigned*> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  unsigned*& e = cache[{dev, s}];
  if (!e) {
    void* p = nullptr;
    if (hipMalloc(&p, 1024 * sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, 1024 * sizeof(unsigned)) != hipSuccess) { (void)hipFree(p); return nullptr; }
    e = (unsigned*)p;
  }
  return e;
}

// the two first-use allocations of a stream, ahead of the launches that need them (host/net.cpp: when a net takes its
// weight-gradient stream, for that stream and the caller's -- not in a later, possibly timed, step)
void warmStreamScratch(hipStream_t s) {
  (void)sk_scratch(s, kSkScratchBytes);
  (void)sk_counters(s);
}

template <class AOp>
static int dispatch_b(const AOp& a, const float* B, int ldb, int b_kcontig, const GemmOut& o, int epi, hipStream_t s) {
  if (b_kcontig) {
    int v = pick_vec(B, ldb, o.K);
    if (v == 4) return launch128(a, PlainOp<true, 4>{B, ldb, o.N, o.K}, o, epi, s);
    if (v == 2) return launch128(a, PlainOp<true, 2>{B, ldb, o.N, o.K}, o, epi, s);
    return launch128(a, PlainOp<true, 1>{B, ldb, o.N, o.K}, o, epi, s);
  }
  int v = pick_vec(B, ldb, o.N);
  if (v == 4) return launch128(a, PlainOp<false, 4>{B, ldb, o.N, o.K}, o, epi, s);
  if (v == 2) return launch128(a, PlainOp<false, 2>{B, ldb, o.N, o.K}, o, epi, s);
  return launch128(a, PlainOp<false, 1>{B, ldb, o.N, o.K}, o, epi, s);
}

// ---- mixed precision (BASELINE config 3): w2l_set_matmul_precision(1) routes the fl::Linear GEMMs through the
// bf16-multiply / fp32-accumulate kernel of gemm_bf16.hpp; operands and results stay fp32 in memory
static std::atomic<int> g_matmul_bf16{0};

static int gemm_bf16(const float* A, int lda, int a_kcontig, const float* B, int ldb, int b_kcontig, const GemmOut& o, int epi,
                     hipStream_t s) {
  const bool va = pick_vec(A, lda, a_kcontig ? o.K : o.M) == 4, vb = pick_vec(B, ldb, b_kcontig ? o.K : o.N) == 4;
  if (a_kcontig) {
    const BfOp<true> a{A, lda, o.M, o.K, va};
    if (b_kcontig) return launch128_bf16(a, BfOp<true>{B, ldb, o.N, o.K, vb}, o, epi, s);
    return launch128_bf16(a, BfOp<false>{B, ldb, o.N, o.K, vb}, o, epi, s);
  }
  const BfOp<false> a{A, lda, o.M, o.K, va};
  if (b_kcontig) return launch128_bf16(a, BfOp<true>{B, ldb, o.N, o.K, vb}, o, epi, s);
  return launch128_bf16(a, BfOp<false>{B, ldb, o.N, o.K, vb}, o, epi, s);
}

int gemm_f32(const float* A, int lda, int a_kcontig, const float* B, int ldb, int b_kcontig, GemmOut o, hipStream_t s,
             bool* colsumDone) {
  const int M = o.M, N = o.N, K = o.K;
  if (colsumDone) *colsumDone = false;
  if (M <= 0 || N <= 0 || K <= 0 || !A || !B || !o.C) return W2L_EINVAL;
  const int epi = gemm_epi(o);
  float* const colsumOut = o.colsum;   // only the 160-wide LDS-DMA kernel produces it (below)
  o.colsum = nullptr;
  if (g_matmul_bf16.load(std::memory_order_relaxed) && K >= 32) return gemm_bf16(A, lda, a_kcontig, B, ldb, b_kcontig, o, epi, s);
  // address range of each operand in bytes (the buffer-addressed instances need 32-bit offsets)
  const unsigned long long ab = 4ull * (a_kcontig ? (unsigned long long)(M - 1) * lda + K : (unsigned long long)(K - 1) * lda + M);
  const unsigned long long bb = 4ull * (b_kcontig ? (unsigned long long)(N - 1) * ldb + K : (unsigned long long)(K - 1) * ldb + N);
  const bool strict = glds_ok(A, lda, M) && glds_ok(B, ldb, N);
  const bool relaxed = !strict && glds_ok_relaxed(A, M) && glds_ok_relaxed(B, N) && ab < 0x7fffffffull && bb < 0x7fffffffull;
  const bool glds = glds_enabled() && (strict || relaxed);
  if (glds && K % 32 != 0 && K >= 256 && epi == 0 && !o.bias) {
    // reduction length not a multiple of the K tile (dX of the final layer: K = 9998): whole K tiles on the LDS-DMA
    // kernel, the tail of K % 32 columns through the register-staged kernel, accumulated into C
    const int K0 = K & ~31;
    int st = gemm_f32(A, lda, a_kcontig, B, ldb, b_kcontig, GemmOut{o.C, nullptr, M, N, K0, o.ldc, 0}, s);
    if (st != W2L_OK) return st;
    const float* A1 = a_kcontig ? A + K0 : A + (size_t)K0 * lda;
    const float* B1 = b_kcontig ? B + K0 : B + (size_t)K0 * ldb;
    return gemm_f32(A1, lda, a_kcontig, B1, ldb, b_kcontig, GemmOut{o.C, nullptr, M, N, K - K0, o.ldc, EPI_ACCUM}, s);
  }
  if (glds && K % 32 == 0) {
    GOp ga{A, lda, M, ab < 0x7fffffffull ? (unsigned)ab : 0u}, gb{B, ldb, N, bb < 0x7fffffffull ? (unsigned)bb : 0u};
    // 160-wide tiles where 128 leaves a ragged last tile column / row (every TDS fc shape: gemm_t160.hpp)
    o.colsum = colsumOut;
    if (const int which = t160_choice(ga, gb, o)) {
      bool launched = false;
      const int st = launch160(ga, a_kcontig != 0, gb, b_kcontig != 0, o, epi, which, s, &launched, colsumDone);
      if (st != W2L_OK || launched) return st;
    }
    o.colsum = nullptr;
    return launch128g(ga, a_kcontig != 0, gb, b_kcontig != 0, o, epi, s);
  }
  if (a_kcontig) {
    int v = pick_vec(A, lda, K);
    if (v == 4) return dispatch_b(PlainOp<true, 4>{A, lda, M, K}, B, ldb, b_kcontig, o, epi, s);
    if (v == 2) return dispatch_b(PlainOp<true, 2>{A, lda, M, K}, B, ldb, b_kcontig, o, epi, s);
    return dispatch_b(PlainOp<true, 1>{A, lda, M, K}, B, ldb, b_kcontig, o, epi, s);
  }
  int v = pick_vec(A, lda, M);
  if (v == 4) return dispatch_b(PlainOp<false, 4>{A, lda, M, K}, B, ldb, b_kcontig, o, epi, s);
  if (v == 2) return dispatch_b(PlainOp<false, 2>{A, lda, M, K}, B, ldb, b_kcontig, o, epi, s);
  return dispatch_b(PlainOp<false, 1>{A, lda, M, K}, B, ldb, b_kcontig, o, epi, s);
}

// LDS-DMA GEMM on operand VIEWS prepared by the caller (overlapping-row convolution operands, conv.hip): no K % 32 or
// alignment requirement beyond dword-aligned pointers.  K is rounded up to whole K tiles; the caller guarantees that
// what the last K tile reads past K is either finite in-bounds data that meets zeros of the other operand, or lies
// outside the operand's byte range (buffer addressing returns zeros).  W2L_EUNSUPPORTED: operand >= 2 GiB.
int gemm_glds_raw(const float* A, int lda, bool akc, size_t aBytes, const float* B, int ldb, bool bkc, size_t bBytes,
                  GemmOut o, int epi, hipStream_t s) {
  if (!glds_enabled()) return W2L_EUNSUPPORTED;
  if (aBytes >= 0x7fffffffull || bBytes >= 0x7fffffffull || ((uintptr_t)A & 3) || ((uintptr_t)B & 3)) return W2L_EUNSUPPORTED;
  GOp ga{A, lda, o.M, (unsigned)aBytes}, gb{B, ldb, o.N, (unsigned)bBytes};
  if (const int which = t160_choice(ga, gb, o)) {
    bool launched = false;
    const int st = launch160(ga, akc, gb, bkc, o, epi, which, s, &launched);
    if (st != W2L_OK || launched) return st;
  }
  return launch128g(ga, akc, gb, bkc, o, epi, s);
}

}  // namespace w2l

using namespace w2l;

// 0 = fp32 MFMA (default), 1 = bf16 multiply / fp32 accumulate for every w2l_linear_* / w2l_gemm_f32 call of this
// process from now on; returns the previous mode.  (fl's --fl_amp_use_mixed_precision, restated for bf16.)
W2L_API int w2l_set_matmul_precision(int mode) { return g_matmul_bf16.exchange(mode ? 1 : 0); }

namespace w2l {
bool matmul_bf16_mode() { return g_matmul_bf16.load(std::memory_order_relaxed) != 0; }
// the bf16-image GEMM for other translation units (conv.hip: overlapping-row operand views)
int gemm_bf16_images(const uint16_t* A, int lda, unsigned long long aView, const uint16_t* B, int ldb, unsigned long long bView,
                     const GemmOut& o, int epi, hipStream_t s, bool aKMajor, bool bKMajor) {
  return launch128h(A, lda, B, ldb, o, epi, s, aView, bView, aKMajor, bKMajor);
}
}  // namespace w2l

// ---- C ABI: fl::linear forward / backward ----------------------------------
// the forward product y[M][out] = x[M][in] . w[in][out] (+ bias) (relu): A k-contiguous, B k-rows
static GemmOut linear_forward_out(int M, int in, int out, const float* bias, float* y, int relu) {
  return GemmOut{y, bias, M, out, in, out, (bias ? EPI_BIAS : 0) | (relu ? EPI_RELU : 0)};
}
static void set_dropout(GemmOut& o, double p, uint32_t seed, uint32_t rngStream) {
  o.dropThr = dropout_threshold(p);
  o.dropSeed = seed; o.dropStream = rngStream;
  o.dropScale = (float)(1.0 / (1.0 - p));
}

W2L_API int w2l_linear_forward(int M, int in, int out, const float* x, const float* w,
                               const float* bias, float* y, int relu, w2l_stream_t stream) {
  return gemm_f32(x, in, 1, w, out, 0, linear_forward_out(M, in, out, bias, y, relu), (hipStream_t)stream);
}

W2L_API int w2l_linear_backward_data(int M, int in, int out, const float* dy, const float* w,
                                     float* dx, int accumulate, const float* maskSrc, float maskScale,
                                     w2l_stream_t stream) {
  // dx[M][in] = dy[M][out] . w[in][out]^T : reduction over `out`, both operands k-contiguous.
  // maskSrc (optional, [M][in]): dx = maskSrc > 0 ? dx * maskScale : 0 -- the ReLU(+dropout)
  // backward of the layer that produced this Linear's input, fused into the epilogue.
  GemmOut o{dx, nullptr, M, in, out, in, accumulate ? EPI_ACCUM : 0};
  o.mask = maskSrc;
  o.maskScale = maskScale;
  return gemm_f32(dy, out, 1, w, out, 1, o, (hipStream_t)stream);
}

// y = dropout(relu?(x w + b)): the dropout of fl::Dropout behind a Linear(+ReLU) folded into the GEMM epilogue; the
// mask is the library's stateless hash of (flat index m * out + n, seed, rngStream) -- bit-identical to
// w2l_linear_forward followed by w2l_dropout_inplace over y, one pass over y fewer
W2L_API int w2l_linear_forward_dropout(int M, int in, int out, const float* x, const float* w, const float* bias,
                                       float* y, int relu, double p, uint32_t seed, uint32_t rngStream,
                                       w2l_stream_t stream) {
  GemmOut o = linear_forward_out(M, in, out, bias, y, relu);
  set_dropout(o, p, seed, rngStream);
  return gemm_f32(x, in, 1, w, out, 0, o, (hipStream_t)stream);
}

// y = dropout(relu?(x w + b)) + add (add has y's layout; p = 0: no dropout): the residual join behind a Linear in the GEMM epilogue,
// bit-identical to w2l_linear_forward_dropout followed by an elementwise add -- fl::TDSBlock's r2 = dropout(lin2(.)) + y1
W2L_API int w2l_linear_forward_dropout_add(int M, int in, int out, const float* x, const float* w, const float* bias,
                                           const float* add, float* y, int relu, double p, uint32_t seed, uint32_t rngStream,
                                           w2l_stream_t stream) {
  if (!add) return W2L_EINVAL;
  GemmOut o = linear_forward_out(M, in, out, bias, y, relu);
  o.addend = add;
  set_dropout(o, p, seed, rngStream);
  return gemm_f32(x, in, 1, w, out, 0, o, (hipStream_t)stream);
}

// dx = add + dy w^T (add has dx's layout): the residual join of a backward pass without a copy of `add` into dx first
W2L_API int w2l_linear_backward_data_add(int M, int in, int out, const float* dy, const float* w, const float* add,
                                         float* dx, w2l_stream_t stream) {
  if (!add) return W2L_EINVAL;
  GemmOut o{dx, nullptr, M, in, out, in, 0};
  o.addend = add;
  return gemm_f32(dy, out, 1, w, out, 1, o, (hipStream_t)stream);
}

W2L_API int w2l_linear_backward_weight(int M, int in, int out, const float* x, const float* dy,
                                       float* dw, w2l_stream_t stream) {
  // dw[in][out] = x[M][in]^T . dy[M][out] : reduction over M, both operands k-rows.
  // The output is small (in x out) and the reduction long: the stream-K schedule splits K.
  return gemm_f32(x, in, 0, dy, out, 0, GemmOut{dw, nullptr, in, out, M, out, 0}, (hipStream_t)stream);
}

// the same product with the bias gradient db[out] = sum_m dy[m][out] (fl::Linear's two parameter gradients).  On the 160-wide
// LDS-DMA kernel the column sums ride on the product (the first tile row adds up the dy fragments it multiplies: no extra pass
// over dy); any other kernel is followed by the column-sum launch -- the same values either way up to the summation order.
W2L_API int w2l_linear_backward_weight_bias(int M, int in, int out, const float* x, const float* dy, float* dw, float* db,
                                            w2l_stream_t stream) {
  if (!db) return w2l_linear_backward_weight(M, in, out, x, dy, dw, stream);
  hipStream_t s = (hipStream_t)stream;
  GemmOut o{dw, nullptr, in, out, M, out, 0};
  o.colsum = db;
  bool colsumDone = false;
  const int st = gemm_f32(x, in, 0, dy, out, 0, o, s, &colsumDone);
  if (st != W2L_OK || colsumDone) return st;
  return colsum(dy, db, (size_t)M, out, s);
}

// ---- mixed precision with bf16 OPERANDS in HBM (gemm_bf16g.hpp): C[M][N] (fp32) = A[M][K] . B[N][K]^T, both operands
// k-contiguous bf16 images written by w2l_bf16_convert (rows zero-padded to a multiple of 64 k), fp32 accumulation and the
// fp32 engine's epilogue: bias[n], ReLU, dropout, mask, addend / accumulate.  The three products of fl::Linear:
//   forward  y  = x w + b      A = x  [M][in]   (row-major image),  B = w^T  [out][in]  (transposed image of w [in][out])
//   dx       dx = dy w^T       A = dy [M][out]  (row-major image),  B = w    [in][out]  (row-major image)
//   dw       dw = x^T dy       A = x^T [in][M]  (transposed image), B = dy^T [out][M]   (transposed image), C = dw [in][out]
// the optional operands of a w2l_gemm_epilogue (may be null) as GemmOut fields; gemm_epi derives the flags.  accumulate without an
// addend means "into C itself" and has no operand, so it is an explicit flag.  (A dropP below 2^-24 has threshold 0: no
// EPI_DROPOUT, which is what the flag would compute -- nothing dropped, and the scale 1 / (1 - p) rounds to 1.f.)
static void set_epilogue(GemmOut& o, const w2l_gemm_epilogue* e, bool allowAccumulate) {
  if (!e) return;
  if (e->mask) { o.mask = e->mask; o.maskScale = e->maskScale; }
  if (e->addend) o.addend = e->addend;
  else if (e->accumulate && allowAccumulate) o.epi |= EPI_ACCUM;
  if (e->dropP > 0.0) set_dropout(o, e->dropP, e->dropSeed, e->dropStream);
}

W2L_API int w2l_gemm_bf16(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc,
                          const float* bias, int relu, const w2l_gemm_epilogue* e, w2l_stream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || !A || !B || !C) return W2L_EINVAL;
  GemmOut o{C, bias, M, N, K, ldc, (bias ? EPI_BIAS : 0) | (relu ? EPI_RELU : 0)};
  set_epilogue(o, e, true);
  return launch128h(A, lda, B, ldb, o, gemm_epi(o), (hipStream_t)stream);
}

// the same product whose RESULT leaves as the two bf16 images the next products read (w2l_bf16_image_sink: what w2l_bf16_convert
// would make of C, bit for bit) instead of, or beside, the fp32 C (C may be NULL when images are given), and whose mask operand may
// be a bf16 row-major image (maskImage [M][ldMask], > 0 test; replaces epilogue->mask): an activation that is only ever a GEMM
// operand and a ReLU / dropout mask (fl::TDSBlock's u = dropout(relu(lin1)), its gradient du; the Transformer's MLP) then lives
// ONLY as bf16 -- no fp32 copy, no conversion pass (the reference's AMP keeps it in half precision: recipes/slimIPL/src/Train.cpp:
// 209-216).  N % 4 == 0; ldc (>= N) still names the flat index m * ldc + n of the dropout hash.
W2L_API int w2l_gemm_bf16_images(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc,
                                 const float* bias, int relu, const w2l_gemm_epilogue* e, const w2l_bf16_image_sink* images,
                                 const uint16_t* maskImage, size_t ldMask, float maskScale, w2l_stream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || !A || !B || (!C && !images)) return W2L_EINVAL;
  GemmOut o{C, bias, M, N, K, ldc, (bias ? EPI_BIAS : 0) | (relu ? EPI_RELU : 0)};
  set_epilogue(o, e, C != nullptr);   // (nothing to accumulate into when only the images leave)
  if (maskImage) {
    if (o.mask) return W2L_EINVAL;
    o.maskH = maskImage; o.ldMaskH = (int)ldMask; o.maskScale = maskScale;
  }
  if (images) {
    o.imgRows = images->rowMajor; o.ldImgRows = (int)images->ldRows;
    o.imgTrans = images->transposed; o.ldImgTrans = (int)images->ldTrans;
  }
  return launch128h(A, lda, B, ldb, o, gemm_epi(o), (hipStream_t)stream);
}

// the same product with k-MAJOR operands read in place (gemm_bf16g.hpp): aKMajor: A is stored [K][lda] (an activation x
// [frames][in] as the A operand of x^T dy), bKMajor: B is stored [K][ldb] (a weight w [in][out] as the B operand of x w) --
// no transposed bf16 image of either is needed
W2L_API int w2l_gemm_bf16_ex(int M, int N, int K, const uint16_t* A, int lda, int aKMajor, const uint16_t* B, int ldb, int bKMajor, float* C,
                             int ldc, const float* bias, int relu, const w2l_gemm_epilogue* e, w2l_stream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || !A || !B || !C) return W2L_EINVAL;
  GemmOut o{C, bias, M, N, K, ldc, (bias ? EPI_BIAS : 0) | (relu ? EPI_RELU : 0)};
  set_epilogue(o, e, true);
  return launch128h(A, lda, B, ldb, o, gemm_epi(o), (hipStream_t)stream, 0, 0, aKMajor != 0, bKMajor != 0);
}

// `groups` (1 .. 4) products of ONE shape in one launch: C_g = A_g . B_g^T (+ bias_g); A, B, C, bias: host arrays of device pointers
W2L_API int w2l_gemm_bf16_grouped(int groups, int M, int N, int K, const uint16_t* const* A, int lda, const uint16_t* const* B, int ldb,
                                  float* const* C, int ldc, const float* const* bias, w2l_stream_t stream) {
  if (!A || !B || !C) return W2L_EINVAL;
  return launch128h_grouped(groups, A, lda, B, ldb, C, ldc, bias, M, N, K, (hipStream_t)stream);
}

// generic entry (tests / benchmarks): C[M][N] = op(A) op(B) (+bias)(relu)
W2L_API int w2l_gemm_f32(int M, int N, int K, const float* A, int lda, int a_kcontig, const float* B,
                         int ldb, int b_kcontig, float* C, int ldc, const float* bias, int relu,
                         int splitk, w2l_stream_t stream) {
  (void)splitk;  // kept for ABI stability: K is split by the stream-K schedule
  return gemm_f32(A, lda, a_kcontig, B, ldb, b_kcontig, GemmOut{C, bias, M, N, K, ldc, (bias ? EPI_BIAS : 0) | (relu ? EPI_RELU : 0)},
                  (hipStream_t)stream);
}

// ---- launch profiling (see gemm.hpp): kind 0 = 128x128 MFMA GEMM (+ stream-K fix-up), 1 = skinny
// implicit-GEMM, 2 = TDS slab convolutions, 3 = FCC transition stream (work = bytes) ----------------
W2L_API int w2l_profile_enable(int on) {
  GemmProf& p = gemm_prof();
  p.on = on != 0;
  p.used = 0;
  p.work.clear();
  p.kind.clear();
  p.dims.clear();
  return W2L_OK;
}
// per-launch rows of one kind (after a device synchronisation): ms[i], work[i], dims[4 i .. 4 i + 3] = M, N, K, kernel tag (see
// prof_begin); returns the number of rows of that kind (rows beyond maxRows are counted, not written)
W2L_API int w2l_profile_launches(int kind, int maxRows, double* ms, double* work, int* dims) {
  GemmProf& p = gemm_prof();
  int n = 0;
  for (size_t i = 0; i + 1 < p.used; i += 2) {
    if (kind >= 0 && p.kind[i / 2] != kind) continue;
    float t = 0.f;
    if (hipEventElapsedTime(&t, p.ev[i], p.ev[i + 1]) != hipSuccess) continue;
    if (n < maxRows) {
      if (ms) ms[n] = t;
      if (work) work[n] = p.work[i / 2];
      if (dims)
        for (int k = 0; k < 4; ++k) dims[4 * n + k] = p.dims[4 * (i / 2) + k];
    }
    ++n;
  }
  return n;
}
// call after a device synchronisation: launches, total ms, total algorithmic work of one kind
W2L_API int w2l_profile_report_kind(int kind, int* launches, double* totalMs, double* totalWork) {
  GemmProf& p = gemm_prof();
  double ms = 0, wk = 0;
  int n = 0;
  for (size_t i = 0; i + 1 < p.used; i += 2) {
    if (kind >= 0 && p.kind[i / 2] != kind) continue;
    float t = 0.f;
    if (hipEventElapsedTime(&t, p.ev[i], p.ev[i + 1]) != hipSuccess) continue;
    ms += t;
    wk += p.work[i / 2];
    ++n;
  }
  if (launches) *launches = n;
  if (totalMs) *totalMs = ms;
  if (totalWork) *totalWork = wk;
  return W2L_OK;
}
W2L_API int w2l_profile_report(int* launches, double* totalMs, double* totalFlops) {
  return w2l_profile_report_kind(PROF_GEMM128, launches, totalMs, totalFlops);
}
