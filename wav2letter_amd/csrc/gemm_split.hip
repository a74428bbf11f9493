// gemm_split.hip -- the split-bf16 GEMM of gemm_split.hpp as a translation unit of its own: built without packed fp32 arithmetic
// (Makefile), which the kernels of gemm.hip keep.  gemm.hip's dispatch and w2l_gemm_f32_split call gemm_split().
#include "gemm_split.hpp"

namespace w2l {

int gemm_split(const float* A, int lda, int a_kcontig, const float* B, int ldb, int b_kcontig, const GemmOut& o, int epi, hipStream_t s) {
  if (o.K < 32) return W2L_EUNSUPPORTED;   // a split buys nothing there (the bf16 route has the same floor)
  const bool va = pick_vec(A, lda, a_kcontig ? o.K : o.M) == 4, vb = pick_vec(B, ldb, b_kcontig ? o.K : o.N) == 4;
  if (a_kcontig) {
    const split::Op<true> a{A, lda, o.M, o.K, va};
    if (b_kcontig) return split::launch128(a, split::Op<true>{B, ldb, o.N, o.K, vb}, o, epi, s);
    return split::launch128(a, split::Op<false>{B, ldb, o.N, o.K, vb}, o, epi, s);
  }
  const split::Op<false> a{A, lda, o.M, o.K, va};
  if (b_kcontig) return split::launch128(a, split::Op<true>{B, ldb, o.N, o.K, vb}, o, epi, s);
  return split::launch128(a, split::Op<false>{B, ldb, o.N, o.K, vb}, o, epi, s);
}

}  // namespace w2l
