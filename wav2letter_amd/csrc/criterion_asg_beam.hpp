// criterion_asg_beam.hpp -- w2l_asg_beam_search and w2l_asg_beam_search_lex: the beam searches of an ASG model (contract:
// include/w2l_hip.h).  Included at the end of criterion_ctc.hip after the three CTC beam headers.  An ASG lattice is the CTC one
// with three changes -- no blank, one transition term per step, no token after itself -- and all three are the policy BeamAsg of
// the two workgroup scans: ctc_beam_lm_scan<., ., BeamAsg> (lexicon-free; a null LM means none) and ctc_beam_lex_scan<., .,
// BeamAsg>.  In the scans' terms an ASG entry's value p is pnb = tot with pb = -inf; the empty prefix is pb = tot = 0 as in CTC.
// The one-wavefront lazy scan of the LM-free CTC search does not apply: A[c][e] depends on (entry, token), so lp_k + p is not
// monotone in k, the reason the LM scan materialises every pair.  Rows: ctc_beam_rows<., true> (every class a token, K up to N).
// Finishes: ctc_beam_lm_finish and ctc_beam_lex_finish as they are (with a null LM the EOS term is off and the LM sums are 0).
//   The transition matrix.  A pair's term A[c][e] is a gather.  When N * N * 4 bytes <= kAsgTransLds (32 KiB: N <= 90, the letter
//   models' 30 x 30 is 3.6 KB) the workgroup copies the matrix into dynamic LDS once, before the first frame; else every pair does
//   one dependent 4-byte load from global memory (N = 9998: 400 MB, L2 and HBM), in flight together with the LM and lexicon
//   lookups of the frame.  The budget: the lexicon scan's own LDS is 10 KB, the LM scan's 5.5 KB; 32 KiB more keeps a 256-thread
//   workgroup at 42 KB, so three of them still fit the 160 KiB of a CU beside one another, and a 1024-thread one (16 of a CU's 32
//   wavefronts) at two per CU: the matrix never lowers the occupancy the scans have without it.  Both paths do the same fp32
//   operations on the same values.  libw2l_hip_probe.so: W2L_ASG_BEAM_TRANS=global forces the gather (the A/B of tools/).
#pragma once
#include <cstring>

namespace w2l {

constexpr size_t kAsgTransLds = 32 * 1024;

struct BeamAsg {
  static constexpr bool kNoBlank = true;
  // the matrix the scan reads: LDS after a copy by the whole workgroup (the scan's first barrier publishes it), or global memory
  __device__ static __forceinline__ const float* stage(const BeamTrans& tr, int N) {
    extern __shared__ float sAsgTrans[];
    if (!tr.lds) return tr.a;
    for (int i = threadIdx.x; i < N * N; i += blockDim.x) sAsgTrans[i] = tr.a[i];
    return sAsgTrans;
  }
  __device__ static __forceinline__ bool none(int c, int e) { return c == e; }   // a repeated letter is a replabel's work
  // (p + A[c][e]) + lp[c]: two fp32 adds in w2l_viterbi_compute's order; from the empty prefix lp[c] alone
  __device__ static __forceinline__ float ext(float lpc, int c, int e, float, float tot, const float* A, int N) {
    if (c == e) return -INFINITY;
    return e < 0 ? lpc : (tot + A[(size_t)c * N + e]) + lpc;
  }
  __device__ static __forceinline__ void stay(float lpe, int e, float, float pnb, float, const float* A, int N, float* spb,
                                              float* spnb) {
    *spb = -INFINITY;
    *spnb = e >= 0 ? (pnb + A[(size_t)e * N + e]) + lpe : -INFINITY;
  }
};

static BeamTrans asg_beam_trans(const float* trans, int N, size_t* ldsBytes) {
  const size_t bytes = (size_t)N * N * sizeof(float);
  bool lds = bytes <= kAsgTransLds;
  if (const char* v = tune_env("W2L_ASG_BEAM_TRANS")) lds = lds && strcmp(v, "global") != 0;
  *ldsBytes = lds ? bytes : 0;
  return BeamTrans{trans, lds ? 1 : 0};
}

// The dispatch of a scan over its (logAdd, lattice policy, lexicon) template parameters: launch(logAdd, policy, lex) gets the two
// flags as std::integral_constant types and a BeamCtc or BeamAsg value, and returns the status of the launch it starts.
template <class Launch>
static int beam_scan_dispatch(int logAdd, bool asg, bool lex, Launch&& launch) {
  auto pol = [&](auto la, auto lx) { return asg ? launch(la, BeamAsg{}, lx) : launch(la, BeamCtc{}, lx); };
  auto la = [&](auto lx) { return logAdd ? pol(std::true_type{}, lx) : pol(std::false_type{}, lx); };
  return lex ? la(std::true_type{}) : la(std::false_type{});
}

}  // namespace w2l
