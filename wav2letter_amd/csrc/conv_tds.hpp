// conv_tds.hpp -- what the translation units of the fp32 TDS time convolution share: the descriptor of one launch and
// the entry points.  conv.hip calls the tds_conv_* functions of conv_tds.hip; conv_tds.hip offers every launch to the
// specialised kernels of conv_tds_special.hip (the order is written down at the top of that file) before its own
// general kernels.
#pragma once

#include "gemm.hpp"

namespace w2l {

struct TdsConvP {
  const float* x;     // tensor being read as the GEMM A operand [B][Tin][H][Cin]
  const float* w;     // [kw][CinW][CoutW] weights of the layer (forward orientation)
  const float* bias;  // [Cout] or null
  const float* add;   // optional addend with the layout of y (residual / upstream gradient), or null
  float* y;           // [B][Tout][H][Cout]
  int B, Tin, Tout, H, Cin, Cout, kw, stride, padl;
  int K, Kp, FS, NF;
  int relu, accum, flip;
  int CinW, CoutW;
  // phase decomposition of a strided backward-data (tds_conv_backward_data): weight tap of flipped tap j is
  // tapOff + tapStep*(kw-1-j); output frame u of the launch is frame oOff + oStep*u of a tensor with ToutFull frames
  int tapOff, tapStep, oOff, oStep, ToutFull;
  int abl;  // timing-only ablations of the probe tool (W2L_TDS_ABL): 1 = no K loop, 2 = no slab staging, 4 = no output
};

// conv_tds.hip: slab-in-LDS kernels for few-channel convolutions (TDS, C2 sub-sampling)
bool tds_conv_applicable(const w2l_conv_desc* d);
int tds_conv_forward(const w2l_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int relu,
                     hipStream_t s);
int tds_conv_backward_data(const w2l_conv_desc* d, const float* dy, const float* w, float* dx, int accumulate,
                           const float* add, hipStream_t s);
int tds_conv_backward_filter(const w2l_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                             hipStream_t s);

// conv_tds_special.hip: true + *status when a specialised kernel ran the launch `p` describes, false when it is not
// theirs (nothing was launched: the caller goes on to the next kernel).  The filter-gradient ones read p.x as the layer
// input and the geometry of the layer (p.Tin frames in, p.Tout frames of dy).
bool tds_c1_fwd_try(const TdsConvP& p, int profKind, hipStream_t s, int* status);
bool tds_tz_try(const TdsConvP& p, int profKind, hipStream_t s, int* status);
bool tds_rsf_try(const TdsConvP& p, const float* dy, float* dw, float* dbias, hipStream_t s, int* status);
bool tds_c1_filter_try(const TdsConvP& p, const float* dy, float* dw, float* dbias, hipStream_t s, int* status);
bool tds_tzf_strided_try(const TdsConvP& p, const float* dy, float* dw, float* dbias, hipStream_t s, int* status);

}  // namespace w2l
