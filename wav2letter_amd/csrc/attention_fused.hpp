// attention_fused.hpp -- the kernel arguments the two fused-attention families share (attention_fused.hip and
// attention_fused_bwd.hip: T <= 192, everything of a (utterance, head) resident; attention_fused_long.hip: 192 < T <= 512,
// keys streamed through LDS) and the long family's entry points for the two dispatchers
#pragma once
#include "common.hpp"

namespace w2l {

struct AfP {
  const float *q, *k, *v;   // [B][T][ld], head h at columns h d .. (h + 1) d
  const float* E;           // position table rows [2 csz - 1][d] (internal layout), or null
  const int* keyLen;
  float *P, *Pd, *ctx;      // P, Pd [B][H][T][T]; ctx [B][T][ldc] (may be null when its images are asked for)
  w2l_bf16_image_sink ctxI; // bf16 images of ctx written in place of a conversion pass (null pointers: none)
  int B, H, T, ld, ldc;
  int W, n0, rlo;           // table rows rlo .. rlo + W are the ones an utterance of T frames reaches
  float scale;
  uint32_t thr, seed, stream;
  float keepScale;
};

struct AbP {
  const float *q, *k, *v;   // [B][T][ld], head h at columns h d .. (h + 1) d
  const float* E;           // position table rows [2 csz - 1][d] (internal layout), or null
  const float* P;           // [B][H][T][T] of the forward pass
  const float* dctx;        // [B][T][ldc]
  float *dq, *dk, *dv;      // [B][T][ld] (each may be null when its images are asked for)
  w2l_bf16_image_sink dqI, dkI, dvI;   // bf16 images of dq / dk / dv written in place of a conversion pass (null pointers: none)
  float* dE;                // [2 n0 + 1][d] or null
  uint16_t *dSt, *Pdt;      // bf16 [B H][TP][TP]: row = key, column = query
  uint16_t* dRt;            // bf16 [B H][GW][TP]: row = window row (global numbering), column = query
  uint16_t* Et;             // bf16 [d][GW]
  float* dEp;               // [B H][GW][d]
  int B, H, T, ld, ldc;
  int W, n0, rlo;
  float scale;
  uint32_t thr, seed, stream;
  float keepScale;
};

// the long family (attention_fused_long.hip): 192 < T <= 512, d in {32, 192, 256}
bool attn_long_supported(int T, int d);
int attn_long_forward(const AfP& p, int d, hipStream_t s);
size_t attn_long_backward_workspace(int B, int H, int T, int d, bool table);   // 0: no kernel
int attn_long_backward(AbP p, int d, void* ws, size_t wsBytes, hipStream_t s);

}  // namespace w2l
