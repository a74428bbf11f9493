// ngram_lm.hpp -- the back-off n-gram LM as one position-independent table (contract: include/w2l_hip.h, w2l_ngram_lm_*).
// Shared by the host builder / scorer (host/ngram_lm.cpp) and the fused beam search (criterion_ctc_beam_lm.hpp): the blob holds
// offsets only, so the same bytes are the table on the host and, after one copy, on the device, and ngram_q below is THE score
// rule on both sides.
//   blob = NgramHeader | bo[numStates] fp32 | suf[numStates] int32 | slot[cap] (16 bytes each)
//   words: 0 .. numTokens-1 the token classes, numTokens = BOS, numTokens+1 = EOS
//   state 0 = the empty context; every n-gram of order < the model order is a state
//   slot: key = (state << 32) | (word + 1), 0 = free; open addressing, linear probing from ngram_hash(key) & (cap-1), cap a power
//         of two >= 2 * edges (load factor <= 1/2, so a free slot ends every chain)
//   q(s, w):  acc = 0
//             loop: if edge (s, w) exists: return (acc + p, next)
//                   if s == 0:             return (acc + unkLogp, 0)
//                   acc = acc + bo[s];  s = suf[s]
//   every add is one fp32 add in this order.  Both loops are bounded (probes by cap, the back-off walk by the model order), every
//   state is clamped into the table and ngram_view holds the header's counts to the header's own `bytes`: within the bytes the
//   header claims -- the caller's promise about the allocation -- a damaged blob gives wrong scores, never a spin or a read
//   outside the blob's arrays.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define W2L_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define W2L_HD inline
#endif

namespace w2l {

constexpr uint32_t kNgramMagic = 0x4d4c4e57u;   // "WNLM"
constexpr int kNgramMaxOrder = 8;

struct NgramHeader {
  uint32_t magic, order, numTokens, numStates;
  uint32_t cap, start, hasBos, hasEos;
  float unkLogp;
  uint32_t edges, pad0, pad1;
  uint64_t bytes;
  uint64_t pad2;
};
static_assert(sizeof(NgramHeader) == 64, "the blob's header is 64 bytes");

struct alignas(16) NgramSlot {
  uint64_t key;
  float p;
  int32_t next;
};
static_assert(sizeof(NgramSlot) == 16, "one 16-byte load per probe");

W2L_HD uint32_t ngram_hash(uint64_t z) {   // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)(z ^ (z >> 31));
}

W2L_HD const float* ngram_bo(const void* blob) { return (const float*)((const char*)blob + sizeof(NgramHeader)); }
W2L_HD const int32_t* ngram_suf(const void* blob, uint32_t numStates) { return (const int32_t*)(ngram_bo(blob) + numStates); }
W2L_HD const NgramSlot* ngram_slots(const void* blob, uint32_t numStates) {
  const uint64_t off = (sizeof(NgramHeader) + (uint64_t)numStates * 8 + 15) & ~(uint64_t)15;
  return (const NgramSlot*)((const char*)blob + off);
}

// the table's constants, read once by a caller that scores many words
struct NgramView {
  const float* bo;
  const int32_t* suf;
  const NgramSlot* slot;
  uint32_t numStates, capm, order;
  float unkLogp;
};

// The header is not trusted either: a state count or capacity that the blob's own size does not hold, or a capacity that is no
// power of two, gives a table of one state and one (free) slot -- every score is then <unk>'s -- instead of reads outside the blob
// or a probe loop of 2^32 rounds.
W2L_HD NgramView ngram_view(const void* blob) {
  const NgramHeader* h = (const NgramHeader*)blob;
  NgramView v;
  uint32_t numStates = h->numStates, cap = h->cap;
  const uint64_t slotOff = (sizeof(NgramHeader) + (uint64_t)numStates * 8 + 15) & ~(uint64_t)15;
  const bool sane = h->magic == kNgramMagic && numStates >= 1 && cap >= 1 && (cap & (cap - 1)) == 0 &&
                    slotOff + (uint64_t)cap * sizeof(NgramSlot) <= h->bytes;
  if (!sane) { numStates = 1; cap = 1; }
  v.numStates = numStates;
  v.bo = ngram_bo(blob);
  v.suf = ngram_suf(blob, numStates);
  v.slot = ngram_slots(blob, numStates);
  v.capm = cap - 1;
  v.order = h->order <= (uint32_t)kNgramMaxOrder ? h->order : (uint32_t)kNgramMaxOrder;
  v.unkLogp = h->unkLogp;
  return v;
}

W2L_HD float ngram_q(const NgramView& v, int state, int word, int* next) {
  float acc = 0.f;
  uint32_t s = (uint32_t)state < v.numStates ? (uint32_t)state : 0u;
  for (uint32_t hop = 0; hop <= v.order; ++hop) {
    const uint64_t key = ((uint64_t)s << 32) | (uint64_t)(uint32_t)(word + 1);
    uint32_t h = ngram_hash(key) & v.capm;
    for (uint32_t probe = 0; probe <= v.capm; ++probe) {
      const NgramSlot e = v.slot[h];
      if (e.key == key) {
        *next = (uint32_t)e.next < v.numStates ? e.next : 0;
        return acc + e.p;
      }
      if (e.key == 0) break;
      h = (h + 1) & v.capm;
    }
    if (s == 0) break;
    acc = acc + v.bo[s];
    const uint32_t n = (uint32_t)v.suf[s];
    s = n < v.numStates ? n : 0u;
  }
  *next = 0;
  return acc + v.unkLogp;
}

}  // namespace w2l
