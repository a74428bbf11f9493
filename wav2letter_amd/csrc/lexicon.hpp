// lexicon.hpp -- the lexicon trie as one position-independent table (contract: include/w2l_hip.h, w2l_lexicon_*).
// Shared by the host builder / walker (host/lexicon.cpp) and the lexicon-constrained beam search (criterion_ctc_beam_lex.hpp): the
// blob holds offsets only, so the same bytes are the table on the host and, after one copy, on the device, and lex_child /
// lex_node below are THE lookups on both sides.
//   blob = LexHeader | node[numNodes] (48 bytes each) | slot[cap] (16 bytes each)
//   node 0 is the root; node v > 0 is reached from its parent by the token node[v].tok
//   node: smear (max of wordSmear over the words kept at or below it), meta = nw | hasChildren << 3, tok, words[6]
//   slot: key = (node << 32) | (token + 1), 0 = free; open addressing, linear probing from lex_hash(key) & (cap-1), cap a power of
//         two >= 2 * edges (load factor <= 1/2, so a free slot ends every chain)
//   The probe loop is bounded by cap, every node id is clamped into the table and lex_view holds the header's counts to the header's
//   own `bytes`: within the bytes the header claims a damaged blob gives wrong nodes, never a spin or a read outside its arrays.
#pragma once
#include <stdint.h>

#ifndef W2L_HD
#ifdef __HIPCC__
#define W2L_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define W2L_HD inline
#endif
#endif

namespace w2l {

constexpr uint32_t kLexMagic = 0x584c4e57u;   // "WNLX"
constexpr int kLexMaxWords = 6;               // words kept per node
constexpr uint32_t kLexMaxNodes = 1u << 28;   // (node << 3) | slot is a 31-bit label of the beam search's prefix table

struct LexHeader {
  uint32_t magic, numTokens, numWords, numNodes;
  uint32_t cap, edges, smeared, pad0;
  int32_t silToken;
  uint32_t pad1, pad2, pad3;
  uint64_t bytes;
  uint64_t pad4;
};
static_assert(sizeof(LexHeader) == 64, "the blob's header is 64 bytes");

struct alignas(16) LexNode {
  float smear;
  uint32_t meta;   // nw | hasChildren << 3
  int32_t tok;     // the token of the edge that reaches this node; -1 for the root
  int32_t pad;
  int32_t words[8];   // kLexMaxWords used, -1 beyond nw
};
static_assert(sizeof(LexNode) == 48, "three 16-byte loads per node");

struct alignas(16) LexSlot {
  uint64_t key;
  int32_t child;
  int32_t pad;
};
static_assert(sizeof(LexSlot) == 16, "one 16-byte load per probe");

W2L_HD uint32_t lex_hash(uint64_t z) {   // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)(z ^ (z >> 31));
}

struct LexView {
  const LexNode* node;
  const LexSlot* slot;
  uint32_t numNodes, capm;
  int32_t silToken;
};

// The header is not trusted: counts the blob's own size does not hold, or a capacity that is no power of two, give a table of the
// root alone with one free slot -- nothing can be spelled then -- instead of reads outside the blob or a probe loop of 2^32 rounds.
W2L_HD LexView lex_view(const void* blob) {
  const LexHeader* h = (const LexHeader*)blob;
  LexView v;
  uint32_t numNodes = h->numNodes, cap = h->cap;
  const uint64_t slotOff = sizeof(LexHeader) + (uint64_t)numNodes * sizeof(LexNode);
  const bool sane = h->magic == kLexMagic && numNodes >= 1 && numNodes < kLexMaxNodes && cap >= 1 && (cap & (cap - 1)) == 0 &&
                    slotOff + (uint64_t)cap * sizeof(LexSlot) <= h->bytes;
  if (!sane) { numNodes = 1; cap = 1; }
  v.numNodes = numNodes;
  v.node = (const LexNode*)((const char*)blob + sizeof(LexHeader));
  v.slot = (const LexSlot*)((const char*)blob + sizeof(LexHeader) + (uint64_t)numNodes * sizeof(LexNode));
  v.capm = cap - 1;
  v.silToken = h->silToken;
  return v;
}

// child of `node` by `token`, -1 when the edge is absent
W2L_HD int lex_child(const LexView& v, int node, int token) {
  const uint32_t u = (uint32_t)node < v.numNodes ? (uint32_t)node : 0u;
  const uint64_t key = ((uint64_t)u << 32) | (uint64_t)(uint32_t)(token + 1);
  uint32_t h = lex_hash(key) & v.capm;
  for (uint32_t probe = 0; probe <= v.capm; ++probe) {
    const LexSlot e = v.slot[h];
    if (e.key == key) return (uint32_t)e.child < v.numNodes && e.child > 0 ? e.child : -1;
    if (e.key == 0) break;
    h = (h + 1) & v.capm;
  }
  return -1;
}

W2L_HD const LexNode& lex_node(const LexView& v, int node) { return v.node[(uint32_t)node < v.numNodes ? (uint32_t)node : 0u]; }
W2L_HD int lex_nw(const LexNode& n) { const int nw = (int)(n.meta & 7u); return nw <= kLexMaxWords ? nw : kLexMaxWords; }
W2L_HD bool lex_has_children(const LexNode& n) { return (n.meta >> 3) & 1u; }

}  // namespace w2l
