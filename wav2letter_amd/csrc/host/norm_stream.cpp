// norm_stream.cpp -- LocalNorm as a session: windowed feature normalisation of many concurrent streams, chunk by chunk.
//
// Protocol restated from the reference's streaming LocalNorm (recipes/streaming_convnets/inference/inference/module/nn/
// LocalNorm.cpp): start() opens the per-frame sum buffers, run() normalises each new frame over itself and up to L frames before
// it.  Here a slot keeps the (sum, sum of squares) pairs of its frames in a ring of L + maxChunk pairs in the caller's state
// buffer.  As in feat_stream.cpp everything ragged is a table computed on the HOST from the counts fed so far, sent with one async
// copy from a pinned ring; the frames themselves are ONE launch (local_norm.hip), whose arithmetic is the batch call's.
#include <cstring>

#include "w2l_host.hpp"

namespace w2l {
void setHostError(const std::string& m);
int norm_stream_launch(const float* x, size_t ld, float* y, size_t ldy, int F, int L, int cap, const int* tab, void* ring, int slots,
                       hipStream_t stream);

namespace {

struct Unsupported : std::runtime_error {
  using std::runtime_error::runtime_error;
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

constexpr int kRing = 4;   // tables in flight (pinned): a step reuses one only after the copy out of it has run

struct NormSession {
  int F = 0, S = 0, maxChunk = 0, L = 0, cap = 0;
  size_t tabBytes = 0, stateBytes = 0;
  // host state per slot: an utterance is open, its frames so far
  std::vector<char> active;
  std::vector<long long> count;
  // bound
  char* state = nullptr;
  int* pinned[kRing] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev[kRing] = {nullptr, nullptr, nullptr, nullptr};
  bool evUsed[kRing] = {false, false, false, false};
  int ring = 0;
  ~NormSession() {
    for (int r = 0; r < kRing; ++r) {
      if (ev[r]) (void)hipEventDestroy(ev[r]);
      if (pinned[r]) (void)hipHostFree(pinned[r]);
    }
  }
  int* devTab() const { return (int*)state; }
  void* pairs() const { return state + tabBytes; }
};

NormSession* buildSession(int nfeat, int slots, int maxChunk, int left, int right) {
  if (right != 0)
    throw std::invalid_argument("norm session: right context " + std::to_string(right) + " is not streamable; the reference's streaming "
                                "LocalNorm refuses rightContextSize != 0 as well (LocalNorm.cpp:33)");
  if (nfeat < 1 || slots < 1 || slots > 65535 || maxChunk < 1) throw std::invalid_argument("norm session: nfeat, slots (1..65535) and maxChunk must be positive");
  if (left < 0) throw std::invalid_argument("norm session: the left context must not be negative");
  if (left + 1 > 65536) throw Unsupported("norm session: a window of left + 1 = " + std::to_string((long long)left + 1) + " frames is above 65536");
  if (nfeat > 4096) throw Unsupported("norm session: nfeat " + std::to_string(nfeat) + " is above 4096");
  if (maxChunk > 65536) throw Unsupported("norm session: maxChunk " + std::to_string(maxChunk) + " is above 65536");
  std::unique_ptr<NormSession> s(new NormSession());
  s->F = nfeat; s->S = slots; s->maxChunk = maxChunk; s->L = left;
  s->cap = left + maxChunk;
  s->tabBytes = align_up((size_t)slots * 4 * sizeof(int), 256);
  s->stateBytes = s->tabBytes + align_up((size_t)slots * s->cap * 2 * sizeof(double), 256);
  s->active.assign(slots, 0);
  s->count.assign(slots, 0);
  return s.release();
}

void stepSession(NormSession& s, const float* x, size_t ld, const int* n, const int* start, float* y, size_t ldy, hipStream_t stream) {
  if (!x || !y || !n) throw std::invalid_argument("norm step: null argument (x, y or the frame counts)");
  if (ld < 1 || ldy < 1) throw std::invalid_argument("norm step: ld and ldy must be positive");
  bool any = false;
  for (int i = 0; i < s.S; ++i) {
    if (n[i] < 0 || n[i] > s.maxChunk)
      throw std::invalid_argument("norm step: slot " + std::to_string(i) + " was given " + std::to_string(n[i]) + " frames, outside 0.." +
                                  std::to_string(s.maxChunk));
    if ((size_t)n[i] > ld || (size_t)n[i] > ldy)
      throw std::invalid_argument("norm step: slot " + std::to_string(i) + " was given " + std::to_string(n[i]) + " frames, more than a row of x or y holds");
    if (n[i] > 0 && !s.active[i] && !(start && start[i]))
      throw std::invalid_argument("norm step: slot " + std::to_string(i) + " is fed before it was started");
    any = any || n[i] > 0;
  }
  if (!(y == x && ldy == ld)) {
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)s.S * s.F * ld * sizeof(float);
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (size_t)s.S * s.F * ldy * sizeof(float);
    if (x0 < y1 && y0 < x1) throw std::invalid_argument("norm step: x and y overlap partially (in place needs y == x and ldy == ld)");
  }
  if (!s.state) throw std::invalid_argument("norm step: no state bound (w2l_norm_session_bind first)");
  // nothing above changed the session; from here on only HIP itself can fail
  const int r = s.ring;
  if (any) {
    if (s.evUsed[r]) hipCheck(hipEventSynchronize(s.ev[r]), "norm table reuse");   // the copy of kRing steps ago: long done
    for (int i = 0; i < s.S; ++i) {
      const long long c = (start && start[i]) ? 0 : s.count[i];
      int e[4] = {(int)(c % s.cap), n[i], (int)std::min<long long>(c, s.L), 0};
      std::memcpy(s.pinned[r] + (size_t)i * 4, e, sizeof(e));
    }
    hipCheck(hipMemcpyAsync(s.devTab(), s.pinned[r], (size_t)s.S * 4 * sizeof(int), hipMemcpyHostToDevice, stream), "norm table");
    hipCheck(hipEventRecord(s.ev[r], stream), "norm table event");
    s.evUsed[r] = true;
    s.ring = (r + 1) % kRing;
    w2lCheck(norm_stream_launch(x, ld, y, ldy, s.F, s.L, s.cap, s.devTab(), s.pairs(), s.S, stream), "norm frames");
  }
  for (int i = 0; i < s.S; ++i) {
    if (start && start[i]) { s.active[i] = 1; s.count[i] = 0; }
    s.count[i] += n[i];
  }
}

}  // namespace
}  // namespace w2l

using namespace w2l;

#define W2L_API extern "C" __attribute__((visibility("default")))
#define NORM_TRY(...)                                                                  \
  try { __VA_ARGS__; return W2L_OK; }                                                  \
  catch (const Unsupported& e) { setHostError(e.what()); return W2L_EUNSUPPORTED; }   \
  catch (const std::invalid_argument& e) { setHostError(e.what()); return W2L_EINVAL; } \
  catch (const std::exception& e) { setHostError(e.what()); return W2L_EHIP; }

W2L_API int w2l_norm_session_query(int nfeat, int slots, int maxChunk, int left, int right, size_t* stateBytes) {
  NORM_TRY({
    std::unique_ptr<NormSession> s(buildSession(nfeat, slots, maxChunk, left, right));
    if (stateBytes) *stateBytes = s->stateBytes;
  });
}

W2L_API int w2l_norm_session_create(int nfeat, int slots, int maxChunk, int left, int right, void** session) {
  NORM_TRY({
    if (!session) throw std::invalid_argument("norm session: null argument");
    *session = nullptr;
    *session = buildSession(nfeat, slots, maxChunk, left, right);
  });
}

W2L_API void w2l_norm_session_destroy(void* session) { delete (NormSession*)session; }
W2L_API size_t w2l_norm_session_state_bytes(void* session) { return session ? ((NormSession*)session)->stateBytes : 0; }

W2L_API int w2l_norm_session_bind(void* session, void* state, size_t stateBytes) {
  NORM_TRY({
    if (!session) throw std::invalid_argument("norm bind: null session");
    NormSession& s = *(NormSession*)session;
    if (!state || ((uintptr_t)state & 255)) throw std::invalid_argument("norm bind: the state buffer must be a 256-byte aligned device pointer");
    if (stateBytes < s.stateBytes) throw std::invalid_argument("norm bind: the state buffer is smaller than w2l_norm_session_state_bytes");
    for (int r = 0; r < kRing; ++r) {
      if (!s.pinned[r]) hipCheck(hipHostMalloc((void**)&s.pinned[r], s.tabBytes, hipHostMallocDefault), "norm table (pinned)");
      if (!s.ev[r]) hipCheck(hipEventCreateWithFlags(&s.ev[r], hipEventDisableTiming), "norm table event");
    }
    s.state = (char*)state;
    // a window never reaches a pair that this utterance did not write, so the ring needs no initialisation; every slot is closed
    s.active.assign(s.S, 0);
    s.count.assign(s.S, 0);
  });
}

W2L_API int w2l_norm_session_step(void* session, const float* x, size_t ld, const int* h_n, const int* h_start, float* y, size_t ldy,
                                  void* stream) {
  NORM_TRY({
    if (!session) throw std::invalid_argument("norm step: null session");
    stepSession(*(NormSession*)session, x, ld, h_n, h_start, y, ldy, (hipStream_t)stream);
  });
}

W2L_API int w2l_norm_session_slot_state(void* session, int slot, int* active, long long* frames) {
  NORM_TRY({
    if (!session) throw std::invalid_argument("norm slot state: null session");
    NormSession& s = *(NormSession*)session;
    if (slot < 0 || slot >= s.S) throw std::invalid_argument("norm slot state: no such slot");
    if (active) *active = s.active[slot];
    if (frames) *frames = s.count[slot];
  });
}

W2L_API int w2l_norm_session_reset(void* session, int slot) {
  NORM_TRY({
    if (!session) throw std::invalid_argument("norm reset: null session");
    NormSession& s = *(NormSession*)session;
    if (slot < 0 || slot >= s.S) throw std::invalid_argument("norm reset: no such slot");
    s.active[slot] = 0;
    s.count[slot] = 0;
  });
}
