// feat_stream.cpp -- the streaming log-mel front end's session: audio chunks of many concurrent streams -> MFSC frames.
//
// Protocol restated from the reference's LogMelFeature (recipes/streaming_convnets/inference/inference/module/feature/
// LogMelFeature.cpp): a slot buffers its samples, a run over `have` buffered samples produces numFrames(have) frames, consumes
// numFrames x stride of them and keeps the rest (fewer than one frame), finish drops what is left.  As in stream.cpp everything
// ragged is a table of counts computed on the HOST from the counts fed so far (a step never asks the device), sent with one async
// copy from a pinned ring; the frames themselves are ONE launch (feat_stream.hip).  The carry is double-buffered per slot: the
// workgroup that writes a slot's next carry runs beside those that still read the old one, and a slot without work keeps its
// buffer, so which of the two is current is part of the slot's host state and travels in its table entry.
#include <cstring>

#include "w2l_host.hpp"

namespace w2l {
void setHostError(const std::string& m);

namespace {

struct Unsupported : std::runtime_error {
  using std::runtime_error::runtime_error;
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

constexpr int kRing = 4;   // count tables in flight (pinned): a step reuses one only after the copy out of it has run

struct FeatSession {
  w2l_feat_desc d{};
  int S = 0, maxSamples = 0, maxOut = 0, carryLd = 0;
  size_t tabBytes = 0, carryOff[2] = {0, 0}, outOff = 0, stateBytes = 0;
  // host state per slot: an utterance is open, its carried samples, its current carry buffer
  std::vector<char> active, parity;
  std::vector<int> carry;
  // bound
  const float *G = nullptr, *H = nullptr;
  char* state = nullptr;
  int* pinned[kRing] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev[kRing] = {nullptr, nullptr, nullptr, nullptr};
  bool evUsed[kRing] = {false, false, false, false};
  int ring = 0;
  ~FeatSession() {
    for (int r = 0; r < kRing; ++r) {
      if (ev[r]) (void)hipEventDestroy(ev[r]);
      if (pinned[r]) (void)hipHostFree(pinned[r]);
    }
  }
  int* devTab() const { return (int*)state; }
  float* carryBuf(int b) const { return (float*)(state + carryOff[b]); }
  float* out() const { return (float*)(state + outOff); }
};

FeatSession* buildSession(const w2l_feat_desc* desc, int slots, int maxSamples) {
  if (!desc) throw std::invalid_argument("feature session: null descriptor");
  const w2l_feat_desc& d = *desc;
  if (d.frameSize < 1 || d.frameStride < 1 || d.nbins < 1 || d.ldSpec < 1 || d.numFilters < 1)
    throw std::invalid_argument("feature session: frameSize, frameStride, nbins, ldSpec and numFilters must be positive");
  if (d.frameStride > d.frameSize) throw std::invalid_argument("feature session: frameStride above frameSize (samples between frames would be skipped)");
  if (d.nbins > d.ldSpec) throw std::invalid_argument("feature session: nbins above ldSpec, the rows of the mel table");
  if (!(d.melFloor > 0.f)) throw std::invalid_argument("feature session: melFloor must be positive");
  if (slots < 1 || slots > 65535 || maxSamples < 1) throw std::invalid_argument("feature session: slots (1..65535) and maxSamples must be positive");
  if (d.frameSize > 512) throw Unsupported("feature session: frameSize " + std::to_string(d.frameSize) + " is above 512");
  if (d.nbins > 257) throw Unsupported("feature session: nbins " + std::to_string(d.nbins) + " is above 257");
  if (d.numFilters > 128) throw Unsupported("feature session: numFilters " + std::to_string(d.numFilters) + " is above 128");
  if (maxSamples > (1 << 24)) throw Unsupported("feature session: maxSamples " + std::to_string(maxSamples) + " is above 2^24");
  std::unique_ptr<FeatSession> s(new FeatSession());
  s->d = d; s->S = slots; s->maxSamples = maxSamples;
  s->maxOut = (d.frameSize - 1 + maxSamples - d.frameSize) / d.frameStride + 1;
  s->carryLd = (d.frameSize + 63) / 64 * 64;   // capacity N - 1
  s->tabBytes = align_up((size_t)slots * 4 * sizeof(int), 256);
  const size_t carryBytes = align_up((size_t)slots * s->carryLd * sizeof(float), 256);
  s->carryOff[0] = s->tabBytes;
  s->carryOff[1] = s->carryOff[0] + carryBytes;
  s->outOff = s->carryOff[1] + carryBytes;
  s->stateBytes = s->outOff + align_up((size_t)slots * d.numFilters * s->maxOut * sizeof(float), 256);
  s->active.assign(slots, 0);
  s->parity.assign(slots, 0);
  s->carry.assign(slots, 0);
  return s.release();
}

// One step's integer bookkeeping.  Validates first; fills table [S][4] (may be null) and nOut [S] (may be null); returns the state
// after the step in the three vectors without committing it.
bool advance(const FeatSession& s, const int* n, const int* start, const int* finish, int* table, int* nOut, std::vector<char>& newActive,
             std::vector<char>& newParity, std::vector<int>& newCarry) {
  if (!n) throw std::invalid_argument("feature step: null sample counts");
  for (int i = 0; i < s.S; ++i) {
    const bool st = start && start[i], fi = finish && finish[i];
    if (n[i] < 0 || n[i] > s.maxSamples)
      throw std::invalid_argument("feature step: slot " + std::to_string(i) + " was given " + std::to_string(n[i]) + " samples, outside 0.." +
                                  std::to_string(s.maxSamples));
    if (!st && !s.active[i] && (fi || n[i] > 0))
      throw std::invalid_argument("feature step: slot " + std::to_string(i) + (fi ? " finishes" : " is fed") + " before it was started");
  }
  newActive = s.active;
  newParity = s.parity;
  newCarry = s.carry;
  const int N = s.d.frameSize, St = s.d.frameStride;
  bool any = false;
  for (int i = 0; i < s.S; ++i) {
    const bool st = start && start[i], fi = finish && finish[i];
    if (st) { newActive[i] = 1; newCarry[i] = 0; }
    int e[4] = {0, 0, 0, 0};
    int out = 0;
    if (newActive[i] && (st || n[i] > 0)) {   // the slot has work: its carry moves to the other buffer
      const int nc = newCarry[i], have = nc + n[i];
      out = have < N ? 0 : 1 + (have - N) / St;
      const int rest = have - out * St;
      if (nc >= N || rest >= N || rest < 0 || out > s.maxOut) throw std::logic_error("feature step: count outside the planned buffers");
      e[0] = nc; e[1] = n[i]; e[2] = out; e[3] = 2 | (newParity[i] ? 1 : 0);
      newCarry[i] = rest;
      newParity[i] ^= 1;
      any = true;
    }
    if (table) std::memcpy(table + (size_t)i * 4, e, sizeof(e));
    if (nOut) nOut[i] = out;
    if (fi) { newActive[i] = 0; newCarry[i] = 0; }
  }
  return any;
}

void bindSession(FeatSession& s, const float* G, const float* H, void* state, size_t bytes) {
  if (!G || !H) throw std::invalid_argument("feature bind: null table");
  if (!state || ((uintptr_t)state & 255)) throw std::invalid_argument("feature bind: the state buffer must be a 256-byte aligned device pointer");
  if (bytes < s.stateBytes) throw std::invalid_argument("feature bind: the state buffer is smaller than w2l_feat_session_state_bytes");
  for (int r = 0; r < kRing; ++r) {
    if (!s.pinned[r]) hipCheck(hipHostMalloc((void**)&s.pinned[r], s.tabBytes, hipHostMallocDefault), "feature count table (pinned)");
    if (!s.ev[r]) hipCheck(hipEventCreateWithFlags(&s.ev[r], hipEventDisableTiming), "feature count table event");
  }
  s.G = G; s.H = H;
  s.state = (char*)state;
  // columns a step does not write read as zero from the first step on, whatever the buffer held
  hipCheck(hipMemset(s.out(), 0, s.stateBytes - s.outOff), "feature output area");
  hipCheck(hipStreamSynchronize(nullptr), "feature output area");
}

void stepSession(FeatSession& s, const void* pcm, int pcmType, const int* n, const int* start, const int* finish, const float** out, int* nOut,
                 hipStream_t stream) {
  if (!pcm || !n || !nOut || !out) throw std::invalid_argument("feature step: null argument");
  if (pcmType != W2L_PCM_F32 && pcmType != W2L_PCM_S16) throw std::invalid_argument("feature step: pcmType must be W2L_PCM_F32 or W2L_PCM_S16");
  if (!s.state) throw std::invalid_argument("feature step: no state bound (w2l_feat_session_bind first)");
  const int r = s.ring;
  if (s.evUsed[r]) hipCheck(hipEventSynchronize(s.ev[r]), "feature count table reuse");   // the copy of kRing steps ago: long done
  std::vector<char> na, np;
  std::vector<int> nc;
  const bool any = advance(s, n, start, finish, s.pinned[r], nOut, na, np, nc);   // throws before anything is enqueued
  if (any) {
    hipCheck(hipMemcpyAsync(s.devTab(), s.pinned[r], (size_t)s.S * 4 * sizeof(int), hipMemcpyHostToDevice, stream), "feature count table");
    hipCheck(hipEventRecord(s.ev[r], stream), "feature count table event");
    s.evUsed[r] = true;
    s.ring = (r + 1) % kRing;
    w2lCheck(w2l_feat_stream_frames(&s.d, s.G, s.H, pcm, pcmType, s.maxSamples, s.devTab(), s.carryBuf(0), s.carryBuf(1), s.carryLd, s.out(),
                                    s.maxOut, s.S, stream), "feature frames");
  }
  *out = s.out();
  s.active.swap(na);
  s.parity.swap(np);
  s.carry.swap(nc);
}

}  // namespace
}  // namespace w2l

using namespace w2l;

#define W2L_API extern "C" __attribute__((visibility("default")))
#define FEAT_TRY(...)                                                                  \
  try { __VA_ARGS__; return W2L_OK; }                                                  \
  catch (const Unsupported& e) { setHostError(e.what()); return W2L_EUNSUPPORTED; }   \
  catch (const std::invalid_argument& e) { setHostError(e.what()); return W2L_EINVAL; } \
  catch (const std::exception& e) { setHostError(e.what()); return W2L_EHIP; }

W2L_API int w2l_feat_session_query(const w2l_feat_desc* desc, int slots, int maxSamples, int* maxOut, size_t* stateBytes) {
  FEAT_TRY({
    std::unique_ptr<FeatSession> s(buildSession(desc, slots, maxSamples));
    if (maxOut) *maxOut = s->maxOut;
    if (stateBytes) *stateBytes = s->stateBytes;
  });
}

W2L_API int w2l_feat_session_create(const w2l_feat_desc* desc, int slots, int maxSamples, void** session) {
  FEAT_TRY({
    if (!session) throw std::invalid_argument("feature session: null argument");
    *session = nullptr;
    *session = buildSession(desc, slots, maxSamples);
  });
}

W2L_API void w2l_feat_session_destroy(void* session) { delete (FeatSession*)session; }
W2L_API int w2l_feat_session_max_out(void* session) { return session ? ((FeatSession*)session)->maxOut : 0; }
W2L_API size_t w2l_feat_session_state_bytes(void* session) { return session ? ((FeatSession*)session)->stateBytes : 0; }

W2L_API int w2l_feat_session_bind(void* session, const float* G, const float* H, void* state, size_t stateBytes) {
  FEAT_TRY({
    if (!session) throw std::invalid_argument("feature bind: null session");
    bindSession(*(FeatSession*)session, G, H, state, stateBytes);
  });
}

W2L_API int w2l_feat_session_counts(void* session, const int* n, const int* start, const int* finish, int* nOut) {
  FEAT_TRY({
    if (!session) throw std::invalid_argument("feature counts: null session");
    FeatSession& s = *(FeatSession*)session;
    std::vector<char> na, np;
    std::vector<int> nc;
    advance(s, n, start, finish, nullptr, nOut, na, np, nc);
    s.active.swap(na);
    s.parity.swap(np);
    s.carry.swap(nc);
  });
}

W2L_API int w2l_feat_session_step(void* session, const void* pcm, int pcmType, const int* n, const int* start, const int* finish,
                                  const float** out, int* nOut, void* stream) {
  FEAT_TRY({
    if (!session) throw std::invalid_argument("feature step: null session");
    stepSession(*(FeatSession*)session, pcm, pcmType, n, start, finish, out, nOut, (hipStream_t)stream);
  });
}

W2L_API int w2l_feat_session_slot_state(void* session, int slot, int* active, int* carrySamples) {
  FEAT_TRY({
    if (!session) throw std::invalid_argument("feature slot state: null session");
    FeatSession& s = *(FeatSession*)session;
    if (slot < 0 || slot >= s.S) throw std::invalid_argument("feature slot state: no such slot");
    if (active) *active = s.active[slot];
    if (carrySamples) *carrySamples = s.carry[slot];
  });
}

W2L_API int w2l_feat_session_reset(void* session, int slot) {
  FEAT_TRY({
    if (!session) throw std::invalid_argument("feature reset: null session");
    FeatSession& s = *(FeatSession*)session;
    if (slot < 0 || slot >= s.S) throw std::invalid_argument("feature reset: no such slot");
    s.active[slot] = 0;
    s.carry[slot] = 0;
  });
}
