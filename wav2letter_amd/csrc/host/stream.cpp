// stream.cpp -- stateful, chunked forward pass for many concurrent audio streams (the streaming TDS-CTC recipe).
//
// Protocol restated from the reference's InferenceModule start / run / finish
// (recipes/streaming_convnets/inference/inference/module/nn/Conv1dFbGemm.cpp:75-185, Residual.cpp, TDSBlock.cpp):
//   * every layer with a time extent keeps, per slot, the input frames it has not consumed yet (its carry);
//   * at `start` a layer with left padding begins with that many zero frames;
//   * a run over nIn frames produces (nIn - kw) / stride + 1 frames and consumes nOut * stride of them;
//   * at `finish` a layer with right padding appends that many zero frames behind what its producer flushed in the same step.
// Here one step runs every layer ONCE over S slots: the producer's frames of this step already hold what it flushed, so the
// cascade is one pass.  The layers run on rectangular windows [S][W][F] through their ordinary forward entry points (B = S,
// T = W, no padding); what is ragged -- each slot's carry, new frames, consumption -- is a table of counts computed on the HOST
// from the counts fed so far (a step never asks the device), sent with one async copy from pinned memory, and applied by one
// hand-over kernel per time-extent layer (stream.hip).  A TDS block's residual hold-back needs no state of its own: the carry of
// its convolution (kw - 1 frames) contains every input frame whose output does not exist yet.
//
// Precision is a property of the session (w2l_stream_*_ex).  A BF16 session runs the layers' mixed-precision forward (Ctx::bf16) with
// two differences a session can afford because its model does not change between steps: the bf16 weight images are written once, on
// the first step after a bind or a refresh, from a copy of the parameter arena that the session keeps in its own state (so nothing
// a step reads can change under it: the snapshot covers biases and LayerNorm scalars too), and the fl::Linear products run on
// w2l_gemm_bf16_smallm (Ctx::smallM), whose rows are bitwise independent of each other -- a slot's emissions do not depend on its
// neighbours -- and which adds in the order of w2l_gemm_bf16: on the recipe's shapes the session equals the trainer's forward bit for bit.  The reference's streaming library serves half-precision weights the same way (fbgemm packs them once).
#include <algorithm>
#include <cstring>

#include "w2l_host.hpp"

namespace w2l {
void setHostError(const std::string& m);
void trainerArch(void* h, std::string& archText, int& nFeat, int& nLabel);
const float* trainerParams(void* h, bool& mixedPrecision);
bool trainerMixedConvs(void* h);

namespace {

struct Unsupported : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct MatmulMode {   // scoped, as the trainer's forward sets it around the network's own calls
  int prev = 0;
  bool on;
  explicit MatmulMode(bool bf16) : on(bf16) { if (on) prev = w2l_set_matmul_precision(1); }
  ~MatmulMode() { if (on) w2l_set_matmul_precision(prev); }
};

struct TimeLayer {
  size_t layer = 0;
  StreamGeom g;
  int F = 0;         // floats per input frame
  int cap = 0;       // carry capacity in frames: max(kw - 1, padL)
  int W = 0;         // window frames: cap + the producer's most frames per step + padR
  int To = 0;        // (W - kw) / stride + 1: the most frames it produces per step
  int srcRows = 0;   // row stride of the producer's buffer, in frames
  size_t carryOff[2] = {0, 0}, winOff = 0, resOff = 0;
};

constexpr int kRing = 4;   // count tables in flight (pinned): a step reuses one only after the copy out of it has run

struct Session {
  std::shared_ptr<Sequential> net;
  void* trainer = nullptr;   // non-null: parameters and mode are the trainer's, read at every step
  int nFeat = 0, nLabel = 0, S = 0, Cmax = 0, maxOut = 0;
  std::vector<TimeLayer> tl;
  std::vector<int> tlOf;   // per layer: index into tl, or -1 (frame-local)
  size_t inOff = 0, arenaFloats = 0, tabBytes = 0, stateBytes = 0;
  // host state: per slot, whether an utterance is open and each time-extent layer's carry count
  std::vector<char> active;
  std::vector<int> carry;   // [S][tl.size()]
  // bound
  const float* params = nullptr;
  char* state = nullptr;
  int* pinned[kRing] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev[kRing] = {nullptr, nullptr, nullptr, nullptr};
  bool evUsed[kRing] = {false, false, false, false};
  int ring = 0, parity = 0;
  // W2L_STREAM_BF16: the state carries, behind the arena, a copy of the parameters
  bool bf16 = false;
  bool weightsStale = true;   // the next step copies the parameters and writes the weight images
  bool freshState = true;     // the next step zero-fills the arena first: the images' zero padding, whatever the buffer held
  size_t snapOff = 0;   // bytes into the state
  float* snapshot() const { return (float*)(state + snapOff); }
  ~Session() {
    for (int r = 0; r < kRing; ++r) {
      if (ev[r]) (void)hipEventDestroy(ev[r]);
      if (pinned[r]) (void)hipHostFree(pinned[r]);
    }
  }
  int* devTab() const { return (int*)state; }
  float* arena() const { return (float*)(state + tabBytes); }
};

Session* buildSession(const std::string& archText, int nFeat, int nLabel, int slots, int maxChunk, int precision = W2L_STREAM_FP32) {
  if (precision != W2L_STREAM_FP32 && precision != W2L_STREAM_BF16)
    throw std::invalid_argument("streaming session: precision must be W2L_STREAM_FP32 or W2L_STREAM_BF16");
  if (slots <= 0 || slots > 65535 || maxChunk <= 0 || nFeat <= 0 || nLabel <= 0)
    throw std::invalid_argument("streaming session: slots (1..65535), max_chunk, NFEAT and NLABEL must be positive");
  std::unique_ptr<Session> s(new Session());
  s->nFeat = nFeat; s->nLabel = nLabel; s->S = slots; s->Cmax = maxChunk;
  s->net = buildSequentialFromText(archText, nFeat, nLabel, false);   // planned below, layer by layer, on the windows
  Planner pl;
  Act a = actInput(slots, maxChunk, nFeat);
  s->inOff = pl.alloc(a.numel());
  int nmax = maxChunk;
  for (size_t i = 0; i < s->net->size(); ++i) {
    Layer& L = s->net->at(i);
    StreamGeom g;
    std::string why;
    if (!L.streamGeom(g, why)) throw Unsupported("streaming session: arch line '" + L.archLine + "' (" + L.name() + ") cannot be streamed: " + why);
    a.T = nmax;
    if (!g.timeExtent) {
      a = L.plan(a, pl);
      s->tlOf.push_back(-1);
      continue;
    }
    TimeLayer t;
    t.layer = i; t.g = g; t.F = a.F; t.srcRows = nmax;
    t.cap = std::max(g.kw - 1, g.padL);
    t.W = t.cap + nmax + g.padR;
    if ((size_t)t.W * t.F > ((size_t)1 << 30)) throw Unsupported("streaming session: window of '" + L.archLine + "' is too large");
    a.T = t.W;
    L.setStreamMode(true);
    a = L.plan(a, pl);
    t.To = a.T;
    if (t.To != (t.W - g.kw) / g.stride + 1) throw std::logic_error("streaming session: '" + L.archLine + "' planned another output length");
    if (t.cap > 0) { t.carryOff[0] = pl.alloc((size_t)slots * t.cap * t.F); t.carryOff[1] = pl.alloc((size_t)slots * t.cap * t.F); }
    t.winOff = pl.alloc((size_t)slots * t.W * t.F);
    if (g.resShift >= 0) t.resOff = pl.alloc((size_t)slots * t.To * t.F);
    nmax = t.To;
    s->tlOf.push_back((int)s->tl.size());
    s->tl.push_back(t);
  }
  requireEmissionLayout(a);
  if (a.F != nLabel) throw std::invalid_argument("streaming session: network output width != NLABEL");
  s->maxOut = nmax;
  s->arenaFloats = pl.used();
  s->tabBytes = (s->tl.size() * (size_t)slots * 4 * sizeof(int) + 255) / 256 * 256;
  s->stateBytes = s->tabBytes + s->arenaFloats * sizeof(float);
  if (precision == W2L_STREAM_BF16) {   // an FP32 session's state is what it always was
    s->bf16 = true;
    s->snapOff = (s->stateBytes + 255) / 256 * 256;
    s->stateBytes = s->snapOff + (s->net->paramFloats() * sizeof(float) + 255) / 256 * 256;
  }
  s->active.assign(slots, 0);
  s->carry.assign((size_t)slots * s->tl.size(), 0);
  return s.release();
}

// One step's integer bookkeeping.  Validates first; fills table [tl][S][4] (may be null) and nOut [S] (may be null); returns the
// state after the step in newActive / newCarry without committing it.
void advance(const Session& s, const int* n, const int* start, const int* finish, int* table, int* nOut, std::vector<char>& newActive,
             std::vector<int>& newCarry) {
  if (!n) throw std::invalid_argument("stream step: null frame counts");
  const size_t Lt = s.tl.size();
  for (int i = 0; i < s.S; ++i) {
    const bool st = start && start[i], fi = finish && finish[i];
    if (n[i] < 0 || n[i] > s.Cmax)
      throw std::invalid_argument("stream step: slot " + std::to_string(i) + " was given " + std::to_string(n[i]) + " frames, outside 0.." +
                                  std::to_string(s.Cmax));
    if (!st && !s.active[i] && (fi || n[i] > 0))
      throw std::invalid_argument("stream step: slot " + std::to_string(i) + (fi ? " finishes" : " is fed") + " before it was started");
  }
  newActive = s.active;
  newCarry = s.carry;
  for (int i = 0; i < s.S; ++i) {
    const bool st = start && start[i], fi = finish && finish[i];
    int* cy = newCarry.data() + (size_t)i * Lt;
    if (st) {
      newActive[i] = 1;
      for (size_t k = 0; k < Lt; ++k) cy[k] = s.tl[k].g.padL;
    }
    int nNew = n[i];
    for (size_t k = 0; k < Lt; ++k) {
      const TimeLayer& t = s.tl[k];
      int e[4] = {0, 0, 0, 0};
      if (newActive[i]) {
        const int nc = cy[k];
        const int nIn = nc + nNew + (fi ? t.g.padR : 0);
        const int out = nIn >= t.g.kw ? (nIn - t.g.kw) / t.g.stride + 1 : 0;
        const int consumed = std::min(out * t.g.stride, nIn);
        if (nc > t.cap || nNew > t.srcRows || nIn > t.W || nIn - consumed > t.cap || out > t.To)
          throw std::logic_error("stream step: count outside the planned window");
        e[0] = nc | (st ? 1 << 30 : 0); e[1] = nNew; e[2] = nIn; e[3] = consumed;
        cy[k] = nIn - consumed;
        nNew = out;
      } else {
        nNew = 0;
      }
      if (table) std::memcpy(table + (k * (size_t)s.S + i) * 4, e, sizeof(e));
    }
    if (!newActive[i]) nNew = 0;
    if (nOut) nOut[i] = nNew;
    if (fi) {
      newActive[i] = 0;
      for (size_t k = 0; k < Lt; ++k) cy[k] = 0;
    }
  }
}

void bindSession(Session& s, const float* params, void* state, size_t bytes) {
  if (!state || ((uintptr_t)state & 255)) throw std::invalid_argument("stream bind: the state buffer must be a 256-byte aligned device pointer");
  if (bytes < s.stateBytes) throw std::invalid_argument("stream bind: the state buffer is smaller than w2l_stream_state_bytes");
  if (!params && !s.trainer) throw std::invalid_argument("stream bind: null parameters");
  s.params = params;
  s.state = (char*)state;
  s.weightsStale = true;
  s.freshState = true;
  const size_t tb = std::max<size_t>(s.tabBytes, 256);
  for (int r = 0; r < kRing; ++r) {
    if (!s.pinned[r]) hipCheck(hipHostMalloc((void**)&s.pinned[r], tb, hipHostMallocDefault), "stream count table (pinned)");
    if (!s.ev[r]) hipCheck(hipEventCreateWithFlags(&s.ev[r], hipEventDisableTiming), "stream count table event");
  }
}

void stepSession(Session& s, const float* x, const int* n, const int* start, const int* finish, const float** out, int* nOut, hipStream_t stream) {
  if (!x || !n || !nOut) throw std::invalid_argument("stream step: null argument");
  if (!s.state) throw std::invalid_argument("stream step: no state bound (w2l_stream_bind first)");
  const float* params = s.params;
  if (s.trainer) {
    bool mixed = false;
    const float* tp = trainerParams(s.trainer, mixed);
    if (mixed && !s.bf16) throw Unsupported("stream step: the trainer is in mixed-precision mode; this session is fp32 (W2L_STREAM_BF16 at creation)");
    if (!mixed && s.bf16) throw std::invalid_argument("stream step: a W2L_STREAM_BF16 session needs the trainer's mixed-precision mode on");
    if (s.bf16 && trainerMixedConvs(s.trainer))
      throw Unsupported("stream step: the trainer's second mixed-precision level (set_mixed_precision_convs) is not planned for sessions");
    if (!params) params = tp;
    if (!params) throw std::invalid_argument("stream step: the trainer has no parameters bound");
  }
  const int r = s.ring;
  if (s.evUsed[r]) hipCheck(hipEventSynchronize(s.ev[r]), "stream count table reuse");   // the copy of kRing steps ago: long done
  std::vector<char> na;
  std::vector<int> nc;
  advance(s, n, start, finish, s.pinned[r], nOut, na, nc);   // throws before anything is enqueued
  bool any = false;
  for (int i = 0; i < s.S; ++i) any = any || n[i] > 0 || (start && start[i]) || (finish && finish[i]);
  float* ar = s.arena();
  if (out) *out = nullptr;
  if (any) {
    Ctx c;
    c.stream = stream;
    c.train = false;
    c.params = const_cast<float*>(params);
    MatmulMode mm(s.bf16);
    if (s.bf16) {
      if (s.freshState) hipCheck(hipMemsetAsync(ar, 0, s.arenaFloats * sizeof(float), stream), "stream state");
      if (s.weightsStale)
        hipCheck(hipMemcpyAsync(s.snapshot(), params, s.net->paramFloats() * sizeof(float), hipMemcpyDeviceToDevice, stream), "stream parameter snapshot");
      c.params = s.snapshot();
      c.bf16 = true;
      c.smallM = true;
      c.weightsReady = !s.weightsStale;
    }
    w2lCheck(w2l_transpose(x, ar + s.inOff, s.S, s.nFeat, s.Cmax, stream), "stream input transpose");
    if (!s.tl.empty()) {
      hipCheck(hipMemcpyAsync(s.devTab(), s.pinned[r], s.tl.size() * (size_t)s.S * 4 * sizeof(int), hipMemcpyHostToDevice, stream),
               "stream count table");
      hipCheck(hipEventRecord(s.ev[r], stream), "stream count table event");
      s.evUsed[r] = true;
      s.ring = (r + 1) % kRing;
    }
    const float* cur = ar + s.inOff;
    for (size_t i = 0; i < s.net->size(); ++i) {
      float* y = nullptr;
      const int k = s.tlOf[i];
      if (k >= 0) {
        const TimeLayer& t = s.tl[k];
        float* res = t.g.resShift >= 0 ? ar + t.resOff : nullptr;
        w2lCheck(w2l_stream_window(cur, t.srcRows, t.cap ? ar + t.carryOff[s.parity] : nullptr, t.cap ? ar + t.carryOff[s.parity ^ 1] : nullptr,
                                   t.cap, ar + t.winOff, t.W, res, std::max(t.g.resShift, 0), t.To, s.devTab() + (size_t)k * s.S * 4, s.S, t.F,
                                   stream), "stream window");
        c.streamRes = res;
        s.net->at(i).forward(c, ar, ar + t.winOff, y);
        c.streamRes = nullptr;
      } else {
        s.net->at(i).forward(c, ar, cur, y);
      }
      cur = y;
    }
    s.parity ^= 1;
    s.weightsStale = false;
    s.freshState = false;
    if (out) *out = cur;
  }
  s.active.swap(na);
  s.carry.swap(nc);
}

}  // namespace
}  // namespace w2l

using namespace w2l;

#define W2L_API extern "C" __attribute__((visibility("default")))
#define STREAM_TRY(...)                                                               \
  try { __VA_ARGS__; return W2L_OK; }                                                  \
  catch (const Unsupported& e) { setHostError(e.what()); return W2L_EUNSUPPORTED; }   \
  catch (const std::invalid_argument& e) { setHostError(e.what()); return W2L_EINVAL; } \
  catch (const std::exception& e) { setHostError(e.what()); return W2L_EHIP; }

W2L_API int w2l_stream_create(const char* archText, int nFeat, int nLabel, int slots, int maxChunk, void** session) {
  STREAM_TRY({
    if (!archText || !session) throw std::invalid_argument("stream create: null argument");
    *session = nullptr;
    *session = buildSession(archText, nFeat, nLabel, slots, maxChunk);
  });
}

W2L_API int w2l_stream_create_ex(const char* archText, int nFeat, int nLabel, int slots, int maxChunk, int precision, void** session) {
  STREAM_TRY({
    if (!archText || !session) throw std::invalid_argument("stream create: null argument");
    *session = nullptr;
    *session = buildSession(archText, nFeat, nLabel, slots, maxChunk, precision);
  });
}

W2L_API int w2l_stream_create_for_trainer_ex(void* trainer, int slots, int maxChunk, int precision, void** session) {
  STREAM_TRY({
    if (!trainer || !session) throw std::invalid_argument("stream create: null argument");
    *session = nullptr;
    if (precision != W2L_STREAM_FP32 && precision != W2L_STREAM_BF16)
      throw std::invalid_argument("streaming session: precision must be W2L_STREAM_FP32 or W2L_STREAM_BF16");
    bool mixed = false;
    (void)trainerParams(trainer, mixed);
    if (precision == W2L_STREAM_FP32) {
      if (mixed) throw Unsupported("streaming session: the trainer is in mixed-precision mode; the streaming step is fp32 only");
    } else {
      if (!mixed) throw std::invalid_argument("streaming session: W2L_STREAM_BF16 needs the trainer's mixed-precision mode on (the session equals the trainer's own forward)");
      if (trainerMixedConvs(trainer))
        throw Unsupported("streaming session: the trainer's second mixed-precision level (set_mixed_precision_convs) is not planned for sessions");
    }
    std::string arch;
    int nFeat = 0, nLabel = 0;
    trainerArch(trainer, arch, nFeat, nLabel);
    Session* s = buildSession(arch, nFeat, nLabel, slots, maxChunk, precision);
    s->trainer = trainer;
    *session = s;
  });
}

W2L_API int w2l_stream_create_for_trainer(void* trainer, int slots, int maxChunk, void** session) {
  return w2l_stream_create_for_trainer_ex(trainer, slots, maxChunk, W2L_STREAM_FP32, session);
}

W2L_API void w2l_stream_destroy(void* session) { delete (Session*)session; }

W2L_API int w2l_stream_query_ex(const char* archText, int nFeat, int nLabel, int slots, int maxChunk, int precision, int* maxOut,
                                size_t* stateBytes) {
  STREAM_TRY({
    if (!archText) throw std::invalid_argument("stream query: null arch");
    std::unique_ptr<Session> s(buildSession(archText, nFeat, nLabel, slots, maxChunk, precision));
    if (maxOut) *maxOut = s->maxOut;
    if (stateBytes) *stateBytes = s->stateBytes;
  });
}

W2L_API int w2l_stream_query(const char* archText, int nFeat, int nLabel, int slots, int maxChunk, int* maxOut, size_t* stateBytes) {
  return w2l_stream_query_ex(archText, nFeat, nLabel, slots, maxChunk, W2L_STREAM_FP32, maxOut, stateBytes);
}

// pure host: the next step of a BF16 session copies the parameters and writes the weight images again
W2L_API int w2l_stream_refresh_weights(void* session) {
  STREAM_TRY({
    if (!session) throw std::invalid_argument("stream refresh weights: null session");
    ((Session*)session)->weightsStale = true;
  });
}

W2L_API int w2l_stream_max_out(void* session) { return session ? ((Session*)session)->maxOut : 0; }
W2L_API size_t w2l_stream_state_bytes(void* session) { return session ? ((Session*)session)->stateBytes : 0; }
W2L_API size_t w2l_stream_param_floats(void* session) { return session ? ((Session*)session)->net->paramFloats() : 0; }
W2L_API int w2l_stream_num_time_layers(void* session) { return session ? (int)((Session*)session)->tl.size() : 0; }

W2L_API int w2l_stream_bind(void* session, const float* params, void* state, size_t stateBytes) {
  STREAM_TRY({
    if (!session) throw std::invalid_argument("stream bind: null session");
    bindSession(*(Session*)session, params, state, stateBytes);
  });
}

W2L_API int w2l_stream_counts(void* session, const int* n, const int* start, const int* finish, int* nOut) {
  STREAM_TRY({
    if (!session) throw std::invalid_argument("stream counts: null session");
    Session& s = *(Session*)session;
    std::vector<char> na;
    std::vector<int> nc;
    advance(s, n, start, finish, nullptr, nOut, na, nc);
    s.active.swap(na);
    s.carry.swap(nc);
  });
}

W2L_API int w2l_stream_slot_state(void* session, int slot, int* active, int* carry, int carryCap) {
  STREAM_TRY({
    if (!session) throw std::invalid_argument("stream slot state: null session");
    Session& s = *(Session*)session;
    if (slot < 0 || slot >= s.S) throw std::invalid_argument("stream slot state: no such slot");
    if (active) *active = s.active[slot];
    for (int k = 0; carry && k < carryCap && k < (int)s.tl.size(); ++k) carry[k] = s.carry[(size_t)slot * s.tl.size() + k];
  });
}

W2L_API int w2l_stream_step(void* session, const float* x, const int* n, const int* start, const int* finish, const float** out, int* nOut,
                            void* stream) {
  STREAM_TRY({
    if (!session) throw std::invalid_argument("stream step: null session");
    stepSession(*(Session*)session, x, n, start, finish, out, nOut, (hipStream_t)stream);
  });
}

W2L_API int w2l_stream_reset(void* session, int slot) {
  STREAM_TRY({
    if (!session) throw std::invalid_argument("stream reset: null session");
    Session& s = *(Session*)session;
    if (slot < 0 || slot >= s.S) throw std::invalid_argument("stream reset: no such slot");
    s.active[slot] = 0;
    for (size_t k = 0; k < s.tl.size(); ++k) s.carry[(size_t)slot * s.tl.size() + k] = 0;
  });
}
