// trainer.cpp -- one optimisation step of the acoustic-model trainer and its C ABI.
// Step order restated from the reference's hot loop (recipes/slimIPL/src/Train.cpp):
//   forward network :1463-1470 -> criterion forward :1675 -> zeroGrad + loss.backward() :1718-1720
//   -> all-reduce of all gradients :1721-1735 (here: ONE collective over the flat arena,
//   issued by the caller between w2l_trainer_forward_backward and w2l_trainer_update)
//   -> grads / totalBatchSize :1748-1784 -> clipGradNorm :1791-1798 -> critopt/netopt step :1801-1802.
// The five af::sync() per step of the reference are gone: a step enqueues ~500 kernels
// on one stream and never blocks the host.
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include <algorithm>

#include "w2l_host.hpp"

namespace w2l {

struct Trainer {
  std::shared_ptr<Sequential> net;
  std::shared_ptr<SequenceCriterion> crit;
  int nFeat = 0, nLabel = 0;
  std::string critName;
  std::string archText;   // as given: a streaming session builds a network of its own from it (host/stream.cpp)
  // geometry
  int B = 0, T = 0, L = 0, Tout = 0;
  size_t netFloats = 0, critFloats = 0, arenaFloats = 0, critWsBytes = 0;
  // bound device memory (owned by the caller)
  float *params = nullptr, *grads = nullptr, *mom = nullptr, *arena = nullptr;
  void* critWs = nullptr;
  float *loss = nullptr, *gradLoss = nullptr, *dEm = nullptr;
  // acc[8] of w2l_grad_guard (include/w2l_hip.h): [2] the last update's squared norm, [4] the count of skipped updates.  Owned, on
  // the DEVICE, allocated and zeroed once (guardBuf) and kept across w2l_trainer_plan / w2l_trainer_bind: both are facts of the
  // run, not of a plan.  (The activation arena keeps the 64 floats it used to lend them, unused: arena sizes do not move.)
  double* sumsq = nullptr;
  double* guardBuf() {
    if (!sumsq) {
      hipCheck(hipMalloc((void**)&sumsq, 8 * sizeof(double)), "guard accumulators");
      hipCheck(hipMemset(sumsq, 0, 8 * sizeof(double)), "guard accumulators");
      hipCheck(hipStreamSynchronize(nullptr), "guard accumulators");   // once: whatever stream the first update runs on sees the zeros
    }
    return sumsq;
  }
  float* batchSlot = nullptr;  // grads[paramFloats]: this rank's utterance count, summed by the SAME all-reduce as the gradients
  const float* emission = nullptr;
  uint32_t step = 0;
  std::shared_ptr<SequenceCriterion> linseg;  // --linseg warm-up criterion (ASG only), used while step < linsegUpdates
  uint32_t linsegUpdates = 0;
  int scaleMode = 0;
  SequenceCriterion* activeCrit() { return (linseg && step < linsegUpdates) ? linseg.get() : crit.get(); }
  std::string lastError;
  int netOptim = 0, critOptim = 0;  // 0 SGD(momentum), 1 Adagrad (variance in the momentum arena), 2 Adadelta (+ state2), 3 Adam (+ state2)
  float adamBeta1 = 0.9f, adamBeta2 = 0.999f, adamEps = 1e-8f, adamWd = 0.f;   // w2l_trainer_set_adam
  // Adam's applied-step counts [network, criterion], owned, on the DEVICE: the update is skipped there (grad_guard_k) and a
  // skipped update must not advance the bias correction.  A buffer of its own (the acc array of w2l_grad_guard keeps its layout).
  uint64_t* adamSteps = nullptr;
  uint64_t* adamStepsBuf() {
    if (!adamSteps) {
      hipCheck(hipMalloc((void**)&adamSteps, 2 * sizeof(uint64_t)), "Adam step counts");
      hipCheck(hipMemset(adamSteps, 0, 2 * sizeof(uint64_t)), "Adam step counts");
      hipCheck(hipStreamSynchronize(nullptr), "Adam step counts");   // once: whatever stream the first update runs on sees the zeros
    }
    return adamSteps;
  }
  const float* inputSizes = nullptr;  // w2l_trainer_set_input_sizes
  float* state2 = nullptr;          // Adadelta's accDelta / Adam's v, same size and layout as the momentum arena
  bool mixedPrecision = false;   // fl's --fl_amp_use_mixed_precision, restated for bf16: the network's fl::Linear GEMMs multiply
                                 // in bf16 (fp32 accumulate, fp32 storage, fp32 master weights); convolutions, LayerNorm, the
                                 // criterion and the optimizer stay fp32
  std::vector<hipEvent_t> bucketEvents;  // owned (w2l_trainer_set_grad_buckets)
  // w2l_trainer_evaluate's loss [B], path [B][T'] and criterion score workspace, apart from every buffer a training step reads
  // or writes: the caller's (w2l_trainer_bind_eval) or, when none is bound, owned and grown on demand
  void* evalMem = nullptr;
  size_t evalBytes = 0;
  void* evalBound = nullptr;
  size_t evalBoundBytes = 0;
  size_t evalNeed() const {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    return up(sizeof(float) * B) + up(sizeof(int) * (size_t)B * Tout) + up(crit->scoreWorkspaceBytes(B, Tout, nLabel, L));
  }
  ~Trainer() {
    for (auto e : bucketEvents) (void)hipEventDestroy(e);
    if (evalMem) (void)hipFree(evalMem);
    if (adamSteps) (void)hipFree(adamSteps);
    if (sumsq) (void)hipFree(sumsq);
  }
};

}  // namespace w2l

using namespace w2l;

#define W2L_API extern "C" __attribute__((visibility("default")))
#define TRY(h, body)                                   \
  try { body; return W2L_OK; }                         \
  catch (const std::invalid_argument& e) { if (h) ((Trainer*)h)->lastError = e.what(); g_err = e.what(); return W2L_EINVAL; } \
  catch (const std::exception& e) { if (h) ((Trainer*)h)->lastError = e.what(); g_err = e.what(); return W2L_EHIP; }

static thread_local std::string g_err;

W2L_API const char* w2l_host_last_error(void) { return g_err.c_str(); }
namespace w2l {
void setHostError(const std::string& m) { g_err = m; }   // for the host entry points of other files (ngram_lm.cpp)
// what a streaming session over a trainer reads (host/stream.cpp): its arch once, its bound parameters and mode at every step
void trainerArch(void* h, std::string& archText, int& nFeat, int& nLabel) {
  Trainer* t = (Trainer*)h;
  archText = t->archText; nFeat = t->nFeat; nLabel = t->nLabel;
}
const float* trainerParams(void* h, bool& mixedPrecision) {
  Trainer* t = (Trainer*)h;
  mixedPrecision = t->mixedPrecision;
  return t->params;
}
bool trainerMixedConvs(void* h) { return ((Trainer*)h)->net->mixedPrecisionConvs(); }
}

// criterion: "ctc" | "asg" ; archText: contents of an .arch file (NFEAT/NLABEL substituted here)
W2L_API void* w2l_trainer_create(const char* archText, int nFeat, int nLabel, const char* criterion,
                                 int scaleMode, double transdiag) {
  try {
    auto t = new Trainer();
    t->nFeat = nFeat; t->nLabel = nLabel; t->critName = criterion ? criterion : "ctc"; t->scaleMode = scaleMode;
    t->archText = archText ? archText : "";
    t->net = buildSequentialFromText(archText, nFeat, nLabel);
    if (t->critName == "ctc") t->crit = makeCTCLoss(scaleMode);
    else if (t->critName == "asg") t->crit = makeASGLoss(nLabel, scaleMode, transdiag);
    else { delete t; throw std::invalid_argument("unsupported criterion: " + std::string(criterion)); }
    t->netFloats = t->net->paramFloats();
    t->critFloats = t->crit->paramFloats();
    return t;
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}

W2L_API void w2l_trainer_destroy(void* h) { delete (Trainer*)h; }

W2L_API size_t w2l_trainer_param_floats(void* h) { Trainer* t = (Trainer*)h; return t->netFloats + t->critFloats; }
W2L_API size_t w2l_trainer_net_param_floats(void* h) { return ((Trainer*)h)->netFloats; }
// size of the GRADIENT arena the caller binds: parameters + a 4-float tail whose first element carries the local
// batch size through the gradient all-reduce (the reference all-reduces it separately, Train.cpp:1743-1747)
W2L_API size_t w2l_trainer_grad_floats(void* h) { Trainer* t = (Trainer*)h; return t->netFloats + t->critFloats + 4; }
W2L_API int w2l_trainer_num_params(void* h) { return (int)((Trainer*)h)->net->params().size(); }
W2L_API const char* w2l_trainer_describe(void* h) {
  Trainer* t = (Trainer*)h;
  t->lastError = t->net->prettyString() + " | criterion: " + t->crit->prettyString();
  return t->lastError.c_str();
}
// name / numel / offset of network parameter i (internal arena order = Flashlight params() order)
W2L_API int w2l_trainer_param_info(void* h, int i, char* name, int nameCap, size_t* numel, size_t* offset) {
  Trainer* t = (Trainer*)h;
  if (i < 0 || i >= (int)t->net->params().size()) return W2L_EINVAL;
  const ParamInfo& p = t->net->params()[i];
  if (name && nameCap > 0) { std::strncpy(name, p.name.c_str(), nameCap - 1); name[nameCap - 1] = 0; }
  if (numel) *numel = p.numel;
  if (offset) *offset = p.offset;
  return W2L_OK;
}

// host-side parameter helpers (h_* are HOST pointers)
W2L_API int w2l_trainer_init_params(void* h, float* h_params, uint64_t seed) {
  Trainer* t = (Trainer*)h;
  TRY(h, { t->net->initParams(h_params, seed); t->crit->initParams(h_params + t->netFloats); });
}
W2L_API int w2l_trainer_import_param(void* h, int i, const float* h_ref, float* h_params) {
  Trainer* t = (Trainer*)h;
  TRY(h, { if (i < 0 || i >= (int)t->net->params().size()) throw std::invalid_argument("bad param index"); t->net->importParam(i, h_ref, h_params); });
}
W2L_API int w2l_trainer_export_param(void* h, int i, const float* h_arena, float* h_ref) {
  Trainer* t = (Trainer*)h;
  TRY(h, { if (i < 0 || i >= (int)t->net->params().size()) throw std::invalid_argument("bad param index"); t->net->exportParam(i, h_arena, h_ref); });
}

// plan for a batch geometry: B utterances of T frames, targets padded to L.  A plan DROPS what belonged to the one before: the
// arena and criterion-workspace binding (sized for the old shape), the emission pointer of the last forward (Sequential::plan has
// forgotten that pass) and the input sizes (B of them, of the old B) -- w2l_trainer_bind, and w2l_trainer_set_input_sizes where
// sizes are used, come again before the next pass.  Everything else stays: parameters, gradients and optimizer arenas, the step
// count, Adam's counts, the guard's count and last norm, optimizer kind and hyperparameters, the precision switches, dropout
// overrides, gradient buckets, the linseg countdown.
W2L_API int w2l_trainer_plan(void* h, int B, int T, int L, size_t* arenaFloats, size_t* critWsBytes,
                             int* Tout) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    if (B <= 0 || T <= 0 || L <= 0) throw std::invalid_argument("plan: B, T, L must be positive");
    t->arena = nullptr; t->critWs = nullptr; t->emission = nullptr; t->inputSizes = nullptr;
    t->dEm = t->loss = t->gradLoss = nullptr;
    t->arenaFloats = 0;   // (a plan that throws leaves no plan)
    size_t used = t->net->plan(B, T, t->nFeat);
    t->B = B; t->T = T; t->L = L;
    t->Tout = t->net->outAct().T;
    if (t->net->outAct().F != t->nLabel) throw std::invalid_argument("network output width != NLABEL");
    const size_t bSlots = ((size_t)B + 63) / 64 * 64;
    size_t extra = ((size_t)B * t->Tout * t->nLabel + 63) / 64 * 64 + 2 * bSlots + 64;  // dEmission, loss, gradLoss, guard doubles
    t->arenaFloats = used + extra;
    t->critWsBytes = t->crit->workspaceBytes(B, t->Tout, t->nLabel, L);
    if (t->linseg) t->critWsBytes = std::max(t->critWsBytes, t->linseg->workspaceBytes(B, t->Tout, t->nLabel, L));
    if (arenaFloats) *arenaFloats = t->arenaFloats;
    if (critWsBytes) *critWsBytes = t->critWsBytes;
    if (Tout) *Tout = t->Tout;
  });
}

// all device pointers; params/grads/momentum hold net params followed by criterion params
W2L_API int w2l_trainer_bind(void* h, float* params, float* grads, float* momentum, float* arena,
                             void* critWs) {
  Trainer* t = (Trainer*)h;
  if (!params || !grads || !arena || !critWs || !t->arenaFloats) return W2L_EINVAL;
  t->params = params; t->grads = grads; t->mom = momentum; t->arena = arena; t->critWs = critWs;
  const size_t bSlots = ((size_t)t->B + 63) / 64 * 64;
  const size_t emSlots = ((size_t)t->B * t->Tout * t->nLabel + 63) / 64 * 64;
  size_t used = t->arenaFloats - (emSlots + 2 * bSlots + 64);
  t->dEm = arena + used;
  t->loss = t->dEm + emSlots;
  t->gradLoss = t->loss + bSlots;
  t->batchSlot = grads + t->netFloats + t->critFloats;   // (the arena's last 64 floats: unused, once the guard accumulators)
  t->emission = nullptr;   // a pass in another arena is not this binding's to differentiate
  return W2L_OK;
}

static void requireBound(Trainer* t) {
  if (!t->arenaFloats || !t->params || !t->grads || !t->arena || !t->critWs)
    throw std::invalid_argument("trainer not planned / bound (w2l_trainer_plan + w2l_trainer_bind first)");
}

struct MatmulMode {   // scoped: the mode only covers the network's own calls (the criterion stays fp32)
  int prev;
  bool on;
  explicit MatmulMode(bool bf16) : prev(0), on(bf16) { if (on) prev = w2l_set_matmul_precision(1); }
  ~MatmulMode() { if (on) w2l_set_matmul_precision(prev); }
};

static Ctx makeCtx(Trainer* t, void* stream, bool train) {
  requireBound(t);
  Ctx c;
  c.stream = (hipStream_t)stream;
  c.train = train;
  c.seed = 0x9E3779B9u * (t->step + 1);
  c.params = t->params;
  c.grads = t->grads;
  c.inputSizes = t->inputSizes; c.inputT = t->T;
  c.bf16 = t->mixedPrecision;
  return c;
}

// network forward only (eval mode when train == 0); returns the device pointer of emissions [B][T'][N]
W2L_API int w2l_trainer_forward(void* h, const float* x, int train, const float** emission, void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    requireBound(t);
    if (!x) throw std::invalid_argument("forward: null input");
    Ctx c = makeCtx(t, stream, train != 0);
    { MatmulMode mm(t->mixedPrecision); t->emission = t->net->forward(c, t->arena, x); }
    if (emission) *emission = t->emission;
  });
}

// forward + criterion + backward: leaves every gradient (network ‖ criterion) in the grads
// arena, UNSCALED (sum over the utterances of this rank).  loss_out (device, [B]) optional.
W2L_API int w2l_trainer_forward_backward(void* h, const float* x, const int* target, float** lossDev,
                                         void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    requireBound(t);
    if (!x || !target) throw std::invalid_argument("forward_backward: null input");   // before anything is enqueued with them
    Ctx c = makeCtx(t, stream, true);
    { MatmulMode mm(t->mixedPrecision); t->emission = t->net->forward(c, t->arena, x); }
    float* cp = t->params + t->netFloats;
    float* cg = t->grads + t->netFloats;
    SequenceCriterion* crit = t->activeCrit();
    crit->forward(c, t->B, t->Tout, t->nLabel, t->L, t->emission, target, t->loss, t->critWs, cp);
    // d(sum_b loss_b)/d loss_b = 1
    hipCheck(hipMemsetAsync(t->gradLoss, 0, sizeof(float) * (((size_t)t->B + 63) / 64 * 64), c.stream), "memset");
    w2lCheck(w2l_fill(t->gradLoss, (size_t)t->B, 1.f, c.stream), "fill");
    w2lCheck(w2l_fill(t->batchSlot, 1, (float)t->B, c.stream), "batch slot");  // rides the gradient all-reduce
    hipCheck(hipMemsetAsync(t->batchSlot + 1, 0, sizeof(float) * 3, c.stream), "memset");
    crit->backward(c, t->B, t->Tout, t->nLabel, t->L, t->emission, target, t->gradLoss, t->dEm, t->critWs, cp, cg);
    { MatmulMode mm(t->mixedPrecision); t->net->backward(c, t->arena, t->dEm); }
    if (lossDev) *lossDev = t->loss;
  });
}

// backward pass of the NETWORK alone from a caller-supplied gradient of the emissions [B][T'][N] -- the fl::Module boundary for
// a binder that keeps its own criterion (and the hook of the teacher-forced per-layer parity tests).  Call after
// w2l_trainer_forward(train = 1) of the same step: leaves the network's gradients in the grads arena (unscaled), the
// criterion's part untouched.
W2L_API int w2l_trainer_backward(void* h, const float* dEmission, void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    requireBound(t);
    if (!dEmission) throw std::invalid_argument("backward: null gradient");
    if (!t->emission) throw std::invalid_argument("backward: no forward pass to differentiate");
    Ctx c = makeCtx(t, stream, true);
    { MatmulMode mm(t->mixedPrecision); t->net->backward(c, t->arena, dEmission); }
  });
}

// optimizer: grads *= 1/totalBatch, global-norm clip (network, and criterion if clampCrit), SGD+momentum
// on the network (lr, momentum), plain SGD on the criterion (lrcrit)  [Train.cpp:577-582, :1791-1802]
W2L_API int w2l_trainer_update(void* h, float lr, float lrcrit, float momentum, float maxGradNorm,
                               float totalBatch, int clampCrit, void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    requireBound(t);
    hipStream_t s = (hipStream_t)stream;
    // totalBatch > 0: the caller's number; <= 0: the all-reduced utterance count in the gradient arena's tail
    const float gs = totalBatch > 0.f ? 1.f / totalBatch : 0.f;
    // what the chosen optimizers need bound, before anything is enqueued
    const bool needState = t->netOptim != 0 || (t->critOptim != 0 && t->critFloats);
    const bool needState2 = t->netOptim >= 2 || (t->critOptim >= 2 && t->critFloats);
    if (needState && !t->mom) throw std::invalid_argument("Adagrad / Adadelta need the momentum arena bound (it holds the gradient statistics)");
    if (needState2 && !t->state2) throw std::invalid_argument("Adadelta needs w2l_trainer_bind_state2");
    t->guardBuf();
    // --linseg: the reference trains the warm-up phase with its OWN optimizers (linNetoptim / linCritoptim,
    // Train.cpp:589-617), so the ASG phase proper starts from fresh optimizer state: clear the momentum arena -- SGD
    // velocity, or the Adagrad / Adadelta / Adam gradient statistics it holds --, the second arena of Adadelta and Adam, and
    // Adam's step counts at the switch
    if (t->linseg && t->linsegUpdates && t->step == t->linsegUpdates) {
      const bool stateful = momentum != 0.f || t->netOptim != 0 || t->critOptim != 0;
      if (t->mom && stateful)
        hipCheck(hipMemsetAsync(t->mom, 0, sizeof(float) * (t->netFloats + t->critFloats), s), "linseg optimizer-state reset");
      if (t->state2 && (t->netOptim >= 2 || t->critOptim >= 2))
        hipCheck(hipMemsetAsync(t->state2, 0, sizeof(float) * (t->netFloats + t->critFloats), s), "linseg optimizer-state reset");
      if (t->adamSteps) hipCheck(hipMemsetAsync(t->adamSteps, 0, 2 * sizeof(uint64_t), s), "linseg optimizer-state reset");
    }
    // the norm is taken on EVERY update (also with --maxgradnorm=0): it is the non-finite guard of the step
    w2lCheck(w2l_sumsq(t->grads, t->netFloats, t->sumsq, 1, s), "sumsq");
    w2lCheck(w2l_sumsq(t->grads + t->netFloats, t->critFloats, t->sumsq + 1, 1, s), "sumsq");
    w2lCheck(w2l_grad_guard(t->sumsq, totalBatch > 0.f ? nullptr : t->batchSlot, clampCrit, s), "guard");
    uint64_t* adamSteps = (t->netOptim == 3 || (t->critOptim == 3 && t->critFloats)) ? t->adamStepsBuf() : nullptr;
    auto stepOne = [&](int kind, size_t off, size_t n, float rate, float mom, float clip, const char* what) {
      float* v = t->mom ? t->mom + off : nullptr;
      if (kind == 1)
        w2lCheck(w2l_adagrad_step_guarded(t->params + off, t->grads + off, v, n, rate, 1e-8f, gs, clip, t->sumsq + 2, s), what);
      else if (kind == 2)
        w2lCheck(w2l_adadelta_step_guarded(t->params + off, t->grads + off, v, t->state2 + off, n, rate, 0.9f, 1e-8f, gs, clip, t->sumsq + 2, s), what);
      else if (kind == 3)   // (weight decay: the network group only, cpc/Train.cpp:569-580)
        w2lCheck(w2l_adam_step_guarded(t->params + off, t->grads + off, v, t->state2 + off, n, rate, t->adamBeta1, t->adamBeta2, t->adamEps,
                                       off ? 0.f : t->adamWd, gs, clip, t->sumsq + 2, 0, adamSteps + (off ? 1 : 0), s), what);
      else
        w2lCheck(w2l_sgd_step_guarded(t->params + off, t->grads + off, mom != 0.f ? v : nullptr, n, rate, mom, gs, clip, t->sumsq + 2, s), what);
    };
    if (t->critFloats) stepOne(t->critOptim, t->netFloats, t->critFloats, lrcrit, 0.f, clampCrit ? maxGradNorm : 0.f, "criterion optimizer");
    stepOne(t->netOptim, 0, t->netFloats, lr, momentum, maxGradNorm, "network optimizer");
    t->step++;
  });
}

// eval-mode network forward (no dropout) + the criterion's score on the planned shape.  Advances no counter: the dropout seed of
// the next training step comes from the update count alone (makeCtx), and the criterion scores on a workspace of its own.
static void evaluateImpl(Trainer* t, const float* x, const int* target, float** lossDev, int** pathDev, void* stream) {
  requireBound(t);
  if (!x || !target) throw std::invalid_argument("evaluate: null input");
  Ctx c = makeCtx(t, stream, false);
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t lossBytes = up(sizeof(float) * t->B), pathBytes = up(sizeof(int) * (size_t)t->B * t->Tout);
  const size_t need = t->evalNeed();
  char* mem = (char*)t->evalBound;
  if (mem && t->evalBoundBytes < need) throw std::invalid_argument("evaluate: the bound buffer is smaller than w2l_trainer_eval_bytes");
  if (!mem) {
    if (need > t->evalBytes) {
      if (t->evalMem) { hipCheck(hipFree(t->evalMem), "evaluate buffers"); t->evalMem = nullptr; t->evalBytes = 0; }
      hipCheck(hipMalloc(&t->evalMem, need), "evaluate buffers");
      t->evalBytes = need;
    }
    mem = (char*)t->evalMem;
  }
  float* loss = (float*)mem;
  int* path = (int*)(mem + lossBytes);
  void* ws = mem + lossBytes + pathBytes;
  const float* em;
  { MatmulMode mm(t->mixedPrecision); em = t->net->forward(c, t->arena, x); }
  t->crit->score(c, t->B, t->Tout, t->nLabel, t->L, em, target, loss, path, ws, t->params + t->netFloats);
  if (lossDev) *lossDev = loss;
  if (pathDev) *pathDev = path;
}
W2L_API int w2l_trainer_evaluate(void* h, const float* x, const int* target, float** lossDev, int** pathDev, void* stream) {
  TRY(h, evaluateImpl((Trainer*)h, x, target, lossDev, pathDev, stream));
}

// bytes of the buffer w2l_trainer_evaluate needs on the planned shape; w2l_trainer_bind_eval hands one over (null: the trainer's own)
W2L_API size_t w2l_trainer_eval_bytes(void* h) {
  Trainer* t = (Trainer*)h;
  return (t && t->arenaFloats) ? t->evalNeed() : 0;
}
W2L_API int w2l_trainer_bind_eval(void* h, void* mem, size_t bytes) {
  if (!h || (mem && !bytes)) return W2L_EINVAL;
  Trainer* t = (Trainer*)h;
  t->evalBound = mem;
  t->evalBoundBytes = mem ? bytes : 0;
  return W2L_OK;
}

W2L_API int w2l_trainer_viterbi(void* h, const float* emission, int* path, void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    Ctx c = makeCtx(t, stream, false);
    t->crit->viterbiPath(c, t->B, t->Tout, t->nLabel, emission, path, t->critWs, t->params + t->netFloats);
  });
}

// Gradient buckets for the data-parallel overlap (fl's CoalescingReducer, recipes/slimIPL/src/Train.cpp:1721-1735,
// restated for one flat arena): offsets[0..n) ascending float offsets into the gradient arena, bucket k =
// [offsets[k], offsets[k+1]) and the last one runs to the end (criterion gradients included).  During
// w2l_trainer_forward_backward an event per bucket is recorded on the step's stream once every gradient at
// offset >= offsets[k] is final; w2l_trainer_wait_bucket makes another stream (the collective's) wait for it.
// n = 0 removes the hooks.
W2L_API int w2l_trainer_set_grad_buckets(void* h, int n, const size_t* offsets) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    if (n < 0 || (n > 0 && !offsets)) throw std::invalid_argument("set_grad_buckets: bad arguments");
    for (int k = 1; k < n; ++k)
      if (offsets[k] <= offsets[k - 1]) throw std::invalid_argument("set_grad_buckets: offsets must ascend");
    for (auto e : t->bucketEvents) (void)hipEventDestroy(e);
    t->bucketEvents.clear();
    std::vector<size_t> off(offsets, offsets + n);
    for (int k = 0; k < n; ++k) {
      hipEvent_t e;
      hipCheck(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
      t->bucketEvents.push_back(e);
    }
    t->net->setGradBuckets(off, t->bucketEvents);
  });
}
W2L_API int w2l_trainer_wait_bucket(void* h, int k, void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    if (k < 0 || k >= (int)t->bucketEvents.size()) throw std::invalid_argument("wait_bucket: no such bucket");
    hipCheck(hipStreamWaitEvent((hipStream_t)stream, t->bucketEvents[k], 0), "hipStreamWaitEvent");
  });
}

// --linseg=n (Train.cpp:589-617, :1866-1883): the first n updates of an ASG run use LinSegCriterion on the ASG
// criterion's own transitions.  Call before w2l_trainer_plan (the criterion workspace is sized for both).
W2L_API int w2l_trainer_set_linseg(void* h, uint32_t updates) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    if (updates && t->critName != "asg") throw std::invalid_argument("linseg may only be used with ASG criterion");
    t->linsegUpdates = updates;
    t->linseg = updates ? makeLinSegCriterion(t->nLabel, t->scaleMode) : nullptr;
    t->arenaFloats = 0;  // forces a new plan / bind
    t->params = t->grads = t->mom = t->arena = nullptr;
    t->critWs = nullptr;
  });
}

// gradient norm of the last w2l_trainer_update (sqrt of the clipped-norm accumulator, BEFORE the 1/totalBatch scale);
// NaN / Inf means that update was skipped.  Synchronises `stream`.
W2L_API int w2l_trainer_grad_norm(void* h, double* norm, void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    if (!t || !norm) throw std::invalid_argument("grad_norm: null argument");
    double s = 0.0;
    if (t->sumsq) {   // (never allocated: no update has run, the norm is 0)
      hipCheck(hipMemcpyAsync(&s, t->sumsq + 2, sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream), "grad norm");
      hipCheck(hipStreamSynchronize((hipStream_t)stream), "grad norm");
    }
    *norm = std::sqrt(s);
  });
}

// number of updates skipped so far because the (all-reduced) gradient or batch size was non-finite.  Synchronises.
W2L_API int w2l_trainer_skipped_updates(void* h, uint64_t* count, void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    if (!t || !count) throw std::invalid_argument("skipped_updates: null argument");
    double s = 0.0;
    if (t->sumsq) {   // (never allocated: no update has run)
      hipCheck(hipMemcpyAsync(&s, t->sumsq + 4, sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream), "skipped");
      hipCheck(hipStreamSynchronize((hipStream_t)stream), "skipped");
    }
    *count = (uint64_t)s;
  });
}

W2L_API int w2l_trainer_set_optimizer(void* h, int netKind, int critKind) {
  if (!h || netKind < 0 || netKind > 3 || critKind < 0 || critKind > 3) return W2L_EINVAL;
  ((Trainer*)h)->netOptim = netKind; ((Trainer*)h)->critOptim = critKind;
  return W2L_OK;
}
W2L_API int w2l_trainer_set_adam(void* h, float beta1, float beta2, float eps, float weightDecay) {
  if (!h || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f) || !(weightDecay >= 0.f)) return W2L_EINVAL;
  Trainer* t = (Trainer*)h;
  t->adamBeta1 = beta1; t->adamBeta2 = beta2; t->adamEps = eps; t->adamWd = weightDecay;
  return W2L_OK;
}
W2L_API int w2l_trainer_adam_steps(void* h, uint64_t* netSteps, uint64_t* critSteps, void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    if (!t || !netSteps || !critSteps) throw std::invalid_argument("adam_steps: null argument");
    uint64_t c[2];
    c[0] = c[1] = 0;
    if (t->adamSteps) {   // (never allocated: no Adam update has run and none was set)
      hipCheck(hipMemcpyAsync(c, t->adamSteps, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream), "adam_steps");
      hipCheck(hipStreamSynchronize((hipStream_t)stream), "adam_steps");
    }
    *netSteps = c[0]; *critSteps = c[1];
  });
}
W2L_API int w2l_trainer_set_adam_steps(void* h, uint64_t netSteps, uint64_t critSteps, void* stream) {
  Trainer* t = (Trainer*)h;
  TRY(h, {
    if (!t) throw std::invalid_argument("set_adam_steps: null handle");
    uint64_t c[2];
    c[0] = netSteps; c[1] = critSteps;
    hipCheck(hipMemcpyAsync(t->adamStepsBuf(), c, sizeof(c), hipMemcpyHostToDevice, (hipStream_t)stream), "set_adam_steps");
    hipCheck(hipStreamSynchronize((hipStream_t)stream), "set_adam_steps");
  });
}
W2L_API int w2l_trainer_set_input_sizes(void* h, const float* inputSizesDev) {
  if (!h) return W2L_EINVAL;
  ((Trainer*)h)->inputSizes = inputSizesDev;
  return W2L_OK;
}
W2L_API int w2l_trainer_bind_state2(void* h, float* state2) {
  if (!h) return W2L_EINVAL;
  ((Trainer*)h)->state2 = state2;
  return W2L_OK;
}
W2L_API int w2l_trainer_set_mixed_precision(void* h, int on) { ((Trainer*)h)->mixedPrecision = on != 0; return W2L_OK; }

// the fp32 backward's weight, bias and filter gradients on the network's own side stream, joined into the caller's stream before
// w2l_trainer_forward_backward / w2l_trainer_backward return (Sequential::setWeightGradStream; on by default).  Same results either
// way; acts from the next backward on.
W2L_API int w2l_trainer_set_weight_grad_stream(void* h, int on) {
  if (!h) return W2L_EINVAL;
  ((Trainer*)h)->net->setWeightGradStream(on != 0);
  return W2L_OK;
}

// the data gradient of the network's input, which a training step has no use for: off by default.  On: every backward from the
// next one on leaves it in the activation arena, frame-major [B][T][NFEAT] (the input arrives time-fastest, [B][NFEAT][T]);
// w2l_trainer_input_gradient hands out where (null before the first such backward).  The parameter gradients are the same either way.
W2L_API int w2l_trainer_set_input_gradient(void* h, int on) {
  if (!h) return W2L_EINVAL;
  ((Trainer*)h)->net->setInputGradient(on != 0);
  return W2L_OK;
}
W2L_API int w2l_trainer_input_gradient(void* h, const float** dInput) {
  if (!h || !dInput) return W2L_EINVAL;
  *dInput = ((Trainer*)h)->net->inputGradient();
  return W2L_OK;
}

// second level of the mixed-precision mode: the wide time convolutions (H == 1, >= 32 channels: the conv_glu recipes, the
// Transformer front end) on bf16 operands too, wherever w2l_conv_bf16_image_elems has a kernel.  It acts only while
// w2l_trainer_set_mixed_precision is on.  The plan holds the layers' weight images and the image scratch: call before
// w2l_trainer_plan -- a change after it drops the plan (plan and bind again, as after w2l_trainer_set_linseg).
W2L_API int w2l_trainer_set_mixed_precision_convs(void* h, int on) {
  if (!h) return W2L_EINVAL;
  Trainer* t = (Trainer*)h;
  if (t->net->mixedPrecisionConvs() == (on != 0)) return W2L_OK;
  t->net->setMixedPrecisionConvs(on != 0);
  t->arenaFloats = 0;
  t->params = t->grads = t->mom = t->arena = nullptr;
  t->critWs = nullptr;
  return W2L_OK;
}

// slimIPL's dynamic dropout: the `TR` layers' probabilities from the next forward on (negative: the arch line's)
W2L_API int w2l_trainer_set_dropout(void* h, double pDropout, double pLayerDrop) {
  if (!h || !(pDropout < 1.0) || !(pLayerDrop < 1.0)) return W2L_EINVAL;   // (NaN fails the comparison)
  ((Trainer*)h)->net->setTransformerDropout(pDropout, pLayerDrop);
  return W2L_OK;
}

W2L_API int w2l_trainer_set_step(void* h, uint32_t step) { ((Trainer*)h)->step = step; return W2L_OK; }

// arch / flags parsing without building kernels (recipes must load unchanged)
W2L_API int w2l_arch_check(const char* archText, int nFeat, int nLabel, int* numLayers) {
  TRY(nullptr, { auto v = parseArch(archText, nFeat, nLabel); if (numLayers) *numLayers = (int)v.size(); });
}
W2L_API int w2l_flags_check(const char* flagsText, int* numFlags) {
  TRY(nullptr, { auto f = parseFlagsText(flagsText); checkFlagDependencies(f); if (numFlags) *numFlags = (int)f.kv.size(); });
}
