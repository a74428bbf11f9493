/*
 * fl_compat/flashlight.h -- the Flashlight (<= 0.3.2) surface the wav2letter recipes' Trainer touches on the
 * acoustic-training hot path, re-hosted on libw2l_hip.so (hand-written HIP for gfx950; no ArrayFire).
 *
 * BASELINE.json north_star: "host code stays C++ and exposes the same fl::Module / SequenceCriterion /
 * fl::app::asr::Trainer surface so recipes/ configs load unchanged".  What is mirrored, with the reference file:line
 * that shows each shape (Flashlight itself is un-vendored, so the in-repo USES are the witnesses):
 *
 *   af::dim4, af::array (device buffer + dims in ArrayFire order, d0 fastest)    every call site below
 *   fl::Variable, fl::input / fl::noGrad, .array() .dims() .grad() .backward()   recipes/slimIPL/src/Train.cpp:1454-1470, :1718-1720
 *   fl::Module / Container / Sequential: forward(std::vector<Variable>),
 *       params(), param(i), setParams(), train(), eval(), prettyString()         recipes/slimIPL/100h_supervised.cpp:37-75; Train.cpp:396-401
 *   fl::pkg::runtime::ModulePlugin(path).arch(nFeature, nLabel)
 *       -> dlopen + extern "C" fl::Module* createModule(int64_t, int64_t)        recipes/slimIPL/100h_supervised.cpp:84-87; Train.cpp:390-395
 *   fl::pkg::speech::buildSequentialModule(archfile, nFeatures, nClasses)        recipes/joint_training_vox_populi/cpc/SequentialBuilder.h:23-26
 *   fl::pkg::speech::SequenceCriterion { forward({emission (N,T,B), target (L,B)}) -> {loss (B)},
 *       viterbiPath(input, inputSize), viterbiPathWithTarget, prettyString }     recipes/joint_training_vox_populi/cpc/CPCCriterion.h:30-50
 *   ASGLoss(N, scaleMode, transdiag), CTCLoss(scaleMode), getCriterionScaleMode  recipes/slimIPL/src/Train.cpp:389, :406-410
 *   fl::SGDOptimizer(params, lr, momentum, wd), zeroGrad(), step(), setLr();
 *       fl::clipGradNorm(params, maxNorm)                                         recipes/slimIPL/src/Train.cpp:577-582, :1718, :1791-1802
 *
 * Not ArrayFire: af::array here is only a ref-counted device buffer with dims and a dtype (f32 / s32) -- enough to
 * carry tensors across this boundary; arithmetic on arrays belongs to the kernels behind the modules.  Memory order
 * is ArrayFire's (column-major, d0 fastest), so an (N, T, B) emission array IS the [B][T][N] buffer of the C ABI.
 *
 * The network built from an arch file is ONE planned pipeline (static layer list, activations in one arena, the
 * parameters / gradients in flat arenas: w2l_host.hpp); fl::Sequential::modules() lists its lines for prettyString
 * and parameter bookkeeping, the forward / backward run as a whole.  A plugin module (createModule) composes such
 * pipelines -- from arch text, or (round 5) from LAYER OBJECTS the way the reference's plugins are written:
 * fl::View / Reorder / Dropout / ReLU / GatedLinearUnit / LayerNorm / Linear / Conv2D / Pool2D / Transformer / TDSBlock /
 * WeightNorm, constructed with the reference's arguments and add()ed to an fl::Sequential, are their lines of the arch
 * grammar, and the Sequential plans one pipeline out of them on first use (tests/cpp/plugin_layers.cpp).  What is NOT
 * provided is per-layer execution (`modules()[i]->forward(x)`, a custom forward() that interleaves af:: arithmetic, as
 * recipes/slimIPL/100h_supervised.cpp:44-66 does for its padding mask): a free-form per-op autograd is outside the hot
 * path; the padding mask that forward builds is what the planned pipeline's Transformer blocks derive from inputSizes.
 */
#pragma once
#include <stdint.h>
#include <cstdio>
#include <initializer_list>

#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#define FL_COMPAT_API __attribute__((visibility("default")))

namespace af {
typedef long long dim_t;

class FL_COMPAT_API dim4 {
 public:
  dim_t dims[4];
  dim4(dim_t d0 = 1, dim_t d1 = 1, dim_t d2 = 1, dim_t d3 = 1) : dims{d0, d1, d2, d3} {}
  dim_t elements() const { return dims[0] * dims[1] * dims[2] * dims[3]; }
  dim_t ndims() const {
    if (elements() == 0) return 0;
    for (int i = 3; i > 0; --i) if (dims[i] != 1) return i + 1;
    return 1;
  }
  dim_t& operator[](int i) { return dims[i]; }
  const dim_t& operator[](int i) const { return dims[i]; }
  bool operator==(const dim4& o) const { return dims[0] == o.dims[0] && dims[1] == o.dims[1] && dims[2] == o.dims[2] && dims[3] == o.dims[3]; }
  bool operator!=(const dim4& o) const { return !(*this == o); }
};

enum dtype { f32 = 0, s32 = 5 };  // ArrayFire's enumerator values

// ref-counted device buffer; copies share storage (like af::array handles)
class FL_COMPAT_API array {
 public:
  array() {}
  explicit array(const dim4& dims, dtype ty = f32);                       // uninitialised
  array(const dim4& dims, const float* host);                             // afHost source
  array(const dim4& dims, const int* host);
  // fl_compat extension: a view over memory somebody else owns (`owner` keeps it alive; may be null)
  static array wrap(void* dev, const dim4& dims, dtype ty, std::shared_ptr<void> owner = nullptr);
  dim4 dims() const { return dims_; }
  dim_t dims(int i) const { return dims_[i]; }
  dim_t elements() const { return ptr_ ? dims_.elements() : 0; }
  dtype type() const { return type_; }
  bool isempty() const { return elements() == 0; }
  size_t bytes() const { return (size_t)elements() * 4; }
  template <class T> T* device() const { return (T*)ptr_; }                // raw device pointer (no lock bookkeeping)
  void unlock() const {}
  template <class T> void host(T* out) const { hostCopy((void*)out); }     // synchronous device -> host
  template <class T> T scalar() const { T v[1]; if (elements() < 1) throw std::invalid_argument("scalar() of an empty array"); firstElement((void*)v); return v[0]; }
  array copy() const;                                                     // deep copy

 private:
  void hostCopy(void* out) const;
  void firstElement(void* out) const;
  std::shared_ptr<void> owner_;
  void* ptr_ = nullptr;
  dim4 dims_{0, 0, 0, 0};
  dtype type_ = f32;
};

FL_COMPAT_API array constant(double v, const dim4& dims, dtype ty = f32);
FL_COMPAT_API void sync();          // wait for the stream every fl_compat call enqueues on
}  // namespace af

namespace fl {
namespace lib {
namespace audio {
class Mfsc;   // fl_compat/audio.h
}
}

FL_COMPAT_API void* currentStream();                 // hipStream_t the facade enqueues on (default: a private non-blocking stream)
FL_COMPAT_API void setCurrentStream(void* stream);

class FL_COMPAT_API Variable {
 public:
  using GradFunc = std::function<void(std::vector<Variable>& inputs, const Variable& gradOutput)>;
  Variable() : s_(std::make_shared<Shared>()) {}
  Variable(af::array data, bool calcGrad) : s_(std::make_shared<Shared>()) { s_->data = std::move(data); s_->calcGrad = calcGrad; }
  Variable(af::array data, std::vector<Variable> inputs, GradFunc gradFunc);
  af::array& array() const { return s_->data; }
  Variable& grad() const;
  bool isCalcGrad() const { return s_->calcGrad; }
  bool isGradAvailable() const { return s_->grad != nullptr; }
  af::dim4 dims() const { return s_->data.dims(); }
  af::dim_t dims(int i) const { return s_->data.dims(i); }
  af::dim_t elements() const { return s_->data.elements(); }
  af::dtype type() const { return s_->data.type(); }
  bool isempty() const { return s_->data.isempty(); }
  void setCalcGrad(bool b) { s_->calcGrad = b; }
  void addGrad(const Variable& g);            // accumulates (axpy on the device) like Flashlight
  void zeroGrad() { s_->grad.reset(); }
  void backward(bool retainGraph = false);    // d/d(this) with an all-ones seed (a loss vector of B utterances: sum)
  void backward(const Variable& grad, bool retainGraph = false);
  template <class T> T scalar() const { return s_->data.scalar<T>(); }
  template <class T> void host(T* p) const { s_->data.host(p); }

 private:
  struct Shared {
    af::array data;
    std::unique_ptr<Variable> grad;
    bool calcGrad = false;
    std::vector<Variable> inputs;
    GradFunc gradFunc;
  };
  std::shared_ptr<Shared> s_;
  friend struct VariableAccess;
};

// scalar arithmetic the Trainer uses on losses and gradients (`p.grad() = p.grad() / totalBatchSize`,
// recipes/slimIPL/src/Train.cpp:1748-1784): results are plain (no-grad) Variables
FL_COMPAT_API Variable operator*(const Variable& v, double s);
FL_COMPAT_API Variable operator/(const Variable& v, double s);

inline Variable input(const af::array& a) { return Variable(a, false); }
inline Variable noGrad(const af::array& a) { return Variable(a, false); }
inline Variable param(const af::array& a) { return Variable(a, true); }

class FL_COMPAT_API Module {
 public:
  virtual ~Module() {}
  virtual std::vector<Variable> params() const { return params_; }   // (virtual: a Sequential of layer objects plans itself on first use)
  Variable param(int i) const { return params().at(i); }   // (through params(): a Sequential of layer objects plans itself on first use)
  virtual void setParams(const Variable& var, int position);
  virtual void train() { train_ = true; }
  virtual void eval() { train_ = false; }
  bool isTrainMode() const { return train_; }
  void zeroGrad() { for (auto& p : params_) p.zeroGrad(); }
  virtual std::vector<Variable> forward(const std::vector<Variable>& inputs) = 0;
  std::vector<Variable> operator()(const std::vector<Variable>& inputs) { return forward(inputs); }
  virtual std::string prettyString() const = 0;

 protected:
  std::vector<Variable> params_;
  bool train_ = true;
};

class FL_COMPAT_API Container : public Module {
 public:
  virtual void add(std::shared_ptr<Module> m);               // the child's parameters join params() (virtual: a layer object added through a
                                                             //  Container reference to an fl::Sequential still contributes its arch line)
  std::shared_ptr<Module> module(int i) const { return modules_.at(i); }
  std::vector<std::shared_ptr<Module>> modules() const { return modules_; }
  void train() override { train_ = true; for (auto& m : modules_) m->train(); }
  void eval() override { train_ = false; for (auto& m : modules_) m->eval(); }
  void setParams(const Variable& var, int position) override;

 protected:
  std::vector<std::shared_ptr<Module>> modules_;
  std::vector<int> childOfParam_, childIndexOfParam_;
};

// A layer AS AN OBJECT, the way a reference model plugin builds its network (recipes/slimIPL/100h_supervised.cpp:24-43:
// `convFrontend_->add(std::make_shared<fl::Conv2D>(nFeature, 1536, 7, 1, 3, 1, -1, 0, 1, 1))`, `fl::View`, `fl::LayerNorm`,
// `fl::GatedLinearUnit`, `fl::Dropout`, `fl::Reorder`, `fl::Transformer`, `fl::Linear`).  Here a layer object IS its line of the
// arch grammar (cpc/SequentialBuilder.cpp:92-626, the same constructor arguments in the same order): add()ed to an
// fl::Sequential it appends that line, and the Sequential plans ONE pipeline out of its lines on first use (params() /
// forward()), exactly as buildSequentialModule does for an arch file.  A layer object cannot run on its own: forward() on it
// throws -- per-layer execution with a free-form autograd is outside the hot path (see the header comment).
class FL_COMPAT_API ArchLayer : public Module {
 public:
  explicit ArchLayer(std::string line) : line_(std::move(line)) {}
  const std::string& archLine() const { return line_; }
  std::vector<Variable> forward(const std::vector<Variable>&) override {
    throw std::logic_error("fl_compat: a layer object runs as part of the fl::Sequential it was added to (one planned pipeline): " + line_);
  }
  std::string prettyString() const override { return line_; }

 protected:
  static std::string join(const char* tok, std::initializer_list<double> v) {
    std::string s(tok);
    for (double x : v) {
      char b[40];
      if (x == (double)(long long)x) snprintf(b, sizeof b, " %lld", (long long)x); else snprintf(b, sizeof b, " %.9g", x);
      s += b;
    }
    return s;
  }
  std::string line_;
};
class View : public ArchLayer { public: explicit View(const af::dim4& d) : ArchLayer(join("V", {(double)d[0], (double)d[1], (double)d[2], (double)d[3]})) {} };
class Reorder : public ArchLayer { public: Reorder(int d0, int d1, int d2 = 2, int d3 = 3) : ArchLayer(join("RO", {(double)d0, (double)d1, (double)d2, (double)d3})) {} };
class Dropout : public ArchLayer { public: explicit Dropout(double p = 0.5) : ArchLayer(join("DO", {p})) {} };
class ReLU : public ArchLayer { public: ReLU() : ArchLayer("R") {} };
class GatedLinearUnit : public ArchLayer { public: explicit GatedLinearUnit(int dim) : ArchLayer(join("GLU", {(double)dim})) {} };
class LayerNorm : public ArchLayer {
 public:
  explicit LayerNorm(const std::vector<int>& axes) : ArchLayer(lineOf(axes)) {}
  explicit LayerNorm(int axis) : ArchLayer(lineOf({axis})) {}   // fl::LayerNorm(int axis, ...)
 private:
  static std::string lineOf(const std::vector<int>& axes) { std::string s("LN"); for (int a : axes) s += " " + std::to_string(a); return s; }
};
class Linear : public ArchLayer {
 public:
  Linear(int in, int out, bool bias = true) : ArchLayer(join("L", {(double)in, (double)out})) {
    if (!bias) throw std::invalid_argument("fl_compat: fl::Linear without bias is not in the arch grammar");
  }
};
// fl::Conv2D(nIn, nOut, wx, wy, sx, sy, px, py, dx, dy, bias, groups): wx along time (ArrayFire dim 0); px / py = -1 is PaddingMode::SAME
class Conv2D : public ArchLayer {
 public:
  Conv2D(int nIn, int nOut, int wx, int wy, int sx = 1, int sy = 1, int px = 0, int py = 0, int dx = 1, int dy = 1, bool bias = true, int groups = 1)
      : ArchLayer(dx == 1 && dy == 1 ? join("C2", {(double)nIn, (double)nOut, (double)wx, (double)wy, (double)sx, (double)sy, (double)px, (double)py})
                                     : join("C2", {(double)nIn, (double)nOut, (double)wx, (double)wy, (double)sx, (double)sy, (double)px, (double)py, (double)dx, (double)dy})) {
    if (!bias || groups != 1) throw std::invalid_argument("fl_compat: fl::Conv2D without bias / with groups is not in the arch grammar");
  }
};
enum class PoolingMode { MAX = 0 };
class Pool2D : public ArchLayer {
 public:
  Pool2D(int wx, int wy, int sx = 1, int sy = 1, int px = 0, int py = 0, PoolingMode mode = PoolingMode::MAX)
      : ArchLayer(px == 0 && py == 0 ? join("M", {(double)wx, (double)wy, (double)sx, (double)sy}) : join("M", {(double)wx, (double)wy, (double)sx, (double)sy, (double)px, (double)py})) { (void)mode; }
};
// fl::Transformer(modelDim, headDim, mlpDim, nHeads, bptt, pDropout, pLayerdrop, useMask, preLN)
class Transformer : public ArchLayer {
 public:
  Transformer(int modelDim, int headDim, int mlpDim, int nHeads, int bptt, float pDropout, float pLayerdrop, bool useMask = false, bool preLN = false)
      : ArchLayer(join("TR", {(double)modelDim, (double)mlpDim, (double)nHeads, (double)bptt, (double)pDropout, (double)pLayerdrop})) {
    if (headDim * nHeads != modelDim || useMask || preLN)
      throw std::invalid_argument("fl_compat: fl::Transformer with headDim * nHeads != modelDim, a causal mask or pre-LN is not in the arch grammar");
  }
};
// fl::TDSBlock(channels, kernelSize, width, dropout, innerLinearDim)
class TDSBlock : public ArchLayer {
 public:
  TDSBlock(int c, int kw, int h, double dropout = 0, int innerLinearDim = 0)
      : ArchLayer(innerLinearDim ? join("TDS", {(double)c, (double)kw, (double)h, dropout, (double)innerLinearDim}) : join("TDS", {(double)c, (double)kw, (double)h, dropout})) {}
};
// fl::WeightNorm(module, dim)
class WeightNorm : public ArchLayer {
 public:
  WeightNorm(const std::shared_ptr<ArchLayer>& child, int dim) : ArchLayer("WN " + std::to_string(dim) + " " + child->archLine()) {}
  WeightNorm(const ArchLayer& child, int dim) : ArchLayer("WN " + std::to_string(dim) + " " + child.archLine()) {}
};

// user-composed chain: output of module i feeds module i + 1.  With layer objects (above) the chain is one planned pipeline:
// the lines of the layers added so far, planned on first use; layer objects and other modules do not mix in one Sequential.
class FL_COMPAT_API Sequential : public Container {
 public:
  void add(std::shared_ptr<Module> m) override;               // a layer object contributes its arch line
  template <class T, class = typename std::enable_if<std::is_base_of<Module, T>::value>::type>
  void add(const T& layer) { add(std::static_pointer_cast<Module>(std::make_shared<T>(layer))); }   // fl's add(const T&)
  std::vector<Variable> params() const override;
  void setParams(const Variable& var, int position) override;
  void train() override;
  void eval() override;
  std::vector<Variable> forward(const std::vector<Variable>& inputs) override;
  Variable forward(const Variable& in) { return forward(std::vector<Variable>{in}).front(); }
  std::string prettyString() const override;
  std::shared_ptr<Sequential> planned() const;                // the pipeline behind a Sequential of layer objects (null otherwise)
  void setInputFeatures(int nFeat) { inputFeatures_ = nFeat; } // fl_compat extension: NFEAT of the (T, NFEAT, 1, B) input when the first layer does not say it
  // fl_compat extension (slimIPL's dynamic dropout, recipes/slimIPL/src/Train.cpp:1465-1469; the recipe's plugin hands the number
  // to its Transformer layers only, 100h_supervised_slimipl.cpp:41-58): the probabilities the `TR` layers of the planned pipeline
  // use from the next forward on (w2l_trainer_set_dropout); a negative value restores the arch value; no new plan
  virtual void setTransformerDropout(double pDropout, double pLayerDrop);

 private:
  void materialize();
  std::string archText_;                                      // lines of the layer objects added so far
  std::shared_ptr<Sequential> planned_;
  int inputFeatures_ = 0;
};

// fl::Residual as the arch grammar builds it (cpc/SequentialBuilder.cpp:525-599; the class itself is un-vendored): layers in
// order, shortcuts between them, a scale where a shortcut lands.  Like every layer object it IS its arch lines -- here several:
//   RES <layers> <shortcuts> 1 / the layers' lines / SKIP <from> <to> [scale]   or   SKIPL <from> <to> <n> [scale] + n projection lines
// -- and runs as part of the fl::Sequential it is added to.  Layer indices count from 1; `from` = 0 is the block's input and
// `to` = layers + 1 its output.  What the pipeline builds is y = scale * (f(x) + p(x)), one shortcut from the input to the output
// (DESIGN 3.29): any other from / to, a second shortcut or a block without one is refused with std::invalid_argument when the
// Sequential plans (params() / forward()), as for an arch file, and so is an output of f that differs from the shortcut's in
// shape or layout.  add() takes layer objects only (no nested fl::Residual); a projection is one layer object or an
// fl::Sequential of them.
class Residual : public ArchLayer {
 public:
  Residual() : ArchLayer("") { compose(); }
  void add(std::shared_ptr<Module> m) {
    auto* l = dynamic_cast<ArchLayer*>(m.get());
    if (!l || dynamic_cast<Residual*>(l)) throw std::invalid_argument("fl_compat: fl::Residual::add takes layer objects (and no nested fl::Residual)");
    layers_.push_back(l->archLine());
    kept_.push_back(std::move(m));
    compose();
  }
  template <class T, class = typename std::enable_if<std::is_base_of<Module, T>::value>::type>
  void add(const T& layer) { add(std::static_pointer_cast<Module>(std::make_shared<T>(layer))); }
  void addShortcut(int fromLayer, int toLayer) { shortcuts_.push_back({fromLayer, toLayer, false, 0.f, {}}); compose(); }
  void addShortcut(int fromLayer, int toLayer, std::shared_ptr<Module> projection) {
    Shortcut s{fromLayer, toLayer, false, 0.f, {}};
    s.linear = true;
    if (auto* l = dynamic_cast<ArchLayer*>(projection.get())) {
      if (dynamic_cast<Residual*>(l)) throw std::invalid_argument("fl_compat: the projection of an fl::Residual shortcut cannot be an fl::Residual");
      s.projection.push_back(l->archLine());
    } else if (auto* c = dynamic_cast<Container*>(projection.get())) {
      for (auto& m : c->modules()) {
        auto* l2 = dynamic_cast<ArchLayer*>(m.get());
        if (!l2 || dynamic_cast<Residual*>(l2)) throw std::invalid_argument("fl_compat: the projection of an fl::Residual shortcut is made of layer objects");
        s.projection.push_back(l2->archLine());
      }
    } else {
      throw std::invalid_argument("fl_compat: the projection of an fl::Residual shortcut is a layer object or an fl::Sequential of them");
    }
    kept_.push_back(std::move(projection));
    shortcuts_.push_back(std::move(s));
    compose();
  }
  template <class T, class = typename std::enable_if<std::is_base_of<Module, T>::value>::type>
  void addShortcut(int fromLayer, int toLayer, const T& projection) { addShortcut(fromLayer, toLayer, std::static_pointer_cast<Module>(std::make_shared<T>(projection))); }
  // the sum that enters layer `beforeLayer` (layers + 1: the block's output) is multiplied by `scale`: the arch grammar writes it
  // on the shortcut line that lands there
  void addScale(int beforeLayer, float scale) {
    for (auto& s : shortcuts_)
      if (s.to == beforeLayer && !s.scaled) { s.scaled = true; s.scale = scale; compose(); return; }
    throw std::invalid_argument("fl_compat: fl::Residual::addScale(" + std::to_string(beforeLayer) + ", ...) needs a shortcut that lands there: add the shortcut first");
  }
  std::string prettyString() const override {
    std::string s = "Residual [";
    for (char ch : line_) { if (ch == '\n') s += " | "; else s += ch; }
    return s + "]";
  }

 private:
  struct Shortcut { int from, to; bool scaled; float scale; std::vector<std::string> projection; bool linear = false; };
  void compose() {
    line_ = "RES " + std::to_string(layers_.size()) + " " + std::to_string(shortcuts_.size()) + " 1";
    for (auto& l : layers_) line_ += "\n" + l;
    for (auto& s : shortcuts_) {
      std::string k = s.linear ? join("SKIPL", {(double)s.from, (double)s.to, (double)s.projection.size()}) : join("SKIP", {(double)s.from, (double)s.to});
      if (s.scaled) k += join("", {(double)s.scale});
      line_ += "\n" + k;
      for (auto& p : s.projection) line_ += "\n" + p;
    }
  }
  std::vector<std::string> layers_;
  std::vector<Shortcut> shortcuts_;
  std::vector<std::shared_ptr<Module>> kept_;
};

// fl::SpecAugment as the Trainer instantiates it from --saug_start_update (recipes/slimIPL/src/Train.cpp:1026-1048, applied
// at :1453-1461): frequency / time masking with zeros on the features (T, NFEAT, 1, B); identity in eval mode.  Same kernel as
// the SAUG arch token (w2l_specaugment_inplace; one mask set per batch).  Time warping (tWarpW) is not applied by the
// reference's own module either in this configuration (the first argument is the filterbank count).
class FL_COMPAT_API SpecAugment : public Module {
 public:
  SpecAugment(int tWarpW, int fMaskF, int nFMask, int tMaskT, float tMaskP, int nTMask);
  std::vector<Variable> forward(const std::vector<Variable>& inputs) override;
  std::string prettyString() const override;
  uint32_t calls() const { return calls_; }          // fl_compat extension: the mask stream position (checkpoints)
  void setCalls(uint32_t n) { calls_ = n; }

 private:
  int fMaskF_, nFMask_, tMaskT_, nTMask_;
  float tMaskP_;
  uint32_t calls_ = 0;
};

// ---- optimizers (recipes/slimIPL/src/Train.cpp:577-582: SGDOptimizer(params, lr, momentum, weightdecay))
class FL_COMPAT_API FirstOrderOptimizer {
 public:
  FirstOrderOptimizer(const std::vector<Variable>& params, double lr) : parameters_(params), lr_(lr) {}
  virtual ~FirstOrderOptimizer() {}
  virtual void step() = 0;
  double getLr() const { return lr_; }
  void setLr(double lr) { lr_ = lr; }
  virtual void zeroGrad() { for (auto& p : parameters_) p.zeroGrad(); }
  virtual std::string prettyString() const = 0;
  // fl_compat extension (checkpoints, fl::pkg::runtime::Serializer): "sgd" | "adagrad" | "adadelta" | "adam", and the per-parameter
  // state arrays -- slot 0: SGD velocity / Adagrad variance / Adadelta accGrad / Adam m, slot 1: Adadelta accDelta / Adam v
  // (empty: stateless); steps(): the updates applied so far where the rule reads them (Adam's bias correction), else 0
  virtual const char* kind() const = 0;
  virtual std::vector<std::vector<af::array>*> state() { return {}; }
  virtual uint64_t steps() const { return 0; }
  virtual void setSteps(uint64_t) {}
  const std::vector<Variable>& parameters() const { return parameters_; }

 protected:
  std::vector<Variable> parameters_;
  double lr_;
  // parameters that are exactly the slices of ONE planned network's flat parameter arena: the optimizer's state arrays are views of
  // flat buffers with the same offsets and step() is a single launch over (parameters, gradients, state) -- the reference walks
  // the parameters one by one (a few hundred launches per update); anything else falls back to that walk
  float* flatParams_ = nullptr;
  float* flatState_[2] = {nullptr, nullptr};
  size_t flatFloats_ = 0;
  std::vector<size_t> flatOffsets_;
  void flatStateViews(int slot, std::vector<af::array>& views);   // allocates flatState_[slot] (zeros) and fills `views`
  bool flatNow(float*& gradBase, const std::vector<af::array>* s0, const std::vector<af::array>* s1) const;
};

// every gradient of `params` multiplied by `s` IN PLACE (Train.cpp:1748-1760 writes `p.grad() = p.grad() / totalBatchSize`, one
// temporary per parameter); gradients that are the slices of one planned network's gradient arena are scaled as the arena
FL_COMPAT_API void scaleGradients(const std::vector<Variable>& params, double s);

class FL_COMPAT_API SGDOptimizer : public FirstOrderOptimizer {
 public:
  SGDOptimizer(const std::vector<Variable>& params, double lr, double momentum = 0, double weightDecay = 0, bool useNesterov = false);
  void step() override;
  std::string prettyString() const override;
  const char* kind() const override { return "sgd"; }
  std::vector<std::vector<af::array>*> state() override { return velocities_.empty() ? std::vector<std::vector<af::array>*>{} : std::vector<std::vector<af::array>*>{&velocities_}; }

 private:
  double mu_, wd_;
  bool nesterov_;
  std::vector<af::array> velocities_;
};

// --netoptim=adagrad (recipes/sota/2019/librivox/train_am_transformer_ctc.cfg:25-26): variance += g^2, p -= lr g / (sqrt(variance) + eps)
class FL_COMPAT_API AdagradOptimizer : public FirstOrderOptimizer {
 public:
  AdagradOptimizer(const std::vector<Variable>& params, double lr, double eps = 1e-8, double weightDecay = 0);
  void step() override;
  std::string prettyString() const override;
  const char* kind() const override { return "adagrad"; }
  std::vector<std::vector<af::array>*> state() override { return {&variance_}; }

 private:
  double eps_;
  std::vector<af::array> variance_;
};

// --netoptim=adadelta (recipes/sota/2019/librispeech/train_am_transformer_ctc.cfg:23-26)
class FL_COMPAT_API AdadeltaOptimizer : public FirstOrderOptimizer {
 public:
  AdadeltaOptimizer(const std::vector<Variable>& params, double lr = 1.0, double rho = 0.9, double eps = 1e-8, double weightDecay = 0);
  void step() override;
  std::string prettyString() const override;
  const char* kind() const override { return "adadelta"; }
  std::vector<std::vector<af::array>*> state() override { return {&accGrad_, &accDelta_}; }

 private:
  double rho_, eps_;
  std::vector<af::array> accGrad_, accDelta_;
};

// --netoptim=adam (recipes/joint_training_vox_populi/sh_voxpopuli/pretrain.sh; cpc/Train.cpp:569-580 passes --adambeta1 --adambeta2
// --optimepsilon and, for the network only, --weightdecay).  [UNVENDORED] Flashlight class, restated as w2l_adam_step_guarded states
// it: t = steps() + 1; clr = lr sqrt(1 - beta2^t) / (1 - beta1^t); p -= weightDecay lr p (decoupled: the moments never see it);
// m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2; p -= clr m / (sqrt(v) + eps), eps outside the bias correction.
// The count lives on the host: the caller decides whether to call step() at all.
class FL_COMPAT_API AdamOptimizer : public FirstOrderOptimizer {
 public:
  AdamOptimizer(const std::vector<Variable>& params, double lr, double beta1 = 0.9, double beta2 = 0.999, double eps = 1e-8, double weightDecay = 0);
  void step() override;
  std::string prettyString() const override;
  const char* kind() const override { return "adam"; }
  std::vector<std::vector<af::array>*> state() override { return {&biasedFirst_, &biasedSecond_}; }
  uint64_t steps() const override { return count_; }
  void setSteps(uint64_t n) override { count_ = n; }
  double beta1() const { return beta1_; }
  double beta2() const { return beta2_; }
  double epsilon() const { return eps_; }
  double weightDecay() const { return wd_; }

 private:
  double beta1_, beta2_, eps_, wd_;
  uint64_t count_ = 0;
  std::vector<af::array> biasedFirst_, biasedSecond_;
};

// global-norm clipping over the gradients that are available; returns the norm before clipping
FL_COMPAT_API double clipGradNorm(const std::vector<Variable>& params, double maxNorm);

// ---- data parallelism (recipes/slimIPL/src/Train.cpp:188-199, :1078-1079, :1721-1747): one process per GPU, RCCL over xGMI.
// librccl.so is dlopen()ed by initDistributed only: a single-GPU run never touches it.
FL_COMPAT_API int getWorldRank();
FL_COMPAT_API int getWorldSize();
FL_COMPAT_API void allReduce(af::array& arr, double scale = 1.0);           // in place, sum over ranks (then * scale)
FL_COMPAT_API void allReduce(Variable& var, double scale = 1.0);
FL_COMPAT_API void allReduceParameters(const std::shared_ptr<const Module>& module);   // average: replicas start identical
FL_COMPAT_API void barrier();

class FL_COMPAT_API Reducer {
 public:
  virtual ~Reducer() {}
  virtual void add(Variable& var) = 0;
  virtual void finalize() = 0;
};
// fl::CoalescingReducer(scale, async, contiguous): gradients are added as backward produces them and reduced in
// buckets; here the parameters of a planned network already sit in ONE flat arena, so adjacent gradients coalesce into
// a single ncclAllReduce over the whole arena (the reference issues dozens of ~20 MB buckets)
class FL_COMPAT_API CoalescingReducer : public Reducer {
 public:
  CoalescingReducer(double scale, bool async, bool contiguous);
  ~CoalescingReducer() override;
  void add(Variable& var) override;
  void finalize() override;
  size_t lastCollectives() const { return lastCollectives_; }   // fl_compat extension: ncclAllReduce calls of the last finalize()
  size_t lastOverlapped() const { return lastOverlapped_; }     // ... of which were issued on the side stream behind a bucket event

 private:
  double scale_;
  bool async_, contiguous_;
  struct Span { float* ptr; size_t n; };
  std::vector<Span> spans_;
  size_t lastCollectives_ = 0, lastOverlapped_ = 0;
};

// ---- fl::ext: fl_compat EXTENSIONS for slimIPL.  The reference has NO such free functions: its Trainer writes the averaged
// network as one ArrayFire expression per parameter (recipes/slimIPL/src/Train.cpp:1823-1832) and selects the labelled utterances
// with an indexing expression on the Variable (:1637-1639).
namespace ext {
// ema <- decay * ema + (1 - decay) * net, fp32.  Two planned networks of the same arch: ONE w2l_ema_update over the parameter
// arenas; anything else: one call per parameter.  Whatever the averaged network derives from its parameters (weight-norm
// products, bf16 weight images) is rebuilt by its next forward.  decay outside [0, 1] / NaN: std::invalid_argument.
FL_COMPAT_API void emaUpdate(const std::shared_ptr<fl::Module>& ema, const std::shared_ptr<fl::Module>& net, double decay);
// the (N, T, |rows|) emissions of the listed utterances of an (N, T, B) batch; backward writes their gradients into a zero-filled
// gradient of the full batch.  All rows in order: the argument itself.
FL_COMPAT_API Variable selectBatch(const Variable& emission, const std::vector<int>& rows);
}  // namespace ext

namespace pkg {
namespace runtime {
// fl::pkg::runtime::initDistributed(worldRank, worldSize, maxDevicesPerNode, rndvFilepath) (Train.cpp:189-194): binds
// this process to GPU worldRank % maxDevicesPerNode and creates the RCCL communicator; the ncclUniqueId travels through
// the file <rndvFilepath>/w2l_nccl_id.<worldSize> written by rank 0 (the reference's file-system rendezvous)
FL_COMPAT_API void initDistributed(int worldRank, int worldSize, int maxDevicesPerNode, const std::string& rndvFilepath);
// fl::pkg::runtime::Serializer::save(filename, version, config, network, criterion, netoptim, critoptim) / load(...)
// (recipes/slimIPL/src/Train.cpp:132-173 header-only load of `continue` / `fork`, :452-463 model loads, :767-790 saves).
// The reference's container is cereal (needs Flashlight to read); this one is the documented W2LAMD01 layout of
// wav2letter_amd/checkpoint.py -- network tensors in the REFERENCE's parameter order and array layouts, the ASG
// transitions, the optimizer state as flat arenas, `config` in the JSON header -- written and read by both languages.
struct FL_COMPAT_API Serializer {
  using Config = std::unordered_map<std::string, std::string>;
  static void save(const std::string& path, const std::string& version, const Config& config, const std::shared_ptr<fl::Module>& network,
                   const std::shared_ptr<fl::Module>& criterion, const std::shared_ptr<fl::FirstOrderOptimizer>& netoptim,
                   const std::shared_ptr<fl::FirstOrderOptimizer>& critoptim);
  static void load(const std::string& path, std::string& version, Config& config);
  static void load(const std::string& path, std::string& version, Config& config, const std::shared_ptr<fl::Module>& network,
                   const std::shared_ptr<fl::Module>& criterion);
  static void load(const std::string& path, std::string& version, Config& config, const std::shared_ptr<fl::Module>& network,
                   const std::shared_ptr<fl::Module>& criterion, const std::shared_ptr<fl::FirstOrderOptimizer>& netoptim,
                   const std::shared_ptr<fl::FirstOrderOptimizer>& critoptim);
};
// dlopen(path, RTLD_LAZY) + dlsym("createModule"): extern "C" fl::Module* createModule(int64_t nFeature, int64_t nLabel)
// returns an OWNING raw pointer (recipes/slimIPL/100h_supervised.cpp:84-87; loader call Train.cpp:390-395).
// A name that ends in ".arch" is not a plugin: arch() then goes through buildSequentialModule, which is what the
// reference's `--arch` flag does when it names an arch file.
class FL_COMPAT_API ModulePlugin {
 public:
  explicit ModulePlugin(const std::string& name);
  ~ModulePlugin();
  std::shared_ptr<fl::Module> arch(int64_t nFeatures, int64_t nClasses);

 private:
  std::string name_;
  void* handle_ = nullptr;
  fl::Module* (*create_)(int64_t, int64_t) = nullptr;
};
}  // namespace runtime

namespace speech {
enum class CriterionScaleMode { NONE = 0, INPUT_SZ = 1, INPUT_SZ_SQRT = 2, TARGET_SZ = 3, TARGET_SZ_SQRT = 4 };
FL_COMPAT_API CriterionScaleMode getCriterionScaleMode(const std::string& onorm, bool sqnorm);

// arch file -> network.  forward({features (T, NFEAT, 1, B) f32 [, inputSizes (1, B)]}) -> {emissions (NLABEL, T', B)}
// (inputSizes may carry one more entry, (1, B + 1): the size the T frames correspond to when the batch is padded beyond its
// longest utterance -- the denominator of the Transformer padding mask; the reference pads to the longest only)
FL_COMPAT_API std::shared_ptr<fl::Sequential> buildSequentialModule(const std::string& archfile, int64_t nFeatures, int64_t nClasses);
FL_COMPAT_API std::shared_ptr<fl::Sequential> buildSequentialModuleFromText(const std::string& archText, int64_t nFeatures, int64_t nClasses);

// fl_compat extension: the chunked streaming forward (w2l_stream_*, include/w2l_hip.h) over a network a plugin or an arch file
// produced.  `slots` concurrent streams, at most `maxChunk` input frames per slot and step; for any utterance and any split of it
// into chunks the concatenated emissions equal the network's eval-mode forward of that utterance alone (fp32 parity).  The
// session reads the network's parameter arena at every step and keeps the network alive.  A network with a line that cannot be
// streamed (TR, M, GLU, LN over time, TDS with lnIncludeTime = 1, SAME padding at a stride above 1) or in mixed-precision mode
// throws std::invalid_argument naming the line.
// mixedPrecision = true: a bf16 session (W2L_STREAM_BF16) over a network whose mixed-precision mode is on (setMixedPrecision;
// std::invalid_argument otherwise, and for the second level, setMixedPrecisionConvolutions): bf16 operands for the fl::Linear
// products and the TDS convolutions, equal to the network's own mixed-precision eval forward within 2e-3.  Such a session holds a
// SNAPSHOT of the model -- it copies the parameters and writes the bf16 weight images at its first step -- and shows later changes
// of the parameters only after refreshWeights(), unlike the fp32 session, which reads the live arena at every step.
class FL_COMPAT_API StreamingSession {
 public:
  StreamingSession(std::shared_ptr<fl::Sequential> network, int slots, int maxChunk, bool mixedPrecision = false);
  ~StreamingSession();
  StreamingSession(const StreamingSession&) = delete;
  StreamingSession& operator=(const StreamingSession&) = delete;
  int slots() const { return slots_; }
  int maxChunk() const { return maxChunk_; }
  int maxOut() const { return maxOut_; }       // emission frames one step can return per slot
  int numLabels() const { return nLabel_; }
  // features (maxChunk, NFEAT, 1, slots) f32: the first counts[s] frames of slot s are used.  start[s]: the slot begins a new
  // utterance; finish[s]: these frames are its last, the network flushes (either vector may be empty = all 0).  Returns the
  // emissions (NLABEL, maxOut, slots) -- a view of the session's state, valid until the next step -- and fills nOut[s], the new
  // frames of slot s (host arithmetic: the step enqueues on fl::currentStream() and does not synchronise).
  af::array step(const af::array& features, const std::vector<int>& counts, const std::vector<int>& start, const std::vector<int>& finish,
                 std::vector<int>& nOut);
  void reset(int slot);                        // closes a slot and discards its state
  bool mixedPrecision() const { return mixed_; }
  void refreshWeights();                       // bf16: the next step takes the parameters again (host only; a no-op for fp32)

 private:
  std::shared_ptr<fl::Sequential> net_;
  std::shared_ptr<void> state_;
  void* h_ = nullptr;
  int slots_ = 0, maxChunk_ = 0, maxOut_ = 0, nFeat_ = 0, nLabel_ = 0;
  bool mixed_ = false;
};

// fl_compat extension: the streaming log-mel front end (w2l_feat_session_*; the contract is in w2l_hip.h), the first module of the
// chain StreamingFeatures -> StreamingSession -> StreamingDecoder.  Built from an fl::lib::audio::Mfsc (fl_compat/audio.h), whose
// tables and geometry it binds and which it keeps a copy of; `slots` concurrent streams, at most maxSamples new samples per slot
// and step.  For any split of an utterance into chunks the concatenated frames are the same bit for bit, and they equal
// Mfsc::apply of the whole utterance up to summation order.  No normalisation.  A geometry beyond the kernel's bounds
// (frameSize 512, 257 bins, 128 filters) throws std::runtime_error naming the field; any other refused argument
// std::invalid_argument.
class FL_COMPAT_API StreamingFeatures {
 public:
  StreamingFeatures(const fl::lib::audio::Mfsc& mfsc, int slots, int maxSamples);
  ~StreamingFeatures();
  StreamingFeatures(const StreamingFeatures&) = delete;
  StreamingFeatures& operator=(const StreamingFeatures&) = delete;
  int slots() const { return slots_; }
  int maxSamples() const { return maxSamples_; }
  int maxOut() const { return maxOut_; }         // frames one step can return per slot: a StreamingSession's maxChunk
  int numFeatures() const { return nFeat_; }
  // pcm (maxSamples, slots) f32: the first counts[s] samples of slot s are used.  start[s]: the slot begins a new utterance;
  // finish[s]: these samples are its last, what does not fill a frame is dropped (either vector may be empty = all 0).  Returns
  // the features (maxOut, NFEAT, 1, slots) -- a view of the session's state, valid until the next step, which
  // StreamingSession::step takes as it is -- and fills nOut[s], the new frames of slot s (host arithmetic: the step enqueues on
  // fl::currentStream() and does not synchronise).  stepInt16: the same over device int16 samples [slots][maxSamples], scaled by
  // exactly 1 / 32768.
  af::array step(const af::array& pcm, const std::vector<int>& counts, const std::vector<int>& start, const std::vector<int>& finish,
                 std::vector<int>& nOut);
  af::array stepInt16(const int16_t* pcmDevice, const std::vector<int>& counts, const std::vector<int>& start, const std::vector<int>& finish,
                      std::vector<int>& nOut);
  void slotState(int slot, bool& active, int& carrySamples) const;
  void reset(int slot);                          // closes a slot and discards its carry

 private:
  af::array run(const void* pcm, int pcmType, const std::vector<int>& counts, const std::vector<int>& start, const std::vector<int>& finish,
                std::vector<int>& nOut);
  af::array G_, H_;
  std::shared_ptr<void> state_;
  void* h_ = nullptr;
  int slots_ = 0, maxSamples_ = 0, maxOut_ = 0, nFeat_ = 0;
};

// fl_compat extension: LocalNorm, the windowed feature normalisation of the streaming recipe (w2l_local_norm, w2l_norm_session_*;
// the contract is in w2l_hip.h).  localNormalize: features (T, NFEAT, 1, B) f32 -> the same shape; frame t of utterance b, which
// has frames[b] frames (an empty vector: T each), is normalised with one mean and deviation over all features of frames
// max(0, t - left) .. min(frames[b] - 1, t + right); frames at or beyond frames[b] come out zero.  Two launches on
// fl::currentStream(), one small copy of `frames`; a refused argument throws std::invalid_argument, a window above 65536 frames
// or NFEAT above 4096 std::runtime_error.
FL_COMPAT_API af::array localNormalize(const af::array& features, const std::vector<int>& frames, int left, int right);

// StreamingLocalNorm is the reference's streaming::LocalNorm(nFeat, left, 0) between StreamingFeatures and StreamingSession:
// `slots` concurrent streams, at most maxChunk new frames per slot and step, and for any split of an utterance's frames into
// chunks the concatenated output is localNormalize(., left, 0) of the whole utterance, bit for bit.  right != 0 throws
// std::invalid_argument, as the reference's module does.
class FL_COMPAT_API StreamingLocalNorm {
 public:
  StreamingLocalNorm(int nFeat, int slots, int maxChunk, int left, int right = 0);
  ~StreamingLocalNorm();
  StreamingLocalNorm(const StreamingLocalNorm&) = delete;
  StreamingLocalNorm& operator=(const StreamingLocalNorm&) = delete;
  int slots() const { return slots_; }
  int maxChunk() const { return maxChunk_; }
  int numFeatures() const { return nFeat_; }
  // features (ld, NFEAT, 1, slots) f32, IN PLACE (StreamingFeatures::step's view as it is): the first counts[s] frames of slot s
  // are normalised, start[s] begins a new utterance (an empty vector = all 0).  One launch on fl::currentStream(), no
  // synchronisation.
  void step(af::array& features, const std::vector<int>& counts, const std::vector<int>& start);
  void slotState(int slot, bool& active, long long& frames) const;
  void reset(int slot);                          // closes a slot

 private:
  std::shared_ptr<void> state_;
  void* h_ = nullptr;
  int slots_ = 0, maxChunk_ = 0, nFeat_ = 0;
};

class FL_COMPAT_API SequenceCriterion : public fl::Container {
 public:
  // inputs {emission (N, T, B) f32, target (L, B) s32 (padded with negative values)} -> {loss (B)}
  std::vector<Variable> forward(const std::vector<Variable>& inputs) override = 0;
  virtual af::array viterbiPath(const af::array& input, const af::array& inputSize = af::array()) = 0;              // (T, B) s32
  virtual af::array viterbiPathWithTarget(const af::array& input, const af::array& target,
                                          const af::array& inputSizes = af::array(), const af::array& targetSizes = af::array()) = 0;
  std::string prettyString() const override = 0;
};

// fl_compat extension: the flat gradient arena behind a network built from an arch file (one data-parallel
// all-reduce / one fused optimizer launch instead of one per parameter); {nullptr, 0} for any other module
struct FlatView { float* ptr; size_t floats; };
FL_COMPAT_API FlatView flatParameters(const std::shared_ptr<fl::Module>& network);
FL_COMPAT_API FlatView flatGradients(const std::shared_ptr<fl::Module>& network);
// --fl_amp_use_mixed_precision, restated for bf16: in a network built from an arch file every fl::Linear product, the TDS and
// sub-sampling convolutions and the attention products (scores, position term, P V and their gradients) multiply bf16 operand
// images with fp32 accumulation; activations, master weights, LayerNorm, the optimizer and the criterion stay fp32 (no-op for
// any other module)
FL_COMPAT_API void setMixedPrecision(const std::shared_ptr<fl::Module>& network, bool on);
// fl_compat extension (--w2l_amp_convs): the second level of that mode -- the wide time convolutions at H == 1 (the `C` lines of
// the conv_glu recipes, the Transformer recipes' front end) multiply bf16 images too (w2l_conv_bf16_*).  Acts only while
// setMixedPrecision is on; the next forward plans again (weight images and image scratch belong to the plan).  No-op for any
// other module.
FL_COMPAT_API void setMixedPrecisionConvolutions(const std::shared_ptr<fl::Module>& network, bool on);
// fl_compat extension: the weight-gradient stream of a network built from an arch file (on by default).  loss.backward() enqueues
// the fp32 weight, bias and filter gradients on a side stream the network owns and joins it into the compute stream before it
// returns; a gradient bucket's event fires once both streams have finished the bucket.  Same results either way
// (w2l_trainer_set_weight_grad_stream in w2l_hip.h says what stays on one stream).  No-op for any other module.
FL_COMPAT_API void setWeightGradStream(const std::shared_ptr<fl::Module>& network, bool on);
// fl_compat extension: forwards so far of a network built from an arch file = the position of its dropout-seed stream
// (restored by Serializer::load; `Train fork` starts it from zero)
FL_COMPAT_API uint32_t networkStep(const std::shared_ptr<fl::Module>& network);
FL_COMPAT_API void setNetworkStep(const std::shared_ptr<fl::Module>& network, uint32_t step);

class NGramLM;   // fl_compat/lm.h
class Lexicon;   // fl_compat/lexicon.h

// The options and the result of CTCLoss::beamSearch and ASGLoss::beamSearch (fl_compat ADDITIONS to the reference's interface).
// "token classes" below are N-1 for CTC (blank = N-1 is none) and all N for ASG.
struct BeamSearchOptions {
  int beamSize = 64;                  // W, 1..64; 1..1024 with wide; 1..8192 with xl or manyTokens
  int beamSizeToken = 64;             // K, clipped to the token classes (CTC: N-1, ASG: N), then <= 64; <= 256 with manyTokens
  float beamThreshold = 1.0f / 0.0f;  // candidates below best - threshold are dropped; +inf: none
  bool logAdd = false;                // false: max over a prefix's alignments (the 1-best is the greedy transcript); true: their sum
  int normalize = -1;                 // 1: search on log-softmax rows, 0: on the raw emissions, -1: CTC as logAdd, ASG 0
  int nbest = 1;                      // M, 1..W
  int maxLen = 0;                     // Lmax, 0 = T (no hypothesis is longer)
  // the search fused with a token-level n-gram LM (w2l_ctc_beam_search_lm); the defaults mean "no LM", and without lm the
  // other three must keep them.  lm: a table over the N-1 token classes (fl_compat/lm.h), alive during the call.
  const NGramLM* lm = nullptr;
  float lmWeight = 0.f;               // every extension by token c adds lmWeight * log p_LM(c | prefix) + classScore[c]
  af::array classScore;               // (N-1) f32 on the device, or empty
  float eosScore = 0.f;               // the end adds lmWeight * log p_LM(EOS | hypothesis) + eosScore; 0 for a model without EOS
  // the search restricted to the spellings of a lexicon (w2l_ctc_beam_search_lex); lm is required then and is a table over the
  // lexicon's WORDS (NGramLM::fromArpa(path, lexicon.words())), classScore must be empty.  lexicon: fl_compat/lexicon.h, alive
  // during the call.  Without lexicon the other two must keep their defaults.
  const Lexicon* lexicon = nullptr;
  float wordScore = 0.f;              // every completed word adds lmWeight * log p_LM(word | words before) + wordScore
  int maxWords = 0;                   // rows of `words`, 0 = Lmax
  bool wide = false;                  // every search above on the wide kernels (the w2l_*_wide entry points): the same contract, the same bytes at W <= 64
  bool xl = false;                    // every search above on the xl kernels (the w2l_*_xl entry points): the same contract, the wide kernels' bytes at W <= 1024; with wide: std::invalid_argument
  // the silence score (the w2l_*_sil entry points; the reference's --silscore): after the frame tokens have been chosen by the
  // acoustic lp alone, class silToken's frame score is lp + silScore wherever the search reads it.  silToken -1 with a lexicon: the
  // lexicon's silence token.  silScore != 0 without any silence token: std::invalid_argument.  silScore == 0: the search without it,
  // the same bytes.  Of the streaming decoders below ManyTokenStreamingDecoder takes the pair; StreamingDecoder and
  // WideStreamingDecoder have no silence score: a non-zero silScore there is std::invalid_argument.
  int silToken = -1;
  float silScore = 0.f;
  // with lexicon: lm is a model over the lexicon's TOKENS, not its words (the w2l_*_beam_search_lextok entry points; the reference's
  // --uselexicon=true --decodertype=tkn): every token that moves along a trie edge adds lmWeight * log p_LM(token | tokens before),
  // a completed word adds wordScore alone.  Without lexicon, or with xl: std::invalid_argument; the streaming decoders refuse it too.
  bool lmToken = false;
  // every whole-utterance search above on the many-token kernels (the w2l_*_mt entry points): the same contract with W up to 8192 and
  // K, after clipping, up to 256 -- the --beamsizetoken of the reference's word-piece recipes; the xl kernels' bytes at K <= 64.
  // With wide, xl or lmToken: std::invalid_argument.  StreamingDecoder and WideStreamingDecoder refuse it; the incremental form of
  // these searches is ManyTokenStreamingDecoder.
  bool manyTokens = false;
};
struct BeamSearchResult {
  af::array labels;    // (Lmax, M, B) s32: the first min(length, Lmax) labels, -1 beyond
  af::array lengths;   // (M, B) s32: the true label count; -1 for a rank that does not exist
  af::array scores;    // (M, B) f32; -inf for a rank that does not exist
  af::array lmScores;  // (M, B) f32 with an LM: the hypotheses' unweighted LM scores (-inf for a rank that does not exist); else empty
  af::array words;       // (maxWords, M, B) s32 with a lexicon: the first min(count, maxWords) word ids, -1 beyond; else empty
  af::array wordCounts;  // (M, B) s32 with a lexicon: the true word count; -1 for a rank that does not exist; else empty
};
// fl_compat extension: the CTC beam search of CTCLoss::beamSearch continued chunk by chunk (w2l_beam_session_*; the contract is
// in w2l_hip.h), beside StreamingSession, whose step() output it takes as it is when maxChunk == session.maxOut().  `slots`
// utterances in progress, at most maxChunk emission frames per slot and step, at most maxFrames per utterance.  The result after
// any number of frames is, bit for bit, CTCLoss::beamSearch over those frames alone, with the same options.  options: beamSize,
// beamSizeToken, beamThreshold, logAdd, normalize (-1: as logAdd), lm, lmWeight, classScore, eosScore, lexicon, wordScore; nbest,
// maxLen (0 = maxFrames) and maxWords (0 = maxLen) apply to result().  lm, lexicon and classScore must outlive the decoder.
// options.wide, a beam or token count above 64: std::runtime_error (WideStreamingDecoder below takes those); any other refused
// argument: std::invalid_argument.
class FL_COMPAT_API StreamingDecoder {
 public:
  StreamingDecoder(int slots, int maxChunk, int maxFrames, int numLabels, const BeamSearchOptions& options);
  ~StreamingDecoder();
  StreamingDecoder(const StreamingDecoder&) = delete;
  StreamingDecoder& operator=(const StreamingDecoder&) = delete;
  // emissions (NLABEL, maxChunk, slots) f32: the first counts[s] frames of slot s are its new ones.  start[s]: the slot begins a
  // new utterance before them (empty = all 0).  Enqueues on fl::currentStream() and does not synchronise.
  void step(const af::array& emissions, const std::vector<int>& counts, const std::vector<int>& start);
  // the hypotheses of every slot for the frames fed so far: BeamSearchResult with B = slots; changes nothing
  BeamSearchResult result();
  int frames(int slot) const;   // emission frames fed to a slot since its start
  void reset(int slot);         // closes a slot
  // What can no longer change, handed out, and the prefix tables compacted (w2l_beam_session_commit; the contract is in w2l_hip.h;
  // the reference's Decoder::prune(lookBack) commits to the best hypothesis instead, which is lossy).  commit[s] != 0: slot s
  // (empty = every started slot).  labels[s] / words[s]: what THIS call committed for slot s, in order (words with a lexicon);
  // live[s]: the nodes of its table afterwards (a slot may then take maxFrames - ceil(live / beamSize) further frames before its
  // next commit).  result() returns the tails behind committed(slot).  Enqueues on fl::currentStream() and WAITS for it.
  struct Committed { std::vector<std::vector<int>> labels, words; std::vector<int> live; };
  Committed commit(const std::vector<int>& commit = {});
  // every label and word slot has committed since its start
  const std::vector<int>& committedLabels(int slot) const;
  const std::vector<int>& committedWords(int slot) const;
  std::pair<std::vector<int>, std::vector<int>> committed(int slot) const { return {committedLabels(slot), committedWords(slot)}; }

 protected:
  struct WideKernels {};   // WideStreamingDecoder's constructor
  StreamingDecoder(int slots, int maxChunk, int maxFrames, int numLabels, const BeamSearchOptions& options, WideKernels);
  struct ManyTokenKernels {};   // ManyTokenStreamingDecoder's constructor
  StreamingDecoder(int slots, int maxChunk, int maxFrames, int numLabels, const BeamSearchOptions& options, ManyTokenKernels);

 private:
  void create(bool wideKernels, bool manyTokenKernels = false);
  BeamSearchOptions o_;
  std::shared_ptr<void> state_;
  void* h_ = nullptr;
  int slots_ = 0, maxChunk_ = 0, maxFrames_ = 0, nLabel_ = 0;
  std::shared_ptr<void> scratch_;                       // commit's, allocated at the first commit
  size_t scratchBytes_ = 0;
  std::vector<std::vector<int>> doneLabels_, doneWords_;   // per slot, since its start
};

// fl_compat extension: StreamingDecoder on the wide kernels (w2l_beam_session_create_wide): the result after any number of frames
// is, bit for bit, CTCLoss::beamSearch with options.wide = true over those frames alone.  beamSize goes up to 1024, beamSizeToken
// (after clipping to NLABEL - 1) up to 64; beyond: std::runtime_error.  options.wide is IGNORED: this class is always wide.  The
// methods are StreamingDecoder's.  A slot's state grows with beamSize * maxFrames: 64 MiB at 1024 and 4096.
class FL_COMPAT_API WideStreamingDecoder : public StreamingDecoder {
 public:
  WideStreamingDecoder(int slots, int maxChunk, int maxFrames, int numLabels, const BeamSearchOptions& options)
      : StreamingDecoder(slots, maxChunk, maxFrames, numLabels, options, WideKernels{}) {}
};

// fl_compat extension: StreamingDecoder on the many-token kernels (w2l_beam_session_create_mt): the result after any number of
// frames is, bit for bit, CTCLoss::beamSearch with options.manyTokens = true over those frames alone, options.silToken / silScore
// included (silToken -1 with a lexicon: the lexicon's silence token).  beamSize goes up to 8192, beamSizeToken (after clipping to
// NLABEL - 1) up to 256 -- the streaming recipes' 500 / 100; beyond: std::runtime_error.  options.manyTokens is IGNORED: this class
// is always many-token.  options.lmToken, wide or xl: std::invalid_argument.  The methods are StreamingDecoder's; commit() needs
// beamSize <= 1024 (beyond: std::runtime_error, nothing changed).
class FL_COMPAT_API ManyTokenStreamingDecoder : public StreamingDecoder {
 public:
  ManyTokenStreamingDecoder(int slots, int maxChunk, int maxFrames, int numLabels, const BeamSearchOptions& options)
      : StreamingDecoder(slots, maxChunk, maxFrames, numLabels, options, ManyTokenKernels{}) {}
};

class FL_COMPAT_API ASGLoss : public SequenceCriterion {
 public:
  ASGLoss(int N, CriterionScaleMode scalemode = CriterionScaleMode::NONE, double transdiag = 0.0);
  std::vector<Variable> forward(const std::vector<Variable>& inputs) override;
  af::array viterbiPath(const af::array& input, const af::array& inputSize = af::array()) override;
  af::array viterbiPathWithTarget(const af::array& input, const af::array& target, const af::array& inputSizes = af::array(),
                                  const af::array& targetSizes = af::array()) override;
  // fl_compat ADDITION: n-best beam search of the ASG lattice under this criterion's own transitions, param(0)
  // (w2l_asg_beam_search, w2l_asg_beam_search_lex; the contract is in w2l_hip.h): no blank, all N classes are tokens -- an LM, a
  // lexicon and classScore are over N classes --, a token never follows itself (replabels spell a repeated letter:
  // Lexicon::fromFile(..., replabel)).  Options, result, inputSizes and exceptions as CTCLoss::beamSearch; normalize -1 means 0.
  BeamSearchResult beamSearch(const af::array& input, const af::array& inputSizes, const BeamSearchOptions& options);
  std::string prettyString() const override;
  Variable transitions() const { return params_[0]; }   // (N, N), [to][from]
  CriterionScaleMode scaleMode() const { return scaleMode_; }

 private:
  int N_;
  CriterionScaleMode scaleMode_;
};

class FL_COMPAT_API CTCLoss : public SequenceCriterion {
 public:
  explicit CTCLoss(CriterionScaleMode scalemode = CriterionScaleMode::NONE);
  std::vector<Variable> forward(const std::vector<Variable>& inputs) override;
  af::array viterbiPath(const af::array& input, const af::array& inputSize = af::array()) override;   // per-frame argmax
  // forced alignment of the known target (w2l_ctc_align): (T, B) s32, one label per frame, blank = N-1, bit-exact with the fp32
  // max-plus recursion on the raw emissions (stay beats advance beats skip on ties); a target that does not fit: a column of -1.
  // inputSizes: empty = all T frames, else (1, B) or (B) s32 EMISSION-frame counts per utterance (frames beyond them hold blank);
  // targetSizes is ignored (sizes are counted on the device).  Bad target type / batch: std::invalid_argument.
  af::array viterbiPathWithTarget(const af::array& input, const af::array& target, const af::array& inputSizes = af::array(),
                                  const af::array& targetSizes = af::array()) override;
  // fl_compat ADDITION to the reference's interface (its lexicon-free decoder is a host class of its own): n-best prefix beam
  // search over the emissions without lexicon or LM (w2l_ctc_beam_search; the contract is in w2l_hip.h).  inputSizes as in
  // viterbiPathWithTarget.  The hypotheses are already collapsed label rows: turn them into letters / words with tknLabels2Ltr /
  // tknLabels2Wrd (fl_compat/text.h), not with tknPrediction2Ltr.  Refused arguments: std::invalid_argument; a beam or token
  // count beyond the kernel's 64 (with options.wide a beam beyond 1024, with options.xl beyond 8192): std::runtime_error.
  using BeamSearchOptions = ::fl::pkg::speech::BeamSearchOptions;   // hoisted: ASGLoss::beamSearch takes the same
  using BeamSearchResult = ::fl::pkg::speech::BeamSearchResult;
  BeamSearchResult beamSearch(const af::array& input, const af::array& inputSizes, const BeamSearchOptions& options);
  std::string prettyString() const override;
  CriterionScaleMode scaleMode() const { return scaleMode_; }

 private:
  CriterionScaleMode scaleMode_;
};

// The criterion of the reference's self-supervised trainer (--criterion=cpc; recipes/joint_training_vox_populi/cpc/CPCCriterion.h,
// CPCCriterion.cpp:38-235) over w2l_cpc_* (the contract is in w2l_hip.h): getMask replaces spans of the encoder output by a learned
// embedding before the context network sees it; forward scores every masked frame's context against its own encoder output and K
// negatives, other masked frames of the same utterance.  The fork's step (cpc/Train.cpp:1155-1205) reads
//     enc = encoder(features);  masked = crit->getMask(enc, maskProb, maskLength);  ctx = context(masked);
//     loss = crit->forward({enc, ctx}).front();  loss.backward();
// params() in the reference's order: the mask embedding (nEncoder), uniform in (-1, 1); the encoder projection's weight and bias;
// the context projection's weight and bias (uniform within 1 / sqrt(fan-in), fl::Linear's rule).  A weight is (in, nMutual) here --
// the C array [nMutual][in] of the kernels' contract --, the transpose of fl::Linear's (out, in).  nOffset, nUnits, nPieces and
// nBuffer are stored and unused, exactly as in the reference.  The draws (initial values, masked spans, negatives) come from this
// project's seeded stream (fl_compat/cpc.h), not from ArrayFire's.  Refused arguments: std::invalid_argument (fewer than 4 masked
// frames per utterance among them); a shape beyond the kernels: std::runtime_error.
class FL_COMPAT_API CPCCriterion : public SequenceCriterion {
 public:
  CPCCriterion(int nEncoder, int nContext, int nMutual, int nOffset, int nUnits, int nPieces, int nNegative, int nBuffer, float temperature);
  // input (nEncoder, T, B) f32 -> the same shape with the masked frames replaced; stores the mask, its frames and the negatives
  // for forward().  The seed of call n is setSeed's value + n.
  Variable getMask(const Variable& input, float maskProb, int maskLength);
  // fl_compat extension: frames[b] restricts the spans of utterance b to its first frames[b] frames (empty: all T, padding included,
  // as the reference), and the seed is the caller's
  Variable getMask(const Variable& input, double maskProb, int maskLength, const std::vector<int>& frames, uint64_t seed);
  void setSeed(uint64_t seed) { seed_ = seed; }
  int numMask() const;                                   // masked frames of the last getMask over the whole batch
  Variable getMaskEmbedding() const { return params_[0]; }
  std::vector<int> maskIndex() const;                    // fl_compat extension: [B][M] frames and [B][M][K] negatives of the last getMask
  std::vector<int> negatives() const;
  // inputs {enc (nEncoder, T, B) f32: the encoder output BEFORE masking, ctx (nContext, T, B) f32} -> {loss (B)}
  std::vector<Variable> forward(const std::vector<Variable>& inputs) override;
  af::array viterbiPath(const af::array& input, const af::array& inputSize = af::array()) override;   // throws std::logic_error
  af::array viterbiPathWithTarget(const af::array& input, const af::array& target, const af::array& inputSizes = af::array(),
                                  const af::array& targetSizes = af::array()) override;                // throws std::logic_error
  std::string prettyString() const override;

 private:
  int nEncoder_, nContext_, nMutual_, nOffset_, nUnits_, nPieces_, nNegative_, nBuffer_;
  float temperature_;
  uint64_t seed_ = 0, calls_ = 0;
  std::shared_ptr<void> state_;
};

// fl_compat extension (the validation loop of the reference's test(), recipes/slimIPL/src/Train.cpp:874-980): loss (B) and
// Viterbi path (T, B) s32 of a held-out batch in one call, instead of forward() followed by viterbiPath().  CTC reads the
// emissions once (w2l_ctc_score); ASG runs its loss sequence and the Viterbi pass.  No gradient; the criterion's training
// workspace is not touched (a workspace of its own), so a forward / backward pair around it is unaffected.
FL_COMPAT_API std::pair<af::array, af::array> w2lScore(SequenceCriterion& criterion, const Variable& emission, const Variable& target);
}  // namespace speech
}  // namespace pkg
}  // namespace fl
