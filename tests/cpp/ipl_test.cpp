// ipl_test.cpp -- fl_compat/ipl.h replayed against its Python twin (tests/ipl_ref.py; compiled and run by tests/test_ipl_host.py).
//   ipl_test scenarios          the scripted runs of ipl_ref.scenarios(), one decision per line
//   ipl_test files <dir> <world> <U> <nUnsup>   cache files in, cache files out (formats, missing rank file, state round trip)
// With -DIPL_TEST_FACADE (linked against libw2l_hip.so, run on the GPU by tests/test_gpu_ema.py):
//   ipl_test facade             fl::ext::selectBatch, fl::ext::emaUpdate and fl::Sequential::setTransformerDropout
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/fl_compat/ipl.h"
#ifdef IPL_TEST_FACADE
#include "../../include/fl_compat/flashlight.h"
#include "../../include/w2l_hip.h"
#endif

using namespace fl::pkg::speech;

static const char* kTypes[4] = {"naive", "cache", "pre-cache", "fixed-pre-cache"};

static std::vector<std::string> ids(long b, int per) {
  std::vector<std::string> v;
  for (int k = 0; k < per; ++k) v.push_back("s" + std::to_string(b) + "_" + std::to_string(k));
  return v;
}
static std::vector<std::string> teacher(long b, int t, int per, const char* mark = "") {
  std::vector<std::string> v;
  for (int k = 0; k < per; ++k) v.push_back("w" + std::to_string(b) + " x" + std::to_string(k) + " t" + std::to_string(t) + mark);
  return v;
}
template <class T> static std::string joined(const std::vector<T>& v, const char* sep) {
  std::ostringstream s;
  for (size_t i = 0; i < v.size(); ++i) s << (i ? sep : "") << v[i];
  return s.str();
}

static void scenario(const std::string& type, long sup, long unsup, long nUnsup, long U, double prob, uint64_t seed) {
  const int steps = 40, supPerEpoch = 4, per = 2;
  SlimIPL::Options o;
  o.type = parseIplType(type); o.supUpdates = sup; o.unsupUpdates = unsup; o.fixedCacheUpdates = U; o.fixedCacheUpdateProb = prob;
  SlimIPL ipl(o, nUnsup, seed);
  ipl.begin();
  bool need = true;
  int supIn = 0;
  for (int t = 1; t <= steps; ++t) {
    if (need) { ipl.startEpoch(); need = false; std::cout << t << " epoch\n"; }
    if (ipl.nextIsSup()) {
      ipl.advanceOrder();
      std::cout << t << " sup\n";
      if (++supIn == supPerEpoch) { need = true; supIn = 0; }
      continue;
    }
    const SlimIPL::Unsup u = ipl.nextUnsup();
    ipl.advanceOrder();
    std::vector<int> rows;
    std::vector<std::string> texts, toSave;
    bool save = false;
    if (o.type == IplType::Naive) {
      texts = teacher(u.trainBatch, t, per);
      for (int k = 0; k < per; ++k) rows.push_back(k);
    } else {
      if (u.trainBatch >= 0) {
        auto l = ipl.labelled(ids(u.trainBatch, per));
        rows = l.rows; texts = l.texts;
        if (ipl.labelBeforeUpdate(rows.size())) { toSave = teacher(u.trainBatch, t, per); save = true; }
      }
      if (u.labelNext >= 0) ipl.store(ids(u.labelNext, per), teacher(u.labelNext, t, per));
    }
    if (save) ipl.store(ids(u.trainBatch, per), toSave);
    if (u.trainBatch >= 0 && ipl.labelAfterUpdate()) ipl.store(ids(u.trainBatch, per), teacher(u.trainBatch, t, per, "'"));
    std::cout << t << " unsup train=" << u.trainBatch << " pos=" << u.position << " relabel=" << (u.relabel ? 1 : 0) << " next=" << u.labelNext
              << " rows=" << joined(rows, ",") << " texts=" << joined(texts, ";") << " update=" << (rows.empty() ? 0 : 1) << "\n";
  }
  std::cout << "cache ";
  for (auto& kv : ipl.plCache) std::cout << kv.first << "|" << kv.second << "/";
  std::cout << "\nfixed ";
  for (long v : ipl.fixedCache) std::cout << v << " ";
  std::cout << "\nstate " << ipl.state() << "\n";
}

#ifdef IPL_TEST_FACADE
#define EXPECT(c) do { if (!(c)) { std::cout << "FAILED line " << __LINE__ << ": " #c "\n"; return 1; } } while (0)
struct Bag : fl::Module {   // a module that is no planned pipeline: emaUpdate walks its parameters
  explicit Bag(const std::vector<std::vector<float>>& v) { for (auto& a : v) params_.push_back(fl::Variable(af::array(af::dim4((af::dim_t)a.size()), a.data()), true)); }
  std::vector<fl::Variable> forward(const std::vector<fl::Variable>& in) override { return in; }
  std::string prettyString() const override { return "Bag"; }
};
static int facade() {
  // ---- selectBatch: B = 4, rows {2, 0}
  const int N = 5, T = 3, B = 4, per = N * T;
  std::vector<float> h((size_t)per * B), g((size_t)per * 2);
  for (size_t i = 0; i < h.size(); ++i) h[i] = 0.25f * (float)i - 3.f;
  for (size_t i = 0; i < g.size(); ++i) g[i] = 1.f + 0.5f * (float)i;
  fl::Variable em(af::array(af::dim4(N, T, B), h.data()), true);
  const std::vector<int> rows = {2, 0};
  fl::Variable sel = fl::ext::selectBatch(em, rows);
  EXPECT(sel.dims(0) == N && sel.dims(1) == T && sel.dims(2) == 2);
  std::vector<float> got((size_t)per * 2);
  sel.host(got.data());
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < per; ++i) EXPECT(got[(size_t)k * per + i] == h[(size_t)rows[(size_t)k] * per + i]);
  sel.backward(fl::Variable(af::array(af::dim4(N, T, 2), g.data()), false));
  std::vector<float> dg((size_t)per * B);
  em.grad().host(dg.data());
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < per; ++i) {
      const float want = b == 2 ? g[(size_t)i] : b == 0 ? g[(size_t)per + i] : 0.f;
      EXPECT(dg[(size_t)b * per + i] == want);
    }
  fl::Variable all = fl::ext::selectBatch(em, {0, 1, 2, 3});
  EXPECT(all.array().device<float>() == em.array().device<float>());   // all rows in order: the argument itself
  bool threw = false;
  try { fl::ext::selectBatch(em, {1, 4}); } catch (const std::invalid_argument&) { threw = true; }
  EXPECT(threw);
  std::cout << "selectBatch ok\n";
  // ---- emaUpdate: two planned networks of one arch -> the arenas in one call; anything else -> per parameter
  const std::string arch = "V -1 1 NFEAT 0\nRO 2 0 3 1\nTR 16 32 2 5 0.3 0.3\nL 16 NLABEL\n";
  auto student = fl::pkg::speech::buildSequentialModuleFromText(arch, 16, 7);
  auto teacher = fl::pkg::speech::buildSequentialModuleFromText(arch, 16, 7);
  auto ps = fl::pkg::speech::flatParameters(student), pt = fl::pkg::speech::flatParameters(teacher);
  EXPECT(ps.ptr && pt.ptr && ps.floats == pt.floats && ps.ptr != pt.ptr);
  EXPECT(w2l_fill(ps.ptr, ps.floats, 2.f, fl::currentStream()) == W2L_OK && w2l_fill(pt.ptr, pt.floats, 1.f, fl::currentStream()) == W2L_OK);
  fl::ext::emaUpdate(teacher, student, 0.75);
  size_t seen = 0;
  for (auto& p : teacher->params()) {
    std::vector<float> v((size_t)p.elements());
    p.host(v.data());
    for (float x : v) EXPECT(x == 1.25f);
    seen += v.size();
  }
  EXPECT(seen > 0);
  for (auto& p : student->params()) { std::vector<float> v((size_t)p.elements()); p.host(v.data()); for (float x : v) EXPECT(x == 2.f); }
  auto a = std::make_shared<Bag>(std::vector<std::vector<float>>{{1.f, 2.f, 3.f}, {4.f}});
  auto b = std::make_shared<Bag>(std::vector<std::vector<float>>{{3.f, 2.f, 1.f}, {8.f}});
  fl::ext::emaUpdate(a, b, 0.5);
  std::vector<float> v0(3), v1(1);
  a->params()[0].host(v0.data()); a->params()[1].host(v1.data());
  EXPECT(v0[0] == 2.f && v0[1] == 2.f && v0[2] == 2.f && v1[0] == 6.f);
  threw = false;
  try { fl::ext::emaUpdate(a, b, 1.5); } catch (const std::invalid_argument&) { threw = true; }
  EXPECT(threw);
  threw = false;
  try { fl::ext::emaUpdate(a, student, 0.5); } catch (const std::invalid_argument&) { threw = true; }
  EXPECT(threw);
  std::cout << "emaUpdate ok\n";
  // ---- setTransformerDropout: a planned pipeline takes it, refuses a probability of 1; a chain of other modules has none
  student->setTransformerDropout(0.1, 0.1);
  student->setTransformerDropout(-1, -1);
  threw = false;
  try { student->setTransformerDropout(1.0, 0.0); } catch (const std::invalid_argument&) { threw = true; }
  EXPECT(threw);
  fl::Sequential chain;
  chain.add(std::static_pointer_cast<fl::Module>(a));
  threw = false;
  try { chain.setTransformerDropout(0.1, 0.1); } catch (const std::logic_error&) { threw = true; }
  EXPECT(threw);
  std::cout << "setTransformerDropout ok\n";
  return 0;
}
#endif

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  try {
#ifdef IPL_TEST_FACADE
    if (mode == "facade") return facade();
#endif
    if (mode == "scenarios") {
      int count = 0;
      for (const char* type : kTypes)
        for (int ratio = 0; ratio < 2; ++ratio)
          for (long nUnsup : {3L, 7L}) {
            const bool fixed = std::string(type) == "fixed-pre-cache";
            const long Us[2] = {2, 5};
            const double probs[3] = {0.0, 0.5, 1.0};
            for (int ui = 0; ui < (fixed ? 2 : 1); ++ui)
              for (int pi = 0; pi < (fixed ? 3 : 1); ++pi) {
                const long sup = ratio == 0 ? 1 : 0, unsup = ratio == 0 ? 3 : 1, U = Us[ui];
                const double prob = fixed ? probs[pi] : 1.0;
                std::cout << "== " << type << " " << sup << " " << unsup << " " << nUnsup << " " << U << " " << prob << "\n";
                scenario(type, sup, unsup, nUnsup, U, prob, (uint64_t)(7 + count));
                ++count;
              }
          }
      return 0;
    }
    if (mode == "files" && argc == 6) {
      const std::string dir = argv[2];
      const int world = atoi(argv[3]);
      SlimIPL::Options o;
      o.type = IplType::FixedPreCache; o.fixedCacheUpdates = atol(argv[4]);
      SlimIPL ipl(o, atol(argv[5]), 1);
      for (int r = 0; r < world; ++r) std::cout << "rank " << r << ": " << ipl.loadCacheDump(dir + "/in_cache" + std::to_string(r)) << "\n";
      std::vector<std::string> all;
      for (auto& kv : ipl.plCacheDump) all.push_back(kv.first);
      auto l = ipl.labelled(all);
      std::cout << "reused " << l.reused.size() << " rows " << l.rows.size() << "\n";
      ipl.saveCache(dir + "/out_cache");
      std::cout << "fixed " << (ipl.loadFixedCache(dir + "/in_fixed") ? 1 : 0) << " " << ipl.fixedCache.size() << "\n";
      std::cout << "missing " << (ipl.loadFixedCache(dir + "/nope") ? 1 : 0) << "\n";
      ipl.saveFixedCache(dir + "/out_fixed");
      ipl.begin();
      ipl.startEpoch();
      for (int k = 0; k < 5; ++k) { if (!ipl.nextIsSup()) ipl.nextUnsup(); ipl.advanceOrder(); }
      SlimIPL twin(o, atol(argv[5]), 99);
      twin.fixedCache = ipl.fixedCache;
      twin.setState(ipl.state());
      std::cout << "state " << (twin.state() == ipl.state() ? "same" : "differs") << "\n";
      for (int k = 0; k < 7; ++k) {
        const bool a = ipl.nextIsSup(), b = twin.nextIsSup();
        long ta = -2, tb = -2;
        if (!a) ta = ipl.nextUnsup().trainBatch;
        if (!b) tb = twin.nextUnsup().trainBatch;
        ipl.advanceOrder(); twin.advanceOrder();
        if (a != b || ta != tb) { std::cout << "resumed run diverges\n"; return 1; }
      }
      std::cout << "resumed same\n";
      return 0;
    }
    if (mode == "refuse") {
      try { parseIplType(argc > 2 ? argv[2] : ""); } catch (const std::invalid_argument& e) { std::cout << e.what() << "\n"; return 0; }
      return 1;
    }
  } catch (const std::exception& e) {
    std::cerr << "ipl_test: " << e.what() << "\n";
    return 1;
  }
  std::cerr << "usage: ipl_test scenarios | files <dir> <world> <U> <nUnsup> | refuse <type>\n";
  return 2;
}
