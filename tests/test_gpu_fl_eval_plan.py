"""fl::Sequential in eval mode runs a plan of its own (include/fl_compat/flashlight.h): a Sequential built from LAYER OBJECTS --
planned without a label count -- put in eval() and run before any train-mode forward still gets emissions (NLABEL, T', B), equal to
what the training plan computes for the same input; an eval forward advances no dropout-seed counter."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "fl_compat/flashlight.h"

int main() {
  const int nf = 8, nl = 7, T = 24, B = 2;
  auto seq = std::make_shared<fl::Sequential>();
  seq->add(std::make_shared<fl::View>(af::dim4(-1, nf, 1, 0)));
  seq->add(std::make_shared<fl::Conv2D>(1, 4, 5, 1, 2, 1, -1, -1));
  seq->add(std::make_shared<fl::ReLU>());
  seq->add(std::make_shared<fl::Dropout>(0.0));
  seq->add(std::make_shared<fl::View>(af::dim4(0, 4 * nf, 1, 0)));
  seq->add(std::make_shared<fl::Reorder>(1, 0, 3, 2));
  seq->add(std::make_shared<fl::Linear>(4 * nf, nl));
  std::vector<float> x((size_t)T * nf * B);
  for (size_t i = 0; i < x.size(); ++i) x[i] = std::sin(0.37f * (float)i);
  fl::Variable in(af::array(af::dim4(T, nf, 1, B), x.data()), false);
  seq->eval();   // eval mode BEFORE any train-mode forward
  auto ev = seq->forward(std::vector<fl::Variable>{in}).front();
  const af::dim4 d = ev.dims();
  const unsigned step0 = fl::pkg::speech::networkStep(seq->planned());
  std::vector<float> he((size_t)ev.elements());
  ev.array().host(he.data());
  seq->train();
  auto tr = seq->forward(std::vector<fl::Variable>{in}).front();
  std::vector<float> ht((size_t)tr.elements());
  tr.array().host(ht.data());
  bool finite = true;
  for (float v : he) finite = finite && std::isfinite(v);
  const bool same = he.size() == ht.size() && std::memcmp(he.data(), ht.data(), he.size() * 4) == 0;
  std::printf("%lld %lld %lld %u %d %d\n", (long long)d[0], (long long)d[1], (long long)d[2], step0, (int)finite, (int)same);
  return 0;
}
'''


def test_layer_object_sequential_in_eval_mode_first(tmp_path):
    lib = os.path.join(ROOT, "wav2letter_amd")
    src = tmp_path / "eval_first.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "eval_first")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + lib, "-lw2l_hip",
                    "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    nl, to, b, step, finite, same = (int(v) for v in out.stdout.split())
    assert (nl, to, b) == (7, 12, 2)        # (NLABEL, T', B): the stride-2 convolution halves T = 24
    assert step == 0                        # the eval forward moved no dropout-seed counter
    assert finite == 1 and same == 1        # eval plan == training plan on the same input (no dropout)
