"""fl::Residual through a compiled C++ caller (tests/cpp/residual_caller.cpp, built by tests/cpp/residual_caller.mk): a block put
together with add / addShortcut / addScale inside an fl::Sequential equals the network built from arch text bit for bit -- outputs,
loss and gradients --, with the identity and with a projection on the shortcut, and what the pipeline does not build throws
std::invalid_argument when the Sequential plans."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fl_residual_equals_the_arch_built_network(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "residual_caller.mk", "residual_caller", f"OUT={tmp_path}"],
                   check=True, capture_output=True)
    out = subprocess.run([str(tmp_path / "residual_caller")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "residual caller ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
