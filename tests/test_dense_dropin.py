"""The dense examples (examples/sample_dense.cpp: sample1.cpp's workload; examples/sample_dense_complex.cpp: sample3.cpp's)
compile with plain g++ against include/ alone, fail loudly without a GPU and solve their systems with one."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

BIN_DIR = os.path.join(ROOT, "examples", "bin")
NAMES = ["sample_dense", "sample_dense_complex"]


def _build(name):
    from liblcg_amd import _lib
    _lib.build()
    os.makedirs(BIN_DIR, exist_ok=True)
    out = os.path.join(BIN_DIR, name)
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", name + ".cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", out])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_dense_samples_compile_with_plain_gxx_and_fail_loudly_without_gpu(name):
    exe = _build(name)
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 3 and "no HIP device" in p.stderr


def test_host_row_pointers_do_not_compile_into_the_dense_overloads(tmp_path):
    """The reference's lcg_matvec(lcg_float **, ...) is host code and is not provided: a program that still passes host row
    pointers must not compile."""
    src = tmp_path / "host_rows.cpp"
    src.write_text('#include "lcg_dropin.hpp"\nint main() { double **A = 0; double x[1], y[1]; lcg_matvec(A, x, y, MatNormal); return 0; }\n')
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode != 0 and "lcg_matvec" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_dense_samples_solve_their_systems(name):
    exe = _build(name)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rets = dict(re.findall(r"^(\w+): ret=(-?\d+) ", p.stdout, flags=re.M))
    assert len(rets) == (7 if name == "sample_dense" else 5), p.stdout
    assert rets["CG" if name == "sample_dense" else "BICG"] == "0", p.stdout
    assert "k_dn_" in p.stdout
