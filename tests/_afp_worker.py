"""Worker of tests/test_gpu_stop_contract.py::test_python_afp_real_loops (started with LCG_HIP_AX_DOT=0, which the library reads once per
process): CG (classic schedule) and BiCGStab at n = 513 with the built-in product and with a Python Afp that forwards to lcg_hip_spmv.
One line per loop: afp <loop> <ret iterations residual sha1(x)> of the caller's product, the same of the built-in one, Afp calls, max |x_own - x_builtin|."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import stop_cases as sc  # noqa: E402
from liblcg_amd import _lib, api  # noqa: E402


def main():
    assert os.environ.get("LCG_HIP_AX_DOT") == "0"
    lib = _lib.load()
    for name in ("cg_classic", "bicgstab"):
        L = sc.BY_NAME[name]
        S = sc.system(L.kind, 513)
        A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
        bd = torch.from_numpy(S["b"]).cuda()
        calls = [0]

        def my_ax(inst, x, y, nn):
            calls[0] += 1
            lib.lcg_hip_spmv(A.h, x, y)
        out, xs = [], []
        api.set_cg_schedule(api.CG_CLASSIC)
        try:
            for afp, inst in ((my_ax, None), ("lcg_hip_csr_ax", A)):
                m = torch.zeros(513, dtype=torch.float64, device="cuda")
                info = api.lcg_solver(afp, None, m, bd, 513, api.lcg_default_parameters(epsilon=L.eps, abs_diff=L.abs_diff), inst, L.sid)
                xs.append(m.cpu().numpy())
                out += [str(info.ret), str(info.iterations), repr(info.residual), hashlib.sha1(m.cpu().numpy().tobytes()).hexdigest()]
        finally:
            api.set_cg_schedule(api.CG_AUTO)
        print("afp", name, *out, calls[0], repr(float(abs(xs[0] - xs[1]).max())))
        A.destroy()


if __name__ == "__main__":
    main()
