"""Shapes, builders, the plans in Python and the staged entries of include/lcg_hip_staging_dense_f32.h (a real dense matrix stored in
fp32): shared by tests/test_dense_f32_cpu.py, tests/test_gpu_dense_f32_product.py and tests/test_gpu_dense_f32_solvers.py.  A helper of
the tests, not a conftest.

The contract under test is one sentence: the fp32 handle is the fp64 handle of the widened matrix and gives the same bits.  So the
oracle of almost every check is the library's own fp64 path on `twin(K)`; tests/exact_ref.py and the liblcg oracle anchor the pair.

Matrices: K = default_rng(1000 m + n).uniform(-1, 1, (m, n)) cast to float32; the twin is K.astype(float64).

Shapes and the branch each is the smallest to reach (dense.hpp: row_plan, col_plan; NP = ceil(N / 2) packs per row):
  (1, 1) W = 4, one row, one pack with a pad       (5, 7) the odd-N pad, W = 4            (37, 29), ld = 40: rows 40 floats apart
  (100, 80) W = 64 ... forced split: two strips; the one-pass K^T.K.x with U = 1          (1000, 800) U = 2; forced split: nine strips
  (2048, 2048) NP = 1024, the last N of the one-pass form (U = 4); 8-deep unrolled loops run twice per lane
  (1, 4097), (3, 5000) the automatic split, odd / even N, N > 2048: two passes            (8191, 1025) 513 packs, forced split
  (4097, 1), (5000, 3) one pack of columns, the column form folded over many strips of rows
"""
import os

import numpy as np

E_ARG, E_NO_DEVICE = -2003, -2001
KS = (2, 4, 8)
AUTO, ROW, ROW_SPLIT, COL, ATA2, ATA1, ATA_SMALL = range(7)

SHAPES = [(1, 1), (1, 4097), (4097, 1), (3, 5000), (5000, 3), (5, 7), (100, 80), (1000, 800), (2048, 2048), (8191, 1025)]
PADDED = (37, 29, 40)           # m, n, ld

_K = {}


def matrix(m, n):
    """The float32 matrix of a shape.  Nobody writes into it."""
    if (m, n) not in _K:
        K = np.random.default_rng(1000 * m + n).uniform(-1.0, 1.0, (m, n)).astype(np.float32)
        K.setflags(write=False)
        _K[(m, n)] = K
    return _K[(m, n)]


def twin(K32):
    """What the fp32 handle is by definition: the same entries as float64 (exact)."""
    assert K32.dtype == np.float32
    return K32.astype(np.float64)


def padded(K32, ld):
    """K32 as a view of rows ld entries apart, the gap filled with a value no product may see."""
    m, n = K32.shape
    wide = np.full((m, ld), 7.0, K32.dtype)
    wide[:, :n] = K32
    return wide[:, :n]


def pair(api, K32, ld=None):
    """(the fp32 handle, the fp64 handle of the widened matrix), both from host arrays."""
    src = K32 if ld is None else padded(K32, ld)
    F = api.DenseMatrix.from_array_f32(src)
    D = api.DenseMatrix.from_array(twin(K32) if ld is None else padded(twin(K32), ld))
    return F, D


def vector(seed, n, k=None):
    """Full-mantissa float64 data over a few binades."""
    rng = np.random.default_rng(seed)
    shape = n if k is None else (n, k)
    return rng.standard_normal(shape) * np.exp2(rng.integers(-3, 4, shape))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the plans, restated (dense.hpp, dense.hip): which variants lcg_hip_dense_set_kernel accepts for a shape -------------------------
def packs(n):
    return (n + 1) // 2


def cdiv(a, b):
    return -(-a // b)


def forced_strips(m, n):
    S = min(cdiv(8192, m), max(1, packs(n) // 16))
    return cdiv(packs(n), cdiv(packs(n), S))


def accepted(m, n):
    """The variants lcg_hip_dense_set_kernel takes for a real m x n handle of either element width."""
    out = [AUTO, ROW, COL, ATA2]
    if forced_strips(m, n) >= 2:
        out.append(ROW_SPLIT)
    if packs(n) <= 1024:
        out += [ATA1, ATA_SMALL]
    return sorted(out)


# ---- the special values ---------------------------------------------------------------------------------------------------------------
def special_matrix():
    """64 x 66 float32: uniform(-1, 1) with fp32 subnormals (1e-40f and the smallest one, both signs), +0 and -0, FLT_MAX, one row
    holding an Inf and one a quiet NaN.  A conversion that flushes subnormals shows as different bits against the twin."""
    rng = np.random.default_rng(6466)
    K = rng.uniform(-1.0, 1.0, (64, 66)).astype(np.float32)
    tiny, least, big = np.float32(1e-40), np.float32(np.finfo(np.float32).smallest_subnormal), np.float32(np.finfo(np.float32).max)
    assert 0 < least < tiny < np.finfo(np.float32).tiny
    K[0, :] = tiny; K[1, :] = -tiny; K[2, :] = least; K[3, ::2] = -least
    K[4, :] = np.float32(0.0); K[5, :] = np.float32(-0.0)
    K[6, 5] = big; K[7, 64] = -big; K[8, 65] = tiny
    K[:, 10] = tiny; K[:, 11] = least; K[:, 12] = np.float32(-0.0)
    K[20, 3] = np.float32(np.inf)
    K[21, 9] = np.float32(np.nan)
    return K


# ---- the staging header and its table -------------------------------------------------------------------------------------------------
ENTRIES = sorted(["lcg_hip_dense_create_f32", "lcg_hip_dense_value_bytes"])


def staging_header():
    from conftest import ROOT
    return os.path.join(ROOT, "include", "lcg_hip_staging_dense_f32.h")


# The lines the staged entries will bring to stream_cases.STREAM_COVERAGE when they move to lcg_hip.h, in that table's format
_STREAMS = "test_gpu_dense_f32_product.py"
STAGING_COVERAGE = {
    "lcg_hip_dense_create_f32": _STREAMS + "::test_callers_stream",
    "lcg_hip_dense_value_bytes": ("exempt", "a query answered on the host: enqueues nothing"),
}


def staged_prototypes():
    """name -> (return type, [argument kinds]) of every function the staging header declares: "void *" for a pointer or a handle,
    otherwise the argument's type."""
    import re
    src = re.sub(r"/\*.*?\*/", "", open(staging_header()).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*([a-z_ 0-9]+?\*?)\s*(c?lcg_hip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        out[name] = (ret.strip(), ["void *" if ("*" in a or a.split()[0].endswith("_t") and a.split()[0] != "int64_t") else a.split()[-2] for a in args])
    return out
