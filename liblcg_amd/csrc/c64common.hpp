// c64common.hpp -- complex64 arithmetic shared by the products (csr_c64.hip) and the loops (solvers_c64.hip), so that the
// Jacobi reciprocal, the callback's z = inv .* r and the loops' fused twin and step lengths round the same way.
#pragma once

#include <hip/hip_runtime.h>

namespace lcgh {

__device__ __forceinline__ float2 c64_mul(float2 a, float2 b)      // a * b, fixed fma order
{
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}

__device__ __forceinline__ float2 c64_div(float2 a, float2 b)      // a / b with the operands scaled by |b.x| + |b.y| (cuCdivf's formula)
{
    float s = fabsf(b.x) + fabsf(b.y);
    float oos = 1.0f / s;
    const float ars = a.x * oos, ais = a.y * oos, brs = b.x * oos, bis = b.y * oos;
    s = brs * brs + bis * bis;
    oos = 1.0f / s;
    return make_float2((ars * brs + ais * bis) * oos, (ais * brs - ars * bis) * oos);
}

} // namespace lcgh
