// Diagnostic kernel for bdpt_debug_math (include/bdpt_amd.h): evaluates the
// device restatements of glibc's sinf / cosf / powf and the sincos pair the
// warps use, element-wise, so tests can compare them bit for bit against the
// host libm the reference links (std::sinf / cosf / powf, src/core/math.h).
// math_check_fw.hip compiles it a second time with BDPT_FAST_WEIGHTS 1, where fn 5-9
// are the weight operations of the default frame kernels (device_math.hpp: pow_w,
// rcp_w, div_w, sqrt_w, rsqrt_w on the hardware's 1-ulp instructions); in this unit
// the same codes are their IEEE forms.
#include <hip/hip_runtime.h>

#include "device_math.hpp"

#ifndef MATH_CHECK_VARIANT
#define MATH_CHECK_VARIANT
#endif
#define MC_PASTE(a, b) a##b
#define MC_NAME_(a, b) MC_PASTE(a, b)
#define MC_NAME(x) MC_NAME_(x, MATH_CHECK_VARIANT)

namespace bdpt {
namespace dev {

__global__ __launch_bounds__(256) void MC_NAME(math_check_kernel)(int32_t fn, const float* __restrict__ x,
                                                                  const float* __restrict__ y,
                                                                  float* __restrict__ out, int64_t n) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = x[i];
    float r;
    switch (fn) {
        case 0: r = glibc_sinf(a); break;
        case 1: r = glibc_cosf(a); break;
        case 2: r = glibc_powf(a, y[i]); break;
        case 3: r = glibc_sincosf2(a).s; break;
        case 5: r = pow_w(a, y[i]); break;
        case 6: r = rcp_w(a); break;
        case 7: r = div_w(a, y[i]); break;
        case 8: r = sqrt_w(a); break;
        case 9: r = rsqrt_w(a); break;
        default: r = glibc_sincosf2(a).c; break;
    }
    out[i] = r;
}

}  // namespace dev

hipError_t MC_NAME(launch_math_check)(int32_t fn, const float* x, const float* y, float* out, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned blocks = static_cast<unsigned>((n + 255) / 256);
    hipLaunchKernelGGL(dev::MC_NAME(math_check_kernel), dim3(blocks), dim3(256), 0, st, fn, x, y, out, n);
    return hipGetLastError();
}

}  // namespace bdpt
