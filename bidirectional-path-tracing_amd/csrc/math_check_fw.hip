// math_check.hip with the fast weight arithmetic of the default frame kernels
// (BDPT_FAST_WEIGHTS 1, device_math.hpp): bdpt_debug_math's pow_w / rcp_w / div_w /
// sqrt_w / rsqrt_w codes run here. The kernel and its launcher get an _fw name.
#define BDPT_FAST_WEIGHTS 1
#define MATH_CHECK_VARIANT _fw
#include "math_check.hip"
