// The per-function BSDF kernel with the default frame kernels' weight arithmetic: the
// same source as kat_kernels.hip with BDPT_FAST_WEIGHTS 1 (device_math.hpp: pow_w as
// exp2(y * log2 x) on the hardware instructions, the 1-ulp rcp_w / div_w / sqrt_w /
// rsqrt_w), as bdpt_kernels.hip sets it for the frame kernels without Russian
// roulette. Only the BSDF kernel and its launcher, with an _fw name.
#define BDPT_FAST_WEIGHTS 1
#define KAT_VARIANT _fw
#include "kat_kernels.hip"
