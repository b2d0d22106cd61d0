// The per-function sampling kernel with the default frame kernels' weight arithmetic: the
// same source as kat_sampling.hip with BDPT_FAST_WEIGHTS 1 (device_math.hpp), where
// sample_emitter's pos_pdf is the 1-ulp rcp_w(area). The kernel and its launcher, with an
// _fw name.
#define BDPT_FAST_WEIGHTS 1
#define SKAT_VARIANT _fw
#include "kat_sampling.hip"
