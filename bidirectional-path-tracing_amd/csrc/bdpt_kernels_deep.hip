// The deep-path build of the BDPT megakernel: rrDepth 29..1024, whose samples
// can draw past the first 227 outputs of their std::mt19937 (the lazy window
// of the default build). Same source as bdpt_kernels.hip with draws n >= 227
// continued from a per-lane ring of untempered MT19937 outputs in HBM
// (mt_u32_long, bdpt_device.hpp); every host-visible symbol gets a _deep name.
#define BDPT_DEEP_RNG 1
#define BDPT_VARIANT _deep
#include "bdpt_kernels.hip"
