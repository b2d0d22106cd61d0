// The deep-path build of the BDPT megakernel: rrDepth 29..1024, whose samples
// can draw past the first 227 outputs of their std::mt19937 (the lazy window
// of the default build). Same source as bdpt_kernels.hip with draws n >= 227
// continued from a per-lane ring of untempered MT19937 outputs in HBM
// (mt_u32_long, dev_rng.hpp); every host-visible symbol gets a _deep name.
#define BDPT_DEEP_RNG 1
// The reference-leaf check stays in the leaf step (bdpt_kernels.hip BDPT_LEAF_DEFER): deferred,
// this build's register allocation spills more (10 -> 18 spilled VGPRs, 176 -> 192 B of scratch).
#ifndef BDPT_LEAF_DEFER
#define BDPT_LEAF_DEFER 0
#endif
#define BDPT_VARIANT _deep
#include "bdpt_kernels.hip"
