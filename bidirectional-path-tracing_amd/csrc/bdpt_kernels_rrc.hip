// The Russian-roulette build for scenes with a dielectric (GlassBSDF): the same
// megakernel as bdpt_kernels_rr.hip plus BDPT_EXPRESS_CHAIN — a lone long walk's
// delta bounces (a subpath trapped in glass by total internal reflection, DESIGN.md
// §8) run back to back inside the express block, each closest hit walked by the
// whole wave, instead of one bounce per pass through the loop top, the walk loop and
// the sweep (Caustic 512^2 x 256: frames 42-45 s -> 35.8-37.4 s). The inline chain
// costs the build's register allocation (92 VGPR spills vs 10), so scenes that
// cannot trap a subpath (no GlassBSDF) keep bdpt_kernels_rr.hip (HardLight RR
// 82.9 vs 78.9 Msamples/s). Chosen per render (bdpt_capi.cpp); every host-visible
// symbol gets an _rrc name.
// Leaf triangles one at a time (dev_traverse.hpp BDPT_WLEAF_GROUP): with pairs
// this build's register allocation spills 79 VGPRs instead of 73 (304 instead
// of 288 bytes of scratch per lane).
#ifndef BDPT_WLEAF_GROUP
#define BDPT_WLEAF_GROUP 1
#endif
#define BDPT_DEEP_RNG 1
#define BDPT_RR 1
#define BDPT_EXPRESS_CHAIN 1
#define BDPT_VARIANT _rrc
#include "bdpt_kernels.hip"
