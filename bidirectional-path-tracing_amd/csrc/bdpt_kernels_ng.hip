// The BDPT megakernel for scenes without a glossy lobe: the same source as
// bdpt_kernels.hip with BDPT_GLOSSY 0 (dev_shade.hpp). It serves material tables
// that hold only DiffuseBSDF, PerfectMirrorBSDF and GlassBSDF records after the
// upload's Ks = 0 conversion (device_bsdfs, bdpt_capi.cpp), in the renders the
// default build serves (no Russian roulette, untextured, rrDepth 4..28, LDS records):
// the Mixture / Phong branches of eval, pdf and sample, the out-of-line sampler call
// and powf are not compiled in, and the ends of a connection skip the test of their
// kind. Task rings, conn_batch and all three <FULL,COUNT,SLACK> instantiations as in
// the default build. Chosen per render (bdpt_capi.cpp; BDPT_NG_BUILD=0/1); every
// host-visible symbol gets an _ng name.
#define BDPT_GLOSSY 0
#define BDPT_VARIANT _ng
#include "bdpt_kernels.hip"
