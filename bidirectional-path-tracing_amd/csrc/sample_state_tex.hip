// The single-sample build (sample_state.hip) of the BDPT integrator for scenes
// with bitmap textures: bdpt_render_sample(_mt) on a textured scene runs this
// bdpt_sample_kernel_tex (BDPT_TEXTURED 1, see bdpt_kernels_tex.hip). The path
// and direct integrators are not built for textured scenes.
#define BDPT_SAMPLER_STATE 1
#define BDPT_RR 2  // as sample_state.hip (textured calls always pass rr_mode 0)
#define BDPT_TEXTURED 1
#define BDPT_VARIANT _tex
#include "bdpt_kernels.hip"
