// The BDPT megakernel that splits a frame by emitter (bdpt_render_light_groups; DESIGN.md
// §7e): the same source as bdpt_kernels.hip with BDPT_GROUPS 1 — the framebuffer is
// n_groups consecutive W x H x 3 planes and every contribution (the eye walk's emitter
// hits, connectToLight, connectVertices, connectToCamera's splats) is added to plane
// DevFrame::emitter_group[e] of the emitter e at the light end of its path instead of one
// RGB value per pixel (bdpt_path.hpp group_index). The paths, the contributions' values,
// the task ring and the schedule are the default build's; only where a value is added
// changes, and no per-sample sum is kept. Serves what the layers build serves: rrDepth
// 1..28 without Russian roulette, untextured scenes with the BSDF table in LDS and all
// three strategies; every host-visible symbol gets a _groups name.
#define BDPT_GROUPS 1
// The reference-leaf check stays in the leaf step (bdpt_kernels.hip BDPT_LEAF_DEFER): deferred,
// this build's register allocation spills more (2 -> 4 spilled VGPRs).
#ifndef BDPT_LEAF_DEFER
#define BDPT_LEAF_DEFER 0
#endif
#define BDPT_VARIANT _groups
#include "bdpt_kernels.hip"
