// The BDPT megakernel that splits a frame by path length (bdpt_render_layers; DESIGN.md
// §7d): the same source as bdpt_kernels.hip with BDPT_LAYERS 1 — the framebuffer is
// DevFrame::n_layers consecutive W x H x 3 planes and every contribution (the eye walk's
// emitter hits, connectToLight, connectVertices, connectToCamera's splats) is added to
// the plane of its path's edge count instead of one RGB value per pixel (bdpt_path.hpp
// layer_index). The paths, the contributions' values and the schedule are the default
// build's; only where a value is added changes, and no per-sample sum is kept. Serves
// rrDepth 1..28 without Russian roulette, untextured scenes with the BSDF table in LDS
// and all three strategies; every host-visible symbol gets a _layers name.
#define BDPT_LAYERS 1
// The reference-leaf check stays in the leaf step (bdpt_kernels.hip BDPT_LEAF_DEFER): deferred,
// this build's register allocation spills more (2 -> 4 spilled VGPRs).
#ifndef BDPT_LEAF_DEFER
#define BDPT_LEAF_DEFER 0
#endif
#define BDPT_VARIANT _layers
#include "bdpt_kernels.hip"
