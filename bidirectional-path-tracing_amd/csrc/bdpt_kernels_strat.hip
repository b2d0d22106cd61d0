// The BDPT megakernel that splits a frame by sampling strategy (bdpt_render_strategies;
// DESIGN.md §7f): the same source as bdpt_kernels.hip with BDPT_STRATS 1 — the framebuffer
// is n_s * n_t consecutive W x H x 3 planes and every contribution (the eye walk's emitter
// hits, connectToLight, connectVertices, connectToCamera's splats) is added to the plane of
// the (s, t) it was formed with, s light-subpath and t eye-subpath vertices, instead of one
// RGB value per pixel (bdpt_path.hpp strat_index). The paths, the contributions' values,
// the task ring and the schedule are the default build's; only where a value is added
// changes, and no per-sample sum is kept. Serves what the layers build serves: rrDepth
// 1..28 without Russian roulette, untextured scenes with the BSDF table in LDS and all
// three strategies; every host-visible symbol gets a _strat name.
// bdpt_kernels_strat_unweighted.hip is this unit without the misWeight factors.
#define BDPT_STRATS 1
#ifndef BDPT_VARIANT
#define BDPT_VARIANT _strat
#endif
#include "bdpt_kernels.hip"
