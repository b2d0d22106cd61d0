// The BDPT megakernel that splits a frame by emitter and by path length at once
// (bdpt_render_group_layers): the same source as bdpt_kernels.hip with
// BDPT_GROUPS 1 and BDPT_LAYERS 1 — the framebuffer is n_groups * n_layers consecutive
// W x H x 3 planes, the group the outer axis, and every contribution is added to plane
// emitter_group[e] * n_layers + min(k - 1, n_layers - 1) of the emitter e at the light end of
// its k-edge path (bdpt_path.hpp crossed_index). A stored light vertex carries its depth and
// its subpath's group in one word (lv_tag). Paths, values, the task ring and the schedule are
// the default build's; serves what the layers and groups builds serve; every host-visible
// symbol gets a _groups_layers name.
#define BDPT_GROUPS 1
#define BDPT_LAYERS 1
// The reference-leaf check stays in the leaf step, as in both parents (bdpt_kernels_layers.hip).
#ifndef BDPT_LEAF_DEFER
#define BDPT_LEAF_DEFER 0
#endif
#define BDPT_VARIANT _groups_layers
#include "bdpt_kernels.hip"
