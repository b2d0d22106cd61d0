// The BDPT megakernel that splits a frame by emitter and by sampling strategy at once
// (bdpt_render_group_strategies): the same source as bdpt_kernels.hip with
// BDPT_GROUPS 1 and BDPT_STRATS 1 — the framebuffer is n_groups * n_s * n_t consecutive
// W x H x 3 planes, the group the outer axis, and every contribution is added to plane
// emitter_group[e] * n_s * n_t + strat_plane(s, t) of the emitter e at the light end of its path
// and the (s, t) it was formed with (bdpt_path.hpp crossed_index). A stored light vertex
// carries its depth and its subpath's group in one word (lv_tag). Paths, values, the task ring
// and the schedule are the default build's; serves what the strategy and groups builds serve;
// every host-visible symbol gets a _groups_strat name.
// bdpt_kernels_groups_strat_unweighted.hip is this unit without the misWeight factors.
#define BDPT_GROUPS 1
#define BDPT_STRATS 1
#ifndef BDPT_VARIANT
#define BDPT_VARIANT _groups_strat
#endif
#include "bdpt_kernels.hip"
