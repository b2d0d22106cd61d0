// The crossed group x strategy build (bdpt_kernels_groups_strat.hip) with
// BDPT_UNWEIGHTED 1: no contribution is multiplied by its misWeight (bdpt_path.hpp
// mis_factor), so plane (g, s, t) is strategy (s, t)'s plain estimator of group g's light.
// Every host-visible symbol gets a _groups_strat_unweighted name.
#define BDPT_UNWEIGHTED 1
#define BDPT_VARIANT _groups_strat_unweighted
#include "bdpt_kernels_groups_strat.hip"
