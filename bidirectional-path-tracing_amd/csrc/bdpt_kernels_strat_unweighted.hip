// The strategy build (bdpt_kernels_strat.hip) with BDPT_UNWEIGHTED 1: no
// contribution is multiplied by its misWeight at any of the four places the reference does
// (bdpt.h:98, :356, :427, :482; bdpt_path.hpp mis_factor), so plane (s, t) is that
// strategy's plain estimator. Paths, draws, the 1 / spp scale and the schedule are the
// weighted build's. A unit of its own, so the weighted instance carries no branch on a
// runtime word; every host-visible symbol gets a _strat_unweighted name.
#define BDPT_UNWEIGHTED 1
#define BDPT_VARIANT _strat_unweighted
#include "bdpt_kernels_strat.hip"
