// The Russian-roulette build of the BDPT megakernel: the reference's NO_RR = 0
// branch (src/integrators/bdpt.h:18, :68, :129-132, :188, :201-204), selected
// per render by bdpt_frame_params.russian_roulette. Subpaths run past rrDepth
// while sampler.next() < rrProbability, so a sample draws an unbounded number of
// random numbers (the deep build's MT19937 rings continue past draw 226) and
// stores up to DevFrame::depth_cap - 1 light vertices. Same source as
// bdpt_kernels.hip; every host-visible symbol gets an _rr name.
#define BDPT_DEEP_RNG 1
#define BDPT_RR 1
#define BDPT_VARIANT _rr
#include "bdpt_kernels.hip"
