// The short-subpath build of the BDPT megakernel (BDPT_SPLIT_CONTINUE 1, chosen
// per render for rrDepth <= kSplitMaxRrDepth, bdpt_capi.cpp): the light
// subpath's ContinuePathRandomWalk (bdpt.h:211-215) and its loop test (:188) run
// before the eye subpath's start in the action sweep, so a light walk that ends
// starts its eye walk (bdpt.h:47-65) in the same shading step instead of
// waiting one loop iteration in ST_DEFER; the eye subpath's continuation
// (bdpt.h:152) becomes a body of its own. Same arithmetic in the same order per
// sample; every host-visible symbol gets a _split name.
#define BDPT_SPLIT_CONTINUE 1
#define BDPT_VARIANT _split
#include "bdpt_kernels.hip"
