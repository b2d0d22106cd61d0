// The BDPT megakernel that renders a sample window for a list of pixels instead of whole rows
// (bdpt_render_pixels): the strategy build, bdpt_kernels_strat.hip, with
// BDPT_PIXEL_LIST 1 — work index s is sample win_first + (s % win_count) * win_stride of pixel
// DevFrame::pixel_list[s / win_count] (bdpt_path.hpp sample_seed), n_pixels * win_count samples in
// all. The host fixes the plane shape at (n_s, n_t) = (1, 2): plane 0 takes the camera splats
// (t = 1), which land on any pixel, plane 1 everything formed at the sample's own pixel (t >= 2).
// Adaptive sampling needs the two apart: once pixels differ in their sample counts, the second
// is a mean over the pixel's own samples and the first a mean over all light paths of the frame.
// The paths, the contributions' values, the seeds, the task ring and the schedule are the
// strategy build's; every host-visible symbol gets a _pixels name.
#define BDPT_STRATS 1
#define BDPT_PIXEL_LIST 1
#ifndef BDPT_VARIANT
#define BDPT_VARIANT _pixels
#endif
#include "bdpt_kernels.hip"
