// The BDPT megakernel for scenes with bitmap textures (map_Kd / map_Ks, the
// reference's BitmapTexture3f, core.h:525-588): the same source as
// bdpt_kernels.hip with BDPT_TEXTURED 1 — every closest hit looks up its texels
// (shade_hit), a path vertex carries their two indices into the flat pool
// (Hit::tkd / tks, an 80-byte light-vertex record) and the BSDF code reads Kd / Ks
// from the pool where a map exists (bsdf_tex). Serves rrDepth 1..28 without
// Russian roulette and all three strategies; every host-visible symbol gets a
// _tex name. Selected by bdpt_render when the scene has at least one map.
#define BDPT_TEXTURED 1
#define bdpt_frame_kernel bdpt_frame_kernel_tex
#define bdpt_sample_kernel bdpt_sample_kernel_tex
#define frame_params_bytes frame_params_bytes_tex
#define launch_frame launch_frame_tex
#define launch_sample launch_sample_tex
#define frame_kernel_blocks_per_cu frame_kernel_blocks_per_cu_tex
#define frame_kernel_lds_stack frame_kernel_lds_stack_tex
#define frame_kernel_block frame_kernel_block_tex
#define light_vertex_fields light_vertex_fields_tex
#include "bdpt_kernels.hip"
