// The BDPT megakernel for scenes with bitmap textures (map_Kd / map_Ks, the
// reference's BitmapTexture3f, core.h:525-588): the same source as
// bdpt_kernels.hip with BDPT_TEXTURED 1 — every closest hit looks up its texels
// (shade_hit), a path vertex carries their two indices into the flat pool
// (Hit::tkd / tks, an 80-byte light-vertex record) and the BSDF code reads Kd / Ks
// from the pool where a map exists (bsdf_tex). Serves rrDepth 1..28 without
// Russian roulette and all three strategies; every host-visible symbol gets a
// _tex name. Selected by bdpt_render when the scene has at least one map.
#define BDPT_TEXTURED 1
#define BDPT_VARIANT _tex
#include "bdpt_kernels.hip"
