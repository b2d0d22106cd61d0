// Device-side BDPT building blocks, one header per concern, in the order their
// definitions must stand (out-of-line functions and __shared__ objects are emitted
// in it). Each function cites the reference code (JackMinn/Bidirectional-Path-Tracing)
// whose arithmetic it reproduces. This header adds FrameBuild, what a frame-kernel
// build tells the host about itself.
#pragma once

#include "dev_scene.hpp"     // records, typed loads, the LDS tables, Ray, Hit
#include "dev_rng.hpp"       // MT19937 per lane, its HBM ring, next1 / next2
#include "dev_warp.hpp"      // sampling warps, shading frames
#include "dev_traverse.hpp"  // slab and triangle tests, stacks, the 4-wide and cooperative walks
#include "dev_shade.hpp"     // shade_hit, textures, the deferred leaf check, BSDFs
#include "dev_emitter.hpp"   // CDF search, sample_emitter

namespace bdpt {

// One build of the BDPT frame kernel (bdpt_kernels.hip, compiled once per
// bdpt_kernels_<x>.hip), as bdpt_capi.cpp picks and launches it. `dparams` is a
// device buffer of params_bytes owned by the caller; a launch fills it on
// `stream` first (stream order protects reuse).
struct FrameBuild {
    typedef hipError_t (*Launch)(const dev::DevScene& sc, const dev::DevFrame& fr, float* fb, float* lvbuf,
                                 uint2* gstack, uint32_t nslots, unsigned long long* work,
                                 unsigned long long* counters, int grid, hipStream_t stream, void* dparams);
    const char* name;  // what bdpt_last_kernel reports
    int glossy;        // 0: no Mixture / Phong lobes (bdpt_last_kernel_glossy)
    Launch launch_frame;
    Launch launch_chain;                   // the continuation pass's chain kernel (BDPT_PARK builds), or null
    int (*blocks_per_cu)(size_t dyn_lds);  // resident 256-lane blocks per CU (VGPR and LDS limited)
    int light_vertex_fields;               // floats per light-vertex record
    int block, lds_stack;                  // lanes per block; traversal-stack entries per lane in LDS
    size_t params_bytes;
};
}  // namespace bdpt
