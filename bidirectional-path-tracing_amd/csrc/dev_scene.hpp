// What the kernels are given: typed global-memory loads and stores, the scene and frame
// records (DevScene, DevFrame), the small tables' LDS copy, Ray and Hit.
// Reads BDPT_BSDF_TABLE (where bsdf_of finds the records) and BDPT_TEXTURED (Hit's texels).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bdpt_types.h"
#include "device_math.hpp"

namespace bdpt {
namespace dev {

constexpr float kPi = 3.14159265358979323846f;        // platform.h:50 (float M_PI)
constexpr float kInvPi = 0.31830988618379067154f;     // platform.h:51
constexpr float kInvTwoPi = 0.15915494309189533577f;  // platform.h:52
constexpr float kEpsilon = 1e-8f;                     // platform.h:56
constexpr float kTriMinT = 0x1.0624dep-10f;           // smallest float t with (double)t > 1e-3 (accel.h:43)
constexpr int kCounters = 32;

// ------------------------------------------------------------------ inputs
// Loads through an address-space-1 pointer compile to global_load (SGPR/VGPR
// addressing, vmcnt only) instead of flat_load: the scene pointers arrive via
// a parameter block, so the compiler cannot infer their address space itself.
typedef float v4f_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 gld4(const float4* p) {
    const v4f_t v = *(const __attribute__((address_space(1))) v4f_t*)(p);
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float gld1(const float* p) { return *(const __attribute__((address_space(1))) float*)(p); }
__device__ __forceinline__ void gst1(float* p, float x) { *(__attribute__((address_space(1))) float*)(p) = x; }
__device__ __forceinline__ void gst4(float4* p, float4 x) {
    *(__attribute__((address_space(1))) v4f_t*)(p) = v4f_t{x.x, x.y, x.z, x.w};
}
typedef float v2f_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 gld2(const float2* p) {
    const v2f_t v = *(const __attribute__((address_space(1))) v2f_t*)(p);
    return make_float2(v.x, v.y);
}
__device__ __forceinline__ void gst2(float2* p, float2 x) { *(__attribute__((address_space(1))) v2f_t*)(p) = v2f_t{x.x, x.y}; }

// Bytes of a shadow-ray task record in the waves' rings (bdpt_path.hpp task_push;
// the host sizes DevFrame::tasks by it).
constexpr uint32_t kTaskBytes = 40;

struct DevScene {
    const float4* __restrict__ tri;
    const float4* __restrict__ shade;
    const float4* __restrict__ nodes;   // the reference's binary tree (2 child boxes per record)
    const float4* __restrict__ wnodes;  // 4-wide traversal nodes (wide_bvh.hpp)
    const float4* __restrict__ qnodes;  // the same nodes compressed to 64 B (quantize_wide_nodes), or null
    const float4* __restrict__ wtri;    // traversal triangles, that tree's leaf order (v0|ref index, e1|ref leaf, e2)
    const float4* __restrict__ lbox;    // exact box of every reference leaf (lo, hi)
    const BsdfRecord* __restrict__ bsdf;
    const EmitterRecord* __restrict__ emit;
    const float4* __restrict__ emit_tri;
    const float* __restrict__ emit_cdf;
    const int32_t* __restrict__ shape_emitter;
    uint32_t root_link, wroot_link;
    // 1: the interior boxes of the traversal tree are tested with slab_fast's
    // ambiguity slack; 0 (host decision per render, node_slack_needed in
    // bdpt_capi.cpp): the padded boxes make a plain tn <= tf conservative
    uint32_t node_slack;
    int32_t nemit, nbsdf, nshapes;
    float inv_nemit;  // 1 / nemit (the host's IEEE division): selectEmitter's pdf (core.h emitter selection)
    // LDS copy of the small tables (scene_tables_to_lds): word offsets of the
    // emitter records and the shape->emitter map, total words (16-byte rounded)
    uint32_t lds_emit_off, lds_shape_off, lds_words;
    uint32_t lds_bsdf_off;  // kLdsHdr, or kNoLds: the BSDF records stay in HBM (too many materials)
    // emitter faces (5 float4 each) and CDFs, also in LDS when they fit without
    // costing a resident block (host decision); kNoLds otherwise
    uint32_t lds_etri_off, lds_ecdf_off;
    int32_t n_etri, n_ecdf;
    // MT19937 continuation ring of the megakernel's lanes (rrDepth > 28, Russian
    // roulette): word k of lane slot s at mt_ring[s * kMtRingSlotWords + k] (one 2.5 KB block per
    // slot: a lane's draws touch one page, not 624 pages a slot-count stride apart —
    // a Russian-roulette subpath trapped in glass draws millions of them alone);
    // mt_ring_stride is the word stride within a block (1); null otherwise
    uint32_t* mt_ring;
    uint32_t mt_ring_stride;
    // The scene box grown by 100 scene diagonals: a query whose origin lies
    // outside (far_origin) walks the reference's own binary tree unculled. Far
    // from the scene Moller-Trumbore's arithmetic loses the hit point (cancellation
    // in o - v0), so the reference can accept a triangle the ray's line misses by
    // more than the traversal tree's padding.
    float near_lo[3], near_hi[3];
    uint32_t q_ok;  // qnodes present (no kernel reads them: the walk takes the float records, wnodes)
    uint32_t gdepth;  // traversal-stack overflow entries per lane slot (beyond the LDS ones)
    // Bitmap textures (null without; read by the BDPT_TEXTURED builds only): per material two
    // int4 records — diffuse, specular map: (first texel's index in this table, w, h, 0), index
    // -1 = none — then the pool of float4 texels (rgb, 0) of every map
    const float4* __restrict__ tex_tab;
};
constexpr uint32_t kNoLds = 0xffffffffu;
constexpr uint32_t kLdsHdr = 4;  // LDS header words: mt_ring (2 words), mt_ring_stride, the block's first lane slot

// Small per-scene tables — BSDF records, emitter records, shape -> emitter
// map — live in the kernels' dynamic LDS: the divergent shading code reads
// them with ds_read instead of chains of dependent global loads. Layout (words):
// [0, kLdsHdr) header, [kLdsHdr, emit_off) BsdfRecord[nbsdf], [emit_off, shape_off) EmitterRecord[nemit],
// [shape_off, ...) int32 shape_emitter[nshapes] (unless kNoLds); anything a kernel keeps in
// dynamic LDS besides goes at lds_words.
extern __shared__ uint32_t g_scene_lds[];
// Where the BSDF records are read: 0 = the LDS table only (the frame kernels'
// default build), 1 = HBM only (bdpt_kernels_hbm.hip: scenes whose records do not
// fit the LDS budget), 2 = chosen per launch by sc.lds_bsdf_off (the single-
// sample and per-function kernels: a generic pointer, flat loads — measured 8 %
// slower in the frame kernel, irrelevant for one wave).
#ifndef BDPT_BSDF_TABLE
#define BDPT_BSDF_TABLE 2
#endif
__device__ __forceinline__ const BsdfRecord& bsdf_of(const DevScene& sc, int m) {
#if BDPT_BSDF_TABLE == 1
    return sc.bsdf[m];
#else
#if BDPT_BSDF_TABLE == 2
    if (sc.lds_bsdf_off == kNoLds) return sc.bsdf[m];
#endif
    return reinterpret_cast<const BsdfRecord*>(g_scene_lds + kLdsHdr)[m];
#endif
}
__device__ __forceinline__ const EmitterRecord& emitter_of(const DevScene& sc, int i) {
    return reinterpret_cast<const EmitterRecord*>(g_scene_lds + sc.lds_emit_off)[i];
}
// The shape -> emitter map stays in global memory when a scene has too many
// shapes for the LDS budget (lds_shape_off == kNoLds; read on emitter hits only).
__device__ __forceinline__ int shape_emitter_of(const DevScene& sc, int shape) {
    if (sc.lds_shape_off == kNoLds) return *(const __attribute__((address_space(1))) int32_t*)(sc.shape_emitter + shape);
    return static_cast<int>(g_scene_lds[sc.lds_shape_off + shape]);
}
// Cooperative copy by the whole block, then a barrier.
__device__ __forceinline__ void scene_tables_to_lds(const DevScene& sc) {
    const uint32_t nb = static_cast<uint32_t>(sc.nbsdf) * (sizeof(BsdfRecord) / 4);
    const uint32_t ne = static_cast<uint32_t>(sc.nemit) * (sizeof(EmitterRecord) / 4);
    const uint32_t* b = reinterpret_cast<const uint32_t*>(sc.bsdf);
    const uint32_t* e = reinterpret_cast<const uint32_t*>(sc.emit);
    const uint32_t* m = reinterpret_cast<const uint32_t*>(sc.shape_emitter);
    if (threadIdx.x == 0) {
        const uint64_t ring = reinterpret_cast<uint64_t>(sc.mt_ring);
        g_scene_lds[0] = static_cast<uint32_t>(ring);
        g_scene_lds[1] = static_cast<uint32_t>(ring >> 32);
        g_scene_lds[2] = sc.mt_ring_stride;
        g_scene_lds[3] = blockIdx.x * blockDim.x;  // the block's first lane slot (mt_ring_slot)
    }
    if (sc.lds_bsdf_off != kNoLds)
        for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) g_scene_lds[kLdsHdr + i] = b[i];
    for (uint32_t i = threadIdx.x; i < ne; i += blockDim.x) g_scene_lds[sc.lds_emit_off + i] = e[i];
    if (sc.lds_shape_off != kNoLds)
        for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(sc.nshapes); i += blockDim.x)
            g_scene_lds[sc.lds_shape_off + i] = m[i];
    if (sc.lds_etri_off != kNoLds) {
        const uint32_t* t = reinterpret_cast<const uint32_t*>(sc.emit_tri);
        const uint32_t* c = reinterpret_cast<const uint32_t*>(sc.emit_cdf);
        for (uint32_t i = threadIdx.x; i < 20u * static_cast<uint32_t>(sc.n_etri); i += blockDim.x)
            g_scene_lds[sc.lds_etri_off + i] = t[i];
        for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(sc.n_ecdf); i += blockDim.x)
            g_scene_lds[sc.lds_ecdf_off + i] = c[i];
    }
    __syncthreads();
}

struct DevFrame {
    CameraConstants cam;
    float cam_o[3];
    int32_t W, H, spp, rr_depth, strategy;
    uint32_t seed_base;
    int32_t row_offset, row_stride, nrows;
    uint32_t flags;
    uint64_t total_samples;  // nrows * W * win_count
    int32_t rr_mode;    // 1: NO_RR = 0 (Russian roulette past rr_depth; the bdpt_kernels_rr.hip build)
    int32_t depth_cap;  // subpath depth bound: rr_depth under NO_RR; with RR a guard (2^25 bounces)
    int32_t lv_max;     // light vertices a lane slot stores: rr_depth - 1 under NO_RR, more with RR
    uint32_t* capped;   // RR: samples that hit depth_cap or lv_max (the frame is then not the reference's)
    // frame-kernel timeline (s_memrealtime ticks): [0] first wave start (min), [1]
    // the claim of the last 64-sample chunk, [2] last wave exit (max) — the end
    // tail a row shard pays is [2] - [1] (kDiag*)
    unsigned long long* diag;
    // 1 / spp and 1 / (W * H) as the host's IEEE divisions, the bits the device's correctly
    // rounded reciprocal (rcp_cr) and division give: per-frame constants the shading bodies
    // would otherwise recompute (~10 instructions each) per splat and per sample
    float inv_spp, inv_pixels;
    // Russian-roulette continuation pass (bdpt_kernels.hip): per lane slot a
    // kParkWords record, then the list of parked slots ([0] count); null: off.
    // park_flags: kParkOn (park walks deeper than park_depth), kParkResume (this
    // launch resumes the records the chain kernel returned instead of claiming)
    uint32_t* park;
    int32_t park_depth;
    uint32_t park_flags;
    // lanes with a finished query that trigger a wave's shading step (the frame
    // kernels; chosen per render by the host: 0 = the build's BDPT_SHADE_READY)
    int32_t shade_ready;
    // Russian-roulette build: a subpath deeper than express_depth bounces puts its
    // wave in express mode (bdpt_kernels.hip); sched_flags kSchedNoCoopGroups walks
    // express waves' 2-4 long walks in turn instead of in lane groups. Schedule
    // only: the same per-sample arithmetic either way (tests/test_gpu_express.py).
    int32_t express_depth;
    uint32_t sched_flags;
    // Shadow-ray task rings of the BDPT_HELP build (bdpt_path.hpp task_push): per
    // wave task_cap records of kTaskBytes, wave w's at tasks + kTaskBytes / 16 * task_cap * w
    // (allocated by the first bdpt_render that launches such a build)
    float4* tasks;
    uint32_t task_cap;
    // the shard's row claim order (bdpt_set_row_order; null: top to bottom) and, in a
    // counting pass, the queries issued per local row (null otherwise).
    // The pixel-list build (bdpt_render_pixels, bdpt_kernels_pixels.hip) keeps its list in the same
    // word: total_samples / win_count ascending pixel indices in [0, W * H). A pixel-list render
    // refuses row shards and a row order, and no other build reads the word as a list, so the
    // record and every other build's code stay as they were.
    union {
        const int32_t* row_order;
        const int32_t* pixel_list;
    };
    // light groups (bdpt_render_light_groups, the bdpt_kernels_groups.hip build): the framebuffer
    // is n_groups consecutive W x H x 3 planes and a contribution goes to plane emitter_group[e]
    // of the emitter e its path ends on (one int32 per emitter, each in [0, n_groups)). It shares
    // row_cost's word, so the record and every other build's code stay as they were: a grouped
    // render is never a counting pass (flags are refused) and no other build reads it. The crossed
    // builds (bdpt_kernels_groups_layers.hip, bdpt_kernels_groups_strat*.hip) read it together with
    // n_layers / strat_shape below, which lie in another union: both are set in one launch.
    union {
        unsigned long long* row_cost;
        const int32_t* emitter_group;
    };
    // sample window (bdpt_render_window): of each pixel's spp samples only k = win_first +
    // i * win_stride, 0 <= i < win_count, are rendered (the whole frame: 0, 1, spp); seeds,
    // inv_spp and camera_dir's spp == 1 rule keep the frame's full spp
    int32_t win_first, win_stride, win_count;
    // path-length layers (bdpt_render_layers, the bdpt_kernels_layers.hip build): the framebuffer
    // is n_layers consecutive W x H x 3 planes and a contribution of a path with k edges goes to
    // plane min(k - 1, n_layers - 1). 0 and unread in every other build.
    // Strategy images (bdpt_render_strategies, the bdpt_kernels_strat*.hip builds) keep their
    // shape in the same word: strat_shape = n_s << 8 | n_t, the framebuffer n_s * n_t planes.
    union {
        int32_t n_layers;
        int32_t strat_shape;
    };
};
enum : uint32_t { kParkOn = 1u, kParkResume = 2u };
// kSchedLeafRecheck (BDPT_LEAF_DEFER builds, a debugging knob): the deferred reference-leaf
// check reports failure for every hit, so every closest hit is walked again in checked mode
enum : uint32_t { kSchedNoCoopGroups = 1u, kSchedLeafRecheck = 2u };

struct Ray {
    f3 o, d;
    float min_t, max_t;
};

// Hit record = the parts of SurfaceInteraction (core.h:173-180) the path reads.
#ifndef BDPT_TEXTURED
#define BDPT_TEXTURED 0  // 1: the builds for scenes with bitmap textures (bdpt_kernels_tex.hip)
#endif
struct Hit {
    f3 p, wo;
    f3 n;  // frameNs.n; s and t are recomputed from it (Frame(n) is a pure function of n)
    float dist;
    int mat, shape;
#if BDPT_TEXTURED
    // BitmapTexture3f::eval's texel (core.h:569-587) of the material's diffuse / specular map
    // at this hit, as an index into DevScene::tex_tab; -1: the material record's constant
    int tkd, tks;
#endif
};

}  // namespace dev
}  // namespace bdpt
