/*
 * bdpt_amd — MI355X-native bidirectional path tracer: the C-ABI drop-in
 * boundary for the reference's BDPT hot path.
 *
 * Reference (JackMinn/Bidirectional-Path-Tracing) interfaces these entry points
 * replace:
 *   bdpt_scene_load_obj      Scene::load                      src/core/renderer.cpp:235-315
 *                            (tinyobj LoadObj :249, BSDFs per illum :258-271,
 *                             emitters :279-305, AcceleratorBVH::build accel.h:115-123)
 *   bdpt_scene_create        the Scene the Integrator holds (core.h:352-358: worldData, bsdfs,
 *                            emitters, bvh) handed over from the caller's memory
 *   bdpt_camera_constants    camera set-up of Renderer::render renderer.cpp:140-153
 *                            and BDPTIntegrator bdpt.h:49-54, :485-489
 *   bdpt_ctx_create          Integrator::init (rgb allocation) src/core/integrator.cpp:16-20
 *                            + upload of the Scene the integrator holds by reference
 *   bdpt_render              the offline loop of Renderer::render renderer.cpp:130-214
 *                            calling BDPTIntegrator::render bdpt.h:219-241 for every
 *                            (pixel, sample), with camera splats (bdpt.h:295-371)
 *                            accumulated into the same framebuffer
 *   bdpt_render_sample_mt    virtual v3f Integrator::render(const Ray&, Sampler&) const
 *                            src/core/integrator.h:31, overridden at bdpt.h:219, with the
 *                            caller's Sampler (std::mt19937 state, src/core/math.h:63-76)
 *   bdpt_render_sample       the same, Sampler given as (seed, draws already taken)
 *   bdpt_bsdf_eval/pdf/sample  BSDF::eval / pdf / sample        src/core/core.h:308-310
 *                            (diffuse.h:35-61, perfectmirror.h:33-59, glass.h:55-108,
 *                             mixture.h:60-151, phong.h) of a scene material, batched
 *   bdpt_intersect           AcceleratorBVH::intersect / occlusion  src/core/accel.h:125-172,
 *                            externals/bvh.h:259-352 (as visibilityQuery calls it, bdpt.h:498-505)
 *   bdpt_splat_to_image_plane  BDPTIntegrator::splatToImagePlane   bdpt.h:485-496
 *   bdpt_ctx_destroy         Integrator/Renderer teardown (renderer.cpp:221-227)
 *   bdpt_config_load_toml    loadTOML                         src/main.cpp:22-116
 *   bdpt_save_exr            Integrator::save -> saveEXR      integrator.cpp:26-30, utils.h:95-156
 *   (CLI lib/tinyrender_amd) main / run                       src/main.cpp:121-181
 *   bdpt_render_path         PathTracerIntegrator::render     src/integrators/path.h:235-245 for every
 *                            (pixel, sample) of the offline loop (the reference's other offline
 *                            integrator, TOML type = "path"), on the same GPU substrate
 *   bdpt_render_direct       DirectIntegrator::render         src/integrators/direct.h:449-462 (TOML
 *                            type = "direct": area / solidAngle / cosineHemisphere / bsdf / mis)
 *   bdpt_render_window       a part of the offline loop's inner sample loop (renderer.cpp:160, the
 *                            samples k = first + i * stride of every pixel) for any of the three
 *                            integrators: progressive, resumable and sample-sharded frames
 *   bdpt_render_aov          (no counterpart) the primary query of every camera sample of that loop
 *                            (renderer.cpp:162-192, accel.h:125-172) as albedo / normal / depth / coverage
 *   bdpt_denoise             (no counterpart) an edge-avoiding filter of a low-spp frame on the device
 *   bdpt_denoise_planes      (no counterpart) that filter for the planes of a split frame, with weights
 *                            of their own or one set for all, under which the planes still add up
 *   bdpt_batch_moments       (no counterpart) the per-pixel sum and variance across sample batches
 *   bdpt_denoise_var         (no counterpart) the filter with its colour weight in standard deviations
 *   bdpt_render_pixels       (no counterpart) a sample window of the BDPT frame for a list of pixels
 *   bdpt_render_adaptive     (no counterpart) further samples only where the batch variance asks
 *   bdpt_reproject           (no counterpart) a preview's history reprojected into the next camera's frame
 *   bdpt_meter               (no counterpart) exposure and white point from a luminance histogram of the frame
 *   bdpt_display             srgb.fs (renderpass.cpp:397) exposure, tone curve and 8-bit encode on the device
 *   bdpt_save_png / _ppm     (no counterpart) the 8-bit frame as a PNG or PPM file
 *
 * Conventions: plain C types only; status 0 = OK, < 0 = error (message from
 * bdpt_last_error(), thread-local). A context is bound to one HIP device and is
 * not thread-safe: callers that render from several threads (the reference's
 * parallel_for, renderer.cpp:157) keep one context per thread. Calls on one
 * context are ordered even across streams (each call waits for the previous
 * call's work on its stream before touching the context's buffers). Nothing
 * here falls back to the CPU: without a HIP device, bdpt_ctx_create fails with
 * BDPT_ERR_NO_DEVICE.
 *
 * Determinism: camera sample (pixel p, sample k) draws from
 * std::mt19937(seed_base + p*spp + k) exactly like the reference's Sampler
 * (src/core/math.h:63-76), and all arithmetic follows the reference's single-
 * precision operation order, so paths are identical to the CPU reference; only
 * the order of floating-point additions into the framebuffer differs.
 */
#ifndef BDPT_AMD_H
#define BDPT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDPT_OK 0
#define BDPT_ERR_INVALID -1
#define BDPT_ERR_IO -2
#define BDPT_ERR_NO_DEVICE -3
#define BDPT_ERR_HIP -4
#define BDPT_ERR_UNSUPPORTED -5

/* Strategy switches of the reference (bdpt.h:16-17, compile-time there). */
#define BDPT_STRATEGY_BDPT 0
#define BDPT_STRATEGY_LIGHT_TRACING 1
#define BDPT_STRATEGY_PATH_TRACING 2

/* bdpt_frame_params.flags */
#define BDPT_FLAG_COUNT 1u            /* counting pass: fill bdpt_stats.counters (slower) */
#define BDPT_FLAG_FULL_TRAVERSAL 2u   /* visit every box the reference visits (no t-culling) */
/* (bit 2, the round-1 wavefront schedule, was removed: the megakernel beat it ~5x; now BDPT_ERR_UNSUPPORTED) */

typedef struct bdpt_scene bdpt_scene; /* host-side ingested scene */
typedef struct bdpt_ctx bdpt_ctx;     /* device context (one HIP device) */

typedef struct {
    int64_t triangles, bvh_nodes, shapes, materials, emitters, bvh_max_depth;
    int64_t device_bytes; /* HBM bytes of the uploaded scene arrays */
    int64_t bvh_leaves;   /* reference BVH leaves (<= 4 triangles each) */
    int64_t wide_nodes;   /* 4-wide traversal nodes */
    int64_t wide_depth, wide_max_stack;
    int64_t wide_leaves;  /* leaves of the traversal tree */
    int64_t triangle_tree; /* 1: SAH tree over single triangles (default); 0: over the reference
                              leaves (environment BDPT_TRAV_TREE=refleaf at scene load) */
} bdpt_scene_info;

typedef struct {
    float eye[3], at[3], up[3]; /* [camera] eye / at / up (main.cpp:31-37) */
    float fov;                  /* degrees */
} bdpt_camera;

typedef struct {
    bdpt_camera camera;
    int32_t width, height; /* [film] (the global image; shards still splat into it) */
    int32_t spp;           /* [renderer] spp */
    int32_t rr_depth;      /* [renderer] rrDepth (bdpt.h:39): with russian_roulette 0 the hard path-depth
                              cap (NO_RR = 1, bdpt.h:18), else where Russian roulette starts; 1..1024 */
    int32_t strategy;      /* BDPT_STRATEGY_* (reference default: BDPT) */
    uint32_t seed_base;    /* 260450963 = the reference's Sampler seed (renderer.cpp:155) */
    int32_t row_offset;    /* shard: render rows row_offset, row_offset+row_stride, ... */
    int32_t row_stride;    /*        (1 = whole image)                                   */
    uint32_t flags;        /* BDPT_FLAG_* */
    int32_t russian_roulette; /* BDPT_RR_*: 0 = the reference as shipped (NO_RR 1, bdpt.h:18); 1 = its
                                 NO_RR 0 branch (bdpt.h:68, :129-132, :188, :201-204) */
} bdpt_frame_params;

/* bdpt_frame_params.russian_roulette */
#define BDPT_RR_NONE 0      /* NO_RR 1: every subpath stops at rrDepth (one draw at the cap) */
#define BDPT_RR_LUMINANCE 1 /* NO_RR 0: past rrDepth a subpath continues while sampler.next() < rr, with
                               rr = (luminance(throughput) < 0.01 ? 0.5 : 1) stored per vertex and entering
                               every pdf (rr * pdf); no depth cap (see bdpt_stats.capped_samples) */

#define BDPT_NUM_COUNTERS 32
/* counters: [0] closest-hit rays, [1] shadow rays, [2] interior-node visits,
 * [3] triangle tests, [4] light vertices stored, [5] light-vertex reads,
 * [6] camera splats, [7] RNG draws; SIMD-efficiency probes: [8] traversal
 * iterations summed over lanes, [9] the same counted once per wave, [10]
 * state-machine actions summed over lanes, [11] action executions per wave;
 * wave clocks (s_memtime, summed over waves): [12] in traversal, [13] in the
 * state advance, [14] whole persistent loop; [15] exact slab fallbacks;
 * traversal-stack depth probes (after each 4-wide node): [16] entries held
 * beyond depth 8, [17] beyond 12, [18] beyond 16; [19] stack entries culled on pop;
 * wave clocks per state-machine step (megakernel): [20] query resolve, [21] eye start,
 * [22] eye vertex, [23] emitter sample, [24] light start, [25] next-event estimation,
 * [26] light vertex + camera connection, [27] vertex connections, [28] BSDF continuation,
 * [29] light-walk loop test, [30] eye-walk loop test, [31] sample finish. */
typedef struct {
    double kernel_ms;      /* HIP-event time of the render kernel(s) of the last call */
    int64_t samples;       /* camera samples rendered by the last call */
    int64_t launches;      /* kernel launches of the last call */
    int64_t counters[BDPT_NUM_COUNTERS];
    int64_t capped_samples; /* Russian roulette: samples of the last call that met a bound the reference
                               does not have - more than max(255, rr_depth - 1) stored light vertices, or
                               2^25 bounces in one subpath (> 0 means the frame is not the reference's,
                               and bdpt_render_host fails) */
    double span_ms;         /* BDPT frame kernel, device clock: first wave start -> last wave exit */
    double tail_ms;         /* BDPT frame kernel, device clock: the frame's last 64-sample chunk claimed ->
                               last wave exit (the end tail a persistent grid pays per launch) */
    int64_t max_light_depth; /* counting pass (BDPT_FLAG_COUNT) maxima over the samples: light-subpath */
    int64_t max_eye_depth;   /* depth, eye-subpath depth, */
    int64_t max_queries;     /* ray queries of one sample */
    int64_t schedule_errors; /* MT19937 draws past the generated ring (or a ring left by another sample), a
                                continuation walk out of stack
                                (any non-zero count is a bug, and bdpt_render_host fails) */
    int64_t sched[4];        /* counting pass (BDPT_FLAG_COUNT), the connection tasks a wave holds when it
                                shades (connectVertices still to run, connectToLight + the connections of a
                                new eye vertex, connectToCamera of a new light vertex): summed over the
                                shading steps, the shading steps, steps with >= 32 and with >= 64 tasks.
                                Builds whose waiting lanes walk the shadow rays (BDPT_HELP): tasks pushed,
                                pushes refused (ring full), claim rounds, tasks claimed */
    int64_t parked_samples;  /* Russian roulette: walks handed to the continuation pass's chain kernel
                                (deeper than BDPT_PARK_DEPTH bounces; a sample may be handed over again) */
    int64_t rr_long_walks_max;  /* Russian roulette: the most subpaths deeper than 512 bounces one wave held
                                   at once (such a wave stops refilling: express mode) */
    int64_t rr_express_iters[3]; /* Russian roulette: loop iterations of express-mode waves holding 1, 2..4,
                                    more than 4 such subpaths (up to 4 are walked in turn by the whole wave) */
} bdpt_stats;

const char* bdpt_last_error(void);
const char* bdpt_version(void);

/* ---- host-side scene ingest (no GPU needed) ---- */
int bdpt_scene_load_obj(const char* obj_path, bdpt_scene** out);
int bdpt_scene_free(bdpt_scene* scene);
int bdpt_scene_get_info(const bdpt_scene* scene, bdpt_scene_info* out);
/* (new) The scene's emitters in Scene::emitters order: index i is what selectEmitter draws, what
 * BDPT_SAMPLING_EMITTER returns and what bdpt_render_light_groups' group_of_emitter is indexed by.
 * shape: the emitting shape's id; material: the material of its first face (the one whose Ke makes
 * it an emitter), an index into the MTL's materials in file order; area: the sum of its faces'
 * areas; radiance: that material's Ke. BDPT_ERR_INVALID: index outside [0, count). */
typedef struct bdpt_emitter_info {
    int32_t shape, material;
    float area;
    float radiance[3];
} bdpt_emitter_info;
int bdpt_scene_emitter_count(const bdpt_scene* scene, int32_t* count);
int bdpt_scene_get_emitter(const bdpt_scene* scene, int32_t index, bdpt_emitter_info* out);
/* Reference-layout export (tests): tri_f32[ntri][18] = v0 v1 v2 n0 n1 n2 in BVH
 * leaf order, tri_i32[ntri][3] = shapeID primID matID, node_f32[nnodes][6] =
 * bbox min/max, node_u32[nnodes][3] = start nPrims rightOffset (flat preorder). */
int bdpt_scene_export(const bdpt_scene* scene, float* tri_f32, int32_t* tri_i32, float* node_f32, uint32_t* node_u32);
/* Traversal-tree export (tests; wide_bvh.hpp): wnodes[wide_nodes][32] (8 float4:
 * child lo.x hi.x lo.y hi.y lo.z hi.z link-bits unused), wtri[triangles][12]
 * (v0|ref index bits, e1|ref leaf id bits, e2|0), lbox[bvh_leaves][8] (lo|0 hi|0),
 * root_link. Any pointer may be NULL. */
int bdpt_scene_export_traversal(const bdpt_scene* scene, float* wnodes, float* wtri, float* lbox, uint32_t* root_link);

/* ---- scene hand-over from the caller's in-memory Scene (src/core/core.h:352-358) ----
 * What Scene::load built (renderer.cpp:235-315), as plain arrays: the caller
 * flattens WorldData, its bsdfs, emitters and the AcceleratorBVH it already has
 * (INTEGRATION.md §2 does it from the reference's own types); nothing is
 * re-parsed or rebuilt, and the result is the same bdpt_scene the OBJ path
 * gives for the same file (bit-identical device arrays, bdpt_scene_export_layout). */
typedef struct {
    int32_t illum;             /* tinyobj material_t::illum: 7 diffuse, 3 mirror, 6 glass, 8 mixture, 5 null,
                                  anything else Phong (renderer.cpp:258-271) */
    float kd[3], ks[3], ke[3], tf[3]; /* diffuse, specular, emission, transmittance */
    float ns, ni;              /* shininess, ior */
    float scale, spec_weight;  /* MixtureBSDF / PhongBSDF::scale, ::specularSamplingWeight as constructed
                                  (mixture.h:39-46, phong.h:40-47); unused by the other kinds */
    int32_t has_texture;       /* non-zero: a bitmap texture (diffuse_/specular_texname) — rejected by
                                  bdpt_scene_create; hand such a scene over with bdpt_scene_create_textured */
} bdpt_material_desc;
typedef struct {
    int32_t shape;             /* Emitter::shapeID */
    float area;                /* Emitter::area */
    float radiance[3];         /* Emitter::radiance */
    int32_t ncdf;              /* faceAreaDistribution.cdf.size() (= the shape's faces + 1) */
    const float* cdf;          /* faceAreaDistribution.cdf, normalized */
} bdpt_emitter_desc;
typedef struct {
    float bmin[3], bmax[3];    /* BVHFlatNode::bbox.min / max (externals/bvh.h:102-105) */
    uint32_t start, nprims, right_offset;
} bdpt_bvh_node_desc;
typedef struct {
    int64_t triangles;         /* AcceleratorBVH::objects.size() */
    const float* positions;    /* [triangles][9] v0 v1 v2, shape by shape, faces in mesh.indices order
                                  (the order AcceleratorBVH::build creates its objects, accel.h:115-123) */
    const float* normals;      /* [triangles][9] the corners' normals (attrib.normals[normal_index]) */
    const int32_t* tri_shape;  /* [triangles] shapeID */
    const int32_t* tri_prim;   /* [triangles] primID = faceID / 3 */
    const int32_t* tri_mat;    /* [triangles] mesh.material_ids[primID] */
    int32_t shapes;            /* worldData.shapes.size() */
    int32_t materials;         /* worldData.materials.size() = bsdfs.size() */
    const bdpt_material_desc* material;
    int32_t emitters;          /* Scene::emitters.size() */
    const bdpt_emitter_desc* emitter;
    int64_t bvh_nodes;         /* nodes of BVH::flatTree reachable from the root (preorder) */
    const bdpt_bvh_node_desc* bvh;
    const int32_t* bvh_order;  /* [triangles]: the triangle (index into the arrays above) that
                                  AcceleratorBVH::objects[i] (= BVH::build_prims[i] after the build) is */
} bdpt_scene_desc;
/* Validates the descriptor (order, ranges, the BVH's layout and box nesting) and
 * copies it; the caller's arrays may be freed afterwards. BDPT_ERR_INVALID with a
 * message when it is inconsistent. */
int bdpt_scene_create(const bdpt_scene_desc* desc, bdpt_scene** out);
/* ---- bitmap textures (map_Kd / map_Ks: BitmapTexture3f, core.h:525-588) ----
 * bdpt_scene_load_obj reads them itself (<name>.ppm next to the OBJ; an unreadable file
 * is BDPT_ERR_IO, not the reference's pink texel). A caller that hands its Scene over
 * passes, next to the unchanged bdpt_scene_desc, what its BitmapTexture3f objects hold. */
typedef struct {
    int32_t width, height;     /* Tex::w, Tex::h */
    const float* rgb;          /* Tex::cs: [height][width][3], gamma-expanded and flipped as loaded */
} bdpt_texture_desc;
typedef struct {
    int32_t ntextures;
    const bdpt_texture_desc* texture;
    const int32_t* diffuse_tex;  /* [desc->materials]: the texture behind diffuseReflectance / albedo, -1 = constant */
    const int32_t* specular_tex; /* [desc->materials]: the texture behind specularReflectance, -1 = constant */
    const float* texcoords;      /* [desc->triangles][6]: attrib.texcoords of the corners' texcoord_index, st0 st1 st2 */
} bdpt_scene_textures;
/* bdpt_scene_create with the textures of materials whose has_texture is set. Ranges are
 * checked; nothing the caller supplies is recomputed (scale / spec_weight come from
 * bdpt_material_desc as the constructors left them). textures may be NULL (= bdpt_scene_create). */
int bdpt_scene_create_textured(const bdpt_scene_desc* desc, const bdpt_scene_textures* textures, bdpt_scene** out);
/* The scene's texture arrays as uploaded, for checking that two ingest paths agree:
 * 0 the table the kernels read (per material two int32[4] records — diffuse, specular map:
 *   first texel's index in this table, w, h, 0; index -1 = none — then the pool of float[4]
 *   texels rgb0), 1 the triangles' texture coordinates float[triangles][6] in BVH leaf order
 *   (bdpt_scene_export's order), 2 int32[materials][2] texture index of the diffuse / specular
 *   map (-1 none), 3 int32[textures][3] = w, h, first texel's index in array 0.
 * Same size protocol as bdpt_scene_export_layout; every array is empty for a scene
 * without bitmap textures. info (may be NULL): [0] textures, [1] texels, [2] HBM bytes
 * of arrays 0 and 1. */
#define BDPT_TEXTURE_ARRAYS 4
int bdpt_scene_export_textures(const bdpt_scene* scene, int32_t array, void* dst, int64_t* bytes, int64_t info[3]);
/* The scene's device arrays as uploaded by bdpt_ctx_create (the
 * same transforms: shade records widened with v0 and the triangle's near-cull
 * graze code in the shape word's top byte, mixture records with Ks = 0 as
 * diffuse, emitter faces with their graze code), for
 * checking that two ingest paths agree bit for bit: 0 tri, 1 shade, 2 nodes (the
 * reference's binary tree), 3 wnodes, 4 wtri, 5 lbox, 6 BSDF records, 7 emitter
 * records, 8 emitter faces, 9 emitter CDFs, 10 shape -> emitter, 11 roots / tree
 * sizes (uint32 root_link, wroot_link, wmax_stack, wdepth), 12 the BSDF records
 * as ingested (before the upload's mixture -> diffuse rewrite). *bytes = the
 * array's size; dst may be NULL (size only), else it must hold *bytes on entry. */
#define BDPT_LAYOUT_ARRAYS 13
int bdpt_scene_export_layout(const bdpt_scene* scene, int32_t array, void* dst, int64_t* bytes);
/* (new) The device shade records as a context uploads them: 8 float4 (128 bytes) per triangle in
 * leaf order — array 1 of bdpt_scene_export_layout plus, in the two last vectors, the triangle's
 * reference leaf box (lo, 0) (hi, 0), or in a scene with bitmap textures (texture coordinates in
 * those vectors) the reference leaf's index in the last word. Same size protocol. */
int bdpt_scene_export_shade_records(const bdpt_scene* scene, void* dst, int64_t* bytes);
/* Camera constants: worldToCamera, cameraToWorld, cameraToClip, NDCToScreen
 * (column-major) then invWidth, invHeight, tan(fov/2), aspect, forward.xyz,
 * virtual near-plane distance — 72 floats. */
int bdpt_camera_constants(const bdpt_camera* cam, int32_t width, int32_t height, float out[72]);

/* ---- device ---- */
int bdpt_device_count(int32_t* count);
int bdpt_ctx_create(const bdpt_scene* scene, int32_t hip_device, bdpt_ctx** out);
int bdpt_ctx_destroy(bdpt_ctx* ctx);

/* Renders every (pixel, sample) of the shard and ADDS the result to fb_device
 * (device pointer, width*height*3 floats, pixel-major RGB, row 0 = top): eye
 * estimates acc/spp per pixel plus every light-path camera splat (which may land
 * on rows outside the shard). Asynchronous on `hip_stream` (hipStream_t; NULL =
 * the context's own stream); timing is read with bdpt_get_stats after a sync. */
int bdpt_render(bdpt_ctx* ctx, const bdpt_frame_params* params, float* fb_device, void* hip_stream);
/* Same, with a host framebuffer (copied to the device, accumulated, copied back). Synchronous. */
int bdpt_render_host(bdpt_ctx* ctx, const bdpt_frame_params* params, float* fb_host);
/* ---- Integrator::render(const Ray&, Sampler&): one camera sample ---- */
/* The reference's Sampler (math.h:63-76) is a std::mt19937 plus a stateless
 * uniform_real_distribution<float>. Its state crosses the ABI as libstdc++ streams
 * it (operator<< / operator>> of std::mersenne_twister_engine): the 624 state words
 * _M_x, then the position _M_p (0..624). */
#define BDPT_MT19937_WORDS 625
typedef struct {
    int32_t pixel; /* index into the W*H framebuffer (row-major, row 0 = top) */
    float rgb[3];  /* radiance * misWeight, added as rgb[pixel] += ... (bdpt.h:363-370) */
} bdpt_splat;
/* The state of std::mt19937(seed) after `draws` outputs (host only). */
int bdpt_sampler_state(uint32_t seed, int64_t draws, uint32_t state[BDPT_MT19937_WORDS]);
/* BDPTIntegrator::render(ray, sampler) (bdpt.h:219-241): ray = o.xyz d.xyz min_t max_t;
 * `state` is the caller's sampler, advanced in place exactly as the reference
 * advances it. Returns Li; the camera splats of the sample's light subpath are
 * returned in order in splats[0 .. *nsplats) for the caller to add to its image
 * (at most rr_depth without Russian roulette). If `capacity` is smaller than the
 * count: BDPT_ERR_INVALID, *nsplats = the count, `state` unchanged (call again
 * with a larger list).
 * Any rr_depth in [1, 1024]. Synchronous. */
int bdpt_render_sample_mt(bdpt_ctx* ctx, const bdpt_frame_params* params, const float ray[8],
                          uint32_t state[BDPT_MT19937_WORDS], float Li[3], bdpt_splat* splats, int32_t capacity,
                          int32_t* nsplats);
/* The same with the sampler given as std::mt19937(sampler_seed) after
 * *sampler_draws draws (updated on return); splats are added to fb_host
 * (W*H*3 floats) in order. Synchronous. */
int bdpt_render_sample(bdpt_ctx* ctx, const bdpt_frame_params* params, const float ray[8], uint32_t sampler_seed,
                       int32_t* sampler_draws, float Li[3], float* fb_host);
int bdpt_get_stats(bdpt_ctx* ctx, bdpt_stats* out);
/* (new) The frame-kernel build the context's last bdpt_render launched: "bdpt_frame_kernel",
 * "_split" (rrDepth <= 3: no deferred shading step between the subpaths), "_deep" (rrDepth > 28),
 * "_rr" (Russian roulette), "_rrc" (Russian roulette in a scene with glass: a lone subpath trapped by
 * total internal reflection bounces inline) or "_hbm" (BSDF records in HBM); "" before the first render. For
 * matching profiler records to the kernel that ran. */
const char* bdpt_last_kernel(const bdpt_ctx* ctx);
/* (new) Whether that build carries the Mixture / Phong lobes: 1, or 0 for the build that a scene
 * whose materials are all diffuse, mirror or glass (after the Ks = 0 mixture is run as diffuse)
 * renders with where it would otherwise launch "bdpt_frame_kernel" (same name; the environment
 * variable BDPT_NG_BUILD=0 forces the full build). 1 before the first render. */
int bdpt_last_kernel_glossy(const bdpt_ctx* ctx);
/* Waits for all work queued by this context (on every stream it was given). */
int bdpt_synchronize(bdpt_ctx* ctx);
/* (new) Claim order of the shard's rows for the context's later bdpt_render calls: order[i]
 * is the i-th row claimed (a permutation of the shard's local rows 0..n-1, local row r =
 * image row row_offset + r * row_stride); n = 0 restores top-to-bottom. The reference's
 * offline loop hands rows to its threads in order (parallel_for over rows,
 * renderer.cpp:157, parallelfor.h:25-65); the order changes no sample (each keeps its
 * (pixel, sample) seed) and so no result beyond the float addition order, only which
 * samples run last: a render whose shard has a different row count fails
 * (BDPT_ERR_INVALID). Costly rows first leaves cheap samples in flight when the work runs
 * out, which shortens the persistent grid's end tail (each of N ranks pays it once). */
int bdpt_set_row_order(bdpt_ctx* ctx, const int32_t* order, int32_t n);
/* (new) Per local row of the last BDPT_FLAG_COUNT render's shard, the ray queries its
 * samples issued (a cost estimate for bdpt_set_row_order). Returns BDPT_ERR_INVALID when
 * n differs from that shard's row count. Synchronous. */
int bdpt_get_row_costs(bdpt_ctx* ctx, int64_t* costs, int32_t n);

/* ---- sample windows: progressive, resumable, sample-sharded frames ---- */
/* Of each pixel's spp samples, the samples k = first + i * stride, 0 <= i < count. Valid iff
 * first >= 0, stride >= 1, count >= 0 and (count == 0 or first + (count - 1) * stride < spp);
 * anything else is BDPT_ERR_INVALID with a message naming the field. A window changes which
 * samples run and nothing about a sample: sample k of pixel p keeps its seed seed_base +
 * p * spp + k and its weight 1 / spp of the frame's FULL spp (and the spp == 1 no-jitter rule
 * looks at the full spp). So windows that partition [0, spp) - contiguous batches, or the
 * residues modulo N - add up to the frame the unwindowed entry renders, up to the order of the
 * float additions, exactly as row shards do; they combine with row shards, bdpt_set_row_order
 * (the row count is unchanged) and BDPT_FLAG_COUNT. */
typedef struct {
    int32_t first, stride, count;
} bdpt_sample_window;

/* ---- the reference's path tracer on the same substrate (src/integrators/path.h) ---- */
typedef struct {
    int32_t is_explicit;     /* [renderer] isExplicit (default true): renderExplicit / renderImplicit */
    int32_t max_depth;       /* maxDepth (default -1 = Russian roulette past rr_depth) */
    int32_t rr_depth;        /* rrDepth (default 5) */
    float rr_prob;           /* rrProb (default 0.95) */
    int32_t emitter_samples; /* emitterSamples (default 1) */
    int32_t bsdf_samples;    /* bsdfSamples (default 0) */
} bdpt_path_params;
/* Renders every (pixel, sample) of the shard with PathTracerIntegrator::render
 * and ADDS acc/spp per pixel to fb_device (same framebuffer, camera, seeding and
 * shard conventions as bdpt_render; params->rr_depth / strategy are not used).
 * Asynchronous. bdpt_get_stats().counters: [1] samples that outgrew the
 * 512-level recursion stack (then the call's result is not the reference's;
 * bdpt_render_path_host fails with BDPT_ERR_UNSUPPORTED), [2] / [3] samples
 * that drew more than 227 / 624 random numbers; with BDPT_FLAG_COUNT also
 * [0] closest-hit rays and [7] random numbers drawn. */
int bdpt_render_path(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_path_params* path, float* fb_device,
                     void* hip_stream);
int bdpt_render_path_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_path_params* path,
                          float* fb_host);
/* One PathTracerIntegrator::render(ray, sampler) call (path.h:235-245) with the
 * caller's sampler state (advanced in place, as bdpt_render_sample_mt). Synchronous. */
int bdpt_render_path_sample_mt(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_path_params* path,
                               const float ray[8], uint32_t state[BDPT_MT19937_WORDS], float Li[3]);
/* The same with the sampler given as std::mt19937(sampler_seed) after
 * *sampler_draws draws, updated on return. */
int bdpt_render_path_sample(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_path_params* path,
                            const float ray[8], uint32_t sampler_seed, int32_t* sampler_draws, float Li[3]);

/* ---- the reference's direct-light integrator (src/integrators/direct.h) ---- */
#define BDPT_DIRECT_AREA 1              /* samplingStrategy "area"             renderArea :143-195 */
#define BDPT_DIRECT_SOLID_ANGLE 2       /* "solidAngle"                        renderSolidAngle :244-311 */
#define BDPT_DIRECT_COSINE_HEMISPHERE 3 /* "cosineHemisphere"                  renderCosineHemisphere :198-233 */
#define BDPT_DIRECT_BSDF 4              /* "bsdf"                              renderBSDF :235-264 */
#define BDPT_DIRECT_MIS 5               /* "mis"                               renderMIS :313-447 */
typedef struct {
    int32_t sampling_strategy; /* BDPT_DIRECT_*; 0 = an unknown samplingStrategy string (rejected) */
    int32_t emitter_samples;   /* [renderer] emitterSamples (default 1) */
    int32_t bsdf_samples;      /* bsdfSamples (default 1) */
} bdpt_direct_params;
/* Renders every (pixel, sample) of the shard with DirectIntegrator::render and ADDS
 * acc/spp per pixel to fb_device (conventions of bdpt_render_path). Emitters are the
 * spheres the reference makes of them (center = the shape's vertex mean, radius =
 * AABB max.x - center.x, renderer.cpp:295-304 / :349-358). An unknown strategy fails
 * with BDPT_ERR_INVALID (the reference prints "Error: wrong strategy" and exits,
 * direct.h:460-461). Asynchronous. */
int bdpt_render_direct(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_direct_params* direct,
                       float* fb_device, void* hip_stream);
int bdpt_render_direct_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_direct_params* direct,
                            float* fb_host);
/* One DirectIntegrator::render(ray, sampler) call (direct.h:449-462), as
 * bdpt_render_path_sample_mt / bdpt_render_path_sample. */
int bdpt_render_direct_sample_mt(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_direct_params* direct,
                                 const float ray[8], uint32_t state[BDPT_MT19937_WORDS], float Li[3]);
int bdpt_render_direct_sample(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_direct_params* direct,
                              const float ray[8], uint32_t sampler_seed, int32_t* sampler_draws, float Li[3]);
/* samplingStrategy string -> BDPT_DIRECT_* (0 when unknown). */
int32_t bdpt_direct_strategy(const char* name);

/* (new) The window's samples of every pixel of the shard, ADDED to the framebuffer as the
 * unwindowed entries add theirs. path / direct as in bdpt_multi_render_host: NULL / NULL is
 * bdpt_render's integrator, else at most one is set (bdpt_render_path / bdpt_render_direct).
 * window NULL = the whole range (exactly the unwindowed entry); count == 0 renders nothing and
 * returns BDPT_OK. Every refusal of the unwindowed entries stands (textures + Russian roulette,
 * HBM records + Russian roulette, ...), the device form is asynchronous and the host form
 * synchronous like theirs, and bdpt_stats.samples is the window's sample count. */
int bdpt_render_window(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                       const bdpt_path_params* path, const bdpt_direct_params* direct, float* fb_device,
                       void* hip_stream);
int bdpt_render_window_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                            const bdpt_path_params* path, const bdpt_direct_params* direct, float* fb_host);

/* ---- first-hit feature buffers and a device filter for preview frames ---- */
/* (new) Neither exists in the reference; both are defined by what the frame entries compute.
 * For every pixel of the row shard and every sample k of the window (NULL = all; validation and
 * count == 0 as bdpt_render_window), the primary ray the frame kernels build for sample (p, k) -
 * seed seed_base + p * spp + k, the two jitter draws iff the full spp > 1, min_t 1, max_t 1000 -
 * and its closest hit by the frame kernels' traversal (the interior-box test a frame of this camera
 * uses, accepted iff min_t <= t <= max_t). ADDS, with weight 1 / spp of the full spp, eight floats
 * to aov[pixel][8] (interleaved, width * height * 8 floats), so row shards and windows that
 * partition the frame sum to the full buffers as the framebuffers do:
 *   [0..2] albedo   [3..5] frameNs.n in world space as bdpt_hit.ns (not flipped; an average of unit
 *   vectors, not renormalised)   [6] t   [7] 1 (coverage);   all 0 on a miss.
 * Albedo by this build's material kind (bdpt_bsdf_type): diffuse Kd; mixture and Phong Kd + Ks, each
 * channel clamped to at most 1; mirror, glass and the null BSDF of illum 5 (emitters) (1, 1, 1). With a
 * map_Kd / map_Ks, Kd / Ks is the texel at the hit (BitmapTexture3f::eval, as the textured frames read it).
 * Materials are read from HBM per hit: no material-count limit, and textured scenes with many
 * materials run. rr_depth, strategy and russian_roulette are not read (they do not affect a first
 * hit); flags other than 0 are BDPT_ERR_UNSUPPORTED. bdpt_get_stats afterwards: kernel_ms, samples,
 * launches of this call. Asynchronous on `hip_stream` like bdpt_render; the host form is synchronous. */
int bdpt_render_aov(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                    float* aov_device, void* hip_stream);
int bdpt_render_aov_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                         float* aov_host);

/* (new) Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by the feature buffers.
 * With c = color * norm and a = aov * norm per pixel p: cov = a[7]; if cov > 0, alb = a[0:3] / cov,
 * N = a[3:6] / cov, z = a[6] / cov, else alb = (1, 1, 1), N = 0, z = 0;
 * I_0 = demodulate ? c / max(alb, 1e-3) : c per channel. Iteration i = 0 .. iterations - 1, step s = 2^i:
 *   I_{i+1}(p) = sum_q h(q - p) w(p, q) I_i(q) / sum_q h(q - p) w(p, q),
 *   q = p + s (dx, dy), dx, dy in -2..2, taps outside the image skipped, h the outer product of
 *   [1, 4, 6, 4, 1] / 16, w = w_c w_n w_z w_cov, the centre tap w = 1, and
 *   w_c = exp(-min(|I_i(p) - I_i(q)|^2 / (sigma_color 2^-i)^2, 80)),
 *   w_n = exp(-min(|N_p - N_q|^2 / sigma_normal^2, 80)),
 *   w_z = exp(-min((z_p - z_q)^2 / (sigma_depth max(z_p, 1e-6))^2, 80)),
 *   w_cov = 1 if (cov_p > 0) == (cov_q > 0), else 0.
 * out = I_iterations * (demodulate ? max(alb, 1e-3) : 1); iterations == 0 copies color * norm. No
 * atomics and a fixed summation order (dy outer, dx inner): two runs give the same bits. out
 * (width * height * 3 floats) must not overlap color or aov (BDPT_ERR_INVALID, as is a bad field, named
 * in the message). The context owns the scratch (packed guides and two ping-pong images, 64 bytes per
 * pixel, allocated at first use and grown when needed). bdpt_get_stats afterwards: kernel_ms and
 * launches of this call. Asynchronous on `hip_stream`; the host form is synchronous. */
typedef struct {
    int32_t iterations;      /* 0..8; 0 copies (color * norm) to out */
    float sigma_color, sigma_normal, sigma_depth; /* each > 0 */
    int32_t demodulate;      /* 0 / 1: filter color / max(albedo, 1e-3), multiply back afterwards */
    float norm;              /* multiplies color and aov on load: spp / samples_done for a partial frame, 1 for
                                a full one; > 0 */
} bdpt_denoise_params;
/* Defaults, chosen on the 4-spp HardLight 64 x 64 frame of tests/test_gpu_denoise.py against its
 * 256-spp frame and on nothing else (a grid over iterations 3..5, sigma_color 0.1..4, sigma_normal
 * 0.1..1, sigma_depth 0.002..0.5, both demodulate: mean squared error 0.00190 against the unfiltered
 * frame's 0.00295; still smaller depth sigmas score a little better there only by leaving sloped
 * surfaces unfiltered). */
#define BDPT_DENOISE_ITERATIONS 5
#define BDPT_DENOISE_SIGMA_COLOR 2.0f
#define BDPT_DENOISE_SIGMA_NORMAL 0.3f
#define BDPT_DENOISE_SIGMA_DEPTH 0.02f
#define BDPT_DENOISE_DEMODULATE 1
int bdpt_denoise(bdpt_ctx* ctx, int32_t width, int32_t height, const float* color_dev, const float* aov_dev,
                 float* out_dev, const bdpt_denoise_params* params, void* hip_stream);
int bdpt_denoise_host(bdpt_ctx* ctx, int32_t width, int32_t height, const float* color_host, const float* aov_host,
                      float* out_host, const bdpt_denoise_params* params);

/* (new) The filter for the planes of a split frame (bdpt_render_layers, _light_groups, _strategies,
 * _group_layers, _group_strategies): planes and out_planes are n_planes consecutive width * height * 3
 * planes, aov and params are bdpt_denoise's. The guides alb, N, z, cov and m = max(alb, 1e-3) come from
 * aov * norm exactly as there; for plane j, c_j = plane_j * norm and I^j_0 = demodulate ? c_j / m : c_j.
 *   BDPT_DENOISE_PLANES_OWN: every plane runs bdpt_denoise's recurrence on its own colour: out_planes[j]
 *   has the bits of bdpt_denoise(plane_j, aov, params). guide_color and out_guide must be NULL. One call,
 *   and, for frames of up to 512 x 512 pixels, the guide work of a tap (two of its three loads, two of
 *   its three exp) done once per 4 planes; larger frames run bdpt_denoise's launches plane by plane.
 *   BDPT_DENOISE_PLANES_SHARED: one colour guide G for all planes: guide_color (width * height * 3
 *   floats) if given, else the planes' float32 sum in ascending plane order starting from plane 0's
 *   value (for n_planes <= 64 the bits of bdpt_layers_compose with every bit set). B_0 is formed from G
 *   as bdpt_denoise forms I_0 from color; in iteration i, w(p, q) is bdpt_denoise's weight with I_i := B_i
 *   and B_{i+1} its update, and every plane uses those weights:
 *     I^j_{i+1}(p) = (sum_q hw I^j_i(q)) / (sum_q hw),   hw = (h_y h_x) w(p, q),
 *   taps in bdpt_denoise's order (dy outer, dx inner, outside taps skipped, the centre w = 1), each
 *   product and each sum rounded on its own, the division last. The filter is then linear in the planes:
 *   up to float32 rounding the filtered planes sum to the filtered G, and a relight of the filtered
 *   planes is the filter of the relit planes under the same guide. out_guide (NULL: not wanted)
 *   receives the bits of bdpt_denoise(G, aov, params).
 * Both: out_planes[j] = I^j_iterations * (demodulate ? m : 1); iterations == 0 copies plane * norm, and
 * G * norm to out_guide. No atomics and a fixed order: two runs give the same bits; a plane that is all
 * zero comes out all zero. BDPT_ERR_INVALID, the field named in the message, for bdpt_denoise's own
 * parameter checks, n_planes < 1, n_planes * width * height >= 2^30, another mode, guide_color or
 * out_guide in OWN mode, and out_planes or out_guide overlapping an input or each other. The context
 * owns the scratch, allocated at first use and grown with the frame: 288 bytes per pixel whatever
 * n_planes (packed guides 32, the guide's images B_0 .. B_7 128 - SHARED mode only -, and the ping-pong
 * pair of the 4 planes in flight 2 x 4 x 16). bdpt_get_stats afterwards: kernel_ms and launches of this
 * call. Asynchronous on `hip_stream`; the host form stages the buffers and is synchronous. */
#define BDPT_DENOISE_PLANES_OWN 0
#define BDPT_DENOISE_PLANES_SHARED 1
int bdpt_denoise_planes(bdpt_ctx* ctx, int32_t width, int32_t height, int32_t n_planes, const float* planes_device,
                        const float* aov_device, const float* guide_color_device, int32_t mode,
                        const bdpt_denoise_params* params, float* out_planes_device, float* out_guide_device,
                        void* hip_stream);
int bdpt_denoise_planes_host(bdpt_ctx* ctx, int32_t width, int32_t height, int32_t n_planes, const float* planes_host,
                             const float* aov_host, const float* guide_color_host, int32_t mode,
                             const bdpt_denoise_params* params, float* out_planes_host, float* out_guide_host);

/* ---- per-pixel variance from sample batches, and the filter guided by it ---- */
/* (new) K = n_batches planes of width * height * 3 floats, consecutive, each the frame rendered from its
 * own equal share of the samples (bdpt_render_window with the windows (first + b stride, stride K,
 * count / K), b = 0 .. K - 1, each into a zeroed plane: complete, independent estimates of the whole
 * frame, light-path splats included, in the units the window entries accumulate). Per pixel and
 * channel, float32, every operation rounded on its own (no fma), no atomics:
 *   S = plane_0 + plane_1 + ...          ascending (the bits of bdpt_layers_compose with every bit set)
 *   mu = S / (float)K
 *   Q = d_0 d_0 + d_1 d_1 + ...          ascending, d_b = plane_b - mu
 *   var = Q * c,  c = (float)K / (float)(K - 1) formed on the host in float
 * out_sum (NULL: not wanted) receives S, the frame of the batches' samples; out_var receives var, the
 * estimated variance of S (K^2 times the variance of the batch mean), both width * height * 3 floats.
 * BDPT_ERR_INVALID, the field named in the message: n_batches outside 2..64, n_batches * width *
 * height >= 2^30, NULL planes or out_var, an output overlapping the planes or the other output.
 * bdpt_get_stats afterwards: kernel_ms and launches of this call. Asynchronous on `hip_stream`; the
 * host form stages the buffers and is synchronous. */
int bdpt_batch_moments(bdpt_ctx* ctx, int32_t width, int32_t height, int32_t n_batches, const float* planes_device,
                       float* out_sum_device, float* out_var_device, void* hip_stream);
int bdpt_batch_moments_host(bdpt_ctx* ctx, int32_t width, int32_t height, int32_t n_batches, const float* planes_host,
                            float* out_sum_host, float* out_var_host);

/* (new) bdpt_denoise's a-trous filter with a colour weight normalised by the pixel's variance (as SVGF,
 * Schied et al. 2017, weights its luminance). params is bdpt_denoise's struct; sigma_color is now a
 * number of standard deviations. With c = color * norm, a = aov * norm, v = var * (norm * norm): the
 * guides alb, N, z, cov and m = max(alb, 1e-3) exactly as bdpt_denoise forms them,
 *   I_0 = demodulate ? c / m : c,
 *   U(p) = demodulate ? (v_r / (m_r m_r) + v_g / (m_g m_g)) + v_b / (m_b m_b) : (v_r + v_g) + v_b,
 *   V_0(p) = sum_q k(q - p) U(q) / sum_q k(q - p),  q = p + (dx, dy), dx, dy in -1..1, taps outside the
 *   image skipped, k the outer product of [1, 2, 1] / 4, dy outer and dx inner.
 * Iteration i = 0 .. iterations - 1, step s = 2^i: taps, h, w_n, w_z, w_cov, the centre tap w = 1 and
 * the summation order are bdpt_denoise's, and with hw = (h_y h_x) w(p, q)
 *   w_c = exp(-min(|I_i(p) - I_i(q)|^2 / ((sigma_color sigma_color) V_i(p) + 1e-10), 80))
 *         (no 2^-i narrowing: the variance shrinks by itself; the centre pixel's variance alone, so a
 *         firefly accepts its neighbours and they do not accept it),
 *   I_{i+1}(p) = sum hw I_i(q) / sum hw,
 *   V_{i+1}(p) = sum (hw hw) V_i(q) / ((sum hw) (sum hw)).
 * out = I_iterations * (demodulate ? m : 1); out_var (width * height floats, NULL: not wanted) =
 * V_iterations, the residual variance in the filter's own (demodulated, channel-summed) domain.
 * iterations == 0: out = color * norm and out_var = V_0. No atomics and a fixed order: two runs give the
 * same bits. BDPT_ERR_INVALID, the field named in the message: bdpt_denoise's parameter checks, a NULL
 * var, an output overlapping an input or the other output. The scratch is bdpt_denoise's (64 bytes per
 * pixel: the variance rides in the fourth float of the images). bdpt_get_stats afterwards: kernel_ms
 * and launches of this call. Asynchronous on `hip_stream`; the host form is synchronous. */
/* Defaults for bdpt_denoise_var; sigma_normal, sigma_depth and demodulate are BDPT_DENOISE_*'s. Chosen on
 * the 8-spp, 8-batch HardLight 64 x 64 frame of tests/test_gpu_batch_moments.py against its 256-spp
 * frame and on nothing else (a grid over iterations 3..5 and sigma_color 0.5, 1, 2, 4, 8: mean squared
 * error 0.00072 against the unfiltered sum's 0.00142 and 0.00104 for bdpt_denoise with its defaults on the
 * same frame; the whole grid is in DESIGN.md §7i). */
#define BDPT_DENOISE_VAR_ITERATIONS 3
#define BDPT_DENOISE_VAR_SIGMA_COLOR 4.0f
int bdpt_denoise_var(bdpt_ctx* ctx, int32_t width, int32_t height, const float* color_dev, const float* var_dev,
                     const float* aov_dev, float* out_dev, float* out_var_dev, const bdpt_denoise_params* params,
                     void* hip_stream);
int bdpt_denoise_var_host(bdpt_ctx* ctx, int32_t width, int32_t height, const float* color_host, const float* var_host,
                          const float* aov_host, float* out_host, float* out_var_host, const bdpt_denoise_params* params);

/* ---- path-length layers: one BDPT frame split by bounce count ---- */
/* (new) Not in the reference. Every contribution the BDPT frame kernel forms belongs to a full path
 * camera -> ... -> emitter of k edges (k = 1: the camera ray hits an emitter; k = 2: direct light).
 * bdpt_render_layers renders what bdpt_render_window (path = direct = NULL) renders - the same paths,
 * the same contribution values - but ADDS each contribution to plane min(k - 1, n_layers - 1) of
 * fb_layers, n_layers consecutive width * height * 3 planes, so the last plane collects every longer
 * path and the planes sum to bdpt_render's frame (up to the order of the float additions; with
 * n_layers = 1 the plane is the frame). All four kinds are layered: eye-walk emitter hits,
 * connectToLight, connectVertices and connectToCamera's splats. The longest k a frame holds is
 * 2 rr_depth - 1 for BDPT_STRATEGY_BDPT and rr_depth for PATH_TRACING (both: nothing at rr_depth 1),
 * and max(1, rr_depth) for LIGHT_TRACING.
 * window NULL = the whole frame; row shards and bdpt_set_row_order work as in bdpt_render.
 * BDPT_ERR_INVALID: n_layers outside 1..64, or n_layers * width * height >= 2^30. BDPT_ERR_UNSUPPORTED
 * (the message says "layers"), before any launch: flags != 0, Russian roulette, rr_depth > 28, a scene
 * with bitmap textures, BSDF records in HBM. bdpt_last_kernel afterwards: "bdpt_frame_kernel_layers".
 * Asynchronous on `hip_stream` like bdpt_render; the host form stages the caller's
 * n_layers * width * height * 3 floats as bdpt_render_host stages its frame and is synchronous. */
int bdpt_render_layers(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                       int32_t n_layers, float* fb_layers_device, void* hip_stream);
int bdpt_render_layers_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                            int32_t n_layers, float* fb_layers_host);
/* (new) out[p] = the sum of the planes l with bit l of `mask` set, float32 additions in ascending
 * layer order starting from the lowest plane's value (no atomics: the bits of that sequential sum).
 * Device pointers; out is width * height * 3 floats and must not overlap the planes. BDPT_ERR_INVALID: an empty mask, a bit at or above n_layers, n_layers
 * outside 1..64 or n_layers * width * height >= 2^30. Asynchronous on `hip_stream`. */
int bdpt_layers_compose(bdpt_ctx* ctx, const float* fb_layers_device, int32_t n_layers, int32_t width,
                        int32_t height, uint64_t mask, float* out_device, void* hip_stream);

/* ---- light groups: one BDPT frame split by emitter, and relit without tracing again ---- */
/* (new) Not in the reference. Every contribution the BDPT frame kernel forms ends on one emitter e:
 * the emitter the eye walk hit (s = 0; light tracing: the camera ray's own hit), the one connectToLight
 * sampled (s = 1), or the one the sample's light subpath started on (connectVertices, connectToCamera).
 * bdpt_render_light_groups renders what bdpt_render_window (path = direct = NULL) renders - the same
 * paths, the same contribution values - but ADDS each contribution to plane group_of_emitter[e] of
 * fb_groups, n_groups consecutive width * height * 3 planes; the planes sum to bdpt_render's frame (up
 * to the order of the float additions; with n_groups = 1 the plane is the frame). group_of_emitter is a
 * HOST array of one int32 per emitter (bdpt_scene_emitter_count; copied before the call returns), NULL
 * = the identity, one plane per emitter. Without Russian roulette a contribution is linear in its
 * emitter's radiance and no path or weight depends on a radiance, so the planes recombined with
 * per-group gains (bdpt_light_groups_relight) are the frame of the scene with those emitters' Ke scaled.
 * window NULL = the whole frame; row shards and bdpt_set_row_order work as in bdpt_render.
 * BDPT_ERR_INVALID (the message names the field): n_groups outside 1..64, n_groups * width * height >=
 * 2^30, a map entry outside [0, n_groups), a NULL map with n_groups other than the emitter count.
 * BDPT_ERR_UNSUPPORTED (the message says "light groups"), before any launch: flags != 0, Russian
 * roulette, rr_depth > 28, a scene with bitmap textures, BSDF records in HBM. bdpt_last_kernel
 * afterwards: "bdpt_frame_kernel_groups". Asynchronous on `hip_stream` like bdpt_render; the host form
 * stages the caller's n_groups * width * height * 3 floats and is synchronous. */
int bdpt_render_light_groups(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                             int32_t n_groups, const int32_t* group_of_emitter, float* fb_groups_device,
                             void* hip_stream);
int bdpt_render_light_groups_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                                  int32_t n_groups, const int32_t* group_of_emitter, float* fb_groups_host);
/* (new) out[p][c] = gains[0][c] * plane_0[p][c], then + gains[g][c] * plane_g[p][c] for g = 1 ..
 * n_groups - 1 in ascending order: float32, each product and each sum rounded on its own (no fma), every
 * group multiplied whatever its gain, no atomics - the bits of that loop, the same every run. `gains`
 * is a HOST array of n_groups x 3 floats and travels as a kernel argument (one launch per call);
 * the planes and out are device pointers, out is width * height * 3 floats and must not overlap the
 * planes. BDPT_ERR_INVALID: n_groups outside 1..64, n_groups * width * height >= 2^30, overlap, a gain
 * that is not finite. Asynchronous on `hip_stream`. */
int bdpt_light_groups_relight(bdpt_ctx* ctx, const float* fb_groups_device, int32_t n_groups, int32_t width,
                              int32_t height, const float* gains, float* out_device, void* hip_stream);

/* ---- strategy images: one BDPT frame split by sampling strategy (s, t), weighted or not ---- */
/* (new) Not in the reference. Every contribution the BDPT frame kernel forms joins a light subpath of
 * s vertices to an eye subpath of t vertices, the camera counted (k = s + t - 1 edges): the eye walk
 * hits an emitter (s = 0, t = depth_eye + 1; light tracing's primary emission is (0, 2)),
 * connectToLight (s = 1, t = depth_eye + 1), connectVertices (s = depth_light + 1, t = depth_eye + 1),
 * connectToCamera (s = depth_light + 1, t = 1); both walks start at depth 1. bdpt_render_strategies
 * renders what bdpt_render_window (path = direct = NULL) renders - the same paths and draws - but ADDS
 * each contribution to plane min(s, n_s - 1) * n_t + min(t, n_t) - 1 of fb_planes, n_s * n_t
 * consecutive width * height * 3 planes: the last row and column collect what is longer. Planes (0, 1)
 * and (1, 1) are always empty. bdpt_strategies_shape gives the shape that holds every strategy of an
 * rr_depth without clamping, n_s = max(rr_depth, 1) + 1 and n_t = max(rr_depth, 2) (one shape for the
 * three BDPT_STRATEGY_* values; it needs no context; rr_depth in 1..28).
 * weighting BDPT_STRATEGIES_WEIGHTED: the contributions have bdpt_render's values and the planes sum to
 * its frame (up to the order of the float additions; at shape (1, 1) the plane is the frame).
 * BDPT_STRATEGIES_UNWEIGHTED: no contribution is multiplied by its misWeight (bdpt.h:98, :356, :427,
 * :482), all else the same, so plane (s, t) is that strategy's plain estimator; the t = 1 planes plus
 * plane (0, 2) then sum to the frame of the reference's LIGHT_TRACING build. Under
 * BDPT_STRATEGY_LIGHT_TRACING / PATH_TRACING the reference weights nothing and both settings agree.
 * window NULL = the whole frame; row shards and bdpt_set_row_order work as in bdpt_render.
 * BDPT_ERR_INVALID (the message names the field): n_s outside 1..29, n_t outside 1..28, a weighting
 * other than the two, n_s * n_t * width * height >= 2^30. BDPT_ERR_UNSUPPORTED (the message says
 * "strategies"), before any launch: flags != 0, Russian roulette, rr_depth > 28, a scene with bitmap
 * textures, BSDF records in HBM. bdpt_last_kernel afterwards: "bdpt_frame_kernel_strat" or
 * "bdpt_frame_kernel_strat_unweighted". Asynchronous on `hip_stream` like bdpt_render; the host form
 * stages the caller's n_s * n_t * width * height * 3 floats and is synchronous. */
#define BDPT_STRATEGIES_WEIGHTED 0
#define BDPT_STRATEGIES_UNWEIGHTED 1
int bdpt_render_strategies(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                           int32_t n_s, int32_t n_t, int32_t weighting, float* fb_planes_device, void* hip_stream);
int bdpt_render_strategies_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                                int32_t n_s, int32_t n_t, int32_t weighting, float* fb_planes_host);
int bdpt_strategies_shape(int32_t rr_depth, int32_t strategy, int32_t* n_s, int32_t* n_t);
/* (new) The contact sheet of the planes: out is one image of n_s * width by n_t * height pixels (x 3
 * floats, rows of n_s * width pixels), the tile of (s, t) at tile column s and tile row t - 1, each
 * float multiplied by gains[s * n_t + t - 1][channel] (one float32 product; gains NULL: copied). No
 * atomics: the bits of that loop, the same every run. `gains` is a HOST array of n_s * n_t x 3 floats
 * (copied before the call returns); planes and out are device pointers. BDPT_ERR_INVALID: n_s outside
 * 1..29, n_t outside 1..28, a sheet of 2^31 floats or more, out overlapping the planes, a gain that is
 * not finite. Asynchronous on `hip_stream`; the host form stages both arrays and is synchronous. */
int bdpt_strategies_sheet(bdpt_ctx* ctx, const float* planes_device, int32_t n_s, int32_t n_t, int32_t width,
                          int32_t height, const float* gains, float* out_device, void* hip_stream);
int bdpt_strategies_sheet_host(bdpt_ctx* ctx, const float* planes_host, int32_t n_s, int32_t n_t, int32_t width,
                               int32_t height, const float* gains, float* out_host);

/* ---- crossed planes: light groups x path-length layers, light groups x strategies ---- */
/* (new) Not in the reference. One BDPT frame split along two of the axes above at once: a plane per
 * (group, layer) or per (group, s, t). The group and layer planes of two renders are two marginals of
 * the same contributions; these entries keep the joint, so one traced frame can be relit per lamp AND
 * per bounce count (a lamp's indirect light only), or show which strategy carries which lamp's light.
 * fb_planes is n_groups * n_inner consecutive width * height * 3 planes, the group the outer axis:
 * plane g * n_inner + inner with n_inner = n_layers and inner as bdpt_render_layers files it, or
 * n_inner = n_s * n_t and inner as bdpt_render_strategies files it (same clamps, same weighting).
 * Summed over the inner axis the planes are bdpt_render_light_groups', summed over the groups the
 * single-kind entry's (up to the order of the float additions). group_of_emitter as in
 * bdpt_render_light_groups: a HOST array of one int32 per emitter, copied before the call returns,
 * NULL = the identity. window NULL = the whole frame; row shards and bdpt_set_row_order as in bdpt_render.
 * BDPT_ERR_INVALID (the message names the field): n_groups outside 1..64, n_layers outside 1..64, n_s
 * outside 1..29, n_t outside 1..28, a weighting other than the two, n_groups * n_inner * width * height
 * >= 2^30, a map entry outside [0, n_groups), a NULL map with n_groups other than the emitter count.
 * BDPT_ERR_UNSUPPORTED (the message says "light groups x layers" / "light groups x strategies"),
 * before any launch: flags != 0, Russian roulette, rr_depth > 28, a scene with bitmap textures, BSDF
 * records in HBM. bdpt_last_kernel afterwards: "bdpt_frame_kernel_groups_layers",
 * "bdpt_frame_kernel_groups_strat" or "bdpt_frame_kernel_groups_strat_unweighted". Asynchronous on
 * `hip_stream` like bdpt_render; the host forms stage the caller's planes and are synchronous. */
int bdpt_render_group_layers(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                             const int32_t* group_of_emitter, int32_t n_groups, int32_t n_layers,
                             float* fb_planes_device, void* hip_stream);
int bdpt_render_group_layers_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                                  const int32_t* group_of_emitter, int32_t n_groups, int32_t n_layers,
                                  float* fb_planes_host);
int bdpt_render_group_strategies(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                                 const int32_t* group_of_emitter, int32_t n_groups, int32_t n_s, int32_t n_t,
                                 int32_t weighting, float* fb_planes_device, void* hip_stream);
int bdpt_render_group_strategies_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                                      const int32_t* group_of_emitter, int32_t n_groups, int32_t n_s, int32_t n_t,
                                      int32_t weighting, float* fb_planes_host);
/* (new) The two-axis form of bdpt_light_groups_relight and bdpt_layers_compose. With acc the first
 * term, for g ascending and within it j ascending:
 *   t = weights[j] * plane[g * n_inner + j][p][c];  t = gains[g][c] * t;  acc = acc + t
 * float32, each operation rounded on its own (no fma), every plane multiplied whatever its gain or
 * weight, no atomics - the bits of that loop, the same every run. `gains` is a HOST array of
 * n_groups x 3 floats (NULL: ones) and travels as a kernel argument; `weights` is a HOST array of n_inner
 * floats (NULL: ones), copied before the call returns into a table the context owns. The planes and out
 * are device pointers, out is width * height * 3 floats and must not overlap the planes.
 * BDPT_ERR_INVALID: n_groups outside 1..64, n_inner outside 1..812 (29 * 28), n_groups * n_inner *
 * width * height >= 2^30, overlap, a gain or weight that is not finite. Asynchronous on `hip_stream`;
 * the host form stages both arrays and is synchronous. */
int bdpt_group_planes_combine(bdpt_ctx* ctx, const float* planes_device, int32_t n_groups, int32_t n_inner,
                              int32_t width, int32_t height, const float* gains, const float* weights,
                              float* out_device, void* hip_stream);
int bdpt_group_planes_combine_host(bdpt_ctx* ctx, const float* planes_host, int32_t n_groups, int32_t n_inner,
                                   int32_t width, int32_t height, const float* gains, const float* weights,
                                   float* out_host);

/* ---- adaptive sampling: a pixel-list frame kernel, its state kernels and the driver ---- */
/* (new) Not in the reference. bdpt_render_pixels renders, for each of the n_pixels pixels of a list, the
 * window's samples k = first + i * stride of that pixel, with the seed seed_base + pixel * spp + k and
 * the 1 / spp weight of the frame's full spp: the very samples bdpt_render_window renders for those
 * pixels. fb is TWO consecutive width * height * 3 planes, ADDED to and never zeroed (so passes
 * accumulate): plane 0 takes the camera splats of the samples' light paths (t = 1: they land on any
 * pixel of the image), plane 1 everything formed at the sample's own pixel (t >= 2) - the planes of
 * bdpt_render_strategies at shape (1, 2). Plane 1 stays untouched at every unlisted pixel. With the
 * list 0 .. width * height - 1 the two planes are bdpt_render_strategies(1, 2)'s.
 * The list: entries in [0, width * height), strictly ascending (so n_pixels <= width * height). The host
 * form checks that (BDPT_ERR_INVALID, the entry named). The DEVICE form trusts it: an index outside the
 * image would send the kernel's atomic adds outside the framebuffer, so pass it only a list that
 * bdpt_adaptive_select wrote or that was checked as the host form checks. n_pixels == 0 or an empty
 * window launches nothing.
 * BDPT_ERR_INVALID: a bad window, n_pixels outside [0, width * height], a NULL list with n_pixels > 0,
 * row_offset != 0 or row_stride != 1, a row order set on the context (bdpt_set_row_order), 2 * width *
 * height >= 2^30. BDPT_ERR_UNSUPPORTED (the message says "pixel lists"), before any launch: what
 * bdpt_render_strategies refuses. bdpt_last_kernel afterwards: "bdpt_frame_kernel_pixels";
 * bdpt_get_stats().samples = n_pixels * count. Asynchronous on `hip_stream`; the host form stages the
 * list and the two planes and is synchronous. */
int bdpt_render_pixels(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                       const int32_t* pixels_device, int32_t n_pixels, float* fb_device, void* hip_stream);
int bdpt_render_pixels_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_sample_window* window,
                            const int32_t* pixels_host, int32_t n_pixels, float* fb_host);

/* (new) The frame and its variance from K = n_batches accumulated plane pairs. planes: K consecutive
 * pairs as bdpt_render_pixels accumulates them, pair b = (T_b splats, E_b eye), each width * height * 3
 * floats. samples_per_batch: int32 m[p] per pixel, the samples of each batch pixel p has had. With
 * M = sum m and the splat scale t = (float)((double)spp * width * height / ((double)K * M)) formed on the
 * host (0 when M == 0), per pixel and channel in float32, every operation rounded on its own:
 *   a = m[p] > 0 ? (float)spp / (float)(K * m[p]) : 0           one IEEE division
 *   plane_b = E_b * a + T_b * t
 * and on those K planes exactly bdpt_batch_moments: out_sum = S, out_var = the variance of S. The eye
 * part of a pixel is a mean over its own samples and the splat part a mean over all M * K light paths
 * of the frame, which is why the two are kept apart. With m = spp / K everywhere both scales are 1 and
 * the outputs have the bits of bdpt_batch_moments on E_b + T_b. No atomics: the same bits every run.
 * splat_total: M as the caller counted it (the driver knows it from its passes); < 0: counted here on
 * the host from samples_per_batch (host form only; the device form needs it >= 0).
 * BDPT_ERR_INVALID, the field named: n_batches outside 2..64, spp < 1, 2 * n_batches * width * height
 * >= 2^30, a NULL pointer. Asynchronous on `hip_stream`; the host form is synchronous. */
int bdpt_adaptive_resolve(bdpt_ctx* ctx, int32_t width, int32_t height, int32_t n_batches, int32_t spp,
                          const float* planes_device, const int32_t* samples_per_batch_device, int64_t splat_total,
                          float* out_sum_device, float* out_var_device, void* hip_stream);
int bdpt_adaptive_resolve_host(bdpt_ctx* ctx, int32_t width, int32_t height, int32_t n_batches, int32_t spp,
                               const float* planes_host, const int32_t* samples_per_batch_host, int64_t splat_total,
                               float* out_sum_host, float* out_var_host);

/* (new) The pixels that get `step` more samples per batch. Per pixel p, float32 in this order:
 *   noisy(p)  = (var_r + var_g + var_b) > (threshold * threshold) * ((S_r + S_g + S_b + eps) * (S_r + S_g + S_b + eps))
 *               (a relative standard deviation against the threshold, without the square root)
 *   wanted(p) = dilate ? noisy(q) for any q of p's 3 x 3 neighbourhood clipped to the image : noisy(p)
 *   active(p) = wanted(p) && m[p] + step <= m_max
 * out_list (room for width * height int32) receives the active pixel indices in ASCENDING order,
 * *out_count their number, and m[p] += step for exactly those pixels. An ordered compaction without
 * atomics: the same list every run. The device form writes out_count on the device (one int32).
 * BDPT_ERR_INVALID, the field named: a threshold or eps that is negative or not finite, step < 1,
 * m_max < 0, dilate outside {0, 1}, width * height >= 2^30, a NULL pointer. */
int bdpt_adaptive_select(bdpt_ctx* ctx, int32_t width, int32_t height, const float* sum_device, const float* var_device,
                         float threshold, float eps, int32_t step, int32_t m_max, int32_t dilate,
                         int32_t* samples_per_batch_device, int32_t* out_list_device, int32_t* out_count_device,
                         void* hip_stream);
int bdpt_adaptive_select_host(bdpt_ctx* ctx, int32_t width, int32_t height, const float* sum_host, const float* var_host,
                              float threshold, float eps, int32_t step, int32_t m_max, int32_t dilate,
                              int32_t* samples_per_batch_host, int32_t* out_list_host, int32_t* out_count_host);

/* (new) The driver. The frame's budget is params->spp = max_passes * step * n_batches samples per
 * pixel (anything else is BDPT_ERR_INVALID). Pass j renders, for every pixel of its list and every
 * batch b, the window (first = j * step * K + b, stride K, count step) with bdpt_render_pixels into
 * batch b's plane pair: K launches. Pass 0 lists every pixel. After a pass: bdpt_adaptive_resolve, then
 * bdpt_adaptive_select with m_max = max_passes * step; the count comes to the host (one 4-byte read per
 * pass), which stops on an empty list or at the budget and runs a last resolve. A pixel that skips a
 * pass skips those sample indices; samples are independent by seed, and a run in which every pixel
 * stays active renders exactly the samples of bdpt_render. Choosing a pixel's samples from the estimate
 * they feed biases it, as in every adaptive sampler of this kind; threshold = 0 (every pixel with any
 * variance stays active) is the unbiased frame.
 * frame, variance: width * height * 3 floats each, overwritten; samples: width * height int32, the
 * samples each pixel has had (K * m). stats (NULL: not wanted): filled when the call returns.
 * record_passes != 0 keeps every pass's list on the host for bdpt_adaptive_pass_lists.
 * BDPT_ERR_INVALID, the field named: n_batches outside 2..64, step < 1, max_passes outside
 * 1..BDPT_ADAPTIVE_MAX_PASSES, spp != max_passes * step * n_batches, a threshold or eps that is negative
 * or not finite, dilate outside {0, 1}; then what bdpt_render_pixels refuses. The device form takes
 * device pointers and returns once the last resolve is enqueued on `hip_stream` (it has waited for each
 * pass's count before); the host form is synchronous. */
#define BDPT_ADAPTIVE_MAX_PASSES 64
typedef struct {
    int32_t n_batches;     /* K */
    int32_t step;          /* c: samples per batch a pass adds to an active pixel */
    int32_t max_passes;
    float threshold;       /* relative standard deviation below which a pixel is settled */
    float eps;             /* floor added to the channel sum of S */
    int32_t dilate;        /* 1: a noisy pixel keeps its 3 x 3 neighbourhood active */
    int32_t record_passes; /* 1: keep the passes' lists for bdpt_adaptive_pass_lists */
} bdpt_adaptive_params;
typedef struct {
    int32_t passes;        /* passes rendered */
    int32_t reserved;
    int64_t samples;       /* camera samples traced: K * step * the sum of active[] */
    int32_t active[BDPT_ADAPTIVE_MAX_PASSES]; /* pixels listed in pass j (0 beyond `passes`) */
} bdpt_adaptive_stats;
int bdpt_render_adaptive(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_adaptive_params* adaptive,
                         float* frame_device, float* variance_device, int32_t* samples_device,
                         bdpt_adaptive_stats* stats, void* hip_stream);
int bdpt_render_adaptive_host(bdpt_ctx* ctx, const bdpt_frame_params* params, const bdpt_adaptive_params* adaptive,
                              float* frame_host, float* variance_host, int32_t* samples_host,
                              bdpt_adaptive_stats* stats);
/* The lists of the last bdpt_render_adaptive with record_passes, one after the other (pass j has
 * stats.active[j] entries). *total receives their length; out (NULL: only the length is wanted) must
 * hold `capacity` >= *total entries (BDPT_ERR_INVALID otherwise). */
int bdpt_adaptive_pass_lists(bdpt_ctx* ctx, int32_t* out, int64_t capacity, int64_t* total);

/* ---- temporal accumulation: the preview's history reprojected across camera moves ---- */
/* (new) Not in the reference. Takes the history carried from the previous camera, the current frame's
 * colour and feature buffers (bdpt_render_aov of the same camera and samples) and the two cameras; gives
 * the accumulated frame and the new history. Scenes are static: a pixel's first hit is looked up where the
 * previous camera saw it. Integrator-agnostic: any colour + aov pair of `cur`'s camera and size.
 *
 * History state: hist is width * height * 8 floats, interleaved per pixel, [I_r, I_g, I_b, n, N_x, N_y, N_z,
 * z]: I the accumulated colour in the filter's domain (demodulated when `demodulate` is set), n the sample
 * count behind it, N and z the pixel's first-hit normal and depth, z = 0 marking a miss. Two 16-byte vectors
 * per pixel; documented, not opaque: a caller may save and reload it. A history is only meaningful with the
 * `demodulate` it was made with.
 *
 * With c = color * norm and a = aov * norm, the guides cov, alb, N, z and m = max(alb, 1e-3) exactly as
 * bdpt_denoise forms them, and I_cur = demodulate ? c / m : c. Float32, every operation rounded on its own
 * (no fma), only + - * /, sqrt, floor, min / max and comparisons; no atomics: two runs give the same bits.
 * Per pixel p = (row i, column j) of the current frame:
 *  1. Miss (cov <= 0): out_color = c, hist_out = [c, n_c, 0, 0, 0, 0].
 *  2. World point X = eye_cur + z * d_p, each component one product then one sum. d_p is the primary ray
 *     direction the frame kernels build for pixel p at spp = 1 (the pixel centre, no jitter draws: the device
 *     function BDPT_SAMPLING_CAMERA pins). eye_cur, eye_prev: the translation of the camera's cameraToWorld
 *     (floats 28..30 of bdpt_camera_constants), so the constants alone state the operation.
 *  3. Into the previous camera, with bdpt_camera_constants(prev_camera, width, height): Xc = worldToCamera_prev
 *     (X, 1), each component ((m0 x + m1 y) + m2 z) + m3 along a matrix row. No history unless -Xc.z >= 1 (the
 *     near plane of the primary rays). u = Xc.x / (-Xc.z * (tan_prev * aspect_prev)), v = Xc.y / (-Xc.z *
 *     tan_prev), fx = ((u + 1) * 0.5) * width - 0.5, fy = ((1 - v) * 0.5) * height - 0.5 (the inverse of the
 *     camera-ray formula). Snap: r = floor(fx + 0.5); if |fx - r| <= 2^-10 then fx = r; the same for fy - a
 *     static camera lands on its own pixel, and history degenerates to plain progressive accumulation.
 *  4. Taps: x0 = floor(fx), ax = fx - x0, likewise y; the bilinear taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
 *     (x0 + 1, y0 + 1) with weights b = (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay; a tap with b == 0 is
 *     skipped. zp = sqrt(|X - eye_prev|^2), the square as (dx dx + dy dy) + dz dz. Tap q is accepted iff it is
 *     inside the image, hist_in[q].z > 0, |hist_in[q].z - zp| <= sigma_depth * zp and |N_p - N_q|^2 <=
 *     sigma_normal * sigma_normal. sw = sum of b over the accepted taps in tap order, starting from 0. No
 *     history if hist_in is NULL, no tap is accepted or sw < min_weight.
 *  5. H = (sum b I_q) / sw per channel, n_h = min((sum b n_q) / sw, max_history), sums in tap order from 0.
 *  6. Clamp (clamp_sigma = k > 0 only): over the in-image 3 x 3 neighbours q of p in the current frame with
 *     cov_q > 0 (p itself counts), dy outer and dx inner: mu = (sum I_cur(q)) / cnt, s2 = (sum (I_cur(q) -
 *     mu)^2) / cnt per channel, sums from 0, sd = sqrt(s2); lo = mu - sd k, hi = mu + sd k;
 *     H = H < lo ? lo : (H > hi ? hi : H). n_h is unchanged.
 *  7. Blend: n_out = n_h + n_c, alpha = n_c / n_out, I_out = H + (I_cur - H) * alpha.
 *  8. out_color = demodulate ? I_out * m : I_out, hist_out = [I_out, n_out, N, z].
 *  A covered pixel without history: out_color = c (the frame's own bits, not (c / m) * m) and hist_out =
 *  [I_cur, n_c, N, z]. So with hist_in NULL, or with a static camera and clamp_sigma 0, the result is the
 *  plain estimator; choosing history by the current estimate (acceptance, clamp) otherwise biases the frame.
 *
 * First-hit reprojection is wrong for what is seen through a mirror or through glass and for caustics that
 * move with the view; only the clamp limits that.
 * BDPT_ERR_INVALID, the field named in the message: a bad field (below); a NULL color, aov, out_color or
 * hist_out; width * height >= 2^28; an output overlapping an input or the other output - so hist_in ==
 * hist_out is refused: callers ping-pong two buffers. Of `cur`, camera, width and height are read. No
 * scratch allocation. bdpt_get_stats afterwards: kernel_ms and launches (1) of this call. Asynchronous on
 * `hip_stream`; the host form stages the buffers and is synchronous. The buffers' 16-byte accesses need
 * aov, hist_in and hist_out 16-byte aligned (any allocation is); otherwise dwords are used, same bits. */
typedef struct {
    bdpt_camera prev_camera;   /* the camera the history was made with */
    float norm;                /* multiplies color and aov on load, as bdpt_denoise_params.norm; > 0 */
    float cur_samples;         /* n_c: samples per pixel behind color * norm; > 0 */
    float max_history;         /* cap on the carried sample count n_h; > 0 */
    float sigma_normal, sigma_depth;  /* tap acceptance, each > 0 */
    float min_weight;          /* least sum of accepted bilinear weights, in (0, 1] */
    float clamp_sigma;         /* k >= 0; 0 = no neighbourhood clamp */
    int32_t demodulate;        /* 0 / 1, as bdpt_denoise */
} bdpt_reproject_params;
/* Defaults. The sigmas are the denoiser's. MAX_HISTORY, MIN_WEIGHT and CLAMP_SIGMA were chosen on the
 * rendered pair of tests/test_gpu_temporal.py (HardLight 40 x 28 at 4 spp, the camera moved sideways by 2 % of
 * the eye-at distance) against camera B's 256-spp frame and on nothing else: a grid over min_weight 0.1 .. 0.75,
 * clamp_sigma 0 .. 3 and both demodulate (mean squared error over the frame 0.000670 against the 4-spp frame's
 * 0.001791; clamp_sigma 0 and 3 score within 0.3 % of 2). One move cannot tell history caps of 4 and more
 * apart, so the cap comes from the same end frame reached in seven moves of 2/7 % (caps 4 .. 64: 16 scores
 * best, 0.000235 against 0.000254 for 32). The whole grid is in DESIGN.md §7k. A recorded choice, not an
 * acceptance number. */
#define BDPT_REPROJECT_SIGMA_NORMAL 0.3f
#define BDPT_REPROJECT_SIGMA_DEPTH 0.02f
#define BDPT_REPROJECT_MAX_HISTORY 16.0f
#define BDPT_REPROJECT_MIN_WEIGHT 0.1f
#define BDPT_REPROJECT_CLAMP_SIGMA 2.0f
#define BDPT_REPROJECT_DEMODULATE 1
int bdpt_reproject(bdpt_ctx* ctx, const bdpt_frame_params* cur, const float* color_device, const float* aov_device,
                   const float* hist_in_device /* NULL: no history */, float* out_color_device, float* hist_out_device,
                   const bdpt_reproject_params* params, void* hip_stream);
int bdpt_reproject_host(bdpt_ctx* ctx, const bdpt_frame_params* cur, const float* color_host, const float* aov_host,
                        const float* hist_in_host, float* out_color_host, float* hist_out_host,
                        const bdpt_reproject_params* params);

/* ---- display output: metered exposure, tone curve, 8-bit encode ---- */
/* (new) The last stage of a preview: a linear float32 frame turned into 8-bit codes on the device. The
 * reference ends its viewer's frame with a linear -> sRGB pass (src/core/renderpass.cpp:397,
 * src/shaders/srgb.fs); exposure metering and the tone curves have no counterpart. Pinned to the formulas
 * below and to their numpy restatements (bdpt_amd.py meter_numpy, display_numpy), bit for bit. Float32,
 * every operation rounded on its own (no fma); only + - * /, comparisons and integer work on the device:
 * no exp, log or pow in any kernel. The counts of the meter are integers added with integer atomics, so
 * any order of the additions gives the same words: two runs give the same bits.
 *
 * Thresholds in place of the transfer curve. Quantising an encoded value to 8 bits, code = round(255 *
 * curve(y)) clamped to 0..255, is a monotone step function of the linear value y, so it is stated by the
 * 255 places where it steps: T_k, k = 1..255, the smallest float32 t with curve(t) >= (k - 0.5) / 255, curve
 * evaluated in double on the host. Then code(y) = #{k : T_k <= y} (numpy: searchsorted(T, y, side="right")),
 * exact for every float32 y, where a float32 pow on the device could differ from the host's by a code at a
 * step. bdpt_display_thresholds needs no device. The curves, on y >= 0:
 *   BDPT_ENCODE_SRGB     IEC 61966-2-1: y <= 0.0031308 ? 12.92 y : 1.055 y^(1/2.4) - 0.055
 *   BDPT_ENCODE_GAMMA22  y^(1/2.2), the inverse of what the texture reader applies to a map (scene.cpp)
 *   BDPT_ENCODE_LINEAR   y
 * Every table is strictly increasing and below 1. BDPT_ERR_INVALID: an unknown encode, a NULL out. */
#define BDPT_ENCODE_SRGB 0
#define BDPT_ENCODE_GAMMA22 1
#define BDPT_ENCODE_LINEAR 2
int bdpt_display_thresholds(int32_t encode, float out[255]);

/* (new) Exposure from a luminance histogram of the frame. color: width * height * 3 floats; aov (NULL: every
 * pixel is a candidate): the frame's feature buffers (bdpt_render_aov, width * height * 8 floats); prev (NULL:
 * none): the 4 output words of an earlier call, for exposure that adapts over a sequence.
 * Per pixel: c = color * norm; Y = (0.212671 r + 0.715160 g) + 0.072169 b (getLuminance's constants,
 * bdpt_path.hpp; two products and a sum, then a product and a sum). The pixel is counted iff it is covered -
 * with aov, cov = aov[7] * norm > 0, as bdpt_denoise forms it - and Y is a positive normal finite float: 16 <=
 * bits(Y) >> 19 < 4080 (a negative Y has the sign bit and lands above). Its bin is bits(Y) >> 19: the 8
 * exponent bits and the top 4 mantissa bits, so 4096 uint32 bins form a piecewise-linear log2 scale of 16
 * steps per stop.
 * Over the frame, T the number of counted pixels: rank_key = (T * key_permille + 999) / 1000 in 64-bit
 * integers; b_key the lowest bin at which the running count (bins ascending, inclusive) reaches rank_key;
 * Y_key the float with bits (b_key << 19) | (1 << 18), the bin's centre; b_white, Y_white likewise from
 * white_permille. e_m = key / Y_key; e = prev[0] + (e_m - prev[0]) * rate when prev is given, prev[0] > 0 and
 * rate < 1, else e_m (at rate 1 the rounded blend would not be e_m itself); w = max(e * Y_white, 1).
 * Output: four 32-bit words on the device, [float e, float w, uint32 T, uint32 b_key | b_white << 16]. With
 * T == 0: [fallback_exposure, fallback_white, 0, 0].
 * Metering sees first-hit coverage only: what a pixel shows through a mirror or glass counts as that
 * pixel's luminance, and an environment seen on a miss is left out when aov is given.
 * BDPT_ERR_INVALID, the field named in the message: a NULL color or out; width * height >= 2^28; norm, key,
 * fallback_exposure or fallback_white not > 0; a permille outside 1..1000; rate outside (0, 1]; out
 * overlapping color, aov or prev. The context owns the 4096-bin histogram (16 KiB, zeroed on the stream each
 * call). bdpt_get_stats afterwards: kernel_ms and launches (2) of this call. Asynchronous on `hip_stream`;
 * the host form stages the buffers, takes prev as 4 host words and returns the words. */
typedef struct {
    float norm;               /* multiplies color and aov on load, as bdpt_denoise_params.norm; > 0 */
    float key;                /* the luminance the key percentile is exposed to; > 0 */
    int32_t key_permille;     /* 1..1000: the percentile (in thousandths) of the counted pixels that is the key */
    int32_t white_permille;   /* 1..1000: the percentile that becomes Reinhard's white point */
    float rate;               /* (0, 1]: the step from prev's exposure towards this frame's; 1 ignores prev */
    float fallback_exposure;  /* e when no pixel is counted; > 0 */
    float fallback_white;     /* w when no pixel is counted; > 0 */
} bdpt_meter_params;
/* Defaults: recorded choices, not acceptance numbers. KEY 0.18 is photographic middle grey; the median as
 * the key and the 99th percentile as white were looked at on the 4-spp HardLight 40 x 28 frame of
 * tests/test_gpu_display.py and the Caustic frame of tools/display_cost.py and on nothing else; RATE 0.25
 * on the three-frame camera move of the same test. */
#define BDPT_METER_KEY 0.18f
#define BDPT_METER_KEY_PERMILLE 500
#define BDPT_METER_WHITE_PERMILLE 990
#define BDPT_METER_RATE 0.25f
#define BDPT_METER_BINS 4096
int bdpt_meter(bdpt_ctx* ctx, int32_t width, int32_t height, const float* color_device, const float* aov_device,
               const uint32_t* prev_device, const bdpt_meter_params* params, uint32_t* out_words_device,
               void* hip_stream);
int bdpt_meter_host(bdpt_ctx* ctx, int32_t width, int32_t height, const float* color_host, const float* aov_host,
                    const uint32_t* prev_host, const bdpt_meter_params* params, uint32_t out_words[4]);
/* The 4096 bin counts of the context's last bdpt_meter / bdpt_meter_host call (waits for it). */
int bdpt_debug_meter_histogram(bdpt_ctx* ctx, uint32_t out[BDPT_METER_BINS]);

/* (new) Float RGB -> 8-bit. color: width * height * 3 floats; meter (NULL: none): bdpt_meter's 4 words on
 * the device, e = word 0 and w = word 1, so metering and display chain with no host round trip; without it
 * e = params.exposure and w = params.white. out: width * height * channels bytes, rows in the framebuffer's
 * order (row 0 = top, as bdpt_save_exr writes them); channels 3, or 4 with alpha = 255.
 * Per channel value v of a pixel:
 *   1. x = (v * norm) * e
 *   2. x = x > 0 ? x : 0            (NaN and -0 become 0)
 *   3. x = x < 65536 ? x : 65536    (+inf becomes 65536)
 *   4. BDPT_TONE_CLAMP:    y = x
 *      BDPT_TONE_REINHARD: y = (x * (1 + x * iw2)) / (1 + x), iw2 = 1 / (w * w) formed on the device
 *      BDPT_TONE_FILMIC:   y = (x * (2.51 x + 0.03)) / (x * (2.43 x + 0.59) + 0.14), in this order: a = 2.51 *
 *                          x; a = a + 0.03; n = x * a; b = 2.43 * x; b = b + 0.59; d = x * b; d = d + 0.14; y = n / d
 *                          (Narkowicz's rational fit of the ACES curve; the constants rounded to float32)
 *   5. code = #{k : T_k <= y}, T the table of params.encode
 * The tone curve is applied per channel, which shifts the hue of saturated colours towards white as they
 * brighten; a luminance-preserving curve is not built. 8 bits with no dither band smooth gradients.
 * BDPT_ERR_INVALID, the field named in the message: a NULL color or out; width * height >= 2^28; norm,
 * exposure or white not > 0 (exposure and white are checked with or without meter); an unknown tone, encode
 * or channels; out overlapping color or meter. bdpt_get_stats afterwards: kernel_ms and launches (1) of this
 * call. Asynchronous on `hip_stream`; the host form stages the buffers (meter: 4 host words) and is
 * synchronous. A lane takes 4 pixels with three 16-byte loads and three dword stores when channels is 3,
 * color is 16-byte and out 4-byte aligned; otherwise pixel by pixel, same bytes. */
#define BDPT_TONE_CLAMP 0
#define BDPT_TONE_REINHARD 1
#define BDPT_TONE_FILMIC 2
typedef struct {
    float norm;        /* multiplies color on load; > 0 */
    float exposure;    /* e without meter words; > 0 */
    float white;       /* w without meter words (Reinhard's white point, in exposed units); > 0 */
    int32_t tone;      /* BDPT_TONE_* */
    int32_t encode;    /* BDPT_ENCODE_* */
    int32_t channels;  /* 3 (RGB) or 4 (RGBA, alpha 255) */
} bdpt_display_params;
int bdpt_display(bdpt_ctx* ctx, int32_t width, int32_t height, const float* color_device,
                 const uint32_t* meter_device, const bdpt_display_params* params, unsigned char* out_device,
                 void* hip_stream);
int bdpt_display_host(bdpt_ctx* ctx, int32_t width, int32_t height, const float* color_host,
                      const uint32_t* meter_host, const bdpt_display_params* params, unsigned char* out_host);

/* ---- several HIP devices in one process ---- */
/* The reference fans the offline loop out over host threads (parallel_for,
 * src/core/parallelfor.h:25-65, renderer.cpp:157); here every device gets one
 * context, one stream and one full-frame buffer. Device i renders the
 * interleaved row shard i, i + N, ... of the image; one RCCL sum-reduce
 * (ncclReduce over communicators from ncclCommInitAll, librccl loaded at first
 * use) brings the frames to devices[0]. A device list naming one device more than
 * once (a single-GPU rehearsal) sums on that device without RCCL. */
#define BDPT_MAX_DEVICES 16
typedef struct bdpt_multi bdpt_multi;
typedef struct {
    int32_t devices;   /* N */
    int32_t rccl;      /* 1: the reduce ran over RCCL */
    double wall_ms;    /* host wall time of the last bdpt_multi_render_host */
    double render_ms;  /* root-device events: start .. every device's render done */
    double reduce_ms;  /* root-device events: the reduce */
    int64_t samples;   /* camera samples over all devices */
    double kernel_ms[BDPT_MAX_DEVICES];      /* per device, HIP events of its render kernel */
    int64_t device_samples[BDPT_MAX_DEVICES];
    int64_t capped_samples;  /* Russian roulette: bdpt_stats.capped_samples summed over the devices; a
                                non-zero sum fails bdpt_multi_render_host as it fails bdpt_render_host */
    int64_t schedule_errors; /* bdpt_stats.schedule_errors summed over the devices; a non-zero sum fails
                                bdpt_multi_render_host (BDPT_ERR_HIP) as it fails bdpt_render_host */
} bdpt_multi_stats;
int bdpt_multi_create(const bdpt_scene* scene, int32_t ndevices, const int32_t* devices, bdpt_multi** out);
int bdpt_multi_destroy(bdpt_multi* multi);
/* The whole image (params->row_offset 0, row_stride 1) over all devices; the frame
 * is ADDED to fb_host (W*H*3 floats) as bdpt_render_host does. path / direct:
 * NULL for BDPT, else the PathTracerIntegrator / DirectIntegrator settings (at most
 * one). Synchronous. */
int bdpt_multi_render_host(bdpt_multi* multi, const bdpt_frame_params* params, const bdpt_path_params* path,
                           const bdpt_direct_params* direct, float* fb_host);
int bdpt_multi_get_stats(bdpt_multi* multi, bdpt_multi_stats* out);
/* (new) How bdpt_multi_render_host splits the frame over the N devices. BDPT_SHARD_ROWS (the
 * default): device i renders rows i, i + N, ... BDPT_SHARD_SAMPLES: device i renders the whole
 * image with the sample window (i, N, ceil((spp - i) / N)) (count 0 when spp <= i: nothing is
 * launched there and its zero frame still joins the reduce). Rows differ in cost, samples of one
 * pixel do not, so sample shards are balanced without a cost model; every device holds a
 * full-frame buffer either way (camera splats land anywhere), so memory and the reduce are the
 * same. Stats and the capped_samples / schedule_errors sums work alike in both modes. */
#define BDPT_SHARD_ROWS 0
#define BDPT_SHARD_SAMPLES 1
int bdpt_multi_set_sharding(bdpt_multi* multi, int32_t mode);

/* ---- the BSDF plugin contract and the path's building blocks, batched on the device ---- */
/* All arrays are host arrays of n elements; directions are in the local shading
 * frame (z = the shading normal) as SurfaceInteraction::wo / wi. Synchronous. */
/* BSDF::eval(i) of material mat[k]: f * cos(wi) (core.h:308). f: n x 3. */
int bdpt_bsdf_eval(bdpt_ctx* ctx, int64_t n, const int32_t* mat, const float* wo, const float* wi, float* f);
/* BSDF::pdf(i): the solid-angle pdf of wi (core.h:309). */
int bdpt_bsdf_pdf(bdpt_ctx* ctx, int64_t n, const int32_t* mat, const float* wo, const float* wi, float* pdf);
/* BSDF::sample(i, u, &pdf) (core.h:310): u = n x 2 samples in [0, 1); returns f * cos
 * (f: n x 3), the sampled wi (n x 3) and *pdf. */
int bdpt_bsdf_sample(bdpt_ctx* ctx, int64_t n, const int32_t* mat, const float* wo, const float* u, float* f,
                     float* wi, float* pdf);
/* BSDF::getType() (core.h:311) of a scene material, and this build's kind
 * (1 diffuse, 2 mirror, 3 glass, 4 mixture, 5 phong, 0 the null BSDF of illum 5). */
int bdpt_bsdf_type(const bdpt_scene* scene, int32_t mat, uint32_t* type, int32_t* kind);
/* What a BDPT connection runs at each of its ends (connectToLight, connectToCamera,
 * connectVertices, bdpt.h:374-483), as the frame kernels compile it. `build` picks the
 * compilation: BDPT_KAT_EXACT the IEEE weight arithmetic of the Russian-roulette and
 * single-sample kernels (bit-exact to the reference's eval / pdf), BDPT_KAT_FAST the default
 * frame kernels' (Phong powers as exp2(n log2 z) on the hardware instructions, 1-ulp
 * reciprocal / square root: the outputs that hold a Phong power differ from the reference
 * by a few ulp, all others are the same bits), BDPT_KAT_NG the build without glossy lobes,
 * which returns BDPT_ERR_UNSUPPORTED unless the scene's material table holds diffuse,
 * mirror and glass records only (the check that picks that frame kernel). Materials that
 * read a bitmap texture are refused as by bdpt_bsdf_eval.
 * bdpt_bsdf_eval_pdfs: out = n x 5 (f[3], fwd, rev) = eval(wi, wo), pdf(wi, wo) and the
 * pdf of the swapped pair, pdf(wo, wi), from one evaluation. A delta material (mirror,
 * glass) gives zeros: connections skip such vertices. */
#define BDPT_KAT_EXACT 0
#define BDPT_KAT_FAST 1
#define BDPT_KAT_NG 2
int bdpt_bsdf_eval_pdfs(bdpt_ctx* ctx, int32_t build, int64_t n, const int32_t* mat, const float* wo,
                        const float* wi, float* out);
/* The world direction v[k] in the shading frame of the unit normal nrm[k], as a connection
 * computes it for evaluating material mat[k] (Frame(n).toLocal(v), core.h:155-157): out = n x 3.
 * For a diffuse material (every material in BDPT_KAT_NG) x and y are left 0, since
 * DiffuseBSDF reads z only. */
int bdpt_bsdf_local_for(bdpt_ctx* ctx, int32_t build, int64_t n, const int32_t* mat, const float* nrm,
                        const float* v, float* out);

/* A closest hit as AcceleratorBVH::intersect fills SurfaceInteraction (accel.h:125-172). */
typedef struct {
    int32_t hit;               /* closest hit accepted (min_t <= t <= max_t) / occluded */
    float t, u, v;             /* t is the search result even when not accepted (accel.h:132) */
    int32_t shape_id, prim_id, mat_id;
    float p[3], ns[3], ng[3];  /* hit point, frameNs.n, frameNg.n */
    float wo[3];               /* frameNs.toLocal(-ray.d) */
    int32_t tri;               /* this build's triangle index (reference BVH leaf order) */
} bdpt_hit;
/* rays: n x 8 (o.xyz d.xyz min_t max_t). occlusion = 0: closest hit (accel.h:125);
 * 1: the any-hit query of visibilityQuery (bvh.h:259-352 with occlusion = true),
 * result in hit only. The traversal is the frame kernels' (culled 4-wide tree,
 * reference-leaf check; origins beyond 100 scene diagonals walk the reference's
 * tree unculled), with the interior-box test a frame would use for the batch's
 * origins: without the ambiguity slack when all lie within 100 scene diagonals
 * and, like the scene box, within 300 diagonals of 0 (the slack-free test's
 * fma planes), with it otherwise. */
int bdpt_intersect(bdpt_ctx* ctx, int64_t n, const float* rays, int32_t occlusion, bdpt_hit* out);
/* The same with the frame kernels' near-cull rule: origin_normals (n x 3) is the
 * normal of the surface each ray leaves (a path vertex's interpolated shading
 * normal, the emitter point's normal), zero for a camera origin; origin_tris
 * (n, may be NULL = all -1) the triangle that surface is (bdpt_hit.tri order),
 * -1 for none. bdpt_intersect (origin_normals NULL) culls no box for lying close
 * to the origin; the frames skip such boxes unless the query leaves its surface
 * at |cos| < 0.02 to the triangle's geometric plane, tested as |dot(d, n_s)| <
 * 0.02 + the triangle's normal-cone margin. */
int bdpt_intersect_from(bdpt_ctx* ctx, int64_t n, const float* rays, const float* origin_normals,
                        const int32_t* origin_tris, int32_t occlusion, bdpt_hit* out);
/* (new) The closest hits of bdpt_intersect_from the way the frame kernels without Russian
 * roulette find them: the walk accepts triangle hits without the reference-leaf
 * check, its winner is checked once against the box in the winner's shade record, and a winner
 * that fails is discarded and the query walked again with the check in the leaf step. The same
 * results as bdpt_intersect_from, bit for bit. rewalked (n, may be NULL): 1 where the query was
 * walked again. With BDPT_DEBUG_KNOBS=1, BDPT_LEAF_RECHECK=1 fails the first check of every hit
 * (here and in the frame kernels), so every hit takes the second walk. */
int bdpt_intersect_deferred(bdpt_ctx* ctx, int64_t n, const float* rays, const float* origin_normals,
                            const int32_t* origin_tris, bdpt_hit* out, int32_t* rewalked);
/* (new) out[0]: the second walks begun, out[1]: the closest hits applied (after the check, inside
 * accel.h:133's range) in the context's last BDPT frame render, counted by a counting pass
 * (BDPT_FLAG_COUNT) of a frame-kernel build with the deferred check; 0 otherwise. */
int bdpt_get_leaf_rewalks(bdpt_ctx* ctx, int64_t out[2]);
/* (new) out[0]: the blocks of a frame-kernel launch (the context's persistent grid), out[1]: the lane
 * slots the context serves at a time (grid x block, before any debugging knob narrows the grid): the
 * feature-buffer kernel runs at most out[1] / 64 blocks and strides over its 8 x 8 tiles beyond that. */
int bdpt_get_grid(const bdpt_ctx* ctx, int64_t out[2]);
/* BDPTIntegrator::splatToImagePlane (bdpt.h:485-496) of points p (n x 3) for the
 * camera and image of params: xy = n x 2 (the reference's int truncation). */
int bdpt_splat_to_image_plane(bdpt_ctx* ctx, const bdpt_frame_params* params, int64_t n, const float* p,
                              int32_t* xy);

/* The sampling side of the path, per function: n elements of host words in (32-bit: floats,
 * ints and raw generator outputs), host words out, through the frame kernels' own device
 * functions. A draw enters as the std::mt19937 output word it is converted from
 * (std::generate_canonical<float, 24>: word / 2^32 in float, moved to the float below 1 where
 * that rounds to 1, i.e. for words >= 0xFFFFFF80). fn, words in -> words out per element:
 *   BDPT_SAMPLING_CANONICAL    word -> Sampler::next() (math.h:70)
 *   BDPT_SAMPLING_HEMISPHERE   u[2] -> Warp::squareToUniformHemisphere (math.h:136-144), d[3]
 *   BDPT_SAMPLING_TRIANGLE     u[2] -> Warp::squareToUniformTriangle (math.h:229-234), uv[2]
 *   BDPT_SAMPLING_SPHERE       u[2] -> Warp::squareToUniformSphere (math.h:119-127), d[3]
 *   BDPT_SAMPLING_SOLID_ANGLE  u[2], p[3], center[3], radius -> sampleSphereBySolidAngle
 *                              (direct.h:111-141): wi[3], pdf
 *   BDPT_SAMPLING_RAY_SPHERE   ray[8] (o d min_t max_t), center[3], radius -> raySphereIntersect's
 *                              result (direct.h:37-69), int
 *   BDPT_SAMPLING_CDF          emitter (int), u -> Distribution1D::sample of that emitter's face
 *                              areas (math.h:107-111), int
 *   BDPT_SAMPLING_EMITTER      4 words -> selectEmitter + sampleEmitterPosition
 *                              (integrator.cpp:46-51, :73-100): id (int), emitter pdf, face (int:
 *                              BDPT_SAMPLING_CDF of word 1), pos[3], n[3], position pdf
 *   BDPT_SAMPLING_CAMERA       pixel (int), 2 words -> the camera ray's direction
 *                              (renderer.cpp:165-195) for the camera, width, height and spp of
 *                              params (the words are read when spp > 1), d[3]
 * params is read by BDPT_SAMPLING_CAMERA only and may be NULL otherwise. build is
 * BDPT_KAT_EXACT (every output has the reference's bits) or BDPT_KAT_FAST (the default frame
 * kernels' weight arithmetic: the position pdf is the 1-ulp reciprocal of the area, all else
 * the same bits). placement picks where BDPT_SAMPLING_CDF and _EMITTER read the emitter faces
 * and CDFs, which are two bodies of code: BDPT_EMITTERS_CTX as the context's frames do,
 * BDPT_EMITTERS_HBM from global memory, BDPT_EMITTERS_LDS from a copy in LDS
 * (BDPT_ERR_UNSUPPORTED when they do not fit the 24 KiB the scene tables may take).
 * *ctx_placement (may be NULL) receives BDPT_EMITTERS_HBM or _LDS: what the context's frames
 * run (LDS when the copy fits and costs no resident block). Synchronous. */
#define BDPT_SAMPLING_CANONICAL 0
#define BDPT_SAMPLING_HEMISPHERE 1
#define BDPT_SAMPLING_TRIANGLE 2
#define BDPT_SAMPLING_SPHERE 3
#define BDPT_SAMPLING_SOLID_ANGLE 4
#define BDPT_SAMPLING_RAY_SPHERE 5
#define BDPT_SAMPLING_CDF 6
#define BDPT_SAMPLING_EMITTER 7
#define BDPT_SAMPLING_CAMERA 8
#define BDPT_EMITTERS_CTX 0
#define BDPT_EMITTERS_HBM 1
#define BDPT_EMITTERS_LDS 2
int bdpt_debug_sampling(bdpt_ctx* ctx, const bdpt_frame_params* params, int32_t build, int32_t fn,
                        int32_t placement, int64_t n, const void* in, void* out, int32_t* ctx_placement);

/* ---- diagnostics ---- */
/* GlassBSDF::FresnelDielectric (glass.h:40-53): in = n x (eta_i, eta_t, cos_i, cos_t). */
int bdpt_debug_fresnel(int32_t device, int64_t n, const float* in, float* out);
/* rayTriangleIntersect (core.h:379-400): rays n x 8, verts n x 9 (v0 v1 v2);
 * out = n x (hit, t, u, v). */
int bdpt_debug_triangle(int32_t device, int64_t n, const float* rays, const float* verts, float* out);
/* The device restatements of glibc's transcendental functions the path uses
 * (std::sinf / cosf / powf in src/core/math.h:125-242, mixture.h:70), element-wise
 * on device `device`: fn 0 sinf(x), 1 cosf(x), 2 powf(x, y), 3 / 4 the sin / cos
 * of the fused sincos the warps call. fn 5-9: the weight arithmetic of the default frame
 * kernels (its BDPT_FAST_WEIGHTS forms on the hardware's 1-ulp instructions): 5 pow_w(x, y)
 * = exp2(y log2 x) (1 for y == 0), 6 rcp_w(x), 7 div_w(x, y) = x * rcp(y), 8 sqrt_w(x),
 * 9 rsqrt_w(x). y is read by fn 2, 5 and 7. Host arrays of n floats; synchronous. */
#define BDPT_MATH_SINF 0
#define BDPT_MATH_COSF 1
#define BDPT_MATH_POWF 2
#define BDPT_MATH_SINCOS_S 3
#define BDPT_MATH_SINCOS_C 4
#define BDPT_MATH_POW_W 5
#define BDPT_MATH_RCP_W 6
#define BDPT_MATH_DIV_W 7
#define BDPT_MATH_SQRT_W 8
#define BDPT_MATH_RSQRT_W 9
int bdpt_debug_math(int32_t device, int32_t fn, const float* x, const float* y, float* out, int64_t n);

/* ---- scene configuration and image output (host only, no GPU needed) ---- */

/* The settings loadTOML (src/main.cpp:22-116) reads from a scene .toml, with its
 * defaults and cpptoml's typed-read rules. obj_file is resolved against the
 * TOML's directory as Scene::load does (renderer.cpp:236-241). */
typedef struct {
    char toml_file[4096];
    char obj_file_raw[4096]; /* [input] objfile as written */
    char obj_file[4096];     /* resolved path */
    bdpt_camera camera;      /* [camera] eye / at / up / fov (defaults 1,1,0 / 0,0,0 / 0,1,0 / 30) */
    int32_t width, height;   /* [film] (defaults 768 x 576) */
    int32_t realtime;        /* [renderer] realtime (default false) */
    char integrator[32];     /* [renderer] type (default "normal") */
    int32_t rr_depth;        /* [renderer] rrDepth (bdpt/path, default 5) */
    float rr_prob;           /* [renderer] rrProb (bdpt default 0; unused: NO_RR, bdpt.h:18) */
    int32_t spp;             /* [renderer] spp (default 1) */
    bdpt_path_params path;   /* type = "path": isExplicit, maxDepth, rrDepth, rrProb, emitterSamples,
                                bsdfSamples (main.cpp:96-101); defaults otherwise */
    bdpt_direct_params direct;       /* type = "direct": emitterSamples, bsdfSamples (main.cpp:88-92) */
    char sampling_strategy[32];      /* type = "direct": samplingStrategy as written (default "emitter") */
} bdpt_config;

/* loadTOML (main.cpp:22-116). BDPT_ERR_INVALID with the parse error otherwise. */
int bdpt_config_load_toml(const char* toml_path, bdpt_config* out);
/* Integrator::save -> saveEXR (integrator.cpp:26-30, utils.h:95-156): the
 * W*H*3 float framebuffer (pixel-major RGB, row 0 = top) as an uncompressed
 * scanline OpenEXR with half-float channels B, G, R — byte-identical to the
 * reference's tinyexr output. bdpt_encode_exr writes into `out` (capacity
 * bytes; out = NULL only reports *size). */
int bdpt_encode_exr(const float* rgb, int32_t width, int32_t height, unsigned char* out, int64_t capacity,
                    int64_t* size);
int bdpt_save_exr(const float* rgb, int32_t width, int32_t height, const char* path);
/* (new) 8-bit image files of bdpt_display's bytes (pixel-major, row 0 = top), host only, no dependency.
 * PNG: channels 3 (colour type 2) or 4 (colour type 6), bit depth 8, every scanline with filter type 0, the
 * data as zlib stored blocks (no compression) of at most 65535 bytes, with the unit's own CRC-32 and
 * Adler-32. bdpt_encode_png as bdpt_encode_exr: out = NULL only reports *size. PPM: "P6\n<width>
 * <height>\n255\n" and the RGB bytes, the header the texture reader of scene.cpp accepts (no comments); 3
 * channels only. BDPT_ERR_INVALID: a NULL argument, width or height < 1, other channels, a capacity below
 * *size; BDPT_ERR_IO: the file cannot be written. */
int bdpt_encode_png(const unsigned char* pixels, int32_t width, int32_t height, int32_t channels, unsigned char* out,
                    int64_t capacity, int64_t* size);
int bdpt_save_png(const unsigned char* pixels, int32_t width, int32_t height, int32_t channels, const char* path);
int bdpt_save_ppm(const unsigned char* rgb, int32_t width, int32_t height, const char* path);

#ifdef __cplusplus
}
#endif
#endif
