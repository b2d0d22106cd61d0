"""Python host binding of the MI355X BDPT library (lib/libbdpt_amd.so).

Mirrors the reference's plugin surface for the BDPT path
(JackMinn/Bidirectional-Path-Tracing):

  Scene(obj_path)                      Scene::load          src/core/renderer.cpp:235-315
  BDPTIntegrator(scene, config)        BDPTIntegrator ctor  src/integrators/bdpt.h:38-43
    .init()                            Integrator::init     src/core/integrator.cpp:16-20 (allocates rgb)
    .render(ray, sampler) -> Li        Integrator::render   bdpt.h:219-241 (one camera sample)
    .render_frame(...)                 Renderer::render offline loop renderer.cpp:130-214
    .render_frame(window=SampleWindow(first, stride, count)) / .render_progressive(batch)
                                       a part of that loop's samples per pixel (bdpt_render_window)
    .rgb                               Integrator::rgb      (W x H x 3 float32, accumulated)
    .render_aov(...) / .aov            first-hit albedo, normal, depth, coverage (bdpt_render_aov; no counterpart)
    .denoise(samples_done=...)         edge-avoiding a-trous filter of a low-spp frame (bdpt_denoise; no counterpart)
    .render_layers(n) / .compose_layers(layers, mask)
                                       the BDPT frame split by path length (bdpt_render_layers; no counterpart)
    .render_light_groups(map, n) / .relight(groups, gains)
                                       the BDPT frame split by emitter and recombined with per-group RGB gains
                                       (bdpt_render_light_groups, bdpt_light_groups_relight; no counterpart)
    .render_strategies(n_s, n_t, unweighted) / .strategies_sheet(planes, gains)
                                       the BDPT frame split by sampling strategy (s, t), with or without the
                                       MIS weights, and its contact sheet (bdpt_render_strategies,
                                       bdpt_strategies_sheet; no counterpart)
    .render_group_layers(n) / .render_group_strategies(n_s, n_t) / .combine_group_planes(planes, gains, weights)
                                       the BDPT frame split by emitter AND by path length or strategy, a plane per
                                       (group, layer) / (group, s, t), recombined with per-group RGB gains and
                                       per-inner-plane weights (bdpt_render_group_layers,
                                       bdpt_render_group_strategies, bdpt_group_planes_combine; no counterpart)
    .denoise_planes(planes, aov, mode, guide)
                                       the filter for the planes of any of those splits, with weights of their own or
                                       one set for all, under which they still add up (bdpt_denoise_planes; no counterpart)
  Sampler(seed)                        Sampler              src/core/math.h:63-76 (seed + draw count)
  Ray(o, d, min_t, max_t)              Ray                  src/core/core.h:117-122
  load_toml(path) -> SceneConfig       loadTOML             src/main.cpp:22-116
  PathTracerIntegrator(scene, config, PathSettings)
                                       PathTracerIntegrator src/integrators/path.h (TOML type = "path")
  save_exr(rgb, W, H, path)            Integrator::save     integrator.cpp:26-30 -> saveEXR utils.h:95-156

Everything renders on the GPU through the C-ABI of include/bdpt_amd.h; there
is no CPU fallback (a missing library or device raises).
"""
from __future__ import annotations

import ctypes
import math
import os
import subprocess
from dataclasses import dataclass, field

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# BDPT_AMD_LIB selects an alternative in-tree build (kernel-variant experiments).
LIB_PATH = os.environ.get("BDPT_AMD_LIB") or os.path.join(HERE, "lib", "libbdpt_amd.so")

STRATEGY_BDPT, STRATEGY_LIGHT_TRACING, STRATEGY_PATH_TRACING = 0, 1, 2
RR_NONE, RR_LUMINANCE = 0, 1  # bdpt_frame_params.russian_roulette (BDPT_RR_*)
FLAG_COUNT, FLAG_FULL_TRAVERSAL = 1, 2
REFERENCE_SEED = 260450963  # renderer.cpp:155
COUNTER_NAMES = ["closest_rays", "shadow_rays", "interior_visits", "tri_tests", "light_verts",
                 "light_vert_reads", "splats", "rng_draws", "trav_lane_iters", "trav_wave_iters",
                 "shade_lane_actions", "shade_wave_actions", "trav_clocks", "shade_clocks", "loop_clocks",
                 "slab_fallbacks", "stack_gt8", "stack_gt12", "stack_gt16", "pop_culled",
                 "clk_resolve", "clk_start_eye", "clk_eye_vertex", "clk_emitter_sample", "clk_start_light",
                 "clk_nee", "clk_light_vertex", "clk_connect", "clk_continue", "clk_light_next", "clk_eye_next",
                 "clk_finish"]


class BdptError(RuntimeError):
    code = 0  # the BDPT_ERR_* status (set by _check)


ERR_INVALID, ERR_IO, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED = -1, -2, -3, -4, -5


class _Camera(ctypes.Structure):
    _fields_ = [("eye", ctypes.c_float * 3), ("at", ctypes.c_float * 3), ("up", ctypes.c_float * 3),
                ("fov", ctypes.c_float)]


class _FrameParams(ctypes.Structure):
    _fields_ = [("camera", _Camera), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("spp", ctypes.c_int32),
                ("rr_depth", ctypes.c_int32), ("strategy", ctypes.c_int32), ("seed_base", ctypes.c_uint32),
                ("row_offset", ctypes.c_int32), ("row_stride", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("russian_roulette", ctypes.c_int32)]


class _SceneInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in
                ("triangles", "bvh_nodes", "shapes", "materials", "emitters", "bvh_max_depth", "device_bytes",
                 "bvh_leaves", "wide_nodes", "wide_depth", "wide_max_stack", "wide_leaves", "triangle_tree")]


class _PathParams(ctypes.Structure):  # bdpt_path_params
    _fields_ = [("is_explicit", ctypes.c_int32), ("max_depth", ctypes.c_int32), ("rr_depth", ctypes.c_int32),
                ("rr_prob", ctypes.c_float), ("emitter_samples", ctypes.c_int32), ("bsdf_samples", ctypes.c_int32)]


class _SampleWindow(ctypes.Structure):  # bdpt_sample_window
    _fields_ = [("first", ctypes.c_int32), ("stride", ctypes.c_int32), ("count", ctypes.c_int32)]


class _DenoiseParams(ctypes.Structure):  # bdpt_denoise_params
    _fields_ = [("iterations", ctypes.c_int32), ("sigma_color", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_depth", ctypes.c_float), ("demodulate", ctypes.c_int32), ("norm", ctypes.c_float)]


class _DirectParams(ctypes.Structure):  # bdpt_direct_params
    _fields_ = [("sampling_strategy", ctypes.c_int32), ("emitter_samples", ctypes.c_int32),
                ("bsdf_samples", ctypes.c_int32)]


class _Config(ctypes.Structure):  # bdpt_config
    _fields_ = [("toml_file", ctypes.c_char * 4096), ("obj_file_raw", ctypes.c_char * 4096),
                ("obj_file", ctypes.c_char * 4096), ("camera", _Camera), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("realtime", ctypes.c_int32), ("integrator", ctypes.c_char * 32),
                ("rr_depth", ctypes.c_int32), ("rr_prob", ctypes.c_float), ("spp", ctypes.c_int32),
                ("path", _PathParams), ("direct", _DirectParams), ("sampling_strategy", ctypes.c_char * 32)]


class _Splat(ctypes.Structure):  # bdpt_splat
    _fields_ = [("pixel", ctypes.c_int32), ("rgb", ctypes.c_float * 3)]


# bdpt_hit (AcceleratorBVH::intersect's SurfaceInteraction fields)
HIT_DTYPE = np.dtype([("hit", np.int32), ("t", np.float32), ("u", np.float32), ("v", np.float32),
                      ("shape_id", np.int32), ("prim_id", np.int32), ("mat_id", np.int32), ("p", np.float32, 3),
                      ("ns", np.float32, 3), ("ng", np.float32, 3), ("wo", np.float32, 3), ("tri", np.int32)])


def _af32(a, cols):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, cols))


def _ai32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))


MAX_DEVICES = 16  # BDPT_MAX_DEVICES


class _MultiStats(ctypes.Structure):  # bdpt_multi_stats
    _fields_ = [("devices", ctypes.c_int32), ("rccl", ctypes.c_int32), ("wall_ms", ctypes.c_double),
                ("render_ms", ctypes.c_double), ("reduce_ms", ctypes.c_double), ("samples", ctypes.c_int64),
                ("kernel_ms", ctypes.c_double * MAX_DEVICES), ("device_samples", ctypes.c_int64 * MAX_DEVICES),
                ("capped_samples", ctypes.c_int64), ("schedule_errors", ctypes.c_int64)]


class _MaterialDesc(ctypes.Structure):  # bdpt_material_desc
    _fields_ = [("illum", ctypes.c_int32), ("kd", ctypes.c_float * 3), ("ks", ctypes.c_float * 3),
                ("ke", ctypes.c_float * 3), ("tf", ctypes.c_float * 3), ("ns", ctypes.c_float), ("ni", ctypes.c_float),
                ("scale", ctypes.c_float), ("spec_weight", ctypes.c_float), ("has_texture", ctypes.c_int32)]


class _EmitterDesc(ctypes.Structure):  # bdpt_emitter_desc
    _fields_ = [("shape", ctypes.c_int32), ("area", ctypes.c_float), ("radiance", ctypes.c_float * 3),
                ("ncdf", ctypes.c_int32), ("cdf", ctypes.c_void_p)]


class _BvhNodeDesc(ctypes.Structure):  # bdpt_bvh_node_desc
    _fields_ = [("bmin", ctypes.c_float * 3), ("bmax", ctypes.c_float * 3), ("start", ctypes.c_uint32),
                ("nprims", ctypes.c_uint32), ("right_offset", ctypes.c_uint32)]


class _SceneDesc(ctypes.Structure):  # bdpt_scene_desc
    _fields_ = [("triangles", ctypes.c_int64), ("positions", ctypes.c_void_p), ("normals", ctypes.c_void_p),
                ("tri_shape", ctypes.c_void_p), ("tri_prim", ctypes.c_void_p), ("tri_mat", ctypes.c_void_p),
                ("shapes", ctypes.c_int32), ("materials", ctypes.c_int32), ("material", ctypes.c_void_p),
                ("emitters", ctypes.c_int32), ("emitter", ctypes.c_void_p), ("bvh_nodes", ctypes.c_int64),
                ("bvh", ctypes.c_void_p), ("bvh_order", ctypes.c_void_p)]


class _TextureDesc(ctypes.Structure):  # bdpt_texture_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("rgb", ctypes.c_void_p)]


class _SceneTextures(ctypes.Structure):  # bdpt_scene_textures
    _fields_ = [("ntextures", ctypes.c_int32), ("texture", ctypes.c_void_p), ("diffuse_tex", ctypes.c_void_p),
                ("specular_tex", ctypes.c_void_p), ("texcoords", ctypes.c_void_p)]


TEXTURE_ARRAYS = ("tex_tab", "tri_st", "mat_tex", "tex_dims")  # bdpt_scene_export_textures ids 0..3

# BsdfKind (bdpt_types.h) -> the MTL illum that selects it (renderer.cpp:258-271)
KIND_ILLUM = {0: 5, 1: 7, 2: 3, 3: 6, 4: 8, 5: 2}
LAYOUT_ARRAYS = ("tri", "shade", "nodes", "wnodes", "wtri", "lbox", "bsdfs", "emitters", "emit_tri", "emit_cdf",
                 "shape_emitter", "roots", "bsdfs_ingested")  # bdpt_scene_export_layout ids 0..12


class _EmitterInfo(ctypes.Structure):
    _fields_ = [("shape", ctypes.c_int32), ("material", ctypes.c_int32), ("area", ctypes.c_float),
                ("radiance", ctypes.c_float * 3)]


@dataclass
class SceneDesc:
    """bdpt_scene_desc as numpy arrays: the Scene a caller already holds in memory
    (core.h:352-358) - triangles in (shape, face) order, materials with their
    constructed constants, emitters with their CDFs, the flat Fast-BVH and the
    BVH's object order."""
    positions: np.ndarray   # float32 (n, 9)
    normals: np.ndarray     # float32 (n, 9)
    tri_shape: np.ndarray   # int32 (n,)
    tri_prim: np.ndarray
    tri_mat: np.ndarray
    shapes: int
    materials: list         # dicts: illum kd ks ke tf ns ni scale spec_weight has_texture
    emitters: list          # dicts: shape area radiance cdf
    bvh: np.ndarray         # structured (bmin f4[3], bmax f4[3], start u4, nprims u4, right_offset u4)
    bvh_order: np.ndarray   # int32 (n,)
    # bitmap textures (bdpt_scene_textures; all None = an untextured scene, bdpt_scene_create)
    textures: list | None = None         # float32 (h, w, 3) arrays: Tex::cs, expanded and flipped
    diffuse_tex: np.ndarray | None = None   # int32 (materials,): texture of the diffuse map, -1 none
    specular_tex: np.ndarray | None = None  # int32 (materials,)
    texcoords: np.ndarray | None = None     # float32 (n, 6): st0 st1 st2 per triangle


BVH_NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("start", "<u4"), ("nprims", "<u4"),
                           ("right_offset", "<u4")])


class _Stats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double), ("samples", ctypes.c_int64), ("launches", ctypes.c_int64),
                ("counters", ctypes.c_int64 * len(COUNTER_NAMES)),  # BDPT_NUM_COUNTERS
                ("capped_samples", ctypes.c_int64), ("span_ms", ctypes.c_double), ("tail_ms", ctypes.c_double),
                ("max_light_depth", ctypes.c_int64), ("max_eye_depth", ctypes.c_int64),
                ("max_queries", ctypes.c_int64), ("schedule_errors", ctypes.c_int64), ("sched", ctypes.c_int64 * 4),
                ("parked_samples", ctypes.c_int64), ("rr_long_walks_max", ctypes.c_int64),
                ("rr_express_iters", ctypes.c_int64 * 3)]


class _AdaptiveParams(ctypes.Structure):  # bdpt_adaptive_params
    _fields_ = [("n_batches", ctypes.c_int32), ("step", ctypes.c_int32), ("max_passes", ctypes.c_int32),
                ("threshold", ctypes.c_float), ("eps", ctypes.c_float), ("dilate", ctypes.c_int32),
                ("record_passes", ctypes.c_int32)]


ADAPTIVE_MAX_PASSES = 64  # BDPT_ADAPTIVE_MAX_PASSES


class _AdaptiveStats(ctypes.Structure):  # bdpt_adaptive_stats
    _fields_ = [("passes", ctypes.c_int32), ("reserved", ctypes.c_int32), ("samples", ctypes.c_int64),
                ("active", ctypes.c_int32 * ADAPTIVE_MAX_PASSES)]


class _ReprojectParams(ctypes.Structure):  # bdpt_reproject_params
    _fields_ = [("prev_camera", _Camera), ("norm", ctypes.c_float), ("cur_samples", ctypes.c_float),
                ("max_history", ctypes.c_float), ("sigma_normal", ctypes.c_float), ("sigma_depth", ctypes.c_float),
                ("min_weight", ctypes.c_float), ("clamp_sigma", ctypes.c_float), ("demodulate", ctypes.c_int32)]


class _MeterParams(ctypes.Structure):  # bdpt_meter_params
    _fields_ = [("norm", ctypes.c_float), ("key", ctypes.c_float), ("key_permille", ctypes.c_int32),
                ("white_permille", ctypes.c_int32), ("rate", ctypes.c_float), ("fallback_exposure", ctypes.c_float),
                ("fallback_white", ctypes.c_float)]


class _DisplayParams(ctypes.Structure):  # bdpt_display_params
    _fields_ = [("norm", ctypes.c_float), ("exposure", ctypes.c_float), ("white", ctypes.c_float),
                ("tone", ctypes.c_int32), ("encode", ctypes.c_int32), ("channels", ctypes.c_int32)]


# Sources that make up the frame kernels' code objects: their hash stamps the
# profiles (PMC passes) so bench.py only reuses a measurement of the same kernel.
KERNEL_SOURCES = ("csrc/bdpt_kernels.hip", "csrc/aov_kernels.hip", "csrc/bdpt_kernels_split.hip", "csrc/bdpt_kernels_ng.hip", "csrc/bdpt_kernels_layers.hip", "csrc/bdpt_kernels_groups.hip", "csrc/bdpt_kernels_strat.hip", "csrc/bdpt_kernels_strat_unweighted.hip", "csrc/bdpt_kernels_pixels.hip", "csrc/adaptive_kernels.hip", "csrc/temporal_kernels.hip", "csrc/display_kernels.hip", "csrc/bdpt_path.hpp", "csrc/bdpt_device.hpp", "csrc/device_math.hpp",
                  "csrc/dev_scene.hpp", "csrc/dev_rng.hpp", "csrc/dev_warp.hpp", "csrc/dev_traverse.hpp", "csrc/dev_shade.hpp", "csrc/dev_emitter.hpp",
                  "csrc/powf_restated.inc", "csrc/bdpt_types.h", "Makefile")


def kernel_build_hash() -> str:
    """sha256[:16] over the frame kernel's sources and build flags."""
    import hashlib

    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        with open(os.path.join(HERE, rel), "rb") as f:
            h.update(rel.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def build(force: bool = False) -> str:
    """Compiles lib/libbdpt_amd.so in-tree with hipcc for gfx950."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", HERE, "-j4"], check=True)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BdptError(f"{LIB_PATH} is missing: run build() (hipcc --offload-arch=gfx950)")
        L = ctypes.CDLL(LIB_PATH)
        vp, i32, f32p = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_float)
        L.bdpt_last_error.restype = ctypes.c_char_p
        L.bdpt_version.restype = ctypes.c_char_p
        L.bdpt_last_kernel.restype = ctypes.c_char_p
        L.bdpt_last_kernel.argtypes = [ctypes.c_void_p]
        L.bdpt_last_kernel_glossy.argtypes = [ctypes.c_void_p]
        L.bdpt_set_row_order.argtypes = [vp, vp, i32]
        L.bdpt_get_row_costs.argtypes = [vp, vp, i32]
        L.bdpt_scene_load_obj.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
        L.bdpt_scene_free.argtypes = [vp]
        L.bdpt_scene_get_info.argtypes = [vp, ctypes.POINTER(_SceneInfo)]
        L.bdpt_scene_export.argtypes = [vp, vp, vp, vp, vp]
        L.bdpt_scene_export_traversal.argtypes = [vp, vp, vp, vp, vp]
        L.bdpt_intersect_from.argtypes = [vp, ctypes.c_int64, vp, vp, vp, i32, vp]
        L.bdpt_intersect_deferred.argtypes = [vp, ctypes.c_int64, vp, vp, vp, vp, vp]
        L.bdpt_get_leaf_rewalks.argtypes = [vp, ctypes.c_int64 * 2]
        L.bdpt_get_grid.argtypes = [vp, ctypes.c_int64 * 2]
        L.bdpt_scene_create.argtypes = [ctypes.POINTER(_SceneDesc), ctypes.POINTER(vp)]
        L.bdpt_scene_export_layout.argtypes = [vp, i32, vp, ctypes.POINTER(ctypes.c_int64)]
        L.bdpt_scene_export_shade_records.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int64)]
        L.bdpt_scene_create_textured.argtypes = [ctypes.POINTER(_SceneDesc), ctypes.POINTER(_SceneTextures),
                                                 ctypes.POINTER(vp)]
        L.bdpt_scene_export_textures.argtypes = [vp, i32, vp, ctypes.POINTER(ctypes.c_int64), vp]
        L.bdpt_camera_constants.argtypes = [ctypes.POINTER(_Camera), i32, i32, f32p]
        L.bdpt_device_count.argtypes = [ctypes.POINTER(i32)]
        L.bdpt_ctx_create.argtypes = [vp, i32, ctypes.POINTER(vp)]
        L.bdpt_ctx_destroy.argtypes = [vp]
        L.bdpt_render.argtypes = [vp, ctypes.POINTER(_FrameParams), vp, vp]
        L.bdpt_render_host.argtypes = [vp, ctypes.POINTER(_FrameParams), vp]
        L.bdpt_render_sample.argtypes = [vp, ctypes.POINTER(_FrameParams), f32p, ctypes.c_uint32,
                                         ctypes.POINTER(i32), f32p, vp]
        L.bdpt_sampler_state.argtypes = [ctypes.c_uint32, ctypes.c_int64, vp]
        L.bdpt_render_sample_mt.argtypes = [vp, ctypes.POINTER(_FrameParams), f32p, vp, f32p,
                                            ctypes.POINTER(_Splat), i32, ctypes.POINTER(i32)]
        L.bdpt_render_path_sample_mt.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_PathParams), f32p,
                                                 vp, f32p]
        L.bdpt_render_direct_sample_mt.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_DirectParams),
                                                   f32p, vp, f32p]
        i64 = ctypes.c_int64
        L.bdpt_bsdf_eval.argtypes = [vp, i64, vp, vp, vp, vp]
        L.bdpt_bsdf_pdf.argtypes = [vp, i64, vp, vp, vp, vp]
        L.bdpt_bsdf_sample.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
        L.bdpt_bsdf_eval_pdfs.argtypes = [vp, i32, i64, vp, vp, vp, vp]
        L.bdpt_bsdf_local_for.argtypes = [vp, i32, i64, vp, vp, vp, vp]
        L.bdpt_bsdf_type.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(i32)]
        L.bdpt_intersect.argtypes = [vp, i64, vp, i32, vp]
        L.bdpt_splat_to_image_plane.argtypes = [vp, ctypes.POINTER(_FrameParams), i64, vp, vp]
        L.bdpt_debug_sampling.argtypes = [vp, ctypes.POINTER(_FrameParams), i32, i32, i32, i64, vp, vp,
                                          ctypes.POINTER(i32)]
        L.bdpt_debug_fresnel.argtypes = [i32, i64, vp, vp]
        L.bdpt_debug_triangle.argtypes = [i32, i64, vp, vp, vp]
        L.bdpt_get_stats.argtypes = [vp, ctypes.POINTER(_Stats)]
        L.bdpt_multi_create.argtypes = [vp, i32, vp, ctypes.POINTER(vp)]
        L.bdpt_multi_destroy.argtypes = [vp]
        L.bdpt_multi_render_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_PathParams),
                                             ctypes.POINTER(_DirectParams), vp]
        L.bdpt_multi_get_stats.argtypes = [vp, ctypes.POINTER(_MultiStats)]
        L.bdpt_multi_set_sharding.argtypes = [vp, i32]
        L.bdpt_render_window.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow),
                                         ctypes.POINTER(_PathParams), ctypes.POINTER(_DirectParams), vp, vp]
        L.bdpt_render_window_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow),
                                              ctypes.POINTER(_PathParams), ctypes.POINTER(_DirectParams), vp]
        L.bdpt_render_aov.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), vp, vp]
        L.bdpt_render_aov_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), vp]
        L.bdpt_denoise.argtypes = [vp, i32, i32, vp, vp, vp, ctypes.POINTER(_DenoiseParams), vp]
        L.bdpt_denoise_host.argtypes = [vp, i32, i32, vp, vp, vp, ctypes.POINTER(_DenoiseParams)]
        L.bdpt_denoise_planes.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, ctypes.POINTER(_DenoiseParams), vp, vp, vp]
        L.bdpt_denoise_planes_host.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, ctypes.POINTER(_DenoiseParams), vp, vp]
        L.bdpt_batch_moments.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
        L.bdpt_batch_moments_host.argtypes = [vp, i32, i32, i32, vp, vp, vp]
        L.bdpt_render_pixels.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), vp, i32, vp, vp]
        L.bdpt_render_pixels_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), vp, i32, vp]
        L.bdpt_adaptive_resolve.argtypes = [vp, i32, i32, i32, i32, vp, vp, ctypes.c_int64, vp, vp, vp]
        L.bdpt_adaptive_resolve_host.argtypes = [vp, i32, i32, i32, i32, vp, vp, ctypes.c_int64, vp, vp]
        f32 = ctypes.c_float
        L.bdpt_adaptive_select.argtypes = [vp, i32, i32, vp, vp, f32, f32, i32, i32, i32, vp, vp, vp, vp]
        L.bdpt_adaptive_select_host.argtypes = [vp, i32, i32, vp, vp, f32, f32, i32, i32, i32, vp, vp, vp]
        L.bdpt_render_adaptive.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_AdaptiveParams), vp, vp, vp,
                                           ctypes.POINTER(_AdaptiveStats), vp]
        L.bdpt_render_adaptive_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_AdaptiveParams), vp, vp,
                                                vp, ctypes.POINTER(_AdaptiveStats)]
        L.bdpt_adaptive_pass_lists.argtypes = [vp, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
        L.bdpt_reproject.argtypes = [vp, ctypes.POINTER(_FrameParams), vp, vp, vp, vp, vp,
                                     ctypes.POINTER(_ReprojectParams), vp]
        L.bdpt_reproject_host.argtypes = [vp, ctypes.POINTER(_FrameParams), vp, vp, vp, vp, vp,
                                          ctypes.POINTER(_ReprojectParams)]
        L.bdpt_display_thresholds.argtypes = [i32, vp]
        L.bdpt_meter.argtypes = [vp, i32, i32, vp, vp, vp, ctypes.POINTER(_MeterParams), vp, vp]
        L.bdpt_meter_host.argtypes = [vp, i32, i32, vp, vp, vp, ctypes.POINTER(_MeterParams), vp]
        L.bdpt_debug_meter_histogram.argtypes = [vp, vp]
        L.bdpt_display.argtypes = [vp, i32, i32, vp, vp, ctypes.POINTER(_DisplayParams), vp, vp]
        L.bdpt_display_host.argtypes = [vp, i32, i32, vp, vp, ctypes.POINTER(_DisplayParams), vp]
        L.bdpt_encode_png.argtypes = [vp, i32, i32, i32, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
        L.bdpt_save_png.argtypes = [vp, i32, i32, i32, ctypes.c_char_p]
        L.bdpt_save_ppm.argtypes = [vp, i32, i32, ctypes.c_char_p]
        L.bdpt_denoise_var.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, ctypes.POINTER(_DenoiseParams), vp]
        L.bdpt_denoise_var_host.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, ctypes.POINTER(_DenoiseParams)]
        L.bdpt_render_layers.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), i32, vp, vp]
        L.bdpt_render_layers_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), i32, vp]
        L.bdpt_layers_compose.argtypes = [vp, vp, i32, i32, i32, ctypes.c_uint64, vp, vp]
        L.bdpt_scene_emitter_count.argtypes = [vp, ctypes.POINTER(i32)]
        L.bdpt_scene_get_emitter.argtypes = [vp, i32, ctypes.POINTER(_EmitterInfo)]
        L.bdpt_render_light_groups.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), i32, vp, vp, vp]
        L.bdpt_render_light_groups_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), i32, vp, vp]
        L.bdpt_light_groups_relight.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
        L.bdpt_render_strategies.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), i32, i32, i32, vp, vp]
        L.bdpt_render_strategies_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), i32, i32, i32, vp]
        L.bdpt_strategies_shape.argtypes = [i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        L.bdpt_strategies_sheet.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp]
        gl = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_SampleWindow), vp, i32, i32]
        L.bdpt_render_group_layers.argtypes = gl + [vp, vp]
        L.bdpt_render_group_layers_host.argtypes = gl + [vp]
        L.bdpt_render_group_strategies.argtypes = gl + [i32, i32, vp, vp]
        L.bdpt_render_group_strategies_host.argtypes = gl + [i32, i32, vp]
        L.bdpt_group_planes_combine.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
        L.bdpt_group_planes_combine_host.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp]
        L.bdpt_synchronize.argtypes = [vp]
        L.bdpt_config_load_toml.argtypes = [ctypes.c_char_p, ctypes.POINTER(_Config)]
        L.bdpt_render_path.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_PathParams), vp, vp]
        L.bdpt_render_path_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_PathParams), vp]
        for fn, pt in (("bdpt_render_path_sample", _PathParams), ("bdpt_render_direct_sample", _DirectParams)):
            getattr(L, fn).argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(pt), f32p, ctypes.c_uint32,
                                       ctypes.POINTER(i32), f32p]
        L.bdpt_render_direct.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_DirectParams), vp, vp]
        L.bdpt_render_direct_host.argtypes = [vp, ctypes.POINTER(_FrameParams), ctypes.POINTER(_DirectParams), vp]
        L.bdpt_direct_strategy.restype = i32
        L.bdpt_direct_strategy.argtypes = [ctypes.c_char_p]
        L.bdpt_debug_math.argtypes = [i32, i32, vp, vp, vp, ctypes.c_int64]
        L.bdpt_encode_exr.argtypes = [vp, i32, i32, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
        L.bdpt_save_exr.argtypes = [vp, i32, i32, ctypes.c_char_p]
        _lib = L
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        e = BdptError(f"bdpt error {rc}: {lib().bdpt_last_error().decode()}")
        e.code = rc
        raise e


def device_count() -> int:
    n = ctypes.c_int32(0)
    _check(lib().bdpt_device_count(ctypes.byref(n)))
    return n.value


@dataclass
class Camera:
    eye: tuple = (0.0, 0.8, 3.8)
    at: tuple = (0.0, 0.8, 0.0)
    up: tuple = (0.0, 1.0, 0.0)
    fov: float = 30.0

    def c(self) -> _Camera:
        c = _Camera()
        c.eye[:], c.at[:], c.up[:] = list(map(float, self.eye)), list(map(float, self.at)), list(map(float, self.up))
        c.fov = float(self.fov)
        return c


@dataclass(frozen=True)
class SampleWindow:
    """bdpt_sample_window: of each pixel's spp samples, k = first + i * stride for
    0 <= i < count. Samples keep the seed and the 1 / spp weight of the frame's full
    spp, so windows that partition range(spp) sum to the unwindowed frame."""
    first: int = 0
    stride: int = 1
    count: int = 0

    def samples(self) -> range:
        return range(self.first, self.first + self.count * self.stride, self.stride)

    def c(self) -> _SampleWindow:
        return _SampleWindow(self.first, self.stride, self.count)

    @staticmethod
    def parse(text: str, spp: int | None = None) -> "SampleWindow":
        """"F:S:C" (the command line's --sample-window); ValueError when malformed or,
        with spp given, invalid for that spp (the C-ABI's rule)."""
        parts = text.split(":")
        if len(parts) != 3:
            raise ValueError(f"sample window {text!r}: expected first:stride:count")
        try:
            w = SampleWindow(*(int(x) for x in parts))
        except ValueError:
            raise ValueError(f"sample window {text!r}: first, stride and count must be integers") from None
        if w.first < 0:
            raise ValueError(f"sample window {text!r}: first must be >= 0")
        if w.stride < 1:
            raise ValueError(f"sample window {text!r}: stride must be >= 1")
        if w.count < 0:
            raise ValueError(f"sample window {text!r}: count must be >= 0")
        if spp is not None and w.count > 0 and w.first + (w.count - 1) * w.stride >= spp:
            raise ValueError(f"sample window {text!r}: count reaches past spp = {spp}")
        return w


@dataclass
class DenoiseSettings:
    """bdpt_denoise_params with the header's defaults (BDPT_DENOISE_*); norm is set per call
    from the samples rendered so far."""
    iterations: int = 5
    sigma_color: float = 2.0
    sigma_normal: float = 0.3
    sigma_depth: float = 0.02
    demodulate: bool = True

    def c(self, norm: float = 1.0) -> _DenoiseParams:
        return _DenoiseParams(int(self.iterations), float(self.sigma_color), float(self.sigma_normal),
                              float(self.sigma_depth), int(self.demodulate), float(norm))


@dataclass
class Config:
    """The subset of the reference's Config (core.h:195-248) the BDPT path reads."""
    camera: Camera = field(default_factory=Camera)
    width: int = 768   # main.cpp:41-42 defaults
    height: int = 576
    spp: int = 1       # main.cpp:112
    rr_depth: int = 5  # main.cpp:105
    rr_prob: float = 0.0  # read but unused by bdpt.h (its rrProbability is luminance-based, bdpt.h:127-129)
    strategy: int = STRATEGY_BDPT
    russian_roulette: int = 0  # RR_NONE: NO_RR = 1 as shipped (bdpt.h:18); RR_LUMINANCE: its NO_RR = 0 branch
    seed_base: int = REFERENCE_SEED


@dataclass
class PathSettings:
    """PathTracerIntegrator settings ([renderer] of a type = "path" scene, main.cpp:96-101)."""
    explicit: bool = True
    max_depth: int = -1
    rr_depth: int = 5
    rr_prob: float = 0.95
    emitter_samples: int = 1
    bsdf_samples: int = 0

    def c(self) -> _PathParams:
        p = _PathParams()
        p.is_explicit, p.max_depth, p.rr_depth = int(self.explicit), self.max_depth, self.rr_depth
        p.rr_prob, p.emitter_samples, p.bsdf_samples = self.rr_prob, self.emitter_samples, self.bsdf_samples
        return p


# DirectIntegrator::render's samplingStrategy strings (direct.h:450-461) -> BDPT_DIRECT_*
DIRECT_STRATEGIES = {"area": 1, "solidAngle": 2, "cosineHemisphere": 3, "bsdf": 4, "mis": 5}


@dataclass
class DirectSettings:
    """DirectIntegrator settings ([renderer] of a type = "direct" scene, main.cpp:88-92)."""
    sampling_strategy: str = "emitter"  # the reference's default, which its render() rejects
    emitter_samples: int = 1
    bsdf_samples: int = 1

    def c(self) -> _DirectParams:
        d = _DirectParams()
        d.sampling_strategy = DIRECT_STRATEGIES.get(self.sampling_strategy, 0)
        d.emitter_samples, d.bsdf_samples = self.emitter_samples, self.bsdf_samples
        return d


@dataclass
class SceneConfig:
    """loadTOML's result (main.cpp:22-116): the scene file settings, plus the
    objfile resolved as Scene::load does (renderer.cpp:236-241)."""
    toml_file: str
    obj_file: str
    obj_file_raw: str
    config: Config
    realtime: bool
    integrator: str
    path: PathSettings = field(default_factory=PathSettings)
    direct: DirectSettings = field(default_factory=DirectSettings)


def load_toml(path: str) -> SceneConfig:
    c = _Config()
    _check(lib().bdpt_config_load_toml(path.encode(), ctypes.byref(c)))
    cam = Camera(eye=tuple(c.camera.eye), at=tuple(c.camera.at), up=tuple(c.camera.up), fov=c.camera.fov)
    cfg = Config(camera=cam, width=c.width, height=c.height, spp=c.spp, rr_depth=c.rr_depth, rr_prob=c.rr_prob)
    pp = c.path
    path = PathSettings(explicit=bool(pp.is_explicit), max_depth=pp.max_depth, rr_depth=pp.rr_depth,
                        rr_prob=pp.rr_prob, emitter_samples=pp.emitter_samples, bsdf_samples=pp.bsdf_samples)
    direct = DirectSettings(sampling_strategy=c.sampling_strategy.decode(), emitter_samples=c.direct.emitter_samples,
                            bsdf_samples=c.direct.bsdf_samples)
    return SceneConfig(toml_file=c.toml_file.decode(), obj_file=c.obj_file.decode(),
                       obj_file_raw=c.obj_file_raw.decode(), config=cfg, realtime=bool(c.realtime),
                       integrator=c.integrator.decode(), path=path, direct=direct)


def encode_exr(rgb: np.ndarray, width: int, height: int) -> bytes:
    """saveEXR's bytes (utils.h:95-156): half-float B, G, R planes, uncompressed."""
    fb = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1)
    if fb.size != width * height * 3:
        raise BdptError(f"framebuffer has {fb.size} floats, expected {width * height * 3}")
    n = ctypes.c_int64(0)
    _check(lib().bdpt_encode_exr(fb.ctypes.data, width, height, None, 0, ctypes.byref(n)))
    out = np.zeros(n.value, np.uint8)
    _check(lib().bdpt_encode_exr(fb.ctypes.data, width, height, out.ctypes.data, n.value, ctypes.byref(n)))
    return out.tobytes()


def save_exr(rgb: np.ndarray, width: int, height: int, path: str) -> None:
    """Integrator::save (integrator.cpp:26-30)."""
    fb = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1)
    if fb.size != width * height * 3:
        raise BdptError(f"framebuffer has {fb.size} floats, expected {width * height * 3}")
    _check(lib().bdpt_save_exr(fb.ctypes.data, width, height, path.encode()))


@dataclass
class Ray:
    o: tuple
    d: tuple
    min_t: float = 1e-8
    max_t: float = 3.402823466e38


MT19937_WORDS = 625  # BDPT_MT19937_WORDS: _M_x[624], _M_p (libstdc++'s operator<< order)


def _mt_twist(x: np.ndarray) -> None:
    """mersenne_twister_engine::_M_gen_rand (libstdc++ random.tcc) on x[0:624] in place."""
    up, lo, a = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x9908B0DF)
    for k in range(624):
        y = (x[k] & up) | (x[(k + 1) % 624] & lo)
        x[k] = x[(k + 397) % 624] ^ (y >> np.uint32(1)) ^ (a if y & np.uint32(1) else np.uint32(0))


class Sampler:
    """The reference's Sampler (src/core/math.h:63-76): a std::mt19937 and a
    uniform_real_distribution<float>. `state` is the engine as libstdc++ streams
    it (_M_x[624], then the position _M_p); the single-sample renders take and
    advance it exactly as the reference does."""

    def __init__(self, seed: int):
        rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)  # init_genrand == std::mt19937(seed)
        key, pos = rs.get_state()[1:3]
        self.state = np.concatenate([key.astype(np.uint32), [np.uint32(pos)]]).astype(np.uint32)

    @staticmethod
    def from_state(state) -> "Sampler":
        s = Sampler(0)
        st = np.ascontiguousarray(state, np.uint32).reshape(-1)
        if st.size != MT19937_WORDS or st[-1] > 624:
            raise ValueError("a std::mt19937 state is 624 words and a position <= 624")
        s.state = st.copy()
        return s

    @staticmethod
    def for_sample(pixel: int, spp: int, k: int, base: int = REFERENCE_SEED) -> "Sampler":
        return Sampler((base + pixel * spp + k) & 0xFFFFFFFF)

    def next_u32(self) -> int:
        x = self.state
        if x[624] >= 624:
            _mt_twist(x)
            x[624] = 0
        y = int(x[int(x[624])])
        x[624] += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF

    def next(self) -> float:
        """Sampler::next: generate_canonical<float, 24> (random.tcc:3348-3380)."""
        f = np.float32(self.next_u32()) / np.float32(4294967296.0)
        return float(f) if f < 1.0 else float(np.float32(0.99999994))

    def next2D(self) -> tuple:
        x = self.next()
        return x, self.next()


class Scene:
    def __init__(self, obj_path: str):
        h = ctypes.c_void_p()
        _check(lib().bdpt_scene_load_obj(obj_path.encode(), ctypes.byref(h)))
        self._h = h
        self.path = obj_path

    @classmethod
    def from_desc(cls, d: SceneDesc) -> "Scene":
        """bdpt_scene_create: the scene handed over from arrays the caller holds."""
        keep = []

        def arr(a, dt, shape=None):
            a = np.ascontiguousarray(np.asarray(a, dt))
            if shape is not None:
                a = a.reshape(shape)
            keep.append(a)
            return a.ctypes.data

        n = int(np.asarray(d.tri_shape).size)
        mats = (_MaterialDesc * max(len(d.materials), 1))()
        for k, m in enumerate(d.materials):
            mats[k].illum = int(m["illum"])
            for f in ("kd", "ks", "ke", "tf"):
                getattr(mats[k], f)[:] = [float(x) for x in m[f]]
            mats[k].ns, mats[k].ni = float(m["ns"]), float(m["ni"])
            mats[k].scale, mats[k].spec_weight = float(m.get("scale", 1.0)), float(m.get("spec_weight", 0.0))
            mats[k].has_texture = int(m.get("has_texture", 0))
        ems = (_EmitterDesc * max(len(d.emitters), 1))()
        for k, e in enumerate(d.emitters):
            ems[k].shape, ems[k].area = int(e["shape"]), float(e["area"])
            ems[k].radiance[:] = [float(x) for x in e["radiance"]]
            ems[k].ncdf = int(np.asarray(e["cdf"]).size)
            ems[k].cdf = arr(e["cdf"], np.float32)
        c = _SceneDesc()
        c.triangles = n
        c.positions, c.normals = arr(d.positions, np.float32), arr(d.normals, np.float32)
        c.tri_shape, c.tri_prim, c.tri_mat = arr(d.tri_shape, np.int32), arr(d.tri_prim, np.int32), arr(d.tri_mat,
                                                                                                           np.int32)
        c.shapes, c.materials, c.material = int(d.shapes), len(d.materials), ctypes.addressof(mats)
        c.emitters, c.emitter = len(d.emitters), ctypes.addressof(ems)
        bvh = np.ascontiguousarray(np.asarray(d.bvh, BVH_NODE_DTYPE))
        keep.append(bvh)
        c.bvh_nodes, c.bvh = int(bvh.size), bvh.ctypes.data
        c.bvh_order = arr(d.bvh_order, np.int32)
        h = ctypes.c_void_p()
        if d.textures is not None:  # bdpt_scene_create_textured
            texs = (_TextureDesc * max(len(d.textures), 1))()
            for k, t in enumerate(d.textures):
                t = np.asarray(t, np.float32)
                texs[k].height, texs[k].width = int(t.shape[0]), int(t.shape[1])
                texs[k].rgb = arr(t, np.float32)
            tx = _SceneTextures()
            tx.ntextures, tx.texture = len(d.textures), ctypes.addressof(texs)
            tx.diffuse_tex, tx.specular_tex = arr(d.diffuse_tex, np.int32), arr(d.specular_tex, np.int32)
            tx.texcoords = arr(d.texcoords, np.float32) if d.texcoords is not None else None
            _check(lib().bdpt_scene_create_textured(ctypes.byref(c), ctypes.byref(tx), ctypes.byref(h)))
        else:
            _check(lib().bdpt_scene_create(ctypes.byref(c), ctypes.byref(h)))
        self = cls.__new__(cls)
        self._h, self.path = h, None
        return self

    def export_layout(self, array) -> bytes:
        """bdpt_scene_export_layout: one of the device arrays (LAYOUT_ARRAYS) as bytes."""
        i = LAYOUT_ARRAYS.index(array) if isinstance(array, str) else int(array)
        n = ctypes.c_int64(0)
        _check(lib().bdpt_scene_export_layout(self._h, i, None, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(n.value, 1))
        _check(lib().bdpt_scene_export_layout(self._h, i, buf, ctypes.byref(n)))
        return buf.raw[:n.value]

    def export_shade_records(self) -> bytes:
        """bdpt_scene_export_shade_records: the device shade records as uploaded (128 bytes per
        triangle; export_layout("shade") plus the reference leaf box or leaf id)."""
        n = ctypes.c_int64(0)
        _check(lib().bdpt_scene_export_shade_records(self._h, None, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(n.value, 1))
        _check(lib().bdpt_scene_export_shade_records(self._h, buf, ctypes.byref(n)))
        return buf.raw[:n.value]

    def export_textures(self, array) -> bytes:
        """bdpt_scene_export_textures: one of the texture arrays (TEXTURE_ARRAYS) as bytes."""
        i = TEXTURE_ARRAYS.index(array) if isinstance(array, str) else int(array)
        n = ctypes.c_int64(0)
        _check(lib().bdpt_scene_export_textures(self._h, i, None, ctypes.byref(n), None))
        buf = ctypes.create_string_buffer(max(n.value, 1))
        _check(lib().bdpt_scene_export_textures(self._h, i, buf, ctypes.byref(n), None))
        return buf.raw[:n.value]

    def texture_info(self) -> dict:
        """Bitmap textures of the scene: their count, texels and HBM bytes."""
        n, info = ctypes.c_int64(0), (ctypes.c_int64 * 3)()
        _check(lib().bdpt_scene_export_textures(self._h, 0, None, ctypes.byref(n), info))
        return dict(textures=info[0], texels=info[1], device_bytes=info[2])

    def textures(self) -> list:
        """The maps as float32 (h, w, 3) arrays (Tex::cs: gamma-expanded, flipped)."""
        dims = np.frombuffer(self.export_textures("tex_dims"), np.int32).reshape(-1, 3)
        tab = np.frombuffer(self.export_textures("tex_tab"), np.float32).reshape(-1, 4)
        return [tab[at:at + w * h, :3].reshape(h, w, 3).copy() for w, h, at in dims]

    def to_desc(self) -> SceneDesc:
        """The descriptor of this scene, rebuilt from its exports (BVH leaf order back
        to (shape, face) order; materials and emitters from the ingested records)."""
        inf = self.info()
        tf, ti, nf, nu = self.export()
        perm = np.lexsort((ti[:, 1], ti[:, 0]))  # (shape, prim) order
        order = np.empty_like(perm)
        order[perm] = np.arange(perm.size)
        rec = np.frombuffer(self.export_layout("bsdfs_ingested"), np.uint32).reshape(-1, 18)
        recf = rec.view(np.float32)
        mats = [dict(illum=KIND_ILLUM[int(r[0])], kd=f[2:5], ks=f[5:8], tf=f[8:11], ke=f[11:14], ns=f[14], ni=f[15],
                     scale=f[16], spec_weight=f[17]) for r, f in zip(rec, recf)]
        em = np.frombuffer(self.export_layout("emitters"), np.int32).reshape(-1, 12)
        cdf = np.frombuffer(self.export_layout("emit_cdf"), np.float32)
        ems = [dict(shape=int(e[0]), area=e.view(np.float32)[4], radiance=e.view(np.float32)[5:8],
                    cdf=cdf[e[3]:e[3] + e[1] + 1]) for e in em]
        bvh = np.zeros(nf.shape[0], BVH_NODE_DTYPE)
        bvh["bmin"], bvh["bmax"] = nf[:, :3], nf[:, 3:]
        bvh["start"], bvh["nprims"], bvh["right_offset"] = nu[:, 0], nu[:, 1], nu[:, 2]
        d = SceneDesc(positions=tf[perm, :9], normals=tf[perm, 9:], tri_shape=ti[perm, 0], tri_prim=ti[perm, 1],
                      tri_mat=ti[perm, 2], shapes=inf["shapes"], materials=mats, emitters=ems, bvh=bvh,
                      bvh_order=order.astype(np.int32))
        if self.texture_info()["textures"]:
            mt = np.frombuffer(self.export_textures("mat_tex"), np.int32).reshape(-1, 2)
            for m, (kd, ks) in zip(mats, mt):
                m["has_texture"] = int(kd >= 0 or ks >= 0)
            d.textures = self.textures()
            d.diffuse_tex, d.specular_tex = mt[:, 0].copy(), mt[:, 1].copy()
            d.texcoords = np.frombuffer(self.export_textures("tri_st"), np.float32).reshape(-1, 6)[perm]
        return d

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.bdpt_scene_free(self._h)
            self._h = None

    def info(self) -> dict:
        i = _SceneInfo()
        _check(lib().bdpt_scene_get_info(self._h, ctypes.byref(i)))
        return {n: getattr(i, n) for n, _ in _SceneInfo._fields_}

    def emitters(self) -> list:
        """The emitters in Scene::emitters order (the index selectEmitter draws and
        render_light_groups' group_of_emitter is indexed by): dicts of shape, material (index
        into the MTL's materials in file order), area and radiance (the material's Ke)."""
        n = ctypes.c_int32()
        _check(lib().bdpt_scene_emitter_count(self._h, ctypes.byref(n)))
        out = []
        for i in range(n.value):
            e = _EmitterInfo()
            _check(lib().bdpt_scene_get_emitter(self._h, i, ctypes.byref(e)))
            out.append(dict(shape=int(e.shape), material=int(e.material), area=float(e.area),
                            radiance=tuple(float(x) for x in e.radiance)))
        return out

    def bsdf_type(self, mat: int) -> tuple:
        """(BSDF::getType() flags, kind) of material `mat` (core.h:311; kind 1 diffuse,
        2 mirror, 3 glass, 4 mixture, 5 phong, 0 null)."""
        t, k = ctypes.c_uint32(0), ctypes.c_int32(0)
        _check(lib().bdpt_bsdf_type(self._h, mat, ctypes.byref(t), ctypes.byref(k)))
        return t.value, k.value

    def export(self):
        """(tri_f32[n,18], tri_i32[n,3], node_f32[m,6], node_u32[m,3]) in the reference's dump layout."""
        inf = self.info()
        n, m = inf["triangles"], inf["bvh_nodes"]
        tf, ti = np.zeros((n, 18), np.float32), np.zeros((n, 3), np.int32)
        nf, nu = np.zeros((m, 6), np.float32), np.zeros((m, 3), np.uint32)
        _check(lib().bdpt_scene_export(self._h, tf.ctypes.data, ti.ctypes.data, nf.ctypes.data, nu.ctypes.data))
        return tf, ti, nf, nu

    def export_traversal(self):
        """(wnodes[k,8,4], wtri[n,3,4], lbox[l,2,4], root_link): the traversal tree
        (wide_bvh.hpp); the link / index / leaf-id words are uint32 bit patterns."""
        inf = self.info()
        wn = np.zeros((inf["wide_nodes"], 8, 4), np.float32)
        wt = np.zeros((inf["triangles"], 3, 4), np.float32)
        lb = np.zeros((inf["bvh_leaves"], 2, 4), np.float32)
        root = ctypes.c_uint32()
        _check(lib().bdpt_scene_export_traversal(self._h, wn.ctypes.data, wt.ctypes.data, lb.ctypes.data,
                                                 ctypes.byref(root)))
        return wn, wt, lb, int(root.value)


def camera_constants(cam: Camera, width: int, height: int) -> np.ndarray:
    out = np.zeros(72, np.float32)
    c = cam.c()
    _check(lib().bdpt_camera_constants(ctypes.byref(c), width, height,
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


def layers_longest_path(rr_depth: int, strategy: int = STRATEGY_BDPT) -> int:
    """The longest full path (camera -> ... -> emitter, in edges) a frame without Russian roulette
    holds, from the subpath loops' `depth < rrDepth` (bdpt.h:68, :188): both subpaths have vertices at
    depths 1 .. rr_depth - 1. Layer k - 1 of render_layers is the last that can be non-zero; 0: the
    frame is black.
      BDPT           connectVertices joins two deepest vertices: (D - 1) + (D - 1) + 1 = 2 D - 1 (0 at D = 1)
      PATH_TRACING   connectToLight at the deepest eye vertex: (D - 1) + 1 = D                  (0 at D = 1)
      LIGHT_TRACING  connectToCamera at the deepest light vertex: D; the camera ray's own emitter hit
                     (1 edge) is added whatever D is: max(1, D)"""
    D = int(rr_depth)
    if strategy == STRATEGY_LIGHT_TRACING:
        return max(1, D)
    if D <= 1:
        return 0
    return D if strategy == STRATEGY_PATH_TRACING else 2 * D - 1


STRATEGIES_WEIGHTED, STRATEGIES_UNWEIGHTED = 0, 1  # bdpt_render_strategies' weighting (BDPT_STRATEGIES_*)
STRATEGIES_MAX_S, STRATEGIES_MAX_T = 29, 28
LAYERS_MAX = GROUPS_MAX = 64  # bdpt_render_layers' / bdpt_render_light_groups' most planes
PLANE_PIXELS_MAX = 1 << 30    # planes * W * H of every plane render stays below it


def strategies_shape(rr_depth: int, strategy: int = STRATEGY_BDPT) -> tuple:
    """bdpt_strategies_shape: (n_s, n_t), the smallest render_strategies shape that holds every
    strategy of an rr_depth without clamping: n_s = max(D, 1) + 1 (s reaches D
    through a light vertex stored at depth D - 1), n_t = max(D, 2) (t reaches D through an eye
    vertex at depth D - 1; light tracing's primary emission is (0, 2) whatever D is)."""
    n_s, n_t = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().bdpt_strategies_shape(int(rr_depth), int(strategy), ctypes.byref(n_s), ctypes.byref(n_t)))
    return n_s.value, n_t.value


def strategy_plane(s: int, t: int, n_s: int, n_t: int) -> int:
    """The plane of render_strategies' (n_s, n_t) framebuffer that strategy (s, t) is added to:
    min(s, n_s - 1) * n_t + min(t, n_t) - 1, the last row and column collecting what is longer
    (s >= 0 light-subpath vertices, t >= 1 eye-subpath vertices with the camera counted)."""
    s, t, n_s, n_t = int(s), int(t), int(n_s), int(n_t)
    if s < 0 or t < 1 or n_s < 1 or n_t < 1:
        raise ValueError(f"strategy_plane: s >= 0, t >= 1, n_s >= 1, n_t >= 1, got {(s, t, n_s, n_t)}")
    return min(s, n_s - 1) * n_t + min(t, n_t) - 1


def _sheet_args(planes, gains):
    """strategies_sheet's arguments checked as bdpt_strategies_sheet checks them (before anything is
    copied): planes (n_s, n_t, H, W, 3) within the shape limits and below 2^31 floats, gains None or
    finite (n_s, n_t, 3) / (n_s, n_t) / (n_s * n_t, 3). -> (float32 planes, float32 (n_s * n_t, 3) or None)."""
    shape = np.shape(planes)
    if len(shape) != 5 or shape[4] != 3:
        raise BdptError(f"strategies_sheet: planes must be (n_s, n_t, H, W, 3), got {shape}")
    n_s, n_t, H, W = shape[:4]
    if not 1 <= n_s <= STRATEGIES_MAX_S or not 1 <= n_t <= STRATEGIES_MAX_T or H < 1 or W < 1:
        raise BdptError(f"strategies_sheet: n_s must be in [1, 29], n_t in [1, 28], H and W > 0, got {shape}")
    if n_s * n_t * H * W * 3 >= 1 << 31:
        raise BdptError("strategies_sheet: the sheet (n_s * n_t * W * H * 3 floats) must be below 2^31 floats")
    g = None
    if gains is not None:
        g = np.asarray(gains, np.float32)
        if g.shape == (n_s, n_t):
            g = np.repeat(g[:, :, None], 3, axis=2)
        if g.shape not in ((n_s, n_t, 3), (n_s * n_t, 3)):
            raise BdptError(f"strategies_sheet: gains must be ({n_s}, {n_t}, 3), ({n_s}, {n_t}) or "
                            f"({n_s * n_t}, 3), got {g.shape}")
        g = np.ascontiguousarray(g.reshape(n_s * n_t, 3))
        if not np.isfinite(g).all():
            raise BdptError("strategies_sheet: a gain is not finite")
    return np.ascontiguousarray(planes, np.float32), g


def strategies_sheet_numpy(planes, gains=None) -> np.ndarray:
    """What bdpt_strategies_sheet computes, as the obvious loop on the host: the (n_t * H, n_s * W, 3)
    float32 image with the tile of (s, t) at tile column s, tile row t - 1, each float one float32
    product gains[s, t - 1, c] * planes[s, t - 1, y, x, c] (no gains: the plane's float)."""
    a, g = _sheet_args(planes, gains)
    n_s, n_t, H, W = a.shape[:4]
    out = np.zeros((n_t * H, n_s * W, 3), np.float32)
    for s in range(n_s):
        for r in range(n_t):  # r = t - 1
            tile = a[s, r] if g is None else g[s * n_t + r][None, None, :] * a[s, r]
            out[r * H:(r + 1) * H, s * W:(s + 1) * W] = tile
    return out


GROUP_INNER_MAX = STRATEGIES_MAX_S * STRATEGIES_MAX_T  # bdpt_group_planes_combine's most planes per group


def _group_planes_args(planes, gains, weights):
    """combine_group_planes' arguments checked as bdpt_group_planes_combine checks them (before anything
    is copied): planes (n_groups, n_layers, H, W, 3) or (n_groups, n_s, n_t, H, W, 3) within the limits,
    gains None or finite (n_groups, 3) / (n_groups,), weights None or finite with the inner axes' shape
    or flat. -> (float32 (n_groups, n_inner, H, W, 3) planes, (n_groups, 3) gains or None, (n_inner,)
    weights or None)."""
    shape = np.shape(planes)
    if len(shape) not in (5, 6) or shape[-1] != 3:
        raise BdptError("combine_group_planes: planes must be (n_groups, n_layers, H, W, 3) or "
                        f"(n_groups, n_s, n_t, H, W, 3), got {shape}")
    n, inner, (H, W) = shape[0], shape[1:-3], shape[-3:-1]
    n_inner = math.prod(inner)
    if not 1 <= n <= GROUPS_MAX or not 1 <= n_inner <= GROUP_INNER_MAX or H < 1 or W < 1:
        raise BdptError(f"combine_group_planes: n_groups must be in [1, {GROUPS_MAX}], the planes per group in "
                        f"[1, {GROUP_INNER_MAX}], H and W > 0, got {shape}")
    if n * n_inner * H * W >= PLANE_PIXELS_MAX:
        raise BdptError("combine_group_planes: n_groups * n_inner * W * H must be below 2^30")
    g = w = None
    if gains is not None:
        g = np.asarray(gains, np.float32)
        if g.shape == (n,):
            g = np.repeat(g[:, None], 3, axis=1)
        if g.shape != (n, 3):
            raise BdptError(f"combine_group_planes: gains must be ({n}, 3) or ({n},), got {g.shape}")
        g = np.ascontiguousarray(g)
        if not np.isfinite(g).all():
            raise BdptError("combine_group_planes: a gain is not finite")
    if weights is not None:
        w = np.asarray(weights, np.float32)
        if w.shape not in (tuple(inner), (n_inner,)):
            raise BdptError(f"combine_group_planes: weights must be {tuple(inner)} or ({n_inner},), got {w.shape}")
        w = np.ascontiguousarray(w.reshape(n_inner))
        if not np.isfinite(w).all():
            raise BdptError("combine_group_planes: a weight is not finite")
    return np.ascontiguousarray(planes, np.float32).reshape(n, n_inner, H, W, 3), g, w


def combine_group_planes_numpy(planes, gains=None, weights=None) -> np.ndarray:
    """What bdpt_group_planes_combine computes, as the obvious loop on the host: with acc the first
    term, for g ascending and within it j ascending t = weights[j] * planes[g, j]; t = gains[g] * t;
    acc = acc + t, every operation a float32 rounding of its own (None: ones, multiplied like any)."""
    a, g, w = _group_planes_args(planes, gains, weights)
    n, n_inner = a.shape[:2]
    g = np.ones((n, 3), np.float32) if g is None else g
    w = np.ones(n_inner, np.float32) if w is None else w
    acc = None
    for i in range(n):
        for j in range(n_inner):
            t = g[i][None, None, :] * (w[j] * a[i, j])
            acc = t if acc is None else acc + t
    assert acc.dtype == np.float32
    return acc


DENOISE_PLANES_OWN, DENOISE_PLANES_SHARED = 0, 1  # bdpt_denoise_planes' mode (BDPT_DENOISE_PLANES_*)


def _denoise_planes_mode(mode) -> int:
    """"own" / "shared" or a DENOISE_PLANES_* value (any other int reaches the library as it is)."""
    if isinstance(mode, str):
        if mode not in ("own", "shared"):
            raise BdptError(f"denoise_planes: mode must be 'own' or 'shared', got {mode!r}")
        return DENOISE_PLANES_SHARED if mode == "shared" else DENOISE_PLANES_OWN
    return int(mode)


def denoise_planes_numpy(planes, aov, mode="shared", guide=None, settings=None, norm=1.0, dt=np.float64):
    """What bdpt_denoise_planes computes, as the header states it, every operation in `dt`: planes of any
    leading shape (..., H, W, 3) filtered with weights of their own ("own") or with the weights of one colour
    guide G ("shared": `guide`, or the planes' sequential float32 sum). -> (filtered planes in planes' shape,
    filtered guide or None in own mode), both in dt. The guide rides along as one more plane whose colour
    forms the weights, so its update is the planes' formula."""
    f = dt
    d = settings or DenoiseSettings()
    shared = _denoise_planes_mode(mode) == DENOISE_PLANES_SHARED
    a = np.asarray(planes, np.float32)
    H, W = a.shape[-3:-1]
    flat = a.reshape((-1, H, W, 3))
    n = flat.shape[0]
    if not shared and guide is not None:
        raise BdptError("denoise_planes: guide must be None in own mode")
    img = flat.astype(dt) * f(norm)
    if shared:
        if guide is None:
            G = flat[0].copy()
            for k in range(1, n):
                G = G + flat[k]  # float32, ascending
        else:
            G = np.asarray(guide, np.float32).reshape(H, W, 3)
        img = np.concatenate([img, (G.astype(dt) * f(norm))[None]])
    if d.iterations == 0:
        return img[:n].reshape(a.shape), (img[n] if shared else None)
    av = np.asarray(aov, np.float32).reshape(H, W, 8).astype(dt) * f(norm)
    cov = av[..., 7]
    hit = cov > 0
    safe = np.where(hit, cov, f(1))
    alb = np.where(hit[..., None], av[..., 0:3] / safe[..., None], f(1))
    N = np.where(hit[..., None], av[..., 3:6] / safe[..., None], f(0))
    z = np.where(hit, av[..., 6] / safe, f(0))
    m = np.maximum(alb, f(1e-3))
    if d.demodulate:
        img = img / m
    kern = np.array([1, 4, 6, 4, 1], dt) / f(16)
    zs = f(d.sigma_depth) * np.maximum(z, f(1e-6))
    for i in range(d.iterations):
        s = 1 << i
        sc = f(d.sigma_color) * f(2.0 ** -i)
        num = np.zeros_like(img)
        den = np.zeros((1 if shared else n, H, W), dt)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                py = slice(max(0, -oy), min(H, H - oy))
                px = slice(max(0, -ox), min(W, W - ox))
                if py.start >= py.stop or px.start >= px.stop:
                    continue
                qy = slice(py.start + oy, py.stop + oy)
                qx = slice(px.start + ox, px.stop + ox)
                h = kern[dy + 2] * kern[dx + 2]
                src = img[n:] if shared else img  # whose colour forms the weights
                if dx == 0 and dy == 0:
                    w = np.ones((src.shape[0], H, W), dt)
                else:
                    dc = src[:, py, px] - src[:, qy, qx]
                    dn = N[py, px] - N[qy, qx]
                    dz = z[py, px] - z[qy, qx]
                    wc = np.exp(-np.minimum(((dc[..., 0] ** 2 + dc[..., 1] ** 2) + dc[..., 2] ** 2) / (sc * sc), f(80)))
                    wn = np.exp(-np.minimum(((dn[..., 0] ** 2 + dn[..., 1] ** 2) + dn[..., 2] ** 2)
                                            / (f(d.sigma_normal) * f(d.sigma_normal)), f(80)))
                    wz = np.exp(-np.minimum((dz * dz) / (zs[py, px] * zs[py, px]), f(80)))
                    w = np.where(hit[py, px] == hit[qy, qx], (wc * wn) * wz, f(0))
                hw = h * w
                num[:, py, px] += hw[..., None] * img[:, qy, qx]
                den[:, py, px] += hw
        img = num / den[..., None]
    if d.demodulate:
        img = img * m
    assert img.dtype == dt
    return img[:n].reshape(a.shape), (img[n] if shared else None)


BATCHES_MIN, BATCHES_MAX = 2, 64  # bdpt_batch_moments' n_batches


def batch_windows(spp: int, n_batches: int, window: "SampleWindow | None" = None) -> list:
    """The sample windows of render_batches: with window (first, stride, count) (None: the whole spp), batch b
    takes (first + b * stride, stride * n_batches, count / n_batches), so the batches interleave, partition the
    window and are equally large (what bdpt_batch_moments' variance formula assumes). ValueError, the argument
    named, for n_batches outside 2..64 or a count that is not a positive multiple of n_batches."""
    n_batches = int(n_batches)
    if not BATCHES_MIN <= n_batches <= BATCHES_MAX:
        raise ValueError(f"render_batches: n_batches must be in [{BATCHES_MIN}, {BATCHES_MAX}], got {n_batches}")
    w = window if window is not None else SampleWindow(0, 1, int(spp))
    if w.count < 1 or w.count % n_batches:
        raise ValueError(f"render_batches: count ({w.count}: the window's, or the spp) must be a positive multiple "
                         f"of n_batches = {n_batches}")
    return [SampleWindow(w.first + b * w.stride, w.stride * n_batches, w.count // n_batches) for b in range(n_batches)]


def batch_moments_numpy(planes, dt=np.float32):
    """What bdpt_batch_moments computes, as the header states it, every operation in `dt`: planes (K, ...) ->
    (sum, var) in dt. In float32 the loop below is the kernel's, operation for operation."""
    a = np.asarray(planes, np.float32).astype(dt)
    K = a.shape[0]
    if not BATCHES_MIN <= K <= BATCHES_MAX:
        raise ValueError(f"batch_moments: n_batches must be in [{BATCHES_MIN}, {BATCHES_MAX}], got {K}")
    S = a[0].copy()
    for b in range(1, K):
        S = S + a[b]
    mu = S / dt(K)
    Q = None
    for b in range(K):
        d = a[b] - mu
        Q = d * d if Q is None else Q + d * d
    var = Q * dt(np.float32(K) / np.float32(K - 1))
    assert S.dtype == dt and var.dtype == dt
    return S, var


ADAPTIVE_EPS = 1e-3  # render_adaptive's default floor under the channel sum of S


def adaptive_splat_scale(spp: int, n_pixels: int, n_batches: int, total: int, dt=np.float32):
    """bdpt_adaptive_resolve's t = spp W H / (K M), formed in double and rounded once to dt (0 when M == 0)."""
    if total <= 0:
        return dt(0)
    return dt(np.float64(spp) * np.float64(n_pixels) / (np.float64(n_batches) * np.float64(total)))


def adaptive_resolve_numpy(planes, m, spp: int, dt=np.float32):
    """What bdpt_adaptive_resolve computes, as the header states it, every operation in `dt`: planes
    (K, 2, H, W, 3), pair b = (T_b splats, E_b eye) as render_pixels accumulates them, m (H, W) int samples per
    batch -> (S, var), both (H, W, 3) in dt. In float32 the loop below is the kernel's, operation for operation."""
    pl = np.asarray(planes)
    if pl.ndim != 5 or pl.shape[1] != 2 or pl.shape[4] != 3:
        raise ValueError(f"adaptive_resolve: planes must be (n_batches, 2, H, W, 3), got {pl.shape}")
    K, _, H, W, _ = pl.shape
    if not BATCHES_MIN <= K <= BATCHES_MAX:
        raise ValueError(f"adaptive_resolve: n_batches must be in [{BATCHES_MIN}, {BATCHES_MAX}], got {K}")
    mm = np.asarray(m, np.int64).reshape(H, W)
    t = adaptive_splat_scale(spp, H * W, K, int(mm.sum()), dt)
    den = np.where(mm > 0, K * mm, 1).astype(dt)
    a = np.where(mm > 0, dt(spp) / den, dt(0)).astype(dt)[..., None]
    pl = pl.astype(dt)

    def plane(b):
        x = pl[b, 1] * a
        y = pl[b, 0] * t
        return x + y

    S = plane(0)
    for b in range(1, K):
        S = S + plane(b)
    mu = S / dt(K)
    Q = None
    for b in range(K):
        d = plane(b) - mu
        Q = d * d if Q is None else Q + d * d
    var = Q * dt(np.float32(K) / np.float32(K - 1))
    assert S.dtype == dt and var.dtype == dt
    return S, var


def adaptive_noisy_numpy(S, var, threshold: float, eps: float) -> np.ndarray:
    """bdpt_adaptive_select's noisy(p), float32 in the header's order: (H, W) bool from S and var (H, W, 3)."""
    f = np.float32
    S, var = np.asarray(S, f), np.asarray(var, f)
    with np.errstate(over="ignore", invalid="ignore"):
        v = (var[..., 0] + var[..., 1]) + var[..., 2]
        s = ((S[..., 0] + S[..., 1]) + S[..., 2]) + f(eps)
        return v > (f(threshold) * f(threshold)) * (s * s)


def adaptive_select_numpy(S, var, m, threshold: float, eps: float, step: int, m_max: int, dilate: bool = True):
    """What bdpt_adaptive_select computes: S, var (H, W, 3), m (H, W) int32 -> (list int32 ascending, m_new (H, W)
    int32): the active pixels (noisy, or with dilate any pixel of the clipped 3 x 3 neighbourhood noisy, and
    m + step <= m_max) and m with step added at exactly those."""
    noisy = adaptive_noisy_numpy(S, var, threshold, eps)
    H, W = noisy.shape
    wanted = noisy
    if dilate:
        pad = np.zeros((H + 2, W + 2), bool)
        pad[1:-1, 1:-1] = noisy
        wanted = np.zeros((H, W), bool)
        for dy in range(3):
            for dx in range(3):
                wanted |= pad[dy:dy + H, dx:dx + W]
    mm = np.asarray(m, np.int32).reshape(H, W)
    active = wanted & (mm.astype(np.int64) + int(step) <= int(m_max))
    lst = np.flatnonzero(active.reshape(-1)).astype(np.int32)
    return lst, (mm + np.where(active, np.int32(step), np.int32(0))).astype(np.int32)


def adaptive_windows(n_batches: int, step: int, n_pass: int) -> list:
    """The sample windows of adaptive pass n_pass, one per batch: (n_pass * step * K + b, K, step)."""
    return [SampleWindow(n_pass * step * n_batches + b, n_batches, step) for b in range(n_batches)]


@dataclass
class ReprojectSettings:
    """bdpt_reproject_params with the header's defaults (BDPT_REPROJECT_*); prev_camera, norm and cur_samples
    are set per call."""
    max_history: float = 16.0
    sigma_normal: float = 0.3
    sigma_depth: float = 0.02
    min_weight: float = 0.1
    clamp_sigma: float = 2.0
    demodulate: bool = True

    def c(self, prev_camera: "Camera", cur_samples: float, norm: float = 1.0) -> _ReprojectParams:
        return _ReprojectParams(prev_camera.c(), float(norm), float(cur_samples), float(self.max_history),
                                float(self.sigma_normal), float(self.sigma_depth), float(self.min_weight),
                                float(self.clamp_sigma), int(self.demodulate))


HISTORY_CHANNELS = 8  # bdpt_reproject's state per pixel: I_r I_g I_b n N_x N_y N_z z


def reproject_numpy(color, aov, hist, dirs, cam_consts_cur, cam_consts_prev, settings=None, norm=1.0, dt=np.float32,
                    cur_samples=1.0):
    """What bdpt_reproject computes, as the header states it, every operation in `dt`: color (H, W, 3), aov
    (H, W, 8), hist (H, W, 8) or None, dirs (H, W, 3) the pixels' primary ray directions at spp 1, the two
    cameras' 72 constants (camera_constants) -> (out_color (H, W, 3), hist_out (H, W, 8)) in dt. In float32
    the steps below are the kernel's, operation for operation."""
    f = dt
    s = settings or ReprojectSettings()
    av = np.asarray(aov, np.float32)
    H, W = av.shape[:2]
    av = av.reshape(H, W, 8).astype(dt) * f(norm)
    c = np.asarray(color, np.float32).reshape(H, W, 3).astype(dt) * f(norm)
    d = np.asarray(dirs, np.float32).reshape(H, W, 3).astype(dt)
    cc = np.asarray(cam_consts_cur, np.float32).reshape(72).astype(dt)
    cp = np.asarray(cam_consts_prev, np.float32).reshape(72).astype(dt)
    n_c, demod, k = f(cur_samples), bool(s.demodulate), f(s.clamp_sigma)
    one, half, zero = f(1), f(0.5), f(0)
    with np.errstate(all="ignore"):
        cov = av[..., 7]
        hit = cov > 0
        sc = np.where(hit, cov, one)
        g = av / sc[..., None]
        m = np.maximum(g[..., 0:3], f(1e-3))
        Np, z = g[..., 3:6], g[..., 6]
        Ic = c / m if demod else c

        has = np.zeros((H, W), bool)
        Hh = np.zeros((H, W, 3), dt)
        n_h = np.zeros((H, W), dt)
        if hist is not None:
            hs = np.asarray(hist, np.float32).reshape(H, W, 8).astype(dt)
            eye_c, eye_p = cc[28:31], cp[28:31]  # cameraToWorld's translation
            X = [eye_c[i] + z * d[..., i] for i in range(3)]
            w = cp[0:16]  # worldToCamera, column-major: row r is w[r], w[4 + r], w[8 + r], w[12 + r]
            xc, yc, zc = (((w[r] * X[0] + w[4 + r] * X[1]) + w[8 + r] * X[2]) + w[12 + r] for r in range(3))
            zc = -zc
            front = hit & (zc >= one)
            zs = np.where(front, zc, one)
            tan = cp[66]
            u = xc / (zs * (tan * cp[67]))
            v = yc / (zs * tan)

            def snap(x):
                r = np.floor(x + half)
                return np.where(np.abs(x - r) <= f(2.0 ** -10), r, x)

            fx = snap(((u + one) * half) * f(W) - half)
            fy = snap(((one - v) * half) * f(H) - half)
            x0f, y0f = np.floor(fx), np.floor(fy)
            near = front & (x0f >= -one) & (x0f < f(2.0 ** 30)) & (y0f >= -one) & (y0f < f(2.0 ** 30))
            x0 = np.where(near, x0f, zero).astype(np.int64)
            y0 = np.where(near, y0f, zero).astype(np.int64)
            ax, ay = fx - x0f, fy - y0f
            bx, by = (one - ax, ax), (one - ay, ay)
            e = [X[i] - eye_p[i] for i in range(3)]
            zp = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            ztol = f(s.sigma_depth) * zp
            sn2 = f(s.sigma_normal) * f(s.sigma_normal)
            sw = np.zeros((H, W), dt)
            sn = np.zeros((H, W), dt)
            sI = np.zeros((H, W, 3), dt)
            for t in range(4):
                qx, qy = x0 + (t & 1), y0 + (t >> 1)
                b = bx[t & 1] * by[t >> 1]
                ok = near & (b != zero) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                hq = hs[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                ok &= (hq[..., 7] > zero) & (np.abs(hq[..., 7] - zp) <= ztol)
                dn = Np - hq[..., 4:7]
                ok &= (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2] <= sn2
                has |= ok
                sw = np.where(ok, sw + b, sw)
                sI = np.where(ok[..., None], sI + b[..., None] * hq[..., 0:3], sI)
                sn = np.where(ok, sn + b * hq[..., 3], sn)
            has &= sw >= f(s.min_weight)
            sws = np.where(has, sw, one)
            Hh = sI / sws[..., None]
            n_h = np.minimum(sn / sws, f(s.max_history))

        if k > zero and has.any():
            pad = np.zeros((H + 2, W + 2), bool)
            pad[1:-1, 1:-1] = hit
            Ip = np.zeros((H + 2, W + 2, 3), dt)
            Ip[1:-1, 1:-1] = Ic
            S, Q, cnt = np.zeros((H, W, 3), dt), np.zeros((H, W, 3), dt), np.zeros((H, W), dt)
            for dy in range(3):
                for dx in range(3):
                    ok = pad[dy:dy + H, dx:dx + W]
                    S = np.where(ok[..., None], S + Ip[dy:dy + H, dx:dx + W], S)
                    cnt = np.where(ok, cnt + one, cnt)
            cs = np.where(cnt > zero, cnt, one)[..., None]
            mu = S / cs
            for dy in range(3):
                for dx in range(3):
                    ok = pad[dy:dy + H, dx:dx + W]
                    dI = Ip[dy:dy + H, dx:dx + W] - mu
                    Q = np.where(ok[..., None], Q + dI * dI, Q)
            sd = np.sqrt(Q / cs)
            lo, hi = mu - sd * k, mu + sd * k
            Hh = np.where(Hh < lo, lo, np.where(Hh > hi, hi, Hh))

        n_out = n_h + n_c
        alpha = (n_c / n_out)[..., None]
        Io = Hh + (Ic - Hh) * alpha
        blended = Io * m if demod else Io
        hb = has[..., None]
        out = np.where(hb, blended, c)
        state = np.zeros((H, W, 8), dt)
        state[..., 0:3] = np.where(hit[..., None], np.where(hb, Io, Ic), c)
        state[..., 3] = np.where(has, n_out, n_c)
        state[..., 4:7] = np.where(hit[..., None], Np, zero)
        state[..., 7] = np.where(hit, z, zero)
    assert out.dtype == dt and state.dtype == dt
    return out, state


TONES = {"clamp": 0, "reinhard": 1, "filmic": 2}      # BDPT_TONE_*
ENCODES = {"srgb": 0, "gamma22": 1, "linear": 2}     # BDPT_ENCODE_*
METER_BINS = 4096  # BDPT_METER_BINS


def _code_of(table, value, what):
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"{what} must be one of {sorted(table)}, not {value!r}")
        return table[value]
    return int(value)  # (the library refuses an unknown code)


@dataclass
class MeterSettings:
    """bdpt_meter_params with the header's defaults (BDPT_METER_*); norm is set per call."""
    key: float = 0.18
    key_permille: int = 500
    white_permille: int = 990
    rate: float = 0.25
    fallback_exposure: float = 1.0
    fallback_white: float = 1.0

    def c(self, norm: float = 1.0) -> _MeterParams:
        return _MeterParams(float(norm), float(self.key), int(self.key_permille), int(self.white_permille),
                            float(self.rate), float(self.fallback_exposure), float(self.fallback_white))


@dataclass
class DisplaySettings:
    """bdpt_display_params; tone and encode by name (TONES, ENCODES) or code; norm is set per call. exposure and
    white are what a call without meter words uses."""
    exposure: float = 1.0
    white: float = 1.0
    tone: "str | int" = "reinhard"
    encode: "str | int" = "srgb"
    channels: int = 3

    def c(self, norm: float = 1.0) -> _DisplayParams:
        return _DisplayParams(float(norm), float(self.exposure), float(self.white), _code_of(TONES, self.tone, "tone"),
                              _code_of(ENCODES, self.encode, "encode"), int(self.channels))


def display_thresholds(encode="srgb") -> np.ndarray:
    """bdpt_display_thresholds: the 255 float32 places where the 8-bit code of `encode` steps (no device)."""
    out = np.zeros(255, np.float32)
    _check(lib().bdpt_display_thresholds(_code_of(ENCODES, encode, "encode"), out.ctypes.data))
    return out


def meter_histogram_numpy(color, aov=None, norm=1.0) -> np.ndarray:
    """The 4096 bin counts bdpt_meter forms (uint32), float32 as the kernel: bin = bits(Y) >> 19 of the
    covered pixels whose Y is a positive normal finite float."""
    f = np.float32
    c = np.asarray(color, f).reshape(-1, 3)
    with np.errstate(all="ignore"):
        c = c * f(norm)
        Y = (f(0.212671) * c[:, 0] + f(0.715160) * c[:, 1]) + f(0.072169) * c[:, 2]
        b = np.ascontiguousarray(Y, f).view(np.uint32) >> np.uint32(19)
        ok = (b >= 16) & (b < 4080)
        if aov is not None:
            ok &= np.asarray(aov, f).reshape(-1, 8)[:, 7] * f(norm) > 0
    return np.bincount(b[ok].astype(np.int64), minlength=METER_BINS).astype(np.uint32)


def meter_numpy(color, aov=None, settings=None, prev=None, norm=1.0) -> np.ndarray:
    """What bdpt_meter computes, as the header states it: color (H, W, 3), aov (H, W, 8) or None, prev an earlier
    call's 4 words or None -> the 4 words [e, w, T, b_key | b_white << 16] as uint32. Float32, operation for
    operation the kernels' own."""
    f = np.float32
    s = settings or MeterSettings()
    hist = meter_histogram_numpy(color, aov, norm)
    T = int(hist.sum())
    out = np.zeros(4, np.uint32)
    if T == 0:
        out[:2] = np.array([s.fallback_exposure, s.fallback_white], f).view(np.uint32)
        return out
    run = np.cumsum(hist.astype(np.int64))
    bins = [int(np.searchsorted(run, (T * int(pm) + 999) // 1000, side="left")) for pm in (s.key_permille, s.white_permille)]
    Yk, Yw = (np.array([b << 19 | 1 << 18], np.uint32).view(f)[0] for b in bins)
    with np.errstate(all="ignore"):
        e = f(s.key) / Yk
        if prev is not None and f(s.rate) < 1:
            e_p = np.asarray(prev, np.uint32).reshape(4)[:1].view(f)[0]
            if e_p > 0:
                e = e_p + (e - e_p) * f(s.rate)
        ew = e * Yw
    w = ew if ew > 1 else f(1)
    out[:2] = np.array([e, w], f).view(np.uint32)
    out[2], out[3] = T, bins[0] | bins[1] << 16
    return out


def display_numpy(color, thresholds, settings=None, meter=None, norm=1.0) -> np.ndarray:
    """What bdpt_display computes, as the header states it: color (H, W, 3), thresholds the library's table of
    settings.encode (display_thresholds), meter bdpt_meter's 4 words or None -> uint8 (H, W, channels). Float32,
    operation for operation the kernel's own; the code is searchsorted(T, y, side="right")."""
    f = np.float32
    s = settings or DisplaySettings()
    c = np.asarray(color, f)
    H, W = c.shape[:2]
    T = np.asarray(thresholds, f).reshape(255)
    e, w = f(s.exposure), f(s.white)
    if meter is not None:
        e, w = np.asarray(meter, np.uint32).reshape(4)[:2].view(f)
    tone = _code_of(TONES, s.tone, "tone")
    with np.errstate(all="ignore"):
        x = (c.reshape(H, W, 3) * f(norm)) * e
        x = np.where(x > 0, x, f(0))
        x = np.where(x < f(65536), x, f(65536))
        if tone == TONES["reinhard"]:
            iw2 = f(1) / (w * w)
            y = (x * (f(1) + x * iw2)) / (f(1) + x)
        elif tone == TONES["filmic"]:
            n = x * (f(2.51) * x + f(0.03))
            d = x * (f(2.43) * x + f(0.59)) + f(0.14)
            y = n / d
        else:
            y = x
    code = np.searchsorted(T, y, side="right").astype(np.uint8)
    if int(s.channels) == 4:
        code = np.concatenate([code, np.full((H, W, 1), 255, np.uint8)], axis=-1)
    return code


def _image_bytes(pixels, width, height, channels):
    a = np.ascontiguousarray(pixels, dtype=np.uint8).reshape(-1)
    if a.size != width * height * channels:
        raise BdptError(f"image has {a.size} bytes, expected {width * height * channels}")
    return a


def encode_png(pixels, width: int, height: int, channels: int = 3) -> bytes:
    """bdpt_encode_png: 8-bit RGB / RGBA as an uncompressed PNG (filter 0, zlib stored blocks)."""
    a = _image_bytes(pixels, width, height, channels)
    n = ctypes.c_int64(0)
    _check(lib().bdpt_encode_png(a.ctypes.data, width, height, channels, None, 0, ctypes.byref(n)))
    out = np.zeros(n.value, np.uint8)
    _check(lib().bdpt_encode_png(a.ctypes.data, width, height, channels, out.ctypes.data, n.value, ctypes.byref(n)))
    return out.tobytes()


def save_png(pixels, width: int, height: int, path: str, channels: int = 3) -> None:
    a = _image_bytes(pixels, width, height, channels)
    _check(lib().bdpt_save_png(a.ctypes.data, width, height, channels, path.encode()))


def save_ppm(rgb, width: int, height: int, path: str) -> None:
    """bdpt_save_ppm: binary P6, maxval 255, the header form the texture reader accepts."""
    a = _image_bytes(rgb, width, height, 3)
    _check(lib().bdpt_save_ppm(a.ctypes.data, width, height, path.encode()))


def denoise_var_settings() -> "DenoiseSettings":
    """bdpt_denoise_var's defaults: the header's BDPT_DENOISE_VAR_ITERATIONS / _SIGMA_COLOR, the other fields
    DenoiseSettings' own."""
    return DenoiseSettings(iterations=3, sigma_color=4.0)


def denoise_var_numpy(color, var, aov, settings=None, norm=1.0, dt=np.float64):
    """What bdpt_denoise_var computes, as the header states it, every operation in `dt`: color and var (H, W, 3),
    aov (H, W, 8) -> (out (H, W, 3), out_var (H, W)) in dt."""
    f = dt
    d = settings or denoise_var_settings()
    c = np.asarray(color, np.float32).astype(dt) * f(norm)
    H, W = c.shape[:2]
    v = np.asarray(var, np.float32).reshape(H, W, 3).astype(dt) * (f(norm) * f(norm))
    av = np.asarray(aov, np.float32).reshape(H, W, 8).astype(dt) * f(norm)
    cov = av[..., 7]
    hit = cov > 0
    safe = np.where(hit, cov, f(1))
    alb = np.where(hit[..., None], av[..., 0:3] / safe[..., None], f(1))
    N = np.where(hit[..., None], av[..., 3:6] / safe[..., None], f(0))
    z = np.where(hit, av[..., 6] / safe, f(0))
    m = np.maximum(alb, f(1e-3))
    img = c / m if d.demodulate else c
    u = v / (m * m) if d.demodulate else v
    U = (u[..., 0] + u[..., 1]) + u[..., 2]

    def taps(radius, s):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                oy, ox = dy * s, dx * s
                py, px = slice(max(0, -oy), min(H, H - oy)), slice(max(0, -ox), min(W, W - ox))
                if py.start < py.stop and px.start < px.stop:
                    yield dy, dx, py, px, slice(py.start + oy, py.stop + oy), slice(px.start + ox, px.stop + ox)

    k3 = np.array([1, 2, 1], dt) / f(4)
    num, den = np.zeros((H, W), dt), np.zeros((H, W), dt)
    for dy, dx, py, px, qy, qx in taps(1, 1):
        k = k3[dy + 1] * k3[dx + 1]
        num[py, px] += k * U[qy, qx]
        den[py, px] += k
    V = num / den
    if d.iterations == 0:
        return c, V
    kern = np.array([1, 4, 6, 4, 1], dt) / f(16)
    zs = f(d.sigma_depth) * np.maximum(z, f(1e-6))
    sc2 = f(d.sigma_color) * f(d.sigma_color)
    for i in range(d.iterations):
        num, numv, den = np.zeros_like(img), np.zeros((H, W), dt), np.zeros((H, W), dt)
        for dy, dx, py, px, qy, qx in taps(2, 1 << i):
            h = kern[dy + 2] * kern[dx + 2]
            if dx == 0 and dy == 0:
                w = np.ones((H, W), dt)
            else:
                dc = img[py, px] - img[qy, qx]
                dn = N[py, px] - N[qy, qx]
                dz = z[py, px] - z[qy, qx]
                wc = np.exp(-np.minimum(((dc[..., 0] ** 2 + dc[..., 1] ** 2) + dc[..., 2] ** 2)
                                        / (sc2 * V[py, px] + f(1e-10)), f(80)))
                wn = np.exp(-np.minimum(((dn[..., 0] ** 2 + dn[..., 1] ** 2) + dn[..., 2] ** 2)
                                        / (f(d.sigma_normal) * f(d.sigma_normal)), f(80)))
                wz = np.exp(-np.minimum((dz * dz) / (zs[py, px] * zs[py, px]), f(80)))
                w = np.where(hit[py, px] == hit[qy, qx], (wc * wn) * wz, f(0))
            hw = h * w
            num[py, px] += hw[..., None] * img[qy, qx]
            numv[py, px] += (hw * hw) * V[qy, qx]
            den[py, px] += hw
        img, V = num / den[..., None], numv / (den * den)
    if d.demodulate:
        img = img * m
    assert img.dtype == dt and V.dtype == dt
    return img, V


class BDPTIntegrator:
    """GPU BDPT integrator with the reference's Integrator interface."""

    def __init__(self, scene: Scene, config: Config, device: int = 0):
        self.scene = scene
        self.config = config
        self.device = device
        h = ctypes.c_void_p()
        _check(lib().bdpt_ctx_create(scene._h, device, ctypes.byref(h)))
        self._h = h
        self.rgb = None
        self.aov = None
        self.batches = None  # render_batches' last planes
        self.var = None      # batch_moments' last variance
        self.adaptive = None  # render_adaptive's last stats

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.bdpt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def init(self) -> bool:
        self.rgb = np.zeros((self.config.height, self.config.width, 3), np.float32)
        self.aov = np.zeros((self.config.height, self.config.width, 8), np.float32)
        return True

    def params(self, row_offset: int = 0, row_stride: int = 1, flags: int = 0) -> _FrameParams:
        c = self.config
        p = _FrameParams()
        p.camera = c.camera.c()
        p.width, p.height, p.spp, p.rr_depth = c.width, c.height, c.spp, c.rr_depth
        p.strategy, p.seed_base = c.strategy, c.seed_base & 0xFFFFFFFF
        p.row_offset, p.row_stride, p.flags = row_offset, row_stride, flags
        p.russian_roulette = c.russian_roulette
        return p

    def render(self, ray: Ray, sampler: Sampler) -> np.ndarray:
        """Integrator::render(const Ray&, Sampler&) (bdpt.h:219-241): Li of one
        camera sample; its light-path splats are added to self.rgb in order; the
        sampler's std::mt19937 state advances as the reference advances it."""
        if self.rgb is None:
            self.init()
        Li, splats = self.render_sample(ray, sampler)
        rgb = self.rgb.reshape(-1, 3)
        for px, v in splats:
            rgb[px] += v
        return Li

    def render_sample(self, ray: Ray, sampler: Sampler):
        """bdpt_render_sample_mt: (Li, [(pixel, rgb float32[3]), ...]) of one sample."""
        r = (ctypes.c_float * 8)(*ray.o, *ray.d, ray.min_t, ray.max_t)
        cap = max(self.config.rr_depth, 1)
        sp = (_Splat * cap)()
        n = ctypes.c_int32(0)
        Li = (ctypes.c_float * 3)()
        p = self.params()
        st = np.ascontiguousarray(sampler.state, np.uint32)
        rc = lib().bdpt_render_sample_mt(self._h, ctypes.byref(p), r, st.ctypes.data, Li, sp, cap, ctypes.byref(n))
        if rc == -1 and n.value > cap:  # Russian roulette: more splats than rr_depth; the state is untouched
            cap = n.value
            sp = (_Splat * cap)()
            rc = lib().bdpt_render_sample_mt(self._h, ctypes.byref(p), r, st.ctypes.data, Li, sp, cap, ctypes.byref(n))
        _check(rc)
        sampler.state = st
        return np.array(Li[:], np.float32), [(sp[k].pixel, np.array(sp[k].rgb[:], np.float32)) for k in range(n.value)]

    # ---- the BSDF plugin contract and the path's building blocks (per-function entry points)
    def bsdf_eval(self, mat, wo, wi) -> np.ndarray:
        """BSDF::eval (core.h:308) of scene materials mat[k] on local directions: f * cos(wi), (n, 3)."""
        m, o, i = _ai32(mat), _af32(wo, 3), _af32(wi, 3)
        out = np.zeros((m.size, 3), np.float32)
        _check(lib().bdpt_bsdf_eval(self._h, m.size, m.ctypes.data, o.ctypes.data, i.ctypes.data, out.ctypes.data))
        return out

    def bsdf_pdf(self, mat, wo, wi) -> np.ndarray:
        """BSDF::pdf (core.h:309): the solid-angle pdf of wi, (n,)."""
        m, o, i = _ai32(mat), _af32(wo, 3), _af32(wi, 3)
        out = np.zeros(m.size, np.float32)
        _check(lib().bdpt_bsdf_pdf(self._h, m.size, m.ctypes.data, o.ctypes.data, i.ctypes.data, out.ctypes.data))
        return out

    def bsdf_sample(self, mat, wo, u):
        """BSDF::sample (core.h:310): (f * cos, wi, pdf) for samples u (n, 2)."""
        m, o, uu = _ai32(mat), _af32(wo, 3), _af32(u, 2)
        f, wi, pdf = np.zeros((m.size, 3), np.float32), np.zeros((m.size, 3), np.float32), np.zeros(m.size, np.float32)
        _check(lib().bdpt_bsdf_sample(self._h, m.size, m.ctypes.data, o.ctypes.data, uu.ctypes.data, f.ctypes.data,
                                      wi.ctypes.data, pdf.ctypes.data))
        return f, wi, pdf

    def bsdf_eval_pdfs(self, mat, wo, wi, build: str = "exact"):
        """What a connection evaluates at one end (bsdf_eval_pdfs of the frame kernels): (f * cos
        (n, 3), pdf(wi, wo) (n,), pdf(wo, wi) (n,)) on local directions. build: "exact" (IEEE
        weights), "fast" (the default frame kernels' arithmetic) or "ng" (the build without
        glossy lobes; refused for a scene with a Mixture / Phong or null BSDF)."""
        m, o, i = _ai32(mat), _af32(wo, 3), _af32(wi, 3)
        if not (m.size == o.shape[0] == i.shape[0]):
            raise ValueError("mat, wo and wi differ in length")
        out = np.zeros((m.size, 5), np.float32)
        _check(lib().bdpt_bsdf_eval_pdfs(self._h, KAT_BUILDS[build], m.size, m.ctypes.data, o.ctypes.data,
                                         i.ctypes.data, out.ctypes.data))
        return out[:, :3].copy(), out[:, 3].copy(), out[:, 4].copy()

    def bsdf_local_for(self, mat, n, v, build: str = "exact") -> np.ndarray:
        """The world directions v (n, 3) in the shading frames of the unit normals n (n, 3) as a
        connection computes them for materials mat (local_for of the frame kernels): (n, 3);
        x = y = 0 for a diffuse material."""
        m, nn, vv = _ai32(mat), _af32(n, 3), _af32(v, 3)
        if not (m.size == nn.shape[0] == vv.shape[0]):
            raise ValueError("mat, n and v differ in length")
        out = np.zeros((m.size, 3), np.float32)
        _check(lib().bdpt_bsdf_local_for(self._h, KAT_BUILDS[build], m.size, m.ctypes.data, nn.ctypes.data,
                                         vv.ctypes.data, out.ctypes.data))
        return out

    def intersect(self, rays, occlusion: bool = False, origin_normals=None, origin_tris=None) -> np.ndarray:
        """AcceleratorBVH::intersect (accel.h:125-172) or the occlusion query of
        visibilityQuery (bvh.h:259-352) on rays (n, 8): a structured bdpt_hit array.
        origin_normals (n, 3): the surfaces the rays leave (the path's interpolated
        shading normals), origin_tris (n,): their triangles (bdpt_hit.tri order, -1:
        none), for the frames' near-cull rule (bdpt_intersect_from); None: no near cull."""
        r = _af32(rays, 8)
        out = np.zeros(r.shape[0], HIT_DTYPE)
        if origin_normals is None:
            _check(lib().bdpt_intersect(self._h, r.shape[0], r.ctypes.data, 1 if occlusion else 0, out.ctypes.data))
        else:
            nr = _af32(origin_normals, 3)
            ot = None if origin_tris is None else np.ascontiguousarray(origin_tris, np.int32).reshape(-1)
            if ot is not None and ot.shape[0] != r.shape[0]:
                raise ValueError("origin_tris needs one entry per ray")
            _check(lib().bdpt_intersect_from(self._h, r.shape[0], r.ctypes.data, nr.ctypes.data,
                                             None if ot is None else ot.ctypes.data, 1 if occlusion else 0,
                                             out.ctypes.data))
        return out

    def intersect_deferred(self, rays, origin_normals=None, origin_tris=None):
        """bdpt_intersect_deferred: the closest hits of intersect() found the way the frame
        kernels without Russian roulette find them (the reference-leaf check deferred to the
        walk's winner; a winner that fails is walked again with the check in the leaf step).
        Returns (bdpt_hit array, int32 (n,) 1 where the query was walked again)."""
        r = _af32(rays, 8)
        out = np.zeros(r.shape[0], HIT_DTYPE)
        again = np.zeros(r.shape[0], np.int32)
        nr = None if origin_normals is None else _af32(origin_normals, 3)
        ot = None if origin_tris is None or nr is None else np.ascontiguousarray(origin_tris, np.int32).reshape(-1)
        if ot is not None and ot.shape[0] != r.shape[0]:
            raise ValueError("origin_tris needs one entry per ray")
        _check(lib().bdpt_intersect_deferred(self._h, r.shape[0], r.ctypes.data, None if nr is None else nr.ctypes.data,
                                             None if ot is None else ot.ctypes.data, out.ctypes.data,
                                             again.ctypes.data))
        return out, again

    def splat_to_image_plane(self, points) -> np.ndarray:
        """BDPTIntegrator::splatToImagePlane (bdpt.h:485-496) of points (n, 3): int32 (n, 2)."""
        q = _af32(points, 3)
        out = np.zeros((q.shape[0], 2), np.int32)
        p = self.params()
        _check(lib().bdpt_splat_to_image_plane(self._h, ctypes.byref(p), q.shape[0], q.ctypes.data, out.ctypes.data))
        return out

    def debug_sampling(self, fn: str, records, build: str = "exact", placement: str = "ctx") -> np.ndarray:
        """bdpt_debug_sampling: one of SAMPLING_FNS on records (n, words in) of 32-bit words
        (uint32; floats and ints by their bits), through the frame kernels' device functions:
        uint32 (n, words out). "camera" uses this integrator's camera, width, height and spp.
        build: "exact" or "fast"; placement ("ctx", "hbm", "lds"): where "cdf" and "emitter"
        read the emitter faces and CDFs."""
        code, nin, nout = SAMPLING_FNS[fn]
        rec = np.ascontiguousarray(records, np.uint32).reshape(-1, nin)
        out = np.zeros((rec.shape[0], nout), np.uint32)
        p = self.params()
        _check(lib().bdpt_debug_sampling(self._h, ctypes.byref(p), KAT_BUILDS[build], code,
                                         EMITTER_PLACEMENTS[placement], rec.shape[0], rec.ctypes.data,
                                         out.ctypes.data, None))
        return out

    def emitter_placement(self) -> str:
        """Where this context's frames read the emitter faces and CDFs: "lds" or "hbm"."""
        got = ctypes.c_int32(-1)
        _check(lib().bdpt_debug_sampling(self._h, None, 0, 0, 0, 0, None, None, ctypes.byref(got)))
        return {v: k for k, v in EMITTER_PLACEMENTS.items()}[got.value]

    def _integrator_params(self):
        """(bdpt_path_params, bdpt_direct_params) of bdpt_render_window: None, None = BDPT."""
        return None, None

    def render_frame(self, row_offset: int = 0, row_stride: int = 1, flags: int = 0,
                     window: SampleWindow | None = None) -> np.ndarray:
        """All pixels x spp of the (sharded) image into self.rgb (host copy); with a
        window only its samples of every pixel. bdpt_render_window_host with this
        integrator's settings: without a window exactly bdpt_render[_path|_direct]_host."""
        if self.rgb is None:
            self.init()
        p = self.params(row_offset, row_stride, flags)
        pp, dp = self._integrator_params()
        w = window and window.c()
        _check(lib().bdpt_render_window_host(self._h, ctypes.byref(p), w and ctypes.byref(w), pp and ctypes.byref(pp),
                                             dp and ctypes.byref(dp), self.rgb.ctypes.data))
        return self.rgb

    def render_device(self, fb_ptr: int, stream_ptr: int = 0, row_offset: int = 0, row_stride: int = 1,
                      flags: int = 0, window: SampleWindow | None = None) -> None:
        """Asynchronous render into a device framebuffer (e.g. a torch tensor's data_ptr()):
        bdpt_render_window, as render_frame calls its host form."""
        p = self.params(row_offset, row_stride, flags)
        pp, dp = self._integrator_params()
        w = window and window.c()
        _check(lib().bdpt_render_window(self._h, ctypes.byref(p), w and ctypes.byref(w), pp and ctypes.byref(pp),
                                        dp and ctypes.byref(dp), ctypes.c_void_p(fb_ptr),
                                        ctypes.c_void_p(stream_ptr)))

    def render_progressive(self, batch: int):
        """Generator: renders the contiguous sample windows [0, batch), [batch, 2 batch), ...
        into self.rgb (zeroed first) and yields (done_spp, preview) after each, with preview =
        self.rgb * (spp / done_spp). Every contribution of a sample, light-path splats
        included, carries 1 / spp, so the preview is the unbiased estimate from the samples
        so far; the last item has done_spp == spp and the full frame (the same samples as
        render_frame()).

        Denoised previews (the feature buffers accumulate over the same windows; samples_done
        gives the filter its norm = spp / done)::

            done0 = 0
            for done, _ in it.render_progressive(4):
                it.render_aov(window=SampleWindow(done0, 1, done - done0))
                show(it.denoise(samples_done=done))
                done0 = done
        """
        if batch < 1:
            raise ValueError("render_progressive: batch must be >= 1")
        spp = self.config.spp
        self.init()
        done = 0
        while done < spp:
            n = min(batch, spp - done)
            self.render_frame(window=SampleWindow(done, 1, n))
            done += n
            yield done, (self.rgb if done == spp else self.rgb * np.float32(spp / done))

    def render_batches(self, n_batches: int, window: SampleWindow | None = None, row_offset: int = 0,
                       row_stride: int = 1) -> np.ndarray:
        """The frame (or the window's samples of it) as n_batches complete, independent estimates: a new
        (n_batches, H, W, 3) array, plane b bdpt_render_window_host of batch_windows()[b] into zeros, with this
        integrator's settings as render_frame passes them. The planes sum to render_frame(window=window) up to
        the order of the float additions; batch_moments() turns them into that sum and its per-pixel variance.
        Kept in self.batches."""
        wins = batch_windows(self.config.spp, n_batches, window)
        H, W = self.config.height, self.config.width
        p = self.params(row_offset, row_stride, 0)
        pp, dp = self._integrator_params()
        out = np.zeros((len(wins), H, W, 3), np.float32)
        for b, win in enumerate(wins):
            w = win.c()
            _check(lib().bdpt_render_window_host(self._h, ctypes.byref(p), ctypes.byref(w), pp and ctypes.byref(pp),
                                                 dp and ctypes.byref(dp), out[b].ctypes.data))
        self.batches = out
        return out

    def render_batches_device(self, n_batches: int, planes_ptr: int, stream_ptr: int = 0,
                              window: SampleWindow | None = None, row_offset: int = 0, row_stride: int = 1) -> None:
        """render_batches with bdpt_render_window: asynchronous, plane b ADDED to the b-th H * W * 3 floats of a
        device buffer (zero it first)."""
        wins = batch_windows(self.config.spp, n_batches, window)
        p = self.params(row_offset, row_stride, 0)
        pp, dp = self._integrator_params()
        plane_bytes = self.config.height * self.config.width * 3 * 4
        for b, win in enumerate(wins):
            w = win.c()
            _check(lib().bdpt_render_window(self._h, ctypes.byref(p), ctypes.byref(w), pp and ctypes.byref(pp),
                                            dp and ctypes.byref(dp), ctypes.c_void_p(planes_ptr + b * plane_bytes),
                                            ctypes.c_void_p(stream_ptr)))

    def batch_moments(self, planes=None):
        """bdpt_batch_moments_host of (K, H, W, 3) batch planes (default self.batches, render_batches' last):
        (sum, var), both (H, W, 3): the frame of the batches' samples and the estimated variance of each of its
        values. Also sets self.rgb = sum and self.var = var, what denoise_var() reads by default."""
        if planes is None:
            planes = getattr(self, "batches", None)
            if planes is None:
                raise BdptError("batch_moments: no planes given and render_batches has not run")
        a = np.ascontiguousarray(planes, np.float32)
        if a.ndim != 4 or a.shape[3] != 3:
            raise BdptError(f"batch_moments: planes must be (n_batches, H, W, 3), got {a.shape}")
        K, H, W = a.shape[:3]
        s, v = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
        _check(lib().bdpt_batch_moments_host(self._h, W, H, K, a.ctypes.data, s.ctypes.data, v.ctypes.data))
        self.rgb, self.var = s, v
        return s, v

    def batch_moments_device(self, planes_ptr: int, n_batches: int, width: int, height: int, sum_ptr: int, var_ptr: int,
                             stream_ptr: int = 0) -> None:
        """bdpt_batch_moments: asynchronous, on device buffers (sum_ptr 0: the sum is not wanted)."""
        _check(lib().bdpt_batch_moments(self._h, int(width), int(height), int(n_batches), ctypes.c_void_p(planes_ptr),
                                        ctypes.c_void_p(sum_ptr or None), ctypes.c_void_p(var_ptr),
                                        ctypes.c_void_p(stream_ptr)))

    # ---- adaptive sampling
    def render_pixels(self, pixels, window: SampleWindow | None = None, out=None, row_offset: int = 0,
                      row_stride: int = 1, flags: int = 0) -> np.ndarray:
        """bdpt_render_pixels_host: the window's samples (None: all spp) of the listed pixels only, ADDED to
        `out` (None: a new zeroed array), a (2, H, W, 3) float32 array that is returned: out[0] the camera
        splats of those samples' light paths, out[1] everything formed at the samples' own pixels (untouched
        at unlisted pixels). pixels: int32 indices y * W + x, strictly ascending; the library checks them."""
        H, W = self.config.height, self.config.width
        px = np.ascontiguousarray(pixels, np.int32).reshape(-1)
        if out is None:
            out = np.zeros((2, H, W, 3), np.float32)
        if out.dtype != np.float32 or out.shape != (2, H, W, 3) or not out.flags.c_contiguous:
            raise BdptError(f"render_pixels: out must be a contiguous float32 (2, {H}, {W}, 3) array")
        p = self.params(row_offset, row_stride, flags)
        w = window.c() if window is not None else None
        _check(lib().bdpt_render_pixels_host(self._h, ctypes.byref(p), w and ctypes.byref(w),
                                             px.ctypes.data if px.size else None, int(px.size), out.ctypes.data))
        return out

    def render_pixels_device(self, pixels_ptr: int, n_pixels: int, fb_ptr: int, window: SampleWindow | None = None,
                             stream_ptr: int = 0) -> None:
        """bdpt_render_pixels: asynchronous, ADDED to a device buffer of 2 * H * W * 3 floats. The list is a
        device array the library TRUSTS (inside the image, strictly ascending): pass only what adaptive_select
        wrote or what was checked as render_pixels checks."""
        p = self.params()
        w = window.c() if window is not None else None
        _check(lib().bdpt_render_pixels(self._h, ctypes.byref(p), w and ctypes.byref(w), ctypes.c_void_p(pixels_ptr or None),
                                        int(n_pixels), ctypes.c_void_p(fb_ptr), ctypes.c_void_p(stream_ptr)))

    def adaptive_resolve(self, planes, m, spp: int | None = None):
        """bdpt_adaptive_resolve_host of (K, 2, H, W, 3) plane pairs and the (H, W) int32 samples per batch:
        (S, var), both (H, W, 3); the bits of adaptive_resolve_numpy."""
        a = np.ascontiguousarray(planes, np.float32)
        if a.ndim != 5 or a.shape[1] != 2 or a.shape[4] != 3:
            raise BdptError(f"adaptive_resolve: planes must be (n_batches, 2, H, W, 3), got {a.shape}")
        K, _, H, W, _ = a.shape
        mm = np.ascontiguousarray(m, np.int32).reshape(H, W)
        S, v = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
        _check(lib().bdpt_adaptive_resolve_host(self._h, W, H, K, int(self.config.spp if spp is None else spp),
                                                a.ctypes.data, mm.ctypes.data, -1, S.ctypes.data, v.ctypes.data))
        return S, v

    def adaptive_resolve_device(self, planes_ptr: int, m_ptr: int, n_batches: int, splat_total: int, sum_ptr: int,
                                var_ptr: int, spp: int | None = None, stream_ptr: int = 0) -> None:
        """bdpt_adaptive_resolve: asynchronous, on device buffers; splat_total = the sum of m, counted by the caller."""
        _check(lib().bdpt_adaptive_resolve(self._h, self.config.width, self.config.height, int(n_batches),
                                           int(self.config.spp if spp is None else spp), ctypes.c_void_p(planes_ptr),
                                           ctypes.c_void_p(m_ptr), int(splat_total), ctypes.c_void_p(sum_ptr),
                                           ctypes.c_void_p(var_ptr), ctypes.c_void_p(stream_ptr)))

    def adaptive_select_device(self, sum_ptr: int, var_ptr: int, m_ptr: int, list_ptr: int, count_ptr: int,
                               threshold: float, eps: float, step: int, m_max: int, dilate: bool = True,
                               stream_ptr: int = 0) -> None:
        """bdpt_adaptive_select: asynchronous, on device buffers (list: W * H int32, count: one int32)."""
        _check(lib().bdpt_adaptive_select(self._h, self.config.width, self.config.height, ctypes.c_void_p(sum_ptr),
                                          ctypes.c_void_p(var_ptr), float(threshold), float(eps), int(step), int(m_max),
                                          int(bool(dilate)), ctypes.c_void_p(m_ptr), ctypes.c_void_p(list_ptr),
                                          ctypes.c_void_p(count_ptr), ctypes.c_void_p(stream_ptr)))

    def adaptive_select(self, S, var, m, threshold: float, eps: float, step: int, m_max: int, dilate: bool = True):
        """bdpt_adaptive_select_host: (list int32 ascending, m_new (H, W) int32); adaptive_select_numpy's."""
        s = np.ascontiguousarray(S, np.float32)
        v = np.ascontiguousarray(var, np.float32)
        if s.ndim != 3 or s.shape[2] != 3 or v.shape != s.shape:
            raise BdptError(f"adaptive_select: S and var must both be (H, W, 3), got {s.shape} and {v.shape}")
        H, W = s.shape[:2]
        mm = np.array(m, np.int32).reshape(H, W)  # a copy: the library updates it
        lst = np.zeros(H * W, np.int32)
        n = ctypes.c_int32(0)
        _check(lib().bdpt_adaptive_select_host(self._h, W, H, s.ctypes.data, v.ctypes.data, float(threshold), float(eps),
                                               int(step), int(m_max), int(bool(dilate)), mm.ctypes.data, lst.ctypes.data,
                                               ctypes.byref(n)))
        return lst[:n.value].copy(), mm

    def render_adaptive(self, threshold: float, n_batches: int = 8, step: int = 1, max_passes: int | None = None,
                        eps: float = ADAPTIVE_EPS, dilate: bool = True, return_passes: bool = False):
        """bdpt_render_adaptive_host: the frame with further samples only where the batch variance asks. The
        budget is config.spp = max_passes * step * n_batches samples per pixel (max_passes None: spp /
        (step * n_batches)). Pass 0 gives every pixel step * n_batches samples; a pixel then stays active while
        its relative standard deviation, estimated from the n_batches batches, exceeds `threshold` (or, with
        dilate, a neighbour's does) and its budget lasts. Returns (frame (H, W, 3), variance (H, W, 3), samples
        (H, W) int32) and, with return_passes, the list of active pixel indices of every pass. Also sets self.rgb,
        self.var and self.adaptive (passes, samples traced, active pixels per pass). threshold = 0 is the
        unbiased frame: choosing samples from the estimate they feed biases it, as in every such sampler."""
        H, W = self.config.height, self.config.width
        a = _AdaptiveParams()
        a.n_batches, a.step = int(n_batches), int(step)
        a.max_passes = int(max_passes) if max_passes is not None else self.config.spp // max(1, int(step) * int(n_batches))
        a.threshold, a.eps, a.dilate, a.record_passes = float(threshold), float(eps), int(bool(dilate)), int(bool(return_passes))
        frame, var = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
        samples = np.zeros((H, W), np.int32)
        st = _AdaptiveStats()
        p = self.params()
        _check(lib().bdpt_render_adaptive_host(self._h, ctypes.byref(p), ctypes.byref(a), frame.ctypes.data,
                                               var.ctypes.data, samples.ctypes.data, ctypes.byref(st)))
        self.rgb, self.var = frame, var
        self.adaptive = dict(passes=st.passes, samples=st.samples, active=list(st.active[:st.passes]))
        if not return_passes:
            return frame, var, samples
        total = ctypes.c_int64(0)
        _check(lib().bdpt_adaptive_pass_lists(self._h, None, 0, ctypes.byref(total)))
        flat = np.zeros(max(total.value, 1), np.int32)
        _check(lib().bdpt_adaptive_pass_lists(self._h, flat.ctypes.data, flat.size, ctypes.byref(total)))
        cuts = np.cumsum([0] + self.adaptive["active"])
        return frame, var, samples, [flat[cuts[j]:cuts[j + 1]].copy() for j in range(st.passes)]

    def render_aov(self, row_offset: int = 0, row_stride: int = 1, window: SampleWindow | None = None) -> np.ndarray:
        """bdpt_render_aov_host: the first-hit feature buffers of the (sharded, windowed) frame
        ADDED to self.aov, (H, W, 8) = albedo rgb, shading normal xyz, t, coverage, each
        weighted 1 / spp as render_frame weights self.rgb."""
        if self.aov is None:
            self.init()
        p = self.params(row_offset, row_stride, 0)
        w = window.c() if window is not None else None
        _check(lib().bdpt_render_aov_host(self._h, ctypes.byref(p), w and ctypes.byref(w), self.aov.ctypes.data))
        return self.aov

    def render_aov_device(self, aov_ptr: int, stream_ptr: int = 0, row_offset: int = 0, row_stride: int = 1,
                          window: SampleWindow | None = None) -> None:
        """bdpt_render_aov: asynchronous, into a device buffer of W * H * 8 floats."""
        p = self.params(row_offset, row_stride, 0)
        w = window.c() if window is not None else None
        _check(lib().bdpt_render_aov(self._h, ctypes.byref(p), w and ctypes.byref(w), ctypes.c_void_p(aov_ptr),
                                     ctypes.c_void_p(stream_ptr)))

    def _render_planes(self, entry, args, planes, ok, window, row_offset, row_stride, flags, fb_ptr=None, stream_ptr=0):
        """One plane render (layers, light groups, strategies, the crossed kinds): entry(ctx, params, window, *args, fb[, stream]).
        planes None: the device entry, ADDED to fb_ptr. Otherwise the host entry into a new planes + (H, W, 3)
        array, which is returned; a count the library refuses (ok false) or a size it refuses, both before it
        touches the buffer, is not allocated here."""
        H, W = self.config.height, self.config.width
        p = self.params(row_offset, row_stride, flags)
        w = window.c() if window is not None else None
        if planes is None:
            _check(entry(self._h, ctypes.byref(p), w and ctypes.byref(w), *args, ctypes.c_void_p(fb_ptr),
                         ctypes.c_void_p(stream_ptr)))
            return None
        ok = ok and math.prod(planes) * W * H < PLANE_PIXELS_MAX
        out = np.zeros(tuple(planes) + (H, W, 3) if ok else (1,), np.float32)
        _check(entry(self._h, ctypes.byref(p), w and ctypes.byref(w), *args, out.ctypes.data))
        return out

    def render_layers(self, n_layers: int, window: SampleWindow | None = None, row_offset: int = 0,
                      row_stride: int = 1, flags: int = 0) -> np.ndarray:
        """bdpt_render_layers_host: the BDPT frame split by path length, a new (n_layers, H, W, 3)
        array. Layer l holds the contributions of paths camera -> ... -> emitter with l + 1 edges
        (0: emitters seen directly, 1: direct light, ...), the last layer everything longer; the
        layers sum to render_frame()'s frame."""
        n_layers = int(n_layers)
        return self._render_planes(lib().bdpt_render_layers_host, (n_layers,), (n_layers,), 1 <= n_layers <= LAYERS_MAX,
                                   window, row_offset, row_stride, flags)

    def render_layers_device(self, n_layers: int, fb_ptr: int, stream_ptr: int = 0,
                             window: SampleWindow | None = None, row_offset: int = 0, row_stride: int = 1) -> None:
        """bdpt_render_layers: asynchronous, ADDED to a device buffer of n_layers * H * W * 3 floats."""
        self._render_planes(lib().bdpt_render_layers, (int(n_layers),), None, True, window, row_offset, row_stride, 0,
                            fb_ptr, stream_ptr)

    @staticmethod
    def layer_mask(mask_or_iterable) -> int:
        """A 64-bit layer mask from an int (taken as is) or an iterable of layer indices."""
        if isinstance(mask_or_iterable, (int, np.integer)):
            m = int(mask_or_iterable)
            if m < 0 or m >= 1 << 64:
                raise ValueError("layer mask: an int mask must fit 64 bits")
            return m
        m = 0
        for l in mask_or_iterable:
            if not 0 <= int(l) < 64:
                raise ValueError(f"layer mask: layer {l} is outside 0..63")
            m |= 1 << int(l)
        return m

    def _combine(self, a, out_shape, call) -> np.ndarray:
        """The round trip of compose_layers, relight, strategies_sheet and combine_group_planes: the contiguous float32 planes go to
        the device, call(planes pointer, out pointer) runs the device form on them, the result comes back."""
        import torch

        dev = torch.device("cuda", self.device)
        d_in = torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
        d_out = torch.zeros(out_shape, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        call(d_in.data_ptr(), d_out.data_ptr())
        self.synchronize()
        return d_out.cpu().numpy()

    @staticmethod
    def _gains(entry, gains, planes, shape):
        """Host gains as a combine entry takes them: contiguous float32, 3 per plane (shape: how the message says it)."""
        g = np.ascontiguousarray(gains, np.float32)
        if g.size != 3 * planes:
            raise BdptError(f"{entry}: gains must hold {shape} x 3 floats, got {g.size}")
        return g

    def compose_layers(self, layers, mask_or_iterable) -> np.ndarray:
        """bdpt_layers_compose on the device: the (H, W, 3) float32 sum of the layers the mask
        names (an int bit mask or an iterable of layer indices), added in ascending layer order.
        The layers go to the device and the sum comes back (a viewer that keeps the planes on
        the device calls compose_layers_device)."""
        a = np.ascontiguousarray(layers, np.float32)
        if a.ndim != 4 or a.shape[3] != 3:
            raise BdptError(f"compose_layers: layers must be (n_layers, H, W, 3), got {a.shape}")
        n, H, W = a.shape[:3]
        mask = self.layer_mask(mask_or_iterable)
        return self._combine(a, (H, W, 3), lambda d_in, d_out: self.compose_layers_device(d_in, n, W, H, mask, d_out))

    def compose_layers_device(self, layers_ptr: int, n_layers: int, width: int, height: int, mask: int, out_ptr: int,
                              stream_ptr: int = 0) -> None:
        """bdpt_layers_compose: asynchronous, on device buffers."""
        _check(lib().bdpt_layers_compose(self._h, ctypes.c_void_p(layers_ptr), int(n_layers), int(width), int(height),
                                         ctypes.c_uint64(mask), ctypes.c_void_p(out_ptr),
                                         ctypes.c_void_p(stream_ptr)))

    def _group_map(self, group_of_emitter, n_groups, entry="render_light_groups"):
        """(int32 array or None, n_groups) as bdpt_render_light_groups takes them: no map is the
        identity, whose plane count defaults to the emitter count; with a map it defaults to
        max(map) + 1."""
        if group_of_emitter is None:
            n = len(self.scene.emitters()) if n_groups is None else int(n_groups)
            return None, n
        m = np.ascontiguousarray(group_of_emitter, np.int32).reshape(-1)
        if m.size != len(self.scene.emitters()):
            raise BdptError(f"{entry}: group_of_emitter has {m.size} entries, the scene "
                            f"{len(self.scene.emitters())} emitters")
        return m, (int(m.max()) + 1 if n_groups is None else int(n_groups))

    def render_light_groups(self, group_of_emitter=None, n_groups: int | None = None, window: SampleWindow | None = None,
                            row_offset: int = 0, row_stride: int = 1, flags: int = 0) -> np.ndarray:
        """bdpt_render_light_groups_host: the BDPT frame split by emitter, a new (n_groups, H, W, 3)
        array. Plane g holds the contributions of the paths that end on an emitter e with
        group_of_emitter[e] == g (Scene.emitters() order; None: one plane per emitter); the planes
        sum to render_frame()'s frame, and relight() recombines them under other emitter colours."""
        m, n = self._group_map(group_of_emitter, n_groups)
        return self._render_planes(lib().bdpt_render_light_groups_host, (n, None if m is None else m.ctypes.data), (n,),
                                   1 <= n <= GROUPS_MAX, window, row_offset, row_stride, flags)

    def render_light_groups_device(self, fb_ptr: int, group_of_emitter=None, n_groups: int | None = None,
                                   stream_ptr: int = 0, window: SampleWindow | None = None, row_offset: int = 0,
                                   row_stride: int = 1) -> None:
        """bdpt_render_light_groups: asynchronous, ADDED to a device buffer of n_groups * H * W * 3 floats."""
        m, n = self._group_map(group_of_emitter, n_groups)
        self._render_planes(lib().bdpt_render_light_groups, (n, None if m is None else m.ctypes.data), None, True, window,
                            row_offset, row_stride, 0, fb_ptr, stream_ptr)

    def relight(self, groups, gains) -> np.ndarray:
        """bdpt_light_groups_relight on the device: the (H, W, 3) float32 frame sum_g gains[g] *
        groups[g] (gains: (n_groups, 3) RGB, or (n_groups,) for grey gains), each product and sum
        rounded in float32 in ascending group order. The planes go to the device and the frame
        comes back (a viewer that keeps the planes on the device calls relight_device)."""
        a = np.ascontiguousarray(groups, np.float32)
        if a.ndim != 4 or a.shape[3] != 3:
            raise BdptError(f"relight: groups must be (n_groups, H, W, 3), got {a.shape}")
        n, H, W = a.shape[:3]
        g = np.asarray(gains, np.float32)
        if g.ndim == 1:
            g = np.repeat(g[:, None], 3, axis=1)
        if g.shape != (n, 3):
            raise BdptError(f"relight: gains must be ({n}, 3) or ({n},), got {g.shape}")
        return self._combine(a, (H, W, 3), lambda d_in, d_out: self.relight_device(d_in, n, W, H, g, d_out))

    def relight_device(self, groups_ptr: int, n_groups: int, width: int, height: int, gains, out_ptr: int,
                       stream_ptr: int = 0) -> None:
        """bdpt_light_groups_relight: asynchronous, on device buffers; gains: host (n_groups, 3) float32."""
        g = self._gains("relight_device", gains, int(n_groups), n_groups)
        _check(lib().bdpt_light_groups_relight(self._h, ctypes.c_void_p(groups_ptr), int(n_groups), int(width),
                                               int(height), g.ctypes.data, ctypes.c_void_p(out_ptr),
                                               ctypes.c_void_p(stream_ptr)))

    def _strategies_shape(self, n_s, n_t):
        if n_s is None or n_t is None:  # (a given shape reaches the library as it is)
            d_s, d_t = strategies_shape(self.config.rr_depth, self.config.strategy)
            return (d_s if n_s is None else int(n_s)), (d_t if n_t is None else int(n_t))
        return int(n_s), int(n_t)

    def render_strategies(self, n_s: int | None = None, n_t: int | None = None, unweighted: bool = False,
                          window: SampleWindow | None = None, row_offset: int = 0, row_stride: int = 1,
                          flags: int = 0) -> np.ndarray:
        """bdpt_render_strategies_host: the BDPT frame split by sampling strategy, a new
        (n_s, n_t, H, W, 3) array. out[s, t - 1] holds the contributions formed with s light-subpath
        and t eye-subpath vertices (the camera counted), the last row and column everything longer;
        the default shape, strategies_shape(rr_depth, strategy), clamps nothing. Weighted, the planes
        sum to render_frame()'s frame; unweighted, no contribution carries its MIS weight and each
        plane is its strategy's plain estimator. `unweighted` may also be a STRATEGIES_* value."""
        n_s, n_t = self._strategies_shape(n_s, n_t)
        return self._render_planes(lib().bdpt_render_strategies_host, (n_s, n_t, int(unweighted)), (n_s, n_t),
                                   1 <= n_s <= STRATEGIES_MAX_S and 1 <= n_t <= STRATEGIES_MAX_T, window, row_offset,
                                   row_stride, flags)

    def render_strategies_device(self, fb_ptr: int, n_s: int | None = None, n_t: int | None = None,
                                 unweighted: bool = False, stream_ptr: int = 0, window: SampleWindow | None = None,
                                 row_offset: int = 0, row_stride: int = 1) -> None:
        """bdpt_render_strategies: asynchronous, ADDED to a device buffer of n_s * n_t * H * W * 3 floats."""
        n_s, n_t = self._strategies_shape(n_s, n_t)
        self._render_planes(lib().bdpt_render_strategies, (n_s, n_t, int(unweighted)), None, True, window, row_offset,
                            row_stride, 0, fb_ptr, stream_ptr)

    def strategies_sheet(self, planes, gains=None) -> np.ndarray:
        """bdpt_strategies_sheet on the device: the contact sheet of render_strategies' planes, an
        (n_t * H, n_s * W, 3) float32 image with the tile of (s, t) at tile column s, tile row t - 1,
        each tile times its gain (gains: (n_s, n_t, 3) RGB or (n_s, n_t) grey; None: copied). The
        bits of strategies_sheet_numpy. The planes go to the device and the sheet comes back."""
        a, g = _sheet_args(planes, gains)
        n_s, n_t, H, W = a.shape[:4]
        return self._combine(a, (n_t * H, n_s * W, 3),
                             lambda d_in, d_out: self.strategies_sheet_device(d_in, n_s, n_t, W, H, g, d_out))

    def strategies_sheet_device(self, planes_ptr: int, n_s: int, n_t: int, width: int, height: int, gains,
                                out_ptr: int, stream_ptr: int = 0) -> None:
        """bdpt_strategies_sheet: asynchronous, on device buffers; gains: None or host n_s * n_t x 3 float32."""
        g = None if gains is None else self._gains("strategies_sheet_device", gains, int(n_s) * int(n_t), f"{n_s} x {n_t}")
        _check(lib().bdpt_strategies_sheet(self._h, ctypes.c_void_p(planes_ptr), int(n_s), int(n_t), int(width),
                                           int(height), None if g is None else g.ctypes.data,
                                           ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream_ptr)))

    def render_group_layers(self, n_layers: int, group_of_emitter=None, n_groups: int | None = None,
                            window: SampleWindow | None = None, row_offset: int = 0, row_stride: int = 1,
                            flags: int = 0) -> np.ndarray:
        """bdpt_render_group_layers_host: the BDPT frame split by emitter and by path length at once, a
        new (n_groups, n_layers, H, W, 3) array. out[g, l] holds the contributions of the paths of l + 1
        edges (the last layer: everything longer) that end on an emitter of group g; summed over l it is
        render_light_groups(), summed over g render_layers(n_layers)."""
        m, n = self._group_map(group_of_emitter, n_groups, "render_group_layers")
        n_layers = int(n_layers)
        return self._render_planes(lib().bdpt_render_group_layers_host, (None if m is None else m.ctypes.data, n, n_layers),
                                   (n, n_layers), 1 <= n <= GROUPS_MAX and 1 <= n_layers <= LAYERS_MAX, window,
                                   row_offset, row_stride, flags)

    def render_group_layers_device(self, n_layers: int, fb_ptr: int, group_of_emitter=None, n_groups: int | None = None,
                                   stream_ptr: int = 0, window: SampleWindow | None = None, row_offset: int = 0,
                                   row_stride: int = 1) -> None:
        """bdpt_render_group_layers: asynchronous, ADDED to a device buffer of n_groups * n_layers * H * W * 3 floats."""
        m, n = self._group_map(group_of_emitter, n_groups, "render_group_layers")
        self._render_planes(lib().bdpt_render_group_layers, (None if m is None else m.ctypes.data, n, int(n_layers)), None,
                            True, window, row_offset, row_stride, 0, fb_ptr, stream_ptr)

    def render_group_strategies(self, n_s: int | None = None, n_t: int | None = None, unweighted: bool = False,
                                group_of_emitter=None, n_groups: int | None = None, window: SampleWindow | None = None,
                                row_offset: int = 0, row_stride: int = 1, flags: int = 0) -> np.ndarray:
        """bdpt_render_group_strategies_host: the BDPT frame split by emitter and by sampling strategy at
        once, a new (n_groups, n_s, n_t, H, W, 3) array. out[g] is render_strategies(n_s, n_t, unweighted)
        of the light that ends on group g's emitters; summed over g it is that render, summed over (s, t)
        of a weighted render it is render_light_groups()."""
        m, n = self._group_map(group_of_emitter, n_groups, "render_group_strategies")
        n_s, n_t = self._strategies_shape(n_s, n_t)
        return self._render_planes(lib().bdpt_render_group_strategies_host,
                                   (None if m is None else m.ctypes.data, n, n_s, n_t, int(unweighted)), (n, n_s, n_t),
                                   1 <= n <= GROUPS_MAX and 1 <= n_s <= STRATEGIES_MAX_S and 1 <= n_t <= STRATEGIES_MAX_T,
                                   window, row_offset, row_stride, flags)

    def render_group_strategies_device(self, fb_ptr: int, n_s: int | None = None, n_t: int | None = None,
                                       unweighted: bool = False, group_of_emitter=None, n_groups: int | None = None,
                                       stream_ptr: int = 0, window: SampleWindow | None = None, row_offset: int = 0,
                                       row_stride: int = 1) -> None:
        """bdpt_render_group_strategies: asynchronous, ADDED to a device buffer of n_groups * n_s * n_t * H * W * 3 floats."""
        m, n = self._group_map(group_of_emitter, n_groups, "render_group_strategies")
        n_s, n_t = self._strategies_shape(n_s, n_t)
        self._render_planes(lib().bdpt_render_group_strategies,
                            (None if m is None else m.ctypes.data, n, n_s, n_t, int(unweighted)), None, True, window,
                            row_offset, row_stride, 0, fb_ptr, stream_ptr)

    def combine_group_planes(self, planes, gains=None, weights=None) -> np.ndarray:
        """bdpt_group_planes_combine on the device: the (H, W, 3) float32 frame sum_g sum_j gains[g] *
        weights[j] * planes[g, j] of render_group_layers' or render_group_strategies' planes (gains:
        (n_groups, 3) RGB or (n_groups,) grey; weights: the inner axes' shape or flat; None: ones). The
        bits of combine_group_planes_numpy. The planes go to the device and the frame comes back."""
        a, g, w = _group_planes_args(planes, gains, weights)
        n, n_inner, H, W = a.shape[:4]
        return self._combine(a, (H, W, 3),
                             lambda d_in, d_out: self.combine_group_planes_device(d_in, n, n_inner, W, H, g, w, d_out))

    def combine_group_planes_device(self, planes_ptr: int, n_groups: int, n_inner: int, width: int, height: int, gains,
                                    weights, out_ptr: int, stream_ptr: int = 0) -> None:
        """bdpt_group_planes_combine: asynchronous, on device buffers; gains: None or host n_groups x 3
        float32, weights: None or host n_inner float32."""
        g = None if gains is None else self._gains("combine_group_planes_device", gains, int(n_groups), n_groups)
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        if w is not None and w.size != int(n_inner):
            raise BdptError(f"combine_group_planes_device: weights must hold {n_inner} floats, got {w.size}")
        _check(lib().bdpt_group_planes_combine(self._h, ctypes.c_void_p(planes_ptr), int(n_groups), int(n_inner),
                                               int(width), int(height), None if g is None else g.ctypes.data,
                                               None if w is None else w.ctypes.data, ctypes.c_void_p(out_ptr),
                                               ctypes.c_void_p(stream_ptr)))

    def denoise(self, rgb=None, aov=None, samples_done: int | None = None, **params) -> np.ndarray:
        """bdpt_denoise_host of rgb (default self.rgb) guided by aov (default self.aov): a new
        (H, W, 3) array. samples_done: the samples per pixel both hold so far (norm = spp /
        samples_done; None = a full frame, norm 1). params: DenoiseSettings fields, or
        settings=DenoiseSettings(...)."""
        H, W = self.config.height, self.config.width
        settings = params.pop("settings", None) or DenoiseSettings()
        if params:
            from dataclasses import replace
            settings = replace(settings, **params)
        if samples_done is not None and samples_done < 1:
            raise ValueError("denoise: samples_done must be >= 1")
        norm = 1.0 if samples_done is None else self.config.spp / samples_done
        c = np.ascontiguousarray(self.rgb if rgb is None else rgb, np.float32)
        a = np.ascontiguousarray(self.aov if aov is None else aov, np.float32)
        if c.size != W * H * 3 or a.size != W * H * 8:
            raise BdptError(f"denoise: rgb / aov have {c.size} / {a.size} floats, expected {W * H * 3} / {W * H * 8}")
        out = np.zeros((H, W, 3), np.float32)
        d = settings.c(norm)
        _check(lib().bdpt_denoise_host(self._h, W, H, c.ctypes.data, a.ctypes.data, out.ctypes.data, ctypes.byref(d)))
        return out

    def denoise_device(self, rgb_ptr: int, aov_ptr: int, out_ptr: int, stream_ptr: int = 0, norm: float = 1.0,
                       settings: "DenoiseSettings | None" = None) -> None:
        """bdpt_denoise: asynchronous, on device buffers."""
        d = (settings or DenoiseSettings()).c(norm)
        _check(lib().bdpt_denoise(self._h, self.config.width, self.config.height, ctypes.c_void_p(rgb_ptr),
                                  ctypes.c_void_p(aov_ptr), ctypes.c_void_p(out_ptr), ctypes.byref(d),
                                  ctypes.c_void_p(stream_ptr)))

    def primary_directions(self) -> np.ndarray:
        """The primary ray direction of every pixel at spp 1 (the pixel centre, no jitter draws), through the
        frame kernels' own camera function (bdpt_debug_sampling's camera entry): float32 (H, W, 3). What
        bdpt_reproject forms its world points from, and reproject_numpy's `dirs`."""
        H, W = self.config.height, self.config.width
        rec = np.zeros((H * W, 3), np.uint32)
        rec[:, 0] = np.arange(H * W, dtype=np.uint32)
        out = np.zeros((H * W, 3), np.uint32)
        p = self.params()
        p.spp = 1
        code = SAMPLING_FNS["camera"][0]
        _check(lib().bdpt_debug_sampling(self._h, ctypes.byref(p), KAT_BUILDS["exact"], code, EMITTER_PLACEMENTS["ctx"],
                                         H * W, rec.ctypes.data, out.ctypes.data, None))
        return out.view(np.float32).reshape(H, W, 3)

    def _reproject_params(self, prev_camera, samples_done, params):
        settings = params.pop("settings", None) or ReprojectSettings()
        if params:
            from dataclasses import replace
            settings = replace(settings, **params)
        if samples_done is not None and samples_done < 1:
            raise ValueError("reproject: samples_done must be >= 1")
        n_c = self.config.spp if samples_done is None else samples_done
        return settings.c(prev_camera, n_c, self.config.spp / n_c)

    def reproject(self, prev_camera: Camera, hist=None, rgb=None, aov=None, samples_done: int | None = None, **params):
        """bdpt_reproject_host: the history `hist` ((H, W, 8), made with prev_camera; None: no history) carried into
        this integrator's camera and blended with rgb (default self.rgb) under the guides aov (default self.aov) ->
        (accumulated colour (H, W, 3), new history (H, W, 8)), both new arrays. samples_done: the samples per pixel
        rgb and aov hold (None = the full spp; norm = spp / samples_done). params: ReprojectSettings fields, or
        settings=ReprojectSettings(...)."""
        H, W = self.config.height, self.config.width
        r = self._reproject_params(prev_camera, samples_done, params)
        c = np.ascontiguousarray(self.rgb if rgb is None else rgb, np.float32)
        a = np.ascontiguousarray(self.aov if aov is None else aov, np.float32)
        h = None if hist is None else np.ascontiguousarray(hist, np.float32)
        if c.size != W * H * 3 or a.size != W * H * 8 or (h is not None and h.size != W * H * 8):
            raise BdptError(f"reproject: rgb / aov / hist have {c.size} / {a.size} / {None if h is None else h.size} "
                            f"floats, expected {W * H * 3} / {W * H * 8} / {W * H * 8}")
        out, state = np.zeros((H, W, 3), np.float32), np.zeros((H, W, HISTORY_CHANNELS), np.float32)
        p = self.params()
        _check(lib().bdpt_reproject_host(self._h, ctypes.byref(p), c.ctypes.data, a.ctypes.data,
                                         None if h is None else h.ctypes.data, out.ctypes.data, state.ctypes.data,
                                         ctypes.byref(r)))
        return out, state

    def reproject_device(self, prev_camera: Camera, rgb_ptr: int, aov_ptr: int, hist_in_ptr: int, out_ptr: int,
                         hist_out_ptr: int, stream_ptr: int = 0, cur_samples: float | None = None, norm: float = 1.0,
                         settings: "ReprojectSettings | None" = None) -> None:
        """bdpt_reproject: asynchronous, on device buffers; hist_in_ptr 0 = no history."""
        r = (settings or ReprojectSettings()).c(prev_camera, self.config.spp if cur_samples is None else cur_samples, norm)
        p = self.params()
        _check(lib().bdpt_reproject(self._h, ctypes.byref(p), ctypes.c_void_p(rgb_ptr), ctypes.c_void_p(aov_ptr),
                                    ctypes.c_void_p(hist_in_ptr or None), ctypes.c_void_p(out_ptr),
                                    ctypes.c_void_p(hist_out_ptr), ctypes.byref(r), ctypes.c_void_p(stream_ptr)))

    def render_sequence(self, cameras, spp_per_frame: int | None = None, denoise: bool = False,
                        display: "DisplaySettings | None" = None, meter: "MeterSettings | None" = None, **params):
        """Generator: one accumulated frame per camera of `cameras`. Frame f renders spp_per_frame samples
        (default the configured spp) and the feature buffers at cameras[f], with the seed base moved on by
        f * width * height * spp so that no two frames repeat a sample, and carries the history of frame f - 1
        into it with reproject (params: ReprojectSettings fields or settings=). Yields the accumulated (H, W, 3)
        frame; with denoise, (accumulated, bdpt_denoise of it at norm 1 under the frame's own guides). With
        display=DisplaySettings(...) the tuple additionally ends in the frame's 8-bit image, a uint8 (H, W,
        channels) array: the last float frame of the tuple metered under the frame's guides (meter=, default
        MeterSettings()) and displayed on the device, each frame's exposure adapted from the previous frame's
        meter words at meter.rate. The configured camera, spp and seed base are put back when the generator ends."""
        cfg = self.config
        saved = (cfg.camera, cfg.spp, cfg.seed_base)
        spp = cfg.spp if spp_per_frame is None else int(spp_per_frame)
        settings = params.pop("settings", None) or ReprojectSettings()
        if params:
            from dataclasses import replace
            settings = replace(settings, **params)
        try:
            hist, prev, words = None, None, None
            for f, cam in enumerate(cameras):
                cfg.camera, cfg.spp = cam, spp
                cfg.seed_base = (saved[2] + f * cfg.width * cfg.height * spp) & 0xFFFFFFFF
                self.init()
                self.render_frame()
                self.render_aov()
                out, hist = self.reproject(cam if prev is None else prev, hist, settings=settings)
                prev = cam
                frames = (out, self.denoise(out)) if denoise else (out,)
                if display is not None:
                    import torch
                    dev = torch.device("cuda", self.device)
                    words = self.meter(torch.from_numpy(frames[-1]).to(dev), torch.from_numpy(self.aov).to(dev), prev=words,
                                       settings=meter)
                    frames += (self.display(torch.from_numpy(frames[-1]).to(dev), meter=words, settings=display).cpu().numpy(),)
                yield frames if len(frames) > 1 else frames[0]
        finally:
            cfg.camera, cfg.spp, cfg.seed_base = saved

    @staticmethod
    def _frame_tensor(entry, t, channels, what):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3
                and t.shape[2] == channels and t.is_contiguous()):
            raise BdptError(f"{entry}: {what} must be a contiguous float32 cuda tensor of shape (H, W, {channels})")
        return t

    @staticmethod
    def _words_tensor(entry, t, what):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.numel() == 4 and t.is_contiguous()):
            raise BdptError(f"{entry}: {what} must be a contiguous int32 cuda tensor of 4 words (meter()'s result)")
        return t

    def _torch_stream(self, device):
        """The handle of torch's current stream for a call on torch tensors. A stream of torch's own orders the
        call with the tensors' other work and nothing waits. Torch's default stream has the handle 0, which the
        library reads as "the context's own stream", and the two are not ordered against each other: then the
        tensors' pending work is waited for here, and the caller waits for the call (_torch_done)."""
        import torch
        s = torch.cuda.current_stream(device)
        if s.cuda_stream == 0:
            s.synchronize()
        return s.cuda_stream

    def _torch_done(self, handle):
        if handle == 0:
            self.synchronize()

    def meter(self, color, aov=None, prev=None, settings: "MeterSettings | None" = None, norm: float = 1.0):
        """bdpt_meter on torch's current stream (_torch_stream): color a float32 cuda tensor (H, W, 3), aov (H, W,
        8) or None, prev an earlier call's words or None -> the 4 words [e, w, T, b_key | b_white << 16] as an
        int32 cuda tensor (the bits; .view(torch.float32)[:2] are e and w)."""
        import torch
        c = self._frame_tensor("meter", color, 3, "color")
        H, W = c.shape[:2]
        a = None if aov is None else self._frame_tensor("meter", aov, 8, "aov")
        if a is not None and tuple(a.shape[:2]) != (H, W):
            raise BdptError(f"meter: aov is {tuple(a.shape[:2])}, color {(H, W)}")
        pw = None if prev is None else self._words_tensor("meter", prev, "prev")
        out = torch.empty(4, dtype=torch.int32, device=c.device)
        st = self._torch_stream(c.device)
        self.meter_device(c.data_ptr(), 0 if a is None else a.data_ptr(), 0 if pw is None else pw.data_ptr(), out.data_ptr(),
                          W, H, st, norm, settings)
        self._torch_done(st)
        return out

    def meter_device(self, rgb_ptr: int, aov_ptr: int, prev_ptr: int, out_ptr: int, width: int | None = None,
                     height: int | None = None, stream_ptr: int = 0, norm: float = 1.0,
                     settings: "MeterSettings | None" = None) -> None:
        """bdpt_meter: asynchronous, on device buffers; aov_ptr / prev_ptr 0 = none."""
        m = (settings or MeterSettings()).c(norm)
        W, H = self.config.width if width is None else width, self.config.height if height is None else height
        _check(lib().bdpt_meter(self._h, W, H, ctypes.c_void_p(rgb_ptr), ctypes.c_void_p(aov_ptr or None),
                                ctypes.c_void_p(prev_ptr or None), ctypes.byref(m), ctypes.c_void_p(out_ptr),
                                ctypes.c_void_p(stream_ptr)))

    def meter_histogram(self) -> np.ndarray:
        """The 4096 bin counts of this context's last meter call (bdpt_debug_meter_histogram; waits for it)."""
        out = np.zeros(METER_BINS, np.uint32)
        _check(lib().bdpt_debug_meter_histogram(self._h, out.ctypes.data))
        return out

    def display(self, color, exposure=None, aov=None, meter=None, prev=None, settings: "DisplaySettings | None" = None,
                meter_settings: "MeterSettings | None" = None, norm: float = 1.0, out=None):
        """bdpt_display on torch's current stream (_torch_stream): color a float32 cuda tensor (H, W, 3) -> a uint8 cuda tensor
        (H, W, channels). exposure: None = settings.exposure, a number = that exposure, "auto" = bdpt_meter of
        color (under aov, from prev, with meter_settings) chained into the display on the device, with no host
        round trip. meter: words of an earlier meter() call to use as they are. out: a uint8 cuda tensor (or a
        view of one) of H * W * channels bytes to write into."""
        import torch
        from dataclasses import replace
        c = self._frame_tensor("display", color, 3, "color")
        H, W = c.shape[:2]
        s = settings or DisplaySettings()
        if isinstance(exposure, str):
            if exposure != "auto":
                raise ValueError(f'display: exposure must be a number, None or "auto", not {exposure!r}')
            if meter is not None:
                raise ValueError('display: exposure="auto" meters the frame itself: give that or meter=, not both')
            meter = self.meter(c, aov, prev, meter_settings, norm)
        elif exposure is not None:
            s = replace(s, exposure=float(exposure))
        mw = None if meter is None else self._words_tensor("display", meter, "meter")
        ch = int(s.channels)
        if out is None:
            out = torch.empty((H, W, ch) if ch in (3, 4) else (H, W, 4), dtype=torch.uint8, device=c.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                  and out.numel() == H * W * ch):
            raise BdptError(f"display: out must be a contiguous uint8 cuda tensor of {H * W * ch} bytes")
        st = self._torch_stream(c.device)
        self.display_device(c.data_ptr(), out.data_ptr(), 0 if mw is None else mw.data_ptr(), W, H, st, norm, s)
        self._torch_done(st)
        return out

    def display_device(self, rgb_ptr: int, out_ptr: int, meter_ptr: int = 0, width: int | None = None,
                       height: int | None = None, stream_ptr: int = 0, norm: float = 1.0,
                       settings: "DisplaySettings | None" = None) -> None:
        """bdpt_display: asynchronous, on device buffers; meter_ptr 0 = settings.exposure and settings.white."""
        d = (settings or DisplaySettings()).c(norm)
        W, H = self.config.width if width is None else width, self.config.height if height is None else height
        _check(lib().bdpt_display(self._h, W, H, ctypes.c_void_p(rgb_ptr), ctypes.c_void_p(meter_ptr or None),
                                  ctypes.byref(d), ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream_ptr)))

    def denoise_var(self, rgb=None, var=None, aov=None, samples_done: int | None = None, return_variance: bool = False,
                    **params):
        """bdpt_denoise_var_host of rgb (default self.rgb) with its per-pixel variance var (default self.var,
        batch_moments' last) guided by aov (default self.aov): a new (H, W, 3) array; return_variance: (filtered,
        residual variance (H, W)). samples_done as denoise(); params: DenoiseSettings fields over
        denoise_var_settings(), or settings=DenoiseSettings(...)."""
        H, W = self.config.height, self.config.width
        settings = params.pop("settings", None) or denoise_var_settings()
        if params:
            from dataclasses import replace
            settings = replace(settings, **params)
        if samples_done is not None and samples_done < 1:
            raise ValueError("denoise_var: samples_done must be >= 1")
        norm = 1.0 if samples_done is None else self.config.spp / samples_done
        if var is None and getattr(self, "var", None) is None:
            raise BdptError("denoise_var: no var given and batch_moments has not run")
        c = np.ascontiguousarray(self.rgb if rgb is None else rgb, np.float32)
        v = np.ascontiguousarray(self.var if var is None else var, np.float32)
        a = np.ascontiguousarray(self.aov if aov is None else aov, np.float32)
        if c.size != W * H * 3 or v.size != W * H * 3 or a.size != W * H * 8:
            raise BdptError(f"denoise_var: rgb / var / aov have {c.size} / {v.size} / {a.size} floats, expected "
                            f"{W * H * 3} / {W * H * 3} / {W * H * 8}")
        out = np.zeros((H, W, 3), np.float32)
        out_var = np.zeros((H, W), np.float32) if return_variance else None
        d = settings.c(norm)
        _check(lib().bdpt_denoise_var_host(self._h, W, H, c.ctypes.data, v.ctypes.data, a.ctypes.data, out.ctypes.data,
                                           None if out_var is None else out_var.ctypes.data, ctypes.byref(d)))
        return (out, out_var) if return_variance else out

    def denoise_var_device(self, rgb_ptr: int, var_ptr: int, aov_ptr: int, out_ptr: int, out_var_ptr: int = 0,
                           stream_ptr: int = 0, norm: float = 1.0, settings: "DenoiseSettings | None" = None) -> None:
        """bdpt_denoise_var: asynchronous, on device buffers (out_var_ptr 0: the residual variance is not wanted)."""
        d = (settings or denoise_var_settings()).c(norm)
        _check(lib().bdpt_denoise_var(self._h, self.config.width, self.config.height, ctypes.c_void_p(rgb_ptr),
                                      ctypes.c_void_p(var_ptr), ctypes.c_void_p(aov_ptr), ctypes.c_void_p(out_ptr),
                                      ctypes.c_void_p(out_var_ptr or None), ctypes.byref(d),
                                      ctypes.c_void_p(stream_ptr)))

    def denoise_planes(self, planes, aov=None, mode="shared", guide=None, samples_done: int | None = None,
                       return_guide: bool = False, **params):
        """bdpt_denoise_planes_host of a split frame's planes, any leading shape (n, H, W, 3), (n_groups,
        n_inner, H, W, 3), ...: a new array of that shape, guided by aov (default self.aov). mode "own":
        every plane as denoise() filters it; "shared": every plane with the weights of one colour guide
        (guide, an (H, W, 3) image, or None: the planes' sum), so that the filtered planes still add up and
        relight. return_guide: also the filtered guide, (planes, guide). samples_done and params as denoise()."""
        H, W = self.config.height, self.config.width
        settings = params.pop("settings", None) or DenoiseSettings()
        if params:
            from dataclasses import replace
            settings = replace(settings, **params)
        if samples_done is not None and samples_done < 1:
            raise ValueError("denoise_planes: samples_done must be >= 1")
        norm = 1.0 if samples_done is None else self.config.spp / samples_done
        p = np.ascontiguousarray(planes, np.float32)
        if p.ndim < 4 or p.shape[-3:] != (H, W, 3):
            raise BdptError(f"denoise_planes: planes must be (..., {H}, {W}, 3), got {p.shape}")
        a = np.ascontiguousarray(self.aov if aov is None else aov, np.float32)
        g = None if guide is None else np.ascontiguousarray(guide, np.float32)
        if a.size != W * H * 8 or (g is not None and g.size != W * H * 3):
            raise BdptError(f"denoise_planes: aov / guide must hold {W * H * 8} / {W * H * 3} floats")
        n = math.prod(p.shape[:-3])
        ok = n >= 1 and n * W * H < PLANE_PIXELS_MAX  # (what the library refuses before it touches a buffer)
        out = np.zeros(p.shape if ok else (1,), np.float32)
        out_guide = np.zeros((H, W, 3), np.float32) if return_guide else None
        d = settings.c(norm)
        _check(lib().bdpt_denoise_planes_host(self._h, W, H, n, p.ctypes.data, a.ctypes.data,
                                              None if g is None else g.ctypes.data, _denoise_planes_mode(mode),
                                              ctypes.byref(d), out.ctypes.data,
                                              None if out_guide is None else out_guide.ctypes.data))
        return (out, out_guide) if return_guide else out

    def denoise_planes_device(self, planes_ptr: int, n_planes: int, aov_ptr: int, out_ptr: int, mode="shared",
                              guide_ptr: int = 0, out_guide_ptr: int = 0, stream_ptr: int = 0, norm: float = 1.0,
                              settings: "DenoiseSettings | None" = None) -> None:
        """bdpt_denoise_planes: asynchronous, on device buffers (0: no guide given / no filtered guide wanted)."""
        d = (settings or DenoiseSettings()).c(norm)
        _check(lib().bdpt_denoise_planes(self._h, self.config.width, self.config.height, int(n_planes),
                                         ctypes.c_void_p(planes_ptr), ctypes.c_void_p(aov_ptr),
                                         ctypes.c_void_p(guide_ptr or None), _denoise_planes_mode(mode), ctypes.byref(d),
                                         ctypes.c_void_p(out_ptr), ctypes.c_void_p(out_guide_ptr or None),
                                         ctypes.c_void_p(stream_ptr)))

    def stats(self) -> dict:
        s = _Stats()
        _check(lib().bdpt_get_stats(self._h, ctypes.byref(s)))
        leaf = (ctypes.c_int64 * 2)()  # (bdpt_get_leaf_rewalks: an entry of its own, bdpt_stats keeps its layout)
        _check(lib().bdpt_get_leaf_rewalks(self._h, leaf))
        grid = (ctypes.c_int64 * 2)()  # (bdpt_get_grid: frame-kernel blocks, lane slots)
        _check(lib().bdpt_get_grid(self._h, grid))
        return dict(leaf_rewalks=leaf[0], leaf_hits=leaf[1], grid=grid[0], slots=grid[1], kernel_ms=s.kernel_ms, samples=s.samples, launches=s.launches,
                    counters=dict(zip(COUNTER_NAMES, list(s.counters))), capped_samples=s.capped_samples,
                    span_ms=s.span_ms, tail_ms=s.tail_ms, max_light_depth=s.max_light_depth,
                    max_eye_depth=s.max_eye_depth, max_queries=s.max_queries, schedule_errors=s.schedule_errors, parked_samples=s.parked_samples,
                    rr_long_walks_max=s.rr_long_walks_max, rr_express_iters=list(s.rr_express_iters),
                    sched=dict(zip(("step_tasks", "shade_steps", "steps_ge32", "steps_ge64"), list(s.sched))),
                    kernel=(lib().bdpt_last_kernel(self._h) or b"").decode(),
                    kernel_glossy=int(lib().bdpt_last_kernel_glossy(self._h)))

    def synchronize(self) -> None:
        _check(lib().bdpt_synchronize(self._h))

    def set_row_order(self, order) -> None:
        """Claim order of the shard's local rows for later renders (bdpt_set_row_order);
        None or [] restores top to bottom. Changes no sample, only which run last."""
        a = np.ascontiguousarray(np.asarray([] if order is None else order, dtype=np.int32))
        _check(lib().bdpt_set_row_order(self._h, a.ctypes.data if a.size else None, int(a.size)))

    def row_costs(self, nrows: int) -> np.ndarray:
        """Queries per local row of the last FLAG_COUNT render (bdpt_get_row_costs)."""
        out = np.zeros(nrows, np.int64)
        _check(lib().bdpt_get_row_costs(self._h, out.ctypes.data, int(nrows)))
        return out

    def save(self, path: str) -> None:
        """Integrator::save: self.rgb as the reference's EXR."""
        save_exr(self.rgb, self.config.width, self.config.height, path)


def cost_row_order(costs) -> np.ndarray:
    """Local rows by descending cost (ties top to bottom): the costly rows are claimed
    first, so the samples still in flight when a shard's work runs out are cheap ones."""
    c = np.asarray(costs)
    return np.lexsort((np.arange(c.size), -c)).astype(np.int32)


class PathTracerIntegrator(BDPTIntegrator):
    """The reference's PathTracerIntegrator (src/integrators/path.h) on the same
    GPU substrate: render(ray, sampler), render_frame and render_device as for BDPT."""

    def __init__(self, scene: Scene, config: Config, path: PathSettings | None = None, device: int = 0):
        super().__init__(scene, config, device)
        self.path = path or PathSettings()

    def render(self, ray: Ray, sampler: Sampler) -> np.ndarray:
        """PathTracerIntegrator::render(const Ray&, Sampler&) (path.h:235-245): Li of
        one sample; the sampler's std::mt19937 state advances."""
        r = (ctypes.c_float * 8)(*ray.o, *ray.d, ray.min_t, ray.max_t)
        Li = (ctypes.c_float * 3)()
        p, pp = self.params(), self.path.c()
        st = np.ascontiguousarray(sampler.state, np.uint32)
        _check(lib().bdpt_render_path_sample_mt(self._h, ctypes.byref(p), ctypes.byref(pp), r, st.ctypes.data, Li))
        sampler.state = st
        return np.array(Li[:], np.float32)

    def _integrator_params(self):
        return self.path.c(), None

    def render_device(self, fb_ptr: int, stream_ptr: int = 0, row_offset: int = 0, row_stride: int = 1,
                      flags: int = 0, window: SampleWindow | None = None) -> None:
        """Asynchronous; call check_levels() after the stream is synchronised: a
        sample that outgrew the 512-level recursion stack makes the frame differ
        from the reference's (render_frame checks this itself)."""
        super().render_device(fb_ptr, stream_ptr, row_offset, row_stride, flags, window)

    def check_levels(self) -> None:
        """Raises BdptError if a sample of the last render_device call outgrew the
        level stack (bdpt_get_stats counters[1] of bdpt_render_path)."""
        n = self.stats()["counters"]["shadow_rays"]
        if n:
            raise BdptError(f"{n} path samples outgrew the 512-level recursion stack")


class DirectIntegrator(BDPTIntegrator):
    """The reference's DirectIntegrator (src/integrators/direct.h) on the same GPU
    substrate: one bounce of direct light by area, solid-angle, cosine-hemisphere,
    BSDF or MIS sampling, with the emitters as the spheres the reference makes of
    them (renderer.cpp:349-358)."""

    def __init__(self, scene: Scene, config: Config, direct: DirectSettings | None = None, device: int = 0):
        super().__init__(scene, config, device)
        self.direct = direct or DirectSettings(sampling_strategy="mis")

    def render(self, ray: Ray, sampler: Sampler) -> np.ndarray:
        """DirectIntegrator::render(const Ray&, Sampler&) (direct.h:449-462): Li of one
        sample; the sampler's std::mt19937 state advances."""
        r = (ctypes.c_float * 8)(*ray.o, *ray.d, ray.min_t, ray.max_t)
        Li = (ctypes.c_float * 3)()
        p, d = self.params(), self.direct.c()
        st = np.ascontiguousarray(sampler.state, np.uint32)
        _check(lib().bdpt_render_direct_sample_mt(self._h, ctypes.byref(p), ctypes.byref(d), r, st.ctypes.data, Li))
        sampler.state = st
        return np.array(Li[:], np.float32)

    def _integrator_params(self):
        return None, self.direct.c()


class MultiDeviceRenderer:
    """One process, several HIP devices (bdpt_multi_*): the reference's parallel_for
    over host threads (parallelfor.h:25-65) as one context and stream per device,
    interleaved row shards, and one RCCL sum-reduce of the frames to devices[0].
    A repeated device (e.g. [0, 0]) rehearses the decomposition on one GPU with a
    local sum instead of RCCL. sharding="samples" splits by samples instead of rows:
    device i renders samples i, i + N, ... of every pixel of the whole image
    (bdpt_multi_set_sharding), equal work per device whatever the rows cost."""

    SHARDING = {"rows": 0, "samples": 1}  # BDPT_SHARD_*

    def __init__(self, scene: Scene, config: Config, devices=(0,), path: PathSettings | None = None,
                 direct: DirectSettings | None = None, sharding: str = "rows"):
        if sharding not in self.SHARDING:
            raise ValueError(f"sharding must be 'rows' or 'samples', not {sharding!r}")
        self.scene, self.config, self.devices = scene, config, list(devices)
        self.path, self.direct, self.sharding = path, direct, sharding
        dev = (ctypes.c_int32 * len(self.devices))(*self.devices)
        h = ctypes.c_void_p()
        _check(lib().bdpt_multi_create(scene._h, len(self.devices), dev, ctypes.byref(h)))
        self._h = h
        _check(lib().bdpt_multi_set_sharding(self._h, self.SHARDING[sharding]))

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.bdpt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def render_frame(self) -> np.ndarray:
        c = self.config
        p = _FrameParams()
        p.camera = c.camera.c()
        p.width, p.height, p.spp = c.width, c.height, c.spp
        p.rr_depth = 1 if (self.path or self.direct) else c.rr_depth  # rrDepth is the BDPT setting
        p.strategy, p.seed_base = c.strategy, c.seed_base & 0xFFFFFFFF
        p.row_offset, p.row_stride, p.flags = 0, 1, 0
        rgb = np.zeros((c.height, c.width, 3), np.float32)
        pp = ctypes.byref(self.path.c()) if self.path else None
        dp = ctypes.byref(self.direct.c()) if self.direct else None
        _check(lib().bdpt_multi_render_host(self._h, ctypes.byref(p), pp, dp, rgb.ctypes.data))
        return rgb

    def stats(self) -> dict:
        s = _MultiStats()
        _check(lib().bdpt_multi_get_stats(self._h, ctypes.byref(s)))
        n = s.devices
        return dict(devices=n, rccl=bool(s.rccl), wall_ms=s.wall_ms, render_ms=s.render_ms, reduce_ms=s.reduce_ms,
                    samples=s.samples, kernel_ms=list(s.kernel_ms)[:n], device_samples=list(s.device_samples)[:n],
                    capped_samples=s.capped_samples, schedule_errors=s.schedule_errors)


KAT_BUILDS = {"exact": 0, "fast": 1, "ng": 2}  # BDPT_KAT_*
# BDPT_SAMPLING_*: code, words in, words out per element
SAMPLING_FNS = {"canonical": (0, 1, 1), "hemisphere": (1, 2, 3), "triangle": (2, 2, 2), "sphere": (3, 2, 3),
                "solid_angle": (4, 9, 4), "ray_sphere": (5, 12, 1), "cdf": (6, 2, 1), "emitter": (7, 4, 10),
                "camera": (8, 3, 3)}
EMITTER_PLACEMENTS = {"ctx": 0, "hbm": 1, "lds": 2}  # BDPT_EMITTERS_*
MATH_FNS = {"sinf": 0, "cosf": 1, "powf": 2, "sincos_s": 3, "sincos_c": 4,  # BDPT_MATH_*
            "pow_w": 5, "rcp_w": 6, "div_w": 7, "sqrt_w": 8, "rsqrt_w": 9}


def debug_math(fn: str, x: np.ndarray, y: np.ndarray | None = None, device: int = 0) -> np.ndarray:
    """The device sinf / cosf / powf (glibc restatements) on float32 inputs:
    fn in {"sinf", "cosf", "powf", "sincos_s", "sincos_c"}; and the fast weight
    arithmetic of the default frame kernels: "pow_w" (x, y), "rcp_w", "div_w" (x / y),
    "sqrt_w", "rsqrt_w"."""
    code = MATH_FNS[fn]
    x = np.ascontiguousarray(x, np.float32)
    yy = None if y is None else np.ascontiguousarray(y, np.float32)
    if fn in ("powf", "pow_w", "div_w") and (yy is None or yy.size != x.size):
        raise ValueError(f"debug_math({fn!r}) needs y of x's size")
    out = np.empty_like(x)
    _check(lib().bdpt_debug_math(device, code, x.ctypes.data, None if yy is None else yy.ctypes.data,
                                 out.ctypes.data, x.size))
    return out


def debug_fresnel(inp, device: int = 0) -> np.ndarray:
    """GlassBSDF::FresnelDielectric (glass.h:40-53) on (n, 4) = (eta_i, eta_t, cos_i, cos_t)."""
    x = _af32(inp, 4)
    out = np.zeros(x.shape[0], np.float32)
    _check(lib().bdpt_debug_fresnel(device, x.shape[0], x.ctypes.data, out.ctypes.data))
    return out


def debug_triangle(rays, verts, device: int = 0) -> np.ndarray:
    """rayTriangleIntersect (core.h:379-400): (n, 4) = (hit, t, u, v) for rays (n, 8), verts (n, 9)."""
    r, v = _af32(rays, 8), _af32(verts, 9)
    out = np.zeros((r.shape[0], 4), np.float32)
    _check(lib().bdpt_debug_triangle(device, r.shape[0], r.ctypes.data, v.ctypes.data, out.ctypes.data))
    return out
