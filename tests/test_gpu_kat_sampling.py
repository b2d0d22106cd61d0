"""The sampling side of the path, per function and per compilation, against the unmodified
reference on inputs chosen at its edges (bdpt_debug_sampling; fixtures kat_sampling_*.npz and
kat_sampler_edges_*.npz of tests/golden/make_kat_goldens.py, populations checked in
tests/test_sampling_kat_cpu.py).

Draws enter as the std::mt19937 output words they come from, so a record can sit on the words
that round to 1 (>= 0xFFFFFF80), on a CDF knot or one float either side of it, or on the float
below 1. Bars: the exact build gives the reference's bits in every output; the fast-weight build
too, except sample_emitter's pos_pdf, which is rcp_w(area) there and within 1 ulp of the
reference's 1.f / area (the accuracy the project states for rcp_w; worst observed on these
records, five distinct areas: 0 ulp).
sample_emitter has two bodies, one reading an LDS copy of the faces and CDFs and one reading HBM:
both run on every record and agree bit for bit.

Mutations of the device code, one at a time, and the tests of this file that failed on an MI355X
(only the per-function kernel rebuilt; every other test passed):
  next1 without the >= 1 clamp                  canonical, emitter (all), camera_dir at spp 4
  cdf_sample with <= for <                      emitter[*-ctx], emitter[*-hbm], emitter_bodies_agree
  cdf_sample_lds with <= for <                  emitter[*-lds], emitter_bodies_agree
  uniform_triangle returning (u * s.y, 1 - u)   warps, emitter (all)
  camera_dir scaling the y jitter by invW       camera_dir[*-80x48-4] only (a square image cannot see it)
  sphere_solid_angle without the fmax(0, .)     sphere_functions
  sample_emitter without the id clamp           not run: no record can see it. u0 * n < n in float for every
                                                u0 < 1 (tests/test_sampling_kat_cpu.py), so the clamp binds
                                                only for the u0 = 1 that next1's clamp removes
"""
import os

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu

GOLD = os.path.join(REPO, "tests", "golden")
TOL = 1e-4  # the suite's per-pixel frame bound (test_gpu_parity.py)
f32 = np.float32
BUILDS = ["exact", "fast"]
_cache = {}


def kat(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLD, name + ".npz")))
    return _cache[name]


def integrator(scene, W=64, H=64, spp=16, rr=None):
    key = (scene, W, H, spp, rr)
    if key not in _cache:
        cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES[scene]["camera"]), width=W, height=H, spp=spp,
                              rr_depth=rr if rr is not None else variants.SCENES[scene]["rr_depth"])
        it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(scene)), cfg)
        it.init()
        _cache[key] = it
    return _cache[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.uint32 else a


def same(got, ref):
    """Per record: every word has the reference's bits (or is an equal float: +0 and -0)."""
    g, r = bits(got).reshape(len(got), -1), bits(ref).reshape(len(ref), -1)
    return ((g == r) | (g.view(f32) == r.view(f32))).all(1)


def assert_same(got, ref, what):
    bad = ~same(got, ref)
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8])


@pytest.mark.parametrize("build", BUILDS)
def test_gpu_canonical_matches_reference(build):
    """Sampler::next() of one crafted word: all of 0xFFFFFF00 .. 0xFFFFFFFF (the upper half rounds
    to 1.0f and is moved below it), 0, 1, the words around every power of two, conversion ties."""
    g = kat("kat_sampling_canonical")
    out = integrator("emit_edges").debug_sampling("canonical", g["word"], build)[:, 0]
    assert_same(out, g["out"], "canonical")
    assert (out.view(f32) < 1).all()


@pytest.mark.parametrize("build", BUILDS)
def test_gpu_warps_match_reference(build):
    """squareToUniformHemisphere / Triangle / Sphere on a grid of 0, 2^-32, 2^-24, .., the float
    below 1 in either coordinate, and random draws."""
    g = kat("kat_sampling_warp")
    it = integrator("emit_edges")
    for fn, key in (("hemisphere", "hemisphere"), ("triangle", "triangle"), ("sphere", "sphere")):
        assert_same(it.debug_sampling(fn, g["u"].view(np.uint32), build), g[key], fn)
    assert (g["hemisphere_pdf"] == f32(0.15915494309189535)).all()  # constants: nothing to run


@pytest.mark.parametrize("build", BUILDS)
def test_gpu_sphere_functions_match_reference(build):
    """The direct integrator's sphere pieces: sampleSphereByArea's normal (uniform_sphere),
    sampleSphereBySolidAngle from outside, on and inside the sphere, raySphereIntersect on random
    rays, exact roots against min_t / max_t and discriminants of exactly 0."""
    g = kat("kat_sampling_sphere")
    it = integrator("emit_edges")
    assert_same(it.debug_sampling("sphere", g["u"].view(np.uint32), build), g["area_ne"], "area ne")
    rec = np.concatenate([g["u"], g["p"], g["center"], g["radius"][:, None]], 1).astype(f32)
    out = it.debug_sampling("solid_angle", rec.view(np.uint32), build)
    assert_same(out[:, :3], g["solid_wi"], "solid angle wi")
    assert_same(out[:, 3], g["solid_pdf"], "solid angle pdf")
    rec = np.concatenate([g["rays"], g["ray_center"], g["ray_radius"][:, None]], 1).astype(f32)
    hit = it.debug_sampling("ray_sphere", rec.view(np.uint32), build)[:, 0]
    bad = hit != g["hit"].astype(np.uint32)
    assert not bad.any(), (int(bad.sum()), np.bincount(g["ray_cls"][bad]), np.flatnonzero(bad)[:8])


def test_gpu_emitter_placement_of_the_test_scenes():
    """Which body of sample_emitter the frames of each scene run (bdpt_ctx_create: the LDS copy
    when it fits 24 KiB and costs no resident block)."""
    got = {sc: integrator(sc).emitter_placement() for sc in ("emit_edges", "caustic")}
    assert got == dict(emit_edges="hbm", caustic="lds")


def ulp_distance(a, b):
    """Of positive floats given as float32 or as their bits (uint32)."""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


@pytest.mark.parametrize("placement", ["ctx", "hbm", "lds"])
@pytest.mark.parametrize("build", BUILDS)
def test_gpu_emitter_matches_reference(build, placement):
    """selectEmitter + sampleEmitterPosition on emit_edges: u1 on every CDF knot of every emitter
    and one float either side, equal consecutive knots, knots one ulp apart, u0 around every k / 5,
    triangle draws at 0 and the float below 1, interpolated normals, 2000 random records."""
    g = kat("kat_sampling_emitter")
    it = integrator("emit_edges")
    out = it.debug_sampling("emitter", g["words"], build, placement)
    for col, key in ((0, "id"), (1, "emitter_pdf"), (2, "face")):
        bad = ~same(out[:, col], g[key])
        assert not bad.any(), (key, int(bad.sum()), np.bincount(g["cls"][bad]), np.flatnonzero(bad)[:8])
    assert_same(out[:, 3:6], g["pos"], "pos")
    assert_same(out[:, 6:9], g["n"], "n")
    if build == "exact":
        assert_same(out[:, 9], g["area_pdf"], "pos_pdf")
    else:
        d = ulp_distance(out[:, 9], g["area_pdf"])
        print("fast build: worst pos_pdf distance", int(d.max()), "ulp")
        assert d.max() <= 1, int(d.max())
    # the CDF search alone, with the float the draw becomes
    u1 = g["words"][:, 1].astype(f32) / f32(4294967296.0)
    u1 = np.where(u1 >= 1, np.nextafter(f32(1), f32(0)), u1).astype(f32)
    rec = np.stack([g["id"].view(np.uint32), u1.view(np.uint32)], 1)
    face = it.debug_sampling("cdf", rec, build, placement)[:, 0]
    assert np.array_equal(face, g["face"].view(np.uint32))


@pytest.mark.parametrize("build", BUILDS)
def test_gpu_emitter_bodies_agree(build):
    """The HBM body and the LDS body of sample_emitter give identical bits on every record."""
    g = kat("kat_sampling_emitter")
    it = integrator("emit_edges")
    a = it.debug_sampling("emitter", g["words"], build, "hbm")
    b = it.debug_sampling("emitter", g["words"], build, "lds")
    assert np.array_equal(a, b)


def test_gpu_debug_sampling_refuses_bad_arguments():
    """An emitter index outside the scene and an unknown placement are refused before any launch."""
    it = integrator("emit_edges")
    with pytest.raises(bdpt_amd.BdptError):
        it.debug_sampling("cdf", np.array([[5, 0]], np.uint32))
    with pytest.raises(KeyError):
        it.debug_sampling("cdf", np.array([[0, 0]], np.uint32), placement="both")


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("size", [(64, 64), (80, 48)])
@pytest.mark.parametrize("build", BUILDS)
def test_gpu_camera_dir_matches_reference(build, size, spp):
    """The camera ray (renderer.cpp:165-195): the spp == 1 branch and the jitter branch, on a square
    and a non-square image, corner pixels, jitter words 0 / 0xFFFFFF7F / 0xFFFFFF80 / 0xFFFFFFFF."""
    W, H = size
    g = kat("kat_sampling_camera")
    it = integrator("caustic", W, H, spp)
    out = it.debug_sampling("camera", g[f"rec_{W}x{H}_spp{spp}"], build)
    assert_same(out, g[f"dir_{W}x{H}_spp{spp}"], "camera direction")


@pytest.mark.parametrize("scene", ["caustic", "emit_edges"])
def test_gpu_whole_samples_from_edge_draws_match_reference(scene):
    """BDPTIntegrator::render(ray, sampler) from states whose first 12 outputs are 0, 0xFFFFFF7F,
    0xFFFFFF80, 0xFFFFFFFF and words on CDF knots: Li, the state after, the splats, compared as
    test_gpu_render_ray_sampler_matches_reference compares its records."""
    import sys

    sys.path.insert(0, GOLD)
    from make_kat_goldens import untemper

    g = kat(f"kat_sampler_edges_bdpt_{scene}")
    it = integrator(scene, int(g["width"]), int(g["height"]), int(g["spp"]), int(g["rr"]))
    for i in range(g["rays"].shape[0]):
        st = np.zeros(625, np.uint32)
        p = int(g["pos"][i])
        st[p: p + g["draws"].shape[1]] = untemper(g["draws"][i])
        st[624] = p
        r = g["rays"][i]
        s = bdpt_amd.Sampler.from_state(st)
        Li, splats = it.render_sample(bdpt_amd.Ray(tuple(r[:3]), tuple(r[3:6]), float(r[6]), float(r[7])), s)
        acc = {}
        for px, v in splats:
            acc[px] = acc.get(px, np.zeros(3, np.float32)) + v
        n = int(g["nsplat"][i])
        assert len(acc) == n, (i, len(acc), n)
        for px, rr_, gg, bb in g["splats"][i][: min(n, 16)]:
            got = acc[int(np.float32(px).view(np.int32))]
            assert same(got[None], np.array([[rr_, gg, bb]], f32)).all(), (i, got)
        assert same(np.asarray(Li, f32)[None], g["Li"][i][None]).all(), (i, Li, g["Li"][i])
        st[624] = g["pos_out"][i]
        assert np.array_equal(s.state, st), i


def test_gpu_emit_edges_frame_matches_reference_golden(golden_manifest):
    """One whole frame of the five-emitter scene at the suite's bound."""
    name = "G14_emit_edges_32x32_spp4"
    m = golden_manifest["framebuffers"][name]
    it = integrator(m["scene"], m["width"], m["height"], m["spp"], m["rr_depth"])
    fb = it.render_frame().reshape(-1, 3).astype(np.float64)
    assert it.stats()["samples"] == m["samples"] and np.isfinite(fb).all()
    ref = load_golden(name).reshape(-1, 3).astype(np.float64)
    err = np.linalg.norm(fb - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-8)
    assert err.max() <= TOL, f"max per-pixel rel L2 {err.max():.3g}"
