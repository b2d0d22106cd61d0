"""First-hit feature buffers (bdpt_render_aov) on the GPU, pinned to bdpt_intersect —
itself pinned to the reference's AcceleratorBVH::intersect (tests/test_gpu_kat.py): the
test builds the offline driver's camera ray of every (pixel, sample) in numpy, sends the
rays through it.intersect and forms the eight channels in float64 from the hit records
and the scene's materials."""
import json
import os

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import REPO, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

TEX = os.path.join(REPO, "scenes", "tex")
AWAY = dict(eye=(0.0, 0.8, 3.8), at=(0.0, 0.8, 7.6), up=(0.0, 1.0, 0.0), fov=30.0)  # the box lies behind


def make(obj, cam, W, H, spp):
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**cam), width=W, height=H, spp=spp, rr_depth=5)
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(obj), cfg)
    it.init()
    return it


def driver_rays(it):
    """driver_ray of tests/test_gpu_parity.py for every (pixel, k), vectorised: the camera
    ray of renderer.cpp:162-192 in the reference's float32 operation order, the two jitter
    draws of std::mt19937(seed + pixel * spp + k) first iff spp > 1. (H * W * spp, 8)."""
    c = it.config
    W, H, spp = c.width, c.height, c.spp
    f32 = np.float32
    cam = bdpt_amd.camera_constants(c.camera, W, H)
    c2w = cam[16:32].reshape(4, 4)  # column-major: c2w[col][row]
    invW, invH, angle, aspect = cam[64:68]
    pix = np.repeat(np.arange(W * H), spp)
    k = np.tile(np.arange(spp), W * H)
    j, i = (pix % W).astype(f32), (pix // W).astype(f32)
    y = (f32(1) - (i + f32(0.5)) * invH) * f32(2) - f32(1)
    x = ((j + f32(0.5)) * invW) * f32(2) - f32(1)
    if spp == 1:
        px, py = x * angle * aspect, y * angle
    else:
        u = np.empty((pix.size, 2), f32)
        for n, seed in enumerate((c.seed_base + pix * spp + k) & 0xFFFFFFFF):
            raw = np.random.RandomState(int(seed)).randint(0, 2**32, size=2, dtype=np.uint32)
            u[n] = raw.astype(f32) / f32(2**32)  # generate_canonical<float, 24>
        u = np.where(u >= f32(1), np.nextafter(f32(1), f32(0)), u)
        px = ((x + (u[:, 0] - f32(0.5)) * invW) * angle) * aspect
        py = (y + (u[:, 1] - f32(0.5)) * invH) * angle
    d = np.stack([(c2w[0][r] * px + c2w[1][r] * py) + (c2w[2][r] * f32(-1) + c2w[3][r] * f32(0)) for r in range(3)], 1)
    d = d * (f32(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))[:, None]
    rays = np.empty((pix.size, 8), f32)
    rays[:, 0:3] = np.asarray(c.camera.eye, f32)
    rays[:, 3:6] = d
    rays[:, 6], rays[:, 7] = 1.0, 1000.0
    return rays


def texel_lookup(scene, desc, hits, which):
    """BitmapTexture3f::eval (core.h:569-587) in float32 at the hits: per hit
    the texel of its material's diffuse (which = 0) / specular (1) map, NaN rows where the
    material has none, and whether st.x * w or st.y * h lies within 1e-3 of an integer."""
    f32 = np.float32
    st = np.frombuffer(scene.export_textures("tri_st"), f32).reshape(-1, 6)[hits["tri"]]  # BVH leaf order
    mt = np.frombuffer(scene.export_textures("mat_tex"), np.int32).reshape(-1, 2)[hits["mat_id"], which]
    u, v = hits["u"], hits["v"]
    w = f32(1) - u - v
    sx = (st[:, 0] * w + st[:, 2] * u) + st[:, 4] * v + f32(1)
    sy = (st[:, 1] * w + st[:, 3] * u) + st[:, 5] * v + f32(1)
    sx, sy = sx - np.floor(sx), sy - np.floor(sy)
    out = np.full((hits.size, 3), np.nan)
    edge = np.zeros(hits.size, bool)
    for t, tex in enumerate(desc.textures):
        sel = mt == t
        th, tw = tex.shape[:2]
        fx, fy = sx[sel] * f32(tw), sy[sel] * f32(th)
        xi = np.clip(fx.astype(np.int32), 0, tw - 1)
        yi = np.clip(fy.astype(np.int32), 0, th - 1)
        out[sel] = tex[yi, xi]
        edge[sel] = (np.abs(fx - np.round(fx)) < 1e-3) | (np.abs(fy - np.round(fy)) < 1e-3)
    return out, edge


def expected(it, textured=True):
    """(aov float64 (H, W, 8), hit counts (H, W), per-pixel "a texel lookup is ambiguous",
    per-pixel "a sample hit a textured material") from it.intersect."""
    c = it.config
    W, H, spp = c.width, c.height, c.spp
    hits = it.intersect(driver_rays(it))
    desc = it.scene.to_desc()
    kinds = np.array([{7: 1, 3: 2, 6: 3, 8: 4, 5: 0}.get(int(m["illum"]), 5) for m in desc.materials])
    kd = np.array([m["kd"] for m in desc.materials], np.float64)[hits["mat_id"]]
    ks = np.array([m["ks"] for m in desc.materials], np.float64)[hits["mat_id"]]
    edge = np.zeros(hits.size, bool)
    mapped = np.zeros(hits.size, bool)
    if textured and desc.textures is not None:
        for which, dst in ((0, kd), (1, ks)):
            tx, e = texel_lookup(it.scene, desc, hits, which)
            has = ~np.isnan(tx[:, 0])
            dst[has] = tx[has]
            edge |= e & has
            mapped |= has
    kind = kinds[hits["mat_id"]]
    alb = np.ones((hits.size, 3))
    alb[kind == 1] = kd[kind == 1]
    glossy = (kind == 4) | (kind == 5)
    alb[glossy] = np.minimum(kd[glossy] + ks[glossy], 1.0)
    ok = hits["hit"] == 1
    ch = np.zeros((hits.size, 8))
    ch[:, 0:3], ch[:, 3:6], ch[:, 6], ch[:, 7] = alb, hits["ns"], hits["t"], 1.0
    ch[~ok] = 0.0
    aov = ch.reshape(H, W, spp, 8).sum(2) / spp
    return (aov, ok.reshape(H, W, spp).sum(2), (edge & ok).reshape(H, W, spp).any(2),
            (mapped & ok).reshape(H, W, spp).any(2))


def group_err(got, ref):
    """Per pixel, the relative L2 error of albedo, normal and depth (worst of the three)."""
    got = got.astype(np.float64)
    errs = []
    for sl in (slice(0, 3), slice(3, 6), slice(6, 7)):
        d = np.linalg.norm(got[..., sl] - ref[..., sl], axis=-1)
        errs.append(d / np.maximum(np.linalg.norm(ref[..., sl], axis=-1), 1e-30))
    return np.max(errs, axis=0)


def check_pinned(it, aov, ref, count):
    spp = it.config.spp
    assert np.isfinite(aov).all()
    assert np.array_equal(aov[..., 7], count.astype(np.float32) * np.float32(1.0 / spp))  # coverage: exact
    err = group_err(aov, ref)
    print("worst per-pixel relative error", err.max())
    assert err.max() <= 1e-5
    assert np.all(aov[count == 0] == 0.0)


@pytest.mark.parametrize("name,W,H,spp", [("cbox_low", 16, 12, 4), ("hardlight", 24, 16, 3), ("caustic", 24, 16, 1)])
def test_gpu_aov_pinned_to_intersect(name, W, H, spp):
    """Diffuse walls (Kd), Phong (min(Kd + Ks, 1)), glass and the emitter (1), spp 1 without
    jitter; odd tile remainders (16 x 12 and 24 x 16 are 2 x 2 and 3 x 2 tiles of 8 x 8)."""
    it = make(variants.obj_path(name), variants.SCENES[name]["camera"], W, H, spp)
    ref, count, _, _ = expected(it)
    assert 0 < (count > 0).sum()
    if name == "hardlight":
        assert {4, 5} & {it.scene.bsdf_type(m)[1] for m in range(it.scene.info()["materials"])}  # a Phong lobe: Kd + Ks
    check_pinned(it, it.render_aov().copy(), ref, count)
    assert it.stats()["samples"] == W * H * spp


def test_gpu_aov_camera_facing_away_is_all_zero():
    it = make(variants.obj_path("cbox_low"), AWAY, 16, 12, 4)
    assert np.all(it.render_aov() == 0.0)


def pixel_err(a, b):
    return np.linalg.norm(a.astype(np.float64) - b, axis=-1) / np.maximum(np.linalg.norm(b.astype(np.float64), axis=-1), 1e-8)


def test_gpu_aov_row_shards_and_windows_sum_to_full():
    cam = variants.SCENES["hardlight"]["camera"]
    full = make(variants.obj_path("hardlight"), cam, 24, 18, 4).render_aov().copy()
    it = make(variants.obj_path("hardlight"), cam, 24, 18, 4)
    for r in range(4):
        it.render_aov(row_offset=r, row_stride=4)
    assert pixel_err(it.aov, full).max() <= 1e-5
    it.init()
    it.render_aov(window=bdpt_amd.SampleWindow(0, 2, 2))
    it.render_aov(window=bdpt_amd.SampleWindow(1, 2, 2))
    assert pixel_err(it.aov, full).max() <= 1e-5


def test_gpu_aov_empty_window_invalid_window_and_flags():
    it = make(variants.obj_path("cbox_low"), variants.SCENES["cbox_low"]["camera"], 16, 12, 4)
    it.aov[:] = 7.0
    it.render_aov(window=bdpt_amd.SampleWindow(1, 1, 0))
    assert np.all(it.aov == 7.0) and it.stats()["samples"] == 0
    with pytest.raises(bdpt_amd.BdptError, match="count") as e:
        it.render_aov(window=bdpt_amd.SampleWindow(2, 1, 3))
    assert e.value.code == bdpt_amd.ERR_INVALID
    import ctypes
    p = it.params(0, 1, 1)
    rc = bdpt_amd.lib().bdpt_render_aov_host(it._h, ctypes.byref(p), None, it.aov.ctypes.data)
    assert rc == bdpt_amd.ERR_UNSUPPORTED and b"flags" in bdpt_amd.lib().bdpt_last_error()
    assert np.all(it.aov == 7.0)


def test_gpu_aov_reads_the_texture_maps():
    """scenes/tex/texbox.obj: Kd / Ks are the texels at the hits. A pixel is left out only
    if one of its samples has st.x * w or st.y * h within 1e-3 of an integer (the lookup's
    truncation may then fall either way); at most 5 % of the textured pixels."""
    with open(os.path.join(REPO, "tests", "golden", "tex_manifest.json")) as f:
        cam = {k: tuple(v) if isinstance(v, list) else v for k, v in json.load(f)["camera"].items()}
    it = make(os.path.join(TEX, "texbox.obj"), cam, 24, 24, 4)
    ref, count, edge, mapped = expected(it)
    aov = it.render_aov().copy()
    assert mapped.sum() >= 200
    share = (edge & mapped).sum() / mapped.sum()
    print(f"left out: {(edge & mapped).sum()} of {mapped.sum()} textured pixels ({100 * share:.2f} %)")
    assert share <= 0.05
    assert np.array_equal(aov[..., 7], count.astype(np.float32) * np.float32(0.25))
    err = group_err(aov, ref)
    assert err[~edge].max() <= 1e-5
    # the maps are read: the materials' constants (what the untextured twin holds) do not pass
    const, _, _, _ = expected(it, textured=False)
    assert (group_err(aov, const)[mapped] > 1e-2).mean() >= 0.25


def test_gpu_aov_many_materials(tmp_path):
    """408 materials: more than the frame kernels' LDS BSDF table holds; the feature buffers
    read materials from HBM and are still the pinned values (chips of all four kinds)."""
    obj = variants.many_materials_obj(str(tmp_path))
    cam = dict(variants.SCENES["cbox_low"]["camera"], eye=(0.0, 2.2, 3.0), at=(0.0, 0.0, 0.0))
    it = make(obj, cam, 24, 16, 2)
    assert it.scene.info()["materials"] == 408
    ref, count, _, _ = expected(it)
    mats = set(it.intersect(driver_rays(it))["mat_id"].tolist())
    assert len(mats) > 10
    check_pinned(it, it.render_aov().copy(), ref, count)
