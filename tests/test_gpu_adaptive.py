"""Adaptive sampling on the GPU: the pixel-list frame kernel against the strategy build and,
sample by sample, against the C oracle; the resolve and select kernels against their numpy restatements bit
for bit; the driver end to end against render_frame and against adaptive_resolve_numpy in float64 on planes
assembled from the oracle's samples; the command line's files.

Tolerance of the rendered frames: the suite's per-pixel relative L2 <= 1e-4 (tests/test_gpu_parity.py). Two
adaptive runs are never compared with each other: the order of the float atomic additions may flip a pixel
that sits at the threshold."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd
import oracle as O
import variants
from bdpt_amd import SampleWindow
from conftest import gpu_available
from test_config_exr import decode_exr
from test_gpu_parity import TOL, integrator, rel_l2, scene

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

f32 = np.float32
KERNEL = "bdpt_frame_kernel_pixels"
HL_RR = variants.SCENES["hardlight"]["rr_depth"]
CLI = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def plane_err(got, ref):
    return rel_l2(np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)).max()


# ------------------------------------------------------------------ 1. the full list
def test_gpu_full_list_equals_the_strategy_build():
    W, H, spp = 40, 28, 8
    w = SampleWindow(1, 2, 3)
    it = integrator("hardlight", W, H, spp, HL_RR)
    got = it.render_pixels(np.arange(W * H), w)
    st = it.stats()
    assert st["kernel"] == KERNEL and st["samples"] == W * H * 3 and st["schedule_errors"] == 0
    ref = integrator("hardlight", W, H, spp, HL_RR).render_strategies(1, 2, window=w)
    assert got.shape == (2, H, W, 3) and ref.shape == (1, 2, H, W, 3)
    assert ref[0, 0].any() and ref[0, 1].any()
    for t in (0, 1):
        worst = plane_err(got[t], ref[0, t])
        print("plane", t, "max per-pixel rel L2", worst)
        assert worst <= TOL, f"plane {t}: max per-pixel rel L2 {worst:.3g}"


# ------------------------------------------------- 2. a partial list, sample by sample
def oracle_planes(osc, p, pixels, window):
    """(splat plane, eye plane) of the window's samples of the listed pixels from the oracle's per-sample
    entry: the eye estimates summed per pixel and scaled by 1 / spp as the oracle's frame render scales
    them, the samples' splat framebuffers added up."""
    n = p.width * p.height
    eye, splat = np.zeros((n, 3), np.float32), np.zeros(n * 3, np.float32)
    inv_spp = f32(1.0) / f32(p.spp)
    for pixel in pixels:
        acc = np.zeros(3, np.float32)
        for k in window.samples():
            Li, fb = osc.sample(p, int(pixel), k)
            acc += Li
            splat += fb
        eye[pixel] += acc * inv_spp
    return splat.reshape(-1, 3), eye


# pixel 0, the last pixel, a run of neighbours across a row end, scattered ones: 37 pixels
LIST37 = np.array(sorted({0, 200, 255} | set(range(100, 120)) | set(range(5, 100, 7))), np.int32)


@pytest.mark.parametrize("window", [SampleWindow(0, 1, 3), SampleWindow(1, 2, 4)], ids=["0_1_3", "1_2_4"])
def test_gpu_partial_list_equals_its_oracle_samples(window):
    W, H, spp, rr = 16, 16, 8, 5
    assert LIST37.size == 37 and (LIST37.size * window.count) % 64 != 0
    it = integrator("cbox_low", W, H, spp, rr)
    got = it.render_pixels(LIST37, window).reshape(2, -1, 3)
    st = it.stats()
    assert st["kernel"] == KERNEL and st["samples"] == 37 * window.count and st["schedule_errors"] == 0
    p = O.make_params(variants.SCENES["cbox_low"]["camera"], W, H, spp, rr)
    splat, eye = oracle_planes(O.Scene(variants.obj_path("cbox_low")), p, LIST37, window)
    unlisted = np.setdiff1d(np.arange(W * H), LIST37)
    assert not got[1][unlisted].any(), "the eye plane must stay exactly zero at unlisted pixels"
    assert np.all(eye[LIST37].sum(1) > 0) and splat.any()
    e_eye, e_splat = plane_err(got[1], eye), plane_err(got[0], splat)
    print("eye", e_eye, "splat", e_splat)
    assert e_eye <= TOL, f"eye plane: max per-pixel rel L2 {e_eye:.3g}"
    assert e_splat <= TOL, f"splat plane: max per-pixel rel L2 {e_splat:.3g}"


def test_gpu_list_chunks_of_one_pixel_each_on_a_one_block_grid(monkeypatch):
    """count 64 on a 4-pixel list: every 64-sample chunk is one list entry's, and on one block a wave claims
    chunks of different entries one after the other."""
    monkeypatch.setenv("BDPT_DEBUG_KNOBS", "1")
    monkeypatch.setenv("BDPT_GRID_BLOCKS", "1")
    W, H, spp, rr = 16, 16, 128, 5
    window = SampleWindow(1, 2, 64)
    pixels = np.array([3, 100, 101, 250], np.int32)
    it = integrator("cbox_low", W, H, spp, rr)  # (the context reads the knob when it is created)
    got = it.render_pixels(pixels, window).reshape(2, -1, 3)
    assert it.stats()["samples"] == 4 * 64 and it.stats()["kernel"] == KERNEL
    p = O.make_params(variants.SCENES["cbox_low"]["camera"], W, H, spp, rr)
    splat, eye = oracle_planes(O.Scene(variants.obj_path("cbox_low")), p, pixels, window)
    assert not got[1][np.setdiff1d(np.arange(W * H), pixels)].any()
    assert plane_err(got[1], eye) <= TOL and plane_err(got[0], splat) <= TOL


# ---------------------------------------------------- 3. accumulation, the empty list
def test_gpu_pixel_renders_accumulate_and_an_empty_list_launches_nothing():
    W, H, spp = 16, 16, 8
    a_list, b_list = np.arange(0, 200, 3, dtype=np.int32), np.arange(50, 256, dtype=np.int32)
    wa, wb = SampleWindow(0, 2, 2), SampleWindow(1, 2, 3)
    it = integrator("hardlight", W, H, spp, HL_RR)
    one = it.render_pixels(a_list, wa)
    both = it.render_pixels(b_list, wb, out=one.copy())
    alone = it.render_pixels(b_list, wb)
    assert plane_err(both[0], one[0] + alone[0]) <= TOL and plane_err(both[1], one[1] + alone[1]) <= TOL
    before = both.copy()
    for px, w in ((np.zeros(0, np.int32), wa), (a_list, SampleWindow(0, 1, 0))):
        out = it.render_pixels(px, w, out=both)
        st = it.stats()
        assert st["samples"] == 0 and st["launches"] == 0
        assert np.array_equal(bits(out), bits(before))


# ----------------------------------------------------------------------- 4. refusals
def refused(call, code, word, out=None):
    with pytest.raises(bdpt_amd.BdptError) as e:
        call()
    assert e.value.code == code, str(e.value)
    assert word in str(e.value), str(e.value)
    if out is not None:
        assert not out.any()


def test_gpu_pixel_list_refusals_before_any_launch():
    from test_gpu_sample_window import tex_integrator

    W, H, spp = 16, 16, 8
    ok = np.arange(10, dtype=np.int32)
    it = integrator("cbox_low", W, H, spp, 5)
    out = np.zeros((2, H, W, 3), np.float32)
    INV, UNS = bdpt_amd.ERR_INVALID, bdpt_amd.ERR_UNSUPPORTED
    refused(lambda: it.render_pixels(ok, out=out, row_offset=1), INV, "row shard", out)
    refused(lambda: it.render_pixels(ok, out=out, row_stride=2), INV, "row shard", out)
    refused(lambda: it.render_pixels(ok, out=out, flags=bdpt_amd.FLAG_COUNT), UNS, "pixel lists", out)
    refused(lambda: it.render_pixels(ok, SampleWindow(0, 1, 9), out=out), INV, "sample window", out)
    for bad, word in (([5, 3, 7], "ascend"), ([3, 3, 7], "ascend"), ([0, 256], "outside"), ([-1, 2], "outside")):
        refused(lambda: it.render_pixels(np.array(bad, np.int32), out=out), INV, word, out)
    it.set_row_order(np.arange(H)[::-1])
    refused(lambda: it.render_pixels(ok, out=out), INV, "row order", out)
    refused(lambda: it.render_adaptive(0.1, n_batches=4, max_passes=2), INV, "row order")
    it.set_row_order(None)
    assert it.render_pixels(ok, out=out).any()  # the same call once the order is cleared

    cam = bdpt_amd.Camera(**variants.SCENES["cbox_low"]["camera"])
    rr = bdpt_amd.BDPTIntegrator(scene("cbox_low"), bdpt_amd.Config(camera=cam, width=W, height=H, spp=spp, rr_depth=5,
                                                                     russian_roulette=bdpt_amd.RR_LUMINANCE))
    refused(lambda: rr.render_pixels(ok), UNS, "Russian roulette")
    refused(lambda: rr.render_adaptive(0.1, n_batches=4, max_passes=2), UNS, "Russian roulette")
    deep = integrator("cbox_low", W, H, spp, 29)
    refused(lambda: deep.render_pixels(ok), UNS, "rr_depth > 28")
    tex, m = tex_integrator("tex_T1_texbox_bdpt")
    refused(lambda: tex.render_pixels(ok), UNS, "textures")
    refused(lambda: tex.render_adaptive(0.1, n_batches=2, max_passes=m["spp"] // 2), UNS, "textures")
    # the driver: spp is not max_passes * step * n_batches
    refused(lambda: it.render_adaptive(0.1, n_batches=4, step=1, max_passes=3), INV, "spp must equal")
    refused(lambda: it.render_adaptive(0.1, n_batches=3), INV, "spp must equal")  # 8 // 3 = 2 passes: 6 != 8
    assert it.stats()["kernel"] == KERNEL  # (nothing ran since the accepted call)


# ------------------------------------------------------------- 5. resolve, bit for bit
def synthetic_pairs(K, H, W, seed):
    rng = np.random.default_rng(seed)
    pl = rng.random((K, 2, H, W, 3), dtype=np.float32) * f32(2)
    flat = pl.reshape(K, 2, -1)
    flat[:, :, 0::7] = 0.0
    flat[:, :, 1::11] = f32(1e-20)
    flat[:, 1, 2::13] = f32(1e6)
    flat[0, 0, 3::17] = f32(1e6)
    return pl


@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("H,W", [(8, 12), (5, 7)], ids=["unit4", "unit1"])  # 288 floats; 105, no multiple of 4
def test_gpu_resolve_has_the_bits_of_the_float32_loop(K, H, W):
    it = integrator("hardlight", 8, 8, 8, HL_RR)
    pl = synthetic_pairs(K, H, W, 10 * K + H)
    assert ((H * W * 3) % 4 == 0) == (H == 8)
    spp = 6 * K
    rng = np.random.default_rng(K)
    m = rng.integers(0, 7, (H, W)).astype(np.int32)
    m[0, 0], m[H - 1, W - 1], m[1, 1] = 0, 6, 0
    S, v = it.adaptive_resolve(pl, m, spp)
    rs, rv = bdpt_amd.adaptive_resolve_numpy(pl, m, spp)
    assert np.array_equal(bits(S), bits(rs)) and np.array_equal(bits(v), bits(rv))
    assert np.isfinite(S).all() and v.max() > 0
    # uniform m = spp / K: both scales are 1, the bits of batch_moments on E + T
    S, v = it.adaptive_resolve(pl, np.full((H, W), 6, np.int32), spp)
    rs, rv = bdpt_amd.batch_moments_numpy(pl[:, 1] + pl[:, 0])
    assert np.array_equal(bits(S), bits(rs)) and np.array_equal(bits(v), bits(rv))
    # nothing traced
    S, v = it.adaptive_resolve(pl, np.zeros((H, W), np.int32), spp)
    assert not S.any() and not v.any()


# -------------------------------------------------------------- 6. select, bit for bit
def select_both(it, S, var, m, thr, eps, step, m_max, dilate):
    lst, m2 = it.adaptive_select(S, var, m, thr, eps, step, m_max, dilate)
    rl, rm = bdpt_amd.adaptive_select_numpy(S, var, m, thr, eps, step, m_max, dilate)
    assert lst.dtype == np.int32 and np.array_equal(lst, rl), (lst[:8], rl[:8], lst.size, rl.size)
    assert np.array_equal(m2, rm)
    assert np.all(np.diff(lst) > 0)
    return lst, m2


_hl = {}


def hardlight_resolved():
    """HardLight 40 x 28, budget 16 spp in 8 batches: pass 0 (one sample per batch) rendered with the pixel-list
    kernel and resolved on the device. Rendered once, never changed."""
    if not _hl:
        W, H, K = 40, 28, 8
        it = integrator("hardlight", W, H, 16, HL_RR)
        full = np.arange(W * H, dtype=np.int32)
        pl = np.stack([it.render_pixels(full, w) for w in bdpt_amd.adaptive_windows(K, 1, 0)])
        m = np.ones((H, W), np.int32)
        S, v = it.adaptive_resolve(pl, m)
        rs, rv = bdpt_amd.adaptive_resolve_numpy(pl, m, 16)
        assert np.array_equal(bits(S), bits(rs)) and np.array_equal(bits(v), bits(rv))
        _hl.update(it=it, S=S, v=v, m=m)
    return _hl["it"], _hl["S"], _hl["v"], _hl["m"]


@pytest.mark.parametrize("dilate", [False, True])
def test_gpu_select_on_a_rendered_frame_at_its_median_metric(dilate):
    it, S, v, m = hardlight_resolved()
    eps = 1e-3
    s = S.astype(np.float64).sum(-1) + eps
    metric = v.astype(np.float64).sum(-1) / (s * s)
    thr = float(np.sqrt(np.median(metric)))
    lst, m2 = select_both(it, S, v, m, thr, eps, 1, 2, dilate)
    print("median threshold", thr, "active", lst.size, "of", m.size)
    assert 0 < lst.size and m2.sum() == m.sum() + lst.size
    if not dilate:  # strictly above the median: at most half of the pixels
        assert lst.size <= m.size // 2


def test_gpu_select_synthetic_cases():
    it = integrator("hardlight", 8, 8, 8, HL_RR)
    rng = np.random.default_rng(3)
    H, W = 61, 70  # 4270 pixels: five blocks of 1024, the last one partial
    S = rng.random((H, W, 3), dtype=np.float32)
    var = rng.random((H, W, 3), dtype=np.float32) * f32(0.5)
    m = rng.integers(0, 5, (H, W)).astype(np.int32)
    for dilate in (False, True):
        lst, _ = select_both(it, S, var, m, 0.4, 1e-3, 2, 5, dilate)
        assert 0 < lst.size < H * W
        lst, m2 = select_both(it, S, var, np.zeros((H, W), np.int32), 0.0, 1e-3, 1, 4, dilate)  # all active
        assert lst.size == H * W and np.all(m2 == 1)
        lst, m2 = select_both(it, S, var, m, 1e3, 1e-3, 1, 8, dilate)  # none active
        assert lst.size == 0 and np.array_equal(m2, m)
        lst, m2 = select_both(it, S, var, np.full((H, W), 4, np.int32), 0.0, 1e-3, 1, 4, dilate)  # all at the budget
        assert lst.size == 0 and np.all(m2 == 4)
    # values exactly at the threshold are not noisy (strict >), one ulp above are
    S1 = np.full((9, 13, 3), f32(0.25), np.float32)
    rhs = (f32(0.5) * f32(0.5)) * ((f32(0.75) + f32(0.25)) * (f32(0.75) + f32(0.25)))
    v1 = np.zeros_like(S1)
    v1[..., 1] = rhs
    z = np.zeros((9, 13), np.int32)
    assert select_both(it, S1, v1, z, 0.5, 0.25, 1, 4, True)[0].size == 0
    v1[4, 6, 1] = np.nextafter(rhs, f32(np.inf))
    assert list(select_both(it, S1, v1, z, 0.5, 0.25, 1, 4, False)[0]) == [4 * 13 + 6]
    assert select_both(it, S1, v1, z, 0.5, 0.25, 1, 4, True)[0].size == 9
    v1[0, 0, 1] = v1[8, 12, 1] = v1[4, 0, 1] = v1[4, 6, 1]  # the border: clipped, no wrap-around
    assert select_both(it, S1, v1, z, 0.5, 0.25, 1, 4, True)[0].size == 9 + 4 + 4 + 6
    # 1 x W and H x 1 images
    for shape in ((1, 300), (300, 1)):
        Sr = rng.random(shape + (3,), dtype=np.float32)
        vr = rng.random(shape + (3,), dtype=np.float32) * f32(0.3)
        for dilate in (False, True):
            lst, _ = select_both(it, Sr, vr, np.zeros(shape, np.int32), 0.5, 1e-3, 1, 2, dilate)
            assert 0 < lst.size < 300


# ------------------------------------------------------------- 7. the driver, end to end
DW, DH, DK, DC, DPASSES, DSPP, DRR = 16, 16, 4, 1, 4, 16, 5
DEPS = 1e-3


def driver():
    return integrator("cbox_low", DW, DH, DSPP, DRR)


def test_gpu_adaptive_threshold_zero_is_the_plain_frame():
    it = driver()
    frame, var, samples, passes = it.render_adaptive(0.0, n_batches=DK, step=DC, max_passes=DPASSES, eps=DEPS,
                                                     return_passes=True)
    assert it.adaptive["passes"] == DPASSES and it.adaptive["active"] == [DW * DH] * DPASSES
    assert it.adaptive["samples"] == DW * DH * DSPP
    assert len(passes) == DPASSES and all(np.array_equal(p, np.arange(DW * DH)) for p in passes)
    assert np.all(samples == DSPP)
    assert it.stats()["kernel"] == KERNEL
    ref = driver().render_frame()
    worst = plane_err(frame, ref)
    print("threshold 0 against render_frame: max per-pixel rel L2", worst)
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"
    assert var.min() >= 0 and var.max() > 0


def pass0():
    """A threshold above every pixel's metric: one pass."""
    it = driver()
    frame, var, samples = it.render_adaptive(1e6, n_batches=DK, step=DC, max_passes=DPASSES, eps=DEPS)
    return it, frame, var, samples


def test_gpu_adaptive_threshold_above_every_metric_stops_after_one_pass():
    it, frame, var, samples = pass0()
    assert it.adaptive == dict(passes=1, samples=DW * DH * DK * DC, active=[DW * DH])
    assert np.all(samples == DK * DC)
    ref = driver().render_frame(window=SampleWindow(0, 1, DK * DC)) * f32(DSPP // (DK * DC))
    worst = plane_err(frame, ref)
    print("one pass against the scaled window: max per-pixel rel L2", worst)
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


def test_gpu_adaptive_at_the_median_metric_equals_the_oracle_samples_its_lists_name():
    """Without dilation, so that at most half of the pixels stay active after pass 0 whatever the image (the
    dilated rule runs in the threshold-0 test above and, bit for bit, in the select tests)."""
    _, frame0, var0, _ = pass0()
    s = frame0.astype(np.float64).sum(-1) + DEPS
    thr = float(np.sqrt(np.median(var0.astype(np.float64).sum(-1) / (s * s))))
    assert thr > 0
    it = driver()
    frame, var, samples, passes = it.render_adaptive(thr, n_batches=DK, step=DC, max_passes=DPASSES, eps=DEPS,
                                                     dilate=False, return_passes=True)
    N = DW * DH
    assert 2 <= len(passes) <= DPASSES and it.adaptive["active"] == [p.size for p in passes]
    count = np.zeros(N, np.int64)
    for p in passes:
        assert p.dtype == np.int32 and np.all(np.diff(p) > 0) and p.min() >= 0 and p.max() < N
        count[p] += 1
    assert np.array_equal(passes[0], np.arange(N))
    assert np.array_equal(samples.reshape(-1), DK * DC * count)
    assert np.unique(samples).size >= 2
    assert it.adaptive["samples"] == DK * DC * count.sum()
    # the batch planes from the oracle, over exactly the (pixel, pass, batch) triples the lists name
    p = O.make_params(variants.SCENES["cbox_low"]["camera"], DW, DH, DSPP, DRR)
    osc = O.Scene(variants.obj_path("cbox_low"))
    planes = np.zeros((DK, 2, N, 3), np.float64)
    inv_spp = 1.0 / DSPP
    for j, lst in enumerate(passes):
        for b, w in enumerate(bdpt_amd.adaptive_windows(DK, DC, j)):
            for pixel in lst:
                for k in w.samples():
                    Li, fb = osc.sample(p, int(pixel), k)
                    planes[b, 1, pixel] += Li.astype(np.float64) * inv_spp
                    planes[b, 0] += fb.reshape(-1, 3)
    ref, _ = bdpt_amd.adaptive_resolve_numpy(planes.reshape(DK, 2, DH, DW, 3), (DC * count).reshape(DH, DW), DSPP,
                                             np.float64)
    worst = plane_err(frame, ref)
    print("median threshold", thr, "active per pass", it.adaptive["active"], "max per-pixel rel L2", worst)
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


# ------------------------------------------------------------------ 8. the command line
def test_gpu_cli_adaptive_writes_the_frame_its_variance_and_the_sample_map(tmp_path):
    cw, ch, spp = 16, 16, 16
    toml = tmp_path / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", cw, ch, spp))
    for flags, word in ((["--adaptive", "0.3", "--batches", "4"], "--batches"), (["--adaptive", "0.3", "--gpus", "1"], "--gpus"),
                        (["--adaptive", "0.3", "--layers", "2"], "--layers"), (["--adaptive", "0.3", "--light-groups"], "--light-groups"),
                        (["--adaptive", "0.3", "--strategies"], "--strategies"), (["--adaptive", "0.3:8:3"], "spp")):
        r = subprocess.run([CLI, str(toml)] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--adaptive" in r.stderr and word in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == ["scene.toml"]
    r = subprocess.run([CLI, str(toml), "--adaptive", "0.3:4:1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["scene.exr", "scene.toml", "scene_samples.exr", "scene_variance.exr"]
    main, var, smp = (decode_exr((tmp_path / f"scene{s}.exr").read_bytes()).astype(np.float32)
                      for s in ("", "_variance", "_samples"))
    assert main.shape == var.shape == smp.shape == (ch, cw, 3)
    assert np.isfinite(main).all() and main.max() > 0 and var.min() >= 0 and var.max() > 0
    assert set(np.unique(smp)) <= {4.0, 8.0, 12.0, 16.0}, np.unique(smp)  # multiples of step * K up to spp
    assert np.array_equal(smp[..., 0], smp[..., 1]) and np.array_equal(smp[..., 0], smp[..., 2])
    assert "adaptive:" in r.stdout
