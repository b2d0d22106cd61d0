"""Strategy images (bdpt_render_strategies): one BDPT frame split by the sampling
strategy (s, t) of each contribution, s light-subpath and t eye-subpath vertices (the camera
counted), plane min(s, n_s - 1) * n_t + min(t, n_t) - 1, with the MIS weights or without them.

The weighted planes must add up to the reference's frame (the goldens, per-pixel relative L2 <=
1e-4, tests/test_gpu_parity.py's metric) and to the path-length layers, the (s, t) index must be
right in absolute terms (scenes/kat/layers_open.obj), the shape helper's bound must be tight, the
unweighted t = 1 planes plus (0, 2) must be the reference's LIGHT_TRACING frame (goldens G9 / G11:
the one check of "unweighted" against the compiled reference), the weights must act as weights,
row shards and sample windows must commute with the split, the ring-full fallback must carry the
strategy, the contact sheet must have the bits of the loop on the host, and what the build does
not serve must be refused.

Frames are at most 64 x 64 x 16 spp (one 64-pixel row at 64 spp for the windows). A render is made
once per (case, shape, weighting) and shared."""
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import gpu_available, load_golden
from plane_cases import (BDPT_CASE, CBOX_CASE, EDGES_CASE, FRAMES, LT_CASE, OPEN_H, OPEN_W, PT_CASE, RING_CASE, STRATEGY,  # noqa: F401
                         bound_of, dilate, golden_integrator, open_first_hits, open_integrator, plane_sum, refused, scene,
                         unsupported_setups, worst_per_plane)
from test_config_exr import decode_exr
from test_gpu_layers import layers_of
from test_gpu_parity import TOL, rel_l2

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

CAUSTIC_CASE, HARDLIGHT_CASE = RING_CASE, "G3_hardlight_64x64_spp16"  # G2, G3: the BDPT twins of G9, G11
KERNEL = {False: "bdpt_frame_kernel_strat", True: "bdpt_frame_kernel_strat_unweighted"}

_planes = {}


def shape_of(name):
    m = FRAMES[name]
    return bdpt_amd.strategies_shape(m["rr_depth"], STRATEGY[m.get("strategy", "bdpt")])


def planes_of(name, shape=None, unweighted=False):
    """The strategy render of a golden's frame, made once (read-only: callers do not write to it)."""
    shape = shape or shape_of(name)
    key = (name, shape, unweighted)
    if key not in _planes:
        it = golden_integrator(name)
        out = it.render_strategies(shape[0], shape[1], unweighted=unweighted)
        st = it.stats()
        assert st["kernel"] == KERNEL[unweighted], st["kernel"]
        assert st["schedule_errors"] == 0 and st["samples"] == FRAMES[name]["samples"]
        assert out.shape == (shape[0], shape[1], FRAMES[name]["height"], FRAMES[name]["width"], 3)
        assert out.dtype == np.float32 and np.isfinite(out).all() and (out >= 0).all()
        out.setflags(write=False)
        _planes[key] = out
    return _planes[key]


def P(planes, s, t):
    return planes[s, t - 1]


def means(planes):
    return {(s, r + 1): float(f"{planes[s, r].mean():.3g}") for s in range(planes.shape[0])
            for r in range(planes.shape[1]) if planes[s, r].any()}


def clamp_to(full, n_s, n_t):
    """The full-shape planes summed (float64) into the planes of a smaller shape by the clamping rule."""
    out = np.zeros((n_s, n_t) + full.shape[2:], np.float64)
    for s in range(full.shape[0]):
        for t in range(1, full.shape[1] + 1):
            p = bdpt_amd.strategy_plane(s, t, n_s, n_t)
            out[p // n_t, p % n_t] += P(full, s, t)
    return out


# ------------------------------------------------ 1. the weighted planes add up to the reference
@pytest.mark.parametrize("name", [CBOX_CASE, CAUSTIC_CASE, LT_CASE, PT_CASE, EDGES_CASE])
def test_gpu_weighted_planes_sum_to_the_reference_frame(name):
    full = planes_of(name)
    ref = load_golden(name)
    worst = rel_l2(plane_sum(full), ref).max()
    print(f"{name} shape {full.shape[:2]}: max per-pixel rel L2 of the plane sum {worst:.3g}; plane means {means(full)}")
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"
    assert not P(full, 0, 1).any() and not P(full, 1, 1).any()  # structurally empty
    one = planes_of(name, (1, 1))
    worst = rel_l2(one[0, 0], ref).max()  # the single plane is the frame
    print(f"{name} shape (1, 1): {worst:.3g}")
    assert worst <= TOL
    small = planes_of(name, (2, 2))
    want = clamp_to(full, 2, 2)
    worst = worst_per_plane(small, want)
    print(f"{name} shape (2, 2) vs the clamped sums of the full planes: {worst:.3g}")
    assert worst <= 1e-4
    assert not small[0, 0].any()  # (0, 1) takes nothing from the longer strategies


# ------------------------------------------------------------ 2. the planes agree with the layers
@pytest.mark.parametrize("name", [CBOX_CASE, CAUSTIC_CASE])
def test_gpu_planes_of_one_length_sum_to_that_layer(name):
    full = planes_of(name)
    n_s, n_t = full.shape[:2]
    bound = bound_of(name)
    layers = layers_of(name, bound + 1)
    worst = 0.0
    for k in range(1, n_s + n_t):  # every k a plane of the shape can hold: s + t - 1
        total = np.zeros(full.shape[2:], np.float64)
        for s in range(n_s):
            t = k + 1 - s
            if 1 <= t <= n_t:
                total += P(full, s, t)
        want = layers[k - 1] if k - 1 < layers.shape[0] else np.zeros_like(layers[0])
        worst = max(worst, rel_l2(total, want).max())
    print(f"{name}: worst per-pixel rel L2 of sum over s + t - 1 = k against layer k - 1: {worst:.3g}")
    assert worst <= 1e-4


# ------------------------------------------------- 3. the strategy index in absolute terms
OPEN_LIT = {"bdpt": {(0, 2), (0, 3), (1, 2), (2, 1)}, "lt": {(0, 2), (2, 1)}, "pt": {(0, 2), (1, 2)}}


@pytest.mark.parametrize("strategy", ["bdpt", "lt", "pt"])
@pytest.mark.parametrize("spp", [1, 8])
def test_gpu_strategy_index_is_absolute_on_the_open_scene(open_first_hits, spp, strategy):
    """Camera -> emitter is (0, 2); camera -> floor -> emitter is (0, 3) by the eye walk, (1, 2) by
    connectToLight and (2, 1) by connectToCamera, and nothing else carries energy (the emitter's Kd
    is 0, the floor is flat and diffuse). An off-by-one in s or t at any of the four sites moves
    energy into a plane that must be empty, or out of one that must not be."""
    emitter, floor = open_first_hits
    it = open_integrator(spp, STRATEGY[strategy])
    n_s, n_t = bdpt_amd.strategies_shape(5, STRATEGY[strategy])
    planes = it.render_strategies()
    assert planes.shape == (n_s, n_t, OPEN_H, OPEN_W, 3) == (6, 5, OPEN_H, OPEN_W, 3)
    assert it.stats()["kernel"] == "bdpt_frame_kernel_strat"
    lit = {(s, t): P(planes, s, t).any(axis=2) for s in range(n_s) for t in range(1, n_t + 1)}
    print(f"{strategy} spp {spp}: non-zero pixels per plane { {k: int(m.sum()) for k, m in lit.items() if m.any()} }")
    for st, m in lit.items():
        if st not in OPEN_LIT[strategy]:
            assert not m.any(), f"plane {st} holds energy"
    assert lit[(0, 2)].any() and not (lit[(0, 2)] & ~dilate(emitter)).any()
    for st in OPEN_LIT[strategy] - {(0, 2)}:
        assert not (lit[st] & ~dilate(floor)).any(), st
        if spp == 8:
            assert lit[st].any(), f"plane {st} is empty"
    if spp == 1:  # no jitter: (0, 2) is exactly the pixels whose ray hits the emitter, at its radiance (Ke)
        assert np.array_equal(lit[(0, 2)], emitter)
        assert np.allclose(P(planes, 0, 2)[emitter], np.float32([17.0, 12.0, 4.0]), rtol=1e-6)
    ref = open_integrator(spp, STRATEGY[strategy]).render_frame()
    assert rel_l2(plane_sum(planes), ref).max() <= TOL


# ------------------------------------------------------------ 4. the shape bound is tight
@pytest.mark.parametrize("rr", [1, 2, 3])
def test_gpu_shape_bound_is_tight(rr):
    """cbox_low 48 x 48 x 8, strategy 0, a shape two larger in each direction than the helper's:
    no plane with s > D or t > D holds anything, and (D, D) and (D, 1) do (D >= 2)."""
    n_s, n_t = bdpt_amd.strategies_shape(rr, bdpt_amd.STRATEGY_BDPT)
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES["cbox_low"]["camera"]), width=48, height=48, spp=8,
                          rr_depth=rr)
    it = bdpt_amd.BDPTIntegrator(scene(variants.obj_path("cbox_low")), cfg)
    it.init()
    planes = it.render_strategies(n_s + 2, n_t + 2)
    print(f"rr_depth {rr}: plane means {means(planes)}")
    for s in range(n_s + 2):
        for t in range(1, n_t + 3):
            if s > rr or t > rr:
                assert not P(planes, s, t).any(), f"rr_depth {rr}: plane ({s}, {t}) is not empty"
    assert not P(planes, 0, 1).any() and not P(planes, 1, 1).any()
    if rr >= 2:
        assert P(planes, rr, rr).any() and P(planes, rr, 1).any()
    else:
        assert not planes.any()


# ------------------------- 5. unweighted: the reference's light tracer on the t = 1 column
@pytest.mark.parametrize("name,lt_golden", [(CAUSTIC_CASE, "G9_caustic_lt_64x64_spp16"),
                                            (HARDLIGHT_CASE, "G11_hardlight_lt_64x64_spp16")])
def test_gpu_unweighted_t1_column_is_the_reference_light_tracer(name, lt_golden):
    """The reference's LIGHT_TRACING build is the t = 1 strategies without weights plus the
    emission the camera sees (bdpt.h:229-231, :355-357), and its light walk makes the draws the
    BDPT build's makes (it runs first, on the same sampler): the unweighted t = 1 planes of the
    BDPT frame plus plane (0, 2) are that build's frame."""
    a, b = FRAMES[name], FRAMES[lt_golden]
    assert all(a[k] == b[k] for k in ("scene", "width", "height", "spp", "rr_depth")) and b["strategy"] == "lt"
    planes = planes_of(name, unweighted=True)
    total = planes[:, 0].astype(np.float64).sum(axis=0) + P(planes, 0, 2)
    worst = rel_l2(total, load_golden(lt_golden)).max()
    print(f"{name} unweighted: sum_s (s, 1) + (0, 2) against {lt_golden}: max per-pixel rel L2 {worst:.3g}")
    assert worst <= TOL


# ------------------------------------------------------------------ 6. weights are weights
@pytest.mark.parametrize("name", [CBOX_CASE, CAUSTIC_CASE, EDGES_CASE])
def test_gpu_weights_are_weights(name):
    w, u = planes_of(name), planes_of(name, unweighted=True)
    n_s, n_t = w.shape[:2]
    ratios = {}
    for s in range(n_s):
        for t in range(1, n_t + 1):
            a, b = P(w, s, t), P(u, s, t)
            assert np.array_equal(a == 0, b == 0), f"plane ({s}, {t}): zero in one render only"
            over = float((a.astype(np.float64) - b.astype(np.float64) * (1 + 1e-4)).max())
            assert over <= 0, f"plane ({s}, {t}): weighted exceeds unweighted by {over:.3g}"
            if b.any():
                ratios[(s, t)] = float(a.sum(dtype=np.float64) / b.sum(dtype=np.float64))
    print(f"{name}: weighted / unweighted totals { {k: float(f'{v:.3g}') for k, v in ratios.items()} }")
    assert P(w, 0, 2).any() and rel_l2(P(w, 0, 2), P(u, 0, 2)).max() <= 1e-4  # never weighted
    inner = [r for (s, t), r in ratios.items() if s >= 2 and t >= 2]
    assert inner and min(inner) < 0.99, "no connection plane lost more than 1 %: the weight was not left out"


@pytest.mark.parametrize("name", [LT_CASE, PT_CASE])
def test_gpu_light_and_path_tracing_carry_no_weights(name):
    worst = worst_per_plane(planes_of(name, unweighted=True), planes_of(name))
    print(f"{name}: unweighted against weighted, worst per-plane per-pixel rel L2 {worst:.3g}")
    assert worst <= 1e-4


# ------------------------------------------------------- 7. decompositions commute
def test_gpu_row_shards_sum_to_the_full_planes():
    full = planes_of(CBOX_CASE)
    n_s, n_t = full.shape[:2]
    parts = [golden_integrator(CBOX_CASE).render_strategies(n_s, n_t, row_offset=o, row_stride=2) for o in (0, 1)]
    # an eye-side contribution (t >= 2) stays in its sample's row; a camera splat (t = 1) lands anywhere
    assert not parts[0][:, 1:, 1::2].any() and not parts[1][:, 1:, 0::2].any()
    worst = worst_per_plane(parts[0] + parts[1], full)
    print(f"two interleaved row shards: worst per-plane per-pixel rel L2 {worst:.3g}")
    assert worst <= 1e-4


def test_gpu_sample_windows_sum_to_the_full_planes():
    """40 + 24 of 64 spp on one pixel row (the whole frame's 64-sample chunks each cover one pixel,
    the windows' chunks do not)."""
    m = FRAMES[CBOX_CASE]
    row = dict(row_offset=40, row_stride=m["height"])
    full = golden_integrator(CBOX_CASE, spp=64).render_strategies(**row)
    a = golden_integrator(CBOX_CASE, spp=64).render_strategies(window=bdpt_amd.SampleWindow(0, 1, 40), **row)
    b = golden_integrator(CBOX_CASE, spp=64).render_strategies(window=bdpt_amd.SampleWindow(40, 1, 24), **row)
    eye = full[:, 1:]  # t >= 2: the sample's own pixel (a camera splat, t = 1, lands on any row)
    assert eye[:, :, 40].any() and not eye[:, :, :40].any() and not eye[:, :, 41:].any() and full[:, 0].any()
    worst = worst_per_plane(a + b, full)
    print(f"sample windows 40 + 24 of 64: worst per-plane per-pixel rel L2 {worst:.3g}")
    assert worst <= 1e-4
    assert rel_l2(plane_sum(full), golden_integrator(CBOX_CASE, spp=64).render_frame(**row)).max() <= TOL


# ------------------------------------------- 8. the ring-full fallback carries the strategy
def test_gpu_ring_full_fallback_carries_the_strategy(monkeypatch):
    """BDPT_TASK_CAP=64 (read when the context is created): pushes are refused and the owner traces
    those shadow rays itself; each such connection must still land in its own plane. A strategy
    render cannot count (flags are refused), so the evidence that the fallback runs is a counting
    pass of the same frame on the same context with the default build, whose schedule this build
    shares (tests/test_gpu_layers.py)."""
    name = CAUSTIC_CASE
    default = planes_of(name)
    monkeypatch.setenv("BDPT_TASK_CAP", "64")
    it = golden_integrator(name)
    small = it.render_strategies()
    assert it.stats()["kernel"] == "bdpt_frame_kernel_strat" and it.stats()["schedule_errors"] == 0
    worst_sum = rel_l2(plane_sum(small), load_golden(name)).max()
    worst = worst_per_plane(small, default)
    print(f"{name} at BDPT_TASK_CAP=64: plane sum vs golden {worst_sum:.3g}, per plane vs default ring {worst:.3g}")
    assert worst_sum <= TOL
    assert worst <= 1e-4
    it.render_frame(flags=bdpt_amd.FLAG_COUNT)
    st = it.stats()
    pushed, refusals = st["sched"]["step_tasks"], st["sched"]["shade_steps"]  # (tests/test_gpu_task_ring.py)
    print(f"{name}: counting pass of the default build at this capacity: pushed {pushed}, refused {refusals}")
    assert refusals > 0, "no push was refused: the ring-full fallback did not run"


# ------------------------------------------------------------------------ 9. the sheet
def test_gpu_sheet_has_the_bits_of_the_host_loop():
    planes = planes_of(CBOX_CASE, (3, 2))  # n_s != n_t
    it = golden_integrator(CBOX_CASE)
    n_s, n_t, H, W = planes.shape[:4]
    rng = np.random.default_rng(11)
    gains = (rng.random((n_s, n_t, 3), dtype=np.float32) * np.float32(4.0)).astype(np.float32)
    gains[1, 0] = 0.0  # a plane switched off
    for g in (None, gains, gains[:, :, 1]):
        got = it.strategies_sheet(planes, g)
        assert got.shape == (n_t * H, n_s * W, 3) and got.dtype == np.float32
        want = bdpt_amd.strategies_sheet_numpy(planes, g)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        again = it.strategies_sheet(planes, g)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    # the tile of (s, t) sits at column s, row t - 1
    got = it.strategies_sheet(planes)
    assert planes[2, 1].any() and np.array_equal(got[H:2 * H, 2 * W:3 * W], planes[2, 1])


def test_gpu_sheet_rejects_bad_inputs():
    import torch

    it = golden_integrator(CBOX_CASE)
    I = bdpt_amd.ERR_INVALID

    d = torch.zeros(2 * 2 * 2 * 4 * 4 * 3, dtype=torch.float32, device="cuda")  # planes, then room for the sheet
    n = 2 * 2 * 4 * 4 * 3
    p, o = d.data_ptr(), d.data_ptr() + 4 * n
    it.strategies_sheet_device(p, 2, 2, 4, 4, None, o)  # the good call
    it.synchronize()
    # a sheet of 2^31 floats or more, from the arguments alone (no such buffer exists; refused before any launch)
    refused(lambda: it.strategies_sheet_device(p, 29, 28, 1024, 1024, None, o), I, "2^31")
    refused(lambda: it.strategies_sheet_device(p, 4, 4, 8192, 8192, None, o), I, "2^31")
    refused(lambda: it.strategies_sheet_device(p, 2, 2, 4, 4, None, p), I, "overlaps")
    refused(lambda: it.strategies_sheet_device(p, 2, 2, 4, 4, None, p + 4 * (n - 1)), I, "overlaps")
    refused(lambda: it.strategies_sheet_device(p + 4 * (n - 1), 2, 2, 4, 4, None, p), I, "overlaps")
    bad = np.ones((4, 3), np.float32)
    for v in (np.nan, np.inf, -np.inf):
        bad[2, 1] = v
        refused(lambda: it.strategies_sheet_device(p, 2, 2, 4, 4, bad, o), I, "gains[2][1]", "finite")
    refused(lambda: it.strategies_sheet_device(p, 0, 2, 4, 4, None, o), I, "n_s")
    refused(lambda: it.strategies_sheet_device(p, 30, 2, 4, 4, None, o), I, "n_s")
    refused(lambda: it.strategies_sheet_device(p, 2, 29, 4, 4, None, o), I, "n_t")
    refused(lambda: it.strategies_sheet_device(p, 2, 2, 0, 4, None, o), I, "width")
    refused(lambda: it.strategies_sheet_device(0, 2, 2, 4, 4, None, o), I, "null")


# ------------------------------------------------- 10. refusals and non-interference
def test_gpu_strategies_unsupported_and_invalid(monkeypatch):
    U, I = bdpt_amd.ERR_UNSUPPORTED, bdpt_amd.ERR_INVALID
    name = CBOX_CASE
    for bad, kw, word in unsupported_setups(name, monkeypatch):
        shape = (4, 4) if word == "rr_depth" else ()  # (the default shape of rr_depth 29 is refused earlier)
        for unweighted in (False, True):
            refused(lambda: bad.render_strategies(*shape, unweighted=unweighted, **kw), U, "strategies", word)
    it = golden_integrator(name)
    refused(lambda: it.render_strategies(0, 2), I, "n_s")
    refused(lambda: it.render_strategies(30, 2), I, "n_s")
    refused(lambda: it.render_strategies(2, 0), I, "n_t")
    refused(lambda: it.render_strategies(2, 29), I, "n_t")
    refused(lambda: it.render_strategies(unweighted=2), I, "weighting")
    refused(lambda: it.render_strategies(unweighted=-1), I, "weighting")
    # n_s * n_t * W * H >= 2^30, in the params only: refused before anything is allocated
    big = golden_integrator(name)
    big.config.width, big.config.height = 32768, 16384
    refused(lambda: big.render_strategies(2, 1), I, "2^30")
    refused(lambda: big.render_strategies(1, 2), I, "2^30")
    big.config.width, big.config.height = 1024, 1024
    refused(lambda: big.render_strategies(32, 32), I, "n_s")  # (the shape is checked first)
    big.config.width, big.config.height = 2048, 1024
    refused(lambda: big.render_strategies(29, 28), I, "2^30")


def test_gpu_plain_frames_around_a_strategy_render_are_unchanged():
    it = golden_integrator(CAUSTIC_CASE)  # caustic: glossy materials, so the default build by name
    before = it.render_frame().copy()
    k0 = it.stats()["kernel"]
    planes = it.render_strategies()
    assert it.stats()["kernel"] == "bdpt_frame_kernel_strat"
    unw = it.render_strategies(unweighted=True)
    assert it.stats()["kernel"] == "bdpt_frame_kernel_strat_unweighted"
    it.rgb[:] = 0
    after = it.render_frame().copy()
    k1 = it.stats()["kernel"]
    assert k0 == k1 == "bdpt_frame_kernel", (k0, k1)
    assert rel_l2(after, before).max() <= 1e-4
    assert rel_l2(before, load_golden(CAUSTIC_CASE)).max() <= TOL
    assert rel_l2(plane_sum(planes), before).max() <= 1e-4
    assert worst_per_plane(unw, planes_of(CAUSTIC_CASE, unweighted=True)) <= 1e-4


# ------------------------------------------------------------------- 11. the command line
def test_gpu_cli_writes_one_exr_per_non_empty_plane_and_the_sheet(tmp_path):
    """--strategies on the small cbox scene at 32 x 32 x 4: one S/T file per plane that is not all
    zero, summing to the main EXR within n half-ulps (n * 2^-11 relative, n the number of files)
    plus 2^-23: the half-rounding argument of tests/test_gpu_layers.py's command-line test (every
    file is rounded to half once, the planes are non-negative, and two renders differ by the order
    of their float32 atomic additions, far below one unit)."""
    W = H = 32
    spp = 4
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    (tmp_path / "scene.toml").write_text(variants.toml_text("cbox_low", W, H, spp))
    r = subprocess.run([cli, str(tmp_path / "scene.toml"), "--strategies"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rr = variants.SCENES["cbox_low"]["rr_depth"]
    n_s, n_t = bdpt_amd.strategies_shape(rr, bdpt_amd.STRATEGY_BDPT)
    # the planes that are not empty, from the library on the same frame
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES["cbox_low"]["camera"]), width=W, height=H, spp=spp,
                          rr_depth=rr)
    it = bdpt_amd.BDPTIntegrator(scene(variants.obj_path("cbox_low")), cfg)
    it.init()
    planes = it.render_strategies()
    names = sorted(f"scene.S{s:02d}T{t:02d}.exr" for s in range(n_s) for t in range(1, n_t + 1) if P(planes, s, t).any())
    assert len(names) >= 4
    assert sorted(os.listdir(tmp_path)) == sorted(names + ["scene.exr", "scene.strategies.exr", "scene.toml"])
    main = decode_exr((tmp_path / "scene.exr").read_bytes()).astype(np.float64)
    total = np.zeros_like(main)
    for f in names:
        part = decode_exr((tmp_path / f).read_bytes()).astype(np.float64)
        assert part.shape == main.shape
        total += part
    tol = len(names) * 2.0 ** -11 * np.maximum(total, main) + 2.0 ** -23
    assert (np.abs(total - main) <= tol).all(), float((np.abs(total - main) / np.maximum(main, 1e-6)).max())
    sheet = decode_exr((tmp_path / "scene.strategies.exr").read_bytes())
    assert sheet.shape[:2] == (n_t * H, n_s * W)
    s, t = 1, 2  # a tile against its own file: the same floats rounded to half the same way
    tile = decode_exr((tmp_path / f"scene.S{s:02d}T{t:02d}.exr").read_bytes())
    assert np.array_equal(sheet[(t - 1) * H:t * H, s * W:(s + 1) * W], tile)
