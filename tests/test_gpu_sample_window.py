"""Sample windows (bdpt_render_window): of every pixel's spp samples only k = first +
i * stride, 0 <= i < count, with the seeds and the 1 / spp weight of the frame's full spp.

Windows that partition range(spp) must add up to the frame the reference rendered
(the goldens), a window alone must be the sum of exactly its samples as the C oracle's
per-sample entry gives them, and the work counters over a partition must equal the
unwindowed frame's as integers. The megakernel's per-wave eye slots are the one place a
window could silently produce a wrong image (a 64-sample chunk covers one pixel iff the
window's count, not spp, is a multiple of 64); those shapes run on a one-block grid
(BDPT_GRID_BLOCKS=1) so that every wave claims many chunks and reuses its slots.

Tolerance: the suite's per-pixel relative L2 <= 1e-4 (tests/test_gpu_parity.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

import bdpt_amd
import bdpt_dist
import oracle as O
import variants
from bdpt_amd import SampleWindow
from conftest import REPO, load_golden
from test_gpu_parity import TOL, integrator, rel_l2, rr_integrator, scene

pytestmark = pytest.mark.gpu

TEX = os.path.join(REPO, "scenes", "tex")
with open(os.path.join(REPO, "tests", "golden", "tex_manifest.json")) as _f:
    TEX_MANIFEST = json.load(_f)


def strided(n, spp):
    """The n residue windows modulo n of range(spp)."""
    return [SampleWindow(i, n, max(0, (spp - i + n - 1) // n)) for i in range(n)]


def tex_integrator(name, **kw):
    m = TEX_MANIFEST["frames"][name]
    cam = bdpt_amd.Camera(**{k: tuple(v) if isinstance(v, list) else v for k, v in TEX_MANIFEST["camera"].items()})
    args = dict(camera=cam, width=m["width"], height=m["height"], spp=m["spp"], rr_depth=m["rr_depth"])
    args.update(kw)
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(os.path.join(TEX, m["obj"])), bdpt_amd.Config(**args))
    it.init()
    return it, m


def golden_integrator(section, name, manifest):
    """(integrator, manifest entry, expected bdpt_last_kernel) of a golden frame."""
    if section == "tex":
        it, m = tex_integrator(name)
        return it, m, "bdpt_frame_kernel_tex"
    m = manifest[section][name]
    if section == "framebuffers":
        kernel = "bdpt_frame_kernel_split" if m["rr_depth"] <= 3 else "bdpt_frame_kernel"
        return integrator(m["scene"], m["width"], m["height"], m["spp"], m["rr_depth"]), m, kernel
    if section == "rr_framebuffers":  # a scene with glass runs the inline-chain build
        kernel = "bdpt_frame_kernel_rrc" if m["scene"] == "caustic" else "bdpt_frame_kernel_rr"
        return rr_integrator(m["scene"], m["width"], m["height"], m["spp"], m["rr_depth"]), m, kernel
    cam = bdpt_amd.Camera(**variants.SCENES[m["scene"]]["camera"])
    cfg = bdpt_amd.Config(camera=cam, width=m["width"], height=m["height"], spp=m["spp"])
    if section == "path_framebuffers":
        it = bdpt_amd.PathTracerIntegrator(scene(m["scene"]), cfg, bdpt_amd.PathSettings(**m["path"]))
    else:
        d = dict(m["direct"])
        it = bdpt_amd.DirectIntegrator(scene(m["scene"]), cfg,
                                       bdpt_amd.DirectSettings(sampling_strategy=d.pop("strategy"), **d))
    it.init()
    return it, m, ""  # the path / direct kernel is no BDPT frame-kernel build


PARTITIONS = [
    # (manifest section, golden, windows(spp))
    ("framebuffers", "G2_caustic_64x64_spp16", lambda spp: [SampleWindow(0, 1, 6), SampleWindow(6, 1, 10)]),
    ("framebuffers", "G2_caustic_64x64_spp16", lambda spp: strided(3, spp)),  # counts 6 / 5 / 5
    ("framebuffers", "G1_cbox_low_64x64_spp4", lambda spp: strided(4, spp)),
    ("framebuffers", "G5_caustic_80x48_spp1", lambda spp: [SampleWindow(0, 1, 1)]),
    ("framebuffers", "G3_hardlight_64x64_spp16", lambda spp: strided(2, spp)),  # the _split build
    ("rr_framebuffers", "R1_caustic_rr_64x64_spp16", lambda spp: [SampleWindow(0, 1, 7), SampleWindow(7, 1, 9)]),
    ("rr_framebuffers", "R5_hardlight_mirror_rr_48x48_spp4", lambda spp: strided(2, spp)),
    ("tex", "tex_T1_texbox_bdpt", lambda spp: strided(3, spp)),
    ("path_framebuffers", "P2_caustic_path_64x64_spp4", lambda spp: [SampleWindow(0, 1, 3), SampleWindow(3, 1, 1)]),
    ("path_framebuffers", "P4_cbox_low_path_implicit_64x64_spp4", lambda spp: strided(2, spp)),
    ("direct_framebuffers", "D5_caustic_direct_mis_48x48_spp4", lambda spp: strided(3, spp)),
    ("framebuffers", "G6_caustic_512x512_spp4_rows16", lambda spp: strided(2, spp)),  # with the row shard
]


@pytest.mark.parametrize("section,name,windows", PARTITIONS,
                         ids=[f"{i}-{n.split('_')[1 if s == 'tex' else 0]}" for i, (s, n, _) in enumerate(PARTITIONS)])
def test_gpu_window_partitions_sum_to_reference_golden(section, name, windows, golden_manifest):
    it, m, kernel = golden_integrator(section, name, golden_manifest)
    wins = windows(m["spp"])
    assert sorted(k for w in wins for k in w.samples()) == list(range(m["spp"]))  # a partition
    stride = m.get("row_stride", 1)
    nrows = len(range(0, m["height"], stride))
    for w in wins:
        it.render_frame(row_offset=0, row_stride=stride, window=w)  # accumulates in it.rgb
        st = it.stats()
        assert st["samples"] == nrows * m["width"] * w.count
        assert st["kernel"] == kernel
        assert st["schedule_errors"] == 0 and st["capped_samples"] == 0
    worst = rel_l2(it.rgb.reshape(-1), load_golden(name)).max()
    print(name, [(w.first, w.stride, w.count) for w in wins], "max per-pixel rel L2", worst)
    assert np.all(np.isfinite(it.rgb))
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


def oracle_window_frame(osc, p, window):
    """The window's frame from the oracle's per-sample entry, combined as tro_render
    combines a pixel's samples: splats are added as the samples run, the eye estimates
    are summed over the pixel's samples and added once, scaled by 1 / spp."""
    L = O.lib()
    fb = np.zeros(p.width * p.height * 3, np.float32)
    Li = np.zeros(3, np.float32)
    inv_spp = np.float32(1.0) / np.float32(p.spp)
    for pixel in range(p.width * p.height):
        acc = np.zeros(3, np.float32)
        for k in window.samples():
            L.tro_sample(osc._h, ctypes.byref(p), pixel, k, Li.ctypes.data, fb.ctypes.data)
            acc += Li
        fb[3 * pixel:3 * pixel + 3] += acc * inv_spp
    return fb


def test_gpu_window_alone_equals_its_oracle_samples():
    W, H, spp, rr = 16, 16, 8, 5
    w = SampleWindow(1, 3, 3)  # k = 1, 4, 7
    it = integrator("cbox_low", W, H, spp, rr)
    fb = it.render_frame(window=w).reshape(-1)
    st = it.stats()
    assert st["samples"] == 16 * 16 * 3
    assert st["kernel"] == "bdpt_frame_kernel" and st["schedule_errors"] == 0
    p = O.make_params(variants.SCENES["cbox_low"]["camera"], W, H, spp, rr)
    ref = oracle_window_frame(O.Scene(variants.obj_path("cbox_low")), p, w)
    assert (ref.reshape(-1, 3).sum(1) > 0).mean() > 0.5
    worst = rel_l2(fb, ref).max()
    print("window (1, 3, 3) alone: max per-pixel rel L2", worst)
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


EXACT = ("closest_rays", "shadow_rays", "light_verts", "splats", "rng_draws")  # counters [0] [1] [4] [6] [7]


def test_gpu_window_partition_runs_exactly_the_frames_samples(golden_manifest):
    """Counting passes: the three stride-3 windows of G2 together issue the rays, store
    the light vertices, splat and draw exactly as the unwindowed frame does, and as the
    oracle does (tests/test_gpu_counters.py: its closest-hit rays minus the re-traced
    primary rays)."""
    m = golden_manifest["framebuffers"]["G2_caustic_64x64_spp16"]
    args = (m["scene"], m["width"], m["height"], m["spp"], m["rr_depth"])
    whole = integrator(*args)
    whole.render_frame(flags=bdpt_amd.FLAG_COUNT)
    ref = whole.stats()
    total = dict.fromkeys(EXACT, 0)
    samples = 0
    it = integrator(*args)
    for w in strided(3, m["spp"]):
        it.render_frame(flags=bdpt_amd.FLAG_COUNT, window=w)
        st = it.stats()
        assert st["schedule_errors"] == 0
        samples += st["samples"]
        for k in EXACT:
            total[k] += st["counters"][k]
        assert it.row_costs(m["height"]).sum() > 0  # bdpt_get_row_costs: the row count is unchanged
    assert samples == ref["samples"] == m["samples"]
    assert total == {k: ref["counters"][k] for k in EXACT}
    O.counters(True)
    _, n = O.Scene(variants.obj_path(m["scene"])).render(O.make_params(variants.SCENES[m["scene"]]["camera"], *args[1:]),
                                                        threads=1)
    o = O.counters(True)
    assert n == samples
    expect = {k: o[k] for k in EXACT}
    expect["closest_rays"] -= o["eye_retraces"]
    assert total == expect
    assert rel_l2(it.rgb.reshape(-1), load_golden("G2_caustic_64x64_spp16")).max() <= TOL  # a counting pass renders too


EYE_SLOT_SHAPES = {
    # spp, windows: count % 64 decides whether a 64-sample chunk covers one pixel
    "a_spp64_as_40_24": (64, [SampleWindow(0, 1, 40), SampleWindow(40, 1, 24)]),   # spp % 64 == 0, count % 64 != 0
    "b_spp128_as_two_stride2": (128, strided(2, 128)),                             # count 64: a chunk's k are strided
    "c_spp96_as_64_32": (96, [SampleWindow(0, 1, 64), SampleWindow(64, 1, 32)]),
}


@pytest.mark.parametrize("shape", sorted(EYE_SLOT_SHAPES))
def test_gpu_window_eye_slot_shapes_on_a_one_block_grid(shape, monkeypatch):
    """cbox_low 16 x 16, rrDepth 5 on one block: each of its 4 waves claims on the order
    of a hundred 64-sample chunks, so the per-wave eye slots (BDPT_EYE_SLOTS = 4) are
    reused all the time. The summed frame must equal the oracle's frame of the same
    configuration; shape (a)'s first window is also compared alone with its oracle
    samples (with the old `spp % 64 == 0` rule its chunks would straddle pixels and
    whole eye estimates would land on the wrong pixel).

    Oracle cost, measured on the 8-CPU build machine with threads=16: the largest shape
    (b, 32 768 samples) takes 0.28 s, (c) 0.48 s, (a) 0.33 s; the 10 240 per-sample calls
    of (a)'s first window 0.36 s."""
    monkeypatch.setenv("BDPT_DEBUG_KNOBS", "1")
    monkeypatch.setenv("BDPT_GRID_BLOCKS", "1")
    spp, wins = EYE_SLOT_SHAPES[shape]
    W, H, rr = 16, 16, 5
    assert sorted(k for w in wins for k in w.samples()) == list(range(spp))
    it = integrator("cbox_low", W, H, spp, rr)  # (the context reads the knob when it is created)
    osc = O.Scene(variants.obj_path("cbox_low"))
    p = O.make_params(variants.SCENES["cbox_low"]["camera"], W, H, spp, rr)
    for i, w in enumerate(wins):
        it.render_frame(window=w)
        st = it.stats()
        assert st["samples"] == W * H * w.count and st["schedule_errors"] == 0
        assert st["kernel"] == "bdpt_frame_kernel"
        if shape.startswith("a_") and i == 0:
            alone = rel_l2(it.rgb.reshape(-1), oracle_window_frame(osc, p, w)).max()
            print(shape, "first window alone: max per-pixel rel L2", alone)
            assert alone <= TOL, f"first window alone: max per-pixel rel L2 {alone:.3g}"
    ref, n = osc.render(p, threads=16)
    assert n == W * H * spp
    worst = rel_l2(it.rgb.reshape(-1), ref).max()
    print(shape, "max per-pixel rel L2", worst)
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


@pytest.mark.parametrize("case,devices", [("G2_caustic_64x64_spp16", [0, 0]), ("tex_T1_texbox_bdpt", [0, 0, 0]),
                                          ("G5_caustic_80x48_spp1", [0, 0])])
def test_gpu_multi_device_sample_sharding_rehearsal(case, devices, golden_manifest):
    """sharding="samples" on a repeated device: device i renders samples i, i + N, ... of
    the whole image (tex_T1: spp 8 over 3 -> 3 / 3 / 2; G5: spp 1 -> the second device
    has an empty window, launches nothing and still joins the sum)."""
    if case.startswith("tex"):
        it, m = tex_integrator(case)
        sc, cfg = it.scene, it.config
    else:
        m = golden_manifest["framebuffers"][case]
        sc = scene(m["scene"])
        cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES[m["scene"]]["camera"]), width=m["width"],
                              height=m["height"], spp=m["spp"], rr_depth=m["rr_depth"])
    r = bdpt_amd.MultiDeviceRenderer(sc, cfg, devices, sharding="samples")
    fb = r.render_frame()
    st = r.stats()
    N = len(devices)
    counts = [len(range(i, m["spp"], N)) for i in range(N)]
    assert counts == [bdpt_dist.sample_shard(i, N, m["spp"]).count for i in range(N)]
    assert st["device_samples"] == [m["width"] * m["height"] * c for c in counts]
    assert st["samples"] == m["width"] * m["height"] * m["spp"]
    assert st["schedule_errors"] == 0 and st["capped_samples"] == 0 and not st["rccl"]
    worst = rel_l2(fb.reshape(-1), load_golden(case)).max()
    print(case, devices, counts, "max per-pixel rel L2", worst)
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


def test_gpu_progressive_render(golden_manifest):
    name = "G2_caustic_64x64_spp16"
    m = golden_manifest["framebuffers"][name]
    args = (m["scene"], m["width"], m["height"], m["spp"], m["rr_depth"])
    first = integrator(*args).render_frame(window=SampleWindow(0, 1, 5)).copy()
    it = integrator(*args)
    done, previews = [], []
    for d, preview in it.render_progressive(5):
        done.append(d)
        previews.append(preview.copy())
    assert done == [5, 10, 15, 16]
    assert rel_l2(previews[-1].reshape(-1), load_golden(name)).max() <= TOL
    assert np.array_equal(previews[-1], it.rgb)
    # the unbiased partial estimate: every contribution carries 1 / spp, so 5 of 16 samples scale by 16 / 5
    assert rel_l2(previews[0].reshape(-1), (first * np.float32(16 / 5)).reshape(-1)).max() <= TOL


@pytest.mark.parametrize("window,word", [((-1, 1, 1), "first"), ((0, 0, 1), "stride"), ((0, 1, -1), "count"),
                                         ((0, 1, 9), "count"), ((2, 3, 3), "count"), ((8, 1, 1), "count")])
@pytest.mark.parametrize("kind", ["bdpt", "path", "direct"])
def test_gpu_window_validation_names_the_field(kind, window, word):
    cam = bdpt_amd.Camera(**variants.SCENES["cbox_low"]["camera"])
    cfg = bdpt_amd.Config(camera=cam, width=8, height=8, spp=8, rr_depth=5)
    sc = scene("cbox_low")
    it = {"bdpt": lambda: bdpt_amd.BDPTIntegrator(sc, cfg),
          "path": lambda: bdpt_amd.PathTracerIntegrator(sc, cfg),
          "direct": lambda: bdpt_amd.DirectIntegrator(sc, cfg, bdpt_amd.DirectSettings(sampling_strategy="mis"))}[kind]()
    it.init()
    with pytest.raises(bdpt_amd.BdptError) as e:
        it.render_frame(window=SampleWindow(*window))
    assert e.value.code == bdpt_amd.ERR_INVALID, str(e.value)
    assert word in str(e.value) and "sample window" in str(e.value), str(e.value)
    assert not it.rgb.any()


def test_gpu_window_edge_cases():
    """count == 0 renders nothing (also past spp: only a non-empty window is bounded); the last
    valid sample is accepted; a null window is the unwindowed entry; path and direct together
    are refused; textures + Russian roulette stay unsupported with a window."""
    it = integrator("cbox_low", 8, 8, 8, 5)
    for w in (SampleWindow(0, 1, 0), SampleWindow(99, 7, 0)):
        fb = it.render_frame(window=w)
        st = it.stats()
        assert st["samples"] == 0 and st["launches"] == 0
        assert not fb.any()
    it.render_frame(window=SampleWindow(7, 5, 1))
    assert it.stats()["samples"] == 64
    whole = integrator("cbox_low", 8, 8, 8, 5).render_frame().copy()
    it2 = integrator("cbox_low", 8, 8, 8, 5)
    p = it2.params()
    bdpt_amd._check(bdpt_amd.lib().bdpt_render_window_host(it2._h, ctypes.byref(p), None, None, None,
                                                           it2.rgb.ctypes.data))
    assert it2.stats()["samples"] == 8 * 8 * 8
    assert rel_l2(it2.rgb.reshape(-1), whole.reshape(-1)).max() <= TOL
    pp, dp = bdpt_amd.PathSettings().c(), bdpt_amd.DirectSettings(sampling_strategy="mis").c()
    rc = bdpt_amd.lib().bdpt_render_window_host(it2._h, ctypes.byref(p), None, ctypes.byref(pp), ctypes.byref(dp),
                                                it2.rgb.ctypes.data)
    assert rc == bdpt_amd.ERR_INVALID
    tex, _ = tex_integrator("tex_T1_texbox_bdpt", russian_roulette=bdpt_amd.RR_LUMINANCE)
    with pytest.raises(bdpt_amd.BdptError) as e:
        tex.render_frame(window=SampleWindow(0, 2, 4))
    assert e.value.code == bdpt_amd.ERR_UNSUPPORTED and "texture" in str(e.value), str(e.value)


def test_gpu_window_render_device_is_asynchronous_on_the_callers_stream(golden_manifest):
    """bdpt_render_window's device form (a torch tensor and stream), path integrator."""
    import torch

    name = "P2_caustic_path_64x64_spp4"
    it, m, _ = golden_integrator("path_framebuffers", name, golden_manifest)
    fb = torch.zeros(m["width"] * m["height"] * 3, dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    for w in strided(2, m["spp"]):
        it.render_device(fb.data_ptr(), s.cuda_stream, window=w)
    s.synchronize()
    it.check_levels()
    assert rel_l2(fb.cpu().numpy(), load_golden(name)).max() <= TOL
