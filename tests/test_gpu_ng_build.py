"""The frame-kernel build without glossy lobes (bdpt_kernels_ng.hip, BDPT_GLOSSY 0).

A scene whose device material table holds only diffuse, mirror and glass records
(after the upload runs a Ks = 0 mixture as diffuse) renders with this build wherever
it would otherwise launch the default megakernel; BDPT_NG_BUILD=0 forces the full
build, =1 asks for the other and is ignored where the table has a glossy record.
bdpt_last_kernel names both "bdpt_frame_kernel"; stats()["kernel_glossy"] tells them
apart. The checks are the suite's: frame goldens at test_gpu_parity's bound and
metric (per-pixel relative L2 <= 1e-4), and the counting pass equal to the oracle's
counters as in test_gpu_counters, which pins that removing branches steered no path.
"""
import json
import os

import numpy as np
import pytest

import bdpt_amd
import oracle as O
import variants
from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_parity.py

_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = bdpt_amd.Scene(variants.obj_path(name))
    return _scenes[name]


def rel_l2(fb, ref):  # per pixel, as tests/test_gpu_parity.py
    a = fb.reshape(-1, 3).astype(np.float64)
    r = ref.reshape(-1, 3).astype(np.float64)
    return np.linalg.norm(a - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-8)


def render_golden(name, manifest, **kw):
    """The golden frame `name` rendered now: (worst per-pixel rel L2, stats)."""
    m = manifest["framebuffers"][name]
    cam = bdpt_amd.Camera(**variants.SCENES[m["scene"]]["camera"])
    cfg = bdpt_amd.Config(camera=cam, width=m["width"], height=m["height"], spp=m["spp"], rr_depth=m["rr_depth"], **kw)
    it = bdpt_amd.BDPTIntegrator(scene(m["scene"]), cfg)
    it.init()
    fb = it.render_frame(row_offset=0, row_stride=m["row_stride"]).reshape(-1)
    st = it.stats()
    assert st["samples"] == m["samples"] and st["schedule_errors"] == 0
    assert np.all(np.isfinite(fb))
    return rel_l2(fb, load_golden(name)).max(), st


def counting_pass(name, W, H, spp, rr):
    cam = bdpt_amd.Camera(**variants.SCENES[name]["camera"])
    it = bdpt_amd.BDPTIntegrator(scene(name), bdpt_amd.Config(camera=cam, width=W, height=H, spp=spp, rr_depth=rr))
    it.init()
    it.render_frame(flags=bdpt_amd.FLAG_COUNT)
    return it.stats()


def assert_oracle_counters(st, name, W, H, spp, rr):
    """tests/test_gpu_counters.py's equality: what steers a path, then the queries."""
    O.counters(True)
    _, n_ref = O.Scene(variants.obj_path(name)).render(O.make_params(variants.SCENES[name]["camera"], W, H, spp, rr))
    o = O.counters(True)
    g = st["counters"]
    assert st["samples"] == n_ref == W * H * spp
    pairs = {k: (g[k], o[k]) for k in ("rng_draws", "light_verts", "light_vert_reads", "shadow_rays", "splats")}
    pairs["closest_rays"] = (g["closest_rays"], o["closest_rays"] - o["eye_retraces"])
    bad = {k: v for k, v in pairs.items() if v[0] != v[1]}
    assert not bad, f"counters differ from the oracle's (gpu, oracle): {bad}"


@pytest.mark.parametrize("name", ["G2_caustic_64x64_spp16", "G5_caustic_80x48_spp1", "G1_cbox_low_64x64_spp4"])
@pytest.mark.parametrize("env", ["1", "0"])
def test_gpu_both_builds_match_the_golden(name, env, golden_manifest, monkeypatch):
    monkeypatch.setenv("BDPT_NG_BUILD", env)
    worst, st = render_golden(name, golden_manifest)
    print(f"{name} BDPT_NG_BUILD={env}: max per-pixel rel L2 {worst:.3g}, kernel_glossy {st['kernel_glossy']}")
    assert st["kernel"] == "bdpt_frame_kernel"
    assert st["kernel_glossy"] == (0 if env == "1" else 1)
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


def test_gpu_fresh_context_reports_the_key():
    cam = bdpt_amd.Camera(**variants.SCENES["caustic"]["camera"])
    it = bdpt_amd.BDPTIntegrator(scene("caustic"), bdpt_amd.Config(camera=cam, width=8, height=8, spp=1, rr_depth=8))
    it.init()
    st = it.stats()
    assert st["kernel"] == "" and st["kernel_glossy"] == 1  # nothing launched yet


def test_gpu_ng_counting_pass_equals_the_oracle(monkeypatch):
    monkeypatch.setenv("BDPT_NG_BUILD", "1")
    case = ("caustic", 64, 64, 16, 8)
    st = counting_pass(*case)
    assert st["kernel"] == "bdpt_frame_kernel" and st["kernel_glossy"] == 0
    assert_oracle_counters(st, *case)


def test_gpu_default_dispatch_by_material_table(golden_manifest, monkeypatch):
    monkeypatch.delenv("BDPT_NG_BUILD", raising=False)
    # Caustic: diffuse, glass and an illum 8 wall with Ks = 0, which the upload runs as diffuse
    worst, st = render_golden("G2_caustic_64x64_spp16", golden_manifest)
    assert (st["kernel"], st["kernel_glossy"]) == ("bdpt_frame_kernel", 0) and worst <= TOL
    # hardlight_mirror: diffuse and a perfect mirror; the smallest case that runs the mirror sampler in this build
    worst, st = render_golden("G4_hardlight_mirror_64x64_spp16", golden_manifest)
    print(f"hardlight_mirror: max per-pixel rel L2 {worst:.3g}")
    assert (st["kernel"], st["kernel_glossy"]) == ("bdpt_frame_kernel", 0) and worst <= TOL
    # HardLight: a mixture sphere with Ks != 0 keeps the full build in the same branch of the dispatch
    st = counting_pass("hardlight", 64, 64, 16, 8)
    assert (st["kernel"], st["kernel_glossy"]) == ("bdpt_frame_kernel", 1)


def test_gpu_glossy_scene_ignores_the_request(golden_manifest, monkeypatch):
    monkeypatch.setenv("BDPT_NG_BUILD", "1")
    worst, st = render_golden("G3_hardlight_64x64_spp16", golden_manifest)  # rrDepth 2: the short-subpath build
    assert st["kernel_glossy"] == 1 and worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"
    case = ("hardlight", 64, 64, 16, 8)  # the branch of the dispatch that holds the choice
    st = counting_pass(*case)
    assert (st["kernel"], st["kernel_glossy"]) == ("bdpt_frame_kernel", 1)
    assert_oracle_counters(st, *case)


def test_gpu_other_builds_keep_their_kernels(golden_manifest, monkeypatch):
    monkeypatch.setenv("BDPT_NG_BUILD", "1")
    _, st = render_golden("G5_caustic_80x48_spp1", golden_manifest, russian_roulette=1)
    assert st["kernel"] == "bdpt_frame_kernel_rrc" and st["kernel_glossy"] == 1
    m = dict(golden_manifest["framebuffers"]["G5_caustic_80x48_spp1"])
    cam = bdpt_amd.Camera(**variants.SCENES["caustic"]["camera"])
    it = bdpt_amd.BDPTIntegrator(scene("caustic"), bdpt_amd.Config(camera=cam, width=m["width"], height=m["height"],
                                                                    spp=1, rr_depth=3))
    it.init()
    it.render_frame()
    st = it.stats()
    assert st["kernel"] == "bdpt_frame_kernel_split" and st["kernel_glossy"] == 1
    with open(os.path.join(REPO, "tests", "golden", "tex_manifest.json")) as f:
        tex = json.load(f)
    t = tex["frames"]["tex_T1_texbox_bdpt"]
    cam = bdpt_amd.Camera(**{k: tuple(v) if isinstance(v, list) else v for k, v in tex["camera"].items()})
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(os.path.join(REPO, "scenes", "tex", t["obj"])),
                                 bdpt_amd.Config(camera=cam, width=t["width"], height=t["height"], spp=t["spp"],
                                                 rr_depth=t["rr_depth"]))
    it.init()
    fb = it.render_frame()
    st = it.stats()
    assert st["kernel"] == "bdpt_frame_kernel_tex" and st["kernel_glossy"] == 1
    assert rel_l2(fb, load_golden("tex_T1_texbox_bdpt")).max() <= TOL
