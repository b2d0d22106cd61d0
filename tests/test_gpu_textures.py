"""Bitmap-textured materials (map_Kd / map_Ks, the reference's BitmapTexture3f) on the
GPU BDPT path: frames of scenes/tex/texbox.obj against the reference's own renders
(tests/golden/make_tex_goldens.py), the single-sample entry, shards, the multi-device
rehearsal and the combinations that are refused instead of rendered wrongly.
Tolerance: per-pixel relative L2 <= 1e-4, the project's bound for every frame golden."""
import json
import os

import numpy as np
import pytest

import bdpt_amd
from conftest import REPO, gpu_available, load_golden
from test_gpu_parity import TOL, rel_l2

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

TEX = os.path.join(REPO, "scenes", "tex")
with open(os.path.join(REPO, "tests", "golden", "tex_manifest.json")) as _f:
    MANIFEST = json.load(_f)
STRATEGY = {"bdpt": bdpt_amd.STRATEGY_BDPT, "lt": bdpt_amd.STRATEGY_LIGHT_TRACING, "pt": bdpt_amd.STRATEGY_PATH_TRACING}
_scenes = {}


def scene(obj):
    if obj not in _scenes:
        _scenes[obj] = bdpt_amd.Scene(os.path.join(TEX, obj))
    return _scenes[obj]


def config(m, **kw):
    cam = bdpt_amd.Camera(**{k: tuple(v) if isinstance(v, list) else v for k, v in MANIFEST["camera"].items()})
    args = dict(camera=cam, width=m["width"], height=m["height"], spp=m["spp"], rr_depth=m["rr_depth"],
                strategy=STRATEGY[m["strategy"]])
    args.update(kw)
    return bdpt_amd.Config(**args)


def integrator(m, **kw):
    it = bdpt_amd.BDPTIntegrator(scene(m["obj"]), config(m, **kw))
    it.init()
    return it


@pytest.mark.parametrize("name", ["tex_T1_texbox_bdpt", "tex_T2_texbox_lt", "tex_T3_texbox_pt", "tex_T4_texbox_bdpt_rr2"])
def test_gpu_textured_frame_matches_reference(name):
    m = MANIFEST["frames"][name]
    it = integrator(m)
    fb = it.render_frame()
    st = it.stats()
    worst = rel_l2(fb, load_golden(name)).max()
    print(name, "max per-pixel rel L2", worst, st["kernel"])
    assert st["kernel"].startswith("bdpt_frame_kernel_tex"), st["kernel"]
    assert st["schedule_errors"] == 0
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


def test_gpu_twin_frame_runs_the_untextured_kernel():
    m = MANIFEST["frames"]["tex_T5_twin_bdpt"]
    it = integrator(m)
    fb = it.render_frame()
    ref = load_golden("tex_T5_twin_bdpt")
    assert it.stats()["kernel"] == "bdpt_frame_kernel"
    assert rel_l2(fb, ref).max() <= TOL
    # the maps are in view: the two reference frames differ on at least a quarter of the pixels
    assert (rel_l2(load_golden("tex_T1_texbox_bdpt"), ref) > 1e-2).mean() >= 0.25


def test_gpu_textured_single_sample_matches_reference():
    """bdpt_render_sample_mt on textured surfaces: Li, the advanced sampler state and the
    splats, compared as tests/test_gpu_kat.py compares the kat_sampler_* records."""
    g = np.load(os.path.join(REPO, "tests", "golden", "tex_kat_sampler_bdpt_texbox.npz"))
    same_bits = lambda a, b: np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    m = dict(obj="texbox.obj", width=int(g["width"]), height=int(g["height"]), spp=int(g["spp"]), rr_depth=int(g["rr"]),
             strategy="bdpt")
    it = integrator(m)
    for i in range(g["rays"].shape[0]):
        r = g["rays"][i]
        s = bdpt_amd.Sampler.from_state(g["state_in"][i])
        Li, splats = it.render_sample(bdpt_amd.Ray(tuple(r[:3]), tuple(r[3:6]), float(r[6]), float(r[7])), s)
        acc = {}
        for px, v in splats:
            acc[px] = acc.get(px, np.zeros(3, np.float32)) + v
        n = int(g["nsplat"][i])
        assert len(acc) == n, (i, len(acc), n)
        for px, rr_, gg, bb in g["splats"][i][: min(n, 16)]:
            got = acc[int(np.float32(px).view(np.int32))]
            assert same_bits(got, np.array([rr_, gg, bb], np.float32)), (i, got)
        assert same_bits(Li, g["Li"][i]), (i, Li, g["Li"][i])
        assert np.array_equal(s.state, g["state_out"][i]), i


def test_gpu_textured_row_shards_sum_to_full_frame():
    m = MANIFEST["frames"]["tex_T1_texbox_bdpt"]
    # (an integrator's frames accumulate in its rgb: one integrator per shard)
    total = integrator(m).render_frame(row_offset=0, row_stride=2) + integrator(m).render_frame(row_offset=1, row_stride=2)
    assert rel_l2(total, load_golden("tex_T1_texbox_bdpt")).max() <= TOL


def test_gpu_textured_multi_device_rehearsal():
    m = MANIFEST["frames"]["tex_T1_texbox_bdpt"]
    r = bdpt_amd.MultiDeviceRenderer(scene(m["obj"]), config(m), [0, 0])
    fb = r.render_frame()
    assert r.stats()["schedule_errors"] == 0
    assert rel_l2(fb, load_golden("tex_T1_texbox_bdpt")).max() <= TOL


def test_gpu_textured_unsupported_combinations():
    m = MANIFEST["frames"]["tex_T1_texbox_bdpt"]
    sc = scene(m["obj"])

    def refused(fn, *words):
        with pytest.raises(bdpt_amd.BdptError) as e:
            fn()
        assert e.value.code == bdpt_amd.ERR_UNSUPPORTED, str(e.value)
        for w in ("texture",) + words:
            assert w in str(e.value), str(e.value)

    refused(lambda: integrator(m, russian_roulette=bdpt_amd.RR_LUMINANCE).render_frame(), "russian_roulette")
    refused(lambda: integrator(m, rr_depth=29).render_frame(), "rr_depth")
    pt = bdpt_amd.PathTracerIntegrator(sc, config(m))
    pt.init()
    refused(pt.render_frame, "path")
    di = bdpt_amd.DirectIntegrator(sc, config(m), bdpt_amd.DirectSettings(sampling_strategy="mis"))
    di.init()
    refused(di.render_frame, "direct")
    it = integrator(m)
    wall = 0  # wall_tex: the first material of texbox.mtl
    up = np.array([[0.0, 0.0, 1.0]], np.float32)
    refused(lambda: it.bsdf_eval([wall], up, up), "bdpt_bsdf")
    # an untextured material of the same scene still evaluates (red: Kd / pi * cos)
    f = it.bsdf_eval([3], up, up)
    assert np.allclose(f, np.array([0.63, 0.065, 0.05], np.float32) / np.pi, rtol=1e-6)
    # and the host-side / geometric calls keep working on the textured scene
    hit = it.intersect(np.array([[0.3, 0.2, 3.6, 0.0, 0.0, -1.0, 1.0, 1000.0]], np.float32))
    assert int(hit["hit"][0]) == 1
