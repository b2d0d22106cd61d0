"""What the GPU tests of the plane renders share (tests/test_gpu_layers.py, test_gpu_light_groups.py,
test_gpu_strategies.py, test_gpu_plane_messages.py): the golden cases and their integrators, the
open scene whose paths are known by length, the sums and worst-case metrics over planes, and the
set-ups every plane build refuses. A plain module: no test lives here."""
import json
import os

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import REPO
from test_gpu_parity import rel_l2

STRATEGY = {"bdpt": bdpt_amd.STRATEGY_BDPT, "lt": bdpt_amd.STRATEGY_LIGHT_TRACING, "pt": bdpt_amd.STRATEGY_PATH_TRACING}
with open(os.path.join(REPO, "tests", "golden", "manifest.json")) as _f:
    FRAMES = json.load(_f)["framebuffers"]


def smallest(strategy):
    """The smallest golden (by samples; the manifest's order breaks ties) of the strategy that
    fits 64 x 64 x 16 spp in one shard. synth1m is left out: building its million triangles
    takes longer than every render here together."""
    fit = [(m["samples"], i, n) for i, (n, m) in enumerate(FRAMES.items())
           if m.get("strategy", "bdpt") == strategy and m["width"] <= 64 and m["height"] <= 64 and m["spp"] <= 16
           and m["row_stride"] == 1 and m["scene"] != "synth1m"]
    return min(fit)[2]


BDPT_CASE, LT_CASE, PT_CASE, CBOX_CASE = smallest("bdpt"), smallest("lt"), smallest("pt"), "G1_cbox_low_64x64_spp4"
RING_CASE = "G2_caustic_64x64_spp16"  # glass (delta light vertices) and, at BDPT_TASK_CAP=64, refused pushes
EDGES_CASE = "G14_emit_edges_32x32_spp4"  # five emitters

_scenes = {}


def scene(path):
    if path not in _scenes:
        _scenes[path] = bdpt_amd.Scene(path)
    return _scenes[path]


def golden_integrator(name, **kw):
    m = FRAMES[name]
    args = dict(camera=bdpt_amd.Camera(**variants.SCENES[m["scene"]]["camera"]), width=m["width"], height=m["height"],
                spp=m["spp"], rr_depth=m["rr_depth"], strategy=STRATEGY[m.get("strategy", "bdpt")])
    args.update(kw)
    it = bdpt_amd.BDPTIntegrator(scene(variants.obj_path(m["scene"])), bdpt_amd.Config(**args))
    it.init()
    return it


def bound_of(name):
    m = FRAMES[name]
    return bdpt_amd.layers_longest_path(m["rr_depth"], STRATEGY[m.get("strategy", "bdpt")])


def plane_sum(planes):
    """The float64 sum of (..., H, W, 3) planes over their leading axes."""
    return planes.astype(np.float64).sum(axis=tuple(range(planes.ndim - 3)))


def worst_per_plane(a, b):
    a, b = a.reshape((-1,) + a.shape[-3:]), b.reshape((-1,) + b.shape[-3:])
    return max(rel_l2(a[k], b[k]).max() for k in range(a.shape[0]))


def refused(fn, code, *words, launched=None):
    """fn() raises BdptError with the code and every word in its text. launched: an integrator whose
    launch count the refused call must leave as it was."""
    if launched is not None:
        launched.render_frame()  # (so that the context has stats of a call that launched)
        before = launched.stats()["launches"]
    with pytest.raises(bdpt_amd.BdptError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    if launched is not None:
        assert launched.stats()["launches"] == before, "a refused call launched"
    return str(e.value)


def textured_integrator():
    with open(os.path.join(REPO, "tests", "golden", "tex_manifest.json")) as f:
        tex = json.load(f)
    tm = tex["frames"]["tex_T1_texbox_bdpt"]
    cam = bdpt_amd.Camera(**{k: tuple(v) if isinstance(v, list) else v for k, v in tex["camera"].items()})
    tcfg = bdpt_amd.Config(camera=cam, width=tm["width"], height=tm["height"], spp=tm["spp"], rr_depth=tm["rr_depth"])
    return bdpt_amd.BDPTIntegrator(scene(os.path.join(REPO, "scenes", "tex", tm["obj"])), tcfg)


def unsupported_setups(name, monkeypatch):
    """What no plane build serves, on the golden `name`: (integrator, render keywords, a word of the
    refusal) for Russian roulette, rr_depth 29, flags, a textured scene and a BSDF table in HBM."""
    yield golden_integrator(name, russian_roulette=bdpt_amd.RR_LUMINANCE), {}, "Russian roulette"
    yield golden_integrator(name, rr_depth=29), {}, "rr_depth"
    yield golden_integrator(name), dict(flags=bdpt_amd.FLAG_COUNT), "flags"
    yield textured_integrator(), {}, "texture"
    with monkeypatch.context() as mp:  # (the context reads it when it is created)
        mp.setenv("BDPT_BSDF_IN_HBM", "1")
        hbm = golden_integrator(name)
    yield hbm, {}, "HBM"


# The open scene: camera -> emitter is one edge, camera -> floor -> emitter two, nothing longer carries energy.
OPEN_OBJ = os.path.join(REPO, "scenes", "kat", "layers_open.obj")
OPEN_CAMERA = dict(eye=(0.0, 0.6, 3.0), at=(0.0, 0.6, 0.0), up=(0.0, 1.0, 0.0), fov=45.0)
OPEN_W = OPEN_H = 48


def open_integrator(spp, strategy=bdpt_amd.STRATEGY_BDPT):
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**OPEN_CAMERA), width=OPEN_W, height=OPEN_H, spp=spp, rr_depth=5,
                          strategy=strategy)
    it = bdpt_amd.BDPTIntegrator(scene(OPEN_OBJ), cfg)
    it.init()
    return it


def dilate(mask):
    """The mask and the 8 neighbours of each of its pixels."""
    p = np.pad(mask, 1)
    out = np.zeros_like(mask)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out


@pytest.fixture(scope="module")
def open_first_hits():
    """Per pixel, what the frame's own spp = 1 camera ray hits first: (emitter mask, floor mask)."""
    it = open_integrator(1)
    px = np.arange(OPEN_W * OPEN_H, dtype=np.uint32)
    rec = np.stack([px, np.zeros_like(px), np.zeros_like(px)], axis=1)
    d = it.debug_sampling("camera", rec).view(np.float32)
    rays = np.zeros((px.size, 8), np.float32)
    rays[:, 0:3] = OPEN_CAMERA["eye"]
    rays[:, 3:6] = d
    rays[:, 6], rays[:, 7] = 1.0, 1000.0  # the camera ray's range (renderer.cpp)
    hit = it.intersect(rays)
    got = hit["hit"] == 1
    y = hit["p"][:, 1]  # the emitter quad lies at y = 1.3, the floor at y = 0
    emitter = (got & (y > 0.5)).reshape(OPEN_H, OPEN_W)
    floor = (got & (y <= 0.5)).reshape(OPEN_H, OPEN_W)
    assert emitter.sum() >= 4 and floor.sum() >= 100 and not (emitter & floor).any()  # the camera sees both
    assert not dilate(emitter)[floor].any()  # and they are apart in the image
    return emitter, floor
