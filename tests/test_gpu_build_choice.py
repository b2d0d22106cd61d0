"""Which frame-kernel build a render launches (pick_frame_build, bdpt_capi.cpp).

One 32x32 frame at 4 spp per decision of the choice, in its order (textured, Russian
roulette without / with glass, rr_depth > 28, BSDF records in HBM, short subpaths, no
glossy lobe, default), and one per environment override. The expected values are those
of the if / else ladder render_bdpt held before the builds became records
(FrameBuild): the name bdpt_last_kernel reports, kernel_glossy, and one launch per
frame (the continuation pass is off). Images are checked elsewhere
(test_gpu_parity, test_gpu_ng_build, test_gpu_textures, test_gpu_express); here a frame
only has to be finite.
"""
import json
import os

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import REPO

pytestmark = pytest.mark.gpu

ENV = ("BDPT_RR_CHAIN", "BDPT_SPLIT_MAX_RR", "BDPT_NG_BUILD", "BDPT_BSDF_IN_HBM", "BDPT_PARK_DEPTH")

_scenes = {}


def scene_and_camera(name):
    """caustic: diffuse + glass, no glossy record; hardlight: a glossy mixture, no glass;
    texbox: bitmap textures."""
    if name not in _scenes:
        if name == "texbox":
            with open(os.path.join(REPO, "tests", "golden", "tex_manifest.json")) as f:
                tex = json.load(f)
            cam = {k: tuple(v) if isinstance(v, list) else v for k, v in tex["camera"].items()}
            obj = os.path.join(REPO, "scenes", "tex", tex["frames"]["tex_T1_texbox_bdpt"]["obj"])
        else:
            cam, obj = variants.SCENES[name]["camera"], variants.obj_path(name)
        _scenes[name] = (bdpt_amd.Scene(obj), bdpt_amd.Camera(**cam))
    return _scenes[name]


# id: (scene, rr_depth, russian_roulette, env, kernel, kernel_glossy)
CASES = {
    "textured": ("texbox", 8, 0, {}, "bdpt_frame_kernel_tex", 1),
    "textured_before_split": ("texbox", 2, 0, {}, "bdpt_frame_kernel_tex", 1),
    "rr_without_glass": ("hardlight", 8, 1, {}, "bdpt_frame_kernel_rr", 1),
    "rr_with_glass": ("caustic", 8, 1, {}, "bdpt_frame_kernel_rrc", 1),
    "rr_depth_29": ("hardlight", 29, 0, {}, "bdpt_frame_kernel_deep", 1),
    "hbm": ("caustic", 8, 0, {"BDPT_BSDF_IN_HBM": "1"}, "bdpt_frame_kernel_hbm", 1),
    "hbm_before_split": ("caustic", 3, 0, {"BDPT_BSDF_IN_HBM": "1"}, "bdpt_frame_kernel_hbm", 1),
    "rr_depth_3": ("hardlight", 3, 0, {}, "bdpt_frame_kernel_split", 1),
    "split_before_no_glossy": ("caustic", 3, 0, {}, "bdpt_frame_kernel_split", 1),
    "no_glossy": ("caustic", 8, 0, {}, "bdpt_frame_kernel", 0),
    "default": ("hardlight", 8, 0, {}, "bdpt_frame_kernel", 1),
    "RR_CHAIN=0": ("caustic", 8, 1, {"BDPT_RR_CHAIN": "0"}, "bdpt_frame_kernel_rr", 1),
    "RR_CHAIN=1": ("hardlight", 8, 1, {"BDPT_RR_CHAIN": "1"}, "bdpt_frame_kernel_rrc", 1),
    "SPLIT_MAX_RR=0": ("hardlight", 3, 0, {"BDPT_SPLIT_MAX_RR": "0"}, "bdpt_frame_kernel", 1),
    "SPLIT_MAX_RR=0_no_glossy": ("caustic", 3, 0, {"BDPT_SPLIT_MAX_RR": "0"}, "bdpt_frame_kernel", 0),
    "NG_BUILD=0": ("caustic", 8, 0, {"BDPT_NG_BUILD": "0"}, "bdpt_frame_kernel", 1),
    "NG_BUILD=1_glossy_table": ("hardlight", 8, 0, {"BDPT_NG_BUILD": "1"}, "bdpt_frame_kernel", 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_gpu_render_launches_the_build_of_its_case(case, monkeypatch):
    name, rr_depth, rr, env, kernel, glossy = CASES[case]
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, cam = scene_and_camera(name)
    it = bdpt_amd.BDPTIntegrator(sc, bdpt_amd.Config(camera=cam, width=32, height=32, spp=4, rr_depth=rr_depth,
                                                     russian_roulette=rr))
    it.init()  # (the context reads BDPT_BSDF_IN_HBM)
    fb = it.render_frame()
    st = it.stats()
    print(f"{case}: kernel {st['kernel']!r}, kernel_glossy {st['kernel_glossy']}, launches {st['launches']}")
    assert (st["kernel"], st["kernel_glossy"], st["launches"]) == (kernel, glossy, 1)
    assert st["samples"] == 32 * 32 * 4
    assert np.all(np.isfinite(fb))
