"""tinyrender_amd --aov --denoise: the extra EXRs are the Python API's buffers, and the
main EXR is the bytes a run without the flags writes."""
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import gpu_available
from test_config_exr import decode_exr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


def half(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def test_gpu_cli_writes_feature_and_denoised_exrs(tmp_path):
    W = H = 32
    spp = 4
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    for sub in ("plain", "extra"):
        (tmp_path / sub).mkdir()
        (tmp_path / sub / "scene.toml").write_text(variants.toml_text("hardlight", W, H, spp))
    r = subprocess.run([cli, str(tmp_path / "plain" / "scene.toml")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([cli, str(tmp_path / "extra" / "scene.toml"), "--aov", "--denoise"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "plain")) == ["scene.exr", "scene.toml"]
    assert sorted(os.listdir(tmp_path / "extra")) == ["scene.exr", "scene.toml", "scene_albedo.exr",
                                                     "scene_denoised.exr", "scene_normal.exr"]
    main = (tmp_path / "extra" / "scene.exr").read_bytes()
    assert main == (tmp_path / "plain" / "scene.exr").read_bytes()

    sc = variants.SCENES["hardlight"]
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=W, height=H, spp=spp, rr_depth=sc["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path("hardlight")), cfg)
    it.init()
    it.render_aov()
    cov = it.aov[..., 7:8]
    safe = np.where(cov > 0, cov, np.float32(1))
    for name, part in (("albedo", it.aov[..., 0:3]), ("normal", it.aov[..., 3:6])):
        img = decode_exr((tmp_path / "extra" / f"scene_{name}.exr").read_bytes()).astype(np.float32)
        assert np.array_equal(img, half(np.where(cov > 0, part / safe, np.float32(0)))), name
    # the filter is deterministic, but the frame it filters differs between two renders by the
    # order of its atomic additions (as every frame does): one half-precision ulp
    den = decode_exr((tmp_path / "extra" / "scene_denoised.exr").read_bytes()).astype(np.float32)
    rgb = decode_exr(main).astype(np.float32)  # what the CLI rendered, at half precision
    it.render_frame()
    api = it.denoise()
    assert np.allclose(den, half(api), rtol=2 ** -9, atol=1e-6)
    assert np.abs(den - rgb).max() > 0  # it is not the unfiltered frame
