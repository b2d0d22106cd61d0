"""Feature buffers and the filter, the parts that need no GPU: the library's new symbols,
the ctypes mirror of bdpt_denoise_params and DenoiseSettings' defaults against the header,
and the command line's refusal of a bad --denoise=ITER before any device is opened."""
import ctypes
import os
import subprocess

import pytest

import bdpt_amd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_new_entry_points():
    L = bdpt_amd.lib()
    for name in ("bdpt_render_aov", "bdpt_render_aov_host", "bdpt_denoise", "bdpt_denoise_host"):
        assert hasattr(L, name), name


def test_denoise_params_mirror_and_defaults_match_header(tmp_path):
    mirror = bdpt_amd._DenoiseParams
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bdpt_amd.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(bdpt_denoise_params));']
    for fname, _ in mirror._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(bdpt_denoise_params, {fname}));')
    lines.append('    printf("d_iterations %d\\nd_demodulate %d\\n", BDPT_DENOISE_ITERATIONS, BDPT_DENOISE_DEMODULATE);')
    lines.append('    printf("d_sigma_color %.9g\\nd_sigma_normal %.9g\\nd_sigma_depth %.9g\\n", BDPT_DENOISE_SIGMA_COLOR, '
                 'BDPT_DENOISE_SIGMA_NORMAL, BDPT_DENOISE_SIGMA_DEPTH);')
    lines.append('    printf("window %zu\\nframe_params %zu\\n", sizeof(bdpt_sample_window), sizeof(bdpt_frame_params));')
    lines += ["    return 0;", "}"]
    src = tmp_path / "denoise_layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "denoise_layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    layout = {k: float(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert [f for f, _ in mirror._fields_] == ["iterations", "sigma_color", "sigma_normal", "sigma_depth",
                                               "demodulate", "norm"]
    assert ctypes.sizeof(mirror) == layout["size"] == 24
    for fname, _ in mirror._fields_:
        assert getattr(mirror, fname).offset == layout[fname], fname
    assert ctypes.sizeof(bdpt_amd._SampleWindow) == layout["window"]
    assert ctypes.sizeof(bdpt_amd._FrameParams) == layout["frame_params"]
    d = bdpt_amd.DenoiseSettings()
    assert (d.iterations, int(d.demodulate)) == (layout["d_iterations"], layout["d_demodulate"])
    c = d.c(1.0)
    for f in ("sigma_color", "sigma_normal", "sigma_depth"):
        assert getattr(c, f) == ctypes.c_float(layout["d_" + f]).value, f
    assert c.norm == 1.0 and d.c(4 / 3).norm == ctypes.c_float(4 / 3).value


@pytest.mark.parametrize("arg", ["--denoise=9", "--denoise=x", "--denoise=-1", "--denoise="])
def test_cli_refuses_a_bad_denoise_count_before_any_device(arg, tmp_path):
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([cli, str(tmp_path / "missing.toml"), arg], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode != 0
    assert "--denoise" in r.stderr and "[0, 8]" in r.stderr  # not the missing scene file, not a device error
