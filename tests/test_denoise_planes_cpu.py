"""The planes filter (bdpt_denoise_planes), the parts that need no GPU: the library's
new symbols with the argument types the Python mirror declares (checked against the header by a C
compiler), the mode constants, the host restatement against the single-plane one, what it promises of
zero planes and of sums, and the command line's --denoise-planes usage errors before any device is
opened."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bdpt_amd
import variants

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS = ("bdpt_ctx*, int32_t, int32_t, int32_t, const float*, const float*, const float*, int32_t, "
        "const bdpt_denoise_params*, float*, float*")
C_TYPES = {
    "bdpt_denoise_planes": f"int (*)({ARGS}, void*)",
    "bdpt_denoise_planes_host": f"int (*)({ARGS})",
}


def test_library_exports_the_planes_filter_with_the_mirrored_types(tmp_path):
    L = bdpt_amd.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    args = [vp, i32, i32, i32, vp, vp, vp, i32, ctypes.POINTER(bdpt_amd._DenoiseParams), vp, vp]
    for name, types in (("bdpt_denoise_planes", args + [vp]), ("bdpt_denoise_planes_host", args)):
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == types, name
    lines = ['#include "bdpt_amd.h"', "int main(void) {"]
    for k, (name, ctype) in enumerate(C_TYPES.items()):
        lines.append(f"    {ctype.replace('(*)', f'(*f{k})')} = {name};")
        lines.append(f"    (void)f{k};")
    lines += ["    return 0;", "}"]
    src = tmp_path / "denoise_planes_decl.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_mode_constants_match_the_header():
    with open(os.path.join(REPO, "include", "bdpt_amd.h")) as f:
        text = f.read()
    got = {k: int(v) for k, v in re.findall(r"^#define BDPT_DENOISE_PLANES_(\w+)\s+(\d+)\s*$", text, re.M)}
    assert got == {"OWN": bdpt_amd.DENOISE_PLANES_OWN, "SHARED": bdpt_amd.DENOISE_PLANES_SHARED}
    assert bdpt_amd._denoise_planes_mode("own") == got["OWN"] and bdpt_amd._denoise_planes_mode("shared") == got["SHARED"]
    with pytest.raises(bdpt_amd.BdptError, match="mode"):
        bdpt_amd._denoise_planes_mode("both")


def test_null_arguments_are_refused_without_a_device():
    L = bdpt_amd.lib()
    one = np.zeros(8, np.float32)
    d = bdpt_amd.DenoiseSettings().c(1.0)
    assert L.bdpt_denoise_planes(None, 1, 1, 1, one.ctypes.data, one.ctypes.data, None, 1, ctypes.byref(d),
                                 one.ctypes.data, None, None) == bdpt_amd.ERR_INVALID
    assert L.bdpt_denoise_planes_host(None, 1, 1, 1, one.ctypes.data, one.ctypes.data, None, 1, ctypes.byref(d),
                                      one.ctypes.data, None) == bdpt_amd.ERR_INVALID
    assert b"null" in L.bdpt_last_error()


def atrous(color, aov, iterations, sigma_color, sigma_normal, sigma_depth, demodulate, norm, dt=np.float64):
    """bdpt_denoise as the header states it, every operation in `dt` (the restatement of
    tests/test_gpu_denoise.py, copied)."""
    f = dt
    c = color.astype(dt) * f(norm)
    a = aov.astype(dt) * f(norm)
    if iterations == 0:
        return c
    H, W = c.shape[:2]
    cov = a[..., 7]
    hit = cov > 0
    safe = np.where(hit, cov, f(1))
    alb = np.where(hit[..., None], a[..., 0:3] / safe[..., None], f(1))
    N = np.where(hit[..., None], a[..., 3:6] / safe[..., None], f(0))
    z = np.where(hit, a[..., 6] / safe, f(0))
    m = np.maximum(alb, f(1e-3))
    img = c / m if demodulate else c
    kern = np.array([1, 4, 6, 4, 1], dt) / f(16)
    zs = f(sigma_depth) * np.maximum(z, f(1e-6))
    for i in range(iterations):
        s = 1 << i
        sc = f(sigma_color) * f(2.0 ** -i)
        num = np.zeros_like(img)
        den = np.zeros((H, W), dt)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                py = slice(max(0, -oy), min(H, H - oy))
                px = slice(max(0, -ox), min(W, W - ox))
                if py.start >= py.stop or px.start >= px.stop:
                    continue
                qy = slice(py.start + oy, py.stop + oy)
                qx = slice(px.start + ox, px.stop + ox)
                h = kern[dy + 2] * kern[dx + 2]
                if dx == 0 and dy == 0:
                    w = np.ones((H, W), dt)
                else:
                    dc = img[py, px] - img[qy, qx]
                    dn = N[py, px] - N[qy, qx]
                    dz = z[py, px] - z[qy, qx]
                    wc = np.exp(-np.minimum(((dc[..., 0] ** 2 + dc[..., 1] ** 2) + dc[..., 2] ** 2) / (sc * sc), f(80)))
                    wn = np.exp(-np.minimum(((dn[..., 0] ** 2 + dn[..., 1] ** 2) + dn[..., 2] ** 2)
                                            / (f(sigma_normal) * f(sigma_normal)), f(80)))
                    wz = np.exp(-np.minimum((dz * dz) / (zs[py, px] * zs[py, px]), f(80)))
                    w = np.where(hit[py, px] == hit[qy, qx], (wc * wn) * wz, f(0))
                hw = h * w
                num[py, px] += hw[..., None] * img[qy, qx]
                den[py, px] += hw
        img = num / den[..., None]
    return img * m if demodulate else img


def synthetic(n, H=9, W=33, seed=5):
    """Random planes over guides with a normal and a depth ramp and a column of miss pixels."""
    rng = np.random.default_rng(seed)
    planes = rng.uniform(0.0, 2.0, (n, H, W, 3)).astype(np.float32)
    aov = np.zeros((H, W, 8), np.float32)
    aov[..., 0:3] = rng.uniform(0.2, 0.9, (H, W, 3))
    nrm = rng.normal(size=(H, W, 3)) * 0.1 + (0, 0, 1)
    aov[..., 3:6] = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
    aov[..., 6] = 2.0 + 0.01 * np.arange(W)[None, :]
    aov[..., 7] = 1.0
    aov[:, 20] = 0.0
    return planes, aov


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("demodulate", [False, True])
def test_restatement_with_one_plane_is_the_single_plane_filter(demodulate, dt):
    planes, aov = synthetic(1)
    kw = dict(sigma_color=1.5, sigma_normal=0.3, sigma_depth=0.1)
    for iterations in (0, 1, 4):
        s = bdpt_amd.DenoiseSettings(iterations=iterations, demodulate=demodulate, **kw)
        ref = atrous(planes[0], aov, iterations, demodulate=demodulate, norm=2.0, dt=dt, **kw)
        for mode in ("own", "shared"):  # one plane is its own sum: the shared guide is the plane
            out, guide = bdpt_amd.denoise_planes_numpy(planes, aov, mode, None, s, 2.0, dt)
            assert out.dtype == dt and out.shape == planes.shape
            assert np.array_equal(out[0], ref), (mode, iterations)
            assert (guide is None) if mode == "own" else np.array_equal(guide, ref)


def test_restatement_own_mode_is_the_single_plane_filter_per_plane_and_keeps_shapes():
    planes, aov = synthetic(6)
    s = bdpt_amd.DenoiseSettings(iterations=3, sigma_color=1.5)
    out, guide = bdpt_amd.denoise_planes_numpy(planes.reshape(2, 3, 9, 33, 3), aov, "own", None, s, 1.0, np.float64)
    assert guide is None and out.shape == (2, 3, 9, 33, 3)
    for j in range(6):
        ref = atrous(planes[j], aov, 3, 1.5, s.sigma_normal, s.sigma_depth, True, 1.0)
        assert np.array_equal(out.reshape(6, 9, 33, 3)[j], ref), j
    with pytest.raises(bdpt_amd.BdptError, match="guide"):
        bdpt_amd.denoise_planes_numpy(planes, aov, "own", planes[0], s)


def test_restatement_shared_mode_is_linear_in_the_planes():
    """With one set of weights the filtered planes sum to the filtered guide and a relight commutes
    with the filter, in float64 to its rounding; a zero plane stays zero; own mode has neither sum."""
    planes, aov = synthetic(5)
    planes[3] = 0.0
    s = bdpt_amd.DenoiseSettings(iterations=4, sigma_color=0.8)
    out, guide = bdpt_amd.denoise_planes_numpy(planes, aov, "shared", None, s)
    assert np.allclose(out.sum(axis=0), guide, rtol=1e-6, atol=0)  # (G is a float32 sum: 2^-24 per addition)
    assert not out[3].any()
    G = planes.sum(axis=0, dtype=np.float32)
    gains = np.float32([0.5, 2.0, 0.0, 4.0, 0.25])  # powers of two: the relit planes are exact in float32
    relit = gains[:, None, None, None] * planes
    again, _ = bdpt_amd.denoise_planes_numpy(relit, aov, "shared", G, s)
    assert np.allclose((gains[:, None, None, None] * out).sum(axis=0), again.sum(axis=0), rtol=1e-12, atol=0)
    own, _ = bdpt_amd.denoise_planes_numpy(planes, aov, "own", None, s)
    assert not own[3].any()
    assert np.abs(own.sum(axis=0) / guide - 1).max() > 1e-3


def test_cli_denoise_planes_usage_errors_before_any_device(tmp_path):
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    toml = tmp_path / "scene.toml"
    toml.write_text(variants.toml_text("emit_edges", 16, 16, 4))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for flags in (["--denoise-planes"], ["--denoise-planes=own"], ["--denoise-planes", "--denoise"],
                  ["--denoise-planes=foo", "--light-groups"], ["--denoise-planes=", "--layers", "3"],
                  ["--denoise-planesx", "--layers", "3"],
                  ["--denoise-planes", "--light-groups", "--sample-window", "0:1:0"]):
        r = subprocess.run([cli, str(toml)] + flags, capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode != 0 and "--denoise-planes" in r.stderr, (flags, r.stderr)
        assert "device" not in r.stderr.lower(), (flags, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["scene.toml"]
