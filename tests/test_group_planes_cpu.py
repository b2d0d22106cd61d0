"""Crossed planes, the parts that need no GPU: the library's new symbols with the
argument types the Python mirror declares (checked against the header by a C compiler), the host
model of the combine order against a float64 sum and against the relight definition, the Python
wrappers' shape and argument checks, and the command line's --cross usage errors before any device
is opened."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd
import variants

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RENDER = "bdpt_ctx*, const bdpt_frame_params*, const bdpt_sample_window*, const int32_t*, int32_t, "
COMBINE = "const float*, int32_t, int32_t, int32_t, int32_t, const float*, const float*, float*"
# the header's declarations, as function-pointer types a C compiler checks the entries against
C_TYPES = {
    "bdpt_render_group_layers": f"int (*)({RENDER}int32_t, float*, void*)",
    "bdpt_render_group_layers_host": f"int (*)({RENDER}int32_t, float*)",
    "bdpt_render_group_strategies": f"int (*)({RENDER}int32_t, int32_t, int32_t, float*, void*)",
    "bdpt_render_group_strategies_host": f"int (*)({RENDER}int32_t, int32_t, int32_t, float*)",
    "bdpt_group_planes_combine": f"int (*)(bdpt_ctx*, {COMBINE}, void*)",
    "bdpt_group_planes_combine_host": f"int (*)(bdpt_ctx*, {COMBINE})",
}


def test_library_exports_the_crossed_entry_points_with_the_mirrored_types(tmp_path):
    L = bdpt_amd.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    head = [vp, ctypes.POINTER(bdpt_amd._FrameParams), ctypes.POINTER(bdpt_amd._SampleWindow), vp, i32]
    want = {
        "bdpt_render_group_layers": head + [i32, vp, vp],
        "bdpt_render_group_layers_host": head + [i32, vp],
        "bdpt_render_group_strategies": head + [i32, i32, i32, vp, vp],
        "bdpt_render_group_strategies_host": head + [i32, i32, i32, vp],
        "bdpt_group_planes_combine": [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp],
        "bdpt_group_planes_combine_host": [vp, vp, i32, i32, i32, i32, vp, vp, vp],
    }
    assert set(want) == set(C_TYPES)
    for name, types in want.items():
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == types, name
    lines = ['#include "bdpt_amd.h"', "int main(void) {"]
    for k, (name, ctype) in enumerate(C_TYPES.items()):
        lines.append(f"    {ctype.replace('(*)', f'(*f{k})')} = {name};")
        lines.append(f"    (void)f{k};")
    lines += ["    return 0;", "}"]
    src = tmp_path / "crossed_decl.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_refused_without_a_device():
    L = bdpt_amd.lib()
    p = bdpt_amd._FrameParams()
    one = np.zeros(3, np.float32)
    assert L.bdpt_render_group_layers(None, ctypes.byref(p), None, None, 1, 1, one.ctypes.data, None) == bdpt_amd.ERR_INVALID
    assert L.bdpt_render_group_strategies_host(None, ctypes.byref(p), None, None, 1, 1, 1, 0, one.ctypes.data) == bdpt_amd.ERR_INVALID
    assert L.bdpt_group_planes_combine(None, one.ctypes.data, 1, 1, 1, 1, None, None, one.ctypes.data, None) == bdpt_amd.ERR_INVALID
    assert L.bdpt_group_planes_combine_host(None, one.ctypes.data, 1, 1, 1, 1, None, None, one.ctypes.data) == bdpt_amd.ERR_INVALID
    assert b"null argument" in L.bdpt_last_error()


def test_combine_model_against_a_float64_sum():
    """The float32 loop of include/bdpt_amd.h (what tests/test_gpu_group_planes.py holds the kernel
    to, bit for bit) against the exact sum: per plane two products and, but for the first, one sum,
    each within half an ulp of its own result, so the error is at most (3 n - 1) * 2^-24 of
    sum |gain * weight * plane| (to first order; the factor 1.01 takes the second)."""
    rng = np.random.default_rng(11)
    G, J = 4, 3
    planes = rng.uniform(0.0, 4.0, (G, J, 6, 5, 3)).astype(np.float32)
    gains = rng.uniform(-2.0, 3.0, (G, 3)).astype(np.float32)
    weights = rng.uniform(-1.0, 2.0, J).astype(np.float32)
    gains[2] = 0.0
    weights[1] = 0.0
    acc = bdpt_amd.combine_group_planes_numpy(planes, gains, weights)
    assert acc.dtype == np.float32 and acc.shape == (6, 5, 3)
    terms = (gains.astype(np.float64)[:, None, None, None, :] * weights.astype(np.float64)[None, :, None, None, None] *
             planes.astype(np.float64))
    exact, scale = terms.sum(axis=(0, 1)), np.abs(terms).sum(axis=(0, 1))
    assert (np.abs(acc.astype(np.float64) - exact) <= 1.01 * (3 * G * J - 1) * 2.0 ** -24 * scale).all()


def test_combine_model_order_and_defaults():
    rng = np.random.default_rng(12)
    planes = rng.uniform(0.0, 4.0, (3, 2, 4, 4, 3)).astype(np.float32)
    gains = rng.uniform(-2.0, 3.0, (3, 3)).astype(np.float32)
    model = bdpt_amd.combine_group_planes_numpy
    # both null: the plain ascending float32 sum, groups outer
    seq = None
    for g in range(3):
        for j in range(2):
            seq = planes[g, j].copy() if seq is None else seq + planes[g, j]
    assert np.array_equal(model(planes).view(np.uint32), seq.view(np.uint32))
    # n_inner = 1, null weights: the relight definition (tests/test_light_groups_cpu.py)
    one = planes[:, :1]
    acc = gains[0][None, None, :] * one[0, 0]
    for g in range(1, 3):
        acc = acc + gains[g][None, None, :] * one[g, 0]
    assert np.array_equal(model(one, gains).view(np.uint32), acc.view(np.uint32))
    # grey gains, weights of the inner axes' shape: the (n_groups, n_s, n_t, H, W, 3) layout
    six = planes.reshape(3, 2, 1, 4, 4, 3)
    w = np.float32([[0.5], [-2.0]])
    grey = np.float32([1, 0, 3])
    assert np.array_equal(model(six, grey, w), model(planes, np.repeat(grey[:, None], 3, 1), w.reshape(2)))
    # a zero gain or weight multiplies: an infinite plane value under it is NaN, not skipped
    inf = planes.copy()
    inf[1, 1, 0, 0, 0] = np.inf
    with np.errstate(invalid="ignore"):
        assert np.isnan(model(inf, weights=np.float32([1, 0]))[0, 0, 0])


def test_wrapper_argument_checks_need_no_device():
    check = bdpt_amd._group_planes_args
    ok = np.zeros((2, 3, 4, 4, 3), np.float32)
    a, g, w = check(ok, None, None)
    assert a.shape == (2, 3, 4, 4, 3) and g is None and w is None
    a, g, w = check(np.zeros((2, 3, 2, 4, 4, 3)), [1, 2], np.ones((3, 2)))
    assert a.shape == (2, 6, 4, 4, 3) and a.dtype == np.float32 and g.shape == (2, 3) and w.shape == (6,)
    for bad, word in ((np.zeros((2, 4, 4, 3)), "planes must be"), (np.zeros((2, 3, 4, 4, 4)), "planes must be"),
                      (np.zeros((65, 1, 1, 1, 3)), "n_groups"), (np.zeros((1, 29, 29, 1, 1, 3)), "planes per group"),
                      (np.zeros((2, 3, 0, 4, 3)), "H and W")):
        with pytest.raises(bdpt_amd.BdptError, match=word):
            check(bad, None, None)
    with pytest.raises(bdpt_amd.BdptError, match="2\\^30"):
        check(np.broadcast_to(np.float32(0), (2, 2, 16384, 16384, 3)), None, None)
    for gains, word in ((np.ones((3, 3)), "gains must be"), (np.ones(6), "gains must be"), ([1, np.nan], "not finite")):
        with pytest.raises(bdpt_amd.BdptError, match=word):
            check(ok, gains, None)
    for weights, word in ((np.ones(2), "weights must be"), (np.ones((3, 1)), "weights must be"), ([1, np.inf, 1], "not finite")):
        with pytest.raises(bdpt_amd.BdptError, match=word):
            check(ok, None, weights)
    assert bdpt_amd.GROUP_INNER_MAX == 29 * 28


def test_cli_cross_usage_errors_before_any_device(tmp_path):
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    toml = tmp_path / "scene.toml"
    toml.write_text(variants.toml_text("emit_edges", 16, 16, 1))
    path = tmp_path / "path.toml"
    path.write_text(variants.path_toml_text("emit_edges", 16, 16, 1))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for flags in (["--cross"], ["--cross", "--layers", "3"], ["--cross", "--strategies"], ["--cross", "--light-groups"],
                  ["--cross", "--light-groups", "--layers", "3", "--strategies=unweighted"]):
        r = subprocess.run([cli, str(toml)] + flags, capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode != 0 and "--cross" in r.stderr, (flags, r.stderr)
    # a path scene is refused as for the single flags (not a device error)
    r = subprocess.run([cli, str(path), "--light-groups", "--layers", "3", "--cross"], capture_output=True, text=True,
                       env=env, timeout=60)
    assert r.returncode != 0 and "path" in r.stderr and ("--layers" in r.stderr or "--light-groups" in r.stderr), r.stderr
    assert sorted(os.listdir(tmp_path)) == ["path.toml", "scene.toml"]
