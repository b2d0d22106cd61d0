"""Strategy images, the parts that need no GPU: the library's new symbols with the
argument types the Python mirror declares (checked against the header by a C compiler), the shape
helper's table, the plane-index rule with its clamping, the contact sheet's restatement on the host
(tile placement, the one float32 product per float, the refusals that need no device) and the
command line's refusal of a bad --strategies value before it looks for a scene or a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the header's declarations, as function-pointer types a C compiler checks the entries against
C_TYPES = {
    "bdpt_render_strategies": "int (*)(bdpt_ctx*, const bdpt_frame_params*, const bdpt_sample_window*, int32_t, int32_t, "
                              "int32_t, float*, void*)",
    "bdpt_render_strategies_host": "int (*)(bdpt_ctx*, const bdpt_frame_params*, const bdpt_sample_window*, int32_t, "
                                   "int32_t, int32_t, float*)",
    "bdpt_strategies_sheet": "int (*)(bdpt_ctx*, const float*, int32_t, int32_t, int32_t, int32_t, const float*, float*, "
                             "void*)",
    "bdpt_strategies_shape": "int (*)(int32_t, int32_t, int32_t*, int32_t*)",
}


def test_library_exports_the_strategy_entry_points_with_the_mirrored_types(tmp_path):
    L = bdpt_amd.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    fp, wp = ctypes.POINTER(bdpt_amd._FrameParams), ctypes.POINTER(bdpt_amd._SampleWindow)
    want = {
        "bdpt_render_strategies": [vp, fp, wp, i32, i32, i32, vp, vp],
        "bdpt_render_strategies_host": [vp, fp, wp, i32, i32, i32, vp],
        "bdpt_strategies_sheet": [vp, vp, i32, i32, i32, i32, vp, vp, vp],
        "bdpt_strategies_shape": [i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)],
    }
    for name, types in want.items():
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == types, name
    # the same shapes in the header: -Werror makes a mismatched pointer type an error
    lines = ['#include "bdpt_amd.h"', "int main(void) {"]
    for k, (name, ctype) in enumerate(C_TYPES.items()):
        lines.append(f"    {ctype.replace('(*)', f'(*f{k})')} = {name};")
        lines.append(f"    (void)f{k};")
    lines += ["    return BDPT_STRATEGIES_WEIGHTED + BDPT_STRATEGIES_UNWEIGHTED - 1;", "}"]
    src = tmp_path / "strategies_decl.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (bdpt_amd.STRATEGIES_WEIGHTED, bdpt_amd.STRATEGIES_UNWEIGHTED) == (0, 1)


@pytest.mark.parametrize("strategy", [bdpt_amd.STRATEGY_BDPT, bdpt_amd.STRATEGY_LIGHT_TRACING,
                                      bdpt_amd.STRATEGY_PATH_TRACING])
def test_shape_helper_table(strategy):
    """n_s = max(D, 1) + 1, n_t = max(D, 2), the same for the three strategies."""
    got = [bdpt_amd.strategies_shape(d, strategy) for d in (1, 2, 3, 8, 28)]
    assert got == [(2, 2), (3, 2), (4, 3), (9, 8), (29, 28)]
    n_s, n_t = got[-1]
    assert n_s <= bdpt_amd.STRATEGIES_MAX_S and n_t <= bdpt_amd.STRATEGIES_MAX_T
    assert n_s * n_t * 64 * 64 < 1 << 30  # the deepest render of a 64 x 64 frame fits the pixel field
    for bad in (0, 29, -1):
        with pytest.raises(bdpt_amd.BdptError) as e:
            bdpt_amd.strategies_shape(bad, strategy)
        assert e.value.code == bdpt_amd.ERR_INVALID and "rr_depth" in str(e.value)


def test_shape_helper_refuses_an_unknown_strategy():
    with pytest.raises(bdpt_amd.BdptError) as e:
        bdpt_amd.strategies_shape(5, 3)
    assert e.value.code == bdpt_amd.ERR_INVALID and "strategy" in str(e.value)


def test_plane_index_follows_the_clamping_rule():
    f = bdpt_amd.strategy_plane
    # the full shape of rr_depth 3: nothing clamps, plane = s * n_t + t - 1
    n_s, n_t = 4, 3
    assert [f(s, t, n_s, n_t) for s in range(4) for t in (1, 2, 3)] == list(range(12))
    # longer strategies fall into the last row (s) and the last column (t)
    assert f(4, 1, n_s, n_t) == f(3, 1, n_s, n_t) == 9 and f(9, 2, n_s, n_t) == 10
    assert f(0, 4, n_s, n_t) == f(0, 3, n_s, n_t) == 2 and f(2, 28, n_s, n_t) == 8
    assert f(7, 7, n_s, n_t) == n_s * n_t - 1
    # one row: every s in it; one column: every t in it; (1, 1): one plane takes everything
    assert [f(s, t, 1, 3) for s in (0, 1, 5) for t in (1, 2, 3, 4)] == [0, 1, 2, 2] * 3
    assert [f(s, t, 3, 1) for s in (0, 1, 2, 3) for t in (1, 2, 9)] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2]
    assert {f(s, t, 1, 1) for s in range(30) for t in range(1, 30)} == {0}
    # (2, 2): the shape test 1 of the GPU suite sums the full planes into
    assert [f(s, t, 2, 2) for s in (0, 1, 2) for t in (1, 2, 3)] == [0, 1, 1, 2, 3, 3, 2, 3, 3]
    for bad in ((-1, 1, 2, 2), (0, 0, 2, 2), (0, 1, 0, 2), (0, 1, 2, 0)):
        with pytest.raises(ValueError):
            f(*bad)


def test_sheet_restatement_places_tiles_and_rounds_one_product():
    rng = np.random.default_rng(7)
    n_s, n_t, H, W = 3, 2, 4, 5
    planes = rng.random((n_s, n_t, H, W, 3), dtype=np.float32) * np.float32(3.0)
    sheet = bdpt_amd.strategies_sheet_numpy(planes)
    assert sheet.shape == (n_t * H, n_s * W, 3) and sheet.dtype == np.float32
    for s in range(n_s):
        for t in range(1, n_t + 1):  # the tile of (s, t): column s, row t - 1
            tile = sheet[(t - 1) * H:t * H, s * W:(s + 1) * W]
            assert np.array_equal(tile.view(np.uint32), planes[s, t - 1].view(np.uint32))
    gains = rng.random((n_s, n_t, 3), dtype=np.float32) + np.float32(0.5)
    gained = bdpt_amd.strategies_sheet_numpy(planes, gains)
    for s in range(n_s):
        for r in range(n_t):
            for y in range(H):
                for x in range(W):
                    for c in range(3):  # one float32 product, gain first
                        want = np.float32(gains[s, r, c]) * np.float32(planes[s, r, y, x, c])
                        assert gained[r * H + y, s * W + x, c].view(np.uint32) == want.view(np.uint32)
    # the product is rounded to float32 (not formed in double and cast once more than needed)
    third = np.full((1, 1, 1, 1, 3), np.float32(1) / np.float32(3), np.float32)
    g = np.full((1, 1, 3), np.float32(0.1), np.float32)
    assert bdpt_amd.strategies_sheet_numpy(third, g)[0, 0, 0] == np.float32(0.1) * (np.float32(1) / np.float32(3))
    # grey gains (n_s, n_t) are the RGB gains with three equal channels
    grey = gains[:, :, 0]
    assert np.array_equal(bdpt_amd.strategies_sheet_numpy(planes, grey),
                          bdpt_amd.strategies_sheet_numpy(planes, np.repeat(grey[:, :, None], 3, axis=2)))
    # gain 1 is the copy
    assert np.array_equal(bdpt_amd.strategies_sheet_numpy(planes, np.ones((n_s, n_t, 3), np.float32)), sheet)


def test_sheet_refusals_that_need_no_device():
    f = bdpt_amd.strategies_sheet_numpy
    ok = np.zeros((2, 2, 2, 2, 3), np.float32)
    for bad in (np.zeros((2, 2, 2, 3), np.float32), np.zeros((2, 2, 2, 2, 4), np.float32),
                np.zeros((30, 1, 1, 1, 3), np.float32), np.zeros((1, 29, 1, 1, 3), np.float32),
                np.zeros((0, 1, 1, 1, 3), np.float32)):
        with pytest.raises(bdpt_amd.BdptError):
            f(bad)
    # 2^31 floats or more: refused from the shape alone (a broadcast view, nothing that size exists)
    huge = np.broadcast_to(np.float32(0), (29, 28, 1024, 1024, 3))
    with pytest.raises(bdpt_amd.BdptError) as e:
        f(huge)
    assert "2^31" in str(e.value)
    for g in (np.full((2, 2, 3), np.nan, np.float32), np.full((2, 2), np.inf, np.float32)):
        with pytest.raises(bdpt_amd.BdptError) as e:
            f(ok, g)
        assert "finite" in str(e.value)
    with pytest.raises(bdpt_amd.BdptError):
        f(ok, np.ones((3, 2, 3), np.float32))
    # without a context the library's entry refuses at once (no device is touched)
    rc = bdpt_amd.lib().bdpt_strategies_sheet(None, None, 2, 2, 2, 2, None, None, None)
    assert rc == bdpt_amd.ERR_INVALID


@pytest.mark.parametrize("arg", ["--strategies=bogus", "--strategies=", "--strategiesx"])
def test_cli_refuses_a_bad_strategies_value_before_any_scene_or_device(arg, tmp_path):
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([cli, str(tmp_path / "missing.toml"), arg], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode != 0
    assert "--strategies" in r.stderr and "unweighted" in r.stderr  # not the missing scene file, not a device error
