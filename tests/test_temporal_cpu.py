"""Temporal accumulation without a GPU: reproject_numpy (bdpt_amd.py), the float32 restatement the kernel is
pinned to, on the synthetic scene of tests/temporal_cases.py; the ctypes mirror of bdpt_reproject_params; the
argument checks that need no device; the command line's camera file and its refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd
import temporal_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
f32 = np.float32
W, H = 96, 64
PLAIN = bdpt_amd.ReprojectSettings(clamp_sigma=0.0, demodulate=False, max_history=1024.0)  # (a cap that never binds)


def test_static_camera_is_plain_progressive_accumulation():
    """K frames of random colour from one camera, no clamp, no demodulation: every hit pixel lands on itself, so
    n is K n_c exactly and the colour is the frames' mean - each step H + (I - H) * (n_c / n) is three roundings
    of values no larger than the largest addend, hence the bound 4 K 2^-24 max|addend|."""
    K, n_c = 6, 4.0
    aov, dirs, surf, consts = tc.buffers(tc.CAM_A, W, H)
    frames = tc.colours(1, W, H, K)
    hist = None
    for k in range(K):
        out, hist = bdpt_amd.reproject_numpy(frames[k], aov, hist, dirs, consts, consts, PLAIN, cur_samples=n_c)
    hit = surf > 0
    assert hit.any() and (~hit).any() and (surf == 1).any() and (surf == 2).any()
    assert np.array_equal(hist[hit][:, 3], np.full(hit.sum(), K * n_c, f32))
    mean = frames.astype(np.float64).mean(0)
    bound = 4 * K * 2.0 ** -24 * float(frames.max())
    assert np.abs(out[hit].astype(np.float64) - mean[hit]).max() <= bound
    assert np.array_equal(hist[hit][:, 0:3], out[hit])
    # a miss carries the last frame's colour, n_c, and no surface
    assert np.array_equal(out[~hit], frames[-1][~hit])
    assert np.array_equal(hist[~hit][:, 3:], np.tile(f32([n_c, 0, 0, 0, 0]), ((~hit).sum(), 1)))
    assert np.array_equal(hist[hit][:, 4:8], np.concatenate([aov[hit][:, 3:6], aov[hit][:, 6:7]], 1))


@pytest.fixture(scope="module")
def moved():
    """History made at camera A, carried to camera B (a pan and a dolly) with the default acceptance."""
    aovA, dirsA, _, cA = tc.buffers(tc.CAM_A, W, H)
    aovB, dirsB, surfB, cB = tc.buffers(tc.CAM_B, W, H)
    cols = tc.colours(2, W, H, 2)
    s = bdpt_amd.ReprojectSettings(clamp_sigma=0.0, demodulate=False)
    _, histA = bdpt_amd.reproject_numpy(cols[0], aovA, None, dirsA, cA, cA, s, cur_samples=4.0)
    out, histB = bdpt_amd.reproject_numpy(cols[1], aovB, histA, dirsB, cB, cA, s, cur_samples=4.0)
    return cols, out, histB, surfB


def test_moved_camera_drops_history_where_the_slab_uncovered_the_floor(moved):
    cols, out, hist, surfB = moved
    hidden, opened = tc.floor_classes(W, H)
    assert hidden.sum() >= 20 and opened.sum() >= 200, (hidden.sum(), opened.sum())
    assert np.array_equal(hist[hidden][:, 3], np.full(hidden.sum(), 4.0, f32))
    assert np.array_equal(out[hidden], cols[1][hidden])
    assert (hist[opened][:, 3] > 4.0).all(), (hist[opened][:, 3] <= 4.0).sum()
    assert (hist[..., 3] <= 8.0).all()


def test_no_history_is_the_frame_itself_also_demodulated():
    aov, dirs, surf, consts = tc.buffers(tc.CAM_A, W, H)
    col = tc.colours(3, W, H)[0]
    for demod in (False, True):
        s = bdpt_amd.ReprojectSettings(demodulate=demod)
        out, hist = bdpt_amd.reproject_numpy(col, aov, None, dirs, consts, consts, s, norm=2.0, cur_samples=2.0)
        assert np.array_equal(out, col * f32(2))
        assert np.array_equal(hist[..., 3], np.full((H, W), 2.0, f32))
        m = np.maximum(aov[..., 0:3], f32(1e-3))
        want = np.where((surf > 0)[..., None] & demod, (col * f32(2)) / m, col * f32(2))
        assert np.array_equal(hist[..., 0:3], want)


def test_max_history_caps_the_carried_count():
    aov, dirs, surf, consts = tc.buffers(tc.CAM_A, W, H)
    frames = tc.colours(4, W, H, 5)
    s = bdpt_amd.ReprojectSettings(clamp_sigma=0.0, demodulate=False, max_history=2.5)
    hist = None
    for k in range(5):
        _, hist = bdpt_amd.reproject_numpy(frames[k], aov, hist, dirs, consts, consts, s, cur_samples=1.0)
    assert np.array_equal(hist[surf > 0][:, 3], np.full((surf > 0).sum(), 3.5, f32))  # min(n, 2.5) + 1


def test_clamp_pulls_a_far_history_to_the_neighbourhoods_bound():
    """A history of 100 everywhere against a current frame near 1: H becomes mu + k sd of the 3 x 3 covered
    neighbours, per channel, and the blend starts from there."""
    aov, dirs, surf, consts = tc.buffers(tc.CAM_A, W, H)
    col = tc.colours(5, W, H)[0]
    hist = np.zeros((H, W, 8), f32)
    hist[..., 0:3], hist[..., 3] = 100.0, 4.0
    hist[..., 4:8] = np.concatenate([aov[..., 3:6], aov[..., 6:7]], -1)
    k = 1.5
    s = bdpt_amd.ReprojectSettings(clamp_sigma=k, demodulate=False)
    out, state = bdpt_amd.reproject_numpy(col, aov, hist, dirs, consts, consts, s, cur_samples=4.0)
    i, j = np.argwhere(surf == 1)[len(np.argwhere(surf == 1)) // 2]
    assert 0 < i < H - 1 and 0 < j < W - 1 and (surf[i - 1:i + 2, j - 1:j + 2] > 0).all()
    nb = col[i - 1:i + 2, j - 1:j + 2].reshape(9, 3).astype(np.float64)
    hi = nb.mean(0) + k * nb.std(0)
    want = hi + (col[i, j] - hi) * 0.5
    assert state[i, j, 3] == 8.0
    assert np.allclose(out[i, j], want, rtol=1e-5, atol=0)
    assert out[surf > 0].max() < 4.0  # nowhere does the far history survive
    free, _ = bdpt_amd.reproject_numpy(col, aov, hist, dirs, consts, consts,
                                       bdpt_amd.ReprojectSettings(clamp_sigma=0.0, demodulate=False), cur_samples=4.0)
    assert np.allclose(free[i, j], 100.0 + (col[i, j] - 100.0) * 0.5, rtol=1e-6)


def test_float64_restatement_agrees_with_float32():
    aovA, dirsA, _, cA = tc.buffers(tc.CAM_A, W, H)
    aovB, dirsB, _, cB = tc.buffers(tc.CAM_B, W, H)
    cols = tc.colours(6, W, H, 2)
    res = {}
    for dt in (np.float32, np.float64):
        _, h = bdpt_amd.reproject_numpy(cols[0], aovA, None, dirsA, cA, cA, dt=dt, cur_samples=4.0)
        res[dt] = bdpt_amd.reproject_numpy(cols[1], aovB, h, dirsB, cB, cA, dt=dt, cur_samples=4.0)
    same = res[np.float32][1][..., 3] == res[np.float64][1][..., 3]  # (a tap on a threshold may flip)
    assert same.mean() > 0.99
    assert np.allclose(res[np.float32][0][same], res[np.float64][0][same], rtol=1e-4, atol=1e-5)


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("abi_temporal")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bdpt_amd.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(bdpt_reproject_params));']
    for fname, _ in bdpt_amd._ReprojectParams._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(bdpt_reproject_params, {fname}));')
    lines += ['    printf("defaults %g %g %g %g %g %d\\n", BDPT_REPROJECT_MAX_HISTORY, BDPT_REPROJECT_SIGMA_NORMAL, '
              'BDPT_REPROJECT_SIGMA_DEPTH, BDPT_REPROJECT_MIN_WEIGHT, BDPT_REPROJECT_CLAMP_SIGMA, BDPT_REPROJECT_DEMODULATE);',
              "    return 0;", "}"]
    src = d / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[0]: ln.split()[1:] for ln in out.splitlines()}


def test_reproject_params_mirror_matches_the_header(c_layout):
    mirror = bdpt_amd._ReprojectParams
    assert ctypes.sizeof(mirror) == int(c_layout["size"][0])
    for fname, _ in mirror._fields_:
        assert getattr(mirror, fname).offset == int(c_layout[fname][0]), fname
    s = bdpt_amd.ReprojectSettings()
    got = [s.max_history, s.sigma_normal, s.sigma_depth, s.min_weight, s.clamp_sigma, int(s.demodulate)]
    assert [float(x) for x in c_layout["defaults"]] == pytest.approx(got, rel=1e-6)


def test_entries_refuse_bad_arguments_before_they_need_a_device():
    """Every check comes before the context is used, except the null context itself, which is reported first."""
    L = bdpt_amd.lib()
    p = bdpt_amd._FrameParams()
    p.width, p.height, p.spp = 4, 4, 1
    one = np.zeros(4 * 4 * 8, f32)
    r = bdpt_amd.ReprojectSettings().c(bdpt_amd.Camera(), 1.0)
    assert L.bdpt_reproject_host(None, ctypes.byref(p), one.ctypes.data, one.ctypes.data, None, one.ctypes.data,
                                 one.ctypes.data, ctypes.byref(r)) == bdpt_amd.ERR_INVALID
    assert b"null ctx" in L.bdpt_last_error()


@pytest.mark.parametrize("text,word", [
    ("0 0.8 3.8 0 0.8 0 0 1 0\n", "line 1: expected ten numbers"),
    ("# a comment\n\n0 0.8 3.8 0 0.8 0 0 1 0 30\n0 0.8 3.8 0 0.8 0 0 1 0 30 7\n", "line 4: expected ten numbers"),
    ("0 0.8 3.8 0 0.8 0 0 1 0 x\n", "line 1: expected ten numbers"),
    ("0 0.8 3.8 0 0.8 0 0 1 0 0\n", "line 1: fov"),
    ("# nothing\n\n", "no camera line"),
    (None, "cannot read"),
])
def test_command_line_refuses_a_bad_camera_file(text, word, tmp_path):
    import variants

    d = tmp_path / "run"
    d.mkdir()
    toml = d / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", 16, 16, 1))
    cams = tmp_path / "cams.txt"
    if text is not None:
        cams.write_text(text)
    r = subprocess.run([CLI, str(toml), "--cameras", str(cams), "--temporal"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--cameras" in r.stderr and word in r.stderr, r.stderr
    assert sorted(os.listdir(d)) == ["scene.toml"]


GOOD_CAMERAS = "# eye at up fov\n0 0.8 3.8 0 0.8 0 0 1 0 30\n\n  0.05 0.8 3.8 0.05 0.8 0 0 1 0 30  \n"


@pytest.mark.parametrize("args,word", [
    (["--temporal"], "--cameras FILE"), (["--cameras", "CAMS"], "--temporal"),
    (["--cameras", "CAMS", "--temporal=0"], "--temporal=0"), (["--cameras", "CAMS", "--temporal=abc"], "--temporal=abc"),
    (["--cameras", "CAMS", "--temporalx"], "--temporalx"),
    (["--cameras", "CAMS", "--temporal", "--gpus", "2"], "--gpus"),
    (["--cameras", "CAMS", "--temporal", "--devices", "0,1"], "--devices"),
    (["--cameras", "CAMS", "--temporal", "--layers", "3"], "--layers"),
    (["--cameras", "CAMS", "--temporal", "--light-groups"], "--light-groups"),
    (["--cameras", "CAMS", "--temporal", "--strategies"], "--strategies"),
    (["--cameras", "CAMS", "--temporal", "--light-groups", "--layers", "2", "--cross"], "--l"),
    (["--cameras", "CAMS", "--temporal", "--batches", "4"], "--batches"),
    (["--cameras", "CAMS", "--temporal=16", "--adaptive", "0.1"], "--adaptive"),
    (["--cameras", "CAMS", "--temporal", "--sample-window", "0:1:4"], "--sample-window"),
    (["--cameras", "CAMS", "--temporal", "--aov"], "--aov"),
])
def test_command_line_refuses_temporal_misuse_before_any_device(args, word, tmp_path):
    import variants

    d = tmp_path / "run"
    d.mkdir()
    toml = d / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", 16, 16, 16))
    cams = tmp_path / "cams.txt"
    cams.write_text(GOOD_CAMERAS)
    args = [str(cams) if a == "CAMS" else a for a in args]
    r = subprocess.run([CLI, str(toml)] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--temporal" in r.stderr and word in r.stderr, r.stderr
    assert sorted(os.listdir(d)) == ["scene.toml"]


def test_command_line_refuses_temporal_for_a_path_scene(tmp_path):
    import variants

    d = tmp_path / "run"
    d.mkdir()
    toml = d / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", 16, 16, 1, kind="path"))
    cams = tmp_path / "cams.txt"
    cams.write_text(GOOD_CAMERAS)
    r = subprocess.run([CLI, str(toml), "--cameras", str(cams), "--temporal"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--temporal" in r.stderr and "path" in r.stderr, r.stderr
    assert sorted(os.listdir(d)) == ["scene.toml"]
