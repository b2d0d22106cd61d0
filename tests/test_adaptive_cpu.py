"""Adaptive sampling, the parts that need no GPU: the numpy restatements
adaptive_resolve_numpy and adaptive_select_numpy against what they must mean, the new structs' layout
against the compiler, and the refusals the driver and its state entries make before they look at a
device (a null context is only refused after them)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pairs(rng, K, H, W):
    """Random plane pairs (K, 2, H, W, 3): [b, 0] the splats T_b, [b, 1] the eye part E_b."""
    return rng.random((K, 2, H, W, 3), dtype=np.float32) * f32(3)


@pytest.mark.parametrize("K,spp", [(2, 8), (3, 12), (8, 64)])
def test_resolve_numpy_with_uniform_m_is_batch_moments_of_e_plus_t(K, spp):
    rng = np.random.default_rng(K)
    H, W = 5, 7
    pl = pairs(rng, K, H, W)
    m = np.full((H, W), spp // K, np.int32)
    assert bdpt_amd.adaptive_splat_scale(spp, H * W, K, int(m.sum())) == f32(1)
    S, v = bdpt_amd.adaptive_resolve_numpy(pl, m, spp)
    rs, rv = bdpt_amd.batch_moments_numpy(pl[:, 1] + pl[:, 0])
    assert S.dtype == np.float32 and v.dtype == np.float32
    assert np.array_equal(bits(S), bits(rs)) and np.array_equal(bits(v), bits(rv))


def test_resolve_numpy_scales_eye_by_own_samples_and_splats_by_all_light_paths():
    """E accumulates Li / spp over a pixel's own samples, T every light path's splat / spp: with K m[p] of spp
    samples done the eye mean is E spp / (K m[p]) per batch share, and with K M of spp W H light paths traced
    the splat image is T spp W H / (K M). m == 0 leaves only the splats."""
    K, H, W, spp = 4, 3, 4, 32
    rng = np.random.default_rng(7)
    pl = pairs(rng, K, H, W).astype(np.float64)
    m = rng.integers(0, spp // K + 1, (H, W)).astype(np.int32)
    m[0, 0], m[1, 1] = 0, spp // K
    S, v = bdpt_amd.adaptive_resolve_numpy(pl, m, spp, np.float64)
    t = spp * H * W / (K * m.sum())
    a = np.where(m > 0, spp / np.maximum(K * m, 1), 0.0)[..., None]
    planes = pl[:, 1] * a + pl[:, 0] * t
    assert np.allclose(S, planes.sum(0), rtol=1e-12)
    # (c = K / (K - 1) is a float32 quotient in every dt, as batch_moments_numpy's: 2^-24 relative)
    assert np.allclose(v, planes.var(0, ddof=1) * K, rtol=2e-7)
    assert np.allclose(S[0, 0], (pl[:, 0, 0, 0] * t).sum(0), rtol=1e-12)
    # nothing traced at all: both scales are 0
    S0, v0 = bdpt_amd.adaptive_resolve_numpy(pl, np.zeros((H, W), np.int32), spp)
    assert not S0.any() and not v0.any()
    with pytest.raises(ValueError, match="n_batches"):
        bdpt_amd.adaptive_resolve_numpy(pl[:1], m, spp)
    with pytest.raises(ValueError, match="planes"):
        bdpt_amd.adaptive_resolve_numpy(pl[:, 0], m, spp)


def hand_made(H, W, noisy_at, s=1.0, eps=0.0, thr=0.5):
    """S = s / 3 per channel everywhere; var just above the threshold's at noisy_at, just below elsewhere."""
    S = np.full((H, W, 3), f32(s) / f32(3), np.float32)
    ssum = ((S[0, 0, 0] + S[0, 0, 1]) + S[0, 0, 2]) + f32(eps)
    rhs = (f32(thr) * f32(thr)) * (ssum * ssum)
    var = np.zeros((H, W, 3), np.float32)
    var[..., 1] = np.nextafter(rhs, f32(0))
    for y, x in noisy_at:
        var[y, x, 1] = np.nextafter(rhs, f32(np.inf))
    return S, var, rhs


def test_select_numpy_rule_is_strict_and_in_the_headers_order():
    H, W = 4, 6
    S, var, rhs = hand_made(H, W, [(1, 2), (3, 5)], s=0.75, eps=0.25, thr=0.5)
    assert rhs == f32(0.25) * f32(1.0)
    m = np.zeros((H, W), np.int32)
    lst, m2 = bdpt_amd.adaptive_select_numpy(S, var, m, 0.5, 0.25, 2, 8, dilate=False)
    assert lst.dtype == np.int32 and list(lst) == [1 * W + 2, 3 * W + 5]
    var[0, 0] = (0, rhs, 0)  # exactly at the threshold: not noisy (strict >)
    lst, _ = bdpt_amd.adaptive_select_numpy(S, var, m, 0.5, 0.25, 2, 8, dilate=False)
    assert list(lst) == [1 * W + 2, 3 * W + 5]
    # m is updated at the listed pixels and nowhere else
    want = np.zeros((H, W), np.int32)
    want.reshape(-1)[lst] = 2
    assert np.array_equal(m2, want) and not m.any()
    # the channel sums are float32 sums in the stated order: a case where another order differs
    S1 = np.array([[[1e8, 1.0, -1e8]]], np.float32)
    v1 = np.array([[[0.5, 0.0, 0.0]]], np.float32)
    assert ((S1[0, 0, 0] + S1[0, 0, 1]) + S1[0, 0, 2]) == 0 and (S1[0, 0, 0] + S1[0, 0, 2]) + S1[0, 0, 1] == 1
    assert list(bdpt_amd.adaptive_select_numpy(S1, v1, [[0]], 1.0, 0.0, 1, 1, False)[0]) == [0]  # 0.5 > 1 * (0 * 0)
    # threshold 0: anything with variance is noisy, nothing without
    lst, _ = bdpt_amd.adaptive_select_numpy(S, np.zeros_like(var), m, 0.0, 1e-3, 1, 8, True)
    assert lst.size == 0
    nan = np.full_like(var, np.nan)
    assert bdpt_amd.adaptive_select_numpy(S, nan, m, 0.5, 0.0, 1, 8, True)[0].size == 0  # NaN compares false


def test_select_numpy_output_ascends_and_dilation_clips_at_the_border():
    H, W = 5, 6
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    S, var, _ = hand_made(H, W, corners)
    m = np.zeros((H, W), np.int32)
    lst, m2 = bdpt_amd.adaptive_select_numpy(S, var, m, 0.5, 0.0, 1, 4, dilate=True)
    want = set()
    for y, x in corners:
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= y + dy < H and 0 <= x + dx < W:  # no wrap-around to the other edge
                    want.add((y + dy) * W + x + dx)
    assert len(want) == 16 and list(lst) == sorted(want)
    assert np.all(np.diff(lst) > 0)
    assert m2.sum() == 16 and set(np.flatnonzero(m2.reshape(-1))) == want
    # an edge pixel in the middle of a row: its row neighbours, not the far end of the previous row
    S, var, _ = hand_made(H, W, [(2, 0)])
    lst, _ = bdpt_amd.adaptive_select_numpy(S, var, m, 0.5, 0.0, 1, 4, dilate=True)
    assert list(lst) == [1 * W, 1 * W + 1, 2 * W, 2 * W + 1, 3 * W, 3 * W + 1]
    # 1 x W and H x 1 images
    S, var, _ = hand_made(1, 7, [(0, 3)])
    assert list(bdpt_amd.adaptive_select_numpy(S, var, np.zeros((1, 7), np.int32), 0.5, 0.0, 1, 4, True)[0]) == [2, 3, 4]
    S, var, _ = hand_made(7, 1, [(6, 0)])
    assert list(bdpt_amd.adaptive_select_numpy(S, var, np.zeros((7, 1), np.int32), 0.5, 0.0, 1, 4, True)[0]) == [5, 6]


def test_select_numpy_budget_exhaustion():
    H, W = 3, 4
    S, var, _ = hand_made(H, W, [(y, x) for y in range(H) for x in range(W)])
    m = np.arange(H * W, dtype=np.int32).reshape(H, W)  # 0 .. 11
    lst, m2 = bdpt_amd.adaptive_select_numpy(S, var, m, 0.5, 0.0, 3, 8, dilate=True)
    assert list(lst) == [0, 1, 2, 3, 4, 5]  # m + 3 <= 8
    assert np.array_equal(m2.reshape(-1), np.where(np.arange(12) <= 5, np.arange(12) + 3, np.arange(12)))
    lst, m3 = bdpt_amd.adaptive_select_numpy(S, var, np.full((H, W), 8, np.int32), 0.5, 0.0, 1, 8, dilate=False)
    assert lst.size == 0 and np.all(m3 == 8)  # every pixel at the budget


def test_adaptive_windows_follow_the_pass():
    W = bdpt_amd.SampleWindow
    assert bdpt_amd.adaptive_windows(4, 1, 0) == [W(0, 4, 1), W(1, 4, 1), W(2, 4, 1), W(3, 4, 1)]
    assert bdpt_amd.adaptive_windows(2, 3, 2) == [W(12, 2, 3), W(13, 2, 3)]
    # every pass of a run in which all pixels stay active: the plain frame's samples, once each
    K, c, passes = 4, 2, 3
    ks = sorted(k for j in range(passes) for w in bdpt_amd.adaptive_windows(K, c, j) for k in w.samples())
    assert ks == list(range(K * c * passes))


STRUCTS = [("bdpt_adaptive_params", bdpt_amd._AdaptiveParams), ("bdpt_adaptive_stats", bdpt_amd._AdaptiveStats)]


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("abi_adaptive")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bdpt_amd.h"', "int main(void) {"]
    lines.append('    printf("max_passes value %d\\n", BDPT_ADAPTIVE_MAX_PASSES);')
    for cname, mirror in STRUCTS:
        lines.append(f'    printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'    printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["    return 0;", "}"]
    src = d / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out.splitlines()}


@pytest.mark.parametrize("cname,mirror", STRUCTS, ids=[c for c, _ in STRUCTS])
def test_adaptive_structs_match_the_header(c_layout, cname, mirror):
    assert ctypes.sizeof(mirror) == c_layout[(cname, "size")], cname
    for fname, _ in mirror._fields_:
        assert getattr(mirror, fname).offset == c_layout[(cname, fname)], (cname, fname)
    assert bdpt_amd.ADAPTIVE_MAX_PASSES == c_layout[("max_passes", "value")]


def frame_params(spp=16, W=8, H=8):
    p = bdpt_amd._FrameParams()
    p.camera = bdpt_amd.Camera().c()
    p.width, p.height, p.spp, p.rr_depth = W, H, spp, 5
    p.row_offset, p.row_stride = 0, 1
    return p


def adaptive_params(**kw):
    a = bdpt_amd._AdaptiveParams()
    a.n_batches, a.step, a.max_passes, a.threshold, a.eps, a.dilate, a.record_passes = 4, 1, 4, 0.1, 1e-3, 1, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("spp,kw,word", [
    (16, dict(n_batches=1), "n_batches"), (16, dict(n_batches=65), "n_batches"), (16, dict(step=0), "step"),
    (16, dict(max_passes=0), "max_passes"), (16 * 65, dict(max_passes=65, n_batches=16), "max_passes"),
    (15, {}, "spp must equal max_passes * step * n_batches"), (32, {}, "spp must equal"),
    (16, dict(threshold=-0.1), "threshold"), (16, dict(threshold=float("nan")), "threshold"),
    (16, dict(eps=float("inf")), "eps"), (16, dict(dilate=2), "dilate"),
])
def test_driver_refuses_bad_parameters_before_it_needs_a_device(spp, kw, word):
    L = bdpt_amd.lib()
    p, a = frame_params(spp), adaptive_params(**kw)
    buf = np.zeros(8 * 8 * 3, np.float32)
    smp = np.zeros(8 * 8, np.int32)
    for rc in (L.bdpt_render_adaptive_host(None, ctypes.byref(p), ctypes.byref(a), buf.ctypes.data, buf.ctypes.data,
                                           smp.ctypes.data, None),
               L.bdpt_render_adaptive(None, ctypes.byref(p), ctypes.byref(a), buf.ctypes.data, buf.ctypes.data,
                                      smp.ctypes.data, None, None)):
        assert rc == bdpt_amd.ERR_INVALID
        msg = L.bdpt_last_error().decode()
        assert "bdpt_render_adaptive" in msg and word in msg, msg


def test_state_entries_refuse_bad_arguments_and_a_null_context_last():
    L = bdpt_amd.lib()
    one = np.zeros(64, np.float32)
    i1 = np.zeros(8, np.int32)
    p, a = frame_params(), adaptive_params()
    # valid parameters: only the context is missing
    assert L.bdpt_render_adaptive_host(None, ctypes.byref(p), ctypes.byref(a), one.ctypes.data, one.ctypes.data,
                                       i1.ctypes.data, None) == bdpt_amd.ERR_INVALID
    assert "null" in L.bdpt_last_error().decode()
    assert L.bdpt_render_adaptive_host(None, ctypes.byref(p), None, one.ctypes.data, one.ctypes.data, i1.ctypes.data,
                                       None) == bdpt_amd.ERR_INVALID
    res = lambda *args: L.bdpt_adaptive_resolve_host(None, *args)  # noqa: E731
    ok = (1, 1, 2, 4, one.ctypes.data, i1.ctypes.data, -1, one.ctypes.data, one.ctypes.data)
    for k, bad, word in ((2, 1, "n_batches"), (2, 65, "n_batches"), (3, 0, "spp"), (0, 0, "width"), (4, None, "planes"),
                         (5, None, "samples_per_batch"), (8, None, "out_var")):
        args = list(ok)
        args[k] = bad
        assert res(*args) == bdpt_amd.ERR_INVALID
        assert word in L.bdpt_last_error().decode(), (k, L.bdpt_last_error())
    assert res(*ok) == bdpt_amd.ERR_INVALID and "null ctx" in L.bdpt_last_error().decode()
    n = ctypes.c_int32(0)
    sel = lambda *args: L.bdpt_adaptive_select_host(None, *args)  # noqa: E731
    ok = [1, 1, one.ctypes.data, one.ctypes.data, 0.1, 1e-3, 1, 4, 1, i1.ctypes.data, i1.ctypes.data, ctypes.byref(n)]
    for k, bad, word in ((4, -1.0, "threshold"), (5, float("nan"), "eps"), (6, 0, "step"), (7, -1, "m_max"),
                         (8, 2, "dilate"), (2, None, "sum"), (9, None, "samples_per_batch"), (10, None, "out_list")):
        args = list(ok)
        args[k] = bad
        assert sel(*args) == bdpt_amd.ERR_INVALID
        assert word in L.bdpt_last_error().decode(), (k, L.bdpt_last_error())
    assert sel(*ok) == bdpt_amd.ERR_INVALID and "null ctx" in L.bdpt_last_error().decode()
    assert L.bdpt_render_pixels(None, ctypes.byref(p), None, None, -1, one.ctypes.data, None) == bdpt_amd.ERR_INVALID
    assert "n_pixels" in L.bdpt_last_error().decode()


@pytest.mark.parametrize("args,word", [
    (["--adaptive", "0.1", "--gpus", "2"], "--gpus"), (["--adaptive", "0.1", "--layers", "3"], "--layers"),
    (["--adaptive", "0.1", "--light-groups"], "--light-groups"), (["--adaptive", "0.1", "--strategies"], "--strategies"),
    (["--adaptive", "0.1", "--batches", "4"], "--batches"), (["--adaptive", "x"], "THR"),
    (["--adaptive", "0.1:1"], "K in [2, 64]"), (["--adaptive", "-1"], "THR"), (["--adaptive", "0.1:4:1:99"], "PASSES"),
    (["--adaptive", "0.1:8:3"], "spp (16) must be PASSES * STEP * K"), (["--adaptive", "0.1:4", "--spp", "18"], "spp (18)"),
    (["--adaptive", "0.1", "--sample-window", "0:1:4"], "--sample-window"),
])
def test_command_line_refuses_adaptive_misuse_before_any_device(args, word, tmp_path):
    import variants

    toml = tmp_path / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", 16, 16, 16))
    r = subprocess.run([CLI, str(toml)] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--adaptive" in r.stderr and word in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["scene.toml"]
