"""The connection-BSDF entry points and the fast-weight math codes, the parts that need no
GPU: the library's symbols, argument validation, the population of the kat_bsdf_edges
fixture's classes, and the float32 numpy restatement of make_frame / to_local that
tests/test_gpu_kat_connection.py holds local_for to, verified here against the reference's
own Frame::toLocal (the wo column of the kat_intersect fixtures)."""
import ctypes
import os

import numpy as np
import pytest

import bdpt_amd

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32


def np_make_frame(n):
    """Frame(n) with coordinateSystem (core.h:155-157, math.h:42-51) in float32, one rounding
    per operation: t = c, s = cross(c, n)."""
    n = np.asarray(n, f32)
    ax, ay, az = n[:, 0], n[:, 1], n[:, 2]
    use_x = np.abs(ax) > np.abs(ay)
    zero = np.zeros_like(ax)
    with np.errstate(divide="ignore", invalid="ignore"):  # (the branch not taken may divide by 0)
        inv_x = f32(1) / np.sqrt(ax * ax + az * az)
        inv_y = f32(1) / np.sqrt(ay * ay + az * az)
        t = np.where(use_x[:, None], np.stack([az * inv_x, zero, -ax * inv_x], 1),
                     np.stack([zero, az * inv_y, -ay * inv_y], 1)).astype(f32)
    s = np.stack([t[:, 1] * az - ay * t[:, 2], t[:, 2] * ax - az * t[:, 0], t[:, 0] * ay - ax * t[:, 1]], 1)
    return s.astype(f32), t


def np_dot(a, b):
    """glm's dot: (x x' + y y') + z z' in float32."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(f32)


def np_to_local(n, v):
    """Frame(n).toLocal(v) = (dot(v, s), dot(v, t), dot(v, n)) in float32."""
    s, t = np_make_frame(n)
    return np.stack([np_dot(v, s), np_dot(v, t), np_dot(v, n)], 1)


def bits_equal(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or np.array_equal(a, b)


@pytest.mark.parametrize("scene", ["caustic", "hardlight", "cbox_low"])
def test_numpy_frame_restatement_matches_reference_wo(scene):
    """SurfaceInteraction::wo = frameNs.toLocal(-ray.d) of the reference's own hits (accel.h:160),
    bit for bit, over flat walls (axis-aligned normals: both branches of coordinateSystem) and
    the curved meshes' interpolated normals."""
    g = np.load(os.path.join(GOLD, f"kat_intersect_{scene}.npz"))
    out, rays = g["out"], g["rays"]
    hit = out[:, 0] == 1
    n, wo, d = out[hit, 10:13], out[hit, 16:19], rays[hit, 3:6]
    assert hit.sum() > 1000
    use_x = np.abs(n[:, 0]) > np.abs(n[:, 1])
    assert use_x.sum() > 50 and (~use_x).sum() > 50
    assert bits_equal(np_to_local(n, -d), wo)


def test_library_exports_the_connection_entries():
    L = bdpt_amd.lib()
    for s in ("bdpt_bsdf_eval_pdfs", "bdpt_bsdf_local_for", "bdpt_debug_math"):
        assert hasattr(L, s), s
    with open(os.path.join(os.path.dirname(GOLD), "..", "include", "bdpt_amd.h")) as f:
        header = f.read()
    for k, v in bdpt_amd.KAT_BUILDS.items():
        assert f"#define BDPT_KAT_{'FAST' if k == 'fast' else k.upper()} {v}" in header
    for k, v in bdpt_amd.MATH_FNS.items():
        assert f"#define BDPT_MATH_{k.upper()} {v}\n" in header
    assert sorted(bdpt_amd.MATH_FNS.values()) == list(range(10))


def test_c_entries_refuse_bad_arguments_before_touching_a_device():
    L = bdpt_amd.lib()
    x = np.ones(4, f32)
    out = np.zeros(20, f32)
    m = np.zeros(4, np.int32)
    # no context
    assert L.bdpt_bsdf_eval_pdfs(None, 0, 4, m.ctypes.data, x.ctypes.data, x.ctypes.data,
                                 out.ctypes.data) == bdpt_amd.ERR_INVALID
    assert L.bdpt_bsdf_local_for(None, 0, 4, m.ctypes.data, x.ctypes.data, x.ctypes.data,
                                 out.ctypes.data) == bdpt_amd.ERR_INVALID
    # unknown fn code; a two-argument fn without y; null x
    for fn, xx, yy in ((10, x.ctypes.data, x.ctypes.data), (-1, x.ctypes.data, x.ctypes.data),
                       (5, x.ctypes.data, None), (7, x.ctypes.data, None), (2, x.ctypes.data, None),
                       (6, None, None)):
        assert L.bdpt_debug_math(0, fn, xx, yy, out.ctypes.data, 4) == bdpt_amd.ERR_INVALID, fn
    assert b"bad argument" in L.bdpt_last_error()


def test_python_wrappers_validate_before_the_call():
    with pytest.raises(KeyError):
        bdpt_amd.debug_math("cbrt_w", np.ones(3, f32))
    for fn in ("pow_w", "div_w", "powf"):
        with pytest.raises(ValueError):
            bdpt_amd.debug_math(fn, np.ones(3, f32))
        with pytest.raises(ValueError):
            bdpt_amd.debug_math(fn, np.ones(3, f32), np.ones(2, f32))

    it = object.__new__(bdpt_amd.BDPTIntegrator)  # no context: the C side must refuse it
    it._h = None
    one = np.array([[0, 0, 1]], f32)
    with pytest.raises(KeyError):
        it.bsdf_eval_pdfs([0], one, one, build="ieee")
    with pytest.raises(ValueError):
        it.bsdf_eval_pdfs([0, 0], one, one)
    with pytest.raises(ValueError):
        it.bsdf_local_for([0], one, np.zeros((2, 3), f32), build="fast")
    with pytest.raises(bdpt_amd.BdptError) as e:
        it.bsdf_eval_pdfs([0], one, one, build="ng")
    assert e.value.code == bdpt_amd.ERR_INVALID


def test_edges_fixture_populates_its_classes():
    """What make_kat_goldens.py asserted when it wrote the fixture, on the committed file: per
    material that evaluates a Phong power, >= 100 records with the float32 lobe cosine above 1,
    >= 100 on 1, >= 200 with an unflushed power at ex |log2 z| in [60, 126] and >= 100 with a
    power below 2^-126, wherever a float32 z can reach that class at the material's exponent
    (x^0 is 1 for every x; at the largest finite Ns the float below 1 is already at 2.9e31)."""
    g = np.load(os.path.join(GOLD, "kat_bsdf_edges.npz"))
    names, ns = list(g["names"]), g["ns"]
    assert ns.max() == np.finfo(f32).max and names[int(ns.argmax())] == "phongNsMax"
    step = -np.log2(np.float64(np.nextafter(f32(1), f32(0))))
    for name in ("phongNs0", "phongNs1", "phongNs100", "phongNs1000", "phongNsMax", "mixSpecw0", "mixSpecw1",
                 "mixOrdinary"):
        m = names.index(name)
        k = g["mat"] == m
        assert k.sum() == 2000
        wo, wi, ex = g["wo"][k], g["wi"][k], float(ns[m])
        z = np_dot(wi, wo * np.array([-1, -1, 1], f32))
        z64 = z.astype(np.float64)
        with np.errstate(divide="ignore"):
            t = np.where(z64 > 0, ex * np.abs(np.log2(np.where(z64 > 0, z64, 1.0))), np.inf)
        below = (z64 >= 0) & (z64 < 1)
        assert (z > 1).sum() >= 100 and (z == 1).sum() >= 100, name
        if 0 < ex * step <= 126:
            assert (below & (t >= 60) & (t <= 126)).sum() >= 200, name
        if ex > 0:
            assert (below & (t > 126)).sum() >= 100, name
        assert np.bincount(g["cls"][k], minlength=8).min() >= (0 if ex == 0 or ex * step > 126 else 100), name
