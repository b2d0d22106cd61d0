"""Crossed planes (bdpt_render_group_layers, bdpt_render_group_strategies, bdpt_group_planes_combine;
DESIGN.md §7g): one BDPT frame split by emitter AND by path length or sampling strategy, a plane per
(group, layer) or (group, s, t), and recombined with per-group RGB gains and per-inner-plane weights.

The joint planes must have the single-kind renders as their marginals, be right in absolute terms
(the reference's frame of emit_edges with each emitter's Ke scaled, tests/golden/
light_groups_emit_edges_relit.npz: a contribution under a wrong group gets a wrong gain, one under a
wrong strategy a wrong weight), carry group and depth together through a stored light vertex's tag,
commute with row shards and sample windows, survive the ring-full fallback, combine as the
sequential float32 loop bit for bit, and refuse what the builds do not serve before any launch.

Frames are at most 64 x 64 x 16 spp; the bound everywhere is the project's frame bound TOL
(per-pixel relative L2 <= 1e-4). A crossed render is made once per (case, arguments) and shared."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import REPO, gpu_available, load_golden
from plane_cases import (CBOX_CASE, EDGES_CASE, FRAMES, RING_CASE, STRATEGY, bound_of, golden_integrator, open_integrator,
                         plane_sum, unsupported_setups, worst_per_plane)
from test_config_exr import decode_exr
from test_gpu_layers import layers_of
from test_gpu_light_groups import RELIT, edges_gains, emitter_count, groups_of, relight_model
from test_gpu_parity import TOL, rel_l2
from test_gpu_strategies import clamp_to, planes_of, shape_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

GL_KERNEL = "bdpt_frame_kernel_groups_layers"
GS_KERNEL = {False: "bdpt_frame_kernel_groups_strat", True: "bdpt_frame_kernel_groups_strat_unweighted"}
I, U = bdpt_amd.ERR_INVALID, bdpt_amd.ERR_UNSUPPORTED

_crossed = {}


def _checked(name, it, out, kernel, shape):
    st = it.stats()
    assert st["kernel"] == kernel, st["kernel"]
    assert st["schedule_errors"] == 0 and st["samples"] == FRAMES[name]["samples"]
    assert out.shape == shape + (FRAMES[name]["height"], FRAMES[name]["width"], 3) and out.dtype == np.float32
    assert np.isfinite(out).all()
    out.setflags(write=False)
    return out


def group_layers_of(name, n_layers, group_map=None, n_groups=None, **kw):
    """The (group, layer) render of a golden's frame, made once (read-only)."""
    key = ("gl", name, n_layers, None if group_map is None else tuple(group_map), n_groups, tuple(sorted(kw.items())))
    if key not in _crossed:
        it = golden_integrator(name, **kw)
        out = it.render_group_layers(n_layers, group_map, n_groups)
        n = n_groups if n_groups is not None else (emitter_count(name) if group_map is None else max(group_map) + 1)
        _crossed[key] = _checked(name, it, out, GL_KERNEL, (n, n_layers))
    return _crossed[key]


def group_strategies_of(name, shape=None, unweighted=False):
    """The (group, s, t) render of a golden's frame under the identity map, made once (read-only)."""
    shape = shape or shape_of(name)
    key = ("gs", name, shape, unweighted)
    if key not in _crossed:
        it = golden_integrator(name)
        out = it.render_group_strategies(shape[0], shape[1], unweighted=unweighted)
        _crossed[key] = _checked(name, it, out, GS_KERNEL[unweighted], (emitter_count(name),) + tuple(shape))
    return _crossed[key]


def over(planes, axes):
    return planes.astype(np.float64).sum(axis=axes)


# ------------------------------------------------------------------------- 1. marginals
@pytest.mark.parametrize("clamped", [False, True], ids=["full", "clamped"])
@pytest.mark.parametrize("name", [EDGES_CASE, RING_CASE])
def test_gpu_group_layers_have_both_renders_as_marginals(name, clamped):
    """Summed over the layers the joint planes are the light groups, summed over the groups the
    layers, summed over both the golden. n = 2 clamps every longer path into the last layer."""
    n = 2 if clamped else bound_of(name)
    gl = group_layers_of(name, n)
    by_group = worst_per_plane(over(gl, 1), groups_of(name))
    by_layer = worst_per_plane(over(gl, 0), layers_of(name, n))
    total = rel_l2(plane_sum(gl), load_golden(name)).max()
    print(f"{name} {gl.shape[:2]}: sum over layers vs light groups {by_group:.3g}, over groups vs layers {by_layer:.3g}, "
          f"over both vs the golden {total:.3g}")
    assert by_group <= TOL and by_layer <= TOL and total <= TOL


@pytest.mark.parametrize("shape", [None, (2, 2)], ids=["full", "clamped"])
@pytest.mark.parametrize("name", [EDGES_CASE, RING_CASE])
def test_gpu_group_strategies_have_both_renders_as_marginals(name, shape):
    gs = group_strategies_of(name, shape)
    by_group = worst_per_plane(over(gs, (1, 2)), groups_of(name))
    by_strategy = worst_per_plane(over(gs, 0), planes_of(name, shape))
    total = rel_l2(plane_sum(gs), load_golden(name)).max()
    print(f"{name} {gs.shape[:3]}: sum over (s, t) vs light groups {by_group:.3g}, over groups vs strategies "
          f"{by_strategy:.3g}, over all vs the golden {total:.3g}")
    assert by_group <= TOL and by_strategy <= TOL and total <= TOL
    assert not gs[:, 0, 0].any()  # (0, 1) is structurally empty in every group
    if shape is not None:  # and the clamped planes are the clamped sums of each group's full planes
        full = group_strategies_of(name)
        want = np.stack([clamp_to(full[g], *shape) for g in range(full.shape[0])])
        assert worst_per_plane(gs, want) <= TOL


@pytest.mark.parametrize("name", [EDGES_CASE, RING_CASE])
def test_gpu_group_strategies_folded_by_length_are_the_group_layers(name):
    gs = group_strategies_of(name)
    n = bound_of(name)
    gl = group_layers_of(name, n)
    n_s, n_t = gs.shape[1:3]
    folded = np.zeros(gl.shape, np.float64)
    for s in range(n_s):
        for t in range(1, n_t + 1):
            k = s + t - 1
            if gs[:, s, t - 1].any():
                assert 1 <= k <= n, (s, t)  # nothing is longer than the bound
                folded[:, k - 1] += gs[:, s, t - 1]
    worst = worst_per_plane(folded, gl)
    print(f"{name}: (g, s, t) planes folded by k = s + t - 1 against the (g, layer) planes: {worst:.3g}")
    assert worst <= TOL


# ------------------------------------------------------- 2. absolute, against the reference
@pytest.mark.parametrize("strategy", ["bdpt", "lt", "pt"])
def test_gpu_relit_group_layers_are_the_reference_frame_of_the_rescaled_scene(strategy):
    n = bound_of(EDGES_CASE)
    planes = group_layers_of(EDGES_CASE, n, strategy=STRATEGY[strategy])
    it = golden_integrator(EDGES_CASE)
    relit = it.combine_group_planes(planes, gains=edges_gains())
    ref = RELIT[strategy]
    worst, plain = rel_l2(relit, ref).max(), rel_l2(plane_sum(planes), ref).max()
    print(f"{strategy}: (group, layer) planes under the emitters' gains vs the rescaled scene's reference frame "
          f"{worst:.3g} (the unscaled sum: {plain:.3g})")
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"
    assert plain > 0.1


def test_gpu_group_and_strategy_are_filed_jointly():
    """The unweighted (g, s, t) planes of the BDPT frame, weight 1 on every t = 1 plane and on (0, 2),
    0 elsewhere, each group under its emitter's gain: the reference's LIGHT_TRACING frame of the
    rescaled scene (tests/test_gpu_strategies.py's identity on G9 / G11, here with the gains). A
    contribution under a wrong group gets a wrong gain, one under a wrong strategy a wrong weight."""
    planes = group_strategies_of(EDGES_CASE, unweighted=True)
    n_s, n_t = planes.shape[1:3]
    weights = np.zeros((n_s, n_t), np.float32)
    weights[:, 0] = 1.0
    weights[0, 1] = 1.0
    it = golden_integrator(EDGES_CASE)
    got = it.combine_group_planes(planes, gains=edges_gains(), weights=weights)
    worst = rel_l2(got, RELIT["lt"]).max()
    no_gains = rel_l2(it.combine_group_planes(planes, weights=weights), RELIT["lt"]).max()
    no_weights = rel_l2(it.combine_group_planes(planes, gains=edges_gains()), RELIT["lt"]).max()
    print(f"unweighted (g, s, t) planes, t = 1 and (0, 2), under the gains vs the relit light tracer: {worst:.3g} "
          f"(without the gains {no_gains:.3g}, without the weights {no_weights:.3g})")
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"
    assert no_gains > 0.1 and no_weights > 0.1  # either half alone misses


# ------------------------------------------------------------------- 3. the tag packing
def test_gpu_group_maps_merge_crossed_planes():
    n = bound_of(EDGES_CASE)
    ident = group_layers_of(EDGES_CASE, n)
    two = group_layers_of(EDGES_CASE, n, [0, 0, 1, 1, 1], 2)
    w0 = worst_per_plane(two[0], over(ident[:2], 0))
    w1 = worst_per_plane(two[1], over(ident[2:], 0))
    print(f"map [0, 0, 1, 1, 1]: group 0 vs identity groups 0 + 1 {w0:.3g}, group 1 vs 2 + 3 + 4 {w1:.3g}")
    assert w0 <= TOL and w1 <= TOL
    eight = group_layers_of(EDGES_CASE, n, [0, 1, 2, 3, 4], 8)
    assert eight.shape[:2] == (8, n)
    assert not eight[5:].any(), "a plane no emitter maps to holds energy"
    assert worst_per_plane(eight[:5], ident) <= TOL


def test_gpu_every_plane_the_marginals_fill_holds_energy():
    """Per group some layer holds energy and per layer some group, wherever the single-kind render's
    plane does; the direct-light layer (two edges: what connectToLight and the eye walk's second
    hit form) holds energy for every one of the five emitters."""
    n = bound_of(EDGES_CASE)
    gl = group_layers_of(EDGES_CASE, n)
    lit = gl.reshape(5, n, -1).any(axis=2)
    print("non-empty (group, layer) planes:\n" + "\n".join("".join("x" if v else "." for v in row) for row in lit))
    assert (lit.any(axis=1) == groups_of(EDGES_CASE).reshape(5, -1).any(axis=1)).all() and lit.any(axis=1).all()
    assert (lit.any(axis=0) == layers_of(EDGES_CASE, n).reshape(n, -1).any(axis=1)).all()
    assert lit[:, 1].all()
    for a in range(5):
        for b in range(a + 1, 5):
            assert not np.array_equal(gl[a], gl[b]), (a, b)


def test_gpu_open_scene_has_two_lengths_and_one_group():
    it = open_integrator(8)
    gl = it.render_group_layers(5)
    assert it.stats()["kernel"] == GL_KERNEL and gl.shape[:2] == (1, 5)
    assert gl[0, 0].any() and gl[0, 1].any()
    assert not gl[0, 2:].any(), "a path longer than two edges carries energy on the open scene"
    assert worst_per_plane(gl[0], open_integrator(8).render_layers(5)) <= TOL


# ------------------------------------------------------- 4. decompositions commute
def test_gpu_row_shards_sum_to_the_full_crossed_planes():
    n = bound_of(EDGES_CASE)
    parts = [golden_integrator(EDGES_CASE).render_group_layers(n, row_offset=o, row_stride=2) for o in (0, 1)]
    worst = worst_per_plane(parts[0] + parts[1], group_layers_of(EDGES_CASE, n))
    shape = shape_of(EDGES_CASE)
    sparts = [golden_integrator(EDGES_CASE).render_group_strategies(*shape, row_offset=o, row_stride=2) for o in (0, 1)]
    sworst = worst_per_plane(sparts[0] + sparts[1], group_strategies_of(EDGES_CASE))
    print(f"two interleaved row shards: (g, layer) {worst:.3g}, (g, s, t) {sworst:.3g}")
    assert worst <= TOL and sworst <= TOL


def test_gpu_sample_windows_sum_to_the_full_crossed_planes():
    """The even and the odd samples of 16 spp on one 64-pixel row of the five-emitter scene."""
    row = dict(row_offset=20, row_stride=64)
    kw = dict(width=64, height=64, spp=16)
    n = bound_of(EDGES_CASE)
    full = golden_integrator(EDGES_CASE, **kw).render_group_layers(n, **row)
    a = golden_integrator(EDGES_CASE, **kw).render_group_layers(n, window=bdpt_amd.SampleWindow(0, 2, 8), **row)
    b = golden_integrator(EDGES_CASE, **kw).render_group_layers(n, window=bdpt_amd.SampleWindow(1, 2, 8), **row)
    assert all(full[g, :, 20].any() for g in range(5))
    worst = worst_per_plane(a + b, full)
    print(f"sample windows 0:2:8 + 1:2:8 of 16: worst per-plane per-pixel rel L2 {worst:.3g}")
    assert worst <= TOL
    assert rel_l2(plane_sum(full), golden_integrator(EDGES_CASE, **kw).render_frame(**row)).max() <= TOL


# ------------------------------------------------- 5. the ring-full path keeps both indices
RING_SCRIPT = """
import json, sys
import numpy as np
import torch
import bdpt_amd, variants
name, W, H, spp, rr, n, out = json.loads(sys.argv[1])
cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES[name]["camera"]), width=W, height=H, spp=spp, rr_depth=rr)
it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(name)), cfg)
it.init()
planes = it.render_group_layers(n)
st = it.stats()
np.save(out, planes)
# a crossed render cannot count (flags are refused): the default build, whose schedule and ring this
# build shares, counts the same frame on the same context
it.render_frame(flags=bdpt_amd.FLAG_COUNT)
sched = it.stats()["sched"]
print("RING " + json.dumps({"kernel": st["kernel"], "schedule_errors": int(st["schedule_errors"]),
                           "samples": int(st["samples"]), "pushed": int(sched["step_tasks"]),
                           "refused": int(sched["shade_steps"])}))
"""


def test_gpu_ring_full_fallback_is_crossed(tmp_path):
    """BDPT_TASK_CAP=64 in a fresh process (the context reads it when it is created): pushes are
    refused and the owner traces those shadow rays itself; each such connection must still land in
    its (group, layer) plane (pend_px). One emitter here, so this pins the layer half of the index;
    the emit_edges cases pin the group half."""
    m = FRAMES[RING_CASE]
    n = bound_of(RING_CASE)
    out = str(tmp_path / "planes.npy")
    env = dict(os.environ, BDPT_TASK_CAP="64")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "bidirectional-path-tracing_amd"),
                                         os.path.join(REPO, "scenes")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    case = [m["scene"], m["width"], m["height"], m["spp"], m["rr_depth"], n, out]
    p = subprocess.run([sys.executable, "-c", RING_SCRIPT, json.dumps(case)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads([line for line in p.stdout.splitlines() if line.startswith("RING ")][-1][5:])
    planes = np.load(out)
    print(f"{RING_CASE} at BDPT_TASK_CAP=64: {got}")
    assert got["kernel"] == GL_KERNEL and got["schedule_errors"] == 0 and got["samples"] == m["samples"]
    assert got["refused"] > 0, "no push was refused: the ring-full fallback did not run"
    assert np.isfinite(planes).all()
    worst = rel_l2(plane_sum(planes), load_golden(RING_CASE)).max()
    per_plane = worst_per_plane(planes, group_layers_of(RING_CASE, n))
    print(f"plane sum vs golden {worst:.3g}, per plane vs the default ring {per_plane:.3g}")
    assert worst <= TOL and per_plane <= TOL


# ------------------------------------------------------------------- 6. the combine's bits
def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_gpu_combine_is_the_sequential_float32_loop():
    n = bound_of(EDGES_CASE)
    planes = group_layers_of(EDGES_CASE, n)
    assert planes.shape == (5, n, 32, 32, 3)
    it = golden_integrator(EDGES_CASE)
    model = bdpt_amd.combine_group_planes_numpy
    rng = np.random.default_rng(20261021)
    gains = rng.uniform(-2.0, 3.0, (5, 3)).astype(np.float32)
    gains[1] = 0.0  # a zero gain multiplies (its planes still enter the sum)
    gains[3, 0] = -0.75
    weights = rng.uniform(-1.5, 2.0, n).astype(np.float32)
    weights[0] = 0.0
    assert (gains < 0).any() and (weights < 0).any()
    got = it.combine_group_planes(planes, gains, weights)
    assert got.shape == (32, 32, 3) and same_bits(got, model(planes, gains, weights))
    assert same_bits(got, it.combine_group_planes(planes, gains, weights))  # two calls, the same bits
    assert same_bits(it.combine_group_planes(planes, gains), model(planes, gains))
    assert same_bits(it.combine_group_planes(planes, weights=weights), model(planes, None, weights))
    seq = None
    for g in range(5):
        for j in range(n):
            seq = planes[g, j].copy() if seq is None else seq + planes[g, j]  # float32 + float32, ascending
    assert same_bits(it.combine_group_planes(planes), seq)
    # the (g, s, t) layout with weights of the inner axes' shape
    gs = group_strategies_of(EDGES_CASE)
    w2 = rng.uniform(-1.0, 1.0, gs.shape[1:3]).astype(np.float32)
    assert same_bits(it.combine_group_planes(gs, gains, w2), model(gs, gains, w2))
    # a frame whose float count is no multiple of 12 (the dword-load kernel), and a 1 x 1 product
    odd = np.ascontiguousarray(planes[:3, :2, :5, :7])
    assert same_bits(it.combine_group_planes(odd, gains[:3], weights[:2]), model(odd, gains[:3], weights[:2]))
    one = np.ascontiguousarray(planes[2:3, 1:2])
    assert same_bits(it.combine_group_planes(one, gains[2:3], weights[1:2]),
                     gains[2][None, None, :] * (weights[1] * planes[2, 1]))
    # n_inner = 1 and null weights: relight's bits on the same planes
    groups = groups_of(EDGES_CASE)
    as_crossed = it.combine_group_planes(groups[:, None], gains)
    assert same_bits(as_crossed, it.relight(groups, gains)) and same_bits(as_crossed, relight_model(groups, gains))


# ------------------------------------------------------------------------ 7. refusals
PIXEL_FIELD = " * W * H must be below 2^30 (the shadow-ray task record's pixel field)"
NOT_BUILT = ["with Russian roulette", "with rr_depth > 28", "with flags (a counting pass or full traversal)",
             "for a scene with bitmap textures", "with the BSDF records in HBM (too many materials for the LDS table)"]
WEIGHTING = "weighting must be BDPT_STRATEGIES_WEIGHTED (0) or BDPT_STRATEGIES_UNWEIGHTED (1)"


def refused_as(call, code, text, launched):
    before = launched.stats()["launches"]
    with pytest.raises(bdpt_amd.BdptError) as e:
        call()
    assert (e.value.code, str(e.value)) == (code, f"bdpt error {code}: {text}")
    assert launched.stats()["launches"] == before, "a refused call launched"


@pytest.fixture(scope="module")
def device_planes():
    import torch

    buf = torch.zeros(64 * 32 * 32 * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return buf


def test_gpu_crossed_renders_refuse_what_no_plane_build_serves(monkeypatch, device_planes):
    fb = device_planes.data_ptr()
    for (bad, kw, _), text in zip(unsupported_setups(CBOX_CASE, monkeypatch), NOT_BUILT):
        bad.render_frame()  # (so that the context has stats of a call that launched)
        # the device wrappers take no flags: the host forms, which check before they stage anything
        refused_as(lambda: bad.render_group_layers(2, **kw), U, f"light groups x layers are not built {text}", bad)
        refused_as(lambda: bad.render_group_strategies(2, 2, **kw), U, f"light groups x strategies are not built {text}", bad)
    it = golden_integrator(EDGES_CASE)
    it.render_frame()
    gl, gs = "bdpt_render_group_layers: ", "bdpt_render_group_strategies: "
    five = [0, 1, 2, 3, 4]
    for n in (0, 65, -1):
        refused_as(lambda: it.render_group_layers_device(2, fb, [0] * 5, n), I, gl + "n_groups must be in [1, 64]", it)
        refused_as(lambda: it.render_group_layers_device(n, fb), I, gl + "n_layers must be in [1, 64]", it)
        refused_as(lambda: it.render_group_strategies_device(fb, 2, 2, False, [0] * 5, n), I, gs + "n_groups must be in [1, 64]", it)
    refused_as(lambda: it.render_group_layers_device(65, fb, [0] * 5, 65), I, gl + "n_groups must be in [1, 64]", it)
    for n_s, n_t, text in ((0, 2, "n_s must be in [1, 29]"), (30, 2, "n_s must be in [1, 29]"), (2, 0, "n_t must be in [1, 28]"),
                           (2, 29, "n_t must be in [1, 28]"), (30, 29, "n_s must be in [1, 29]")):
        refused_as(lambda: it.render_group_strategies_device(fb, n_s, n_t), I, gs + text, it)
    for weighting in (2, -1):
        refused_as(lambda: it.render_group_strategies_device(fb, 2, 2, weighting), I, gs + WEIGHTING, it)
    for n in (4, 6):
        null_map = f"a null group_of_emitter is the identity map and needs n_groups equal to the emitter count (5), got {n}"
        refused_as(lambda: it.render_group_layers_device(2, fb, None, n), I, gl + null_map, it)
        refused_as(lambda: it.render_group_strategies_device(fb, 2, 2, False, None, n), I, gs + null_map, it)
    refused_as(lambda: it.render_group_layers_device(2, fb, [0, 1, 2, 3, 5], 5), I,
               gl + "group_of_emitter[4] = 5 is outside [0, n_groups)", it)
    refused_as(lambda: it.render_group_strategies_device(fb, 2, 2, False, [0, -1, 2, 3, 4], 5), I,
               gs + "group_of_emitter[1] = -1 is outside [0, n_groups)", it)
    # n_groups * n_inner * W * H >= 2^30, in the params only: refused before anything is touched
    big = golden_integrator(EDGES_CASE)
    big.render_frame()
    big.config.width, big.config.height = 32768, 4096  # 2^27 pixels: 5 x 2 planes reach 2^30, 5 x 1 do not
    refused_as(lambda: big.render_group_layers_device(2, fb), I, gl + "n_groups * n_layers" + PIXEL_FIELD, big)
    refused_as(lambda: big.render_group_layers_device(2, fb, five, 8), I, gl + "n_groups * n_layers" + PIXEL_FIELD, big)
    refused_as(lambda: big.render_group_strategies_device(fb, 2, 1), I, gs + "n_groups * n_s * n_t" + PIXEL_FIELD, big)
    refused_as(lambda: big.render_group_layers(2), I, gl + "n_groups * n_layers" + PIXEL_FIELD, big)
    refused_as(lambda: big.render_group_strategies(2, 2, unweighted=True), I, gs + "n_groups * n_s * n_t" + PIXEL_FIELD, big)
    # the count before the size, the size before the map and before what is not built
    refused_as(lambda: big.render_group_layers_device(65, fb), I, gl + "n_layers must be in [1, 64]", big)
    refused_as(lambda: big.render_group_layers_device(2, fb, [0, 1, 2, 3, 9], 8), I, gl + "n_groups * n_layers" + PIXEL_FIELD, big)


def test_gpu_combine_refusals(device_planes):
    it = golden_integrator(EDGES_CASE)
    it.render_frame()
    d = device_planes.data_ptr()
    plane = 32 * 32 * 3
    out = d + 4 * 6 * plane  # behind 2 x 3 planes
    name = "bdpt_group_planes_combine: "
    ones = np.ones((2, 3), np.float32)

    def combine(n=2, n_inner=3, w=32, h=32, gains=ones, weights=None, planes=d, out=out):
        return lambda: it.combine_group_planes_device(planes, n, n_inner, w, h, gains, weights, out)

    shape = name + "width/height must be > 0 and n_groups * n_inner * W * H below 2^30"
    for n in (0, 65):
        refused_as(combine(n=n, gains=None), I, name + "n_groups must be in [1, 64]", it)
    for n_inner in (0, 813):
        refused_as(combine(n_inner=n_inner), I, name + "n_inner must be in [1, 812]", it)
    refused_as(combine(w=0), I, shape, it)
    refused_as(combine(h=-1), I, shape, it)
    refused_as(combine(n_inner=2, w=32768, h=8192), I, shape, it)
    for i, j, v in ((1, 2, np.nan), (0, 1, -np.inf)):
        g = ones.copy()
        g[i, j] = v
        refused_as(combine(gains=g), I, name + f"gains[{i}][{j}] is not finite", it)
    refused_as(combine(weights=np.float32([1, np.inf, 1])), I, name + "weights[1] is not finite", it)
    refused_as(combine(weights=np.float32([1, 1, np.nan])), I, name + "weights[2] is not finite", it)
    for o in (d, d + 4 * (6 * plane - 1)):  # on the planes, on their last float
        refused_as(combine(out=o), I, name + "out overlaps the planes", it)
    refused_as(combine(planes=d + 4 * (plane - 1), out=d), I, name + "out overlaps the planes", it)
    g = ones.copy()
    g[0, 0] = np.inf
    refused_as(combine(gains=g, out=d), I, name + "gains[0][0] is not finite", it)  # the gains before the overlap
    for bad in (np.float32([[1, 1, np.nan]] * 5), np.float32([[1, np.inf, 1]] * 5)):  # the host wrapper checks too
        with pytest.raises(bdpt_amd.BdptError, match="finite"):
            it.combine_group_planes(np.zeros((5, 2, 4, 4, 3), np.float32), bad)


# --------------------------------------------------------------- 8. non-interference
def test_gpu_plain_frames_around_a_crossed_render_are_unchanged():
    it = golden_integrator(RING_CASE)  # caustic: glossy materials, so the default build by name
    before = it.render_frame().copy()
    k0 = it.stats()["kernel"]
    n = bound_of(RING_CASE)
    planes = it.render_group_layers(n)
    assert it.stats()["kernel"] == GL_KERNEL
    more = it.render_group_strategies(unweighted=True)
    assert it.stats()["kernel"] == GS_KERNEL[True]
    weighted = it.render_group_strategies()
    assert it.stats()["kernel"] == GS_KERNEL[False]
    it.rgb[:] = 0
    after = it.render_frame().copy()
    k1 = it.stats()["kernel"]
    assert k0 == k1 == "bdpt_frame_kernel", (k0, k1)
    assert rel_l2(after, before).max() <= TOL
    assert rel_l2(plane_sum(planes), before).max() <= TOL and rel_l2(plane_sum(weighted), before).max() <= TOL
    assert more.shape == weighted.shape


def test_gpu_group_map_may_be_overwritten_after_the_call():
    """The asynchronous entries copy the caller's map before they return."""
    import torch

    it = golden_integrator(EDGES_CASE)
    n = bound_of(EDGES_CASE)
    fb = torch.zeros((2, n, 32, 32, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m = np.int32([0, 0, 1, 1, 1])
    it.render_group_layers_device(n, fb.data_ptr(), m, 2)
    m[:] = 0
    it.synchronize()
    assert worst_per_plane(fb.cpu().numpy(), group_layers_of(EDGES_CASE, n, [0, 0, 1, 1, 1], 2)) <= TOL
    shape = shape_of(EDGES_CASE)
    fs = torch.zeros((5,) + tuple(shape) + (32, 32, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m = np.int32([0, 1, 2, 3, 4])
    it.render_group_strategies_device(fs.data_ptr(), shape[0], shape[1], False, m, 5)
    m[:] = 0
    it.synchronize()
    assert worst_per_plane(fs.cpu().numpy(), group_strategies_of(EDGES_CASE)) <= TOL


# ------------------------------------------------------------------- 9. the command line
def test_gpu_cli_cross_writes_one_exr_per_group_and_layer(tmp_path):
    """--light-groups --layers 3 --cross on emit_edges: fifteen extra EXRs that sum to the main one
    within half-float rounding, the bound of the light-group and layer CLI tests: every file is
    rounded to half once (relative error <= 2^-11 for a normal half) and the planes are
    non-negative, so the sum of the rounded planes is within 2^-11 of the exact sum, the main file
    within 2^-11 more, and two renders differ by the order of their float32 atomic additions (<=
    1e-4, about 0.2 of 2^-11): within 3 * 2^-11. Subnormal halves round absolutely, by at most
    2^-25 in each file: the floor 2^-22 (sixteen files here, 2^-21 at worst; the floor is kept and
    holds because subnormal values do not meet in one pixel of many planes)."""
    W = H = 32
    spp = 4
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    for sub in ("cross", "both", "usage"):
        (tmp_path / sub).mkdir()
        (tmp_path / sub / "scene.toml").write_text(variants.toml_text("emit_edges", W, H, spp))
    crossed = [f"scene.E{e:02d}L{l:02d}.exr" for e in range(5) for l in range(3)]
    r = subprocess.run([cli, str(tmp_path / "cross" / "scene.toml"), "--light-groups", "--layers", "3", "--cross"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "cross")) == sorted(crossed + ["scene.exr", "scene.toml"])
    main = decode_exr((tmp_path / "cross" / "scene.exr").read_bytes()).astype(np.float64)
    parts = [decode_exr((tmp_path / "cross" / f).read_bytes()).astype(np.float64) for f in crossed]
    assert all(p.shape == main.shape for p in parts)
    total = sum(parts)
    tol = 3 * 2.0 ** -11 * np.maximum(total, main) + 2.0 ** -22
    assert (np.abs(total - main) <= tol).all(), float((np.abs(total - main) / np.maximum(main, 1e-6)).max())
    # without --cross the two flags write what they write today: two independent sets
    r = subprocess.run([cli, str(tmp_path / "both" / "scene.toml"), "--light-groups", "--layers", "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "both")) == sorted([f"scene.E{e:02d}.exr" for e in range(5)] +
                                                           [f"scene.L{l:02d}.exr" for l in range(3)] + ["scene.exr", "scene.toml"])
    # usage errors name --cross and write nothing
    for flags in (["--cross"], ["--cross", "--layers", "3"], ["--cross", "--light-groups"],
                  ["--cross", "--light-groups", "--layers", "3", "--strategies"]):
        r = subprocess.run([cli, str(tmp_path / "usage" / "scene.toml")] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--cross" in r.stderr, (flags, r.stderr)
    assert os.listdir(tmp_path / "usage") == ["scene.toml"]
