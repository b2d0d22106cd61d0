"""Every refusal of the plane entries, by its whole text (bdpt_last_error) and its code:
bdpt_render_layers[_host], bdpt_render_light_groups[_host], bdpt_render_strategies[_host],
bdpt_layers_compose, bdpt_light_groups_relight and bdpt_strategies_sheet[_host]. The texts are
those of the library before the entries shared one plane description; words would not show a
changed message, equality does. Where several refusals apply, the row names the one that wins.

Everything here is refused before a launch. The frames are G1_cbox_low_64x64_spp4's (one
emitter), the set-ups nothing plane-shaped serves are plane_cases.unsupported_setups', and the
combine entries see 2 x 8 x 8 x 3 buffers. The render entries get buffers of 64 planes."""
import ctypes

import numpy as np
import pytest

import bdpt_amd
from conftest import gpu_available
from plane_cases import CBOX_CASE, golden_integrator, unsupported_setups

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

I, U = bdpt_amd.ERR_INVALID, bdpt_amd.ERR_UNSUPPORTED
vp, i32 = ctypes.c_void_p, ctypes.c_int32
PIXEL_FIELD = " * W * H must be below 2^30 (the shadow-ray task record's pixel field)"
NOT_BUILT = {"rr": "with Russian roulette", "deep": "with rr_depth > 28",
             "flags": "with flags (a counting pass or full traversal)", "tex": "for a scene with bitmap textures",
             "hbm": "with the BSDF records in HBM (too many materials for the LDS table)"}
# kind: (entry, arguments of a call that is served, the phrase of "... are not built ...")
KINDS = {"layers": ("bdpt_render_layers", (4,), "path-length layers"),
         "groups": ("bdpt_render_light_groups", (1, None), "light groups"),
         "strategies": ("bdpt_render_strategies", (2, 2, 0), "strategies (per-(s, t) images)")}


@pytest.fixture(scope="module")
def env():
    import torch

    mp = pytest.MonkeyPatch()
    e = dict(zip(("rr", "deep", "flags", "tex", "hbm"), (s[0] for s in unsupported_setups(CBOX_CASE, mp))))
    mp.undo()
    e["good"] = golden_integrator(CBOX_CASE)
    for name, (w, h) in (("big", (32768, 16384)), ("huge", (32768, 32768))):  # in the params only
        e[name] = golden_integrator(CBOX_CASE)
        e[name].config.width, e[name].config.height = w, h
    e["host"] = np.zeros(64 * 64 * 64 * 3, np.float32)
    e["dev"] = torch.zeros(64 * 64 * 64 * 3, dtype=torch.float32, device="cuda")
    e["planes"] = torch.zeros(3 * 8 * 8 * 3, dtype=torch.float32, device="cuda")  # 2 planes, then the frame
    e["sheet"] = torch.zeros(2 * 2 * 8 * 8 * 3, dtype=torch.float32, device="cuda")  # 2 x 1 planes, then their sheet
    e["hplanes"] = np.zeros(2 * 8 * 8 * 3, np.float32)
    torch.cuda.synchronize()
    L = bdpt_amd.lib()
    L.bdpt_strategies_sheet_host.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    return e


def render(kind, form, it="good", args=None, flags=0, fb=True, window=None, **params):
    """A call of the kind's host or device render entry on env[it], the served arguments unless given."""
    def call(e):
        p = e[it].params(0, 1, flags)
        for k, v in params.items():
            setattr(p, k, v)
        w = None if window is None else ctypes.byref(bdpt_amd.SampleWindow(*window).c())
        a = [x.ctypes.data if isinstance(x, np.ndarray) else x for x in (KINDS[kind][1] if args is None else args)]
        if form == "host":
            return getattr(bdpt_amd.lib(), KINDS[kind][0] + "_host")(e[it]._h, ctypes.byref(p), w, *a,
                                                                     e["host"].ctypes.data if fb else None)
        return getattr(bdpt_amd.lib(), KINDS[kind][0])(e[it]._h, ctypes.byref(p), w, *a, e["dev"].data_ptr() if fb else None,
                                                       None)
    return call


TWO = 2 * 8 * 8 * 3  # floats of two 8 x 8 planes


def at(buffer, floats):
    """A pointer that many floats into a device buffer (None: null). Every row stays inside its buffer."""
    return None if floats is None else buffer.data_ptr() + 4 * floats


def compose(n=2, w=8, h=8, mask=3, planes=0, out=TWO, ctx=True):
    return lambda e: bdpt_amd.lib().bdpt_layers_compose(e["good"]._h if ctx else None, at(e["planes"], planes), n, w, h, mask,
                                                        at(e["planes"], out), None)


def relight(n=2, w=8, h=8, gains=np.ones(6, np.float32), planes=0, out=TWO):
    return lambda e: bdpt_amd.lib().bdpt_light_groups_relight(e["good"]._h, at(e["planes"], planes), n, w, h,
                                                              None if gains is None else gains.ctypes.data,
                                                              at(e["planes"], out), None)


def sheet(n_s=2, n_t=1, w=8, h=8, gains=None, planes=0, out=TWO, host=False):
    def call(e):
        g = None if gains is None else gains.ctypes.data
        if host:
            return bdpt_amd.lib().bdpt_strategies_sheet_host(e["good"]._h, None if planes is None else e["hplanes"].ctypes.data,
                                                             n_s, n_t, w, h, g, None if out is None else e["host"].ctypes.data)
        return bdpt_amd.lib().bdpt_strategies_sheet(e["good"]._h, at(e["sheet"], planes), n_s, n_t, w, h, g, at(e["sheet"], out),
                                                    None)
    return call


def bad_gains(n, i, j, v):
    g = np.ones((n, 3), np.float32)
    g[i, j] = v
    return g


ROWS = []  # (id, call(env) -> status, code, the whole message)
for form in ("host", "device"):
    def row(kind, label, call_args, code, text):
        ROWS.append((f"{KINDS[kind][0]}{'_host' if form == 'host' else ''}-{label}", render(kind, form, **call_args), code, text))

    for kind, (entry, _, phrase) in KINDS.items():
        row(kind, "null fb", dict(fb=False), I, "null argument")
        row(kind, "params first", dict(rr_depth=0, args=(0, None) if kind == "groups" else (0, 0, 0)[:len(KINDS[kind][1])]),
            U, "rr_depth must be in [1, 1024]")
        row(kind, "window first", dict(window=(0, 0, 1), args=(0, None) if kind == "groups" else (0, 0, 0)[:len(KINDS[kind][1])]),
            I, "sample window: stride must be >= 1")
        for what, text in NOT_BUILT.items():
            row(kind, what, dict(it=what, flags=bdpt_amd.FLAG_COUNT if what == "flags" else 0), U,
                f"{phrase} are not built {text}")
        row(kind, "flags before roulette", dict(it="rr", flags=bdpt_amd.FLAG_COUNT), U, f"{phrase} are not built {NOT_BUILT['flags']}")
        row(kind, "roulette before rr_depth", dict(it="rr", rr_depth=29), U, f"{phrase} are not built {NOT_BUILT['rr']}")
    for n in (0, 65, -1):
        row("layers", f"n_layers {n}", dict(args=(n,)), I, "bdpt_render_layers: n_layers must be in [1, 64]")
        row("groups", f"n_groups {n}", dict(args=(n, np.int32([0]))), I, "bdpt_render_light_groups: n_groups must be in [1, 64]")
    row("layers", "count before flags", dict(args=(65,), flags=bdpt_amd.FLAG_COUNT), I, "bdpt_render_layers: n_layers must be in [1, 64]")
    row("layers", "2^30", dict(it="big", args=(2,)), I, "bdpt_render_layers: n_layers" + PIXEL_FIELD)
    row("layers", "2^30 one plane", dict(it="huge", args=(1,)), I, "bdpt_render_layers: n_layers" + PIXEL_FIELD)
    row("layers", "count before 2^30", dict(it="big", args=(65,)), I, "bdpt_render_layers: n_layers must be in [1, 64]")
    row("layers", "2^30 before flags", dict(it="big", args=(2,), flags=bdpt_amd.FLAG_COUNT), I,
        "bdpt_render_layers: n_layers" + PIXEL_FIELD)
    row("groups", "2^30", dict(it="big", args=(2, np.int32([0]))), I, "bdpt_render_light_groups: n_groups" + PIXEL_FIELD)
    row("groups", "2^30 before the map", dict(it="big", args=(2, np.int32([7]))), I,
        "bdpt_render_light_groups: n_groups" + PIXEL_FIELD)
    row("groups", "null map", dict(args=(4, None)), I,
        "bdpt_render_light_groups: a null group_of_emitter is the identity map and needs n_groups equal to the emitter "
        "count (1), got 4")
    row("groups", "map above", dict(args=(5, np.int32([5]))), I,
        "bdpt_render_light_groups: group_of_emitter[0] = 5 is outside [0, n_groups)")
    row("groups", "map below", dict(args=(5, np.int32([-1]))), I,
        "bdpt_render_light_groups: group_of_emitter[0] = -1 is outside [0, n_groups)")
    row("groups", "map before roulette", dict(it="rr", args=(5, np.int32([5]))), I,
        "bdpt_render_light_groups: group_of_emitter[0] = 5 is outside [0, n_groups)")
    for n_s in (0, 30):
        row("strategies", f"n_s {n_s}", dict(args=(n_s, 2, 0)), I, "bdpt_render_strategies: n_s must be in [1, 29]")
    for n_t in (0, 29):
        row("strategies", f"n_t {n_t}", dict(args=(2, n_t, 0)), I, "bdpt_render_strategies: n_t must be in [1, 28]")
    row("strategies", "n_s before n_t", dict(args=(30, 29, 2)), I, "bdpt_render_strategies: n_s must be in [1, 29]")
    for weighting in (2, -1):
        row("strategies", f"weighting {weighting}", dict(args=(2, 2, weighting)), I,
            "bdpt_render_strategies: weighting must be BDPT_STRATEGIES_WEIGHTED (0) or BDPT_STRATEGIES_UNWEIGHTED (1)")
    row("strategies", "shape before 2^30", dict(it="big", args=(32, 32, 0)), I, "bdpt_render_strategies: n_s must be in [1, 29]")
    row("strategies", "weighting before 2^30", dict(it="big", args=(2, 1, 2)), I,
        "bdpt_render_strategies: weighting must be BDPT_STRATEGIES_WEIGHTED (0) or BDPT_STRATEGIES_UNWEIGHTED (1)")
    for shape in ((2, 1), (1, 2)):
        row("strategies", f"2^30 {shape}", dict(it="big", args=shape + (1,)), I, "bdpt_render_strategies: n_s * n_t" + PIXEL_FIELD)
    row("strategies", "2^30 before flags", dict(it="big", args=(2, 1, 0), flags=bdpt_amd.FLAG_COUNT), I,
        "bdpt_render_strategies: n_s * n_t" + PIXEL_FIELD)

ROWS += [
    ("bdpt_layers_compose-null ctx", compose(ctx=False), I, "null argument"),
    ("bdpt_layers_compose-null planes", compose(planes=None), I, "null argument"),
    ("bdpt_layers_compose-null out", compose(out=None), I, "null argument"),
    ("bdpt_layers_compose-n 0", compose(n=0), I, "bdpt_layers_compose: n_layers must be in [1, 64]"),
    ("bdpt_layers_compose-n 65", compose(n=65), I, "bdpt_layers_compose: n_layers must be in [1, 64]"),
    ("bdpt_layers_compose-width 0", compose(w=0), I, "bdpt_layers_compose: width/height must be > 0 and n_layers * W * H below 2^30"),
    ("bdpt_layers_compose-height -1", compose(h=-1), I, "bdpt_layers_compose: width/height must be > 0 and n_layers * W * H below 2^30"),
    ("bdpt_layers_compose-2^30", compose(w=32768, h=16384), I,
     "bdpt_layers_compose: width/height must be > 0 and n_layers * W * H below 2^30"),
    ("bdpt_layers_compose-empty mask", compose(mask=0), I, "bdpt_layers_compose: empty layer mask"),
    ("bdpt_layers_compose-mask above", compose(mask=4), I, "bdpt_layers_compose: the mask has bits at or above n_layers"),
    ("bdpt_layers_compose-count before mask", compose(n=65, mask=0), I, "bdpt_layers_compose: n_layers must be in [1, 64]"),
    ("bdpt_light_groups_relight-null planes", relight(planes=None), I, "null argument"),
    ("bdpt_light_groups_relight-null gains", relight(gains=None), I, "null argument"),
    ("bdpt_light_groups_relight-null out", relight(out=None), I, "null argument"),
    ("bdpt_light_groups_relight-n 0", relight(n=0), I, "bdpt_light_groups_relight: n_groups must be in [1, 64]"),
    ("bdpt_light_groups_relight-n 65", relight(n=65, gains=np.ones(195, np.float32)), I,
     "bdpt_light_groups_relight: n_groups must be in [1, 64]"),
    ("bdpt_light_groups_relight-width 0", relight(w=0), I,
     "bdpt_light_groups_relight: width/height must be > 0 and n_groups * W * H below 2^30"),
    ("bdpt_light_groups_relight-2^30", relight(w=32768, h=16384), I,
     "bdpt_light_groups_relight: width/height must be > 0 and n_groups * W * H below 2^30"),
    ("bdpt_light_groups_relight-nan gain", relight(gains=bad_gains(2, 1, 2, np.nan)), I,
     "bdpt_light_groups_relight: gains[1][2] is not finite"),
    ("bdpt_light_groups_relight-inf gain", relight(gains=bad_gains(2, 0, 1, -np.inf)), I,
     "bdpt_light_groups_relight: gains[0][1] is not finite"),
    ("bdpt_light_groups_relight-out on the planes", relight(out=0), I,
     "bdpt_light_groups_relight: out overlaps the planes"),
    ("bdpt_light_groups_relight-out on the last float", relight(out=TWO - 1), I,
     "bdpt_light_groups_relight: out overlaps the planes"),
    ("bdpt_light_groups_relight-planes on out's end", relight(n=1, planes=8 * 8 * 3 - 1, out=0), I,
     "bdpt_light_groups_relight: out overlaps the planes"),
    ("bdpt_light_groups_relight-gains before overlap",
     relight(gains=bad_gains(2, 0, 0, np.inf), out=0), I,
     "bdpt_light_groups_relight: gains[0][0] is not finite"),
]
for host in (False, True):
    name = "bdpt_strategies_sheet" + ("_host" if host else "")
    ROWS += [
        (f"{name}-null planes", sheet(planes=None, host=host), I, "null argument"),
        (f"{name}-null out", sheet(out=None, host=host), I, "null argument"),
        (f"{name}-n_s 0", sheet(n_s=0, host=host), I, "bdpt_strategies_sheet: n_s must be in [1, 29]"),
        (f"{name}-n_s 30", sheet(n_s=30, host=host), I, "bdpt_strategies_sheet: n_s must be in [1, 29]"),
        (f"{name}-n_t 0", sheet(n_t=0, host=host), I, "bdpt_strategies_sheet: n_t must be in [1, 28]"),
        (f"{name}-n_t 29", sheet(n_t=29, host=host), I, "bdpt_strategies_sheet: n_t must be in [1, 28]"),
        (f"{name}-width 0", sheet(w=0, host=host), I, "bdpt_strategies_sheet: width/height must be > 0"),
        (f"{name}-height -1", sheet(h=-1, host=host), I, "bdpt_strategies_sheet: width/height must be > 0"),
        (f"{name}-2^31", sheet(n_s=29, n_t=28, w=1024, h=1024, host=host), I,
         "bdpt_strategies_sheet: the sheet (n_s * n_t * W * H * 3 floats) must be below 2^31 floats"),
        (f"{name}-nan gain", sheet(gains=bad_gains(2, 1, 0, np.nan), host=host), I, "bdpt_strategies_sheet: gains[1][0] is not finite"),
        (f"{name}-inf gain", sheet(gains=bad_gains(2, 0, 2, np.inf), host=host), I, "bdpt_strategies_sheet: gains[0][2] is not finite"),
    ]
ROWS += [
    ("bdpt_strategies_sheet-out on the planes", sheet(out=0), I,
     "bdpt_strategies_sheet: out overlaps the planes"),
    ("bdpt_strategies_sheet-out on the last float", sheet(out=TWO - 1), I,
     "bdpt_strategies_sheet: out overlaps the planes"),
    ("bdpt_strategies_sheet-planes on out's end", sheet(planes=TWO - 1, out=0), I,
     "bdpt_strategies_sheet: out overlaps the planes"),
    ("bdpt_strategies_sheet-gains before overlap", sheet(gains=bad_gains(2, 1, 1, np.inf), out=0), I,
     "bdpt_strategies_sheet: gains[1][1] is not finite"),
]


@pytest.mark.parametrize("call,code,text", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_gpu_plane_entry_refuses_with_the_same_message(env, call, code, text):
    status = call(env)
    assert (status, bdpt_amd.lib().bdpt_last_error().decode()) == (code, text)
