"""Cost of keeping a frame as planes: python tools/planes_cost.py layers | groups | strategies |
group-layers | group-strategies.
Kernel time by HIP events (stats()["kernel_ms"]), 512^2 x 64, 2 warm-up + 7 alternating rounds per
scene, medians; one JSON line per table.
  layers      Caustic: the plain frame vs n_layers 1 / 4 / 8 / 16, and composing 8 layers.
  groups      emit_edges (five emitters) and Caustic (one): the plain frame vs the grouped render
              (identity map); then the relight kernel with 5 and 64 planes (a loop of launches
              between two synchronises, and the bytes it reads and writes over that time).
  strategies  Caustic: the plain frame, 16 layers, weighted and unweighted strategies at the shape
              helper's full shape, and the contact sheet. Then, on scenes/kat/layers_open.obj
              (diffuse, no delta surface), the frame means of the unweighted planes (0, 3), (1, 2)
              and (2, 1) at a few spp: three unbiased estimators of one direct-light image
              (printed, not compared).
  group-layers      Caustic (one emitter) and emit_edges (five): the plain frame, the grouped render,
              16 layers and the crossed (group, layer) render at 16 layers; then the combine kernel
              on the crossed planes just rendered.
  group-strategies  The same two scenes: the plain frame, the grouped render, the weighted and
              unweighted strategies at the shape helper's full shape, the crossed (group, s, t)
              renders of both weightings, and the combine kernel on the crossed planes."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("scenes", "bidirectional-path-tracing_amd"):
    sys.path.insert(0, os.path.join(REPO, sub))
import bdpt_amd  # noqa: E402
import variants  # noqa: E402

W = H = 512
SPP = 64
WARMUP, ROUNDS = 2, 7
DEV = torch.device("cuda", 0)


def integrator(name):
    sc = variants.SCENES[name]
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=W, height=H, spp=SPP, rr_depth=sc["rr_depth"])
    return bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(name)), cfg)


def alternate(it, calls):
    """WARMUP + ROUNDS rounds of the labelled calls in order -> ({label: [kernel_ms]}, {label: kernel})."""
    series, kernels = {label: [] for label in calls}, {}
    for r in range(WARMUP + ROUNDS):
        for label, call in calls.items():
            call()
            it.synchronize()
            st = it.stats()
            kernels[label] = st["kernel"]
            if r >= WARMUP:
                series[label].append(st["kernel_ms"])
    return series, kernels


def rounded(series, digits=3):
    return {k: [round(x, digits) for x in v] for k, v in series.items()}


def layers():
    it = integrator("caustic")
    fb = torch.zeros(16 * W * H * 3, dtype=torch.float32, device=DEV)
    out = torch.zeros(W * H * 3, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    calls = {"plain": lambda: it.render_device(fb.data_ptr())}
    for n in (1, 4, 8, 16):
        calls[str(n)] = lambda n=n: it.render_layers_device(n, fb.data_ptr())
    calls["compose8"] = lambda: it.compose_layers_device(fb.data_ptr(), 8, W, H, 0xff, out.data_ptr())
    series, kernels = alternate(it, calls)
    med = {k: statistics.median(v) for k, v in series.items()}
    print(json.dumps({"series_ms": rounded(series), "median_ms": med,
                      "ratio_vs_plain": {k: round(med[k] / med["plain"], 4) for k in ("1", "4", "8", "16")},
                      "kernel": kernels["compose8"]}))


def groups():
    out = {"frame": f"{W}x{H}x{SPP}", "rounds": ROUNDS}
    fb = torch.zeros(64 * W * H * 3, dtype=torch.float32, device=DEV)
    res = torch.zeros(W * H * 3, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    for name in ("emit_edges", "caustic"):
        it = integrator(name)
        series, kernels = alternate(it, {"plain": lambda: it.render_device(fb.data_ptr()),
                                         "grouped": lambda: it.render_light_groups_device(fb.data_ptr())})
        med = {k: statistics.median(v) for k, v in series.items()}
        out[name] = {"emitters": len(it.scene.emitters()), "kernels": kernels, "series_ms": rounded(series),
                     "median_ms": {k: round(v, 3) for k, v in med.items()},
                     "grouped_over_plain": round(med["grouped"] / med["plain"], 4)}
    # relight: planes as the last render left them (any finite floats serve). Per call: a host clock
    # around LAUNCHES calls on the context's stream that ends in a synchronise (the call's own
    # bookkeeping - two small memsets and two event records - included); kernel_ms: the call's own
    # event pair around its one launch.
    LAUNCHES = 200
    for n in (5, 64):
        gains = np.linspace(0.25, 4.0, 3 * n, dtype=np.float32).reshape(n, 3)
        for _ in range(10):
            it.relight_device(fb.data_ptr(), n, W, H, gains, res.data_ptr())
        it.synchronize()
        times, kernel = [], []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(LAUNCHES):
                it.relight_device(fb.data_ptr(), n, W, H, gains, res.data_ptr())
            it.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / LAUNCHES)
            kernel.append(it.stats()["kernel_ms"])
        ms, kms = statistics.median(times), statistics.median(kernel)
        read, written = n * W * H * 3 * 4, W * H * 3 * 4
        out[f"relight_{n}"] = {"ms_per_call": round(ms, 5), "series_ms": [round(x, 5) for x in times],
                               "kernel_ms": round(kms, 5), "kernel_series_ms": [round(x, 5) for x in kernel],
                               "plane_bytes_read": read, "bytes_written": written,
                               "GBps_per_call": round((read + written) / ms / 1e6, 1),
                               "GBps_kernel": round((read + written) / kms / 1e6, 1)}
    print(json.dumps(out))


def strategies():
    it = integrator("caustic")
    n_s, n_t = bdpt_amd.strategies_shape(it.config.rr_depth, it.config.strategy)
    fb = torch.zeros(n_s * n_t * W * H * 3, dtype=torch.float32, device=DEV)
    sheet = torch.zeros(n_s * n_t * W * H * 3, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    series, kernels = alternate(it, {
        "plain": lambda: it.render_device(fb.data_ptr()),
        "layers16": lambda: it.render_layers_device(16, fb.data_ptr()),
        "weighted": lambda: it.render_strategies_device(fb.data_ptr(), n_s, n_t),
        "unweighted": lambda: it.render_strategies_device(fb.data_ptr(), n_s, n_t, unweighted=True),
        "sheet": lambda: it.strategies_sheet_device(fb.data_ptr(), n_s, n_t, W, H, None, sheet.data_ptr()),
    })
    med = {k: statistics.median(v) for k, v in series.items()}
    print(json.dumps({"shape": [n_s, n_t], "series_ms": rounded(series), "median_ms": {k: round(v, 3) for k, v in med.items()},
                      "range_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in series.items()},
                      "ratio_vs_plain": {k: round(med[k] / med["plain"], 4) for k in ("layers16", "weighted", "unweighted")},
                      "ratio_vs_layers16": {k: round(med[k] / med["layers16"], 4) for k in ("weighted", "unweighted")},
                      "kernels": kernels}))
    del fb, sheet
    # three estimators of one image: the unweighted k = 2 planes of the open scene (tests/plane_cases.py's camera)
    camera = dict(eye=(0.0, 0.6, 3.0), at=(0.0, 0.6, 0.0), up=(0.0, 1.0, 0.0), fov=45.0)
    scene = bdpt_amd.Scene(os.path.join(REPO, "scenes", "kat", "layers_open.obj"))
    rows = {}
    for n in (1, 8, 64, 512):
        o = bdpt_amd.BDPTIntegrator(scene, bdpt_amd.Config(camera=bdpt_amd.Camera(**camera), width=48, height=48, spp=n, rr_depth=5))
        o.init()
        p = o.render_strategies(unweighted=True)
        rows[n] = {f"({s}, {t})": [float(f"{x:.5g}") for x in p[s, t - 1].astype("float64").mean(axis=(0, 1))]
                   for s, t in ((0, 3), (1, 2), (2, 1))}
    print(json.dumps({"layers_open_unweighted_k2_frame_means_rgb": rows}))


def crossed(inner):
    """inner(it) -> (planes per group, {label: single-kind call(fb)}, {label: crossed call(fb)}); one JSON line."""
    out = {"frame": f"{W}x{H}x{SPP}", "rounds": ROUNDS}
    res = torch.zeros(W * H * 3, dtype=torch.float32, device=DEV)
    for name in ("caustic", "emit_edges"):
        it = integrator(name)
        n_groups = len(it.scene.emitters())
        n_inner, single, cross = inner(it)
        fb = torch.zeros(n_groups * n_inner * W * H * 3, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        calls = {"plain": lambda: it.render_device(fb.data_ptr()), "grouped": lambda: it.render_light_groups_device(fb.data_ptr())}
        calls.update({k: (lambda f=f: f(fb.data_ptr())) for k, f in {**single, **cross}.items()})
        gains = np.linspace(0.25, 4.0, 3 * n_groups, dtype=np.float32).reshape(n_groups, 3)
        weights = np.linspace(0.5, 2.0, n_inner, dtype=np.float32)
        calls["combine"] = lambda: it.combine_group_planes_device(fb.data_ptr(), n_groups, n_inner, W, H, gains, weights,
                                                                  res.data_ptr())
        series, kernels = alternate(it, calls)
        med = {k: statistics.median(v) for k, v in series.items()}
        parents = ["grouped"] + list(single)
        out[name] = {"emitters": n_groups, "planes_per_group": n_inner, "kernels": kernels, "series_ms": rounded(series),
                     "median_ms": {k: round(v, 3) for k, v in med.items()},
                     "range_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in series.items()},
                     "ratio_vs_plain": {k: round(med[k] / med["plain"], 4) for k in parents + list(cross)},
                     "crossed_over_dearer_parent": {k: round(med[k] / max(med[q] for q in parents), 4) for k in cross},
                     "combine_bytes": (n_groups * n_inner + 1) * W * H * 3 * 4}
        del fb
    print(json.dumps(out))


def group_layers():
    n = 16
    crossed(lambda it: (n, {f"layers{n}": lambda fb: it.render_layers_device(n, fb)},
                        {"crossed": lambda fb: it.render_group_layers_device(n, fb)}))


def group_strategies():
    def inner(it):
        n_s, n_t = bdpt_amd.strategies_shape(it.config.rr_depth, it.config.strategy)
        return (n_s * n_t,
                {"weighted": lambda fb: it.render_strategies_device(fb, n_s, n_t),
                 "unweighted": lambda fb: it.render_strategies_device(fb, n_s, n_t, unweighted=True)},
                {"crossed_weighted": lambda fb: it.render_group_strategies_device(fb, n_s, n_t),
                 "crossed_unweighted": lambda fb: it.render_group_strategies_device(fb, n_s, n_t, unweighted=True)})
    crossed(inner)


if __name__ == "__main__":
    modes = {"layers": layers, "groups": groups, "strategies": strategies, "group-layers": group_layers,
             "group-strategies": group_strategies}
    if len(sys.argv) != 2 or sys.argv[1] not in modes:
        sys.exit("usage: planes_cost.py " + " | ".join(modes))
    modes[sys.argv[1]]()
