"""Cost of light groups: a plain frame vs the grouped render of the same frame (identity map) on
emit_edges (five emitters) and Caustic (one), 512^2 x 64, alternating rounds, medians of
kernel_ms; then the relight kernel at 512^2 with 5 and 64 planes (a loop of launches between two
synchronises, and the bytes it reads and writes over that time)."""
import os, sys, statistics, json
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("scenes", "bidirectional-path-tracing_amd"):
    sys.path.insert(0, os.path.join(REPO, sub))
import bdpt_amd, variants
W = H = 512
spp = 64
ROUNDS = 7
dev = torch.device("cuda", 0)
out = {"frame": f"{W}x{H}x{spp}", "rounds": ROUNDS}
fb = torch.zeros(64 * W * H * 3, dtype=torch.float32, device=dev)
res = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
torch.cuda.synchronize()
it = None
for name in ("emit_edges", "caustic"):
    sc = variants.SCENES[name]
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=W, height=H, spp=spp, rr_depth=sc["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(name)), cfg)
    n = len(it.scene.emitters())
    def plain():
        it.render_device(fb.data_ptr()); it.synchronize(); return it.stats()["kernel_ms"], it.stats()["kernel"]
    def grouped():
        it.render_light_groups_device(fb.data_ptr()); it.synchronize(); return it.stats()["kernel_ms"], it.stats()["kernel"]
    for _ in range(2):
        plain(); grouped()
    series = {"plain": [], "grouped": []}
    kernels = {}
    for _ in range(ROUNDS):
        for label, f in (("plain", plain), ("grouped", grouped)):
            ms, k = f()
            series[label].append(ms)
            kernels[label] = k
    med = {k: statistics.median(v) for k, v in series.items()}
    out[name] = {"emitters": n, "kernels": kernels, "series_ms": {k: [round(x, 3) for x in v] for k, v in series.items()},
                 "median_ms": {k: round(v, 3) for k, v in med.items()}, "grouped_over_plain": round(med["grouped"] / med["plain"], 4)}
# relight: planes as the last render left them (any finite floats serve). Per call: a host clock
# around LAUNCHES calls on the context's stream that ends in a synchronise (the call's own
# bookkeeping - two small memsets and two event records - included); kernel_ms: the call's own
# event pair around its one launch.
import time
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
