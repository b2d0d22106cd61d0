"""Cost of the strategy images: Caustic 512^2 x 64 (rr_depth 8), kernel time by HIP events, 2 warm-up + 7
alternating rounds of (plain frame, 16 layers, weighted strategies, unweighted strategies, both at the
shape helper's full shape) on this build; the contact sheet's time. Then, on scenes/kat/layers_open.obj
(diffuse, no delta surface), the frame means of the unweighted planes (0, 3), (1, 2) and (2, 1) at a few
spp: three unbiased estimators of the same direct-light image (printed, not compared)."""
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("scenes", "bidirectional-path-tracing_amd"):
    sys.path.insert(0, os.path.join(REPO, sub))
import bdpt_amd  # noqa: E402
import variants  # noqa: E402

W = H = 512
spp = 64
sc = variants.SCENES["caustic"]
cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=W, height=H, spp=spp, rr_depth=sc["rr_depth"])
it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path("caustic")), cfg)
n_s, n_t = bdpt_amd.strategies_shape(cfg.rr_depth, cfg.strategy)
dev = torch.device("cuda", 0)
fb = torch.zeros(n_s * n_t * W * H * 3, dtype=torch.float32, device=dev)
sheet = torch.zeros(n_s * n_t * W * H * 3, dtype=torch.float32, device=dev)
torch.cuda.synchronize()
kernels = {}


def timed(label, call):
    call()
    it.synchronize()
    kernels[label] = it.stats()["kernel"]
    return it.stats()["kernel_ms"]


ROUND = {
    "plain": lambda: it.render_device(fb.data_ptr()),
    "layers16": lambda: it.render_layers_device(16, fb.data_ptr()),
    "weighted": lambda: it.render_strategies_device(fb.data_ptr(), n_s, n_t),
    "unweighted": lambda: it.render_strategies_device(fb.data_ptr(), n_s, n_t, unweighted=True),
    "sheet": lambda: it.strategies_sheet_device(fb.data_ptr(), n_s, n_t, W, H, None, sheet.data_ptr()),
}
for _ in range(2):
    for label, call in ROUND.items():
        timed(label, call)
res = {label: [] for label in ROUND}
for _ in range(7):
    for label, call in ROUND.items():
        res[label].append(timed(label, call))
med = {k: statistics.median(v) for k, v in res.items()}
print(json.dumps({"shape": [n_s, n_t], "series_ms": {k: [round(x, 3) for x in v] for k, v in res.items()},
                  "median_ms": {k: round(v, 3) for k, v in med.items()},
                  "range_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in res.items()},
                  "ratio_vs_plain": {k: round(med[k] / med["plain"], 4) for k in ("layers16", "weighted", "unweighted")},
                  "ratio_vs_layers16": {k: round(med[k] / med["layers16"], 4) for k in ("weighted", "unweighted")},
                  "kernels": kernels}))
del fb, sheet

# three estimators of one image: the unweighted k = 2 planes of the open scene (tests/test_gpu_layers.py's camera)
OPEN_CAMERA = dict(eye=(0.0, 0.6, 3.0), at=(0.0, 0.6, 0.0), up=(0.0, 1.0, 0.0), fov=45.0)
scene = bdpt_amd.Scene(os.path.join(REPO, "scenes", "kat", "layers_open.obj"))
rows = {}
for n in (1, 8, 64, 512):
    c = bdpt_amd.Config(camera=bdpt_amd.Camera(**OPEN_CAMERA), width=48, height=48, spp=n, rr_depth=5)
    o = bdpt_amd.BDPTIntegrator(scene, c)
    o.init()
    p = o.render_strategies(unweighted=True)
    rows[n] = {f"({s}, {t})": [float(f"{x:.5g}") for x in p[s, t - 1].astype("float64").mean(axis=(0, 1))]
               for s, t in ((0, 3), (1, 2), (2, 1))}
print(json.dumps({"layers_open_unweighted_k2_frame_means_rgb": rows}))
