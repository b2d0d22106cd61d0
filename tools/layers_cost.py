"""Cost of layering: Caustic 512^2 x 64, plain frame vs n_layers 1/4/8/16 on this build, alternating; compose time."""
import os, sys, statistics, json
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("scenes", "bidirectional-path-tracing_amd"):
    sys.path.insert(0, os.path.join(REPO, sub))
import bdpt_amd, variants
W = H = 512
spp = 64
sc = variants.SCENES["caustic"]
cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=W, height=H, spp=spp, rr_depth=sc["rr_depth"])
it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path("caustic")), cfg)
dev = torch.device("cuda", 0)
fb = torch.zeros(16 * W * H * 3, dtype=torch.float32, device=dev)
out = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
torch.cuda.synchronize()
def plain():
    it.render_device(fb.data_ptr()); it.synchronize(); return it.stats()["kernel_ms"]
def layered(n):
    it.render_layers_device(n, fb.data_ptr()); it.synchronize(); return it.stats()["kernel_ms"]
def compose():
    it.compose_layers_device(fb.data_ptr(), 8, W, H, 0xff, out.data_ptr()); it.synchronize(); return it.stats()["kernel_ms"]
for _ in range(2):
    plain(); [layered(n) for n in (1, 4, 8, 16)]; compose()
res = {"plain": [], 1: [], 4: [], 8: [], 16: [], "compose8": []}
for r in range(7):
    res["plain"].append(plain())
    for n in (1, 4, 8, 16):
        res[n].append(layered(n))
    res["compose8"].append(compose())
med = {str(k): statistics.median(v) for k, v in res.items()}
print(json.dumps({"series_ms": {str(k): [round(x, 3) for x in v] for k, v in res.items()}, "median_ms": med,
                  "ratio_vs_plain": {k: round(med[k] / med["plain"], 4) for k in ("1", "4", "8", "16")},
                  "kernel": it.stats()["kernel"]}))
