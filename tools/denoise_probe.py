"""Kernel times of the preview path (python tools/denoise_probe.py [scene] [reps]): for 512^2
and 1024^2, bdpt_render_aov at spp 1 and spp 16, bdpt_denoise at 5 iterations, and the 1-spp
bdpt_render of the same frame (what the filter is an overhead on). Device buffers, the
library's HIP events around the kernels of each call (bdpt_stats.kernel_ms), 3 warm-up calls,
then `reps` calls: median, min and max in ms. One JSON object on stdout."""
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bidirectional-path-tracing_amd"), os.path.join(REPO, "scenes")]
import bdpt_amd  # noqa: E402
import variants  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "caustic"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
WARMUP = 3
sc = variants.SCENES[name]
scene = bdpt_amd.Scene(variants.obj_path(name))
dev = torch.device("cuda", 0)


def timed(it, call):
    ms = []
    for r in range(WARMUP + reps):
        call()
        it.synchronize()
        if r >= WARMUP:
            ms.append(it.stats()["kernel_ms"])
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


out = dict(scene=name, reps=reps, warmup=WARMUP, device=torch.cuda.get_device_name(0),
           kernel_build=bdpt_amd.kernel_build_hash(), sizes={})
for side in (512, 1024):
    res = {}
    rgb = torch.zeros(side * side * 3, dtype=torch.float32, device=dev)
    aov = torch.zeros(side * side * 8, dtype=torch.float32, device=dev)
    den = torch.zeros(side * side * 3, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for spp in (1, 16):
        cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=side, height=side, spp=spp,
                              rr_depth=sc["rr_depth"])
        it = bdpt_amd.BDPTIntegrator(scene, cfg)
        res[f"render_aov_spp{spp}"] = timed(it, lambda: it.render_aov_device(aov.data_ptr()))
        if spp == 1:
            res["bdpt_render_spp1"] = timed(it, lambda: it.render_device(rgb.data_ptr()))
            # a frame and its feature buffers of exactly one pass each for the filter to work on
            rgb.zero_(), aov.zero_()
            torch.cuda.synchronize()
            it.render_device(rgb.data_ptr())
            it.render_aov_device(aov.data_ptr())
            it.synchronize()
            res["denoise_5_iterations"] = timed(
                it, lambda: it.denoise_device(rgb.data_ptr(), aov.data_ptr(), den.data_ptr(),
                                              settings=bdpt_amd.DenoiseSettings(iterations=5)))
            assert bool(torch.isfinite(den).all())
        it.close()
    res["denoise_over_render_spp1"] = round(res["denoise_5_iterations"]["median_ms"] /
                                            res["bdpt_render_spp1"]["median_ms"], 3)
    out["sizes"][f"{side}x{side}"] = res
print(json.dumps(out))
