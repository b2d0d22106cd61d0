"""Times of the planes filter (python tools/denoise_planes_probe.py [scene] [reps]): for 512^2 and
1024^2 and 5, 16 and 64 path-length layers of a 4-spp frame, bdpt_denoise_planes at 5 iterations in
both modes against n_planes successive bdpt_denoise calls on the same planes (what one had before).
Device buffers; every variant between one pair of HIP events on one stream, so the gaps between a
variant's launches and calls count as they do for a viewer; 3 warm-up rounds, then `reps`: median,
min and max in ms. ok: the batched call is not slower than the loop by more than the loop's own
min-max spread. One JSON object on stdout."""
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
stream = torch.cuda.Stream(dev)
settings = bdpt_amd.DenoiseSettings(iterations=5)


def timed(it, call):
    ms = []
    for r in range(WARMUP + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        it.synchronize()
        if r >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


out = dict(scene=name, reps=reps, warmup=WARMUP, iterations=settings.iterations, device=torch.cuda.get_device_name(0),
           kernel_build=bdpt_amd.kernel_build_hash(), sizes={})
for side in (512, 1024):
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=side, height=side, spp=4, rr_depth=sc["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(scene, cfg)
    aov = torch.zeros(side * side * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    it.render_aov_device(aov.data_ptr())
    it.synchronize()
    plane = side * side * 3
    for n in (5, 16, 64):
        planes = torch.zeros(n * plane, dtype=torch.float32, device=dev)
        den = torch.zeros(n * plane, dtype=torch.float32, device=dev)
        guide = torch.zeros(plane, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        it.render_layers_device(n, planes.data_ptr())
        it.synchronize()
        P, A, D, S = planes.data_ptr(), aov.data_ptr(), den.data_ptr(), stream.cuda_stream

        def loop():
            for j in range(n):
                it.denoise_device(P + 4 * plane * j, A, D + 4 * plane * j, S, settings=settings)

        res = dict(loop_of_denoise=timed(it, loop))
        res["planes_own"] = timed(it, lambda: it.denoise_planes_device(P, n, A, D, "own", stream_ptr=S, settings=settings))
        res["planes_own"]["launches"] = it.stats()["launches"]
        res["planes_shared"] = timed(it, lambda: it.denoise_planes_device(P, n, A, D, "shared", out_guide_ptr=guide.data_ptr(),
                                                                          stream_ptr=S, settings=settings))
        res["planes_shared"]["launches"] = it.stats()["launches"]
        assert bool(torch.isfinite(den).all()) and bool(torch.isfinite(guide).all())
        base = res["loop_of_denoise"]
        for mode in ("planes_own", "planes_shared"):
            res[mode]["loop_over_planes"] = round(base["median_ms"] / res[mode]["median_ms"], 3)
            res[mode]["ok"] = res[mode]["median_ms"] <= base["median_ms"] + (base["max_ms"] - base["min_ms"])
        out["sizes"].setdefault(f"{side}x{side}", {})[f"{n}_planes"] = res
        del planes, den, guide
    it.close()
print(json.dumps(out))
