"""Cost of temporal accumulation: kernel_ms of bdpt_reproject on device buffers of a 1-spp Caustic frame
(camera moved sideways by 1 % between the two frames), with and without the neighbourhood clamp, next to one
iteration and a default call of bdpt_denoise on the same buffers and the frame render they serve, in one
process; one JSON line per size. Each figure is the median of --repeat timed calls after a
warm-up call.

    python tools/temporal_cost.py [--sizes 512,1024] [--repeat 9]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("bidirectional-path-tracing_amd", "scenes"):
    sys.path.insert(0, os.path.join(REPO, sub))
import torch  # noqa: E402  (the HIP runtime both bind to, as tests/conftest.py)

import bdpt_amd  # noqa: E402
import variants  # noqa: E402


def median_ms(it, call, repeat):
    ms = []
    for k in range(repeat + 1):  # the first call warms up
        call()
        it.synchronize()
        if k:
            ms.append(it.stats()["kernel_ms"])
    return statistics.median(ms)


def measure(size, repeat):
    sc = variants.SCENES["caustic"]
    cam = bdpt_amd.Camera(**sc["camera"])
    eye, at = cam.eye, cam.at
    shift = 0.01 * sum((a - e) ** 2 for a, e in zip(at, eye)) ** 0.5  # sideways: +x for the Cornell box camera
    cam_b = bdpt_amd.Camera(eye=(eye[0] + shift, eye[1], eye[2]), at=(at[0] + shift, at[1], at[2]), up=cam.up, fov=cam.fov)
    cfg = bdpt_amd.Config(camera=cam, width=size, height=size, spp=1, rr_depth=sc["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path("caustic")), cfg)
    dev = "cuda:0"
    buf = lambda c: torch.zeros(size, size, c, device=dev)  # noqa: E731
    rgb, aov, hist_a, hist_b, out, den = buf(3), buf(8), buf(8), buf(8), buf(3), buf(3)

    def render():  # (torch's stream and the context's are not ordered against each other: wait in between)
        it.synchronize()
        rgb.zero_()
        torch.cuda.synchronize()
        it.render_device(rgb.data_ptr())

    frame_ms = median_ms(it, render, repeat)
    it.render_aov_device(aov.data_ptr())
    it.reproject_device(cam, rgb.data_ptr(), aov.data_ptr(), 0, out.data_ptr(), hist_a.data_ptr(), cur_samples=1)
    cfg.camera = cam_b
    it.synchronize()
    aov.zero_()
    render()
    it.render_aov_device(aov.data_ptr())
    res = dict(size=size, frame_1spp_ms=round(frame_ms, 4))
    for name, s in (("reproject_ms", bdpt_amd.ReprojectSettings()),
                    ("reproject_noclamp_ms", bdpt_amd.ReprojectSettings(clamp_sigma=0.0))):
        res[name] = round(median_ms(it, lambda: it.reproject_device(cam, rgb.data_ptr(), aov.data_ptr(), hist_a.data_ptr(),
                                                                    out.data_ptr(), hist_b.data_ptr(), cur_samples=1,
                                                                    settings=s), repeat), 4)
    it.synchronize()
    res["with_history"] = round(float((hist_b[..., 3] > 1).float().mean().item()), 3)
    for name, iters in (("denoise_1iter_ms", 1), ("denoise_default_ms", bdpt_amd.DenoiseSettings().iterations)):
        d = bdpt_amd.DenoiseSettings(iterations=iters)
        res[name] = round(median_ms(it, lambda: it.denoise_device(out.data_ptr(), aov.data_ptr(), den.data_ptr(), settings=d),
                                    repeat), 4)
    # (a 1-iteration call is the prepare launch plus one a-trous launch)
    it.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--repeat", type=int, default=9)
    a = ap.parse_args()
    for size in (int(s) for s in a.sizes.split(",")):
        print(json.dumps(measure(size, a.repeat)), flush=True)


if __name__ == "__main__":
    main()
