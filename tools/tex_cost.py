"""Cost of the textured megakernel: renders scenes/tex/texbox.obj (bdpt_frame_kernel_tex)
and its untextured twin (the default bdpt_frame_kernel, the yardstick) at 512x512x64 and
prints both rates and their ratio as one JSON line.

    python tools/tex_cost.py [--size 512] [--spp 64] [--repeat 3]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bidirectional-path-tracing_amd"))
sys.path.insert(0, os.path.join(REPO, "scenes", "tex"))
import torch  # noqa: E402,F401  (the HIP runtime both bind to, as tests/conftest.py)

import bdpt_amd  # noqa: E402
import make_scene  # noqa: E402


def rate(obj, size, spp, repeat):
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**make_scene.CAMERA), width=size, height=size, spp=spp, rr_depth=5)
    best, kernel = 0.0, ""
    for _ in range(repeat + 1):  # the first render warms up
        it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(os.path.join(REPO, "scenes", "tex", obj)), cfg)
        it.init()
        it.render_frame()
        st = it.stats()
        kernel = st["kernel"]
        if _ > 0:
            best = max(best, size * size * spp / (st["kernel_ms"] * 1e3))
        it.close()
    return best, kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    tex, ktex = rate("texbox.obj", a.size, a.spp, a.repeat)
    twin, ktwin = rate("texbox_twin.obj", a.size, a.spp, a.repeat)
    print(json.dumps(dict(size=a.size, spp=a.spp, textured_msamples_s=round(tex, 2), textured_kernel=ktex,
                          twin_msamples_s=round(twin, 2), twin_kernel=ktwin, ratio=round(tex / twin, 3))))


if __name__ == "__main__":
    main()
