"""Generates the bitmap-texture fixtures (tex_*.npz, tex_manifest.json) from the
UNMODIFIED reference, as make_goldens.py does for the untextured scenes:

    make -C oracle/ref            # builds oracle/_ref/ref_bdpt{,_lt,_pt}
    python tests/golden/make_tex_goldens.py

Frames of scenes/tex/texbox.obj (48x48, spp 8) from the reference's BDPT, light-tracing
and path-tracing builds, one at rrDepth 2, the untextured twin's BDPT frame, and
`sample_state` records (Integrator::render(ray, sampler)) whose rays hit the textured
surfaces. The generator checks that the maps are in view: at least 25 % of the pixels
differ between the textured and the twin frame by more than 1e-2 relative L2.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "scenes", "tex"))
sys.path.insert(0, HERE)
import make_scene  # noqa: E402
from make_kat_goldens import states  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref", "ref_bdpt")
REF_STRATEGY = {"bdpt": REF, "lt": REF + "_lt", "pt": REF + "_pt"}
CAMERA = make_scene.CAMERA
W = H = 48
SPP = 8

# name: (obj, rrDepth, strategy)
FRAMES = {
    "tex_T1_texbox_bdpt": ("texbox.obj", 5, "bdpt"),
    "tex_T2_texbox_lt": ("texbox.obj", 5, "lt"),
    "tex_T3_texbox_pt": ("texbox.obj", 5, "pt"),
    "tex_T4_texbox_bdpt_rr2": ("texbox.obj", 2, "bdpt"),
    "tex_T5_twin_bdpt": ("texbox_twin.obj", 5, "bdpt"),
}


def toml_text(obj: str, rr: int) -> str:
    f3 = lambda v: "[ " + ", ".join(repr(float(x)) for x in v) + " ]"
    return (f'[input]\nobjfile = "{os.path.join(REPO, "scenes", "tex", obj)}"\n\n[camera]\neye = {f3(CAMERA["eye"])}\n'
            f'at = {f3(CAMERA["at"])}\nup = {f3(CAMERA["up"])}\nfov = {float(CAMERA["fov"])!r}\n\n[film]\n'
            f'width = {W}\nheight = {H}\n\n[renderer]\nrealtime = false\ntype = "bdpt"\nrrDepth = {rr}\n'
            f'rrProb = 0.95\nspp = {SPP}\n')


def rel_l2(a, b):
    a = a.reshape(-1, 3).astype(np.float64)
    b = b.reshape(-1, 3).astype(np.float64)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-8)


def main() -> None:
    tmp = tempfile.mkdtemp()
    manifest = {"generator": "oracle/_ref/ref_bdpt{,_lt,_pt} on scenes/tex (tests/golden/make_tex_goldens.py)",
                "camera": {k: list(v) if isinstance(v, tuple) else v for k, v in CAMERA.items()},
                "frames": {}}
    frames = {}
    for name, (obj, rr, strategy) in FRAMES.items():
        toml = os.path.join(tmp, name + ".toml")
        with open(toml, "w") as f:
            f.write(toml_text(obj, rr))
        out = os.path.join(tmp, name + ".f32")
        r = subprocess.run([REF_STRATEGY[strategy], "render", toml, str(W), str(H), str(SPP), "--rr", str(rr), "--out", out],
                           capture_output=True, text=True, check=True)
        assert "Err loading texture" not in r.stdout, r.stdout
        fb = np.fromfile(out, np.float32)
        frames[name] = fb
        np.savez_compressed(os.path.join(HERE, name + ".npz"), fb=fb)
        manifest["frames"][name] = dict(obj=obj, width=W, height=H, spp=SPP, rr_depth=rr, strategy=strategy,
                                        sha256=hashlib.sha256(fb.tobytes()).hexdigest(),
                                        mean_rgb=[float(x) for x in fb.reshape(-1, 3).mean(0)])
        print(name, manifest["frames"][name]["mean_rgb"])
    differ = float((rel_l2(frames["tex_T1_texbox_bdpt"], frames["tex_T5_twin_bdpt"]) > 1e-2).mean())
    print("pixels that differ between the textured and the twin frame:", differ)
    assert differ >= 0.25, "the maps are not in view: move the camera"
    manifest["textured_vs_twin_differing_pixels"] = differ

    # sampler records: rays from the eye to points on the back wall, the floor and the cube
    n, rr = 64, 5
    rng = np.random.default_rng(77)
    eye = np.array(CAMERA["eye"], np.float32)
    tgt = np.concatenate([
        np.stack([rng.uniform(-1.9, 1.9, 24), rng.uniform(-1.9, 1.9, 24), np.full(24, -2.0)], 1),  # back wall
        np.stack([rng.uniform(-1.9, 1.9, 20), np.full(20, -2.0), rng.uniform(-1.9, 2.0, 20)], 1),  # floor
        np.stack([rng.uniform(-0.8, 0.2, 20), rng.uniform(-1.9, -0.7, 20), rng.uniform(-0.9, 0.1, 20)], 1),  # cube
    ])
    d = tgt - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.repeat(eye[None], n, 0), d, np.ones((n, 1)), np.full((n, 1), 1000.0)], 1).astype(np.float32)
    st = states(rng, n)
    rec = np.concatenate([rays, st.view(np.float32)], 1)
    fin, fout = os.path.join(tmp, "sampler.in"), os.path.join(tmp, "sampler.out")
    rec.astype(np.float32).tofile(fin)
    toml = os.path.join(tmp, "sampler.toml")
    with open(toml, "w") as f:
        f.write(toml_text("texbox.obj", rr))
    subprocess.run([REF, "sample_state", toml, str(W), str(H), str(SPP), str(rr), fin, fout, "-"], check=True,
                   capture_output=True)
    out = np.fromfile(fout, np.float32).reshape(n, 3 + 625 + 1 + 64)
    np.savez_compressed(os.path.join(HERE, "tex_kat_sampler_bdpt_texbox.npz"), rays=rays, state_in=st, Li=out[:, :3],
                        state_out=out[:, 3:628].view(np.uint32), nsplat=out[:, 628].view(np.int32),
                        splats=out[:, 629:].reshape(n, 16, 4), width=W, height=H, spp=SPP, rr=rr)
    print("sampler records", n, "splat counts", np.bincount(out[:, 628].view(np.int32)),
          "non-zero Li", int((out[:, :3] != 0).any(1).sum()))
    with open(os.path.join(HERE, "tex_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
