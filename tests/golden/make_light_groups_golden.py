#!/usr/bin/env python3
"""The relit frames tests/test_gpu_light_groups.py holds the light-group planes to. Run by hand
after build() (it needs the reference binaries oracle/_ref/ref_bdpt, ref_bdpt_lt, ref_bdpt_pt):

    python tests/golden/make_light_groups_golden.py

scenes/kat/emit_edges (five emitters) with every emitter material's Ke multiplied per channel by
a gain, rendered by the reference at 32 x 32 x 4 spp, rrDepth 5, with each of the three
strategies. The gains are distinct per emitter and channel-wise from {0.25, 0.5, 1, 2, 3, 4}, so
the shipped integer Ke values scale to exactly representable floats and "%.9g" writes them
exactly; none is zero (a black material is no emitter: the reference's scene would lose it and
selectEmitter would change). The patched MTL goes to a scratch directory; the output,
light_groups_emit_edges_relit.npz, holds the three frames, the gains and each gain's material
name. Nothing is written to the manifest."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "scenes"))
import variants  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref", "ref_bdpt")
REF_STRATEGY = {"bdpt": REF, "lt": REF + "_lt", "pt": REF + "_pt"}
SCENE, W, H, SPP, RR = "emit_edges", 32, 32, 4, 5
# material -> per-channel gain (R, G, B)
GAINS = {
    "lightSingle": (0.25, 2.0, 1.0),
    "lightFan33": (3.0, 0.5, 0.25),
    "lightCurved": (0.5, 1.0, 4.0),
    "lightZeroFace": (2.0, 0.25, 3.0),
    "lightQuad": (1.0, 4.0, 0.5),
}


def patched_mtl(text):
    """The MTL with every GAINS material's Ke scaled (float32 products, printed exactly)."""
    out, cur, seen = [], None, {}
    for line in text.splitlines():
        m = re.match(r"\s*newmtl\s+(.*)$", line)
        if m:
            cur = m.group(1).strip()
        f = line.split()
        if cur in GAINS and f and f[0] == "Ke":
            ke = np.float32([float(x) for x in f[1:4]])
            scaled = ke * np.float32(GAINS[cur])
            assert scaled.dtype == np.float32 and (scaled > 0).all()
            assert (scaled.astype(np.float64) == ke.astype(np.float64) * np.float64(GAINS[cur])).all(), "not exact"
            line = "Ke " + " ".join("%.9g" % x for x in scaled)
            seen[cur] = scaled
            print(f"{cur}: Ke {' '.join('%.9g' % x for x in ke)} -> {line[3:]}")
        out.append(line)
    assert set(seen) == set(GAINS), sorted(set(GAINS) - set(seen))
    return "\n".join(out) + "\n"


def main():
    assert len({g for g in GAINS.values()}) == len(GAINS)
    assert all(x in (0.25, 0.5, 1.0, 2.0, 3.0, 4.0) for g in GAINS.values() for x in g)
    src = variants.obj_path(SCENE)
    tmp = tempfile.mkdtemp()
    try:
        obj = os.path.join(tmp, os.path.basename(src))
        shutil.copyfile(src, obj)
        with open(src) as f:
            mtllib = re.search(r"^mtllib\s+(\S+)", f.read(), re.M).group(1)
        with open(os.path.join(os.path.dirname(src), mtllib)) as f:
            text = patched_mtl(f.read())
        with open(os.path.join(tmp, mtllib), "w") as f:
            f.write(text)
        toml = os.path.join(tmp, "relit.toml")
        with open(toml, "w") as f:
            f.write(variants.toml_text(SCENE, W, H, SPP, RR).replace(src, obj))
        frames = {}
        for strategy, ref in REF_STRATEGY.items():
            out = os.path.join(tmp, strategy + ".f32")
            r = subprocess.run([ref, "render", toml, str(W), str(H), str(SPP), "--rr", str(RR), "--out", out],
                               capture_output=True, text=True, check=True)
            info = json.loads(r.stdout.strip().splitlines()[-1])
            assert info["samples"] == W * H * SPP, info
            frames[strategy] = np.fromfile(out, np.float32).reshape(H, W, 3)
            print(strategy, info, "mean rgb", frames[strategy].reshape(-1, 3).mean(0))
        names = sorted(GAINS)
        np.savez_compressed(os.path.join(HERE, "light_groups_emit_edges_relit.npz"),
                            bdpt=frames["bdpt"], lt=frames["lt"], pt=frames["pt"],
                            materials=np.array(names), gains=np.float32([GAINS[n] for n in names]),
                            shape=np.int32([W, H, SPP, RR]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
