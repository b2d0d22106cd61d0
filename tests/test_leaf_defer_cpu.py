"""The device shade records carry what the deferred reference-leaf check reads (bdpt_types.h
kShadeBox, bdpt_capi.cpp device_shade; no GPU): per triangle the six floats of its reference
leaf box, bit for bit lbox[leaf(triangle)], in the record's slots 6 and 7 — or, where a scene
with bitmap textures keeps texture coordinates there, the leaf id in slot 7's last word — and
every word the record held before is what it was: the host's five vectors with the graze code
in the shape word, v0, the texture coordinates.
"""
import os

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import REPO

SHADE_STRIDE, SHADE_V0, SHADE_BOX = 8, 5, 6
TEX_SCENES = ["texbox.obj", "texbox_twin.obj"]
KAT_SCENES = ["bsdf_edges.obj", "emit_edges.obj", "layers_open.obj"]


def scene_paths():
    out = [(name, variants.obj_path(name)) for name in sorted(variants.SCENES) if name != "synth1m"]
    out += [(f, os.path.join(REPO, "scenes", "tex", f)) for f in TEX_SCENES]
    out += [(f, os.path.join(REPO, "scenes", "kat", f)) for f in KAT_SCENES]
    return [(n, p) for n, p in out if p and os.path.exists(p)]


def arrays(sc):
    u32 = lambda name: np.frombuffer(sc.export_layout(name), np.uint32)  # noqa: E731
    tri = u32("tri").reshape(-1, 3, 4)
    shade = np.frombuffer(sc.export_shade_records(), np.uint32).reshape(-1, SHADE_STRIDE, 4)
    # the layout export keeps the records without the leaf-box words: everything else is the same
    old = u32("shade").reshape(-1, SHADE_STRIDE, 4)
    assert np.array_equal(shade[:, :SHADE_BOX], old[:, :SHADE_BOX])
    return tri, shade, u32("wtri").reshape(-1, 3, 4), u32("lbox").reshape(-1, 2, 4)


@pytest.mark.parametrize("name,path", scene_paths(), ids=[n for n, _ in scene_paths()])
def test_shade_records_hold_the_reference_leaf_box(name, path):
    sc = bdpt_amd.Scene(path)
    tri, shade, wtri, lbox = arrays(sc)
    n = tri.shape[0]
    assert shade.shape[0] == wtri.shape[0] == n and n > 0
    # a traversal triangle names its shade record (v0's w) and its reference leaf (e1's w)
    leaf = np.empty(n, np.int64)
    ref = wtri[:, 0, 3].astype(np.int64)
    assert np.array_equal(np.sort(ref), np.arange(n))
    leaf[ref] = wtri[:, 1, 3]
    assert leaf.max() < lbox.shape[0]
    st = np.frombuffer(sc.export_textures("tri_st"), np.uint32)
    if st.size:  # a scene with bitmap textures
        st = st.reshape(n, 6)
        assert np.array_equal(shade[:, SHADE_BOX, :], st[:, 0:4])
        assert np.array_equal(shade[:, SHADE_BOX + 1, 0:2], st[:, 4:6])
        assert np.all(shade[:, SHADE_BOX + 1, 2] == 0)
        assert np.array_equal(shade[:, SHADE_BOX + 1, 3], leaf.astype(np.uint32))
    else:
        assert np.array_equal(shade[:, SHADE_BOX, :], lbox[leaf, 0, :])
        assert np.array_equal(shade[:, SHADE_BOX + 1, :], lbox[leaf, 1, :])
        assert np.all(shade[:, SHADE_BOX:, 3] == 0)  # (lo, 0) (hi, 0), as lbox holds them


@pytest.mark.parametrize("name,path", scene_paths(), ids=[n for n, _ in scene_paths()])
def test_shade_records_keep_their_earlier_words(name, path):
    """Slots 0..5 against what they are built from: the normals and ids of the host's triangles in
    leaf order (bdpt_scene_export), v1, v2 and v0; the graze code only in the shape word's top byte."""
    sc = bdpt_amd.Scene(path)
    tri, shade, _, _ = arrays(sc)
    n = tri.shape[0]
    tri_f32, tri_i32 = sc.export()[:2]
    pos = np.asarray(tri_f32, np.float32).reshape(n, 18)[:, :9].reshape(n, 3, 3).view(np.uint32)
    nrm = np.asarray(tri_f32, np.float32).reshape(n, 18)[:, 9:].reshape(n, 3, 3).view(np.uint32)
    ids = np.asarray(tri_i32, np.int32).reshape(n, 3)  # shape, prim, mat
    assert np.array_equal(shade[:, 0:3, 0:3], nrm)
    assert np.array_equal(shade[:, 0, 3].view(np.int32), ids[:, 2])
    assert np.array_equal((shade[:, 1, 3] & 0xFFFFFF).view(np.int32), ids[:, 0])
    assert np.array_equal(shade[:, 2, 3].view(np.int32), ids[:, 1])
    assert np.array_equal(shade[:, 3, 0:3], pos[:, 1]) and np.array_equal(shade[:, 4, 0:3], pos[:, 2])
    assert np.array_equal(shade[:, SHADE_V0, 0:3], pos[:, 0]) and np.array_equal(shade[:, SHADE_V0, :], tri[:, 0, :])
    assert np.all(shade[:, 3:6, 3] == 0)
