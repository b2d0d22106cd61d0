"""Host ingest of bitmap textures (map_Kd / map_Ks, the reference's BitmapTexture3f,
core.h:417-588), no GPU: texel decode against glibc's powf, per-triangle texture
coordinates, agreement of the OBJ and the hand-over ingest paths, the rejected inputs,
the ctypes mirrors of the new structs, and untextured scenes loading exactly as before."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import bdpt_amd
import variants

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEX = os.path.join(REPO, "scenes", "tex")


@pytest.fixture(scope="module")
def texbox():
    return bdpt_amd.Scene(os.path.join(TEX, "texbox.obj"))


def read_ppm(path):
    raw = open(path, "rb").read()
    magic, w, h, maxval = raw.split(None, 4)[:4]
    n = int(w) * int(h) * 3
    return int(w), int(h), int(maxval), np.frombuffer(raw[len(raw) - n:], np.uint8).reshape(int(h), int(w), 3)


def test_texels_are_glibc_powf_of_the_flipped_ppm(texbox):
    """Tex::loadpxm / pf / fl (core.h:430-486): cs = powf(float(byte) / float(maxval), 2.2f), rows
    flipped; bit for bit what libm's powf gives. The maps are non-square, one has maxval 100."""
    libm = ctypes.CDLL("libm.so.6")
    libm.powf.restype = ctypes.c_float
    libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
    maps = texbox.textures()
    # texbox.mtl's order of first use: wall, floor, cube_kd (named .png in the MTL), cube_ks
    for tex, name, size, mv in zip(maps, ["wall", "floor", "cube_kd", "cube_ks"], [(5, 3), (4, 4), (2, 3), (3, 2)],
                                   [255, 100, 255, 255]):
        w, h, maxval, px = read_ppm(os.path.join(TEX, name + ".ppm"))
        assert (w, h, maxval) == size + (mv,)
        assert tex.shape == (h, w, 3)
        want = np.array([libm.powf(np.float32(b) / np.float32(maxval), np.float32(2.2)) for b in px[::-1].ravel()],
                        np.float32).reshape(h, w, 3)
        assert np.array_equal(want.view(np.uint32), tex.view(np.uint32)), name
    info = texbox.texture_info()
    assert info["textures"] == 4 and info["texels"] == 15 + 16 + 6 + 6


def parse_obj_corners(path):
    """(v, vt, [faces: list of (v index, vt index or None)]) with tinyobj's index rule."""
    v, vt, faces = [], [], []
    for ln in open(path):
        t = ln.split()
        if not t:
            continue
        if t[0] == "v":
            v.append([np.float32(x) for x in t[1:4]])
        elif t[0] == "vt":
            vt.append([np.float32(x) for x in t[1:3]])
        elif t[0] == "f":
            face = []
            for c in t[1:]:
                p = c.split("/")
                fix = lambda s, n: int(s) - 1 if int(s) > 0 else n + int(s)
                face.append((fix(p[0], len(v)), fix(p[1], len(vt)) if len(p) > 1 and p[1] else None))
            faces.append(face)
    return np.array(v, np.float32), np.array(vt, np.float32), faces


def test_triangle_texture_coordinates_follow_the_corner_indices(texbox):
    """[triangles][6] = attrib.texcoords of each corner's texcoord_index (core.h:572-577), through
    absolute and relative (negative) `vt` indices; faces without vt carry zeros."""
    v, vt, faces = parse_obj_corners(os.path.join(TEX, "texbox.obj"))
    want = {}
    for face in faces:  # every face is a convex quad: corners (0, 1, 2) and (0, 2, 3)
        for tri in ((0, 1, 2), (0, 2, 3)):
            key = tuple(v[[face[k][0] for k in tri]].ravel().view(np.uint32).tolist())
            st = np.zeros(6, np.float32) if face[0][1] is None else vt[[face[k][1] for k in tri]].ravel()
            want[key] = st
    tf, ti, _, _ = texbox.export()
    st = np.frombuffer(texbox.export_textures("tri_st"), np.float32).reshape(-1, 6)
    assert st.shape[0] == tf.shape[0] == 26
    textured = 0
    for i in range(tf.shape[0]):
        key = tuple(tf[i, :9].view(np.uint32).tolist())
        assert np.array_equal(st[i].view(np.uint32), want[key].view(np.uint32)), i
        textured += bool(st[i].any())
    assert textured == 2 + 2 + 12  # back wall, floor, cube
    assert st.min() < -1.0 and st.max() > 2.0  # the wall's UVs run below -1 and beyond 1
    # and the copy the kernels read rides in slots 6, 7 of the 128-byte shade records
    shade = np.frombuffer(texbox.export_layout("shade"), np.float32).reshape(-1, 8, 4)
    assert np.array_equal(shade[:, 6:8].reshape(-1, 8)[:, :6].view(np.uint32), st.view(np.uint32))


def test_obj_and_handover_ingest_paths_agree(texbox):
    d = texbox.to_desc()
    assert len(d.textures) == 4 and d.texcoords.shape == (26, 6)
    other = bdpt_amd.Scene.from_desc(d)
    for i in range(len(bdpt_amd.LAYOUT_ARRAYS)):
        assert texbox.export_layout(i) == other.export_layout(i), bdpt_amd.LAYOUT_ARRAYS[i]
    for name in bdpt_amd.TEXTURE_ARRAYS:
        a = texbox.export_textures(name)
        assert len(a) > 0 and a == other.export_textures(name), name
    mt = np.frombuffer(texbox.export_textures("mat_tex"), np.int32).reshape(-1, 2)
    assert mt.tolist() == [[0, -1], [1, -1], [2, 3], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]
    # the glossy constants come from the maps' getMax / getAverage (mixture.h:39-46): not the twin's
    rec = np.frombuffer(texbox.export_layout("bsdfs_ingested"), np.float32).reshape(-1, 18)
    twin = np.frombuffer(bdpt_amd.Scene(os.path.join(TEX, "texbox_twin.obj")).export_layout("bsdfs_ingested"),
                         np.float32).reshape(-1, 18)
    assert not np.array_equal(rec[1:3, 16:], twin[1:3, 16:])
    maps = texbox.textures()
    mx = (maps[3].reshape(-1, 3).max(0) + maps[2].reshape(-1, 3).max(0)).max()
    assert rec[2, 16] == np.float32(0.99) * (np.float32(1.0) / mx)


def copy_scene(tmp_path):
    d = tmp_path / "tex"
    shutil.copytree(TEX, d)
    return d


def load_error(path):
    with pytest.raises(bdpt_amd.BdptError) as e:
        bdpt_amd.Scene(str(path))
    return e.value


def test_rejected_inputs(tmp_path, texbox):
    d = copy_scene(tmp_path)
    os.remove(d / "floor.ppm")
    e = load_error(d / "texbox.obj")
    assert e.code == bdpt_amd.ERR_IO and "floor.ppm" in str(e)  # (the reference: a 1 x 1 pink texture)
    d = copy_scene(tmp_path / "short")
    raw = (d / "wall.ppm").read_bytes()
    (d / "wall.ppm").write_bytes(raw[:-1])
    e = load_error(d / "texbox.obj")
    assert e.code == bdpt_amd.ERR_INVALID and "shorter" in str(e)
    for k, header in enumerate([b"P6\n0 3\n255\n", b"P6\n5 3\n256\n", b"P6\n5 3\n0\n", b"P6\n# c\n5 3\n255\n"]):
        d = copy_scene(tmp_path / f"hdr{k}")
        (d / "wall.ppm").write_bytes(header + raw[-45:])
        e = load_error(d / "texbox.obj")
        assert e.code == bdpt_amd.ERR_INVALID and "header" in str(e), header
    d = copy_scene(tmp_path / "novt")  # a face of a textured material without texture coordinates
    obj = (d / "texbox.obj").read_text().replace("f 1/1/1 2/2/1 3/3/1 4/4/1", "f 1//1 2//1 3//1 4//1")
    (d / "texbox.obj").write_text(obj)
    e = load_error(d / "texbox.obj")
    assert e.code == bdpt_amd.ERR_INVALID and "texture coordinates" in str(e)
    # the plain hand-over entry still refuses a textured material
    desc = texbox.to_desc()
    desc.textures = None
    with pytest.raises(bdpt_amd.BdptError) as ei:
        bdpt_amd.Scene.from_desc(desc)
    assert ei.value.code == bdpt_amd.ERR_INVALID and "texture" in str(ei.value)
    desc = texbox.to_desc()
    desc.diffuse_tex = desc.diffuse_tex.copy()
    desc.diffuse_tex[0] = 4
    with pytest.raises(bdpt_amd.BdptError) as ei:
        bdpt_amd.Scene.from_desc(desc)
    assert ei.value.code == bdpt_amd.ERR_INVALID and "out of range" in str(ei.value)


STRUCTS = [("bdpt_texture_desc", bdpt_amd._TextureDesc), ("bdpt_scene_textures", bdpt_amd._SceneTextures)]


def test_texture_struct_mirrors_match_header(tmp_path):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bdpt_amd.h"', "int main(void) {"]
    for cname, mirror in STRUCTS:
        lines.append(f'    printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'    printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.c"), "-o",
                        str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    layout = {}
    for ln in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines():
        cname, key, val = ln.split()
        layout[(cname, key)] = int(val)
    for cname, mirror in STRUCTS:
        assert ctypes.sizeof(mirror) == layout[(cname, "size")], cname
        for fname, _ in mirror._fields_:
            assert getattr(mirror, fname).offset == layout[(cname, fname)], (cname, fname)


# sha256 over the 13 layout arrays (bdpt_scene_export_layout 0..12, concatenated) as the commit
# before bitmap textures loaded these scenes
PARENT_LAYOUT_SHA = {
    "cbox_low": "2c0e9055a84384fd686755a63b704d61aa61c1cc3ea23be3b5703e1278d02392",
    "caustic": "45bed5fe0294302989f9f431ea58fe03d48bc36706e3a31c10c3bd385a78cbc2",
    "hardlight": "54d97f86ea02923c081fe6af844927396503eed4f156c76d702c74ce92a5e917",
    "hardlight_mirror": "b6d846a65f6096b52dbc776475403ca188c4b3ba1595f7aa9fcb17a013cb6afa",
    "hardlight_phong": "31fdaaa484f5f59a89ee8ac4c1c427f3f8a9911cc7ec217a408f579ea8c07625",
    "texbox_twin": "081aee7075e7638f00adea2fc5af499cc1bb98406271e734450d02f10e74ff3f",
}
PARENT_TWIN_SHADE_SHA = "cded555bb242990547bf5f6200f531989e78bb87b4c64ed481598429a4bc455b"


@pytest.mark.parametrize("name", list(PARENT_LAYOUT_SHA))
def test_untextured_scenes_load_as_before(name):
    path = os.path.join(TEX, "texbox_twin.obj") if name == "texbox_twin" else variants.obj_path(name)
    s = bdpt_amd.Scene(path)
    got = hashlib.sha256(b"".join(s.export_layout(i) for i in range(len(bdpt_amd.LAYOUT_ARRAYS)))).hexdigest()
    assert got == PARENT_LAYOUT_SHA[name]
    assert s.texture_info() == dict(textures=0, texels=0, device_bytes=0)
    assert all(s.export_textures(a) == b"" for a in bdpt_amd.TEXTURE_ARRAYS)
    if name == "texbox_twin":
        assert hashlib.sha256(s.export_layout("shade")).hexdigest() == PARENT_TWIN_SHADE_SHA
