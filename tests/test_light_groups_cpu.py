"""Light groups, the parts that need no GPU: Scene.emitters() against the scene's MTL, the
relight definition against a float64 sum, the library's new symbols with the argument types the
Python mirror declares (checked against the header by a C compiler), and the command line's
refusal of --light-groups on a path scene before any device is opened."""
import ctypes
import os
import re
import subprocess

import numpy as np

import bdpt_amd
import variants

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the header's declarations, as function-pointer types a C compiler checks the entries against
C_TYPES = {
    "bdpt_scene_emitter_count": "int (*)(const bdpt_scene*, int32_t*)",
    "bdpt_scene_get_emitter": "int (*)(const bdpt_scene*, int32_t, bdpt_emitter_info*)",
    "bdpt_render_light_groups": "int (*)(bdpt_ctx*, const bdpt_frame_params*, const bdpt_sample_window*, int32_t, "
                                "const int32_t*, float*, void*)",
    "bdpt_render_light_groups_host": "int (*)(bdpt_ctx*, const bdpt_frame_params*, const bdpt_sample_window*, int32_t, "
                                     "const int32_t*, float*)",
    "bdpt_light_groups_relight": "int (*)(bdpt_ctx*, const float*, int32_t, int32_t, int32_t, const float*, float*, void*)",
}


def mtl_materials(obj):
    """[(name, Ke)] of the OBJ's MTL in file order (the material indices of the scene)."""
    with open(os.path.splitext(obj)[0] + ".mtl") as f:
        text = f.read()
    out = []
    for block in re.split(r"^\s*newmtl\s+", text, flags=re.M)[1:]:
        ke = re.search(r"^\s*Ke\s+(\S+)\s+(\S+)\s+(\S+)", block, re.M)
        out.append((block.split()[0], tuple(float(x) for x in ke.groups())))
    return out


def test_scene_emitters_match_the_mtl():
    obj = variants.obj_path("emit_edges")
    em = bdpt_amd.Scene(obj).emitters()
    mats = mtl_materials(obj)
    assert len(em) == 5 == bdpt_amd.Scene(obj).info()["emitters"]
    # file order = emitter index (the comment at the top of emit_edges.obj)
    assert [mats[e["material"]][0] for e in em] == ["lightSingle", "lightFan33", "lightCurved", "lightZeroFace", "lightQuad"]
    for e in em:
        assert e["radiance"] == mats[e["material"]][1] and any(e["radiance"])
        assert e["area"] > 0 and e["shape"] >= 0
    assert len({e["shape"] for e in em}) == 5
    one = bdpt_amd.Scene(variants.obj_path("cbox_low")).emitters()
    assert len(one) == 1
    info = bdpt_amd._EmitterInfo()
    L = bdpt_amd.lib()
    s = bdpt_amd.Scene(obj)
    for bad in (-1, 5):
        assert L.bdpt_scene_get_emitter(s._h, bad, ctypes.byref(info)) == bdpt_amd.ERR_INVALID


def test_relight_definition_against_a_float64_sum():
    """The float32 loop of include/bdpt_amd.h (what tests/test_gpu_light_groups.py holds the
    kernel to, bit for bit) against the exact sum: n products and n - 1 sums, each within half an
    ulp of its own result, so the error is at most (2 n - 1) * 2^-24 of sum |gain * plane|."""
    rng = np.random.default_rng(7)
    n = 5
    planes = rng.uniform(0.0, 4.0, (n, 8, 8, 3)).astype(np.float32)
    gains = rng.uniform(-2.0, 3.0, (n, 3)).astype(np.float32)
    gains[2] = 0.0
    acc = gains[0][None, None, :] * planes[0]
    for g in range(1, n):
        acc = acc + gains[g][None, None, :] * planes[g]
    assert acc.dtype == np.float32
    exact = (gains.astype(np.float64)[:, None, None, :] * planes.astype(np.float64)).sum(axis=0)
    scale = np.abs(gains.astype(np.float64)[:, None, None, :] * planes.astype(np.float64)).sum(axis=0)
    assert (np.abs(acc.astype(np.float64) - exact) <= (2 * n - 1) * 2.0 ** -24 * scale).all()


def test_library_exports_the_light_group_entry_points_with_the_mirrored_types(tmp_path):
    L = bdpt_amd.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    fp, wp = ctypes.POINTER(bdpt_amd._FrameParams), ctypes.POINTER(bdpt_amd._SampleWindow)
    want = {
        "bdpt_scene_emitter_count": [vp, ctypes.POINTER(i32)],
        "bdpt_scene_get_emitter": [vp, i32, ctypes.POINTER(bdpt_amd._EmitterInfo)],
        "bdpt_render_light_groups": [vp, fp, wp, i32, vp, vp, vp],
        "bdpt_render_light_groups_host": [vp, fp, wp, i32, vp, vp],
        "bdpt_light_groups_relight": [vp, vp, i32, i32, i32, vp, vp, vp],
    }
    for name, types in want.items():
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == types, name
    # the same shapes in the header (-Werror makes a mismatched pointer type an error), then the
    # emitter record's layout against its ctypes mirror
    lines = ['#include "bdpt_amd.h"', "int main(void) {"]
    for k, (name, ctype) in enumerate(C_TYPES.items()):
        lines.append(f"    {ctype.replace('(*)', f'(*f{k})')} = {name};")
        lines.append(f"    (void)f{k};")
    lines += ["    return 0;", "}"]
    src = tmp_path / "groups_decl.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bdpt_amd.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(bdpt_emitter_info));']
    for fname, _ in bdpt_amd._EmitterInfo._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(bdpt_emitter_info, {fname}));')
    lines += ["    return 0;", "}"]
    src = tmp_path / "emitter_info.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "emitter_info"
    r = subprocess.run(["gcc", "-std=c11", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(bdpt_amd._EmitterInfo)
    for fname, _ in bdpt_amd._EmitterInfo._fields_:
        assert int(got[fname]) == getattr(bdpt_amd._EmitterInfo, fname).offset, fname


def test_cli_refuses_light_groups_on_a_path_scene_before_any_device(tmp_path):
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    toml = tmp_path / "path.toml"
    toml.write_text(variants.path_toml_text("emit_edges", 16, 16, 1))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([cli, str(toml), "--light-groups"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode != 0
    assert "--light-groups" in r.stderr and "path" in r.stderr  # not a device error
    assert os.listdir(tmp_path) == ["path.toml"]
