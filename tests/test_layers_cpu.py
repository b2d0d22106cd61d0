"""Path-length layers, the parts that need no GPU: the library's new symbols with the argument
types the Python mirror declares (checked against the header by a C compiler), the longest path a
given rr_depth admits, the layer-mask helper and the command line's refusal of a bad --layers N
before any device is opened."""
import ctypes
import os
import subprocess

import pytest

import bdpt_amd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the header's declarations, as function-pointer types a C compiler checks the entries against
C_TYPES = {
    "bdpt_render_layers": "int (*)(bdpt_ctx*, const bdpt_frame_params*, const bdpt_sample_window*, int32_t, float*, void*)",
    "bdpt_render_layers_host": "int (*)(bdpt_ctx*, const bdpt_frame_params*, const bdpt_sample_window*, int32_t, float*)",
    "bdpt_layers_compose": "int (*)(bdpt_ctx*, const float*, int32_t, int32_t, int32_t, uint64_t, float*, void*)",
}


def test_library_exports_the_layer_entry_points_with_the_mirrored_types(tmp_path):
    L = bdpt_amd.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    fp, wp = ctypes.POINTER(bdpt_amd._FrameParams), ctypes.POINTER(bdpt_amd._SampleWindow)
    want = {
        "bdpt_render_layers": [vp, fp, wp, i32, vp, vp],
        "bdpt_render_layers_host": [vp, fp, wp, i32, vp],
        "bdpt_layers_compose": [vp, vp, i32, i32, i32, ctypes.c_uint64, vp, vp],
    }
    for name, types in want.items():
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == types, name
    # the same shapes in the header: -Werror makes a mismatched pointer type an error
    lines = ['#include "bdpt_amd.h"', "int main(void) {"]
    for k, (name, ctype) in enumerate(C_TYPES.items()):
        lines.append(f"    {ctype.replace('(*)', f'(*f{k})')} = {name};")
        lines.append(f"    (void)f{k};")
    lines += ["    return 0;", "}"]
    src = tmp_path / "layers_decl.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_longest_path_per_strategy():
    f = bdpt_amd.layers_longest_path
    B, LT, PT = bdpt_amd.STRATEGY_BDPT, bdpt_amd.STRATEGY_LIGHT_TRACING, bdpt_amd.STRATEGY_PATH_TRACING
    assert [f(d, B) for d in (1, 2, 3, 5, 8, 28)] == [0, 3, 5, 9, 15, 55]
    assert [f(d, PT) for d in (1, 2, 3, 8)] == [0, 2, 3, 8]
    assert [f(d, LT) for d in (1, 2, 3, 8)] == [1, 2, 3, 8]
    assert f(28, B) + 1 <= 64  # the deepest layered render still fits one layer per length


def test_layer_mask_helper():
    m = bdpt_amd.BDPTIntegrator.layer_mask
    assert m([0]) == 1 and m((1, 3)) == 0b1010 and m(range(2, 6)) == 0b111100 and m(0b101) == 5
    assert m([63]) == 1 << 63 and m([]) == 0
    for bad in ([64], [-1], -1, 1 << 64):
        with pytest.raises(ValueError):
            m(bad)


@pytest.mark.parametrize("n", ["0", "x", "65"])
def test_cli_refuses_a_bad_layer_count_before_any_device(n, tmp_path):
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([cli, str(tmp_path / "missing.toml"), "--layers", n], capture_output=True, text=True, env=env,
                       timeout=60)
    assert r.returncode != 0
    assert "--layers" in r.stderr and "[1, 64]" in r.stderr  # not the missing scene file, not a device error
