"""Sample windows, the parts that need no GPU: the ctypes mirror of bdpt_sample_window
against the header (as tests/test_abi_layout_cpu.py checks the other structs), the
sample shards of bdpt_dist, SampleWindow's own arithmetic, and the command line's
refusal of a malformed or out-of-range --sample-window before any device is used."""
import ctypes
import os
import subprocess

import pytest

import bdpt_amd
import bdpt_dist
from bdpt_amd import SampleWindow

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_window_ctypes_mirror_matches_header(tmp_path):
    mirror = bdpt_amd._SampleWindow
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bdpt_amd.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(bdpt_sample_window));']
    for fname, _ in mirror._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(bdpt_sample_window, {fname}));')
    # the sharding modes MultiDeviceRenderer passes, and the untouched frame parameters
    lines.append('    printf("rows %d\\nsamples %d\\n", BDPT_SHARD_ROWS, BDPT_SHARD_SAMPLES);')
    lines.append('    printf("frame_params %zu\\n", sizeof(bdpt_frame_params));')
    lines += ["    return 0;", "}"]
    src = tmp_path / "window_layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "window_layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    layout = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert [f for f, _ in mirror._fields_] == ["first", "stride", "count"]
    assert ctypes.sizeof(mirror) == layout["size"] == 12
    for fname, _ in mirror._fields_:
        assert getattr(mirror, fname).offset == layout[fname], fname
    assert bdpt_amd.MultiDeviceRenderer.SHARDING == {"rows": layout["rows"], "samples": layout["samples"]}
    assert ctypes.sizeof(bdpt_amd._FrameParams) == layout["frame_params"]
    w = SampleWindow(3, 5, 7).c()
    assert (w.first, w.stride, w.count) == (3, 5, 7)


def test_sample_shards_partition_the_samples():
    for world in range(1, 10):
        for spp in range(1, 21):
            wins = [bdpt_dist.sample_shard(r, world, spp) for r in range(world)]
            assert all(isinstance(w, SampleWindow) for w in wins)
            assert sorted(k for w in wins for k in w.samples()) == list(range(spp)), (world, spp)
            for r, w in enumerate(wins):
                assert (w.first, w.stride) == (r, world)
                assert w.count == len(range(r, spp, world))  # ceil((spp - r) / world), clipped at 0
                assert w.count == 0 or w.first + (w.count - 1) * w.stride < spp
            assert max(w.count for w in wins) - min(w.count for w in wins) <= 1  # balanced
    for bad in [(2, 2, 8), (-1, 2, 8), (0, 0, 8), (0, 1, 0)]:
        with pytest.raises(ValueError):
            bdpt_dist.sample_shard(*bad)


def test_sample_window_parse_applies_the_abi_rule():
    assert SampleWindow.parse("1:3:3", spp=8) == SampleWindow(1, 3, 3)
    assert SampleWindow.parse("7:9:1", spp=8) == SampleWindow(7, 9, 1)
    assert SampleWindow.parse("40:1:0", spp=8).count == 0  # an empty window is valid anywhere
    assert list(SampleWindow(1, 3, 3).samples()) == [1, 4, 7]
    for text, word in [("3:0:1", "stride"), ("a:b", "first:stride:count"), ("0:1:99", "count"), ("-1:1:1", "first"),
                       ("0:1:-1", "count"), ("1:3:4", "count"), ("1:2:x", "integers"), ("1:2:3:4", "first:stride:count")]:
        with pytest.raises(ValueError, match=word):
            SampleWindow.parse(text, spp=8)


@pytest.mark.parametrize("window,word", [("3:0:1", "stride"), ("a:b", "first:stride:count"), ("0:1:99", "count")])
def test_cli_rejects_a_bad_sample_window_before_any_device(window, word, tmp_path):
    """spp 8; the CLI names the fault and exits non-zero having neither loaded the scene
    nor created a context (no device is needed to get this far, and no image is written)."""
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    out = tmp_path / "never.exr"
    toml = os.path.join(REPO, "scenes", "cbox", "cbox_low_bdpt.toml")
    r = subprocess.run([cli, toml, "nogui", "--width", "8", "--height", "8", "--spp", "8", "--out", str(out),
                        "--sample-window", window], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--sample-window" in r.stderr and word in r.stderr, r.stderr
    assert "bdpt_ctx_create" not in r.stderr and "Scene::load" not in r.stderr and "Render took" not in r.stdout
    assert not out.exists()


def test_cli_rejects_misplaced_window_and_shard_options(tmp_path):
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    toml = os.path.join(REPO, "scenes", "cbox", "cbox_low_bdpt.toml")
    for extra, word in [(["--shard", "pixels", "--gpus", "2"], "--shard"), (["--shard", "samples"], "multi-device"),
                        (["--sample-window", "0:1:1", "--gpus", "2"], "one device")]:
        r = subprocess.run([cli, toml, "--out", str(tmp_path / "never.exr")] + extra, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
