"""CPU-side checks of the getter that tells the two "bdpt_frame_kernel" builds apart
(bdpt_last_kernel_glossy; the build without glossy lobes is bdpt_kernels_ng.hip).
A context needs a device, so what stats() reports on a fresh one is checked in
tests/test_gpu_ng_build.py; here: the export, its declaration, its value without a
context, and that the wrapper reads it into stats() and hashes the new unit."""
import ctypes
import inspect
import os
import re

import bdpt_amd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_getter():
    L = bdpt_amd.lib()
    assert hasattr(L, "bdpt_last_kernel_glossy")
    assert L.bdpt_last_kernel_glossy(ctypes.c_void_p(None)) == 1  # as before the first render: the full build


def test_header_declares_the_getter():
    with open(os.path.join(REPO, "include", "bdpt_amd.h")) as f:
        text = f.read()
    assert re.search(r"^int\s+bdpt_last_kernel_glossy\s*\(\s*const\s+bdpt_ctx\s*\*\s*ctx\s*\)\s*;", text, re.M)


def test_wrapper_reports_the_key_and_hashes_the_unit():
    assert "kernel_glossy" in inspect.getsource(bdpt_amd.BDPTIntegrator.stats)
    assert "csrc/bdpt_kernels_ng.hip" in bdpt_amd.KERNEL_SOURCES
    assert os.path.exists(os.path.join(os.path.dirname(bdpt_amd.__file__), "csrc", "bdpt_kernels_ng.hip"))
