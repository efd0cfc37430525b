"""The layer the passes over a finished mesh share (mc33_c_library_amd/csrc/mc33_mesh.hip.h), the part that needs no
GPU: its kernels in the gfx950 code object of every sample type, and its place in the translation unit and in both builds.

MESH_KERNELS (tests/mesh_checks.py) is the one list of the shared kernels.  The tests of the parts that launch them (test_measure_cpu.py,
test_topology_cpu.py, test_filter_cpu.py, test_smooth_cpu.py, test_simplify_cpu.py, test_clip_cpu.py) take the names their entry
points launch from it through launched(), beside the kernels of their own.  On the device the layer is held to the oracles by
the GPU tests of those parts and by tests/test_gpu_mesh_scratch.py."""
import os

import pytest

from mesh_checks import MESH_KERNELS, assert_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_shared_kernels_are_in_the_code_object(dtype):
    assert_kernels(dtype, MESH_KERNELS)  # (at most 64 registers: eight waves per SIMD)


def test_the_part_is_built_and_included_before_the_parts_that_use_it():
    from mc33_c_library_amd import build
    assert "mc33_mesh.hip.h" in build.HIP_HEADERS
    assert " mc33_mesh.hip.h" in open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "Makefile")).read()
    kernels = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_kernels.hip")).read()
    assert '#include "mc33_property.hip.h"\n#include "mc33_mesh.hip.h"\n#include "mc33_measure.hip.h"\n' in kernels and "k_mesh_" in kernels
