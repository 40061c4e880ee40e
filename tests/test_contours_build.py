"""Compile-time guards on contours.hip (hipcc cross-compiles without a GPU), from the compiler's kernel resource remarks alone: the
contour kernels use no scratch memory and spill nothing, the LDS form's bit map and point staging stay within kContourLdsBytes plus
the stage, and the tracer exists in exactly two instantiations (the LDS form and the global form)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sbb_textline_detection_amd", "csrc")


def _constant(name):
    text = open(os.path.join(CSRC, "contour_walk.h")).read()
    expr = re.search(r"constexpr int %s = ([0-9 *]+);" % name, text).group(1)
    value = 1
    for factor in expr.split("*"):
        value *= int(factor)
    return value


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_contour_kernels_have_no_scratch_and_two_tracer_forms(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", os.path.join(CSRC, "contours.hip"),
                          "-o", str(tmp_path / "contours.s"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lds_limit, stage_bytes = _constant("kContourLdsBytes"), _constant("kContourStage") * 8
    assert lds_limit == 64 * 1024
    tracers = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        name = b.split()[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        spill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        sgpr_spill = int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        assert scratch == 0 and spill == 0 and sgpr_spill == 0, (name, scratch, spill, sgpr_spill)
        if "contour_trace_kernel" in name:
            tracers[name] = lds
    assert len(tracers) == 2, tracers
    small, large = sorted(tracers.values())
    assert small <= stage_bytes + 16, tracers                       # the global form: the stage only
    assert lds_limit <= large <= lds_limit + stage_bytes, tracers   # the LDS form: bit map + stage; two blocks fit a CU's 160 KiB
    assert 2 * large <= 160 * 1024
