"""Compile-time guards on line_extent.hip (hipcc cross-compiles without a GPU): the kernels of the text-line x extents use no scratch memory
and spill nothing; the border scan's LDS stays within the limit csrc/line_extent.h states (three bit maps of at most 60 KB together, plus
the stage of kept points) and the other kernels use none; and the float64 arithmetic of the inside test is NOT contracted to FMAs -- the
signs it takes do not depend on it, but the header promises OpenCV's operation order."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_extent_kernels_have_no_scratch_and_bounded_lds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sbb_textline_detection_amd", "csrc", "line_extent.hip")
    asm = tmp_path / "line_extent.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip", src, "-o", str(asm),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = asm.read_text()
    seen = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        name = b.split()[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        spill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        sgpr_spill = int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
        vgprs = int(re.search(r" VGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        body = re.search(r"^%s:.*?\n(.*?)\n\s*s_endpgm" % re.escape(name), text, re.S | re.M).group(1)
        assert scratch == 0 and spill == 0 and sgpr_spill == 0 and "scratch_" not in body, (name, scratch, spill, sgpr_spill)
        assert vgprs <= 128, (name, vgprs)
        # (the warp kernel's only v_fmac_f64 is the exact hi / lo split of llrint's float64 -> int64 conversion, as in region_lines.hip)
        assert "v_fma_f64" not in body and ("extent_lines_kernel" not in name or "v_fmac_f64" not in body), "%s: float64 arithmetic was contracted" % name
        assert "atomic" not in body, "%s: the tables must come out bit-identical from run to run" % name
        seen[name] = lds
    by_kernel = {}
    for kernel in ("extent_fill_kernel", "extent_warp_kernel", "extent_scan_kernel", "extent_lines_kernel"):
        by_kernel[kernel] = [lds for n, lds in seen.items() if kernel in n]
    assert [len(v) for v in by_kernel.values()] == [1, 1, 2, 1], seen
    assert by_kernel["extent_fill_kernel"] == [0] and by_kernel["extent_warp_kernel"] == [0] and by_kernel["extent_lines_kernel"] == [0]
    stage = 64 * 8                                                   # kContourStage kept points of two ints
    assert sorted(by_kernel["extent_scan_kernel"]) == [stage, 60 * 1024 + stage], by_kernel      # the global form, the LDS form
