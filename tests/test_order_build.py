"""Compile-time guards on order.hip (hipcc cross-compiles without a GPU): the reading-order kernels use no scratch memory and spill
nothing, within the register and LDS bounds of the line-split kernels, and their float64 arithmetic is NOT contracted to FMAs -- scipy and
numpy round every multiply and every add, and the kernels have to give the same bits (csrc/order.h)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_order_kernels_have_no_scratch_and_no_fma(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sbb_textline_detection_amd", "csrc", "order.hip")
    asm = tmp_path / "order.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip", src, "-o", str(asm),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = asm.read_text()
    seen = set()
    for b in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        name = b.split()[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        spill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        sgpr_spill = int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
        vgprs = int(re.search(r" VGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        body = re.search(r"^%s:.*?\n(.*?)\n\s*s_endpgm" % re.escape(name), text, re.S | re.M).group(1)
        assert scratch == 0 and spill == 0 and sgpr_spill == 0 and "scratch_" not in body, (name, scratch, spill, sgpr_spill)
        assert vgprs <= 128 and lds <= 64 * 1024, (name, vgprs, lds)
        assert "v_fma_f64" not in body and "v_fmac_f64" not in body, "%s: float64 arithmetic was contracted (or a divide sequence crept in)" % name
        seen.add(name)
    for kernel in ("row_sums_kernel", "order_edges_kernel", "contour_moments_kernel", "order_rank_kernel"):
        assert sum(1 for n in seen if kernel in n) == 1, (kernel, seen)
