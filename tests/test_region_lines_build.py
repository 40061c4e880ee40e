"""Compile-time guards on region_lines.hip (hipcc cross-compiles without a GPU): the morphology, warp and column-sum kernels use no
scratch memory and spill nothing, stay within 128 VGPRs, and the warp kernel reads its per-region tables through the scalar cache."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_region_line_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sbb_textline_detection_amd", "csrc", "region_lines.hip")
    asm = tmp_path / "region_lines.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", str(asm),
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
        body = re.search(r"^%s:.*?\n(.*?)\n\s*s_endpgm" % re.escape(name), text, re.S | re.M).group(1)
        assert scratch == 0 and spill == 0 and sgpr_spill == 0 and "scratch_" not in body, (name, scratch, spill, sgpr_spill)
        assert vgprs <= 128, (name, vgprs)                       # room for four 256-thread blocks per CU
        if "region_line_warp_kernel" in name:
            assert "s_load_dword" in body, "the geometry / inverse-map tables are no longer read through the scalar cache"
            assert "global_atomic" not in body and "ds_add" not in body, "one plain store per row: no atomics"
            assert "v_fma_f64" not in body and "v_mul_f32" not in body, "after the coordinates the warp is integer arithmetic"
        if "region_line_cols_kernel" in name:
            assert "global_atomic" not in body, "the column sums are a plain pass over the stored mask"
        seen.add(name)
    for kernel in ("region_line_morph_kernel", "region_line_warp_kernel", "region_line_cols_kernel"):
        assert any(kernel in n for n in seen), kernel
