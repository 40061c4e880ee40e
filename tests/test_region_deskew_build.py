"""Compile-time guards on region_deskew.hip (hipcc cross-compiles without a GPU): the batched rotate-and-project kernel and the crop /
erode kernel use no scratch memory and spill nothing, and the per-region tables are read through the scalar cache."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_region_deskew_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sbb_textline_detection_amd", "csrc", "region_deskew.hip")
    asm = tmp_path / "region_deskew.s"
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
        if "region_deskew_profile_kernel" in name:
            assert "s_load_dword" in body, "the geometry / inverse-map tables are no longer read through the scalar cache"
            assert "global_atomic" not in body and "ds_add" not in body, "one plain store per row: no atomics"
        seen.add(name)
    assert any("region_deskew_profile_kernel" in n for n in seen) and any("region_crop_erode_kernel" in n for n in seen)
