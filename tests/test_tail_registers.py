"""Register budget of the fused fp32 tail, read from the code-object metadata of the built library: the 8-wave kernels run two waves
per SIMD (256 VGPRs), the 4-wave kernels three workgroups per CU (168 VGPRs); none may spill or use scratch (csrc/tail.hip)."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import __graft_entry__ as ge


def _kernel_metadata(lib):
    """{(maxnt, layers, waves): (vgpr_count, vgpr_spill_count, private_segment_fixed_size)} of every decoder_tail_kernel"""
    objdump = ge._objdump()
    readelf = os.path.join(os.path.dirname(objdump), "llvm-readelf")
    tmp = tempfile.mkdtemp(prefix="gem_meta_")
    try:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib, local)
        subprocess.run([objdump, "--offloading", local], check=True, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        notes = "\n".join(subprocess.run([readelf, "--notes", p], check=True, capture_output=True, text=True).stdout
                          for p in sorted(glob.glob(local + ".*gfx950*")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # the keys of a kernel's map are sorted: .name, .private_segment_fixed_size, ..., .vgpr_count, .vgpr_spill_count
    pat = re.compile(r"\.name:\s+(_ZN3gem9TailTilesILi(\d)EE19decoder_tail_kernelILi(\d)ELi(\d)EE\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                     r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")
    return {(int(m[2]), int(m[3]), int(m[4])): (int(m[6]), int(m[7]), int(m[5])) for m in pat.finditer(notes)}


def test_tail_kernels_fit_their_occupancy():
    if not os.path.exists(ge.LIB):
        pytest.skip("the library has not been built")
    meta = _kernel_metadata(ge.LIB)
    # 8 waves: compiled for two and for four tiles per wave; 4 waves: two tiles per pass; one to six fused layers each
    assert sorted(meta) == sorted([(2, n, 8) for n in range(1, 7)] + [(4, n, 8) for n in range(1, 7)] + [(2, n, 4) for n in range(1, 7)]), sorted(meta)
    for (maxnt, layers, waves), (vgprs, spilled, scratch) in sorted(meta.items()):
        print("TailTiles<%d>::decoder_tail_kernel<%d, %d>: %d VGPRs, %d spilled, %d bytes of scratch" % (maxnt, layers, waves, vgprs, spilled, scratch))
        assert vgprs <= (256 if waves == 8 else 168), (maxnt, layers, waves, vgprs)
        assert spilled == 0 and scratch == 0, (maxnt, layers, waves, spilled, scratch)
