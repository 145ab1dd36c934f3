"""Resources of the followed feature kernel (pt_follow_kernel), read from the code-object notes of the built
libpathtrace_hip.so as tests/test_kernel_resources.py reads the path kernel's: every instantiation -- stack window (8 | 4) x records
(HBM | LDS; the small window only with records in LDS) x (single frame | views) -- has no scratch, no VGPR spill, at most 128 VGPRs (four
waves per SIMD) and no AGPRs."""
import os
import re
import subprocess

import pytest

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
MAX_VGPRS = 128
INSTANTIATIONS = 6


def kernel_notes(lib, tmp_path, needle):
    data = open(lib, "rb").read()
    # code objects sit in .hip_fatbin as ELF images behind a clang offload bundle header; the first ELF is the host library itself
    starts = [m.start() for m in re.finditer(b"\x7fELF\x02\x01\x01", data)][1:]
    kernels = {}
    for i, s in enumerate(starts):
        path = tmp_path / ("co%d.o" % i)
        path.write_bytes(data[s:])
        out = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True).stdout
        rec = {}
        for line in out.splitlines():
            m = re.match(r"\s+[-\s]*\.(\w+):\s+(.*)$", line)
            if not m:
                continue
            rec[m.group(1)] = m.group(2).strip()
            if m.group(1) == "wavefront_size":
                if needle in rec.get("name", ""):
                    kernels[rec["name"]] = rec
                rec = {}
    return kernels


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf of ROCm not found")
    from cpupathtrace_amd import build
    return kernel_notes(build.build(), tmp_path_factory.mktemp("co"), "pt_follow_kernel")


def test_every_instantiation_is_found(kernels):
    assert len(kernels) == INSTANTIATIONS, sorted(kernels)
    assert not [name for name in kernels if "pt_path_kernel" in name]


def test_no_scratch_no_spills_four_waves(kernels):
    for name, k in kernels.items():
        print(name, "vgprs", k["vgpr_count"], "sgprs", k["sgpr_count"], "scratch", k["private_segment_fixed_size"])
        assert int(k["private_segment_fixed_size"]) == 0, (name, k["private_segment_fixed_size"])
        assert int(k["vgpr_spill_count"]) == 0, (name, k["vgpr_spill_count"])
        assert int(k.get("sgpr_spill_count", "0")) == 0, (name, k["sgpr_spill_count"])
        assert int(k["vgpr_count"]) <= MAX_VGPRS, (name, k["vgpr_count"])
        assert int(k.get("agpr_count", "0")) == 0, (name, k["agpr_count"])
