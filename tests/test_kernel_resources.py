"""Register budget of the path kernel, read from the code-object notes of the built libpathtrace_hip.so (as tools/kernel_regs.py does).

Every instantiation of pt_path_kernel must stay at 128 VGPRs or fewer (four waves per SIMD: the occupancy its __launch_bounds__ asks
for), and its VGPR spills must not grow back above what the packed slot state and the lane values bound per traversal-loop entry brought them down to
(DESIGN §5.5).  Lower this bound when a change removes more of them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

MAX_VGPRS = 128
MAX_VGPR_SPILLS = 29  # compact slot word: 25, wide slot word: 28-29
MAX_SCRATCH_BYTES = 100
INSTANTIATIONS = 6  # slot word (compact | wide) x records (HBM | LDS) x stack window (8 | 4 entries in LDS)


def path_kernel_notes(lib, tmp_path):
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
                if "pt_path_kernel" in rec.get("name", ""):
                    kernels[rec["name"]] = rec
                rec = {}
    return kernels


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf of ROCm not found")
    from cpupathtrace_amd import build
    lib = build.build()
    return path_kernel_notes(lib, tmp_path_factory.mktemp("co"))


def test_every_instantiation_is_found(kernels):
    assert len(kernels) == INSTANTIATIONS, sorted(kernels)


def test_vgprs_within_four_waves(kernels):
    for name, k in kernels.items():
        assert int(k["vgpr_count"]) <= MAX_VGPRS, (name, k["vgpr_count"])
        assert int(k.get("agpr_count", "0")) == 0, (name, k["agpr_count"])


def test_vgpr_spills_do_not_grow(kernels):
    for name, k in kernels.items():
        assert int(k["vgpr_spill_count"]) <= MAX_VGPR_SPILLS, (name, k["vgpr_spill_count"])
        assert int(k["private_segment_fixed_size"]) <= MAX_SCRATCH_BYTES, (name, k["private_segment_fixed_size"])
