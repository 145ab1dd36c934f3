"""Resources of the feature kernel that also writes motion (pt_motion_kernel), read from the code-object notes of the
built libpathtrace_hip.so as tests/test_feature_kernel_resources.py reads the followed kernel's: every instantiation -- stack window
(8 | 4) x records (HBM | LDS; the small window only with records in LDS), single frames only -- has no scratch, no VGPR spill, at most 128
VGPRs (four waves per SIMD) and no AGPRs."""
import os

import pytest

from tests.test_feature_kernel_resources import MAX_VGPRS, READELF, kernel_notes

INSTANTIATIONS = 3


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf of ROCm not found")
    from cpupathtrace_amd import build
    return kernel_notes(build.build(), tmp_path_factory.mktemp("co"), "pt_motion_kernel")


def test_every_instantiation_is_found(kernels):
    assert len(kernels) == INSTANTIATIONS, sorted(kernels)
    assert not [name for name in kernels if "pt_follow_kernel" in name or "pt_path_kernel" in name]


def test_no_scratch_no_spills_four_waves(kernels):
    for name, k in kernels.items():
        print(name, "vgprs", k["vgpr_count"], "sgprs", k["sgpr_count"], "scratch", k["private_segment_fixed_size"])
        assert int(k["private_segment_fixed_size"]) == 0, (name, k["private_segment_fixed_size"])
        assert int(k["vgpr_spill_count"]) == 0, (name, k["vgpr_spill_count"])
        assert int(k.get("sgpr_spill_count", "0")) == 0, (name, k["sgpr_spill_count"])
        assert int(k["vgpr_count"]) <= MAX_VGPRS, (name, k["vgpr_count"])
        assert int(k.get("agpr_count", "0")) == 0, (name, k["agpr_count"])
