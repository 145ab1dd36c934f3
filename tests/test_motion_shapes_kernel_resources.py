"""Resources of the feature kernel that reprojects deformed meshes per vertex (pt_motion_shapes_kernel) and of the face
table kernel (pt_face_table_kernel), read from the code-object notes of the built libpathtrace_hip.so as
tests/test_motion_kernel_resources.py reads the motion kernel's, with its limits: every instantiation -- stack window (8 | 4) x records
(HBM | LDS; the small window only with records in LDS), single frames only -- has no scratch, no VGPR spill, at most 128 VGPRs (four waves
per SIMD) and no AGPRs.  The single-kernel form shipped: there is no pt_motion_shapes_resolve_kernel."""
import os

import pytest

from tests.test_feature_kernel_resources import MAX_VGPRS, READELF, kernel_notes

INSTANTIATIONS = 3
OTHERS = ("pt_motion_kernel", "pt_feature_kernel", "pt_follow_kernel", "pt_path_kernel")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf of ROCm not found")
    from cpupathtrace_amd import build
    lib, tmp = build.build(), tmp_path_factory.mktemp("co")
    return {needle: kernel_notes(lib, tmp, needle) for needle in ("pt_motion_shapes_kernel", "pt_face_table_kernel", "pt_motion_shapes_resolve_kernel")}


def test_every_instantiation_is_found(notes):
    kernels = notes["pt_motion_shapes_kernel"]
    assert len(kernels) == INSTANTIATIONS, sorted(kernels)
    assert len(notes["pt_face_table_kernel"]) == 1, sorted(notes["pt_face_table_kernel"])
    assert not notes["pt_motion_shapes_resolve_kernel"]  # the single-kernel form
    # the names are found by none of the other resource tests' substrings
    for name in list(kernels) + list(notes["pt_face_table_kernel"]):
        assert not [other for other in OTHERS if other in name], name


def test_no_scratch_no_spills_four_waves(notes):
    assert len(notes["pt_motion_shapes_kernel"]) == INSTANTIATIONS and len(notes["pt_face_table_kernel"]) == 1  # (nothing found is no pass)
    for name, k in list(notes["pt_motion_shapes_kernel"].items()) + list(notes["pt_face_table_kernel"].items()):
        print(name, "vgprs", k["vgpr_count"], "sgprs", k["sgpr_count"], "scratch", k["private_segment_fixed_size"])
        assert int(k["private_segment_fixed_size"]) == 0, (name, k["private_segment_fixed_size"])
        assert int(k["vgpr_spill_count"]) == 0, (name, k["vgpr_spill_count"])
        assert int(k.get("sgpr_spill_count", "0")) == 0, (name, k["sgpr_spill_count"])
        assert int(k["vgpr_count"]) <= MAX_VGPRS, (name, k["vgpr_count"])
        assert int(k.get("agpr_count", "0")) == 0, (name, k["agpr_count"])
