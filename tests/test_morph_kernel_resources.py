"""Resources of the blend-shape kernel (kd_morph), read from the code-object notes of the built libpathtrace_hip.so as
tests/test_feature_kernel_resources.py reads the followed kernel's: every instantiation -- K = 0 .. 8 x the two table forms -- has no
scratch and no spill; the LDS form holds at most the 20 KiB a block has at full occupancy (8 blocks of 256 threads share a CU's
160 KiB), the cache form none.  The skinning kernel beside it in the same unit keeps its sixteen instantiations without scratch."""
import os
import re

import pytest

from tests.test_feature_kernel_resources import READELF, kernel_notes

LDS_PER_BLOCK = 160 * 1024 // 8


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf of ROCm not found")
    from cpupathtrace_amd import build
    lib = build.build()
    return kernel_notes(lib, tmp_path_factory.mktemp("morph_co"), "kd_morph"), kernel_notes(lib, tmp_path_factory.mktemp("skin_co"), "kd_skin")


def test_every_instantiation_is_found(notes):
    morph, skin = notes
    found = sorted((int(m.group(1)), int(m.group(2))) for m in (re.search(r"kd_morphILi(\d+)ELb(\d)E", name) for name in morph))
    assert found == [(k, form) for k in range(9) for form in (0, 1)], sorted(morph)
    assert len(skin) == 16, sorted(skin)


def test_no_scratch_no_spills_and_lds_within_a_blocks_share(notes):
    morph, skin = notes
    for name, k in list(morph.items()) + list(skin.items()):
        print(name, "vgprs", k["vgpr_count"], "sgprs", k["sgpr_count"], "lds", k["group_segment_fixed_size"], "scratch", k["private_segment_fixed_size"])
        assert int(k["private_segment_fixed_size"]) == 0, (name, k["private_segment_fixed_size"])
        assert int(k["vgpr_spill_count"]) == 0, (name, k["vgpr_spill_count"])
        assert int(k.get("sgpr_spill_count", "0")) == 0, (name, k["sgpr_spill_count"])
    for name, k in morph.items():
        staged = re.search(r"kd_morphILi(\d+)ELb(\d)E", name).group(2) == "1"
        lds = int(k["group_segment_fixed_size"])
        assert (0 < lds <= LDS_PER_BLOCK) if staged else lds == 0, (name, lds)
