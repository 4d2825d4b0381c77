"""VPR_SKINNY_FETCH without a GPU: the library knows the switch (set, get, unset through vpr_tuning_set / vpr_tuning_get), the
header names it among the switches, and NOT among those whose values change result bits: both fetch forms run one K partition
and one order of sums (tests/test_skinny_fetch_gpu.py holds them to the bits of the library before the switch existed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_knows_the_switch_and_the_header_promises_equal_bits():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    old = _lib.tuning_get("VPR_SKINNY_FETCH")
    try:
        for v in (0, 1, None):
            _lib.tuning_set("VPR_SKINNY_FETCH", v)
            assert _lib.tuning_get("VPR_SKINNY_FETCH") == v
    finally:
        _lib.tuning_set("VPR_SKINNY_FETCH", old)
    text = open(os.path.join(ROOT, "include", "vpr_amd.h")).read()
    assert "VPR_SKINNY_FETCH" in text[text.index("Tuning switches"):text.index("int vpr_tuning_set")]
    para = text[text.index("(2) per PROCESS"):text.index("dtype conventions")]
    clause = para[para.index("bit-identical results, except"):para.index("Timing-only")]
    assert "VPR_SKINNY_FETCH" not in re.findall(r"VPR_[A-Z0-9_]+", clause)
    # the wave-count and row-block switches of the kernel are still there
    for name in ("VPR_SKINNY_NW", "VPR_SKINNY_MBW"):
        _lib.tuning_get(name)
