"""The live-mesh kernels' scratch, LDS and registers (DESIGN.md section 4 "Live mesh"), read from the built library's
kernel metadata; no GPU is needed.  No kernel of vh_live_mesh.hip uses scratch or LDS -- the digest's reduction and the
list appends go through the wave -- and the kernels that run over blocks, positions and triangles stay at eight waves a
SIMD."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

# the kernel's name: LDS bytes
LDS = {
    "k_live_begin": 0,
    "k_live_digest": 0,
    "k_live_vanished": 0,
    "k_live_dilate": 0,
    "k_live_drop": 0,
    "k_live_seal": 0,
    "k_live_finish": 0,
    "k_live_digest_list": 0,
}
AT_MOST_64_VGPRS = ("k_live_digest", "k_live_digest_list", "k_live_vanished", "k_live_dilate", "k_live_drop")


@pytest.fixture(scope="module")
def kernels():
    from voxelhashing_amd import lib
    rows = {r["kernel"].split("(")[0].split(" ")[-1]: r for r in KR.library_resources(lib.LIB_PATH)}
    assert len(rows) > 40, f"the library's kernel metadata was not found ({len(rows)} kernels)"
    return rows


def test_the_live_mesh_kernels_are_the_ones_listed(kernels):
    assert sorted(k for k in kernels if "k_live_" in k) == sorted(LDS)


@pytest.mark.parametrize("name", sorted(LDS))
def test_no_scratch_and_the_stated_lds(kernels, name):
    r = kernels[name]
    print(name, r)
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, f"{name}: {r}"
    assert r["lds_bytes"] == LDS[name], f"{name}: {r['lds_bytes']} bytes of LDS, stated are {LDS[name]}"
    if name in AT_MOST_64_VGPRS:
        assert r["vgprs"] <= 64, f"{name}: {r['vgprs']} vector registers: fewer than eight waves per SIMD"
