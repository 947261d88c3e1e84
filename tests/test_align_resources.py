"""The scene registration kernels' registers, scratch and LDS (DESIGN.md section 4 "Scene registration"), read from the
built library's kernel metadata; no GPU is needed.  No kernel of vh_align.hip uses scratch or spills; the step kernel's
LDS is its 125 block pointers, the four waves' 29 partial sums and their flags (1,444 bytes) and what the block-wide
vote adds (268 bytes, as in k_resample_blocks); its registers are those of the 6x6 solve it ends with, as k_icp_step's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

# the kernel's name: (LDS bytes, the most vector registers DESIGN.md states)
KERNELS = {
    "k_align_step": (1712, 208),
    "k_align_rule": (768, 128),
    "k_align_bounds": (0, 32),
    "k_align_raise": (0, 32),
}


@pytest.fixture(scope="module")
def kernels():
    from voxelhashing_amd import lib
    rows = {r["kernel"].split("(")[0]: r for r in KR.library_resources(lib.LIB_PATH)}
    assert len(rows) > 40, f"the library's kernel metadata was not found ({len(rows)} kernels)"
    return rows


def test_the_registration_kernels_are_the_four_listed(kernels):
    names = sorted(k.split(" ")[-1] for k in kernels if "k_align_" in k)
    assert names == sorted(KERNELS), names


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_no_scratch_no_spills_the_stated_lds_and_registers(kernels, name):
    rows = {k: r for k, r in kernels.items() if k.split(" ")[-1] == name}
    assert len(rows) == 1, f"{name}: {sorted(rows)}"
    lds, vgprs = KERNELS[name]
    for full, r in rows.items():
        print(full, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, f"{full}: {r}"
        assert r["lds_bytes"] == lds, f"{full}: {r['lds_bytes']} bytes of LDS, stated are {lds}"
        assert r["vgprs"] <= vgprs, f"{full}: {r['vgprs']} vector registers, stated are at most {vgprs}"


def test_the_resampler_kept_its_resources(kernels):
    """the blend moved to a header that both units share: k_resample_blocks is the kernel it was"""
    r = kernels["k_resample_blocks"]
    assert (r["vgprs"], r["lds_bytes"], r["scratch_bytes"]) == (48, 784, 0), r
