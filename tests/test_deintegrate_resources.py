"""The frame de-integration kernels' scratch and LDS (DESIGN.md section 4 "Frame de-integration"), read from the built
library's kernel metadata; no GPU is needed.  No kernel of vh_deintegrate.hip uses scratch, and the apply kernel's LDS is
its four fact words."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

# prefix of the kernel's name: LDS bytes
LDS = {
    "k_deint_apply<false": 16,
    "k_deint_apply<true": 16,
    "k_deint_delete": 0,
    "k_deint_rule": 0,
}


@pytest.fixture(scope="module")
def kernels():
    from voxelhashing_amd import lib
    rows = {r["kernel"].split("(")[0]: r for r in KR.library_resources(lib.LIB_PATH)}
    assert len(rows) > 40, f"the library's kernel metadata was not found ({len(rows)} kernels)"
    return rows


def test_the_deintegration_kernels_are_the_four_listed(kernels):
    names = sorted(k for k in kernels if "k_deint_" in k)
    assert len(names) == len(LDS), names
    for name in names:
        assert any(name.startswith(p) or name.split(" ")[-1].startswith(p) for p in LDS), name


@pytest.mark.parametrize("prefix", sorted(LDS))
def test_no_scratch_and_the_stated_lds(kernels, prefix):
    rows = {k: r for k, r in kernels.items() if k.split(" ")[-1].startswith(prefix)}
    assert len(rows) == 1, f"{prefix}: {sorted(rows)}"
    for name, r in rows.items():
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, f"{name}: {r}"
        assert r["lds_bytes"] == LDS[prefix], f"{name}: {r['lds_bytes']} bytes of LDS, stated are {LDS[prefix]}"
        assert r["vgprs"] <= 64, f"{name}: {r['vgprs']} vector registers: fewer than eight waves per SIMD"
