"""The ray-casting kernels' registers and scratch with the SLP vectorizer out of the frame-loop unit and the march's packed
fp32 written by hand, read from the built library's kernel metadata; no GPU is needed.

The bounds are the figures of the kernels as the vectorizer left them (at 858c1da): taking it out must not cost a kernel its
occupancy.  k_render_large with gradients took 177 registers without the vectorizer, two waves per SIMD where its tables
allow three; 168 registers are three waves."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402


@pytest.fixture(scope="module")
def kernels():
    from voxelhashing_amd import lib
    rows = {r["kernel"].split("(")[0]: r for r in KR.library_resources(lib.LIB_PATH)}
    assert len(rows) > 40, f"the library's kernel metadata was not found ({len(rows)} kernels)"
    return rows


# prefix of the kernel's name: (vector registers at most, scratch bytes at most)
BOUNDS = {
    "k_render<false": (73, 0),
    "k_render_large<false": (117, 0),
    "k_render_large<true": (168, None),
    "k_render<true": (80, 2352),
}


@pytest.mark.parametrize("prefix", sorted(BOUNDS))
def test_ray_caster_keeps_its_registers(kernels, prefix):
    vgprs, scratch = BOUNDS[prefix]
    rows = {k: r for k, r in kernels.items() if k.startswith(prefix)}
    assert len(rows) == 2, f"{prefix}: both voxel addressings: {sorted(rows)}"
    for name, r in rows.items():
        print(name, r)
        assert r["vgprs"] <= vgprs, f"{name}: {r['vgprs']} vector registers, at most {vgprs}"
        if scratch is not None:
            assert r["scratch_bytes"] <= scratch, f"{name}: {r['scratch_bytes']} bytes of scratch, at most {scratch}"


def test_the_frame_loop_unit_is_built_without_the_slp_vectorizer():
    """one table of extra flags by source, honoured by the library's build, by a variant's and by the resources tool"""
    from voxelhashing_amd import build as B
    assert "-fno-slp-vectorize" in B.flags("vh_kernels.hip")
    assert "-fno-slp-vectorize" in B.flags(os.path.join(B.CSRC, "vh_kernels.hip"))
    for s in B.SOURCES:
        if s != "vh_kernels.hip":
            assert B.flags(s) == B.flags(), s
    assert "-ffp-contract=off" in B.flags("vh_kernels.hip") and "-fno-fast-math" in B.flags("vh_kernels.hip")
