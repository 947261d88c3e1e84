"""What the ray caster's kernels cost in registers and scratch, read from the built library's own kernel metadata (no GPU
is needed), and the launcher's rule for 32-bit voxel offsets.

The march of k_render is bound by vector-instruction issue at six waves per SIMD, that is 80 vector registers; what does
not fit is spilled to scratch memory, and a spill inside the march costs more than the instructions a change saves
(DESIGN.md section 6).  The bounds below are the ones the kernel was brought to; a change that exceeds them has to show
where the spills went before it raises them."""
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


def variants(kernels, prefix):
    out = {k: r for k, r in kernels.items() if k.startswith(prefix)}
    assert out, f"no kernel named {prefix}...: {sorted(k for k in kernels if 'render' in k)}"
    return out


def test_small_table_ray_caster_fits_six_waves(kernels):
    """k_render without gradients, with either voxel addressing: at most 80 vector registers and 16 bytes of scratch"""
    rows = variants(kernels, "k_render<false")
    assert len(rows) == 2, sorted(rows)
    for name, r in rows.items():
        print(name, r)
        assert r["vgprs"] <= 80, f"{name}: {r['vgprs']} vector registers"
        assert r["scratch_bytes"] <= 16, f"{name}: {r['scratch_bytes']} bytes of scratch"
        assert r["lds_bytes"] == 4 * 2 * 64 * 12 * 4, f"{name}: the four tile tables are 24 KB"


def test_pipelined_ray_caster_has_no_scratch(kernels):
    rows = variants(kernels, "k_render_large<false")
    assert len(rows) == 2, sorted(rows)
    for name, r in rows.items():
        print(name, r)
        assert r["scratch_bytes"] == 0, f"{name}: {r['scratch_bytes']} bytes of scratch"
        assert r["vgpr_spills"] == 0, f"{name}: {r['vgpr_spills']} spilled vector registers"


def test_offsets32_rule(vh):
    """32-bit byte offsets as long as the pool is at most 2^32 bytes: 2^20 blocks of 4096 bytes, and not one more"""
    from voxelhashing_amd import lib
    assert vh.vh_render_offsets32(1 << 20) == 1
    assert vh.vh_render_offsets32((1 << 20) + 1) == 0
    assert vh.vh_render_offsets32(1) == 1 and vh.vh_render_offsets32(1 << 21) == 0 and vh.vh_render_offsets32(0xffffffff) == 0
    try:
        assert vh.vh_debug_render_force_offsets64(1) == 0
        assert vh.vh_render_offsets32(1 << 20) == 0 and vh.vh_render_offsets32(1) == 0
    finally:
        vh.vh_debug_render_force_offsets64(0)
    assert vh.vh_render_offsets32(1 << 20) == 1


# image sizes by their number of 8x8 tiles; from 300 on they are tests/test_gpu_tile_intervals.py's SIZES
SCHEDULE_SIZES = {0: (0, 0), 1: (8, 8), 300: (160, 120), 1023: (264, 248), 1024: (256, 256), 1056: (264, 256), 1073: (291, 227)}


@pytest.mark.parametrize("n_tiles", list(SCHEDULE_SIZES))
def test_schedule_buffer_size(vh, n_tiles):
    """the schedule buffer's words as tests/test_gpu_tile_intervals.py::Schedule lays it out: 4 header words, a cost class
    per tile padded to whole quads, two words per launch slot for 4 * ceil((tiles + 256) / 4) slots -- room for the most
    tiles any image has split; and the tiles this image has split, against tile_intervals.split_tiles"""
    import tile_intervals as TI
    W, H = SCHEDULE_SIZES[n_tiles]
    assert ((W + 7) // 8) * ((H + 7) // 8) == n_tiles
    quads = lambda n: (n + 3) // 4  # noqa: E731
    words = 4 + 4 * quads(n_tiles) + 2 * 4 * quads(n_tiles + 256)
    nbytes = vh.vh_render_schedule_bytes(W, H)
    print(n_tiles, "tiles:", nbytes, "bytes, the layout", 4 * words)
    assert nbytes % 4 == 0 and nbytes // 4 == words
    assert vh.vh_render_split_tiles(W, H) == TI.split_tiles(n_tiles)
    # the slots a launch uses lie inside the buffer
    assert 4 + 4 * quads(n_tiles) + 2 * 4 * quads(n_tiles + TI.split_tiles(n_tiles)) <= words


ASM = """
	.text
	.globl	_Z3fooPf
_Z3fooPf:                               ; @_Z3fooPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v0, 0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	s_waitcnt lgkmcnt(0)
	global_store_dword v0, v0, s[0:1]
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _Z3fooPf
	.end_amdhsa_kernel
.Lfunc_end0:
	.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .name:           p
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 512
    .kernarg_segment_align: 8
    .kernarg_segment_size: 8
    .max_flat_workgroup_size: 256
    .name:           _Z3fooPf
    .private_segment_fixed_size: 24
    .sgpr_count:     12
    .sgpr_spill_count: 2
    .symbol:         _Z3fooPf.kd
    .vgpr_count:     7
    .vgpr_spill_count: 3
    .wavefront_size: 64
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
	.end_amdgpu_metadata
"""


def test_the_tool_reads_device_assembly():
    rows = KR.resources(ASM)
    assert len(rows) == 1
    r = rows[0]
    assert r["name"] == "_Z3fooPf" and r["kernel"].startswith("foo(")
    assert (r["vgprs"], r["sgprs"], r["lds_bytes"], r["scratch_bytes"], r["vgpr_spills"], r["sgpr_spills"]) == (7, 12, 512, 24, 3, 2)
    assert r["instruction_lines"] == 5
    assert "| `foo` | 7 | 12 | 512 | 24 | 5 | 5 |" in KR.table(rows)


def test_the_tool_lists_instruction_sequences():
    """what --against compares: the kernel's instructions alone, without the label of the loop and its comment"""
    seqs = KR.instruction_sequences(ASM)
    assert seqs == {"_Z3fooPf": ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v0, 0", "s_waitcnt lgkmcnt(0)",
                                 "global_store_dword v0, v0, s[0:1]", "s_endpgm"]}
    branch = ASM.replace("\ts_endpgm", "\ts_cbranch_scc1 .LBB0_1\n\ts_endpgm")
    renumbered = branch.replace(".LBB0_1", ".LBB7_12")
    assert KR.instruction_sequences(branch) == KR.instruction_sequences(renumbered)
    assert KR.against(seqs, KR.instruction_sequences(branch)) == [("_Z3fooPf", "differs (6 → 5 lines)")]
    assert KR.against(seqs, {}) == [("_Z3fooPf", "only here")] and KR.against({}, seqs) == [("_Z3fooPf", "only there")]
