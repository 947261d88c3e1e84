"""The drop-in boundary without a GPU: the library loads, exports every symbol
include/vh_api.h declares, the ctypes mirrors have the C layouts, and argument
validation works (no kernel is launched here)."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest

from voxelhashing_amd import lib, vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "vh_api.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(vh_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_library_is_built_in_tree():
    assert os.path.exists(lib.LIB_PATH), "run `python -m voxelhashing_amd.build` (or __graft_entry__.build())"
    assert os.path.dirname(lib.LIB_PATH) == os.path.join(ROOT, "voxelhashing_amd")


def test_every_declared_symbol_is_exported_and_prototyped():
    names = declared_functions()
    assert len(names) > 60
    L = C.CDLL(lib.LIB_PATH)
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, f"declared in vh_api.h but not exported: {missing}"
    assert sorted(lib.PROTOTYPES) == names, (set(names) ^ set(lib.PROTOTYPES))
    lib.load()
    assert b"gfx950" in lib.load().vh_version()


def test_struct_layouts_match_the_c_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "vh_types.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(VhHashEntry), sizeof(VhVoxel), sizeof(VhHashParams),
         sizeof(VhDepthCameraParams), sizeof(VhRayCastParams), sizeof(VhHashData), sizeof(VhDepthCameraData),
         sizeof(VhRayCastData), sizeof(VhSDFBlockDesc), sizeof(VhSceneOptions));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(VhFrameJob), sizeof(VhReconstructionOptions), sizeof(VhSequenceFrame), sizeof(VhReconstructionStats),
         offsetof(VhFrameJob, lockToken), offsetof(VhReconstructionOptions, s_streamingRadius), offsetof(VhSequenceFrame, color));
  printf("%zu %zu %zu %zu %zu\n", offsetof(VhHashParams, m_hashNumBuckets), offsetof(VhHashParams, m_virtualVoxelSize),
         offsetof(VhHashParams, m_streamingVoxelExtents), offsetof(VhRayCastParams, m_width), offsetof(VhHashData, d_bucketCount));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    sizes = [int(v) for v in out[0].split()]
    want = [C.sizeof(t) for t in (T.HashEntry, T.Voxel, T.HashParams, T.DepthCameraParams, T.RayCastParams, T.HashData,
                                  T.DepthCameraData, T.RayCastData, T.SDFBlockDesc, T.SceneOptions)]
    assert sizes == want
    assert sizes[:5] == [32, 8, 224, 32, 304]  # reference layouts
    loop = [int(v) for v in out[1].split()]
    assert loop == [C.sizeof(T.FrameJob), C.sizeof(T.ReconstructionOptions), C.sizeof(T.SequenceFrame), C.sizeof(T.ReconstructionStats),
                    T.FrameJob.lockToken.offset, T.ReconstructionOptions.s_streamingRadius.offset, T.SequenceFrame.color.offset]
    out = [out[0]] + out[2:]
    offs = [int(v) for v in out[1].split()]
    assert offs == [T.HashParams.m_hashNumBuckets.offset, T.HashParams.m_virtualVoxelSize.offset,
                    T.HashParams.m_streamingVoxelExtents.offset, T.RayCastParams.m_width.offset, T.HashData.d_bucketCount.offset]


def test_argument_validation_without_gpu():
    L = lib.load()
    assert L.vh_reset(None, None, None) == 4  # VH_ERR_BAD_ARGUMENT
    assert L.vh_alloc(None, None, None, None, None, -1, None) == 4
    assert L.vh_render(None, None, None, None, None, None) == 4
    assert L.vh_scene_rep_integrate(None, None, None, None, None) == 4
    hp = T.make_hash_params(16, 16, 0.04)
    hp.m_hashBucketSize = 7  # the bucket size is a compile-time constant of the path
    hd = T.HashData()
    assert L.vh_hash_data_alloc(C.byref(hd), C.byref(hp)) == 4
    assert L.vh_error_string(4) == b"bad argument"
    assert L.vh_error_string(1) == b"SDF block heap exhausted"


def test_cpp_host_header_compiles_standalone():
    """include/vh.hpp needs no HIP headers: a reference-side translation unit can include it"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "vh.hpp"\nint main(){ vh::mat4f m = vh::mat4f(); (void)m; return sizeof(CUDASceneRepHashSDF) > 0 ? 0 : 1; }\n')
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src])


OWNERS_PROGRAM = r"""
#include "vh.hpp"
#include <cstdio>
// counting deleters in place of the library's: the program does not link it
static int g_device = 0, g_pinned = 0, g_event = 0, g_stream = 0;
void vh::DeviceFree::operator()(void*) const noexcept { g_device++; }
void vh::PinnedFree::operator()(void*) const noexcept { g_pinned++; }
void vh::EventDestroy::operator()(void*) const noexcept { g_event++; }
void vh::StreamDestroy::operator()(void*) const noexcept { g_stream++; }
static int g_made = 0;
void* vh::pinnedAllocBytes(size_t, bool, const char*) { static char host[64]; g_made++; return host; }
void* vh::deviceAlias(void* host, const char*) { return (char*)host + 1; }
#define EXPECT(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
template <class Owner, class T> static int rules(int& count, T* a, T* b)
{
    count = 0;
    { Owner o(a); }
    EXPECT(count == 1);                       // once on scope exit
    { Owner o(a); EXPECT(o.release() == a); }
    EXPECT(count == 1);                       // not at all after release()
    { Owner o(a); o = Owner(b); EXPECT(count == 2 && o.get() == b); }
    EXPECT(count == 3);                       // once for the old value on assignment, once for the new one at the end
    { Owner o(a); Owner p(std::move(o)); EXPECT(!o && p.get() == a); }
    EXPECT(count == 4);                       // a moved-from owner frees nothing
    { Owner o; }
    EXPECT(count == 4);                       // nor does an empty one
    return 0;
}
int main()
{
    float f[2];
    uint32_t w[2];
    int x[2];
    if (rules<vh::DevicePtr<float>>(g_device, &f[0], &f[1])) return 1;
    if (rules<vh::PinnedPtr<uint32_t>>(g_pinned, &w[0], &w[1])) return 1;
    if (rules<vh::Event>(g_event, (void*)&x[0], (void*)&x[1])) return 1;
    if (rules<vh::Stream>(g_stream, (void*)&x[0], (void*)&x[1])) return 1;
    g_pinned = 0;
    {
        vh::Mapped<uint32_t> m(4, "mapped");  // the host pointer and its device alias travel together
        EXPECT(m.host() && (char*)m.device() == (char*)m.host() + 1);
        vh::Mapped<uint32_t> n(std::move(m));
        EXPECT(!m.host() && !m.device() && n.host() && n.device());
        n = vh::Mapped<uint32_t>(4, "mapped");
        EXPECT(g_pinned == 1 && g_made == 2);
        vh::Mapped<uint32_t> empty;
        EXPECT(!empty.host() && !empty.device());
    }
    EXPECT(g_pinned == 2);
    std::printf("ok\n");
    return 0;
}
"""


def test_owners_free_exactly_once():
    """the owning types of include/vh_owners.hpp (device and pinned memory, events, streams, mapped words): freed once on
    scope exit, not after release(), once for the old value on assignment, never by a moved-from or empty owner"""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        open(src, "w").write(OWNERS_PROGRAM)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        res = subprocess.run([exe], stdout=subprocess.PIPE)
        assert res.returncode == 0 and res.stdout.decode().strip() == "ok", res.stdout.decode()


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "voxelhashing_amd")
    bad = []
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                if re.search(r"(from|import)\s+oracle|libvh_oracle|vh_oracle\.h|vho_", txt):
                    bad.append(f)
    assert not bad, f"product files reference the oracle: {bad}"


def test_every_entry_point_refuses_null_arguments():
    """all pointers NULL, all numbers 0: an error code, never a crash and never a launch (the arguments are checked
    before anything touches the device).  vh_bind_input_depth_color_textures is the reference's texture binding: a
    documented no-op.  vh_device_synchronize() has no arguments and vh_stream_synchronize(NULL) waits for the null
    stream: valid calls, which succeed where there is a device and fail with an error code where there is none."""
    import ctypes as C
    from voxelhashing_amd import lib
    L = lib.load()
    # asked of the library's own HIP runtime (not torch's, which may be a second one in this process): one byte
    p = C.c_void_p()
    have_device = L.vh_malloc(C.byref(p), 1) == 0
    if have_device:
        lib.check(L.vh_free(p), "vh_free")
    checked = 0
    for name, (res, args) in lib.PROTOTYPES.items():
        if res is not C.c_int:
            continue
        vals = [0 if a in (C.c_int, C.c_uint32, C.c_uint64, C.c_int32, C.c_size_t) else 0.0 if a in (C.c_float, C.c_double) else None for a in args]
        rc = getattr(L, name)(*vals)
        if name == "vh_bind_input_depth_color_textures":
            assert rc == 0
        elif name in ("vh_device_synchronize", "vh_stream_synchronize"):
            assert (rc == 0) == have_device, (name, rc)
        else:
            assert rc != 0, name
        checked += 1
    assert checked > 120
