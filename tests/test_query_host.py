"""The batch queries at the drop-in boundary, without a device: the four symbols and the two C++ methods exist, and the
launchers check their arguments before anything touches the GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from voxelhashing_amd import lib, vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 4  # VH_ERR_BAD_ARGUMENT
FAKE = 0x1000  # a non-NULL address no launcher may dereference on the host


def params():
    hp = T.make_hash_params(1 << 10, 1 << 8, 0.04)
    cp = T.make_depth_camera_params(64, 48)
    rp = T.make_raycast_params(hp, cp)
    hd = T.HashData()
    hd.d_hash = FAKE
    return hd, hp, rp


def test_the_four_symbols_are_exported_and_prototyped():
    L = lib.load()
    for name in ("vh_query_points", "vh_query_rays", "vh_scene_rep_query_points", "vh_ray_cast_cast_rays"):
        assert name in lib.PROTOTYPES and hasattr(L, name), name


def test_the_host_classes_have_the_two_methods():
    prog = r'''
#include "vh.hpp"
void (CUDASceneRepHashSDF::*points)(const float*, unsigned int, float*, uint32_t*, float*, uint8_t*) = &CUDASceneRepHashSDF::queryPoints;
void (CUDARayCastSDF::*rays)(const HashData&, const HashParams&, const float*, const float*, const float*, const float*, unsigned int, float*, float*, uint32_t*, uint8_t*) = &CUDARayCastSDF::castRays;
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write(prog)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src])


def test_sample_cap_is_the_same_in_the_header_and_in_python():
    src = open(os.path.join(ROOT, "include", "vh_types.h")).read()
    m = re.search(r"#define\s+VH_QUERY_MAX_SAMPLES\s+(\d+)", src)
    assert m and int(m.group(1)) == T.QUERY_MAX_SAMPLES == 65536


def test_query_points_refuses_null_arrays():
    L = lib.load()
    hd, hp, _ = params()
    args = dict(points=FAKE, sdf=FAKE, color=FAKE, gradient=FAKE, valid=FAKE)

    def call(n=16, hd_=C.byref(hd), hp_=C.byref(hp), **over):
        a = dict(args, **over)
        return L.vh_query_points(hd_, hp_, a["points"], n, a["sdf"], a["color"], a["gradient"], a["valid"], None)

    for k in ("points", "sdf", "color", "valid"):
        assert call(**{k: None}) == BAD, k
    assert call(hd_=None) == BAD and call(hp_=None) == BAD
    empty = T.HashData()
    assert call(hd_=C.byref(empty)) == BAD  # a table that was never allocated
    # n = 0 with valid pointers: success, and no launch (there may be no device here at all)
    assert call(n=0) == 0 and call(n=0, gradient=None) == 0
    assert L.vh_scene_rep_query_points(None, FAKE, 1, FAKE, FAKE, FAKE, FAKE) == BAD


def test_query_rays_refuses_null_arrays_and_bad_increments():
    L = lib.load()
    hd, hp, rp = params()
    names = ("origins", "directions", "t_min", "t_max", "t", "normals", "color", "status")

    def call(n=16, hd_=C.byref(hd), hp_=C.byref(hp), rp_=C.byref(rp), **over):
        a = dict({k: FAKE for k in names}, **over)
        return L.vh_query_rays(hd_, hp_, rp_, a["origins"], a["directions"], a["t_min"], a["t_max"], n, a["t"], a["normals"], a["color"],
                               a["status"], None)

    for k in names:
        if k != "normals":
            assert call(**{k: None}) == BAD, k
    assert call(hd_=None) == BAD and call(hp_=None) == BAD and call(rp_=None) == BAD
    assert call(n=0) == 0 and call(n=0, normals=None) == 0
    for inc in (0.0, -0.16, float("nan"), float("inf"), -float("inf")):
        bad = T.make_raycast_params(hp, T.make_depth_camera_params(64, 48))
        bad.m_rayIncrement = inc
        assert call(rp_=C.byref(bad)) == BAD, inc
        assert call(n=0, rp_=C.byref(bad)) == BAD, inc
    assert L.vh_ray_cast_cast_rays(None, C.byref(hd), C.byref(hp), FAKE, FAKE, FAKE, FAKE, 1, FAKE, FAKE, FAKE, FAKE) == BAD
