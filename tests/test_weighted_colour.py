"""The weighted colour average (HashParams.m_colorIntegration = 1, CUDASceneRepHashSDF::setColorIntegration) without a
GPU: the rule's float32 and integer forms, the arithmetic the device uses for it, the numpy reference of
tests/weighted_colour.py against the oracle, the closed RGB-D tracking loop the rule is there for, and the ABI."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import rgbd_icp as G
import weighted_colour as WC
from helpers import small_config
from test_rgbd_tracking import all_colour_settings, pose_error
from voxelhashing_amd import synth, vhtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float32_rule_equals_the_integer_rule_for_every_pair():
    """(uchar)(n / d + 0.5f) in float32 == (2 n + d) // (2 d) for every n = c0 w0 + c1 w1 <= 255 d, d = w0 + w1 in 1..510
    (33 228 285 pairs; n and d are exact in float32, so the pair is all the formula sees)"""
    pairs = 0
    for d in range(1, 511):
        n = np.arange(0, 255 * d + 1, dtype=np.int64)
        got = (n.astype(np.float32) / np.float32(d) + np.float32(0.5)).astype(np.uint8)
        assert np.array_equal(got, ((2 * n + d) // (2 * d)).astype(np.uint8)), d
        pairs += len(n)
    assert pairs == 33228285
    # the three-term form the helper offers, on quadruples
    rng = np.random.default_rng(5)
    c0, w0, c1 = (rng.integers(0, 256, 1 << 20) for _ in range(3))
    w1 = rng.integers(1, 256, 1 << 20)
    assert np.array_equal(WC.rule_weighted_float32(c0, w0, c1, w1), WC.rule_weighted(c0, w0, c1, w1))


@pytest.mark.parametrize("ulps", [-2, 0, 2])
def test_device_arithmetic_of_the_rule_in_exact_integers(ulps):
    """vh_device.hpp weighted_colour: t = 2 n + d, yh = fl(y * (1/2 + 2^-22)) for a reciprocal y of d that is up to two
    ulp off, then ONE rounding of t * yh + (2^23 - 1/2) to an integer (an fma; the sum is at least 2^23), whose low byte
    is the colour.  Restated with yh = M 2^-K as integers, for every (n, d): equal to (2 n + d) // (2 d).  (The device
    itself runs every (c0, w0, c1, w1): test_gpu_weighted_colour.py.)"""
    for d in range(1, 511):
        y = np.float32(1.0) / np.float32(d)
        y = (y.view(np.uint32).astype(np.int64) + ulps).astype(np.uint32).view(np.float32)
        yh = np.float32(y * np.float32(0.5 + 2.0 ** -22))
        m, e = np.frexp(np.float64(yh))
        M, K = int(m * 2 ** 24), 24 - int(e)
        t = 2 * np.arange(0, 255 * d + 1, dtype=np.int64) + d
        num, den = 2 * t * M - (1 << K), 1 << (K + 1)  # t yh - 1/2 = num / den, to be rounded to nearest, ties to even
        q, r = np.divmod(num, den)
        got = q + ((2 * r > den) | ((2 * r == den) & (q & 1 == 1)))
        assert np.array_equal(got, t // (2 * d)), d


def orbit_frames(scene_name, n, n_orbit, cp):
    from oracle import oracle as O
    spheres, inside, radius = synth.scene(scene_name)
    for k in range(n):
        pose = synth.orbit_pose(k, n_orbit, radius)
        yield k, pose, O.synth_frame(spheres, inside, pose, cp)


def test_helper_reproduces_the_oracle_under_the_running_average(oracle_lib):
    """tests/weighted_colour.py with its rule set to combineVoxel's own, (c0 + c1 + 1) >> 1: the colours it keeps (w1 and
    c1 from the probe scene, blocks dropped with the table) equal the oracle's bit for bit on every frame, with garbage
    collection and starving on; and on frames without starving the oracle's weight is min(weightMax, w0 + w1)"""
    hp, cp, rp = small_config(160, 120, "P4")
    s = WC.WeightedColourScene(hp, cp, rp, T.make_scene_options(offline=True, gc=True, starve=3), rule=WC.rule_running)
    freed = updated = 0
    for k, pose, (d, c) in orbit_frames("S1", 6, 150, cp):
        s.integrate(pose, d, c)
        L = s.last
        assert L["starved"] == (k == 3)
        freed += len(set(L["seen"]) - set(L["after"]))
        updated += L["updated"]
        for pos, want in L["oracle_colours"].items():
            got = s.colours.get(pos)
            if got is None:
                assert not want.any(), (k, pos)
            else:
                assert np.array_equal(got, want), f"frame {k} block {pos}: colours differ from the oracle's"
        if not L["starved"]:
            vox = s.o.sdf_blocks().reshape(-1, T.SDF_BLOCK_VOXELS)
            for pos, bid in L["after"].items():
                w0 = L["w0"][bid] if pos in L["before"] else 0
                assert np.array_equal(vox["weight"][bid], np.minimum(hp.m_integrationWeightMax, w0 + L["w1"][bid])), (k, pos)
    assert updated > 100000 and freed > 0, (updated, freed)
    s.close()


def closed_loop_cpu(n_frames, rule):
    """the restatement's loop: frame k tracked (tests/rgbd_icp.py apply_ct, colour on every level) against the oracle's
    ray cast of the model at pose k - 1, integrated at the tracked pose -> per frame (translation error m, rotation
    error degrees), None from the frame on that lost tracking"""
    hp, cp, rp = small_config(160, 120, "P1", num_buckets=1 << 15, num_sdf_blocks=1 << 14)
    s = WC.WeightedColourScene(hp, cp, rp, T.make_scene_options(offline=True, gc=False), rule=rule)
    truth = [G.plane_pose(0.012 * k, -0.003 * k) for k in range(n_frames)]
    ts, eye = all_colour_settings(), np.eye(4, dtype=np.float32)
    pose, errors = truth[0], []
    for k in range(n_frames):
        depth, rgbx = G.plane_frame(truth[k], cp)
        inp, inp_n, inp_col = G.sensor_maps(depth, rgbx, cp)
        if k > 0:
            m = s.render(pose)
            got, _ = G.apply_ct(inp, inp_n, inp_col, m["depth4"], m["normals"], m["colors"], pose, ts, eye, cp, 3)
            if got is None:
                errors.append(None)
                break
            pose = np.asarray(got, np.float32).reshape(16)
            errors.append(pose_error(pose, truth[k]))
        s.integrate(pose, depth, inp_col)
    s.close()
    return errors


def test_closed_rgbd_loop_holds_with_the_weighted_average(oracle_lib):
    """What the rule is for.  The textured plane at 160x120, 1 cm voxels, the camera moving 12 mm / -3 mm a frame in the
    plane (which only the photometric term sees), every frame tracked against the ray cast of the model so far.  With
    the weighted average every frame stays within 3 mm and 0.1 degrees of the truth (measured: 0.4 mm, 0.04 degrees).
    With the running 50/50 average a surface seen once is ray-cast at half its brightness, the model's intensity steps
    by more than s_colorThres at the edge of what has been seen, and the same loop is 60 mm off on its first tracked
    frame and 593 mm / 25 degrees on the third (measured, not asserted)."""
    errors = closed_loop_cpu(8, WC.rule_weighted)
    assert len(errors) == 7 and None not in errors, errors
    print("closed loop, weighted average: worst", max(e[0] for e in errors), "m", max(e[1] for e in errors), "degrees")
    for k, (dt, da) in enumerate(errors, 1):
        assert dt < 0.003 and da < 0.1, (k, dt, da)


HASH_PARAMS_OFFSETS = dict(m_rigidTransform=0, m_rigidTransformInverse=64, m_hashNumBuckets=128, m_hashBucketSize=132,
                           m_hashMaxCollisionLinkedListSize=136, m_numSDFBlocks=140, m_SDFBlockSize=144, m_virtualVoxelSize=148,
                           m_numOccupiedBlocks=152, m_maxIntegrationDistance=156, m_truncScale=160, m_truncation=164,
                           m_integrationWeightSample=168, m_integrationWeightMax=172, m_streamingVoxelExtents=176,
                           m_streamingGridDimensions=188, m_streamingMinGridPos=200, m_streamingInitialChunkListSize=212,
                           m_colorIntegration=216)


def test_the_switch_is_the_spare_word_and_every_constructor_leaves_it_off():
    """VhHashParams keeps its 224 bytes and every field its offset (the reference's layout; the switch is the spare word
    at 216) in the C header and in the ctypes mirror; make_hash_params and vh_hash_params_from_app_state leave it 0;
    vh_scene_rep_set_color_integration takes 0 and 1 only"""
    from voxelhashing_amd import lib
    names = list(HASH_PARAMS_OFFSETS)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vh_types.h"\nint main(void) {\n'
            + "".join(f'  printf("%zu\\n", offsetof(VhHashParams, {n}));\n' for n in names)
            + '  printf("%zu %d %d\\n", sizeof(VhHashParams), VH_COLOR_RUNNING_AVERAGE, VH_COLOR_WEIGHTED_AVERAGE);\n  return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    assert [int(v) for v in out[:len(names)]] == list(HASH_PARAMS_OFFSETS.values())
    assert out[len(names)].split() == ["224", "0", "1"]
    assert [getattr(T.HashParams, n).offset for n in names] == list(HASH_PARAMS_OFFSETS.values()) and C.sizeof(T.HashParams) == 224
    assert (T.COLOR_RUNNING_AVERAGE, T.COLOR_WEIGHTED_AVERAGE) == (0, 1)

    assert T.make_hash_params(16, 16, 0.04).m_colorIntegration == 0
    assert T.make_hash_params(16, 16, 0.04, weighted_colour=True).m_colorIntegration == 1
    L = lib.load()
    hp = T.HashParams()
    C.memset(C.byref(hp), 0xff, C.sizeof(hp))
    L.vh_hash_params_from_app_state(C.byref(T.AppState()), C.byref(hp))
    assert hp.m_colorIntegration == 0 and hp.m_dummy == 0
    # (no scene without a device: the argument check comes first; with a scene, test_gpu_weighted_colour.py)
    for mode in (0, 1, 2, 0xffffffff):
        assert L.vh_scene_rep_set_color_integration(None, mode) == 4  # VH_ERR_BAD_ARGUMENT
