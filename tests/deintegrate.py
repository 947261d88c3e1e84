"""The frame de-integration restated in numpy on canonical forms (DESIGN.md section 4 "Frame de-integration").  TEST
INFRASTRUCTURE ONLY.

A scene is (positions [n, 3] int32, voxels [n, 512] VOXEL_DTYPE), as in tests/scene_merge.py and tests/scene_cut.py.  A
frame is (depth [H, W] float32, colour [H, W, 4] float32 or None).  deintegrate() returns the scene afterwards, sorted by
position, the positions of the freed blocks and the counts that do not depend on the order in which the device's deletes
ran.

  * the observation of voxel l of the block at pos, pi = 8 pos + (l & 7, (l >> 3) & 7, l >> 6) in wrapping int32, is what
    the integrate pass hands to combineVoxel: every operation below is one float32 operation, in the pass's order;
  * the take-out of (o, co, wo) from (s, c, w): nothing without an observation or with w == 0; zero bytes for wo >= w;
    else w' = w - wo, s' = (s w - o wo) / w' in float32, the colour kept (running average) or per channel
    clamp(floor((2 (c w - co wo) + w') / (2 w')), 0, 255) in integers;
  * a block is processed iff isSDFBlockInCameraFrustumApprox holds at the frame's pose; a processed block without a
    voxel of weight > 0 afterwards leaves the scene.
"""
import numpy as np

from oracle import oracle as O
from scene_cut import voxel_coords
from scene_merge import sort_scene
from voxelhashing_amd import vhtypes as T

V = T.SDF_BLOCK_VOXELS
COUNT_KEYS = ("blocks_in", "processed", "changed", "freed", "voxels_changed", "voxels_reset", "voxels_at_cap", "status")
MINF = np.float32(-np.inf)
f32 = np.float32


def f2i(v):
    """float32 -> int32, toward zero, saturating, NaN -> 0 (v_cvt_i32_f32), as int64"""
    v = np.asarray(v, np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(np.trunc(np.clip(v, -2.0 ** 31, 2.0 ** 31)), -2 ** 31, 2 ** 31 - 1).astype(np.int64)


def f2uc(v):
    """float32 -> byte: clamped to [0, 255] (a NaN gives 0), then toward zero"""
    v = np.fmin(np.fmax(np.asarray(v, np.float32), f32(0)), f32(255))
    return np.trunc(v).astype(np.uint8)


def mat_mul_p(m, x, y, z):
    """float4x4 * (x, y, z, 1), rows 0..2, summed left to right"""
    m = np.asarray(m, np.float32).reshape(16)
    return tuple(((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] * f32(1) for r in range(3))


def observe(frame, pose, hp, cp, positions, with_depth=False):
    """the observations the frame makes of every voxel of the blocks at `positions` -> VOXEL_DTYPE [n, 512]; weight 0: no
    observation (an observation weighs at least 1).  with_depth: -> (the observations, the depth each was made at)"""
    depth_map, colour_map = frame
    inv = O.mat4_inverse(np.asarray(pose, np.float32))
    positions = np.ascontiguousarray(positions, np.int32).reshape(-1, 3)
    out = np.zeros((len(positions), V), T.VOXEL_DTYPE)
    if len(positions) == 0 or colour_map is None:  # (without a colour map the colour is MINF: the gate fails)
        return (out, np.zeros(out.shape, np.float32)) if with_depth else out
    vs = f32(hp.m_virtualVoxelSize)
    pi = voxel_coords(positions).astype(np.float32)
    with np.errstate(all="ignore"):
        px, py, pz = mat_mul_p(inv, pi[..., 0] * vs, pi[..., 1] * vs, pi[..., 2] * vs)
        sx = f2i((px * f32(cp.fx) / pz + f32(cp.mx)) + f32(0.5)) & 0xFFFFFFFF
        sy = f2i((py * f32(cp.fy) / pz + f32(cp.my)) + f32(0.5)) & 0xFFFFFFFF
        W, H = int(cp.m_imageWidth), int(cp.m_imageHeight)
        inside = (sx < W) & (sy < H)
        pix = np.where(inside, sy * W + sx, 0)
        depth = np.ascontiguousarray(depth_map, np.float32).reshape(-1)[pix]
        colour = np.ascontiguousarray(colour_map, np.float32).reshape(-1, 4)[pix]
        ok = inside & (colour[..., 0] != MINF) & (depth != MINF) & (depth < f32(hp.m_maxIntegrationDistance))
        zero_one = (depth - f32(cp.m_sensorDepthWorldMin)) / (f32(cp.m_sensorDepthWorldMax) - f32(cp.m_sensorDepthWorldMin))
        sdf = depth - pz
        trunc = f32(hp.m_truncation) + f32(hp.m_truncScale) * depth
        ok &= sdf > -trunc
        sdf = np.where(sdf >= f32(0), np.fmin(trunc, sdf), np.fmax(-trunc, sdf))
        weight = f2uc(np.fmax(f32(hp.m_integrationWeightSample) * f32(1.5) * (f32(1) - zero_one), f32(1)))
        rgb = f2uc(f32(255) * colour[..., :3])
    for a in (px, sdf, trunc, zero_one):
        assert a.dtype == np.float32
    out["sdf"] = np.where(ok, sdf, f32(0))
    out["color"] = np.where(ok[..., None], rgb, np.uint8(0))
    out["weight"] = np.where(ok, weight, np.uint8(0))
    return (out, np.where(ok, depth, f32(0))) if with_depth else out


def applies(stored, obs):
    """where the take-out changes a voxel: it has an observation and weight > 0"""
    return (stored["weight"] > 0) & (obs["weight"] > 0)


def take_out(hp, stored, obs):
    """the per-voxel rule on two VOXEL_DTYPE arrays of one shape -> the voxels afterwards"""
    stored, obs = np.ascontiguousarray(stored, T.VOXEL_DTYPE), np.ascontiguousarray(obs, T.VOXEL_DTYPE)
    out = stored.copy()
    hit = applies(stored, obs)
    w, wo = stored["weight"].astype(np.int64), obs["weight"].astype(np.int64)
    reset = hit & (wo >= w)
    sub = hit & ~reset
    out[reset] = np.zeros((), T.VOXEL_DTYPE)
    wn = np.where(sub, w - wo, 1)
    with np.errstate(all="ignore"):
        fw, fwo, fwn = w.astype(np.float32), wo.astype(np.float32), wn.astype(np.float32)
        sdf = (stored["sdf"] * fw - obs["sdf"] * fwo) / fwn
    assert sdf.dtype == np.float32
    # (written through the bits: a NaN's payload is the device's business only where the test says so)
    new_sdf = out["sdf"].copy()
    new_sdf[sub] = sdf[sub]
    out["sdf"] = new_sdf
    new_w = out["weight"].copy()
    new_w[sub] = wn[sub].astype(np.uint8)
    out["weight"] = new_w
    if hp.m_colorIntegration != 0:
        n = stored["color"].astype(np.int64) * w[..., None] - obs["color"].astype(np.int64) * wo[..., None]
        c = np.clip((2 * n + wn[..., None]) // (2 * wn[..., None]), 0, 255).astype(np.uint8)  # (// floors)
        new_c = out["color"].copy()
        new_c[sub] = c[sub]
        out["color"] = new_c
    return out


def block_in_frustum(pose, hp, cp, positions):
    """isSDFBlockInCameraFrustumApprox at the pose, in float32 -> [n] bool"""
    inv = O.mat4_inverse(np.asarray(pose, np.float32))
    positions = np.ascontiguousarray(positions, np.int32).reshape(-1, 3)
    vs = f32(hp.m_virtualVoxelSize)
    base = (positions.view(np.uint32) * np.uint32(8)).view(np.int32).astype(np.float32)
    off = vs * f32(0.5) * (f32(8) - f32(1))
    with np.errstate(all="ignore"):
        w = [base[:, k] * vs + off for k in range(3)]
        pcx, pcy, pcz = mat_mul_p(inv, w[0], w[1], w[2])
        px = pcx * f32(cp.fx) / pcz + f32(cp.mx)
        py = pcy * f32(cp.fy) / pcz + f32(cp.my)
        wm1, hm1 = f32(cp.m_imageWidth) - f32(1), f32(cp.m_imageHeight) - f32(1)
        x = (f32(2) * px - wm1) / wm1
        y = (hm1 - f32(2) * py) / hm1
        z = (pcz - f32(cp.m_sensorDepthWorldMin)) / (f32(cp.m_sensorDepthWorldMax) - f32(cp.m_sensorDepthWorldMin))
        x, y, z = x * f32(0.95), y * f32(0.95), z * f32(0.95)
        assert x.dtype == np.float32 and z.dtype == np.float32
        return ~((x < f32(-1)) | (x > f32(1)) | (y < f32(-1)) | (y > f32(1)) | (z < f32(0)) | (z > f32(1)))


def deintegrate(scene, frame, pose, hp, cp, count_only=False):
    """scene: (positions, voxels) -> dict(positions, voxels: the scene afterwards; freed: positions; counts: COUNT_KEYS
    by name; at_cap: [n, 512] bool over the sorted scene that came in)"""
    pos, vox = sort_scene(*scene)
    processed = block_in_frustum(pose, hp, cp, pos) if len(pos) else np.zeros(0, bool)
    obs = observe(frame, pose, hp, cp, pos)
    obs[~processed] = np.zeros((), T.VOXEL_DTYPE)
    hit = applies(vox, obs)
    after = take_out(hp, vox, obs)
    freed = processed & ~(after["weight"] > 0).any(axis=1)
    at_cap = hit & (vox["weight"] == hp.m_integrationWeightMax)
    counts = dict(blocks_in=len(pos), processed=int(processed.sum()), changed=int(hit.any(axis=1).sum()), freed=int(freed.sum()),
                  voxels_changed=int(hit.sum()), voxels_reset=int((hit & (obs["weight"] >= vox["weight"])).sum()), voxels_at_cap=int(at_cap.sum()),
                  status=0)
    if count_only:
        return dict(positions=pos, voxels=vox, freed=np.zeros((0, 3), np.int32), counts=counts, at_cap=at_cap)
    return dict(positions=np.ascontiguousarray(pos[~freed]), voxels=np.ascontiguousarray(after[~freed]), freed=pos[freed], counts=counts, at_cap=at_cap)


def assert_counts(got, want, what=""):
    """the device's counts against the restatement's, on the fields no schedule changes"""
    for k in COUNT_KEYS:
        assert got[k] == want[k], f"{what}: {k} is {got[k]}, the restatement says {want[k]} ({ {q: got[q] for q in COUNT_KEYS} } vs {want})"


def sdf_bound(hp, depth_max, w_total, w_a):
    """8 * 2^-24 * T * W / w_A with T the truncation at depth_max"""
    t = float(hp.m_truncation) + float(hp.m_truncScale) * float(depth_max)
    return 8.0 * 2.0 ** -24 * t * np.asarray(w_total, np.float64) / np.asarray(w_a, np.float64)
