"""Reference for the weighted colour average (HashParams.m_colorIntegration = 1).  TEST INFRASTRUCTURE ONLY.

The oracle knows combineVoxel's running 50/50 colour average only, and colour is all that the two rules differ in.  So the
reference is the oracle for the block set, sdf, weights and heap, plus the colour rule in numpy:

    colour = floor((2 n + d) / (2 d)),  n = c0 w0 + c1 w1,  d = w0 + w1     (per channel)

which is uchar((c0 w0 + c1 w1) / (w0 + w1) + 0.5f) in float32 (test_weighted_colour.py checks the identity for every
n <= 255 d, d in 1..510).  Per voxel and frame the rule needs w0 (the oracle's weight before the frame), and w1 and c1 (what
this frame observed).  The last two come from a probe: a second OracleScene that holds the main scene's table and heap
from before the frame with every voxel cleared, garbage collection off, integrating the same pose and depth.  Its weight
after the frame is w1 (0: the voxel was not updated).  Its colour image holds the pixel index, seven bits per channel as
the even value 2 v: a cleared voxel blended 50/50 with 2 v (or with 2 v - 1, where 255 * (2 v / 255) falls short) reads
back v, so the probe's colour bytes name the pixel a voxel took its observation from, and c1 is that pixel's colour of the
real frame, through f2uc(255 c).

WeightedColourScene keeps the colours by block position, drops the positions the main table no longer holds after the
frame (garbage collection, so that and starving need no special case) and writes its colours over the oracle's in the
oracle's voxel array: after integrate() the oracle scene IS the expected scene, for canonical.assert_same_scene and for
the oracle's ray cast.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
from voxelhashing_amd import vhtypes as T

MINF = np.float32(-np.inf)
V = T.SDF_BLOCK_VOXELS


def rule_weighted(c0, w0, c1, w1):
    """integer form of the weighted average; arrays of equal shape (or broadcastable), w0 + w1 >= 1"""
    c0, w0, c1, w1 = (np.asarray(a).astype(np.int64) for a in (c0, w0, c1, w1))
    n, d = c0 * w0 + c1 * w1, w0 + w1
    return ((2 * n + d) // (2 * d)).astype(np.uint8)


def rule_weighted_float32(c0, w0, c1, w1):
    """the definition: (uchar)((c0 w0 + c1 w1) / (w0 + w1) + 0.5f), float32 with IEEE division"""
    f = np.float32
    c0, w0, c1, w1 = (np.asarray(a).astype(f) for a in (c0, w0, c1, w1))
    return ((c0 * w0 + c1 * w1) / (w0 + w1) + f(0.5)).astype(np.uint8)


def rule_running(c0, w0, c1, w1):
    """combineVoxel's 50/50 average in integer form (tests/test_oracle_math.py)"""
    return ((np.asarray(c0).astype(np.int64) + np.asarray(c1).astype(np.int64) + 1) >> 1).astype(np.uint8)


def f2uc(x):
    """(uchar) of a float clamped to [0, 255], as integrateDepthMapKernel converts 255 * colour (fmaxf / fminf drop a NaN)"""
    x = np.asarray(x, np.float32)
    return np.fmin(np.fmax(x, np.float32(0.0)), np.float32(255.0)).astype(np.uint8)


def index_image(color):
    """the probe's colour image for a frame whose colour image is `color` (H, W, 4): the pixel index in even bytes, and
    no colour where the frame has none (the pass skips a pixel whose red is MINF)"""
    H, W = color.shape[:2]
    assert H * W <= 1 << 21
    p = np.arange(H * W, dtype=np.uint32).reshape(H, W)
    out = np.ones((H, W, 4), np.float32)
    for ch in range(3):
        out[..., ch] = (2 * ((p >> (7 * ch)) & 127)).astype(np.float32) / np.float32(255.0)
    out[color[..., 0] == MINF, :3] = MINF
    return out


def _copy_array(dst_scene, src_scene, field, dtype, count):
    dst_scene.array(field, dtype, count)[:] = src_scene.array(field, dtype, count)


class WeightedColourScene:
    """An OracleScene (self.o) whose colours follow `rule` (rule_weighted by default).  integrate() as OracleScene's."""

    def __init__(self, hp, cp, rp=None, options=None, rule=rule_weighted):
        self.o = O.OracleScene(hp, cp, rp, options)
        probe_opt = O._copy_struct(self.o.opt)
        probe_opt.s_garbageCollectionEnabled = 0
        self.probe = O.OracleScene(hp, cp, rp, probe_opt)
        self.rule = rule
        self.colours = {}   # block position -> [512, 3] bytes
        self.last = None    # what the last frame's checks want to look at

    def close(self):
        self.o.close()
        self.probe.close()

    def _blocks(self, scene):
        """{position: block id} of a scene's table"""
        t = scene.hash_table()
        occ = t["ptr"] != T.FREE_ENTRY
        return {tuple(int(v) for v in p): int(q) // V for p, q in zip(t["pos"][occ], t["ptr"][occ])}

    def set_colours(self, positions, colours):
        """blocks that came into the table by another way than integrate() (stream-in): their colours as stored"""
        for p, c in zip(positions, colours):
            self.colours[tuple(int(v) for v in p)] = np.array(c, np.uint8).reshape(V, 3)

    def observe(self, pose, depth, color):
        """the probe's frame on the main scene's table as it is now -> (blocks of the probe, w1 [blocks, 512], c1 [blocks, 512, 3])"""
        o, pr = self.o, self.probe
        nb, ne = o.hp.m_numSDFBlocks, o.num_entries()
        _copy_array(pr, o, "d_hash", T.HASH_ENTRY_DTYPE, ne)
        _copy_array(pr, o, "d_heap", np.uint32, nb)
        _copy_array(pr, o, "d_heapCounter", np.uint32, 1)
        pr.sdf_blocks().view(np.uint64)[:] = 0
        C.memmove(C.byref(pr.hp), C.byref(o.hp), C.sizeof(o.hp))
        pr.integrate(pose, depth, index_image(color))
        vox = pr.sdf_blocks().reshape(nb, V)
        w1 = vox["weight"].astype(np.int64)
        idx = vox["color"].astype(np.int64)
        pix = idx[..., 0] | (idx[..., 1] << 7) | (idx[..., 2] << 14)
        c1 = f2uc(np.float32(255.0) * np.ascontiguousarray(color, np.float32).reshape(-1, 4)[:, :3])[pix]
        return self._blocks(pr), w1, c1

    def integrate(self, pose, depth, color):
        o = self.o
        nb = o.hp.m_numSDFBlocks
        before = self._blocks(o)
        w0_all = o.sdf_blocks().reshape(nb, V)["weight"].astype(np.int64).copy()
        seen, w1_all, c1_all = self.observe(pose, depth, color)
        frame = int(o.frames.value)
        o.integrate(pose, depth, color)
        after = self._blocks(o)
        vox = o.sdf_blocks().reshape(nb, V)
        updated = 0
        for pos, bid in seen.items():
            w1 = w1_all[bid]
            hit = w1 > 0
            if not hit.any():
                continue
            # (the probe allocates as the main scene does, from the same table and heap: the same block ids)
            w0 = w0_all[bid] if pos in before else np.zeros(V, np.int64)
            assert pos not in before or before[pos] == bid
            c0 = self.colours.get(pos)
            if c0 is None:
                c0 = np.zeros((V, 3), np.uint8)
            new = c0.copy()
            new[hit] = self.rule(c0[hit], w0[hit][:, None], c1_all[bid][hit], w1[hit][:, None])
            self.colours[pos] = new
            updated += int(hit.sum())
        self.colours = {p: c for p, c in self.colours.items() if p in after}
        starved = bool(o.opt.s_garbageCollectionEnabled and frame > 0 and o.opt.s_garbageCollectionStarve != 0
                       and frame % o.opt.s_garbageCollectionStarve == 0)
        self.last = dict(before=before, after=after, seen=seen, w0=w0_all, w1=w1_all, starved=starved, updated=updated,
                         oracle_colours={p: vox["color"][b].copy() for p, b in after.items()})
        # the colours of the rule over the oracle's own
        for pos, bid in after.items():
            c = self.colours.get(pos)
            if c is not None:
                vox["color"][bid] = c

    def state(self):
        return self.o.state()

    def render(self, pose):
        return self.o.render(pose)
