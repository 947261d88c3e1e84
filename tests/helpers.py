"""shared helpers of the parity tests"""
import numpy as np

from voxelhashing_amd import synth, vhtypes as T


def small_config(width=160, height=120, params="P4", num_buckets=1 << 14, num_sdf_blocks=1 << 13, **hp_over):
    ps = dict(synth.PARAM_SETS[params])
    ps.update(hp_over)
    hp = T.make_hash_params(num_buckets, num_sdf_blocks, **ps)
    cp = T.make_depth_camera_params(width, height)
    rp = T.make_raycast_params(hp, cp)
    return hp, cp, rp


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_maps_equal(got, want, what=""):
    """bit-exact comparison of raycast output maps (depth / depth4 / normals / colors)"""
    for k in ("depth", "depth4", "colors", "normals"):
        g, w = bits(got[k]), bits(want[k])
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            i = tuple(bad[0])
            raise AssertionError(f"{what}: map '{k}' differs at {len(bad)} elements, first {i}: got {got[k][i]!r} want {want[k][i]!r}")


MINF = np.float32(-np.inf)


def make_depth(w, h, seed, holes=0.1):
    """a smooth depth image with noise, a depth step in its bottom fifth and holes (MINF)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    d = (1.5 + 0.5 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + 0.02 * rng.standard_normal((h, w))).astype(np.float32)
    d[yy > 0.8 * h] += np.float32(1.0)
    d[rng.random((h, w)) < holes] = MINF
    return d


def make_color_rgbx(w, h, seed):
    """random RGBX bytes, 5 % black (invalid), alpha 0 / 128 / 255"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    c[rng.random((h, w)) < 0.05, :3] = 0
    c[..., 3] = rng.choice(np.array([0, 128, 255], dtype=np.uint8), size=(h, w))
    return c


def stream_out_replay(scene, hash_of, leaves=None):
    """Stream-out pass 1 over every entry of an oracle.OracleScene with radius 0 (every live block leaves; or, with
    leaves(pos) -> bool, the blocks it says), replayed slot by slot with the oracle's single operations on that scene.  -> (the oracle's heap pushes in order, the
    reference's, the extra ids): the reference's list branch pushes again after deleteHashEntryElement, the id
    ptr / 512 of what the slot holds after the delete."""
    want_o, want_r, extras = [], [], []
    table = scene.hash_table()
    for i in range(scene.num_entries()):
        e = table[i].copy()
        if e["ptr"] == T.FREE_ENTRY or (leaves is not None and not leaves(e["pos"])):
            continue
        own = int(e["ptr"]) // T.SDF_BLOCK_VOXELS
        if e["offset"] != 0 or hash_of(e["pos"]) != i // T.HASH_BUCKET_SIZE:
            if scene.delete_block(e["pos"]):  # deleteHashEntryElement pushes the entry's block
                extra = int(np.uint32(np.int32(table[i]["ptr"]))) // T.SDF_BLOCK_VOXELS
                extras.append(extra)
                want_o.append(own)
                want_r += [own, extra]
        else:
            table[i]["ptr"] = T.FREE_ENTRY
            table[i]["offset"] = 0
            table[i]["pos"] = 0
            want_o.append(own)
            want_r.append(own)
    return want_o, want_r, extras
