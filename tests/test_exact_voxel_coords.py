"""The identities behind three short cuts of the device code (vh_device.hpp, vh_ray_lookup.hpp), in numpy's float32 / int32:

  * round_half_away:  (int)(p + copysignf(0.5f, p))  ==  (int)(p + sign(p) * 0.5f), the reference's worldToVirtualVoxelPos,
    with the device's conversion (toward zero, saturating, NaN -> 0);
  * vvp_to_block1:    v >> 3  ==  (v < 0 ? v - 7 : v) / 8, the reference's virtualVoxelPosToSDFBlock, for v >= INT_MIN + 7;
  * TileLookup::slot_of: the slot from 24-bit multiply-adds (v_mul_u32_u24, v_mad_u32_u24) == the slot from 32-bit ones.
"""
import numpy as np

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def f2i(x):
    """v_cvt_i32_f32: toward zero, saturating, NaN -> 0"""
    x = np.asarray(x, dtype=np.float32)
    t = np.trunc(np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=float(INT_MAX), neginf=float(INT_MIN)))
    return np.clip(t, INT_MIN, INT_MAX).astype(np.int64).astype(np.int32)


def round_by_sign(p):
    p = np.asarray(p, dtype=np.float32)
    sign = (np.float32(0.0) < p).astype(np.int32) - (p < np.float32(0.0)).astype(np.int32)
    with np.errstate(invalid="ignore"):
        return f2i(p + sign.astype(np.float32) * np.float32(0.5))


def round_half_away(p):
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return f2i(p + np.copysign(np.float32(0.5), p))


def block_by_division(v):
    """(v < 0 ? v - 7 : v) / 8 with C's division (toward zero), in 64 bits so that the test itself never overflows"""
    v = np.asarray(v, dtype=np.int64)
    w = np.where(v < 0, v - 7, v)
    return (np.sign(w) * (np.abs(w) // 8)).astype(np.int64)


def block_by_shift(v):
    return (np.asarray(v, dtype=np.int32) >> np.int32(3)).astype(np.int64)


def ulps_around(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def test_rounding():
    vals = []
    for x in (0.0, 0.5, 1.0, 1.5, 2.5):
        for y in ulps_around(x):
            vals += [y, -y]
    k = np.concatenate([np.arange(0, 4097), 2 ** np.arange(12, 24), 2 ** np.arange(12, 24) - 1, [2 ** 23 - 2, 2 ** 23 - 1, 2 ** 23]]).astype(np.float64)
    halves = (k + 0.5).astype(np.float32)  # (exact below 2^23; at 2^23 the half is rounded away, as it is on the device)
    rng = np.random.default_rng(7)
    patterns = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    edge = np.array([2.0 ** 31, -2.0 ** 31, np.nextafter(np.float32(2.0 ** 31), np.float32(0)), -np.nextafter(np.float32(2.0 ** 31), np.float32(0)),
                     2.0 ** 32, -2.0 ** 32, 1e-45, -1e-45, 1e-40, -1e-40, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny,
                     np.inf, -np.inf, np.nan, -np.nan, 3.4e38, -3.4e38], dtype=np.float32)
    p = np.concatenate([np.array(vals, dtype=np.float32), halves, -halves, patterns, edge])
    assert (np.signbit(p) & (p == 0.0)).any() and (~np.signbit(p) & (p == 0.0)).any()  # both zeros are among them
    old, new = round_by_sign(p), round_half_away(p)
    bad = np.flatnonzero(old != new)
    assert bad.size == 0, f"{bad.size} operands differ, first {p[bad[0]]!r}: {old[bad[0]]} against {new[bad[0]]}"
    # what the two are for: the halves round away from zero, zero stays, NaN is 0, the ends saturate
    assert round_half_away(np.float32(2.5)) == 3 and round_half_away(np.float32(-2.5)) == -3
    assert round_half_away(np.float32(-0.0)) == 0 and round_half_away(np.float32(np.nan)) == 0
    assert round_half_away(np.float32(-np.inf)) == INT_MIN and round_half_away(np.float32(np.inf)) == INT_MAX


def test_block_division():
    v = np.arange(-70000, 70001, dtype=np.int64)
    assert np.array_equal(block_by_division(v), block_by_shift(v))
    ends = np.array([INT_MIN + 7, INT_MIN + 8, INT_MIN + 9, INT_MIN + 15, INT_MIN + 16, INT_MAX - 8, INT_MAX - 7, INT_MAX - 1, INT_MAX], dtype=np.int64)
    assert np.array_equal(block_by_division(ends), block_by_shift(ends))
    rng = np.random.default_rng(8)
    r = rng.integers(INT_MIN + 7, INT_MAX, size=1 << 20, dtype=np.int64, endpoint=True)
    assert np.array_equal(block_by_division(r), block_by_shift(r))
    # below INT_MIN + 7 the reference's v - 7 does not fit an int: there is no result of it to keep
    assert (np.arange(INT_MIN, INT_MIN + 7, dtype=np.int64) - 7 < INT_MIN).all()


HASH = (0x9E3779, 0x7F4A7D, 0x85EBCB)
M32 = np.uint64(0xFFFFFFFF)
M24 = np.uint64(0xFFFFFF)


def slot_32(b, slots):
    """(bx * c0 + by * c1 + bz * c2) mod 2^32, bits 10 and up"""
    s = np.zeros(len(b), dtype=np.uint64)
    for a in range(3):
        s = (s + (b[:, a].astype(np.int64).astype(np.uint64) & M32) * np.uint64(HASH[a])) & M32
    return (s >> np.uint64(10)) & np.uint64(slots - 1)


def slot_24(b, slots):
    """v_mul_u32_u24 / v_mad_u32_u24: the operands' low 24 bits, the product's low 32, the sum mod 2^32"""
    s = np.zeros(len(b), dtype=np.uint64)
    for a in range(3):
        s = (s + (((b[:, a].astype(np.int64).astype(np.uint64) & M24) * (np.uint64(HASH[a]) & M24)) & M32)) & M32
    return (s >> np.uint64(10)) & np.uint64(slots - 1)


def test_slot_of_24_bit_multiplies():
    r = np.arange(-40, 41, dtype=np.int32)
    near = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(9)
    far = rng.integers(INT_MIN, INT_MAX, size=(1 << 20, 3), dtype=np.int64, endpoint=True).astype(np.int32)
    for slots in (128, 256):  # 2 x VH_TILE_LIST_CAPACITY, 2 x VH_TILE_LIST_CAPACITY_LARGE
        for b in (near, far):
            assert np.array_equal(slot_24(b, slots), slot_32(b, slots))
        # (and the hash does what it is there for: a dense slab of blocks does not land in one run of slots)
        assert len(np.unique(slot_24(near, slots))) == slots
