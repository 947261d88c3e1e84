"""Marching cubes on crafted voxel fields (tests/mc_fields.py), CPU side: the oracle against a float64 restatement of
the extraction, cell by cell, on fields that reach all 254 cube cases, the edge-mask-255 rule, snapped vertices and
cells skipped for an unobserved tap; and the oracle's triangle counts where the threshold comparison is stepped over
its rounding edge ulp by ulp.  tests/test_gpu_marching_cubes_cases.py holds the kernels to the oracle on the same
fields, tests/test_reference_pinning_kernels.py the oracle to the reference's own code."""
import numpy as np
import pytest

import mc_fields as F


def oracle_scene(O, hp, cp, descs, blocks):
    o = O.OracleScene(hp, cp)
    assert o.stream_in(descs, blocks) == 0
    return o


@pytest.fixture(scope="module")
def fields(oracle_lib):
    """(parameter set, field name) -> the field, the oracle's soup of it, the float64 reference and the soup's
    triangles matched to the reference's; made once"""
    cache = {}

    def get(name, which):
        if (name, which) in cache:
            return cache[(name, which)]
        hp, cp, mp, vs = F.config(name)
        thres = float(mp.m_threshMarchingCubes)
        if which == "planted":
            descs, blocks = F.planted(F.NEAR, vs, np.float32(10.0) * vs)
        else:
            descs, blocks = F.random_field(F.block_ids(), which, thres, **F.RANDOM)
        tris, n = oracle_scene(oracle_lib, hp, cp, descs, blocks).extract_iso_surface(mp)
        assert n == len(tris)
        ref = F.reference(descs, blocks, vs, mp)
        cell_of, tied = F.group_by_cell(tris, ref, vs)
        assert np.all(cell_of >= 0), "a triangle without a cell"
        count = np.bincount(cell_of, minlength=len(ref["cell"]))
        # the k-th triangle of a cell in the buffer is the k-th of the case's list (the oracle emits them in order)
        order = np.argsort(cell_of, kind="stable")
        srt = cell_of[order]
        start = np.concatenate([[0], np.flatnonzero(srt[1:] != srt[:-1]) + 1]) if len(srt) else np.zeros(0, np.int64)
        rank = np.empty(len(srt), np.int64)
        rank[order] = np.arange(len(srt)) - np.repeat(start, np.diff(np.concatenate([start, [len(srt)]])))
        first = np.concatenate([[0], np.cumsum(ref["ntri"])[:-1]])
        cache[(name, which)] = dict(hp=hp, mp=mp, vs=vs, thres=thres, descs=descs, blocks=blocks, tris=tris, ref=ref, cell_of=cell_of,
                                    count=count, rank=rank, first=first, tied=tied)
        return cache[(name, which)]

    return get


@pytest.mark.parametrize("name", ["P2", "P4"])
def test_planted_field_reaches_every_case_and_counts_agree_per_cell(fields, name):
    x = fields(name, "planted")
    ref, dec = x["ref"], x["ref"]["decided"]
    undecided = float((~dec).mean())
    print(f"{name}: {len(x['tris'])} triangles, {int(ref['valid'].sum())} cells with eight samples, {int(ref['emits'].sum())} emit, "
          f"undecided {int((~dec).sum())} of {len(dec)} ({undecided:.4%}), triangles that needed the colour {x['tied']}")
    assert undecided <= 0.01
    assert np.array_equal(x["count"][dec], ref["ntri"][dec])
    assert len(x["tris"]) == 18626
    live = dec & ref["valid"]
    hist = np.bincount(ref["case"][live], minlength=256)
    assert np.all(hist[1:255] >= 2), "a cube case the field does not reach twice"
    # the reference's edgeTable == 255 rule: cases 85 and 170 occur and emit nothing, 4 triangles each by the tables
    for c in (85, 170):
        at = live & (ref["case"] == c)
        assert at.sum() > 0 and not ref["emits"][at].any() and x["count"][at].sum() == 0
    dropped = int((live & np.isin(ref["case"], (85, 170))).sum())
    assert dropped == 226 and len(x["tris"]) == 18626 == int(ref["ntri"].sum())
    # ... among them the two cells the builder planted as such
    planted = [p for p in range(256) if F.case_of_pattern(p) in (85, 170)]
    assert len(planted) == 2
    for p in planted:
        v = np.array(F.NEAR) * F.B + F.pattern_voxel(p)
        i = int(np.flatnonzero(np.all(ref["cell"] == v, axis=1))[0])
        assert live[i] and ref["case"][i] == F.case_of_pattern(p) and x["count"][i] == 0
    # and every planted pattern gives its case
    for p in range(256):
        v = np.array(F.NEAR) * F.B + F.pattern_voxel(p)
        i = int(np.flatnonzero(np.all(ref["cell"] == v, axis=1))[0])
        assert ref["valid"][i] and ref["case"][i] == F.case_of_pattern(p)


@pytest.mark.parametrize("name,seed", F.RANDOM_SEEDS)
def test_random_field_counts_agree_per_cell(fields, name, seed):
    x = fields(name, seed)
    ref, dec = x["ref"], x["ref"]["decided"]
    undecided = float((~dec).mean())
    snaps = [int(((ref["tri_snap"] == k) & dec[ref["tri_cell"]][:, None]).sum()) for k in (1, 2)]
    skipped = int((ref["holed"] & ~ref["valid"]).sum())
    cases = len(set(ref["case"][ref["emits"] & dec].tolist()))
    print(f"{name} seed {seed}: {len(x['tris'])} triangles, {cases} cases, snapped vertices {snaps}, cells skipped for a weight-0 tap "
          f"{skipped}, undecided {int((~dec).sum())} of {len(dec)} ({undecided:.4%}), triangles that needed the colour {x['tied']}")
    assert undecided <= 0.01
    assert np.array_equal(x["count"][dec], ref["ntri"][dec])
    assert cases >= 240 and min(snaps) > 0 and skipped > 1000 and len(x["tris"]) > 5000


@pytest.mark.parametrize("name,which", [("P2", "planted"), ("P4", "planted")] + list(F.RANDOM_SEEDS))
def test_vertex_positions(fields, name, which):
    """Every oracle vertex of a decided cell within tol of the float64 one:
        tol = |p| 2^-22 + voxel * 4 eps_d / |d2 - d1|
    |p| 2^-22: the cell centre, the corner and the interpolated position are a rounding each (2^-24 |p|), and the
    corner difference p2 - p1 is within 2^-24 |p| of one voxel.  The second term is the change of
    mu = -d1 / (d2 - d1) when both samples move by eps_d (mc_fields.sample_error_bound): |d mu| <= eps_d / |gap| +
    |d1| 2 eps_d / gap^2 <= 3 eps_d / |gap| since |d1| <= |gap| on a crossing edge; the division and product round
    once more each, far below the fourth eps_d / |gap|.  On the planted field |d2 - d1| is amplitude / 4 on every
    edge; on the random fields edges with |d2 - d1| < thres / 64 are exempt (at most 5 % of the vertices)."""
    x = fields(name, which)
    ref = x["ref"]
    cell_of = x["cell_of"]
    good = ref["decided"][cell_of] & (x["count"][cell_of] == ref["ntri"][cell_of])
    at = x["first"][cell_of[good]] + x["rank"][good]
    want, gap, snap = ref["tri_pos"][at], ref["tri_gap"][at], ref["tri_snap"][at]
    got = x["tris"]["v"]["p"][good].astype(np.float64)
    exempt = (gap < x["thres"] / 64.0) & (snap == 0)
    if which == "planted":
        assert np.allclose(gap, 10.0 * float(x["vs"]) / 4.0, rtol=1e-6) and not exempt.any() and good.all()
    with np.errstate(divide="ignore"):
        tol = np.abs(want).max(axis=-1) * 2.0 ** -22 + float(x["vs"]) * np.where(snap == 0, 4.0 * ref["margin"] / gap, 0.0)
    err = np.abs(got - want).max(axis=-1)
    print(f"{name} {which}: {int((~exempt).sum())} vertices checked, exempt share {float(exempt.mean()):.4%}, largest error / tol "
          f"{float((err / tol)[~exempt].max()):.3f}")
    assert exempt.mean() <= 0.05
    assert np.all(err[~exempt] <= tol[~exempt])
    # colours: the own voxel's bytes / 255 on every vertex
    want_c = (ref["color"][cell_of].astype(np.float32) / np.float32(255.0))[:, None, :]
    assert np.array_equal(x["tris"]["v"]["c"], np.broadcast_to(want_c, x["tris"]["v"]["c"].shape))


@pytest.mark.parametrize("name", ["P2", "P4"])
@pytest.mark.parametrize("origin", [F.NEAR, F.FAR])
def test_threshold_sweep(oracle_lib, name, origin):
    """amplitude = 4 thres (1 + k 2^-22): |d_k| + |d_l| on a crossing edge is thres (1 + k 2^-22) up to rounding, so
    hundreds of cells flip per ulp; far from the origin the trilinear weights are no longer 1/2 and other cells flip"""
    hp, cp, mp, vs = F.config(name)
    got = []
    for k in F.SWEEP_KS:
        descs, blocks = F.planted(origin, vs, F.sweep_amplitude(mp.m_threshMarchingCubes, k))
        got.append(oracle_scene(oracle_lib, hp, cp, descs, blocks).extract_iso_surface(mp)[1])
    print(name, origin, got)
    assert tuple(got) == F.SWEEP_COUNTS[origin]
