"""The reference side of tests/special_rays.py, without a GPU: on every family the oracle's brute force equals the oracle's BVH in every bit, and agrees with the independent
float64 formulation on all decided rays (hit / miss, ids, distance within rtol 2e-5 + atol 1e-6, u and v within 5e-4: test_independent_f64.py's figures).  The
preconditions are asserted here, so that tests/test_special_rays.py can neither pass vacuously nor fail for the reference's own reasons."""
import numpy as np
import pytest

import special_rays as S


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _reference_is_consistent(c, name):
    fam, brute, j = c.families[name], c.closest[name], c.judged[name]
    bvh = c.oracle.intersect_closest(fam.rays)
    for f in S.FIELDS:
        bad = np.flatnonzero(_bits(bvh[f]) != _bits(brute[f]))
        assert len(bad) == 0, f"{name} {f}: the oracle's BVH and its brute force differ for {len(bad)} rays, first {bad[0]} ({fam.tags[bad[0]]}): {bvh[bad[0]]} != {brute[bad[0]]}"
    assert np.array_equal(c.oracle.intersect_any(fam.rays), c.occluded[name]), f"{name}: any-hit, BVH against brute force"
    # (any-hit and closest hit see the same interval: inclusive at both ends)
    assert np.array_equal(c.occluded[name] == 1, brute["type"] == 1), name
    return S.assert_matches_f64(c.tris, j, brute, name, S.judged_mask(name, fam))


@pytest.mark.parametrize("two_level", [False, True], ids=["flat", "two_level"])
def test_families_on_the_hostile_scene(mrt, orc, two_level):
    c = S.case(mrt, orc, two_level)
    assert c.oracle.triangles == len(c.tris) == 2834
    decided_hits = {name: _reference_is_consistent(c, name) for name in ("F1", "F2", "F3", "F4")}
    print(decided_hits)

    f1, j1 = c.families["F1"], c.judged["F1"]
    assert len(f1.rays) == 2240 and len(set(f1.tags)) == 56
    nz = S.carries_neg_zero(f1.rays)
    assert nz.sum() == 1200
    assert j1["decided"].mean() >= 0.9 and j1["hit"].mean() > 0.6
    assert (j1["hit"] & nz).sum() >= 1000, (j1["hit"] & nz).sum()

    f2 = c.families["F2"]
    d2 = f2.rays[:, 4:7]
    assert (d2 != 0).all() and (np.abs(d2) < 1e-18).any(1).all() and set(f2.tags) == set(S.TINY)
    assert decided_hits["F2"] >= 100
    for tag in S.TINY:          # every value, either side of the clamp, is judged on hits
        assert (c.judged["F2"]["decided"] & c.judged["F2"]["hit"] & (f2.tags == tag)).sum() >= 100, tag

    f3, j3 = c.families["F3"], c.judged["F3"]
    assert decided_hits["F3"] >= 100
    in_plane = f3.tags == "in_plane"
    assert (f3.rays[in_plane, 1] == 0).all() and (f3.rays[in_plane, 5] == 0).all()
    floor = c.closest["F3"]["instance_id"] == 0
    assert not (floor & in_plane & (c.closest["F3"]["type"] == 1)).any(), "the floor's determinant is 0 for a ray in its plane"
    assert (j3["decided"] & j3["hit"] & in_plane).sum() >= 100, "what crosses the floor's plane is hit by the rays that lie in it"
    assert S.carries_neg_zero(f3.rays).sum() >= 0.5 * len(f3.rays)


@pytest.mark.parametrize("two_level", [False, True], ids=["flat", "two_level"])
def test_interval_edges_are_inclusive_at_both_ends(mrt, orc, two_level):
    """F4 by the oracle's brute force, which defines the answer: a hit at the float32 distance t is inside [min_distance, max_distance] exactly when min <= t <= max"""
    c = S.case(mrt, orc, two_level)
    fam, rec, occ = c.families["F4"], c.closest["F4"], c.occluded["F4"]
    n = S.F4_BASE
    assert len(fam.rays) == n * len(S.F4_CASES)
    by = {name: rec[fam.tags == name] for name in S.F4_CASES}
    base = by["base"]
    assert (fam.tags.reshape(len(S.F4_CASES), n) == np.array(S.F4_CASES)[:, None]).all() and len(base) == n >= 100
    assert (base["type"] == 1).all() and S.carries_neg_zero(fam.rays[:n]).sum() >= 20
    for name in ("max=t", "max=t+", "min=t", "min=t-", "min=max=t"):          # t is inside: the very same record
        for f in S.FIELDS:
            assert np.array_equal(_bits(by[name][f]), _bits(base[f])), (name, f)
    for name in ("max=t-", "max=0", "min>max"):                               # nothing can be inside
        assert (by[name]["type"] != 1).all(), name
    beyond = by["min=t+"]                                                       # the next surface, or nothing: never the base hit again
    hit = beyond["type"] == 1
    assert 20 <= hit.sum() and (beyond["distance"][hit] > base["distance"][hit]).all()
    assert np.array_equal(occ == 1, rec["type"] == 1)


def test_instance_induced_negative_zero(mrt, orc):
    c = S.case_f5(mrt, orc)
    fam, j, pairs = c.families["F5"], c.judged["F5"], c.pairs
    shared = mrt.flatten_scene(c.scene, share=True)
    assert [e[4] for e in shared] == [-1, -1, 1, 1, 1], "three rotated instances of one sphere"
    assert sum(np.asarray(idx).size // 3 for idx, _ in shared[1][3]) > 8, "at 8 triangles or fewer the instance is walked as packets and no BLAS node is ever tested"
    assert _reference_is_consistent(c, "F5") >= 100
    assert not S.carries_neg_zero(fam.rays).any()
    assert not pairs[:, :2].any() and pairs[:, 2:].any(0).all(), "every rotated instance turns some +0 ray into a -0 one; the unrotated one none"
    inst = np.where(j["hit"], c.tris.ids[np.maximum(j["tri"], 0), 0], -1)
    on_it = sum(int((pairs[:, k] & j["decided"] & (inst == k)).sum()) for k in range(pairs.shape[1]))
    assert pairs.sum() >= 20 and on_it >= 20, (pairs.sum(), on_it)
    # the example of the finding: straight down onto the instance turned by 200 degrees
    rows = S.world_to_object_rows(mrt, shared[2][2])
    dd = S.object_direction(rows, np.array([[0.0, -1.0, 0.0]], np.float32))[0]
    assert S.neg_zero(dd).any() and dd[1] < 0, dd
