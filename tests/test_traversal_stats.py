"""DeviceScene.traversal_stats (mrt_debug_traversal_stats, k_query_stats): the one-ray-per-lane walks with their counters compiled in, the only instantiation of STATS
(DESIGN.md §10s).  Two coincident 16 x 16 grids of quads — every hit is a tie of two triangles at one distance, every any-hit ray ends at its first — committed on
the 8-wide and on the rope layout; 250 rays (the fourth wave is partial), among them rays that miss the sheet, rays whose min_distance lies before the hit and rays
whose min_distance lies behind it.

Exact: words 0, 1, 2, 3, 6, 7 of every row (node visits, leaf visits, triangle tests, hit id, wave iterations, empty | stale << 16) equal
tests/golden/traversal_stats.npz, recorded from the library of the commit before the walks were shared (tools/make_golden.py --traversal-stats); for closest hits word 3
is also intersect_closest's primitive_id (one mesh with one submesh: the global id is the primitive id).  Words 4 and 5 are clock ticks."""
import os

import numpy as np
import pytest

import multihit_reference as M
from test_bvh_bounds import _quad

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traversal_stats.npz")
LAYOUTS = {"wide": {"wide": 1}, "rope": {"wide": 0}}
WORDS = [0, 1, 2, 3, 6, 7]
N = 250


def stats_scene(mrt):
    pos, idx = _quad((0, 0, 0), np.eye(3)[0], np.eye(3)[2], 16)
    pos = np.vstack([pos, pos]); idx = np.vstack([idx, idx + len(pos) // 2])
    assert len(idx) == 1024
    return M.raw_scene(mrt, [(pos, idx, M._plain(mrt))])


def stats_rays():
    """origins 0.5 to 2 above or below the sheet y = 0 over [-1.4, 1.4]^2 (the sheet is [-1, 1]^2), aimed at points of [-1.4, 1.4]^2 on it: about half the rays cross
    the plane outside the sheet.  Every fifth ray has min_distance = 0.25 (before any hit), every seventh min_distance = 8 (behind every hit)."""
    rng = np.random.default_rng(20250)
    o = rng.uniform(-1.4, 1.4, (N, 3)); o[:, 1] = rng.uniform(0.5, 2.0, N) * np.where(np.arange(N) % 3 == 0, -1.0, 1.0)
    t = rng.uniform(-1.4, 1.4, (N, 3)); t[:, 1] = 0.0
    d = t - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((N, 8), np.float32); rays[:, 0:3] = o; rays[:, 4:7] = d; rays[:, 7] = np.inf
    rays[::5, 3] = 0.25; rays[::7, 3] = 8.0
    return rays


def stats_rows(mrt, ctx):
    """{layout_query: (250, 6) uint32}: the compared words of every case"""
    rays, out = stats_rays(), {}
    for layout, opts in LAYOUTS.items():
        ds = mrt.DeviceScene(ctx, stats_scene(mrt), opts)
        assert ds.stats.wide_layout == opts["wide"]
        for query, any_hit in (("closest", False), ("any", True)):
            out[f"{layout}_{query}"] = ds.traversal_stats(rays, any_hit=any_hit)[:, WORDS]
        out[f"{layout}_primitive"] = ds.intersect_closest(rays)["primitive_id"].astype(np.int64)
        ds.close()
    return out


@pytest.fixture(scope="module")
def rows(mrt, gpu_ctx):
    return stats_rows(mrt, gpu_ctx)


@pytest.mark.parametrize("query", ["closest", "any"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_counters_are_the_recorded_ones(rows, layout, query):
    got, want = rows[f"{layout}_{query}"], np.load(GOLDEN)[f"{layout}_{query}"]
    assert got.shape == want.shape == (N, len(WORDS)) and got.dtype == want.dtype == np.uint32
    bad = np.argwhere((got != want).any(-1))[:, 0]
    assert bad.size == 0, f"{len(bad)} rows differ; first, ray {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_closest_id_is_intersect_closest(rows, layout):
    gid = rows[f"{layout}_closest"][:, 3].astype(np.int64)
    prim = rows[f"{layout}_primitive"]
    assert np.array_equal(np.where(gid == 0xFFFFFFFF, -1, gid), prim)
    assert 40 < (prim >= 0).sum() < N - 40, "the rays are meant to hit and to miss"
    hit = prim >= 0
    assert (prim[hit] < 512).all(), "a tie of the two grids goes to the lower id"
    assert (rows[f"{layout}_any"][:, 2][hit] >= 1).all() and (rows[f"{layout}_any"][:, 2] <= rows[f"{layout}_closest"][:, 2]).all(), "an any-hit walk ends at its first hit"
