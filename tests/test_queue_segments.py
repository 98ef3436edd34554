"""Segmented queues (renderer option queue_segments): the default pass keeps its bounce-ray queue, hit records and shadow-ray queue as eight segments,
each with its own tail word — shade block j reserves on and writes segment j % 8, a packing block reads one segment and writes the same one, and the pulling traversal
launch takes region x = segment x.  Results do not depend on queue order (a hit belongs to its ray, a contribution to its pixel's plane and bounce, the closest hit is the
minimum over (t, id)), so everything here is bit-exact: eight segments == one queue == the oracle.  The shapes are the smallest at which a segment can go wrong; persistent = 1
makes small images take the pulling launch, and every test reads the option back to know that the segmented form was in force."""
import ctypes as C
import functools
import math
import time

import numpy as np
import pytest

K, SHADE_THREADS = 8, 256
_STUCK = []          # renderers whose draw did not end (test_empty_segments): kept alive, never closed


def _renderer(mrt, ctx, sc, size, segs, shard=None):
    r = mrt.Renderer(size, sc, ctx=ctx, seed=1)
    if shard: r.set_shard(*shard)
    r.set_option("persistent", 1); r.set_option("frame_batch", 8); r.set_option("queue_segments", segs)
    assert r.get_option("queue_segments") == segs
    return r


def _draw(mrt, ctx, sc, size, segs, frames=8, shard=None):
    r = _renderer(mrt, ctx, sc, size, segs, shard)
    r.draw(frames, wait=True)
    assert r.get_option("queue_segments") == segs, "the pass did not run in the form asked for"
    out = r.accumulation().copy(), (r.stats.closest_rays, r.stats.shadow_rays, r.stats.primary_rays)
    assert r.framesCompleted == frames
    r.close()
    return out


def _oracle(orc, mrt, sc, size, frames=8):
    o = orc.OracleRenderer(orc.OracleScene(mrt.flatten_scene(sc), sc.lights), size[0], size[1], seed=1, max_bounces=3, camera=sc.camera)
    o.render(frames)
    return o.accumulation(), o.counters() + (frames * size[0] * size[1],)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 64), (72, 40)])          # 64 tiles: one shade(0) block per half tile, 16 per segment; 45 tiles: 90 blocks — segments of 12 and of 11 — and ragged right-hand tiles
def test_eight_segments_equal_one_queue_equal_the_oracle(mrt, orc, gpu_ctx, size):
    sc = mrt.CornellScene(size)
    want, counts = _oracle(orc, mrt, sc, size)
    for segs in (8, 1):
        r = _renderer(mrt, gpu_ctx, sc, size, segs)
        r.draw(8)                                    # not waited for: a wave that never leaves the stealing loop must fail this test, not stall the suite
        deadline = time.monotonic() + 20.0           # (the draw is a few hundred microseconds of device time)
        while r.framesCompleted < 8 and time.monotonic() < deadline: time.sleep(0.002)
        if r.framesCompleted < 8:
            _STUCK.append(r)                         # (closing it would wait for the device)
            pytest.fail(f"queue_segments = {segs}: the draw did not end")
        assert r.get_option("queue_segments") == segs
        img, cnt = r.accumulation(), (r.stats.closest_rays, r.stats.shadow_rays, r.stats.primary_rays)
        r.close()
        assert cnt == counts, (segs, cnt, counts)
        assert _same(img, want), segs


def _top_rows_scene(mrt, size):
    """A small sphere on the ray through the middle of the image's first row of tiles, three pixel rows in radius: every other row of tiles sees nothing."""
    w, h = size
    sc = mrt.Scene(size)
    cam = sc.camera
    v = lambda f: np.array([f.x, f.y, f.z], np.float64)
    d = v(cam.forward) + (-1.0 + 8.0 / h) * v(cam.up)          # uv = (0, pixel row 4)
    dist = 3.0
    centre = v(cam.position) + dist * d / np.linalg.norm(d)
    radius = 3.0 * (2.0 / h) * np.linalg.norm(v(cam.up)) * dist / np.linalg.norm(d)
    sc.models = [mrt.Model(name="sphere", position=[float(c) for c in centre], scale=float(radius))]
    sc.lights = [mrt.Light.pointLight([float(c) for c in v(cam.position)], [3, 3, 3])]
    return sc


@pytest.mark.gpu
def test_empty_segments(mrt, orc, gpu_ctx):
    """16 x 64: two tiles a row, four shade(0) blocks, so a row of tiles feeds segments 0-3 or 4-7.  Geometry in the first row of tiles only: segments 4-7 hold no ray at bounces
    1 and 2 (and 0-3 few), their packing blocks leave at once and the traversal waves whose home they are go on with the next region.  The draw must end."""
    size = (16, 64)
    sc = _top_rows_scene(mrt, size)
    want, counts = _oracle(orc, mrt, sc, size)
    assert want[:8, :, :3].max() > 0 and not want[8:, :, :3].any(), "the camera must see geometry in the first row of tiles only"
    assert counts[1] > 0 and counts[0] > counts[2], counts          # shadow rays and bounce rays are queued from the first row of tiles
    for segs in (8, 1):
        r = _renderer(mrt, gpu_ctx, sc, size, segs)
        r.draw(8)                                    # not waited for: a wave that never leaves the stealing loop must fail this test, not stall the suite
        deadline = time.monotonic() + 20.0           # (the draw is a few hundred microseconds of device time)
        while r.framesCompleted < 8 and time.monotonic() < deadline: time.sleep(0.002)
        if r.framesCompleted < 8:
            _STUCK.append(r)                         # (closing it would wait for the device)
            pytest.fail(f"queue_segments = {segs}: the draw did not end")
        assert r.get_option("queue_segments") == segs
        img, cnt = r.accumulation(), (r.stats.closest_rays, r.stats.shadow_rays, r.stats.primary_rays)
        r.close()
        assert cnt == counts, (segs, cnt, counts)
        assert _same(img, want), segs


@pytest.mark.gpu
def test_pass_sizes_in_one_renderer(mrt, gpu_ctx):
    """136 x 72 (153 tiles): passes of 1, 7 and 8 frames in one renderer.  One frame runs unbundled, hence on one queue; seven frames bundle 9 x 7 lanes of a wave (252 entries
    a block); eight fill it.  The lane's counters and queues pass from one form to the other between draws."""
    size = (136, 72)
    sc = mrt.CornellScene(size)
    rs = {segs: _renderer(mrt, gpu_ctx, sc, size, segs) for segs in (8, 1)}
    done = 0
    for frames, in_force in ((1, 1), (7, 8), (8, 8), (1, 1), (8, 8)):
        for r in rs.values(): r.draw(frames, wait=True)
        done += frames
        assert rs[8].get_option("queue_segments") == in_force and rs[1].get_option("queue_segments") == 1
        a, b = rs[8], rs[1]
        assert (a.stats.closest_rays, a.stats.shadow_rays, a.stats.primary_rays) == (b.stats.closest_rays, b.stats.shadow_rays, b.stats.primary_rays), frames
        assert a.framesCompleted == b.framesCompleted == done
        assert _same(a.accumulation(), b.accumulation()), frames
    for r in rs.values(): r.close()


@pytest.mark.gpu
def test_shards_sum_to_the_single_device_image(mrt, gpu_ctx):
    size = (96, 54)

    class SmallDragonScene(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mo for mo in mrt.DragonScene(size).models if mo.name != "dragon"]
    sc = SmallDragonScene(size)
    full, counts = _draw(mrt, gpu_ctx, sc, size, 1)
    acc, tot = np.zeros_like(full), np.zeros(3, np.int64)
    for rank in range(2):
        img, cnt = _draw(mrt, gpu_ctx, sc, size, 8, shard=(rank, 2))
        acc += img; tot += np.array(cnt, np.int64)
    assert tuple(int(t) for t in tot) == counts
    assert _same(acc, full)


# ---------------------------------------------------------------- capacity (no GPU)
@functools.lru_cache(maxsize=None)
def _received(capacity, B):
    """Entries per queue the segments can receive from shade(0) of a bundled pass: the active lanes of its blocks (shade.h bounce0_slot), block j to segment j % 8."""
    groups = (B + 7) // 8; bw = (B + groups - 1) // groups; per_wave = 64 // bw
    waves = -(-capacity * groups // per_wave); blocks = -(-waves * 64 // SHADE_THREADS)
    t = np.arange(blocks * SHADE_THREADS, dtype=np.int64)
    lane, wave = t & 63, t >> 6
    bi = lane // bw; q = wave * per_wave + bi
    slot = q // groups; sub = (q - slot * groups) * bw + (lane - bi * bw)
    active = (bi < per_wave) & (sub < B) & (slot < capacity)
    per_block = active.reshape(blocks, SHADE_THREADS).sum(1)
    assert per_block.sum() == capacity * B
    return blocks, [int(per_block[x::K].sum()) for x in range(K)], int(per_block.max())


def test_segment_capacity_holds_what_a_segment_can_receive(mrt):
    out = (C.c_uint64 * 4)()
    for w in range(1, 41):
        for h in range(1, 41):
            capacity = math.ceil(w / 8) * math.ceil(h / 8) * 64
            for B in (1, 7, 8, 32):
                assert mrt.lib.mrt_debug_segment_sizing(capacity, B, out) == 0
                blocks, per_block, seg_cap, allocated = (int(v) for v in out)
                want_blocks, received, most = _received(capacity, B)
                assert blocks == want_blocks and per_block >= most, (w, h, B)
                assert seg_cap >= max(received), (w, h, B, seg_cap, received)          # bounce 0; later bounces write at most what they read, segment by segment
                assert K * seg_cap <= allocated, (w, h, B, seg_cap, allocated)          # eight segments fit what a lane allocates ...
                assert allocated - capacity * B <= K * SHADE_THREADS, (w, h, B, allocated)          # ... which is at most K x SHADE_THREADS entries more than one queue took
