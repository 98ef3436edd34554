"""distributed.ShardedRenderer with real ranks (torch.distributed.run, backend gloo, every rank on this box's GPU) through every order of the two ways to
assemble a tile-sharded image — reduce(sum) of whole buffers (R) and the compact gather of owned tiles (C) — with draws between them, at ragged sizes and at
one where a rank owns no tile.  One launch per world size runs every case (tests/sharded_ranks.py); this process checks what the ranks wrote against
one-device renders of its own:
  * rank 0's image after every gather == one Renderer that drew the same frames, bit for bit (and the oracle's, once per size);
  * every rank's own accumulation buffer after every gather == a one-device renderer of that shard, bit for bit, and 0 outside its tiles — an assemble
    that leaves other shards' pixels in a rank's buffer is caught whatever the parity of the swaps after it;
  * sample sharding: the image == the float64 mean of the per-rank renders;
  * the ranks' ray counters add up to one device's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sharded_ranks as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[2, 3], ids=lambda n: f"world{n}")
def ranks(request, tmp_path_factory):
    """(world, [rank r's records]): ONE launch of the rank program per world size (parent + 3 ranks at most have the GPU open)."""
    n = request.param
    out = tmp_path_factory.mktemp(f"sharded{n}")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(29571 + n),
                        os.path.join(ROOT, "tests", "sharded_ranks.py"), str(out)], capture_output=True, text=True, cwd=ROOT, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    recs = []
    for r in range(n):
        with np.load(out / f"rank{r}.npz") as z:
            recs.append({k: z[k] for k in z.files})
    return n, recs


class _Refs:
    """One-device renders on the test's own context, each made once."""

    def __init__(self, mrt, ctx):
        self.mrt, self.ctx, self.memo = mrt, ctx, {}

    def _renderer(self, size, **opts):
        r = self.mrt.Renderer(size, self.mrt.CornellScene(size), ctx=self.ctx, seed=S.SEED, max_bounces=S.BOUNCES)
        for k, v in opts.items():
            r.set_option(k, v)
        return r

    def full(self, size, frames):
        """(image, (closest, shadow, primary)) of one renderer that drew `frames` frames in one call."""
        k = ("full", size, frames)
        if k not in self.memo:
            r = self._renderer(size); r.draw(frames, wait=True)
            st = r.stats
            self.memo[k] = (r.accumulation(), (st.closest_rays, st.shadow_rays, st.primary_rays))
            r.close()
        return self.memo[k]

    def shard(self, size, rank, world, frames, upto=S.FIRST + 3):
        """Shard (rank, world) of one renderer with the library's default passes, after FIRST, FIRST + 1, ..., `upto` frames."""
        k = ("shard", size, rank, world)
        if k not in self.memo:
            r = self._renderer(size); r.set_shard(rank, world)
            r.draw(S.FIRST, wait=True); acc = {S.FIRST: r.accumulation()}
            for f in range(S.FIRST + 1, upto + 1):
                r.draw(1, wait=True); acc[f] = r.accumulation()
            self.memo[k] = acc; r.close()
        return self.memo[k][frames]

    def sample(self, size, rank, offset, frames):
        """(image, (closest, shadow, primary)) of a whole-frame renderer whose sample indices start at `offset`, after FIRST frames and after `frames`."""
        k = ("sample", size, rank, offset, frames)
        if k not in self.memo:
            r = self._renderer(size, sample_offset=offset)
            r.draw(S.FIRST, wait=True); out = {S.FIRST: r.accumulation()}
            if frames > S.FIRST:
                r.draw(frames - S.FIRST, wait=True); out[frames] = r.accumulation()
            st = r.stats
            self.memo[k] = (out, (st.closest_rays, st.shadow_rays, st.primary_rays)); r.close()
        return self.memo[k]


@pytest.fixture(scope="module")
def refs(mrt, gpu_ctx):
    return _Refs(mrt, gpu_ctx)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _cases():
    for size in S.TILE_SIZES:
        for seq in S.TILE_SEQUENCES:
            for i, frames in enumerate(S.gather_frames(seq)):
                yield size, seq, i, frames


def test_tile_image_after_every_gather_is_the_one_device_image(ranks, refs):
    n, recs = ranks
    wrong = [f"{w}x{h} {seq} gather {i}" for (w, h), seq, i, frames in _cases() if not _same(recs[0][S.key("tile", (w, h), seq, f"{i}_img")], refs.full((w, h), frames)[0])]
    assert not wrong, f"world {n}: assembled image differs from one device's after " + "; ".join(wrong)


def test_tile_image_matches_the_oracle(ranks, mrt, orc):
    from test_gpu_parity import assert_parity, oracle_render
    n, recs = ranks
    for w, h in S.TILE_SIZES:
        oimg, _ = oracle_render(orc, mrt, mrt.CornellScene((w, h)), w, h, S.FIRST, bounces=S.BOUNCES, seed=S.SEED)
        assert_parity(recs[0][S.key("tile", (w, h), "C", "0_img")], oimg, exact_frac=1.0)


def test_every_rank_buffer_holds_its_own_shard_alone(ranks, refs):
    """A gather must leave each rank's accumulation buffer as it was: that rank's shard, other pixels 0 — what the next draw and a checkpoint read."""
    from metal_raytracing_amd.distributed import tile_owner_map
    n, recs = ranks
    wrong = []
    for (w, h), seq, i, frames in _cases():
        for r in range(n):
            acc = recs[r][S.key("tile", (w, h), seq, f"{i}_acc")]
            foreign = tile_owner_map(w, h, n) != r
            if not _same(acc, refs.shard((w, h), r, n, frames)) or np.any(acc[foreign] != 0):
                wrong.append(f"rank {r} {w}x{h} {seq} gather {i}")
    assert not wrong, f"world {n}: a rank's own buffer is not its shard after " + "; ".join(wrong)


def test_tile_ray_counts_add_up_to_one_device(ranks, refs):
    n, recs = ranks
    for size in S.TILE_SIZES:
        for seq in S.TILE_SEQUENCES:
            got = sum(recs[r][S.key("tile", size, seq, "rays")].astype(np.int64) for r in range(n))
            assert tuple(int(x) for x in got) == refs.full(size, S.frames_total(seq))[1], (size, seq)


def test_sample_image_is_the_mean_of_the_rank_renders(ranks, refs):
    """Sample sharding: rank r renders whole frames from sample index r x frames_total; rank 0 gets the mean of the n images (gloo's summation order is not
    fixed: a tolerance, not bits).  Every rank's own buffer and ray counters are its one-device render's exactly."""
    n, recs = ranks
    size = S.SAMPLE_SIZE
    for seq in S.SAMPLE_SEQUENCES:
        ft = S.frames_total(seq)
        per_rank = [refs.sample(size, r, r * ft, ft) for r in range(n)]
        for i, frames in enumerate(S.gather_frames(seq)):
            mean = np.mean([img[frames].astype(np.float64) for img, _ in per_rank], axis=0)
            np.testing.assert_allclose(recs[0][S.key("sample", size, seq, f"{i}_img")], mean, rtol=1e-6, atol=0, err_msg=f"{seq} gather {i}")
            for r in range(n):
                assert _same(recs[r][S.key("sample", size, seq, f"{i}_acc")], per_rank[r][0][frames]), (seq, i, r)
        for r in range(n):
            assert tuple(int(x) for x in recs[r][S.key("sample", size, seq, "rays")]) == per_rank[r][1], (seq, r)
