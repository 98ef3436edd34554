"""Rank program of tests/test_sharded_assembly.py (a helper, not a test module): started by `python -m torch.distributed.run --nproc-per-node N
tests/sharded_ranks.py OUT`, backend gloo, every rank on device 0.  Each rank drives distributed.ShardedRenderer through every gather order the
test checks and writes what it saw to OUT/rank<r>.npz: after each gather, rank 0's assembled image and this rank's own accumulation buffer; after
each run, this rank's ray counters.  The parent compares all of it with one-device renders of its own."""
import os
import sys

import numpy as np

TILE_SIZES = ((203, 117), (9, 5), (64, 48))          # ragged edge tiles; two tiles (a rank of three owns none); whole tiles
# R = gather by reduce(sum), C = compact gather, dK = draw K more frames.  Tile runs pass ONE frame per pass with one pass in flight, so a draw of
# K frames is K swaps of the renderer's two accumulation buffers: the draws after a compact gather take an odd (d1, d3) and an even (d2) number
TILE_SEQUENCES = ("R", "C", "R,R", "C,C", "R,d1,C", "C,d1,R", "C,d2,R", "C,d3,R", "C,d2,C,d1,R")
SAMPLE_SIZE = (64, 48)
SAMPLE_SEQUENCES = ("R", "R,d2,R")
FIRST = 2                  # frames every run draws before its sequence
SEED, BOUNCES = 1, 3


def gather_frames(seq):
    """Frames drawn in all when each gather of `seq` runs: "C,d2,R" -> [2, 4]."""
    f, out = FIRST, []
    for op in seq.split(","):
        if op[0] == "d":
            f += int(op[1:])
        else:
            out.append(f)
    return out


def frames_total(seq):
    return FIRST + sum(int(op[1:]) for op in seq.split(",") if op[0] == "d")


def key(mode, size, seq, what):
    return f"{mode}_{size[0]}x{size[1]}_{seq.replace(',', '-')}_{what}"


def main(out):
    import torch                    # (before the library: torch's HIP runtime is the one the process shares, tests/conftest.py)
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import metal_raytracing_amd as mrt
    from metal_raytracing_amd.distributed import ShardedRenderer

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = mrt.Context(0)
    rec = {}

    def run(mode, size, seq):
        sr = ShardedRenderer(size, mrt.CornellScene(size), rank, world, mode=mode, device=0, frames_total=frames_total(seq), backend="gloo",
                             seed=SEED, max_bounces=BOUNCES, ctx=ctx)
        if mode == "tile":
            sr.renderer.set_option("frame_batch", 1)
            sr.renderer.set_option("frames_in_flight", 1)
        sr.draw(FIRST)
        i = 0
        for op in seq.split(","):
            if op[0] == "d":
                sr.draw(int(op[1:]))
                continue
            img = sr.gather(compact=op == "C")
            if rank == 0:
                rec[key(mode, size, seq, f"{i}_img")] = img.cpu().numpy()
            rec[key(mode, size, seq, f"{i}_acc")] = sr.renderer.accumulation()
            i += 1
        st = sr.renderer.stats
        rec[key(mode, size, seq, "rays")] = np.array([st.closest_rays, st.shadow_rays, st.primary_rays], np.uint64)
        sr.close()

    for size in TILE_SIZES:
        for seq in TILE_SEQUENCES:
            run("tile", size, seq)
    for seq in SAMPLE_SEQUENCES:
        run("sample", SAMPLE_SIZE, seq)
    np.savez(os.path.join(out, f"rank{rank}.npz"), **rec)
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()
    print(f"rank {rank} of {world} ok")


if __name__ == "__main__":
    main(sys.argv[1])
