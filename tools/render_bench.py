"""Device top views (VecMazeEnv.render_batch, mz_render) against the host rasteriser (render.render_top_down): ms per batch, frames/s,
the bytes the images take and their share of the HBM bandwidth.  Needs the MI355X.

    python tools/render_bench.py [--iters 20] [--warmup 3] [--out DIR]

Each case warms up, then times `iters` renders between two HIP events after a synchronise; the envs hold the state of a few random
steps.  Written bytes are the algorithm's (count x H x W x 3 uint8; nothing is read but the states); the HBM share is those bytes
over the batch time against the 8 TB/s spec peak.  For kernel times take a run of its own under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/render_bench.py --iters 5`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E spec
CASES = [("AntUMaze-v0", 4096, (64, 64)), ("PointUMaze-v0", 4096, (64, 64)), ("AntUMaze-v0", 256, (600, 480))]


def time_case(env_id, n, shape, iters, warmup):
    import torch

    import mujoco_maze_amd as mm

    env = mm.make(env_id, num_envs=n, force_vec=True)
    env.reset(seed=0)
    rng = np.random.default_rng(0)
    for _ in range(4):
        env.step(torch.as_tensor(rng.uniform(env.action_space.low, env.action_space.high, (n, env.nu)).astype(np.float32), device=env.device))
    out = torch.empty((n, shape[1], shape[0], 3), dtype=torch.uint8, device=env.device)
    for _ in range(warmup):
        env.render_batch(image_shape=shape, out=out)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        env.render_batch(image_shape=shape, out=out)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / iters
    nbytes = n * shape[0] * shape[1] * 3
    env.close()
    return dict(case=f"{env_id} x{n} {shape[0]}x{shape[1]}", ms_per_batch=ms, frames_per_s=n / (ms * 1e-3), bytes_written=nbytes,
                hbm_share=nbytes / (ms * 1e-3) / HBM_PEAK)


def host_frame(iters):
    from mujoco_maze_amd import model, render
    from mujoco_maze_amd import registration

    spec = registration.REGISTRY["AntUMaze-v0"]
    kw = spec.kwargs
    cm = model.compile_model(kw["model_cls"].ROBOT, kw["maze_task"](kw["maze_size_scaling"]), kw["maze_size_scaling"])
    q = np.array([cm.c.qpos0[i] for i in range(cm.c.nq)])
    render.render_top_down(cm, q, (600, 480))
    t = time.perf_counter()
    for _ in range(iters):
        render.render_top_down(cm, q, (600, 480))
    ms = (time.perf_counter() - t) * 1e3 / iters
    return dict(case="host render_top_down AntUMaze-v0 600x480 (one frame)", ms_per_batch=ms, frames_per_s=1e3 / ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for render_bench.json")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("render_bench.py needs the MI355X (no CPU fallback)")
    rows = [time_case(env_id, n, shape, a.iters, a.warmup) for env_id, n, shape in CASES]
    rows.append(host_frame(max(3, a.iters // 4)))
    for r in rows:
        extra = f"  {r['bytes_written'] / 1e6:8.1f} MB written  {100 * r['hbm_share']:6.2f} % of HBM peak" if "bytes_written" in r else ""
        print(f"{r['case']:<52s} {r['ms_per_batch']:9.3f} ms/batch {r['frames_per_s']:12.0f} frames/s{extra}")
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "render_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
