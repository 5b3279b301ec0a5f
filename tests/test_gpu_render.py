"""VecMazeEnv.render_batch (mz_render, csrc/render_kernels.hip) on the MI355X against render.render_top_down of the states
get_state() returns.  The host build of the same drawing code equals render_top_down in every pixel (tests/test_render_host.py);
on the device only the state-dependent sin / cos / atan2 of the device math library may differ from glibc by an ulp, so an image
may differ in at most max(1, 1e-4 x pixels) pixels, each of which has an 8-neighbour of the device's colour in the host image."""
import ctypes as C

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import render
from tests.test_render_host import IDS, render_with_goals

pytestmark = pytest.mark.gpu

N = 64


def assert_close_to_host(dev, host, what):
    """dev, host: uint8 [H, W, 3].  The ulp allowance of the module docstring."""
    diff = (dev != host).any(-1)
    nd = int(diff.sum())
    if nd == 0:
        return
    h, w = diff.shape
    assert nd <= max(1, int(1e-4 * h * w)), f"{what}: {nd} pixels differ"
    for y, x in zip(*np.nonzero(diff)):
        nb = host[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].reshape(-1, 3)
        assert (nb == dev[y, x]).all(-1).any(), f"{what}: pixel ({y}, {x}) = {dev[y, x]} has no such neighbour in the host image"


def _env(env_id, n=N, **kw):
    import torch

    torch.cuda.set_device(0)
    if env_id == "chain5":
        from tests.test_mjcf import chain_swimmer_xml

        return mm.make("SwimmerUMaze-v0", num_envs=n, robot_xml=chain_swimmer_xml(5), **kw)
    if env_id in ("HalfBlockMaze/point", "SpinCellMaze/point"):
        from mujoco_maze_amd.maze_env import VecMazeEnv
        from tests.test_general_engine import SpinCellMaze
        from tests.test_top_down_view import HalfBlockMaze

        task = HalfBlockMaze if env_id.startswith("Half") else SpinCellMaze
        return VecMazeEnv(mm.PointEnv, task, num_envs=n, maze_size_scaling=4.0, **kw)
    return mm.make(env_id, num_envs=n, **kw)


def _walk(env, steps, seed):
    import torch

    env.reset(seed=seed)
    rng = np.random.default_rng(seed)
    lo, hi = env.action_space.low, env.action_space.high
    for _ in range(steps):
        env.step(torch.as_tensor(rng.uniform(lo, hi, (env.num_envs, env.nu)).astype(np.float32), device=env.device))


@pytest.mark.parametrize("env_id", IDS + ["chain5", "HalfBlockMaze/point", "SpinCellMaze/point", "AntUMaze-v0/general"])
def test_render_batch_equals_render_top_down(env_id):
    import torch

    general = env_id.endswith("/general")
    env = _env(env_id.split("/general")[0], engine="general") if general else _env(env_id)
    if general:
        assert env.launch_info()["engine"] == 1
    _walk(env, 5, seed=3)
    for shape in ((64, 64), (97, 31)):
        imgs = env.render_batch(image_shape=shape)
        qpos = env.get_state()[0]
        torch.cuda.synchronize()
        assert imgs.shape == (N, shape[1], shape[0], 3) and imgs.dtype == torch.uint8 and imgs.device == env.device
        imgs, qpos = imgs.cpu().numpy(), qpos.cpu().numpy()
        for e in range(N):
            assert_close_to_host(imgs[e], render.render_top_down(env.model, qpos[e].astype(np.float64), shape), f"{env_id} {shape} env {e}")
    big = env.render_batch([0, N - 1], image_shape=(600, 480)).cpu().numpy()
    qpos = env.get_state()[0].cpu().numpy()
    for i, e in enumerate((0, N - 1)):
        assert_close_to_host(big[i], render.render_top_down(env.model, qpos[e].astype(np.float64), (600, 480)), f"{env_id} 600x480 env {e}")
    env.close()


def test_explicit_qpos_indices_and_out():
    import torch

    env = _env("AntPush-v0")
    _walk(env, 3, seed=1)
    q = env.get_state()[0]
    qn = q.cpu().numpy()
    idx = [5, 2, 5, 63, 0, 2]
    sub = env.render_batch(idx, image_shape=(97, 31))
    full = env.render_batch(image_shape=(97, 31))
    torch.cuda.synchronize()
    assert torch.equal(sub, full[idx])
    # an index tensor on the device, in any order with repeats
    assert torch.equal(env.render_batch(torch.tensor(idx, device=env.device), image_shape=(97, 31)), sub)
    # explicit states: row i is drawn for image i (here: every env's state moved by half a cell)
    q2 = q.clone()
    q2[:, 0] += 0.5 * env.model.world.scale
    moved = env.render_batch(image_shape=(64, 64), qpos=q2)
    q2n = q2.cpu().numpy()
    for e in (0, 17, 63):
        assert_close_to_host(moved[e].cpu().numpy(), render.render_top_down(env.model, q2n[e].astype(np.float64), (64, 64)), f"qpos env {e}")
    assert not torch.equal(moved, env.render_batch(image_shape=(64, 64)))
    # explicit states for a subset of envs; numpy input
    two = env.render_batch([3, 3], image_shape=(64, 64), qpos=qn[[7, 9]])
    for i, e in enumerate((7, 9)):
        assert_close_to_host(two[i].cpu().numpy(), render.render_top_down(env.model, qn[e].astype(np.float64), (64, 64)), f"subset {i}")
    # out= is drawn into and returned
    out = torch.full((len(idx), 31, 97, 3), 7, dtype=torch.uint8, device=env.device)
    r = env.render_batch(idx, image_shape=(97, 31), out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(out, sub)
    out.fill_(0)
    env.render_batch(idx, image_shape=(97, 31), out=out)
    assert torch.equal(out, sub)
    # an empty selection
    assert env.render_batch([], image_shape=(8, 8)).shape == (0, 8, 8, 3)
    env.close()


def test_out_of_range_device_indices_give_zero_images():
    import torch

    env = _env("PointUMaze-v0", n=8)
    env.reset(seed=0)
    imgs = env.render_batch(torch.tensor([1, -1, 8, 1 << 30], device=env.device), image_shape=(33, 17))
    torch.cuda.synchronize()
    assert imgs[0].any() and not imgs[1:].any()
    env.close()


def test_stream_order_after_step():
    """Renders enqueued straight after each step (no synchronisation) show that step's state."""
    import torch

    env = _env("AntUMaze-v0")
    env.reset(seed=2)
    rng = np.random.default_rng(2)
    imgs, states = [], []
    for _ in range(4):
        env.step(torch.as_tensor(rng.uniform(-1, 1, (N, env.nu)).astype(np.float32), device=env.device))
        imgs.append(env.render_batch(image_shape=(64, 64)))
        states.append(env.get_state()[0])
    torch.cuda.synchronize()
    again = env.render_batch(image_shape=(64, 64))
    torch.cuda.synchronize()
    assert torch.equal(again, imgs[-1])
    assert not torch.equal(imgs[0], imgs[-1])
    for t in (0, 3):
        qn = states[t].cpu().numpy()
        for e in (0, 31, 63):
            assert_close_to_host(imgs[t][e].cpu().numpy(), render.render_top_down(env.model, qn[e].astype(np.float64), (64, 64)), f"step {t} env {e}")
    env.close()


@pytest.mark.parametrize("model_cls", ["PointEnv", "AntEnv"])
def test_per_env_goals(model_cls):
    """A task that resamples its goal per env: each image shows that env's own goal row (env_goals)."""
    import torch

    from mujoco_maze_amd.maze_env import VecMazeEnv
    from tests.test_custom_task import RandomGoalCross

    env = VecMazeEnv(getattr(mm, model_cls), RandomGoalCross, maze_size_scaling=4.0, num_envs=N, auto_reset=True)
    env.reset(seed=1)
    _walk_no_reset(env, 3)
    goals = env.env_goals.cpu().numpy()
    assert len(np.unique(goals[:, 0, 0])) > N // 2  # (envs that reached the goal took a pool member again)
    imgs = env.render_batch(image_shape=(97, 31)).cpu().numpy()
    qpos = env.get_state()[0].cpu().numpy()
    ng = env.model.c.ngoal
    for e in range(N):
        want = render_with_goals(env.model, goals[e, :ng], qpos[e].astype(np.float64), (97, 31))
        assert_close_to_host(imgs[e], want, f"{model_cls} env {e}")
    # image i of a selection takes env_indices[i]'s goals
    sel = env.render_batch([9, 4], image_shape=(97, 31)).cpu().numpy()
    assert np.array_equal(sel[0], imgs[9]) and np.array_equal(sel[1], imgs[4])
    env.close()


def _walk_no_reset(env, steps):
    import torch

    rng = np.random.default_rng(4)
    for _ in range(steps):
        env.step(torch.as_tensor(rng.uniform(env.action_space.low, env.action_space.high, (env.num_envs, env.nu)).astype(np.float32),
                                 device=env.device))


def test_refusals():
    import torch

    from mujoco_maze_amd import maze_task as T
    from mujoco_maze_amd.maze_env import VecMazeEnv
    from tests.user_robots import robot_classes

    env = _env("PointUMaze-v0", n=8)
    env.reset(seed=0)
    for shape in ((1, 64), (64, 1), (0, 0)):
        with pytest.raises(ValueError, match="image_shape"):
            env.render_batch(image_shape=shape)
    for idx in ([0, 8], [-1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="env_indices"):
            env.render_batch(idx, image_shape=(8, 8))
    with pytest.raises(ValueError, match="env_indices"):
        env.render_batch(torch.zeros((2, 2), dtype=torch.int32, device=env.device))
    for q in (torch.zeros((8, env.nq + 1), device=env.device), torch.zeros(env.nq, device=env.device), torch.zeros((9, env.nq), device=env.device)):
        with pytest.raises(ValueError, match="qpos"):
            env.render_batch(image_shape=(8, 8), qpos=q)
    with pytest.raises(ValueError, match="qpos"):
        env.render_batch([0, 1, 2], image_shape=(8, 8), qpos=torch.zeros((2, env.nq), device=env.device))
    with pytest.raises(ValueError, match="out"):
        env.render_batch(image_shape=(8, 8), out=torch.zeros((8, 8, 8, 3), dtype=torch.float32, device=env.device))
    with pytest.raises(ValueError, match="out"):
        env.render_batch(image_shape=(8, 8), out=torch.zeros((8, 8, 9, 3), dtype=torch.uint8, device=env.device))
    # the C-ABI refuses on its own
    lib = env._lib
    rgb, size = (np.ascontiguousarray(a) for a in render.goal_style(env.model))
    out = torch.zeros((16, 8, 8, 3), dtype=torch.uint8, device=env.device)

    def call(count, w, h, ngoal):
        return lib.mz_render(env._h, None, None, count, w, h, ngoal, rgb.ctypes.data_as(C.c_void_p), size.ctypes.data_as(C.c_void_p),
                             C.c_void_p(out.data_ptr()), env._stream())

    assert call(8, 8, 8, len(size)) == 0
    assert call(9, 8, 8, len(size)) == -1 and b"num_envs" in lib.mz_last_error(env._h)
    assert call(-1, 8, 8, len(size)) == -1
    assert call(8, 1, 8, len(size)) == -1 and b"width" in lib.mz_last_error(env._h)
    assert call(8, 8, 8, len(size) + 1) == -1 and b"ngoal_style" in lib.mz_last_error(env._h)
    torch.cuda.synchronize()
    env.close()
    # a user robot: render.py does not draw its geoms
    BipedAnt, _ = robot_classes()
    user = VecMazeEnv(BipedAnt, T.DistRewardUMaze, maze_size_scaling=4.0, num_envs=4)
    with pytest.raises(NotImplementedError, match="user robot"):
        user.render_batch(image_shape=(8, 8))
    assert user.model.c.ngoal == len(size)
    rc = user._lib.mz_render(user._h, None, None, 4, 8, 8, len(size), rgb.ctypes.data_as(C.c_void_p),
                             size.ctypes.data_as(C.c_void_p), C.c_void_p(out.data_ptr()), user._stream())
    assert rc == -3 and b"user robot" in user._lib.mz_last_error(user._h)
    user.close()


@pytest.mark.parametrize("env_id", ["AntUMaze-v0", "PointBilliard-v0"])
def test_rendering_has_no_side_effects(env_id):
    """Stepping with render_batch calls in between gives bit-identical results to stepping without them."""
    import torch

    runs = []
    for with_render in (False, True):
        env = _env(env_id, auto_reset=True, max_episode_steps=6)
        env.reset(seed=11)
        rng = np.random.default_rng(11)
        rec = []
        for t in range(10):
            a = torch.as_tensor(rng.uniform(env.action_space.low, env.action_space.high, (N, env.nu)).astype(np.float32), device=env.device)
            if with_render:
                env.render_batch(image_shape=(64, 64))
            obs, rew, done, _ = env.step(a)
            if with_render:
                env.render_batch([t % N, 1], image_shape=(33, 17))
            rec.append([x.clone() for x in (obs, rew, done)] + [s.clone() for s in env.get_state()])
        torch.cuda.synchronize()
        runs.append(rec)
        env.close()
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
