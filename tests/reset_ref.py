"""What an in-step auto-reset must draw — TEST INFRASTRUCTURE ONLY.

Every step kernel that ends an env's episode resets it inside the launch from `episode_seed(seed, episode)` (csrc/mz_rng.h) and the
env's global slot; mz_reset draws episode 0, whose seed is the handle's seed itself.  The oracle's reset takes a plain seed, so the
expected state of an env in its k-th episode since the last mz_reset is `oracle.reset(cm, n, episode_seed(seed, k), env0=env0)`."""
import numpy as np

from mujoco_maze_amd.policy import _mix64

_EPISODE_MUL = 0xD6E8FEB86659FD93
_M64 = (1 << 64) - 1


def episode_seed(seed: int, episode: int) -> int:
    """csrc/mz_rng.h episode_seed: a Python int in [0, 2^64); `episode` is the kernel's uint32 counter."""
    seed, episode = int(seed) & _M64, int(episode) & 0xFFFFFFFF
    if episode == 0:
        return seed
    z = seed ^ ((_EPISODE_MUL * episode) & _M64)
    with np.errstate(over="ignore"):
        return int(_mix64(np.array([z], dtype=np.uint64))[0])


def expected_reset(oracle, cm, n, seed, episodes, env0):
    """(state, obs) of the oracle where env e of n has just started episode episodes[e] under the handle seed `seed`, the batch's
    first env sitting in global slot env0: one oracle.reset per distinct episode count, its rows taken for the envs that carry it."""
    episodes = np.asarray(episodes)
    assert episodes.shape == (n,)
    st = obs = None
    for k in np.unique(episodes):
        s, o = oracle.reset(cm, n, episode_seed(seed, int(k)), env0=env0)
        if st is None:
            st, obs = {key: np.zeros_like(v) for key, v in s.items()}, np.zeros_like(o)
        rows = episodes == k
        for key in st:
            st[key][rows] = s[key][rows]
        obs[rows] = o[rows]
    return st, obs
