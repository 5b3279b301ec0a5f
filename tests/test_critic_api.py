"""The critic and GAE without a GPU: the three C-ABI entries at the boundary, and the arithmetic of mz_value (csrc/mz_policy.h
mzp_value_row) and mz_gae (csrc/mz_gae.h), built for the host under tests/critic_host with g++ -ffp-contract=off, against
mujoco_maze_amd/policy.py.

The affine critic is two separately rounded fp32 operations per term in a fixed order: bit equality with numpy.  With a tanh hidden
layer the value carries libm's tanhf, so it goes against a float64 evaluation within the bound tests/test_policy_api.py derives for
the actor's tanh path (`f64_and_bound`, with nu = 1 and no squash).  The GAE scan is additions, products and selects in a fixed order:
bit equality — and a three-step case whose expected numbers are written out below in float64, so that the C scan and its numpy
mirror cannot agree on a wrong recurrence."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mujoco_maze_amd import _capi, policy
from tests.test_policy_api import f64_and_bound, random_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "critic_host")
MZ_ERR_ARG = -1

_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HERE])
        lib = C.CDLL(os.path.join(HERE, "libcritichost.so"))
        vp, i32 = C.c_void_p, C.c_int
        lib.mzc_host_sizeof_critic.restype = C.c_ulonglong
        lib.mzc_host_value.restype = i32
        lib.mzc_host_value.argtypes = [vp, C.c_longlong, i32, i32, vp, i32, vp]
        lib.mzc_host_gae.restype = i32
        lib.mzc_host_gae.argtypes = [i32, i32, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp]
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_value(vparams, obs, hidden=0):
    """mzp_value_row on the CPU: float32 [R] for the rows obs [R, obs_dim]; vparams [nvpar] or [R, nvpar]."""
    p, x = np.ascontiguousarray(vparams, np.float32), np.ascontiguousarray(obs, np.float32)
    out = np.full(x.shape[0], np.nan, np.float32)
    rc = _load().mzc_host_value(_p(p), p.shape[1] if p.ndim == 2 else 0, x.shape[1], hidden, _p(x), x.shape[0], _p(out))
    assert rc == 0, rc
    return out


def host_gae(rewards, dones, values, next_values, gamma, lam, with_ret=True):
    """mzg_scan on the CPU over [K, N] rows: (adv, ret) float32 [K, N]."""
    r, v, nv = (np.ascontiguousarray(a, np.float32) for a in (rewards, values, next_values))
    d = np.ascontiguousarray(dones, np.uint8)
    adv, ret = np.full(r.shape, np.nan, np.float32), np.full(r.shape, np.nan, np.float32)
    rc = _load().mzc_host_gae(r.shape[0], r.shape[1], _p(r), _p(d), _p(v), _p(nv), gamma, lam, _p(adv), _p(ret) if with_ret else None)
    assert rc == 0, rc
    return adv, ret


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------- the C-ABI boundary
def test_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "mazestep.h")).read()
    val = re.search(r"int32_t\s+mz_value\s*\(([^;]*)\);", header)
    roll = re.search(r"int32_t\s+mz_rollout_actor_critic\s*\(([^;]*)\);", header)
    gae = re.search(r"int32_t\s+mz_gae\s*\(([^;]*)\);", header)
    assert val and roll and gae, "include/mazestep.h does not declare mz_value / mz_rollout_actor_critic / mz_gae"
    v, r, g = ([s.strip() for s in m.group(1).replace("\n", " ").split(",")] for m in (val, roll, gae))
    assert len(v) == 7 and v[2] == "int64_t env_stride" and v[3] == "int32_t hidden" and v[-1] == "void* stream"
    assert len(r) == 20 and r[1] == "int32_t n_steps" and r[7] == "int32_t sample" and r[10] == "const mz_critic* critic" and r[11] == "float* obs_dev"
    assert len(g) == 11 and g[6] == "double gamma" and g[7] == "double lam" and g[9] == "float* ret_dev"
    for name in ("mz_value", "mz_rollout_actor_critic", "mz_gae"):
        assert name in _capi.SYMBOLS
        assert hasattr(_capi.load(), name)
    assert re.search(r"#define MZ_ABI_VERSION 8\b", header)
    # the defining loop and the recurrence are part of the interface
    assert "next_value_seq[k][i] = (auto_reset && done[k][i]) ? mz_value(row i of the bound final_obs) : mz_value(row i of obs_dev)" in header
    assert "b     = (done & 1) ? 0.0f : g * next_value" in header and "c     = done ? 0.0f : gl * carry" in header


def test_the_ctypes_mirror_of_mz_critic_has_the_c_structs_size():
    assert C.sizeof(_capi.MzCritic) == _load().mzc_host_sizeof_critic() == 40
    assert [f[0] for f in _capi.MzCritic._fields_] == ["params_dev", "env_stride", "hidden", "reserved", "value_seq_dev", "next_value_seq_dev"]
    assert _capi.MzCritic.hidden.offset == 16 and _capi.MzCritic.value_seq_dev.offset == 24


def test_entries_refuse_a_null_handle():
    lib = _capi.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.mz_value(None, p, 0, 0, p, p, None) == MZ_ERR_ARG
    assert lib.mz_rollout_actor_critic(None, 4, p, 0, 0, 0, 1.0, 0, 0, 0, None, p, p, p, None, None, None, None, None, None) == MZ_ERR_ARG
    assert lib.mz_gae(None, 4, p, p, p, p, 0.99, 0.95, p, p, None) == MZ_ERR_ARG


# ---------------------------------------------------------------------------------------------- the critic's arithmetic
@pytest.mark.parametrize("obs_dim", [7, 30, 123])
def test_host_affine_value_is_bit_equal_to_the_numpy_model(obs_dim):
    rng = np.random.default_rng(obs_dim)
    obs = rng.uniform(-3.0, 3.0, (64, obs_dim)).astype(np.float32)
    for vparams in (random_policy(rng, obs_dim, 1, 0), random_policy(rng, obs_dim, 1, 0, rows=64)):
        assert vparams.shape[-1] == policy.param_count(obs_dim, 1, 0) == obs_dim + 1
        got, want = host_value(vparams, obs), policy.value_reference(vparams, obs)
        assert got.shape == want.shape == (64,) and want.dtype == np.float32
        assert np.array_equal(_bits(got), _bits(want))
        # the value IS the pre-squash output of the policy with nu = 1
        assert np.array_equal(_bits(want), _bits(policy.reference(vparams, obs, 1)[:, 0]))
        val, bound = f64_and_bound(vparams, obs, 1, 0, False, 1.0)
        assert np.all(np.abs(got.astype(np.float64) - val[:, 0]) <= bound[:, 0])


@pytest.mark.parametrize("hidden", [1, 5, 64])
@pytest.mark.parametrize("obs_dim", [7, 30, 123])
def test_host_tanh_value_within_the_actors_bound(obs_dim, hidden):
    rng = np.random.default_rng(obs_dim * 100 + hidden)
    obs = rng.uniform(-3.0, 3.0, (64, obs_dim)).astype(np.float32)
    for vparams in (random_policy(rng, obs_dim, 1, hidden), random_policy(rng, obs_dim, 1, hidden, rows=64)):
        val, bound = f64_and_bound(vparams, obs, 1, hidden, False, 1.0)
        for name, got in (("host build", host_value(vparams, obs, hidden)), ("policy.value_reference", policy.value_reference(vparams, obs, hidden))):
            err = np.abs(got.astype(np.float64) - val[:, 0])
            print(f"{name}: obs_dim {obs_dim} Hv {hidden}: max err {err.max():.3e}, max err / bound {(err / bound[:, 0]).max():.3f}")
            assert np.all(err <= bound[:, 0]), name


def test_value_rows_are_independent_and_nan_stays_in_its_row():
    rng = np.random.default_rng(11)
    obs = rng.uniform(-3.0, 3.0, (9, 11)).astype(np.float32)
    vparams = random_policy(rng, 11, 1, 5, rows=9)
    vparams[4, 3] = np.nan
    got, ref = host_value(vparams, obs, 5), policy.value_reference(vparams, obs, 5)
    for out in (got, ref):
        assert np.isnan(out[4]) and np.isfinite(np.delete(out, 4)).all()
    for r in range(9):
        assert np.array_equal(_bits(got[r: r + 1]), _bits(host_value(vparams[r], obs[r: r + 1], 5)))
    assert policy.value_reference(vparams[0], obs[0], 5).shape == ()
    with pytest.raises(ValueError):
        policy.value_reference(np.zeros(13), obs)  # 11 + 1 = 12


# ---------------------------------------------------------------------------------------------- the GAE scan
def gae_inputs(rng, K, N):
    """Random [K, N] rows that hold every done value (0, 1, 2, 3) where K * N allows, and NaN next_values behind done & 1."""
    r = rng.normal(0.0, 1.0, (K, N)).astype(np.float32)
    v = rng.normal(0.0, 2.0, (K, N)).astype(np.float32)
    nv = rng.normal(0.0, 2.0, (K, N)).astype(np.float32)
    d = rng.choice(np.array([0, 0, 0, 0, 1, 2, 3], np.uint8), (K, N))
    term = (d & 1) != 0
    nv[term & (rng.random((K, N)) < 0.5)] = np.nan
    return r, d, v, nv


@pytest.mark.parametrize("K,N", [(1, 64), (2, 5), (37, 130), (300, 3)])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_host_gae_is_bit_equal_to_the_numpy_model(K, N, gamma, lam):
    rng = np.random.default_rng(K * 1000 + N)
    r, d, v, nv = gae_inputs(rng, K, N)
    if K * N >= 64:
        assert {0, 1, 2, 3} <= set(np.unique(d).tolist())
        assert np.isnan(nv[(d & 1) != 0]).any() and not np.isnan(nv[(d & 1) == 0]).any()
    adv, ret = host_gae(r, d, v, nv, gamma, lam)
    want_adv, want_ret = policy.gae_reference(r, d, v, nv, gamma, lam)
    assert want_adv.dtype == want_ret.dtype == np.float32 and want_adv.shape == (K, N)
    assert np.isfinite(want_adv).all() and np.isfinite(want_ret).all()  # NaN behind a true termination does not leak
    assert np.array_equal(_bits(adv), _bits(want_adv)) and np.array_equal(_bits(ret), _bits(want_ret))
    adv2, ret2 = host_gae(r, d, v, nv, gamma, lam, with_ret=False)  # ret is nullable
    assert np.array_equal(_bits(adv2), _bits(adv)) and np.isnan(ret2).all()


def test_gae_nan_leaks_where_it_should():
    """A NaN bootstrap value behind a time limit alone (done == 2) or mid-episode IS used, and reaches the steps before it only up to
    the previous episode end."""
    r, v = np.ones((4, 1), np.float32), np.zeros((4, 1), np.float32)
    nv = np.array([[1.0], [1.0], [np.nan], [1.0]], np.float32)
    d = np.array([[0], [3], [2], [0]], np.uint8)
    for fn in (host_gae, policy.gae_reference):
        adv, _ = fn(r, d, v, nv, 0.5, 0.5)
        assert np.isfinite(adv[3, 0]) and np.isnan(adv[2, 0]) and np.isfinite(adv[1, 0]) and np.isfinite(adv[0, 0])


def test_gae_three_steps_worked_out_by_hand():
    """gamma = lam = 0.5 (g = 0.5, gl = 0.25) and inputs with few mantissa bits: every intermediate is exact in fp32, so the float64
    expressions below, which spell the recurrence out step by step, are the expected fp32 results to the bit.  Three envs: no episode
    end; a true termination at k = 1 with a NaN next_value behind it; a time limit at k = 1 whose terminal value 4.0 is not v[2]."""
    g, gl = 0.5, 0.25
    r = np.array([[1.0] * 3, [2.0] * 3, [3.0] * 3], np.float32)
    v = np.array([[0.5] * 3, [1.0] * 3, [1.5] * 3], np.float32)
    nv = np.array([[1.0, 1.0, 1.0], [1.5, np.nan, 4.0], [2.0, 2.0, 2.0]], np.float32)
    d = np.array([[0, 0, 0], [0, 1, 2], [0, 0, 0]], np.uint8)
    # k = 2, all envs: no end, carry 0
    a2 = (3.0 + g * 2.0) - 1.5 + gl * 0.0                     # 2.5
    # env 0: no episode end
    a1_0 = (2.0 + g * 1.5) - 1.0 + gl * a2                    # 1.75 + 0.625 = 2.375
    a0_0 = (1.0 + g * 1.0) - 0.5 + gl * a1_0                  # 1.0 + 0.59375 = 1.59375
    # env 1: true termination at k = 1 — no bootstrap (the NaN is not read), recursion cut
    a1_1 = (2.0 + 0.0) - 1.0 + 0.0                            # 1.0
    a0_1 = (1.0 + g * 1.0) - 0.5 + gl * a1_1                  # 1.25
    # env 2: time limit at k = 1 — bootstrap from the terminal value 4.0, recursion cut
    a1_2 = (2.0 + g * 4.0) - 1.0 + 0.0                        # 3.0
    a0_2 = (1.0 + g * 1.0) - 0.5 + gl * a1_2                  # 1.75
    assert (a2, a1_0, a0_0, a1_1, a0_1, a1_2, a0_2) == (2.5, 2.375, 1.59375, 1.0, 1.25, 3.0, 1.75)
    want_adv = np.array([[a0_0, a0_1, a0_2], [a1_0, a1_1, a1_2], [a2, a2, a2]], np.float64)
    want_ret = want_adv + v.astype(np.float64)
    for name, fn in (("host build", host_gae), ("policy.gae_reference", policy.gae_reference)):
        adv, ret = fn(r, d, v, nv, 0.5, 0.5)
        assert np.array_equal(adv.astype(np.float64), want_adv), name
        assert np.array_equal(ret.astype(np.float64), want_ret), name


def test_gae_reference_refuses_mismatched_shapes():
    z = np.zeros
    with pytest.raises(ValueError):
        policy.gae_reference(z((3, 2)), z((3, 2)), z((3, 2)), z((2, 2)))
    with pytest.raises(ValueError):
        policy.gae_reference(z(3), z(3), z(3), z(3))
