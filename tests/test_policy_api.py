"""Device-side policies without a GPU: the two C-ABI entries at the boundary, and the policy's arithmetic (csrc/mz_policy.h, built for
the host under tests/policy_host with g++ -ffp-contract=off) against mujoco_maze_amd/policy.py.

The affine, unsquashed policy is two separately rounded fp32 operations per term in a fixed order, which numpy reproduces: bit
equality.  With a tanh the result carries libm's tanhf, so those cases go against a float64 evaluation within a bound computed from
the test's own data (`f64_and_bound`), derived as follows with eps = 2^-23:
  * a unit b + sum_i w_i x_i of n inputs, accumulated in fp32 in index order: |error| <= (n + 2) eps (|b| + sum |w_i| |x_i|), the
    standard dot-product bound (n products and n sums, gamma_(n+1) <= (n + 2) eps);
  * each tanhf: 4 eps absolute (4 ulp at |tanh| <= 1); tanh is 1-Lipschitz, so an input error passes through undiminished at most;
  * the hidden layer's errors d_j reach output u as sum_j |W2[u, j]| d_j, and the output's own dot product runs over |h_j| + d_j;
  * squash multiplies by float32(action_scale); the tests use 0.5, whose product is exact, so the bound is simply scaled by it.
If glibc's tanhf ever exceeded the 4-ulp allowance these tests would fail: that is to be reported, not absorbed by a wider bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mujoco_maze_amd import _capi, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "policy_host")
MZ_ERR_ARG = -1
EPS = 2.0 ** -23
SCALE = 0.5

_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HERE])
        lib = C.CDLL(os.path.join(HERE, "libpolicyhost.so"))
        vp, i32 = C.c_void_p, C.c_int
        lib.mzp_host_param_count.restype = i32
        lib.mzp_host_param_count.argtypes = [i32, i32, i32]
        lib.mzp_host_policy.restype = i32
        lib.mzp_host_policy.argtypes = [vp, C.c_longlong, i32, i32, i32, i32, C.c_double, vp, i32, vp]
        _lib = lib
    return _lib


def host_policy(params, obs, nu, hidden=0, squash=False, action_scale=1.0):
    """mz_policy.h on the CPU: float32 [R, nu] for the rows obs [R, obs_dim]; params [npar] or [R, npar]."""
    lib = _load()
    p, x = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(obs, np.float32)
    out = np.full((x.shape[0], nu), np.nan, np.float32)
    stride = p.shape[1] if p.ndim == 2 else 0
    rc = lib.mzp_host_policy(p.ctypes.data_as(C.c_void_p), stride, x.shape[1], nu, hidden, int(bool(squash)), float(action_scale),
                             x.ctypes.data_as(C.c_void_p), x.shape[0], out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


def random_policy(rng, obs_dim, nu, hidden, rows=None):
    """Packed params with weights and biases uniform in +-1 / sqrt(fan_in) (nn.Linear's default): [npar], or [rows, npar]."""
    def one():
        def lin(out, fan_in):
            k = 1.0 / np.sqrt(fan_in)
            return rng.uniform(-k, k, (out, fan_in)).astype(np.float32), rng.uniform(-k, k, out).astype(np.float32)
        if hidden:
            (W1, b1), (W2, b2) = lin(hidden, obs_dim), lin(nu, hidden)
            return policy.pack(W1, b1, W2, b2)
        return policy.pack_linear(*lin(nu, obs_dim))
    return one() if rows is None else np.stack([one() for _ in range(rows)])


def f64_and_bound(params, obs, nu, hidden, squash, action_scale):
    """(float64 evaluation [R, nu], bound [R, nu] on |fp32 result - it|) of the policy on rows of float32 obs; see the module docstring."""
    x = np.atleast_2d(np.asarray(obs, np.float32)).astype(np.float64)
    p = np.asarray(params, np.float32).astype(np.float64)
    R, od = x.shape
    p = np.broadcast_to(p, (R, p.shape[-1]))

    def layer(inp, dinp, Wt, b):  # value and bound of b + inp @ Wt, inp known to within dinp
        n = inp.shape[1]
        val = b + np.einsum("ri,rio->ro", inp, Wt)
        mag = np.abs(b) + np.einsum("ri,rio->ro", np.abs(inp) + dinp, np.abs(Wt))
        return val, (n + 2) * EPS * mag + np.einsum("ri,rio->ro", dinp, np.abs(Wt))

    zero = np.zeros_like(x)
    if hidden:
        o1, o2, o3 = od * hidden, od * hidden + hidden, od * hidden + hidden + hidden * nu
        pre, e1 = layer(x, zero, p[:, :o1].reshape(R, od, hidden), p[:, o1:o2])
        h, dh = np.tanh(pre), e1 + 4 * EPS
        acc, e = layer(h, dh, p[:, o2:o3].reshape(R, hidden, nu), p[:, o3:])
    else:
        acc, e = layer(x, zero, p[:, : od * nu].reshape(R, od, nu), p[:, od * nu:])
    if squash:
        s = float(np.float32(action_scale))
        assert np.frexp(s)[0] == 0.5, "the bound assumes a power-of-two action_scale (an exact product)"
        return s * np.tanh(acc), abs(s) * (e + 4 * EPS)
    return acc, e


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------- the C-ABI boundary
def test_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "mazestep.h")).read()
    act = re.search(r"int32_t\s+mz_policy_act\s*\(([^;]*)\);", header)
    roll = re.search(r"int32_t\s+mz_rollout_policy\s*\(([^;]*)\);", header)
    assert act and roll, "include/mazestep.h does not declare mz_policy_act / mz_rollout_policy"
    a = [s.strip() for s in act.group(1).replace("\n", " ").split(",")]
    r = [s.strip() for s in roll.group(1).replace("\n", " ").split(",")]
    assert len(a) == 9 and a[0].startswith("mz_handle*") and a[2] == "int64_t param_env_stride" and a[5] == "double action_scale" and a[-1] == "void* stream"
    assert len(r) == 15 and r[1] == "int32_t n_steps" and r[3] == "int64_t param_env_stride" and r[7] == "float* obs_dev" and r[-2] == "float* actions_seq_dev"
    assert "mz_policy_act" in _capi.SYMBOLS and "mz_rollout_policy" in _capi.SYMBOLS
    lib = _capi.load()
    assert hasattr(lib, "mz_policy_act") and hasattr(lib, "mz_rollout_policy")
    assert re.search(r"#define MZ_ABI_VERSION 8\b", header)
    assert re.search(r"#define MZ_POLICY_MAX_HIDDEN 64\b", header) and policy.MAX_HIDDEN == 64
    # the defining property, the in/out observation buffer and the two notes on stale observations are part of the interface
    assert re.search(r"exactly as this loop on the same stream would", header)
    assert "IN/OUT" in header and re.search(r"mz_set_state does NOT refresh", header) and "all-zero mask" in header


def test_entries_refuse_a_null_handle():
    lib = _capi.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.mz_policy_act(None, p, 0, 0, 0, 1.0, p, p, None) == MZ_ERR_ARG
    assert lib.mz_rollout_policy(None, 4, p, 0, 0, 0, 1.0, p, p, p, None, None, None, None, None) == MZ_ERR_ARG


# ---------------------------------------------------------------------------------------------- the arithmetic
DIMS = [(od, nu) for od in (7, 30, 123) for nu in (2, 8)]


@pytest.mark.parametrize("obs_dim,nu", DIMS)
def test_host_affine_is_bit_equal_to_the_numpy_model(obs_dim, nu):
    rng = np.random.default_rng(obs_dim * 10 + nu)
    obs = rng.uniform(-3.0, 3.0, (64, obs_dim)).astype(np.float32)
    for params in (random_policy(rng, obs_dim, nu, 0), random_policy(rng, obs_dim, nu, 0, rows=64)):
        got, want = host_policy(params, obs, nu), policy.reference(params, obs, nu)
        assert got.shape == want.shape == (64, nu) and want.dtype == np.float32
        assert np.array_equal(_bits(got), _bits(want))
        # ... and it is the affine map: within the dot-product bound of float64
        val, bound = f64_and_bound(params, obs, nu, 0, False, 1.0)
        assert np.all(np.abs(got.astype(np.float64) - val) <= bound)


@pytest.mark.parametrize("squash", [0, 1])
@pytest.mark.parametrize("hidden", [1, 5, 64])
@pytest.mark.parametrize("obs_dim,nu", DIMS)
def test_host_tanh_paths_within_the_derived_bound(obs_dim, nu, hidden, squash):
    rng = np.random.default_rng(obs_dim * 1000 + nu * 100 + hidden * 2 + squash)
    obs = rng.uniform(-3.0, 3.0, (64, obs_dim)).astype(np.float32)
    for params in (random_policy(rng, obs_dim, nu, hidden), random_policy(rng, obs_dim, nu, hidden, rows=64)):
        val, bound = f64_and_bound(params, obs, nu, hidden, squash, SCALE)
        for name, got in (("host build", host_policy(params, obs, nu, hidden, squash, SCALE)),
                          ("policy.reference", policy.reference(params, obs, nu, hidden, squash, SCALE))):
            err = np.abs(got.astype(np.float64) - val)
            print(f"{name}: obs_dim {obs_dim} nu {nu} H {hidden} squash {squash}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
            assert np.all(err <= bound), name
    # affine with squash: the same bound without a hidden layer
    p0 = random_policy(rng, obs_dim, nu, 0)
    if squash:
        val, bound = f64_and_bound(p0, obs, nu, 0, 1, SCALE)
        assert np.all(np.abs(host_policy(p0, obs, nu, 0, 1, SCALE).astype(np.float64) - val) <= bound)


def test_per_row_policies_are_the_rows_own():
    rng = np.random.default_rng(3)
    obs = rng.uniform(-3.0, 3.0, (9, 11)).astype(np.float32)
    params = random_policy(rng, 11, 3, 5, rows=9)
    got, ref = host_policy(params, obs, 3, 5, 1, 2.0), policy.reference(params, obs, 3, 5, True, 2.0)
    for r in range(9):
        assert np.array_equal(_bits(got[r]), _bits(host_policy(params[r], obs[r: r + 1], 3, 5, 1, 2.0)[0]))
        assert np.array_equal(_bits(ref[r]), _bits(policy.reference(params[r], obs[r], 3, 5, True, 2.0)))


def test_nan_propagates():
    rng = np.random.default_rng(4)
    obs = rng.uniform(-3.0, 3.0, (4, 7)).astype(np.float32)
    obs[1, 3] = np.nan
    for hidden, squash in ((0, 0), (0, 1), (5, 0), (5, 1)):
        params = random_policy(rng, 7, 2, hidden)
        for out in (host_policy(params, obs, 2, hidden, squash), policy.reference(params, obs, 2, hidden, bool(squash))):
            assert np.isnan(out[1]).all() and np.isfinite(out[[0, 2, 3]]).all()


# ---------------------------------------------------------------------------------------------- packing
def test_param_count():
    lib = _load()
    for od, nu, H in ((7, 2, 0), (30, 8, 0), (123, 8, 64), (7, 2, 1), (22, 5, 17)):
        want = od * H + H + H * nu + nu if H else od * nu + nu
        assert policy.param_count(od, nu, H) == want == lib.mzp_host_param_count(od, nu, H)
    assert policy.param_count(123, 8, 64) * 4 < 40 * 1024
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            policy.param_count(7, 2, bad)


@pytest.mark.parametrize("use_torch", [False, True])
def test_pack_round_trips_against_nn_linear_orientation(use_torch):
    import torch

    rng = np.random.default_rng(5)
    od, nu, H = 30, 8, 5
    x = rng.uniform(-3.0, 3.0, (64, od)).astype(np.float32)
    W, b = rng.uniform(-0.2, 0.2, (nu, od)).astype(np.float32), rng.uniform(-0.2, 0.2, nu).astype(np.float32)
    W1, b1 = rng.uniform(-0.2, 0.2, (H, od)).astype(np.float32), rng.uniform(-0.2, 0.2, H).astype(np.float32)
    W2, b2 = rng.uniform(-0.4, 0.4, (nu, H)).astype(np.float32), rng.uniform(-0.4, 0.4, nu).astype(np.float32)
    conv = (lambda a: torch.nn.Parameter(torch.as_tensor(a))) if use_torch else (lambda a: a)
    p0 = policy.pack_linear(conv(W), conv(b))
    p1 = policy.pack(conv(W1), conv(b1), conv(W2), conv(b2))
    assert p0.dtype == p1.dtype == np.float32 and p0.shape == (policy.param_count(od, nu, 0),) and p1.shape == (policy.param_count(od, nu, H),)
    assert np.array_equal(p0[: od * nu].reshape(od, nu), W.T) and np.array_equal(p0[od * nu:], b)
    x64 = x.astype(np.float64)
    want0 = x64 @ W.T.astype(np.float64) + b
    want1 = np.tanh(x64 @ W1.T.astype(np.float64) + b1) @ W2.T.astype(np.float64) + b2
    for params, hidden, want in ((p0, 0, want0), (p1, H, want1)):
        val, bound = f64_and_bound(params, x, nu, hidden, False, 1.0)
        assert np.allclose(val, want, rtol=0, atol=1e-12)  # the test's float64 evaluation is the textbook formula
        for got in (policy.reference(params, x, nu, hidden), host_policy(params, x, nu, hidden)):
            assert np.all(np.abs(got.astype(np.float64) - want) <= bound + 1e-12)


def test_pack_and_reference_refuse_wrong_shapes():
    z = np.zeros
    with pytest.raises(ValueError):
        policy.pack_linear(z((2, 7)), z(3))
    with pytest.raises(ValueError):
        policy.pack(z((5, 7)), z(5), z((2, 4)), z(2))
    with pytest.raises(ValueError):
        policy.pack(z((65, 7)), z(65), z((2, 65)), z(2))
    with pytest.raises(ValueError):
        policy.reference(z(17), z((3, 7)), 2)  # 7 * 2 + 2 = 16
    with pytest.raises(ValueError):
        policy.reference(z((4, 16)), z((3, 7)), 2)
    assert policy.reference(z(16), z(7), 2).shape == (2,)
