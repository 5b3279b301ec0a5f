"""Normalised observations and the return scan without a GPU: the two C-ABI entries at the boundary, and the arithmetic of
mz_bind_obs_norm (csrc/mz_policy.h mzp_norm_elem) and mz_return_scan (csrc/mz_returns.h), built for the host under tests/norm_host with
g++ -ffp-contract=off, against mujoco_maze_amd/policy.py; and normalize.RunningMeanStd on CPU torch against numpy.

A normalised element is a difference, a product and two selects, each rounded on its own: bit equality with numpy, NaN, +-inf, -0.0,
inv_std = 0 and clip = inf included, and therefore bit equality end to end for an affine or a ReLU network without squash.  The scan
is a product, a sum and two selects per step: bit equality — and a four-step case whose expected numbers are written out below, so
that the C scan and its numpy mirror cannot agree on a wrong recurrence."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mujoco_maze_amd import _capi, policy
from tests.test_deep_policy_api import random_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "norm_host")
MZ_ERR_ARG = -1

_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HERE])
        lib = C.CDLL(os.path.join(HERE, "libnormhost.so"))
        vp, i32 = C.c_void_p, C.c_int
        lib.mzh_norm_rows.restype = i32
        lib.mzh_norm_rows.argtypes = [vp, i32, i32, vp, vp, C.c_double, vp]
        lib.mzh_norm_policy.restype = i32
        lib.mzh_norm_policy.argtypes = [vp, C.c_longlong, i32, i32, vp, vp, i32, vp, vp, C.c_double, vp]
        lib.mzh_return_scan.restype = i32
        lib.mzh_return_scan.argtypes = [i32, i32, vp, vp, C.c_double, vp, vp, vp, vp]
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def host_norm(obs, mean, inv_std, clip):
    x, m, s = (np.ascontiguousarray(a, np.float32) for a in (obs, mean, inv_std))
    y = np.full(x.shape, 7.0, np.float32)
    rc = _load().mzh_norm_rows(_p(x), x.shape[0], x.shape[1], _p(m), _p(s), clip, _p(y))
    assert rc == 0, rc
    return y


def host_norm_policy(params, obs, nu, hidden, activation, mean, inv_std, clip):
    p, x, m, s = (np.ascontiguousarray(a, np.float32) for a in (params, obs, mean, inv_std))
    widths, act = policy.net_shape(hidden, activation)
    shape = (C.c_int * 4)(len(widths), *(widths + (0, 0))[:2], act)
    out = np.full((x.shape[0], nu), np.nan, np.float32)
    rc = _load().mzh_norm_policy(_p(p), p.shape[1] if p.ndim == 2 else 0, x.shape[1], nu, shape, _p(x), x.shape[0], _p(m), _p(s), clip, _p(out))
    assert rc == 0, rc
    return out


def host_scan(rewards, dones, gamma, carry, length_carry=None, with_len=True):
    """mzr_scan on the CPU over [K, N] rows; carry / length_carry are updated in place.  Returns (ret_seq, len_seq or None)."""
    r, d = np.ascontiguousarray(rewards, np.float32), np.ascontiguousarray(dones, np.uint8)
    ret = np.full(r.shape, np.nan, np.float32)
    ln = np.full(r.shape, -7, np.int32) if (with_len and length_carry is not None) else None
    rc = _load().mzh_return_scan(r.shape[0], r.shape[1], _p(r), _p(d), gamma, _p(carry), _p(length_carry), _p(ret), _p(ln))
    assert rc == 0, rc
    return ret, ln


def normaliser_inputs(rng, rows, obs_dim):
    """Rows of O(1) .. O(20) values with the special cases of the issue: NaN, +-inf and -0.0 entries, a constant column (d == 0), a
    column with inv_std = 0, one with a huge inv_std; (obs, mean, inv_std)."""
    x = (rng.normal(size=(rows, obs_dim)) * rng.uniform(0.01, 20.0, obs_dim)).astype(np.float32)
    mean = (x.mean(axis=0) + rng.normal(size=obs_dim) * 0.1).astype(np.float32)
    inv = (1.0 / (x.std(axis=0) + 0.1)).astype(np.float32)
    x[:, 2] = np.float32(1.25)
    mean[2] = np.float32(1.25)  # a constant column: d == 0
    inv[2] = np.float32(3.0e38)
    inv[3] = 0.0
    inv[4] = np.float32(1.0e30)  # a huge product, far beyond any finite clip
    x[0, 0], x[1, 1], x[2, 5], x[3, 6], x[4, 0] = np.nan, np.inf, -np.inf, -0.0, -0.0
    x[5, 3] = np.inf  # inf * 0 = NaN, which passes through
    mean[6] = -0.0
    return x, mean, inv


# ---------------------------------------------------------------------------------------------- the C-ABI boundary
def test_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "mazestep.h")).read()
    want = {
        "mz_bind_obs_norm": "mz_handle* h, const float* mean_dev, const float* inv_std_dev, double clip, void* stream",
        "mz_return_scan": "mz_handle* h, int32_t n_steps, const float* reward_dev, const uint8_t* done_dev, double gamma, float* carry_dev, "
                          "int32_t* len_carry_dev, float* ret_seq_dev, int32_t* len_seq_dev, void* stream",
    }
    lib = _capi.load()
    for name, args in want.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\);", header)
        assert m, f"include/mazestep.h does not declare {name}"
        assert " ".join(m.group(1).split()) == args
        assert name in _capi.SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == args.count(",") + 1
    assert re.search(r"#define MZ_ABI_VERSION 8\b", header)  # additive entries
    # the formula, the raw / normalised split and the recurrence are part of the interface
    assert "d = x[i] - mean[i];   y = d * inv_std[i];   y = y < -c ? -c : (y > c ? c : y)" in header
    assert "p = g * carry;  s = p + reward[k];  ret_seq[k] = s;  len = len + 1;  len_seq[k] = len" in header
    assert "carry = done[k] ? 0.0f : s;         len = done[k] ? 0 : len" in header
    for word in ("normalised", "raw", "final_obs", "obs_seq_dev", "task predicate", '"obs_norm"'):
        assert word in header, word


def test_entries_refuse_a_null_handle():
    lib = _capi.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.mz_bind_obs_norm(None, p, p, 10.0, None) == MZ_ERR_ARG
    assert lib.mz_bind_obs_norm(None, None, None, 10.0, None) == MZ_ERR_ARG
    assert lib.mz_return_scan(None, 4, p, p, 0.99, p, p, p, p, None) == MZ_ERR_ARG


# ---------------------------------------------------------------------------------------------- normalised rows
@pytest.mark.parametrize("obs_dim", [7, 30, 123])
def test_host_normalised_rows_are_bit_equal_to_the_numpy_model(obs_dim):
    rng = np.random.default_rng(obs_dim)
    x, mean, inv = normaliser_inputs(rng, 64, obs_dim)
    for clip in (0.7, 10.0, float("inf")):
        got, want = host_norm(x, mean, inv, clip), policy.normalize_reference(x, mean, inv, clip)
        assert got.dtype == want.dtype == np.float32 and got.shape == x.shape
        assert np.array_equal(_bits(got), _bits(want))
        c = np.float32(clip)
        assert np.isnan(got[0, 0]) and np.isnan(got[5, 3])  # a NaN passes through both selects
        assert got[1, 1] == c and got[2, 5] == -c  # +-inf becomes +-c (clip = inf: stays +-inf)
        assert (got[:, 2] == 0).all()  # the constant column, whatever inv_std is
        assert (got[np.isfinite(x[:, 3]), 3] == 0).all()  # inv_std = 0
        fin = np.isfinite(x[:, 4])
        if np.isfinite(clip):
            assert (np.abs(got[fin, 4]) == c).all()  # |d * 1e30| is far beyond any clip
        ok = ~np.isnan(got)
        assert (np.abs(got[ok]) <= c).all()
        if np.isfinite(clip):
            inner = ok & (np.abs(got) < c)
            with np.errstate(invalid="ignore"):
                y = ((x - mean).astype(np.float32) * inv).astype(np.float32)
            assert np.array_equal(_bits(got[inner]), _bits(y[inner]))  # no rounding from the clip
    # -0.0 - (-0.0) = +0.0 ... the signs are IEEE's, pinned by the bit comparison above; the clip itself is a float32 of the double
    assert np.array_equal(_bits(host_norm(x, mean, inv, 0.1)), _bits(policy.normalize_reference(x, mean, inv, np.float32(0.1))))


def test_normalize_reference_refuses_wrong_shapes_and_clips():
    x = np.zeros((4, 7), np.float32)
    with pytest.raises(ValueError, match="mean and inv_std"):
        policy.normalize_reference(x, np.zeros(6, np.float32), np.zeros(6, np.float32), 1.0)
    for clip in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="clip"):
            policy.normalize_reference(x, np.zeros(7, np.float32), np.ones(7, np.float32), clip)


@pytest.mark.parametrize("obs_dim", [7, 30, 123])
@pytest.mark.parametrize("hidden,activation", [(0, "tanh"), ((5, 3), "relu")], ids=["affine", "relu-5-3"])
def test_networks_on_normalised_rows_are_bit_equal_end_to_end(obs_dim, hidden, activation):
    rng = np.random.default_rng(100 + obs_dim)
    x, mean, inv = normaliser_inputs(rng, 64, obs_dim)
    nu = 3
    for rows in (None, 64):
        p = random_net(rng, obs_dim, nu, hidden, rows)
        for clip in (1.5, float("inf")):
            got = host_norm_policy(p, x, nu, hidden, activation, mean, inv, clip)
            with np.errstate(invalid="ignore"):  # (row 5 carries inf * 0)
                want = policy.reference(p, policy.normalize_reference(x, mean, inv, clip), nu, hidden, activation=activation)
            assert np.array_equal(_bits(got), _bits(want))
            assert np.isnan(got[0]).all() and np.isfinite(got[10:]).all()


# ---------------------------------------------------------------------------------------------- the return scan
def scan_inputs(rng, K=37, N=130):
    """rewards and dones [K, N] with episode ends at k = 0, at k = K - 1 and in consecutive steps, and both done bits"""
    r = rng.normal(size=(K, N)).astype(np.float32)
    d = (rng.uniform(size=(K, N)) < 0.12).astype(np.uint8) * rng.integers(1, 4, (K, N)).astype(np.uint8)
    d[0, ::3] = 1
    d[K - 1, 1::3] = 2
    d[10:13, 5::7] = 1  # three consecutive steps
    d[:, 4] = 0  # one env that never finishes
    d[:, 8] = 3  # and one that always does
    return r, d


@pytest.mark.parametrize("gamma", [1.0, 0.99])
def test_host_scan_is_bit_equal_to_the_numpy_model(gamma):
    rng = np.random.default_rng(5)
    r, d = scan_inputs(rng)
    K, N = r.shape
    c0 = rng.normal(size=N).astype(np.float32)
    l0 = rng.integers(0, 50, N).astype(np.int32)
    ch, lh, cn, ln = c0.copy(), l0.copy(), c0.copy(), l0.copy()
    got, glen = host_scan(r, d, gamma, ch, lh)
    want, wlen = policy.return_scan_reference(r, d, gamma, cn, ln)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(glen, wlen) and glen.dtype == np.int32
    assert np.array_equal(_bits(ch), _bits(cn)) and np.array_equal(lh, ln)
    assert (ch[d[-1] != 0] == 0).all() and (lh[d[-1] != 0] == 0).all()
    assert np.array_equal(_bits(ch[d[-1] == 0]), _bits(got[-1][d[-1] == 0])) and not np.array_equal(ch, c0)
    # without length tracking the returns are the same and nothing else is written
    c2 = c0.copy()
    got2, none = host_scan(r, d, gamma, c2, None)
    assert none is None and np.array_equal(_bits(got2), _bits(got)) and np.array_equal(_bits(c2), _bits(ch))
    # a length carry without a len_seq
    c3, l3 = c0.copy(), l0.copy()
    got3, none = host_scan(r, d, gamma, c3, l3, with_len=False)
    assert none is None and np.array_equal(_bits(got3), _bits(got)) and np.array_equal(l3, lh)
    # fresh zeros
    fresh, flen = policy.return_scan_reference(r, d, gamma)
    z, zl = np.zeros(N, np.float32), np.zeros(N, np.int32)
    got0, glen0 = host_scan(r, d, gamma, z, zl)
    assert np.array_equal(_bits(got0), _bits(fresh)) and np.array_equal(glen0, flen)


def test_scan_of_four_steps_by_hand():
    """gamma = 0.5 (exact products): env 0 never ends; env 1 ends at k = 1 (a time limit: done = 2) and again at k = 2; carries 4.0 / 8.0
    and lengths 10 / 3 come in.
        env 0: 0.5 * 4 + 1 = 3;  0.5 * 3 + 2 = 3.5;  0.5 * 3.5 - 1 = 0.75;  0.5 * 0.75 + 0.5 = 0.875          lengths 11 12 13 14
        env 1: 0.5 * 8 + 1 = 5;  0.5 * 5 + 2 = 4.5 (done);  0 - 1 = -1 (done);  0 + 0.5 = 0.5                   lengths 4 5 | 1 | 1"""
    r = np.array([[1.0, 1.0], [2.0, 2.0], [-1.0, -1.0], [0.5, 0.5]], np.float32)
    d = np.array([[0, 0], [0, 2], [0, 1], [0, 0]], np.uint8)
    want = np.array([[3.0, 5.0], [3.5, 4.5], [0.75, -1.0], [0.875, 0.5]], np.float32)
    wlen = np.array([[11, 4], [12, 5], [13, 1], [14, 1]], np.int32)
    for scan in ("host", "numpy"):
        c, ln = np.array([4.0, 8.0], np.float32), np.array([10, 3], np.int32)
        got, glen = host_scan(r, d, 0.5, c, ln) if scan == "host" else policy.return_scan_reference(r, d, 0.5, c, ln)
        assert np.array_equal(got, want) and np.array_equal(glen, wlen), scan
        assert np.array_equal(c, np.array([0.875, 0.5], np.float32)) and np.array_equal(ln, np.array([14, 1], np.int32)), scan
    # an episode end in the LAST step leaves zero carries
    c, ln = np.array([4.0, 8.0], np.float32), np.array([10, 3], np.int32)
    host_scan(r[:3], d[:3], 0.5, c, ln)
    assert np.array_equal(c, np.array([0.75, 0.0], np.float32)) and np.array_equal(ln, np.array([13, 0], np.int32))
    # a NaN return does not survive the episode's end
    rn = r.copy()
    rn[0, 1] = np.nan
    c, ln = np.zeros(2, np.float32), np.zeros(2, np.int32)
    got, _ = host_scan(rn, d, 0.5, c, ln)
    assert np.isnan(got[:2, 1]).all() and np.array_equal(got[2:, 1], want[2:, 1])


@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("K1", [1, 12, 36])
def test_split_scans_equal_one_scan(K1, gamma):
    rng = np.random.default_rng(9)
    r, d = scan_inputs(rng)
    N = r.shape[1]
    for scan in (host_scan, policy.return_scan_reference):
        c, ln = np.zeros(N, np.float32), np.zeros(N, np.int32)
        whole, wlen = scan(r, d, gamma, c, ln)
        c2, l2 = np.zeros(N, np.float32), np.zeros(N, np.int32)
        a, al = scan(r[:K1], d[:K1], gamma, c2, l2)
        b, bl = scan(r[K1:], d[K1:], gamma, c2, l2)
        assert np.array_equal(_bits(np.concatenate([a, b])), _bits(whole)) and np.array_equal(np.concatenate([al, bl]), wlen)
        assert np.array_equal(_bits(c2), _bits(c)) and np.array_equal(l2, ln)


def test_gamma_one_gives_episode_returns_and_lengths():
    rng = np.random.default_rng(13)
    r, d = scan_inputs(rng)
    K, N = r.shape
    got, glen = host_scan(r, d, 1.0, np.zeros(N, np.float32), np.zeros(N, np.int32))
    ends = 0
    for e in range(N):
        acc, steps = np.float32(0.0), 0
        for k in range(K):
            acc = np.float32(acc + r[k, e])  # the sequential fp32 sum of the episode's rewards
            steps += 1
            if d[k, e]:
                assert got[k, e].view(np.int32) == acc.view(np.int32) and glen[k, e] == steps
                acc, steps, ends = np.float32(0.0), 0, ends + 1
    assert ends > 300 and (glen[:, 8] == 1).all() and np.array_equal(glen[:, 4], np.arange(1, K + 1))


def test_return_scan_reference_refuses_bad_arguments():
    r, d = np.zeros((3, 4), np.float32), np.zeros((3, 4), np.uint8)
    with pytest.raises(ValueError, match="share one"):
        policy.return_scan_reference(r, d[:2])
    with pytest.raises(ValueError, match="carry"):
        policy.return_scan_reference(r, d, 1.0, carry=np.zeros(4, np.float64))
    with pytest.raises(ValueError, match="length_carry"):
        policy.return_scan_reference(r, d, 1.0, length_carry=np.zeros(3, np.int32))


# ---------------------------------------------------------------------------------------------- RunningMeanStd
@pytest.mark.parametrize("shape", [(7,), ()], ids=["rows-of-7", "scalars"])
def test_running_mean_std_against_numpy_two_pass(shape):
    """10 000 rows of O(1) values merged in unequal chunks against numpy's float64 two-pass mean and variance.  Chan's merge in
    float64 accumulates an error of about n * 2^-53 ~ 1e-12 relative; rtol 1e-9 leaves a margin of about 1000."""
    import torch

    from mujoco_maze_amd.normalize import RunningMeanStd

    rng = np.random.default_rng(21)
    x = rng.normal(size=(10000,) + shape) * 1.5 + 0.7
    rms = RunningMeanStd(shape, "cpu")
    ptrs = (rms.mean32.data_ptr(), rms.inv_std32.data_ptr())
    assert rms.mean32.dtype == rms.inv_std32.dtype == torch.float32 and tuple(rms.mean32.shape) == tuple(rms.inv_std32.shape) == shape
    edges = [0, 1, 4, 130, 131, 2600, 2601, 7777, 10000]
    for a, b in zip(edges[:-1], edges[1:]):
        chunk = torch.as_tensor(x[a:b])
        if shape and (b - a) % 2 == 0 and b - a > 2:
            chunk = chunk.reshape(2, (b - a) // 2, *shape)  # [K, N, *shape] rows, as a rollout returns them
        rms.update(chunk.float().double() if a == 4 else chunk)
        assert (rms.mean32.data_ptr(), rms.inv_std32.data_ptr()) == ptrs
        assert float(rms.count) == b
    x[4:130] = x[4:130].astype(np.float32)  # (that chunk went through float32)
    mean, var = x.mean(axis=0), x.var(axis=0)
    np.testing.assert_allclose(rms.mean.numpy(), mean, rtol=1e-9, atol=0)
    np.testing.assert_allclose(rms.var.numpy(), var, rtol=1e-9, atol=0)
    assert rms.mean.dtype == torch.float64 and rms.m2.dtype == torch.float64 and rms.count.dtype == torch.float64
    assert np.array_equal(rms.mean32.numpy(), mean.astype(np.float32)) or np.allclose(rms.mean32.numpy(), mean, rtol=2.0 ** -23, atol=0)
    np.testing.assert_allclose(rms.inv_std32.numpy(), 1.0 / np.sqrt(var + 1e-8), rtol=2.0 ** -22, atol=0)
    with pytest.raises(ValueError, match="shape"):
        RunningMeanStd((7,), "cpu").update(torch.zeros(5, 6))


def test_running_mean_std_before_any_update_is_the_identity():
    from mujoco_maze_amd.normalize import RunningMeanStd

    rms = RunningMeanStd((3,), "cpu")
    assert (rms.mean32 == 0).all() and (rms.inv_std32 == 1).all() and float(rms.count) == 0
