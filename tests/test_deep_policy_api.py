"""Networks of up to two hidden layers with tanh or ReLU units, without a GPU: the three C-ABI entries at the boundary, the packed
layout, and the arithmetic of the mzp_net_* row functions (csrc/mz_policy.h, built for the host under tests/net_host with
g++ -ffp-contract=off) against mujoco_maze_amd/policy.py.

ReLU is a select that adds no rounding, so a ReLU network without squash is two separately rounded fp32 operations per term in a
fixed order at any depth, which numpy reproduces: bit equality.  With a tanh the result carries libm's tanhf; those cases go against
a float64 evaluation within a bound computed from the test's own data (`f64_and_bound_net`): the recursion documented at the top of
tests/test_policy_api.py carried through one more layer —
  * a unit of n inputs known to within d_i: |error| <= (n + 2) eps (|b| + sum |w_i| (|x_i| + d_i)) + sum |w_i| d_i;
  * a tanh hidden unit adds 4 eps (4 ulp of tanhf at |tanh| <= 1) and, 1-Lipschitz, passes its input's error on undiminished at
    most; a ReLU hidden unit is 1-Lipschitz and adds nothing;
  * the second hidden layer is a layer like the first whose inputs are the first hidden vector with its errors;
  * squash multiplies by float32(action_scale) = 0.5, an exact product: the bound is scaled by it.
For one hidden layer the function reproduces tests/test_policy_api.py f64_and_bound number for number (checked below).  The 4-ulp
allowance is not widened here: if it did not hold, these tests would fail and that would be the finding."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mujoco_maze_amd import _capi, policy
from tests.test_policy_api import EPS, SCALE, f64_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "net_host")
MZ_ERR_ARG = -1
SHAPES = [(5, 3), (3, 5), (64, 64), (64, 1), (1, 64), (7,)]

_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HERE])
        lib = C.CDLL(os.path.join(HERE, "libnethost.so"))
        vp, i32, ll, u64 = C.c_void_p, C.c_int, C.c_longlong, C.c_ulonglong
        lib.mzn_host_param_count.restype = i32
        lib.mzn_host_param_count.argtypes = [i32, i32, vp]
        lib.mzn_host_policy.restype = i32
        lib.mzn_host_policy.argtypes = [vp, ll, i32, i32, vp, i32, C.c_double, vp, i32, vp, i32]
        lib.mzn_host_sample.restype = i32
        lib.mzn_host_sample.argtypes = [vp, ll, i32, i32, vp, i32, C.c_double, u64, u64, vp, vp, i32, vp, vp, i32]
        lib.mzn_host_value.restype = i32
        lib.mzn_host_value.argtypes = [vp, ll, i32, vp, vp, i32, vp, i32]
        _lib = lib
    return _lib


def _shape(hidden, activation):
    widths, act = policy.net_shape(hidden, activation)
    return (C.c_int * 4)(len(widths), *(widths + (0, 0))[:2], act)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_policy(params, obs, nu, hidden, activation="tanh", squash=False, action_scale=1.0, legacy=False):
    p, x = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(obs, np.float32)
    out = np.full((x.shape[0], nu), np.nan, np.float32)
    rc = _load().mzn_host_policy(_ptr(p), p.shape[1] if p.ndim == 2 else 0, x.shape[1], nu, _shape(hidden, activation), int(bool(squash)),
                                 float(action_scale), _ptr(x), x.shape[0], _ptr(out), int(legacy))
    assert rc == 0, rc
    return out


def host_sample(params, obs, nu, hidden, activation="tanh", squash=False, action_scale=1.0, noise_seed=0, noise_step=0, slots=None, legacy=False):
    p, x = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(obs, np.float32)
    sl = np.ascontiguousarray(np.arange(x.shape[0]) if slots is None else slots, np.uint64)
    out, logp = np.full((x.shape[0], nu), np.nan, np.float32), np.full(x.shape[0], np.nan, np.float32)
    rc = _load().mzn_host_sample(_ptr(p), p.shape[1] if p.ndim == 2 else 0, x.shape[1], nu, _shape(hidden, activation), int(bool(squash)),
                                 float(action_scale), noise_seed, noise_step, _ptr(sl), _ptr(x), x.shape[0], _ptr(out), _ptr(logp), int(legacy))
    assert rc == 0, rc
    return out, logp


def host_value(vparams, obs, hidden, activation="tanh", legacy=False):
    p, x = np.ascontiguousarray(vparams, np.float32), np.ascontiguousarray(obs, np.float32)
    out = np.full(x.shape[0], np.nan, np.float32)
    rc = _load().mzn_host_value(_ptr(p), p.shape[1] if p.ndim == 2 else 0, x.shape[1], _shape(hidden, activation), _ptr(x), x.shape[0], _ptr(out),
                                int(legacy))
    assert rc == 0, rc
    return out


def random_net(rng, obs_dim, nout, hidden, rows=None, log_std=False):
    """Packed params with weights and biases uniform in +-1 / sqrt(fan_in) (nn.Linear's default): [count], or [rows, count]; with
    `log_std`, log_std [nout] uniform in [-1, 0] behind the network."""
    sizes = (obs_dim,) + policy.net_shape(hidden)[0] + (nout,)

    def one():
        layers = []
        for fan_in, out in zip(sizes[:-1], sizes[1:]):
            k = 1.0 / np.sqrt(fan_in)
            layers.append((rng.uniform(-k, k, (out, fan_in)).astype(np.float32), rng.uniform(-k, k, out).astype(np.float32)))
        return policy.pack_mlp(layers, log_std=rng.uniform(-1, 0, nout).astype(np.float32) if log_std else None)
    return one() if rows is None else np.stack([one() for _ in range(rows)])


def f64_and_bound_net(params, obs, nout, hidden, activation, squash, action_scale):
    """(float64 evaluation [R, nout], bound [R, nout] on |fp32 result - it|) of a network on rows of float32 obs; see the module
    docstring."""
    widths, act = policy.net_shape(hidden, activation)
    x = np.atleast_2d(np.asarray(obs, np.float32)).astype(np.float64)
    p = np.asarray(params, np.float32).astype(np.float64)
    R = x.shape[0]
    p = np.broadcast_to(p, (R, p.shape[-1]))

    def layer(inp, dinp, Wt, b):  # value and bound of b + inp @ Wt, inp known to within dinp
        n = inp.shape[1]
        val = b + np.einsum("ri,rio->ro", inp, Wt)
        mag = np.abs(b) + np.einsum("ri,rio->ro", np.abs(inp) + dinp, np.abs(Wt))
        return val, (n + 2) * EPS * mag + np.einsum("ri,rio->ro", dinp, np.abs(Wt))

    h, dh, off = x, np.zeros_like(x), 0
    for k, m in enumerate(widths + (nout,)):
        n = h.shape[1]
        acc, e = layer(h, dh, p[:, off: off + n * m].reshape(R, n, m), p[:, off + n * m: off + n * m + m])
        off += n * m + m
        if k < len(widths):
            h, dh = (np.maximum(acc, 0.0), e) if act else (np.tanh(acc), e + 4 * EPS)
    if squash:
        s = float(np.float32(action_scale))
        assert np.frexp(s)[0] == 0.5, "the bound assumes a power-of-two action_scale (an exact product)"
        return s * np.tanh(acc), abs(s) * (e + 4 * EPS)
    return acc, e


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _obs_rows(rng, rows, obs_dim):
    """Rows in [-2, 2] with a NaN in row 1 and a -0.0 in row 2 (and in the last column of every row)."""
    x = rng.uniform(-2, 2, (rows, obs_dim)).astype(np.float32)
    x[:, -1] = -0.0
    x[1, obs_dim // 2] = np.nan
    x[2, 0] = -0.0
    return x


# ---------------------------------------------------------------------------------------------- the C-ABI boundary
def test_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "mazestep.h")).read()
    want = {"mz_net_act": 9, "mz_net_value": 5, "mz_rollout_net": 18}
    lib = _capi.load()
    for name, nargs in want.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\);", header)
        assert m, f"include/mazestep.h does not declare {name}"
        args = [s.strip() for s in m.group(1).replace("\n", " ").split(",")]
        assert len(args) == nargs and args[0].startswith("mz_handle*") and args[-1] == "void* stream", (name, args)
        assert name in _capi.SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs, name
    r = [s.strip() for s in re.search(r"int32_t\s+mz_rollout_net\s*\(([^;]*)\);", header).group(1).replace("\n", " ").split(",")]
    assert r[1] == "int32_t n_steps" and r[2] == "const mz_net* actor" and r[3] == "int32_t sample" and r[6] == "const mz_net* critic"
    assert r[7] == "float* value_seq_dev" and r[8] == "float* next_value_seq_dev" and r[9] == "float* obs_dev" and r[-2] == "float* logp_seq_dev"
    # the struct: field for field what _capi.MzNet lays out, its size first
    body = re.search(r"typedef struct mz_net \{(.*?)\} mz_net;", header, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _capi.MzNet._fields_] and fields[0] == "struct_size"
    assert C.sizeof(_capi.MzNet) == 48 and _capi.MzNet.params_dev.offset == 32 and _capi.MzNet.action_scale.offset == 24
    assert re.search(r"#define MZ_NET_MAX_HIDDEN_LAYERS 2\b", header) and policy.MAX_HIDDEN_LAYERS == 2
    assert re.search(r"#define MZ_ACT_TANH 0\b", header) and re.search(r"#define MZ_ACT_RELU 1\b", header)
    assert policy.ACTIVATIONS == ("tanh", "relu") and (_capi.ACT_TANH, _capi.ACT_RELU) == (0, 1)
    assert re.search(r"#define MZ_ABI_VERSION 8\b", header), "additive entries keep the ABI number"


def test_entries_refuse_a_null_handle():
    lib = _capi.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    net = _capi.make_net(p, 0, (), 0)
    assert lib.mz_net_act(None, C.byref(net), 0, 0, 0, p, p, None, None) == MZ_ERR_ARG
    assert lib.mz_net_value(None, C.byref(net), p, p, None) == MZ_ERR_ARG
    assert lib.mz_rollout_net(None, 4, C.byref(net), 0, 0, 0, None, None, None, p, p, p, None, None, None, None, None, None) == MZ_ERR_ARG


# ---------------------------------------------------------------------------------------------- layout
def test_param_count_accepts_an_int_or_a_sequence():
    assert policy.param_count(7, 2, 0) == 7 * 2 + 2
    assert policy.param_count(7, 2, 5) == policy.param_count(7, 2, (5,)) == policy.param_count(7, 2, [5]) == 7 * 5 + 5 + 5 * 2 + 2
    assert policy.param_count(7, 2, (5, 3)) == 7 * 5 + 5 + 5 * 3 + 3 + 3 * 2 + 2
    assert policy.param_count(7, 2, (5, 3), stochastic=True) == policy.param_count(7, 2, (5, 3)) + 2
    assert policy.param_count(123, 8, (64, 64)) == 123 * 64 + 64 + 64 * 64 + 64 + 64 * 8 + 8
    lib = _load()
    for od, nout, hidden in ((7, 2, 0), (7, 2, 5), (123, 8, (64, 64)), (7, 1, (1, 64)), (7, 1, (64, 1))):
        assert lib.mzn_host_param_count(od, nout, _shape(hidden, "relu")) == policy.param_count(od, nout, hidden)


@pytest.mark.parametrize("with_log_std", [False, True])
def test_pack_mlp_layout_against_hand_built_vectors(with_log_std):
    rng = np.random.default_rng(3)
    od, nu = 7, 2
    ls = rng.normal(size=nu).astype(np.float32) if with_log_std else None
    tail = [ls] if with_log_std else []

    def lin(out, inp):
        return rng.normal(size=(out, inp)).astype(np.float32), rng.normal(size=out).astype(np.float32)

    (W, b) = lin(nu, od)
    want = np.concatenate([W.T.ravel(), b] + tail)
    got = policy.pack_mlp([(W, b)], log_std=ls)
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(got, policy.pack_linear(W, b, log_std=ls))
    (W1, b1), (W2, b2) = lin(5, od), lin(nu, 5)
    want = np.concatenate([W1.T.ravel(), b1, W2.T.ravel(), b2] + tail)
    got = policy.pack_mlp([(W1, b1), (W2, b2)], log_std=ls)
    assert np.array_equal(got, want) and np.array_equal(got, policy.pack(W1, b1, W2, b2, log_std=ls))
    (W1, b1), (W2, b2), (W3, b3) = lin(5, od), lin(3, 5), lin(nu, 3)
    got = policy.pack_mlp([(W1, b1), (W2, b2), (W3, b3)], log_std=ls)
    want = np.concatenate([W1.T.ravel(), b1, W2.T.ravel(), b2, W3.T.ravel(), b3] + tail)
    assert np.array_equal(got, want) and got.shape == (policy.param_count(od, nu, (5, 3), stochastic=with_log_std),)
    # element by element: W2t [H1][H2] sits behind b1, input-major
    o2 = od * 5 + 5
    assert got[o2 + 4 * 3 + 2] == W2[2, 4] and got[o2 + 5 * 3 + 1] == b2[1] and got[o2 + 5 * 3 + 3 + 2 * nu + 1] == W3[1, 2]
    with pytest.raises(ValueError, match="layers"):
        policy.pack_mlp([(W1, b1), (W2, b2), (W3, b3), (W3, b3)])
    with pytest.raises(ValueError, match=r"layers\[1\]"):
        policy.pack_mlp([(W1, b1), (W3, b3)])
    with pytest.raises(ValueError, match="layers"):
        policy.pack_mlp([])


# ---------------------------------------------------------------------------------------------- ReLU: bit equality
@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
@pytest.mark.parametrize("nu", [2, 8])
@pytest.mark.parametrize("obs_dim", [7, 123])
@pytest.mark.parametrize("hidden", SHAPES, ids=str)
def test_relu_unsquashed_equals_numpy_bit_for_bit(hidden, obs_dim, nu, per_row):
    rng = np.random.default_rng(hash((hidden, obs_dim, nu, per_row)) % 2 ** 32)
    rows = 6
    x = _obs_rows(rng, rows, obs_dim)
    p = random_net(rng, obs_dim, nu, hidden, rows if per_row else None)
    got = host_policy(p, x, nu, hidden, "relu")
    want = policy.reference(p, x, nu, hidden, activation="relu")
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isnan(got[1]).all() and np.isfinite(np.delete(got, 1, axis=0)).all(), "the NaN stays in its row and reaches every output of it"
    vp = random_net(rng, obs_dim, 1, hidden, rows if per_row else None)
    gv, wv = host_value(vp, x, hidden, "relu"), policy.value_reference(vp, x, hidden, activation="relu")
    assert np.array_equal(_bits(gv), _bits(wv)) and np.isnan(gv[1]) and np.isfinite(np.delete(gv, 1)).all()
    # a draw: with log_std = -inf the action is the mean (z = m + 0 * eps), so it equals the deterministic output; with a finite
    # log_std the log-prob depends on the noise and on log_std alone — an affine policy with the same log_std gives the same bits
    slots = np.arange(rows) + 100
    ga, gl = host_sample(np.concatenate([p, np.full(p.shape[:-1] + (nu,), -np.inf, np.float32)], axis=-1), x, nu, hidden, "relu", noise_seed=5,
                         noise_step=9, slots=slots)
    assert np.array_equal(np.isnan(ga), np.isnan(got)) and np.array_equal(ga[~np.isnan(ga)], got[~np.isnan(got)]) and np.isposinf(gl).all()
    ls = rng.uniform(-1, 0, nu).astype(np.float32)
    _, gl = host_sample(np.concatenate([p, np.broadcast_to(ls, p.shape[:-1] + (nu,))], axis=-1), x, nu, hidden, "relu", noise_seed=5, noise_step=9,
                        slots=slots)
    _, al = host_sample(np.concatenate([np.zeros(policy.param_count(obs_dim, nu, 0), np.float32), ls]), x, nu, 0, "tanh", noise_seed=5, noise_step=9,
                        slots=slots, legacy=True)
    assert np.array_equal(_bits(gl), _bits(al))


def test_relu_keeps_negative_zero_and_lets_a_nan_through():
    """All weights positive, all biases and inputs -0.0: every product and every sum is -0.0, and the select returns it unchanged at
    both layers (fmaxf(-0.0f, 0.0f) may return +0.0, and fmaxf drops a NaN)."""
    od, nu, hidden = 4, 2, (3, 2)
    layers = [(np.ones((o, i), np.float32), np.full(o, -0.0, np.float32)) for i, o in ((od, 3), (3, 2), (2, nu))]
    p = policy.pack_mlp(layers)
    x = np.full((2, od), -0.0, np.float32)
    x[1, 0] = np.nan
    got, want = host_policy(p, x, nu, hidden, "relu"), policy.reference(p, x, nu, hidden, activation="relu")
    assert np.array_equal(_bits(got), _bits(want))
    assert (got[0] == 0).all() and np.signbit(got[0]).all() and np.isnan(got[1]).all()


# ---------------------------------------------------------------------------------------------- tanh: the derived bound
def test_bound_reproduces_the_one_layer_recursion():
    rng = np.random.default_rng(1)
    x = rng.uniform(-2, 2, (5, 7)).astype(np.float32)
    for hidden in (0, 6):
        for squash in (False, True):
            p = random_net(rng, 7, 2, hidden)
            a, ea = f64_and_bound(p, x, 2, hidden, squash, SCALE)
            b, eb = f64_and_bound_net(p, x, 2, hidden, "tanh", squash, SCALE)
            assert np.array_equal(a, b) and np.array_equal(ea, eb)


@pytest.mark.parametrize("squash", [False, True], ids=["plain", "squash"])
@pytest.mark.parametrize("obs_dim,nu", [(7, 2), (123, 8)])
@pytest.mark.parametrize("hidden", SHAPES, ids=str)
def test_tanh_within_the_derived_bound(hidden, obs_dim, nu, squash):
    rng = np.random.default_rng(hash((hidden, obs_dim, nu, squash)) % 2 ** 32)
    rows = 16
    x = rng.uniform(-2, 2, (rows, obs_dim)).astype(np.float32)
    for per_row in (False, True):
        p = random_net(rng, obs_dim, nu, hidden, rows if per_row else None)
        ref, bound = f64_and_bound_net(p, x, nu, hidden, "tanh", squash, SCALE)
        for got in (host_policy(p, x, nu, hidden, "tanh", squash, SCALE), policy.reference(p, x, nu, hidden, squash, SCALE)):
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= bound).all(), (err / bound).max()
        vp = random_net(rng, obs_dim, 1, hidden, rows if per_row else None)
        vref, vbound = f64_and_bound_net(vp, x, 1, hidden, "tanh", False, 1.0)
        for got in (host_value(vp, x, hidden), policy.value_reference(vp, x, hidden)):
            assert (np.abs(got.astype(np.float64) - vref[:, 0]) <= vbound[:, 0]).all()


def test_relu_with_squash_within_the_derived_bound():
    rng = np.random.default_rng(8)
    x = rng.uniform(-2, 2, (16, 7)).astype(np.float32)
    p = random_net(rng, 7, 2, (64, 64))
    ref, bound = f64_and_bound_net(p, x, 2, (64, 64), "relu", True, SCALE)
    got = host_policy(p, x, 2, (64, 64), "relu", True, SCALE)
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()


# ---------------------------------------------------------------------------------------------- one layer, tanh: today's bits
@pytest.mark.parametrize("squash", [False, True], ids=["plain", "squash"])
@pytest.mark.parametrize("hidden", [0, 1, 7, 64])
def test_one_layer_tanh_through_the_new_functions_gives_todays_bits(hidden, squash):
    rng = np.random.default_rng(40 + hidden)
    for obs_dim, nu in ((7, 2), (123, 8)):
        x = _obs_rows(rng, 6, obs_dim)
        for per_row in (False, True):
            p = random_net(rng, obs_dim, nu, hidden, 6 if per_row else None)
            new, old = (host_policy(p, x, nu, hidden, "tanh", squash, SCALE, legacy=leg) for leg in (False, True))
            assert np.array_equal(_bits(new), _bits(old))
            sp = random_net(rng, obs_dim, nu, hidden, 6 if per_row else None, log_std=True)
            (na, nl), (oa, ol) = (host_sample(sp, x, nu, hidden, "tanh", squash, SCALE, 3, 4, np.arange(6) + 50, legacy=leg) for leg in (False, True))
            assert np.array_equal(_bits(na), _bits(oa)) and np.array_equal(_bits(nl), _bits(ol))
            vp = random_net(rng, obs_dim, 1, hidden, 6 if per_row else None)
            assert np.array_equal(_bits(host_value(vp, x, hidden)), _bits(host_value(vp, x, hidden, legacy=True)))
        # and a sequence of one width is the int
        assert np.array_equal(_bits(policy.reference(p, x, nu, hidden, squash, SCALE)),
                              _bits(policy.reference(p, x, nu, (hidden,) if hidden else 0, squash, SCALE, activation="tanh")))


# ---------------------------------------------------------------------------------------------- refusals on the Python side
def test_python_side_refusals():
    x = np.zeros((3, 7), np.float32)
    good = np.zeros(policy.param_count(7, 2, (5, 3)), np.float32)
    for fn in (lambda h, a: policy.param_count(7, 2, h), lambda h, a: policy.reference(good, x, 2, h, activation=a),
               lambda h, a: policy.value_reference(good, x, h, a), lambda h, a: policy.sample_reference(good, x, 2, h, activation=a)):
        with pytest.raises(ValueError, match="hidden"):
            fn((5, 3, 2), "tanh")  # three hidden layers
        with pytest.raises(ValueError, match="hidden"):
            fn((5, 0), "tanh")
        with pytest.raises(ValueError, match="hidden"):
            fn((65, 5), "tanh")
        with pytest.raises(ValueError, match="hidden"):
            fn(65, "tanh")
    for fn in (lambda a: policy.reference(good, x, 2, (5, 3), activation=a), lambda a: policy.value_reference(good, x, (5, 3), a),
               lambda a: policy.sample_reference(good, x, 2, (5, 3), activation=a), lambda a: policy.net_shape((5, 3), a)):
        with pytest.raises(ValueError, match="activation"):
            fn("gelu")
    with pytest.raises(ValueError, match="params must have shape"):
        policy.reference(good, x, 2, (3, 5))  # the count of (5, 3), not of (3, 5)
    with pytest.raises(ValueError, match="params must have shape"):
        policy.reference(np.zeros((2, good.size), np.float32), x, 2, (5, 3))  # two rows of parameters for three rows
    with pytest.raises(ValueError, match="params must have shape"):
        policy.sample_reference(good, x, 2, (5, 3))  # no log_std behind the network
    with pytest.raises(ValueError, match="value_params must have shape"):
        policy.value_reference(good, x, (5, 3))
    lib = _load()
    bad = (C.c_int * 4)(3, 5, 3, 0)
    assert lib.mzn_host_param_count(7, 2, bad) == MZ_ERR_ARG
