"""State-dependent log-std heads without a GPU: mz_net_sample_head / mz_rollout_head at the C-ABI boundary, and the head arithmetic
of csrc/mz_policy.h (mzp_net_sample_head_row, built for the host under tests/sac_head_host with g++ -ffp-contract=off) against
mujoco_maze_amd/policy.py and against a float64 evaluation.

By bits, where nothing but the same operations is involved: a constant head against the existing row function with a trailing
log_std; the clamp; the deterministic limit; NaN isolation.

Against float64, derived (EPS = 2^-23, twice the unit roundoff, as in tests/test_policy_api.py; `f64_and_bound_net` of
tests/test_deep_policy_api.py bounds the 2 nu output sums: e_m on the means, e_r on the raw log-stds).  Per unit:
  * ls = clamp(r): two selects, 1-Lipschitz, no rounding: e_ls = e_r;
  * s = expf(ls) (2 ulp, inside the 4 EPS below) is off by the factor exp(+-e_ls) as well: |s32 - s64| <= s (expm1(e_ls) + ..);
  * p = s eps carries s 1e-5 (the eps bar of tests/test_policy_sample_api.py) + |s eps| (4 EPS + expm1(e_ls)); z = m + p adds e_m
    and one rounding |z| EPS:   e_z = e_m + s 1e-5 + |s eps| (4 EPS + expm1(e_ls)) + |z| EPS;
  * the action is z, or A tanh(z) with A = 0.5 (an exact product), tanh 1-Lipschitz, tanhf 4 EPS:   e_a = A (e_z + 4 EPS);
  * the Gaussian term t = ((-0.5 eps^2) - ls) - c0, c0 the fp32 constant on both sides: q = eps^2 carries (2 |eps| + 1e-5) 1e-5 and
    one rounding q EPS, h = -0.5 q is exact, each difference one rounding:
        e_t = 0.5 ((2 |eps| + 1e-5) 1e-5 + q EPS) + e_ls + |h - ls| EPS + |t| EPS;
  * the row's logp adds the terms in order, one rounding per partial sum:   e_logp = sum_u e_t_u + sum_u |acc_u| EPS.
With logp_squashed the term loses c(z) = 2 ((0.6931472 - z) - softplus(-2 z)) + logA, whose slope in z is -2 tanh(z): it passes e_z
on at most doubled.  Its own fp32 evaluation goes through expf and log1pf, and the suite holds no ulp bound for log1pf — so that
part is MEASURED, not derived: where no libm bound is known none is invented.  `CORRECTION_MEASURED` below is the largest
|host t - float64 t| of the corrected term over this module's own z (every case of `test_against_float64`: the z of the float64
model rounded to fp32 and fed to mzp_head_logp_term with eps = ls = 0, where t = -C0 - c(z), logA included), and the assertion
allows four times that per unit: e_t += 2 e_z + 4 CORRECTION_MEASURED + |t| EPS.  The numpy model's figure for the form itself is
2.9e-6 up to |z| = 88 (csrc/mz_policy.h); both are in profiles/rollout/sac_head.md."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mujoco_maze_amd import _capi, policy
from tests.test_deep_policy_api import f64_and_bound_net, host_policy, random_net
from tests.test_policy_api import EPS, SCALE, _bits
from tests.test_transitions_api import _header_fields
from tests.test_transitions_api import host_sample as host_param_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "sac_head_host")
MZ_ERR_ARG = -1
# (hidden, activation): affine, tanh-5, ReLU (5, 3), ReLU (64, 64)
NETS = [(0, "tanh"), (5, "tanh"), ((5, 3), "relu"), ((64, 64), "relu")]
DIMS = [(7, 2), (30, 8)]
BOUNDS = (-20.0, 2.0)
# largest |host t - float64 t| of the corrected term over the z of test_against_float64, |z| < 45 (measured on the host build, where it
# is rounding at |t| ~ 88 rather than libm: 2.265e-6 in every case; the test prints it)
CORRECTION_MEASURED = 2.27e-6

_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HERE, "libsacheadhost.so"])
        lib = C.CDLL(os.path.join(HERE, "libsacheadhost.so"))
        vp, i32, u64, f32 = C.c_void_p, C.c_int, C.c_ulonglong, C.c_float
        lib.mzh_host_logp_term.restype = f32
        lib.mzh_host_logp_term.argtypes = [f32, f32, f32, i32, f32]
        lib.mzh_host_clamp.restype = f32
        lib.mzh_host_clamp.argtypes = [f32, f32, f32]
        lib.mzh_host_param_count.restype = i32
        lib.mzh_host_param_count.argtypes = [i32] * 5
        lib.mzh_host_sample_head.restype = i32
        lib.mzh_host_sample_head.argtypes = [vp, C.c_longlong, i32, i32, i32, i32, i32, i32, i32, C.c_double, f32, f32, i32, u64, u64, vp, vp, i32, vp, vp]
        _lib = lib
    return _lib


def host_head(params, obs, nu, hidden=0, activation="tanh", squash=False, action_scale=1.0, bounds=BOUNDS, squashed_logp=False, noise_seed=0,
              noise_step=0, slots=None):
    """mz_policy.h's head actor on the CPU: (float32 [R, nu], float32 [R]) for the rows obs [R, obs_dim]."""
    lib = _load()
    widths, act = policy.net_shape(hidden, activation)
    p, x = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(obs, np.float32)
    R = x.shape[0]
    sl = np.ascontiguousarray(np.arange(R) if slots is None else slots, np.uint64)
    out, logp = np.full((R, nu), np.nan, np.float32), np.full(R, np.nan, np.float32)
    w = (widths + (0, 0))[:2]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.mzh_host_sample_head(vp(p), p.shape[1] if p.ndim == 2 else 0, x.shape[1], nu, len(widths), w[0], w[1], act, int(bool(squash)),
                                  float(action_scale), bounds[0], bounds[1], int(bool(squashed_logp)), noise_seed, noise_step, vp(sl), vp(x), R, vp(out),
                                  vp(logp))
    assert rc == 0, rc
    return out, logp


def model_head(params, obs, nu, bounds=BOUNDS, **kw):
    """policy.sample_reference on a head actor, with host_head's argument names"""
    return policy.sample_reference(params, obs, nu, log_std="state", log_std_bounds=bounds, **kw)


def with_head(net, obs_dim, nu, hidden, Wh_t, bh):
    """The head vector of a mean network: net [count] or [R, count] (policy.param_count(obs_dim, nu, hidden)) with the raw log-std
    columns Wh_t [.., nin, nu] and biases bh [.., nu] put behind the means' in the output layer — the inverse of policy.mean_actor."""
    net = np.asarray(net, np.float32)
    widths = policy.net_shape(hidden)[0]
    nin = widths[-1] if widths else obs_dim
    lead = net.shape[:-1]
    body = net.shape[-1] - (nin * nu + nu)
    Wt = net[..., body: body + nin * nu].reshape(lead + (nin, nu))
    W2 = np.concatenate([Wt, np.broadcast_to(np.asarray(Wh_t, np.float32), lead + (nin, nu))], axis=-1).reshape(lead + (nin * 2 * nu,))
    b2 = np.concatenate([net[..., body + nin * nu:], np.broadcast_to(np.asarray(bh, np.float32), lead + (nu,))], axis=-1)
    return np.concatenate([net[..., :body], W2, b2], axis=-1).astype(np.float32)


def constant_head(net, obs_dim, nu, hidden, bias):
    widths = policy.net_shape(hidden)[0]
    nin = widths[-1] if widths else obs_dim
    return with_head(net, obs_dim, nu, hidden, np.zeros((nin, nu), np.float32), bias)


def random_head(rng, obs_dim, nu, hidden, rows=None):
    """A head actor with nn.Linear's default initialisation throughout (the raw log-stds then lie well inside BOUNDS)"""
    return random_net(rng, obs_dim, 2 * nu, hidden, rows=rows)


# ---------------------------------------------------------------------------------------------- the C-ABI boundary
def test_struct_fields_equal_the_header_in_order():
    header = open(os.path.join(ROOT, "include", "mazestep.h")).read()
    fields = _header_fields(header, "mz_head")
    assert fields == [f[0] for f in _capi.MzHead._fields_] == ["struct_size", "kind", "log_std_min", "log_std_max", "logp_squashed", "reserved"]
    assert C.sizeof(_capi.MzHead) == 24
    assert [(_capi.MzHead.__dict__[n].offset, _capi.MzHead.__dict__[n].size) for n in fields] == [(0, 4), (4, 4), (8, 4), (12, 4), (16, 4), (20, 4)]
    assert re.search(r"#define MZ_HEAD_STATE_STD 1\b", header) and _capi.HEAD_STATE_STD == 1
    assert re.search(r"#define MZ_ABI_VERSION 8\b", header)  # additive entries
    # the structs the head does not ride in keep their sizes
    assert C.sizeof(_capi.MzNet) == 48 and C.sizeof(_capi.MzNoise) == 24 and C.sizeof(_capi.MzRolloutIo) == 8 + 16 * 8
    hd = _capi.make_head(-20.0, 2.0, True)
    assert (hd.struct_size, hd.kind, hd.log_std_min, hd.log_std_max, hd.logp_squashed, hd.reserved) == (24, 1, -20.0, 2.0, 1, 0)


def test_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "mazestep.h")).read()
    smp = re.search(r"int32_t\s+mz_net_sample_head\s*\(([^;]*)\);", header)
    roll = re.search(r"int32_t\s+mz_rollout_head\s*\(([^;]*)\);", header)
    assert smp and roll, "include/mazestep.h does not declare mz_net_sample_head / mz_rollout_head"
    assert [s.strip() for s in smp.group(1).replace("\n", " ").split(",")] == [
        "mz_handle* h", "const mz_net* actor", "const mz_head* head", "const mz_noise* noise", "const float* obs_dev", "float* actions_dev",
        "float* logp_dev", "void* stream"]
    assert [s.strip() for s in roll.group(1).replace("\n", " ").split(",")] == ["mz_handle* h", "const mz_rollout_io* io", "const mz_head* head",
                                                                                "void* stream"]
    assert "mz_net_sample_head" in _capi.SYMBOLS and "mz_rollout_head" in _capi.SYMBOLS
    lib = _capi.load()
    assert hasattr(lib, "mz_net_sample_head") and hasattr(lib, "mz_rollout_head")
    assert len(lib.mz_net_sample_head.argtypes) == 8 and len(lib.mz_rollout_head.argtypes) == 4
    # the entries they extend keep their signatures
    assert re.search(r"int32_t\s+mz_net_sample\s*\(([^;]*)\);", header).group(1).count(",") == 6
    assert re.search(r"int32_t\s+mz_rollout_ex\s*\(([^;]*)\);", header).group(1).count(",") == 2


def test_entries_refuse_a_null_handle():
    lib = _capi.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    net = _capi.make_net(p, 0, (), 0, True, 0.9)
    nz = _capi.make_noise(_capi.NOISE_PRE_SQUASH, 1, 2)
    hd = _capi.make_head(-20.0, 2.0, True)
    io = _capi.make_rollout_io(4, actor=net, noise=nz, obs_dev=p, reward_dev=p, done_dev=p)
    assert lib.mz_net_sample_head(None, C.byref(net), C.byref(hd), C.byref(nz), p, p, p, None) == MZ_ERR_ARG
    assert lib.mz_net_sample_head(None, C.byref(net), None, C.byref(nz), p, p, p, None) == MZ_ERR_ARG
    assert lib.mz_rollout_head(None, C.byref(io), C.byref(hd), None) == MZ_ERR_ARG
    assert lib.mz_rollout_head(None, C.byref(io), None, None) == MZ_ERR_ARG
    assert lib.mz_rollout_head(None, None, None, None) == MZ_ERR_ARG


# ---------------------------------------------------------------------------------------------- the packed layout
def test_param_count_pack_and_mean_actor():
    rng = np.random.default_rng(0)
    for obs_dim, nu in DIMS:
        for hidden, _ in NETS:
            widths = policy.net_shape(hidden)[0]
            sizes = (obs_dim,) + widths + (2 * nu,)
            count = sum(a * b + b for a, b in zip(sizes[:-1], sizes[1:]))
            assert policy.param_count(obs_dim, nu, hidden, log_std="state") == count
            assert policy.param_count(obs_dim, nu, hidden, stochastic=True, log_std="state") == count  # no trailing log_std
            assert _load().mzh_host_param_count(obs_dim, nu, len(widths), *(widths + (0, 0))[:2]) == count
            layers = [(rng.normal(size=(o, i)).astype(np.float32), rng.normal(size=o).astype(np.float32))
                      for i, o in zip((obs_dim,) + widths, widths + (nu,))]
            nin = layers[-1][0].shape[1]
            Wh, bh = rng.normal(size=(nu, nin)).astype(np.float32), rng.normal(size=nu).astype(np.float32)
            packed = policy.pack_mlp(layers, log_std_head=(Wh, bh))
            assert packed.shape == (count,) and packed.dtype == np.float32
            mean = policy.pack_mlp(layers)
            assert np.array_equal(packed, with_head(mean, obs_dim, nu, hidden, Wh.T, bh))
            # the output layer, input-major: row i holds the nu mean weights of input i, then its nu log-std weights
            Wt = packed[count - 2 * nu - nin * 2 * nu: count - 2 * nu].reshape(nin, 2 * nu)
            assert np.array_equal(Wt[:, :nu], layers[-1][0].T) and np.array_equal(Wt[:, nu:], Wh.T)
            assert np.array_equal(packed[-2 * nu: -nu], layers[-1][1]) and np.array_equal(packed[-nu:], bh)
            assert np.array_equal(policy.mean_actor(packed, obs_dim, nu, hidden), mean)
            rows = np.stack([packed, packed + 1])
            assert np.array_equal(policy.mean_actor(rows, obs_dim, nu, hidden), np.stack([mean, mean + 1]))
    with pytest.raises(ValueError):
        policy.pack_mlp(layers, log_std=bh, log_std_head=(Wh, bh))
    with pytest.raises(ValueError):
        policy.pack_mlp(layers, log_std_head=(Wh[:, :-1], bh))
    with pytest.raises(ValueError):
        policy.mean_actor(mean, obs_dim, nu, hidden)
    with pytest.raises(ValueError):
        policy.param_count(7, 2, 0, log_std="learned")


def test_the_python_side_refuses_what_the_library_refuses():
    z = np.zeros
    par = z(policy.param_count(7, 2, 0, log_std="state"), np.float32)
    ok = dict(log_std="state", squash=True)
    a, lp = policy.sample_reference(par, z((3, 7)), 2, squashed_logp=True, **ok)
    assert a.shape == (3, 2) and lp.shape == (3,)
    for bad in (dict(ok, log_std="learned"), dict(ok, noise="action"), dict(log_std="state", squashed_logp=True),
                dict(ok, log_std_bounds=(1.0, -1.0)), dict(ok, log_std_bounds=(np.nan, 1.0)), dict(ok, log_std_bounds=(1.0,)),
                dict(squashed_logp=True, squash=True)):
        with pytest.raises(ValueError):
            policy.sample_reference(par if bad.get("log_std") == "state" else z(18, np.float32), z((3, 7)), 2, **bad)
    with pytest.raises(ValueError):  # the parametrised vector is not a head vector
        policy.sample_reference(z(18, np.float32), z((3, 7)), 2, log_std="state")


# ---------------------------------------------------------------------------------------------- by bits
@pytest.mark.parametrize("hidden,activation", NETS)
@pytest.mark.parametrize("obs_dim,nu", DIMS)
def test_constant_head_is_the_parametrised_policy_by_bits(obs_dim, nu, hidden, activation):
    """zero weights into the log-std units, finite rows, a bias inside the bounds: r_u = b exactly, and the actions and the
    un-squashed logp are the bits of mzp_net_sample_row with log_std = b behind the network — on the host and in the model"""
    rng = np.random.default_rng(obs_dim + nu)
    obs = rng.uniform(-3.0, 3.0, (33, obs_dim)).astype(np.float32)
    slots = np.arange(33) + 1000
    for rows in (None, 33):
        net = random_net(rng, obs_dim, nu, hidden, rows=rows)
        b = rng.uniform(-1.5, 0.5, net.shape[:-1] + (nu,)).astype(np.float32)
        head, par = constant_head(net, obs_dim, nu, hidden, b), np.concatenate([net, b], axis=-1)
        for squash in (False, True):
            kw = dict(hidden=hidden, activation=activation, squash=squash, action_scale=0.9, noise_seed=9, noise_step=4, slots=slots)
            a, lp = host_head(head, obs, nu, **kw)
            ra, rlp = host_param_sample(par, obs, nu, mode=0, **kw)
            assert np.isfinite(a).all() and np.array_equal(_bits(a), _bits(ra)) and np.array_equal(_bits(lp), _bits(rlp))
            ma, mlp = policy.sample_reference(head, obs, nu, log_std="state", **kw)
            mra, mrlp = policy.sample_reference(par, obs, nu, **kw)
            assert np.array_equal(_bits(ma), _bits(mra)) and np.array_equal(_bits(mlp), _bits(mrlp))
            if squash:  # the squashed log-prob is another number, the actions are not
                a2, lp2 = host_head(head, obs, nu, squashed_logp=True, **kw)
                assert np.array_equal(_bits(a2), _bits(a)) and not np.array_equal(_bits(lp2), _bits(lp))


@pytest.mark.parametrize("hidden,activation", NETS)
def test_clamp_by_bits(hidden, activation):
    """biases +-50 with bounds (-20, 2) give the bits of biases -20 and 2"""
    obs_dim, nu = 30, 8
    rng = np.random.default_rng(2)
    obs = rng.uniform(-3.0, 3.0, (16, obs_dim)).astype(np.float32)
    net = random_net(rng, obs_dim, nu, hidden, rows=16)
    sign = np.where(np.arange(nu) % 2 == 0, 1.0, -1.0).astype(np.float32)
    far, at = constant_head(net, obs_dim, nu, hidden, 50.0 * sign), constant_head(net, obs_dim, nu, hidden, np.where(sign > 0, 2.0, -20.0))
    for squashed in (False, True):
        kw = dict(hidden=hidden, activation=activation, squash=True, action_scale=0.9, squashed_logp=squashed, noise_seed=1, noise_step=2)
        for f in (host_head, model_head):
            (a, lp), (b, lq) = f(far, obs, nu, bounds=BOUNDS, **kw), f(at, obs, nu, bounds=BOUNDS, **kw)
            assert np.isfinite(a).all() and np.isfinite(lp).all()
            assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(lp), _bits(lq))
            # and open sides let the biases through
            _, lr = f(far, obs, nu, bounds=(-np.inf, np.inf), **kw)
            assert not np.array_equal(_bits(lp), _bits(lr))
    lib = _load()
    f32 = np.float32
    assert lib.mzh_host_clamp(f32(-50), f32(-20), f32(2)) == -20 and lib.mzh_host_clamp(f32(50), f32(-20), f32(2)) == 2
    assert lib.mzh_host_clamp(f32(0.25), f32(-20), f32(2)) == 0.25 and np.isnan(lib.mzh_host_clamp(f32(np.nan), f32(-20), f32(2)))
    assert lib.mzh_host_clamp(f32(-np.inf), f32(-np.inf), f32(2)) == -np.inf and lib.mzh_host_clamp(f32(1e30), f32(-20), f32(np.inf)) == f32(1e30)


@pytest.mark.parametrize("hidden,activation", NETS)
@pytest.mark.parametrize("obs_dim,nu", DIMS)
def test_deterministic_limit_by_bits(obs_dim, nu, hidden, activation):
    """bounds (-inf, 2) with a bias of -inf: s = 0, z = m + (+-0), and the actions are the bits of the deterministic actor on
    mean_actor(params), wherever the mean is not -0"""
    rng = np.random.default_rng(3 * obs_dim + nu)
    obs = rng.uniform(-3.0, 3.0, (33, obs_dim)).astype(np.float32)
    for rows in (None, 33):
        net = random_net(rng, obs_dim, nu, hidden, rows=rows)
        head = constant_head(net, obs_dim, nu, hidden, -np.inf)
        assert np.array_equal(policy.mean_actor(head, obs_dim, nu, hidden), net)
        for squash in (False, True):
            kw = dict(hidden=hidden, activation=activation, squash=squash, action_scale=0.9)
            a, lp = host_head(head, obs, nu, bounds=(-np.inf, 2.0), noise_seed=5, noise_step=6, **kw)
            want = host_policy(net, obs, nu, **kw)
            assert not np.any((want == 0) & np.signbit(want))
            assert np.array_equal(_bits(a), _bits(want)) and np.all(np.isposinf(lp))
            ma, mlp = policy.sample_reference(head, obs, nu, log_std="state", log_std_bounds=(-np.inf, 2.0), noise_seed=5, noise_step=6, **kw)
            assert np.array_equal(_bits(ma), _bits(policy.reference(net, obs, nu, **kw))) and np.all(np.isposinf(mlp))
            if not squash and (activation == "relu" or hidden == 0):  # numpy reproduces these networks bit for bit
                assert np.array_equal(_bits(a), _bits(ma))


def test_nan_log_std_unit_reaches_its_action_and_its_rows_logp_only():
    rng = np.random.default_rng(3)
    obs_dim, nu, hidden = 11, 3, (5, 3)
    obs = rng.uniform(-3.0, 3.0, (9, obs_dim)).astype(np.float32)
    par = random_head(rng, obs_dim, nu, hidden, rows=9)
    for squashed in (False, True):
        kw = dict(hidden=hidden, activation="relu", squash=True, action_scale=2.0, squashed_logp=squashed, noise_seed=5, noise_step=6)
        got, glp = host_head(par, obs, nu, **kw)
        bad = par.copy()
        bad[4, -2] = np.nan  # the bias of the raw log-std of unit 1 of row 4
        for act, lp in (host_head(bad, obs, nu, **kw), model_head(bad, obs, nu, **kw)):
            assert np.isnan(act[4, 1]) and np.isnan(lp[4]) and np.isfinite(act[4, [0, 2]]).all()
            assert np.isfinite(np.delete(act, 4, axis=0)).all() and np.isfinite(np.delete(lp, 4)).all()
        act, lp = host_head(bad, obs, nu, **kw)
        keep = np.arange(9) != 4
        assert np.array_equal(_bits(act[keep]), _bits(got[keep])) and np.array_equal(_bits(lp[keep]), _bits(glp[keep]))
        assert np.array_equal(_bits(act[4, [0, 2]]), _bits(got[4, [0, 2]]))


# ---------------------------------------------------------------------------------------------- against float64
C0, LN2 = float(np.float32(0.9189385)), float(np.float32(0.6931472))


def correction64(z, logA):
    """c(z) = 2 ((LN2 - z) - softplus(-2 z)) + logA in float64, the fp32 constants as the device holds them"""
    x = -2.0 * z
    return 2.0 * ((LN2 - z) - (np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))))) + logA


def f64_head_and_bounds(par, obs, nu, hidden, activation, squash, A, bounds, squashed, eps):
    """float64 evaluation of the head actor on the model's eps, and the bounds of the module docstring:
    (actions, e_a, logp, e_logp, z)"""
    out, e = f64_and_bound_net(par, obs, 2 * nu, hidden, activation, False, 1.0)
    m, r, e_m, e_ls = out[:, :nu], out[:, nu:], e[:, :nu], e[:, nu:]
    lo, hi = (float(np.float32(b)) for b in bounds)
    ls = np.where(r < lo, lo, np.where(r > hi, hi, r))
    s = np.exp(ls)
    z = m + s * eps
    e_z = e_m + s * 1e-5 + np.abs(s * eps) * (4 * EPS + np.expm1(e_ls)) + np.abs(z) * EPS
    Af = float(np.float32(A))
    act, e_a = (Af * np.tanh(z), Af * (e_z + 4 * EPS)) if squash else (z, e_z)
    logA = float(np.float32(np.log(np.float64(np.float32(A)))))
    acc, e_acc = np.zeros(len(z)), np.zeros(len(z))
    for u in range(nu):
        q = eps[:, u] ** 2
        h = -0.5 * q
        t1 = h - ls[:, u]
        t = t1 - C0
        e_t = 0.5 * ((2 * np.abs(eps[:, u]) + 1e-5) * 1e-5 + q * EPS) + e_ls[:, u] + np.abs(t1) * EPS + np.abs(t) * EPS
        if squashed:
            c = correction64(z[:, u], logA)
            e_t = e_t + 2 * e_z[:, u] + 4 * CORRECTION_MEASURED + np.abs(t - c) * EPS
            t = t - c
        acc = acc + t
        e_acc = e_acc + e_t + np.abs(acc) * EPS
    return act, e_a, acc, e_acc, z


MEASURED = {}


@pytest.mark.parametrize("hidden,activation", NETS)
@pytest.mark.parametrize("obs_dim,nu", DIMS)
def test_against_float64(obs_dim, nu, hidden, activation):
    """actions, un-squashed and squashed logp of the host build and of the numpy model inside the derived bounds, with the
    correction term's own evaluation error at four times what was measured (module docstring)"""
    assert np.frexp(SCALE)[0] == 0.5  # a power of two: A * tanh is an exact product
    rng = np.random.default_rng(17 + obs_dim)
    obs = rng.uniform(-3.0, 3.0, (64, obs_dim)).astype(np.float32)
    slots = np.arange(64) + 5
    eps = policy.noise(3, 11, slots, nu).astype(np.float64)
    lib = _load()
    for rows in (None, 64):
        par = random_head(rng, obs_dim, nu, hidden, rows=rows)
        # spread the raw log-stds over the clamp's inside and both sides: the biases of the log-std units
        par[..., -nu:] += rng.uniform(-3.0, 3.0, par.shape[:-1] + (nu,)).astype(np.float32)
        for squash, squashed in ((False, False), (True, False), (True, True)):
            for bounds in (BOUNDS, (-1.0, 0.5)):
                val, e_a, lp64, e_lp, z = f64_head_and_bounds(par, obs, nu, hidden, activation, squash, SCALE, bounds, squashed, eps)
                kw = dict(hidden=hidden, activation=activation, squash=squash, action_scale=SCALE, squashed_logp=squashed, noise_seed=3, noise_step=11,
                          slots=slots)
                for name, (act, logp) in (("host build", host_head(par, obs, nu, bounds=bounds, **kw)),
                                          ("policy.sample_reference", model_head(par, obs, nu, bounds=bounds, **kw))):
                    ea, el = np.abs(act.astype(np.float64) - val), np.abs(logp.astype(np.float64) - lp64)
                    print(f"{name}: hidden {hidden} {activation} nu {nu} squash {squash} squashed_logp {squashed} bounds {bounds}: "
                          f"action err / bound {(ea / e_a).max():.3f}, logp err {el.max():.3e}, err / bound {(el / e_lp).max():.3f}")
                    assert act.dtype == np.float32 and logp.dtype == np.float32
                    assert np.all(ea <= e_a), name
                    assert np.all(el <= e_lp), name
                if squashed:  # what CORRECTION_MEASURED records: the corrected term's own evaluation, on this case's z
                    logA = np.float32(np.log(np.float64(np.float32(SCALE))))
                    z32 = z.astype(np.float32).ravel()
                    got = np.array([lib.mzh_host_logp_term(0.0, 0.0, float(v), 1, float(logA)) for v in z32], np.float64)
                    # eps = ls = 0: t = -C0 exactly before the correction, so the term is fl(-C0 - c32(z))
                    err = np.abs(got - (-C0 - correction64(z32.astype(np.float64), float(logA)))).max()
                    MEASURED[(obs_dim, nu, hidden, activation, rows, bounds)] = err
                    print(f"correction term, host build against float64 on {z32.size} z in [{z32.min():.2f}, {z32.max():.2f}]: max err {err:.3e}")
                    assert err <= 4 * CORRECTION_MEASURED


def test_the_stable_correction_stays_finite_where_the_naive_one_does_not():
    """log(1 - tanh^2) is -inf in fp32 from |z| ~ 9; the form the device evaluates follows float64 to 2.9e-6 up to |z| = 88"""
    lib = _load()
    f32 = np.float32
    z = np.concatenate([np.linspace(-88, 88, 1409), [9.5, -9.5, 20.0, -20.0]]).astype(np.float32)
    with np.errstate(divide="ignore"):
        naive = np.log((f32(1.0) - np.tanh(z) ** 2).astype(np.float32))
    assert np.isneginf(naive[np.abs(z) > 10]).all()
    got = np.array([-(lib.mzh_host_logp_term(0.0, 0.0, float(v), 1, 0.0) + f32(0.9189385)) for v in z], np.float64)
    want = correction64(z.astype(np.float64), 0.0)
    assert np.isfinite(got).all()
    # 2.9e-6 (the form itself in fp32, csrc/mz_policy.h) + one rounding of |t| <= 352 for undoing the constant here
    assert np.abs(got - want).max() <= 2.9e-6 + 352 * EPS
    assert np.isnan(lib.mzh_host_logp_term(0.0, 0.0, float("nan"), 1, 0.0))
    # logA is 0 exactly for A = 1 and enters as one sum
    a = lib.mzh_host_logp_term(0.3, -0.5, 0.7, 1, 0.0)
    b = lib.mzh_host_logp_term(0.3, -0.5, 0.7, 1, float(np.log(np.float32(0.9))))
    assert abs((a - b) - float(np.log(np.float32(0.9)))) < 4 * EPS
