"""Parameters of the device-side policies (VecMazeEnv.policy_act / rollout_policy, mz_policy_act / mz_rollout_policy) and their
numpy model.

One policy is a flat float32 vector, weights input-major (`nn.Linear.weight.T`):

    hidden == 0 (affine)      Wt [obs_dim, nu], b [nu]                                  obs_dim * nu + nu numbers
    1 <= hidden <= 64         W1t [obs_dim, H], b1 [H], W2t [H, nu], b2 [nu]            obs_dim * H + H + H * nu + nu numbers

`pack` / `pack_linear` build it from weights in nn.Linear orientation (torch or numpy); `reference` is the arithmetic of
csrc/mz_policy.h in numpy float32, operation by operation: every unit starts from its bias and adds w * x over the inputs in index
order, the product and the sum rounded separately; hidden units are tanh of that, an output is the sum or
float32(action_scale) * tanh(sum).  For the affine, unsquashed case it equals the device's result bit for bit; with a tanh it
differs by what numpy's float32 tanh and the device's tanhf differ.

Stochastic policies (VecMazeEnv.policy_sample / rollout_policy_sample, mz_policy_sample / mz_rollout_policy_sample) are a diagonal
Gaussian around the same network: the vector carries `log_std [nu]` behind it (`param_count(..., stochastic=True)`, the `log_std=`
argument of `pack` / `pack_linear`).  `noise` is the device's eps(noise_seed, noise_step, slot, u) — a pure function of four integers,
slot being the global env slot —, `sample_reference` the draw and its log-probability:

    key = mix64(noise_seed ^ (0xA24BAED4963EE407 * (noise_step + 1)))                    uint64, wrap-around
    x1, x2 = rng_u32(key, slot, 2u), rng_u32(key, slot, 2u + 1)
    u1 = ((x1 >> 8) + 1) * 2^-24, u2 = (x2 >> 8) * 2^-24, eps = sqrt(-2 log(u1)) * cos(float32(6.2831855) * u2)
    z_u = m_u + exp(log_std_u) * eps_u           (m_u: the pre-squash sum; product and sum rounded separately, float32)
    action_u = z_u, or float32(action_scale) * tanh(z_u) with squash
    logp = sum_u (-0.5 * eps_u^2 - log_std_u - 0.9189385), u in order, float32, every operation rounded separately

logp is the density of z; with squash it is the PRE-tanh density, and the caller applies the tanh correction from the actions.
The integer part is exact; the float part runs float64 libm on the float32 u1, u2 and the float32 angle and rounds the factors to
float32, so it differs from the device by libm ulps only.

Critics (VecMazeEnv.value, the `value_params=` of the rollouts; mz_value / mz_rollout_actor_critic) are policies with nu = 1, never
squashed, in a vector of their own (`param_count(obs_dim, 1, hidden)`, packed by `pack` / `pack_linear`): `value_reference` is the
pre-squash sum of the one output unit, bit-equal to the device for hidden == 0.  `gae_reference` is the backward scan of
VecMazeEnv.gae / mz_gae (csrc/mz_gae.h) in float32, operation by operation: bit-equal to the device.

Deeper networks (mz_net_act / mz_net_value / mz_rollout_net): wherever a function here takes `hidden` it is an int as above or a
sequence of one or two widths, and `activation` is "tanh" or "relu", one choice for both hidden layers.  Two hidden layers pack as

    W1t [obs_dim, H1], b1 [H1], W2t [H1, H2], b2 [H2], W3t [H2, nout], b3 [nout]         (`pack_mlp`)

then log_std [nu] for a stochastic actor.  ReLU is `0 if acc < 0 else acc`: no rounding, -0.0 stays -0.0, NaN propagates — so a
ReLU network without squash equals the device bit for bit at any depth.

Normalised observations (VecMazeEnv.bind_obs_norm, mz_bind_obs_norm): while a normaliser is bound the device evaluates its networks
on `normalize_reference(obs, mean, inv_std, clip)` — bit-equal to the device — so the model of a bound call is
`reference(params, normalize_reference(obs, mean, inv_std, clip), ...)`, and likewise for `sample_reference` / `value_reference`.
`return_scan_reference` is the forward scan of VecMazeEnv.return_scan / mz_return_scan (csrc/mz_returns.h), bit-equal too.

State-dependent log-std heads (`log_std="state"`; mz_net_sample_head / mz_rollout_head; SAC): the output layer has 2 nu units — the
means, then the raw log-stds — and no log_std vector follows (`param_count(..., log_std="state")`, `pack_mlp(..,
log_std_head=(W, b))`).  `sample_reference(..., log_std="state", log_std_bounds=(lo, hi), squashed_logp=)`:

    ls_u = lo if r_u < lo else (hi if r_u > hi else r_u)              two selects: NaN passes
    z_u = m_u + exp(ls_u) * eps_u;  action_u as above;  logp's term t_u as above with ls_u, and with squashed_logp
    x = -2 z_u;  sp = (x if x > 0 else 0) + log1p(exp(-|x|));  c = 2 * ((0.6931472 - z_u) - sp) + logA;  t_u = t_u - c

float32, every operation rounded separately, logA = log(float32(action_scale)) rounded to float32: the density of the squashed
action, finite wherever z is.  `mean_actor` cuts the deterministic actor (the means' columns) out of a head vector.

Wide networks (`VecMazeEnv.set_option("wide_nets", 1)`, option "wide_nets" of include/mazestep.h): hidden layers of up to MAX_WIDTH =
256 units, evaluated by the tiled kernel of csrc/mz_net_tile.h with the same arithmetic, so everything above holds at every width.
`net_shape`, `param_count`, `pack_mlp`, `mean_actor`, `reference`, `sample_reference` and `value_reference` take `max_width=`
(default MAX_HIDDEN = 64, which refuses 65 as ever): pass `max_width=MAX_WIDTH` for such a network.
"""
import numpy as np

MAX_HIDDEN = 64  # MZ_POLICY_MAX_HIDDEN (include/mazestep.h)
MAX_WIDTH = 256  # MZ_NET_MAX_WIDTH: the widest hidden layer of an mz_net network on a handle with option "wide_nets" on
MAX_HIDDEN_LAYERS = 2  # MZ_NET_MAX_HIDDEN_LAYERS
ACTIVATIONS = ("tanh", "relu")  # index: MZ_ACT_TANH, MZ_ACT_RELU


def net_shape(hidden=0, activation: str = "tanh", what: str = "hidden", max_width: int = MAX_HIDDEN):
    """(widths, activation index) of a network: `hidden` an int (0: affine) or a sequence of one or two widths 1 .. max_width,
    `activation` "tanh" or "relu".  `what` names the argument in the errors.  max_width: MAX_HIDDEN (64) by default, up to MAX_WIDTH
    (256) for a network of a handle with `set_option("wide_nets", 1)`; every function here that takes it passes it down."""
    max_width = int(max_width)
    if not MAX_HIDDEN <= max_width <= MAX_WIDTH:
        raise ValueError(f"max_width must be {MAX_HIDDEN} .. {MAX_WIDTH}, got {max_width}")
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be 'tanh' or 'relu', got {activation!r}")
    if np.ndim(hidden) == 0:
        h = int(hidden)
        if not 0 <= h <= max_width:
            raise ValueError(f"{what} must be 0 .. {max_width}, got {h}" + _WIDE_HINT * (max_width < MAX_WIDTH and h <= MAX_WIDTH))
        return ((h,) if h else ()), ACTIVATIONS.index(activation)
    widths = tuple(int(w) for w in hidden)
    if not 1 <= len(widths) <= MAX_HIDDEN_LAYERS:
        raise ValueError(f"{what} must be an int or a sequence of one or two widths, got {len(widths)} hidden layers")
    if any(not 1 <= w <= max_width for w in widths):
        raise ValueError(f"{what}: a hidden layer has 1 .. {max_width} units, got {widths}"
                         + _WIDE_HINT * (max_width < MAX_WIDTH and all(1 <= w <= MAX_WIDTH for w in widths)))
    return widths, ACTIVATIONS.index(activation)


# what a refusal of a width 65 .. 256 adds
_WIDE_HINT = f" (up to {MAX_WIDTH} on an env with set_option('wide_nets', 1), and with max_width={MAX_WIDTH} here)"


LOG_STD_KINDS = ("param", "state")


def _log_std_kind(log_std: str) -> bool:
    """True for a state-dependent head."""
    if log_std not in LOG_STD_KINDS:
        raise ValueError(f"log_std must be 'param' or 'state', got {log_std!r}")
    return log_std == "state"


def param_count(obs_dim: int, nu: int, hidden=0, stochastic: bool = False, log_std: str = "param", max_width: int = MAX_HIDDEN) -> int:
    """Floats of one policy; with `stochastic` the network's count plus log_std [nu].  hidden: an int or a sequence of one or two
    widths.  log_std="state": a head actor — an output layer of 2 nu units and nothing behind it (`stochastic` is not read)."""
    obs_dim, nu = int(obs_dim), int(nu)
    if _log_std_kind(log_std):
        nu, stochastic = 2 * nu, False
    sizes = (obs_dim,) + net_shape(hidden, max_width=max_width)[0] + (nu,)
    return sum(a * b + b for a, b in zip(sizes[:-1], sizes[1:])) + (nu if stochastic else 0)


def _np(x):
    if hasattr(x, "detach"):  # a torch tensor
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float32)


def _with_log_std(parts, nu, log_std):
    if log_std is None:
        return np.concatenate(parts)
    ls = _np(log_std)
    if ls.shape != (nu,):
        raise ValueError(f"log_std must be [nu] = {(nu,)}, got {ls.shape}")
    return np.concatenate(parts + [ls])


def pack_linear(W, b, log_std=None):
    """Affine policy a = W @ obs + b: W [nu, obs_dim], b [nu] (nn.Linear's weight and bias) -> float32 [obs_dim * nu + nu]; with
    `log_std` [nu] the stochastic policy's vector, nu numbers longer."""
    W, b = _np(W), _np(b)
    if W.ndim != 2 or b.shape != (W.shape[0],):
        raise ValueError(f"W must be [nu, obs_dim] and b [nu], got {W.shape} and {b.shape}")
    return _with_log_std([W.T.ravel(), b], W.shape[0], log_std)


def pack(W1, b1, W2, b2, log_std=None):
    """One tanh hidden layer, a = W2 @ tanh(W1 @ obs + b1) + b2: W1 [H, obs_dim], b1 [H], W2 [nu, H], b2 [nu] -> float32 [npar];
    with `log_std` [nu] the stochastic policy's vector, nu numbers longer."""
    W1, b1, W2, b2 = _np(W1), _np(b1), _np(W2), _np(b2)
    if W1.ndim != 2 or W2.ndim != 2 or b1.shape != (W1.shape[0],) or W2.shape[1] != W1.shape[0] or b2.shape != (W2.shape[0],):
        raise ValueError(f"want W1 [H, obs_dim], b1 [H], W2 [nu, H], b2 [nu], got {W1.shape}, {b1.shape}, {W2.shape}, {b2.shape}")
    if not 1 <= W1.shape[0] <= MAX_HIDDEN:
        raise ValueError(f"the hidden layer has 1 .. {MAX_HIDDEN} units, got {W1.shape[0]}")
    return _with_log_std([W1.T.ravel(), b1, W2.T.ravel(), b2], W2.shape[0], log_std)


def pack_mlp(layers, log_std=None, log_std_head=None, max_width: int = MAX_HIDDEN):
    """A network of 0, 1 or 2 hidden layers from 1 .. 3 `(W, b)` pairs in nn.Linear orientation, first layer first: W [out, in],
    b [out] -> float32 [count], every layer as W.T then b; with `log_std` [nu] the stochastic policy's vector, nu numbers longer.
    One pair is `pack_linear`, two pairs are `pack`.  `log_std_head=(W [nu, nin], b [nu])`: the second nn.Linear of a SAC actor, whose
    rows are appended to the last layer's — the head actor's output layer of 2 nu units (not together with `log_std`)."""
    pairs = [(_np(W), _np(b)) for W, b in layers]
    if log_std_head is not None:
        if log_std is not None:
            raise ValueError("log_std and log_std_head exclude each other: a head actor has no log_std vector")
        if not pairs:
            raise ValueError(f"layers must hold 1 .. {MAX_HIDDEN_LAYERS + 1} (W, b) pairs, got 0")
        Wh, bh = _np(log_std_head[0]), _np(log_std_head[1])
        Wm, bm = pairs[-1]
        if Wh.shape != Wm.shape or bh.shape != bm.shape:
            raise ValueError(f"log_std_head: want W {Wm.shape} and b {bm.shape} like the last layer's, got {Wh.shape} and {bh.shape}")
        pairs[-1] = (np.concatenate([Wm, Wh], axis=0), np.concatenate([bm, bh]))
    if not 1 <= len(pairs) <= MAX_HIDDEN_LAYERS + 1:
        raise ValueError(f"layers must hold 1 .. {MAX_HIDDEN_LAYERS + 1} (W, b) pairs, got {len(pairs)}")
    for k, (W, b) in enumerate(pairs):
        if W.ndim != 2 or b.shape != (W.shape[0],) or (k and W.shape[1] != pairs[k - 1][0].shape[0]):
            raise ValueError(f"layers[{k}]: want W [out, in] and b [out] with in = the width of the layer before, got {W.shape} and {b.shape}")
        if k < len(pairs) - 1 and not 1 <= W.shape[0] <= int(max_width):
            raise ValueError(f"layers[{k}]: a hidden layer has 1 .. {int(max_width)} units, got {W.shape[0]}"
                             + _WIDE_HINT * (int(max_width) < MAX_WIDTH and 1 <= W.shape[0] <= MAX_WIDTH))
    net_shape(0, max_width=max_width)  # (refuses a max_width outside MAX_HIDDEN .. MAX_WIDTH)
    return _with_log_std([a for W, b in pairs for a in (W.T.ravel(), b)], pairs[-1][0].shape[0], log_std)


def _layer(x, Wt, b):
    """b + sum_i Wt[.., i, :] * x[.., i] in index order, float32, two roundings per term.  x [R, n]; Wt [n, m] or [R, n, m]; b [m] or [R, m]."""
    acc = np.broadcast_to(b, (x.shape[0], Wt.shape[-1])).astype(np.float32)
    for i in range(x.shape[1]):
        p = (Wt[..., i, :] * x[:, i: i + 1]).astype(np.float32)
        acc = (acc + p).astype(np.float32)
    return acc


def _pre_squash(x, p, nu, shape):
    """The output units' sums before the squash: x [R, obs_dim], p [npar] or [R, npar], shape = net_shape(..) -> float32 [R, nu]."""
    widths, act = shape
    lead, off, h = p.shape[:-1], 0, x
    for k, m in enumerate(widths + (nu,)):
        n = h.shape[1]
        acc = _layer(h, p[..., off: off + n * m].reshape(lead + (n, m)), p[..., off + n * m: off + n * m + m])
        off += n * m + m
        if k == len(widths):
            return acc
        # hidden units: tanh, or the select of mzp_activate (no rounding, -0.0 and NaN pass)
        h = np.where(acc < 0, np.float32(0.0), acc).astype(np.float32) if act else np.tanh(acc).astype(np.float32)


def mean_actor(params, obs_dim: int, nu: int, hidden=0, max_width: int = MAX_HIDDEN):
    """The deterministic actor inside a head vector: params [count_h] or [R, count_h] with count_h = param_count(obs_dim, nu, hidden,
    log_std="state") -> float32 [count] or [R, count], count = param_count(obs_dim, nu, hidden): every hidden layer as it is, the
    means' columns of the output layer and their biases.  What `rollout_policy` evaluates a trained SAC actor with."""
    p = np.asarray(_np(params))
    obs_dim, nu = int(obs_dim), int(nu)
    ch, widths = param_count(obs_dim, nu, hidden, log_std="state", max_width=max_width), net_shape(hidden, max_width=max_width)[0]
    if p.shape[-1:] != (ch,) or p.ndim not in (1, 2):
        raise ValueError(f"params must have shape {(ch,)} or [R, {ch}], got {p.shape}")
    nin = widths[-1] if widths else obs_dim
    body = ch - (nin * 2 * nu + 2 * nu)
    lead = p.shape[:-1]
    W = p[..., body: body + nin * 2 * nu].reshape(lead + (nin, 2 * nu))[..., :nu].reshape(lead + (nin * nu,))
    b = p[..., body + nin * 2 * nu: body + nin * 2 * nu + nu]
    return np.ascontiguousarray(np.concatenate([p[..., :body], W, b], axis=-1), dtype=np.float32)


def _squashed(acc, squash, action_scale):
    return (np.float32(action_scale) * np.tanh(acc).astype(np.float32)).astype(np.float32) if squash else acc


def reference(params, obs, nu: int, hidden=0, squash: bool = False, action_scale: float = 1.0, activation: str = "tanh",
              max_width: int = MAX_HIDDEN):
    """The policy of csrc/mz_policy.h on rows of observations: obs [R, obs_dim] (or [obs_dim]); params [npar] shared by the rows or
    [R, npar], one policy per row; hidden / activation as in `net_shape`.  Returns float32 [R, nu] (or [nu])."""
    x = np.asarray(obs, dtype=np.float32)
    single = x.ndim == 1
    x = np.atleast_2d(x)
    p = np.asarray(params, dtype=np.float32)
    R, od, nu, shape = x.shape[0], x.shape[1], int(nu), net_shape(hidden, activation, max_width=max_width)
    npar = param_count(od, nu, hidden, max_width=max_width)
    if p.shape not in ((npar,), (R, npar)):
        raise ValueError(f"params must have shape {(npar,)} or {(R, npar)}, got {p.shape}")
    out = _squashed(_pre_squash(x, p, nu, shape), squash, action_scale)
    return out[0] if single else out


_M64 = (1 << 64) - 1
_GOLDEN, _STEP_MUL = np.uint64(0x9E3779B97F4A7C15), 0xA24BAED4963EE407


def _mix64(z):
    """csrc/mz_rng.h mix64 on a uint64 array (numpy's uint64 arithmetic wraps around)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise_key(noise_seed: int, noise_step: int) -> int:
    """The key of one step's noise (csrc/mz_policy.h mzp_noise_key), a Python int in [0, 2^64)."""
    k = (int(noise_seed) & _M64) ^ ((_STEP_MUL * ((int(noise_step) + 1) & _M64)) & _M64)
    with np.errstate(over="ignore"):
        return int(_mix64(np.array([k], dtype=np.uint64))[0])


def noise_words(noise_seed: int, noise_step: int, slots, nu: int):
    """The integer stream behind `noise`: uint32 [len(slots), nu, 2], words rng_u32(key, slot, 2u) and rng_u32(key, slot, 2u + 1)."""
    key = np.uint64(noise_key(noise_seed, noise_step))
    sl = np.array([int(s) & _M64 for s in np.atleast_1d(np.asarray(slots, dtype=object)).ravel()], dtype=np.uint64)
    c = np.arange(2 * int(nu), dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = _mix64(key + _GOLDEN * (sl + np.uint64(1)))
        z = _mix64(z[:, None] + _GOLDEN * (c[None, :] + np.uint64(1)))
    return (z >> np.uint64(32)).astype(np.uint32).reshape(len(sl), int(nu), 2)


def noise(noise_seed: int, noise_step: int, slots, nu: int):
    """eps(noise_seed, noise_step, slot, u) of csrc/mz_policy.h for the global env slots `slots` and u = 0 .. nu - 1: float32
    [len(slots), nu].  A value depends on its four integers only."""
    w = noise_words(noise_seed, noise_step, slots, nu)
    u1 = (((w[..., 0] >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)).astype(np.float32)
    u2 = ((w[..., 1] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)
    t = (np.float32(-2.0) * np.log(u1.astype(np.float64)).astype(np.float32)).astype(np.float32)
    r = np.sqrt(t.astype(np.float64)).astype(np.float32)
    ang = (np.float32(6.2831855) * u2).astype(np.float32)
    c = np.cos(ang.astype(np.float64)).astype(np.float32)
    return (r * c).astype(np.float32)


_eps = noise  # (sample_reference has an argument of that name)


def sample_reference(params, obs, nu: int, hidden=0, squash: bool = False, action_scale: float = 1.0, noise_seed: int = 0,
                     noise_step: int = 0, slots=None, activation: str = "tanh", noise: str = "pre_squash", log_std: str = "param",
                     log_std_bounds=(-20.0, 2.0), squashed_logp: bool = False, max_width: int = MAX_HIDDEN):
    """The stochastic policy of csrc/mz_policy.h on rows of observations: obs [R, obs_dim] (or [obs_dim]); params [npar_s] shared by
    the rows or [R, npar_s]; slots: the rows' global env slots, default 0 .. R - 1.  Returns (actions float32 [R, nu], logp float32
    [R]) — or ([nu], scalar) for a single row.

    noise="pre_squash" (MZ_NOISE_PRE_SQUASH): z = m + s * eps, a = action_scale * tanh(z) with `squash`.  noise="action"
    (MZ_NOISE_ACTION, TD3 / DDPG exploration): b = action_scale * tanh(m) with `squash` else m, z = b + s * eps, and with `squash`
    a = z clipped to +-action_scale by two selects (NaN passes).  eps and logp are the same in both modes.

    log_std="state" (mz_net_sample_head): params [count_h] or [R, count_h], count_h = param_count(.., log_std="state"); the raw
    log-stds are output units nu .. 2 nu - 1, clamped to log_std_bounds by two selects; squashed_logp: logp is the density of the
    squashed action (needs `squash`; the head of this module).  Needs noise="pre_squash"."""
    if noise not in ("pre_squash", "action"):
        raise ValueError(f"noise must be 'pre_squash' or 'action', got {noise!r}")
    if _log_std_kind(log_std):
        return _sample_head_reference(params, obs, nu, hidden, squash, action_scale, noise_seed, noise_step, slots, activation, noise,
                                      log_std_bounds, squashed_logp, max_width)
    if squashed_logp:
        raise ValueError("squashed_logp needs log_std='state'")
    x = np.asarray(obs, dtype=np.float32)
    single = x.ndim == 1
    x = np.atleast_2d(x)
    p = np.asarray(params, dtype=np.float32)
    R, od, nu, shape = x.shape[0], x.shape[1], int(nu), net_shape(hidden, activation, max_width=max_width)
    npar = param_count(od, nu, hidden, max_width=max_width)
    if p.shape not in ((npar + nu,), (R, npar + nu)):
        raise ValueError(f"params must have shape {(npar + nu,)} or {(R, npar + nu)} (the network, then log_std [nu]), got {p.shape}")
    sl = np.arange(R) if slots is None else np.atleast_1d(np.asarray(slots, dtype=object)).ravel()
    if len(sl) != R:
        raise ValueError(f"slots must name one global env slot per row ({R}), got {len(sl)}")
    ls = np.broadcast_to(p[..., npar:], (R, nu))
    m = _pre_squash(x, p[..., :npar], nu, shape)
    eps = _eps(noise_seed, noise_step, sl, nu)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.exp(ls.astype(np.float64)).astype(np.float32)
        if noise == "action" and squash:
            A = np.float32(action_scale)
            z = (_squashed(m, True, action_scale) + (s * eps).astype(np.float32)).astype(np.float32)
            act = np.where(z < -A, -A, np.where(z > A, A, z)).astype(np.float32)
        else:
            z = (m + (s * eps).astype(np.float32)).astype(np.float32)
            act = _squashed(z, squash, action_scale)
        logp = np.zeros(R, dtype=np.float32)
        for u in range(nu):
            q = (eps[:, u] * eps[:, u]).astype(np.float32)
            t = ((np.float32(-0.5) * q).astype(np.float32) - ls[:, u]).astype(np.float32)
            t = (t - np.float32(0.9189385)).astype(np.float32)
            logp = (logp + t).astype(np.float32)
    return (act[0], logp[0]) if single else (act, logp)


def head_bounds(log_std_bounds):
    """(lo, hi) of a head's clamp as float32: -inf / +inf allowed, NaN or lo > hi refused."""
    try:
        lo, hi = (np.float32(v) for v in log_std_bounds)
    except (TypeError, ValueError):
        raise ValueError(f"log_std_bounds must be a pair (lo, hi), got {log_std_bounds!r}") from None
    if np.isnan(lo) or np.isnan(hi) or lo > hi:
        raise ValueError(f"log_std_bounds must be (lo, hi) with lo <= hi and no NaN, got {log_std_bounds!r}")
    return lo, hi


def _sample_head_reference(params, obs, nu, hidden, squash, action_scale, noise_seed, noise_step, slots, activation, noise, log_std_bounds,
                           squashed_logp, max_width=MAX_HIDDEN):
    if noise != "pre_squash":
        raise ValueError("log_std='state' needs noise='pre_squash'")
    if squashed_logp and not squash:
        raise ValueError("squashed_logp needs squash=True: it is the density of action_scale * tanh(z)")
    lo, hi = head_bounds(log_std_bounds)
    x = np.asarray(obs, dtype=np.float32)
    single = x.ndim == 1
    x = np.atleast_2d(x)
    p = np.asarray(params, dtype=np.float32)
    R, od, nu, shape = x.shape[0], x.shape[1], int(nu), net_shape(hidden, activation, max_width=max_width)
    ch = param_count(od, nu, hidden, log_std="state", max_width=max_width)
    if p.shape not in ((ch,), (R, ch)):
        raise ValueError(f"params must have shape {(ch,)} or {(R, ch)} (an output layer of 2 nu units), got {p.shape}")
    sl = np.arange(R) if slots is None else np.atleast_1d(np.asarray(slots, dtype=object)).ravel()
    if len(sl) != R:
        raise ValueError(f"slots must name one global env slot per row ({R}), got {len(sl)}")
    eps = _eps(noise_seed, noise_step, sl, nu)
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        out = _pre_squash(x, p, 2 * nu, shape)
        m, r = out[:, :nu], out[:, nu:]
        ls = np.where(r < lo, lo, np.where(r > hi, hi, r)).astype(f)
        s = np.exp(ls.astype(np.float64)).astype(f)
        z = (m + (s * eps).astype(f)).astype(f)
        act = _squashed(z, squash, action_scale)
        logA = np.log(np.float64(f(action_scale))).astype(f)
        logp = np.zeros(R, dtype=f)
        for u in range(nu):
            q = (eps[:, u] * eps[:, u]).astype(f)
            t = ((f(-0.5) * q).astype(f) - ls[:, u]).astype(f)
            t = (t - f(0.9189385)).astype(f)
            if squashed_logp:
                zu = z[:, u]
                xx = (f(-2.0) * zu).astype(f)
                e = np.exp(-np.abs(xx).astype(np.float64)).astype(f)
                l = np.log1p(e.astype(np.float64)).astype(f)
                sp = (np.where(xx > 0, xx, f(0.0)).astype(f) + l).astype(f)
                c = (f(0.6931472) - zu).astype(f)
                c = (c - sp).astype(f)
                c = (f(2.0) * c).astype(f)
                c = (c + logA).astype(f)
                t = (t - c).astype(f)
            logp = (logp + t).astype(f)
    return (act[0], logp[0]) if single else (act, logp)


def value_reference(value_params, obs, hidden=0, activation: str = "tanh", max_width: int = MAX_HIDDEN):
    """The critic of csrc/mz_policy.h (mzp_value_row) on rows of observations: a policy with nu = 1, never squashed, whose value is
    the pre-squash sum of its one output unit.  obs [R, obs_dim] (or [obs_dim]); value_params [nvpar] shared by the rows or
    [R, nvpar], nvpar = param_count(obs_dim, 1, hidden).  Returns float32 [R] (or a scalar); bit-equal to the device for hidden == 0."""
    x = np.asarray(obs, dtype=np.float32)
    single = x.ndim == 1
    x = np.atleast_2d(x)
    p = np.asarray(value_params, dtype=np.float32)
    R, od, shape = x.shape[0], x.shape[1], net_shape(hidden, activation, max_width=max_width)
    npar = param_count(od, 1, hidden, max_width=max_width)
    if p.shape not in ((npar,), (R, npar)):
        raise ValueError(f"value_params must have shape {(npar,)} or {(R, npar)}, got {p.shape}")
    with np.errstate(over="ignore", invalid="ignore"):
        v = _pre_squash(x, p, 1, shape)[:, 0]
    return v[0] if single else v


def gae_reference(rewards, dones, values, next_values, gamma: float = 0.99, lam: float = 0.95):
    """The backward scan of csrc/mz_gae.h (mz_gae) on [K, N] rows, float32, every operation rounded separately, k from K - 1 down to
    0 with carry = 0:

        g = float32(gamma); gl = g * float32(lam)
        b     = 0 if done & 1 else g * next_value        (true termination: no bootstrap; a time limit alone bootstraps)
        delta = (reward + b) - value
        c     = 0 if done else gl * carry                (any episode end cuts the recursion)
        adv   = delta + c; carry = adv; ret = adv + value

    Selects, not products with a mask: NaN behind a true termination does not leak.  Returns (advantages, returns), float32 [K, N]."""
    r, v, nv = (np.asarray(a, dtype=np.float32) for a in (rewards, values, next_values))
    d = np.asarray(dones, dtype=np.uint8)
    if r.ndim != 2 or not (r.shape == d.shape == v.shape == nv.shape):
        raise ValueError(f"rewards, dones, values and next_values must share one [K, N] shape, got {r.shape}, {d.shape}, {v.shape}, {nv.shape}")
    g = np.float32(gamma)
    gl = np.float32(g * np.float32(lam))
    adv, ret = np.empty_like(r), np.empty_like(r)
    carry = np.zeros(r.shape[1], dtype=np.float32)
    zero = np.float32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(r.shape[0] - 1, -1, -1):
            b = np.where((d[k] & 1) != 0, zero, (g * nv[k]).astype(np.float32)).astype(np.float32)
            delta = ((r[k] + b).astype(np.float32) - v[k]).astype(np.float32)
            c = np.where(d[k] != 0, zero, (gl * carry).astype(np.float32)).astype(np.float32)
            carry = (delta + c).astype(np.float32)
            adv[k] = carry
            ret[k] = (carry + v[k]).astype(np.float32)
    return adv, ret


def normalize_reference(obs, mean, inv_std, clip: float = 10.0):
    """The normalised rows of csrc/mz_policy.h (mzp_norm_elem) in float32, operation by operation, every operation rounded separately:

        d = x - mean;  y = d * inv_std;  y = -c if y < -c else (c if y > c else y)        c = float32(clip)

    A product with inv_std, not a quotient; two selects, not minimum / maximum: NaN passes through, clip = inf switches the clip off,
    x = +-inf becomes +-c, a constant column (d == 0) becomes 0 for any finite inv_std.  obs [..., obs_dim]; mean, inv_std
    [obs_dim].  Returns float32 of obs's shape; bit-equal to the device."""
    x = _np(obs)
    m, s = _np(mean), _np(inv_std)
    if m.ndim != 1 or m.shape != s.shape or x.shape[-1:] != m.shape:
        raise ValueError(f"mean and inv_std must be [obs_dim] = {x.shape[-1:]}, got {m.shape} and {s.shape}")
    c = np.float32(clip)
    if not c > 0:
        raise ValueError(f"clip must be > 0, got {clip}")
    with np.errstate(over="ignore", invalid="ignore"):
        d = (x - m).astype(np.float32)
        y = (d * s).astype(np.float32)
        y = np.where(y < -c, -c, np.where(y > c, c, y)).astype(np.float32)
    return y


MAX_CONTEXT = 32  # MZ_MAX_CONTEXT (include/mazestep.h)


def context_row(obs, context, mean=None, inv_std=None, clip: float = 10.0):
    """The input row r = [y | c] of a network with a context (csrc/mz_policy.h mzp_input_row): y = `normalize_reference(obs, ...)`
    with a normaliser (mean given), else obs; c = context as it is, never normalised.  obs [..., obs_dim], context [..., C] with
    1 <= C <= MAX_CONTEXT.  The model of a device call with `context=` is `reference(params, context_row(obs, ctx, ...), ...)` (and
    `sample_reference`, `value_reference` likewise) with params packed for obs_dim + C inputs."""
    x, c = _np(obs), _np(context)
    if c.shape[:-1] != x.shape[:-1] or not 1 <= c.shape[-1] <= MAX_CONTEXT:
        raise ValueError(f"context must be {x.shape[:-1]} + (C,) with 1 <= C <= {MAX_CONTEXT}, got {c.shape}")
    y = normalize_reference(x, mean, inv_std, clip) if mean is not None else x
    return np.concatenate([y, c], axis=-1).astype(np.float32)


def context_transition_reference(context, obs, next_obs, dones, dims: int):
    """HIRO's goal transition h(s, g, s') = s + g - s' of `context_update="relative"` (csrc/mz_policy.h mzp_ctx_next) in float32, a
    sum then a difference, two roundings:  tmp = c[d] + s[d];  c[d] = tmp - s'[d]  for d < dims, where dones == 0; rows with
    dones != 0 and entries d >= dims hold.  context [N, C]; obs, next_obs [N, obs_dim] the RAW rows before and behind the step (the
    "next_observations" row, never normalised); dones [N].  Returns a new float32 [N, C]; bit-equal to the device."""
    c, s, s2 = _np(context).copy(), _np(obs), _np(next_obs)
    d = int(dims)
    if c.ndim != 2 or not 1 <= d <= min(c.shape[1], s.shape[-1]):
        raise ValueError(f"dims must be 1 .. min(C, obs_dim) = {min(c.shape[-1], s.shape[-1])} for a context [N, C], got {d}")
    go = np.asarray(dones).reshape(-1) == 0
    with np.errstate(over="ignore", invalid="ignore"):
        tmp = (c[:, :d] + s[:, :d]).astype(np.float32)
        new = (tmp - s2[:, :d]).astype(np.float32)
    c[:, :d] = np.where(go[:, None], new, c[:, :d])
    return c


def return_scan_reference(rewards, dones, gamma: float = 1.0, carry=None, length_carry=None):
    """The forward scan of csrc/mz_returns.h (mz_return_scan) on [K, N] rows, float32, every operation rounded separately, k from 0 up:

        g = float32(gamma)
        p = g * carry; s = p + reward; ret_seq[k] = s; len = len + 1; len_seq[k] = len
        carry = 0 if done else s;  len = 0 if done else len

    carry float32 [N] and length_carry int32 [N] are numpy arrays UPDATED IN PLACE as the device updates its tensors (None: fresh
    zeros for this call), so two scans in a row equal one over the joined rows.  Returns (ret_seq float32 [K, N], len_seq int32
    [K, N]); bit-equal to the device."""
    r = np.asarray(rewards, dtype=np.float32)
    d = np.asarray(dones, dtype=np.uint8)
    if r.ndim != 2 or r.shape != d.shape:
        raise ValueError(f"rewards and dones must share one [K, N] shape, got {r.shape}, {d.shape}")
    N = r.shape[1]
    for what, a, dt in (("carry", carry, np.float32), ("length_carry", length_carry, np.int32)):
        if a is not None and (not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != (N,)):
            raise ValueError(f"{what} must be a numpy {np.dtype(dt).name} array of shape {(N,)} (it is updated in place)")
    c = np.zeros(N, dtype=np.float32) if carry is None else carry
    ln = np.zeros(N, dtype=np.int32) if length_carry is None else length_carry
    g = np.float32(gamma)
    ret, lens = np.empty_like(r), np.empty(r.shape, dtype=np.int32)
    zero = np.float32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(r.shape[0]):
            s = ((g * c).astype(np.float32) + r[k]).astype(np.float32)
            n = (ln + np.int32(1)).astype(np.int32)
            ret[k], lens[k] = s, n
            c[:] = np.where(d[k] != 0, zero, s)
            ln[:] = np.where(d[k] != 0, np.int32(0), n)
    return ret, lens
