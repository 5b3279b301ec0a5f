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
"""
import numpy as np

MAX_HIDDEN = 64  # MZ_POLICY_MAX_HIDDEN (include/mazestep.h)


def param_count(obs_dim: int, nu: int, hidden: int = 0) -> int:
    obs_dim, nu, hidden = int(obs_dim), int(nu), int(hidden)
    if not 0 <= hidden <= MAX_HIDDEN:
        raise ValueError(f"hidden must be 0 .. {MAX_HIDDEN}, got {hidden}")
    return obs_dim * hidden + hidden + hidden * nu + nu if hidden else obs_dim * nu + nu


def _np(x):
    if hasattr(x, "detach"):  # a torch tensor
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float32)


def pack_linear(W, b):
    """Affine policy a = W @ obs + b: W [nu, obs_dim], b [nu] (nn.Linear's weight and bias) -> float32 [obs_dim * nu + nu]."""
    W, b = _np(W), _np(b)
    if W.ndim != 2 or b.shape != (W.shape[0],):
        raise ValueError(f"W must be [nu, obs_dim] and b [nu], got {W.shape} and {b.shape}")
    return np.concatenate([W.T.ravel(), b])


def pack(W1, b1, W2, b2):
    """One tanh hidden layer, a = W2 @ tanh(W1 @ obs + b1) + b2: W1 [H, obs_dim], b1 [H], W2 [nu, H], b2 [nu] -> float32 [npar]."""
    W1, b1, W2, b2 = _np(W1), _np(b1), _np(W2), _np(b2)
    if W1.ndim != 2 or W2.ndim != 2 or b1.shape != (W1.shape[0],) or W2.shape[1] != W1.shape[0] or b2.shape != (W2.shape[0],):
        raise ValueError(f"want W1 [H, obs_dim], b1 [H], W2 [nu, H], b2 [nu], got {W1.shape}, {b1.shape}, {W2.shape}, {b2.shape}")
    if not 1 <= W1.shape[0] <= MAX_HIDDEN:
        raise ValueError(f"the hidden layer has 1 .. {MAX_HIDDEN} units, got {W1.shape[0]}")
    return np.concatenate([W1.T.ravel(), b1, W2.T.ravel(), b2])


def _layer(x, Wt, b):
    """b + sum_i Wt[.., i, :] * x[.., i] in index order, float32, two roundings per term.  x [R, n]; Wt [n, m] or [R, n, m]; b [m] or [R, m]."""
    acc = np.broadcast_to(b, (x.shape[0], Wt.shape[-1])).astype(np.float32)
    for i in range(x.shape[1]):
        p = (Wt[..., i, :] * x[:, i: i + 1]).astype(np.float32)
        acc = (acc + p).astype(np.float32)
    return acc


def reference(params, obs, nu: int, hidden: int = 0, squash: bool = False, action_scale: float = 1.0):
    """The policy of csrc/mz_policy.h on rows of observations: obs [R, obs_dim] (or [obs_dim]); params [npar] shared by the rows or
    [R, npar], one policy per row.  Returns float32 [R, nu] (or [nu])."""
    x = np.asarray(obs, dtype=np.float32)
    single = x.ndim == 1
    x = np.atleast_2d(x)
    p = np.asarray(params, dtype=np.float32)
    R, od, nu, H = x.shape[0], x.shape[1], int(nu), int(hidden)
    npar = param_count(od, nu, H)
    if p.shape not in ((npar,), (R, npar)):
        raise ValueError(f"params must have shape {(npar,)} or {(R, npar)}, got {p.shape}")
    lead = p.shape[:-1]
    if H:
        o1, o2, o3 = od * H, od * H + H, od * H + H + H * nu
        h = np.tanh(_layer(x, p[..., :o1].reshape(lead + (od, H)), p[..., o1:o2])).astype(np.float32)
        acc = _layer(h, p[..., o2:o3].reshape(lead + (H, nu)), p[..., o3:])
    else:
        acc = _layer(x, p[..., : od * nu].reshape(lead + (od, nu)), p[..., od * nu:])
    out = (np.float32(action_scale) * np.tanh(acc).astype(np.float32)).astype(np.float32) if squash else acc
    return out[0] if single else out
