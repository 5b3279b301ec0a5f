"""Running statistics for observation normalisation and reward scaling (the two halves of VecNormalize), kept on the device.

`RunningMeanStd` holds a count, a mean and a sum of squared deviations (M2) in float64 torch tensors and merges every batch with Chan's
parallel formula, without a host synchronisation.  `mean32` and `inv_std32 = 1 / sqrt(var + eps)` are float32 tensors refreshed IN
PLACE by `update`, so an env bound to them (`VecMazeEnv.bind_obs_norm(norm.mean32, norm.inv_std32)`) sees the new statistics at its
next call:

    norm = RunningMeanStd((env.obs_dim,), env.device)
    env.bind_obs_norm(norm.mean32, norm.inv_std32, clip=10.0)
    ...
    norm.update(rows_the_policy_acted_on)            # [K, N, obs_dim]: the kernels read the new numbers from the next call on

For reward scaling the shape is `()`: feed it the discounted returns of `VecMazeEnv.return_scan(rewards, dones, gamma, carry)` and
multiply the rewards by `inv_std32`.
"""
import torch


class RunningMeanStd:
    """Mean and variance of a stream of rows [..., *shape], float64 on `device`; see the module's docstring."""

    def __init__(self, shape, device, eps: float = 1e-8):
        self.shape = tuple(int(s) for s in shape)
        self.device = torch.device(device)
        self.eps = float(eps)
        self.count = torch.zeros((), dtype=torch.float64, device=self.device)
        self.mean = torch.zeros(self.shape, dtype=torch.float64, device=self.device)
        self.m2 = torch.zeros(self.shape, dtype=torch.float64, device=self.device)
        self.mean32 = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        self.inv_std32 = torch.ones(self.shape, dtype=torch.float32, device=self.device)

    @property
    def var(self):
        """The population variance M2 / count (0 before the first update), float64."""
        return self.m2 / torch.clamp(self.count, min=1.0)

    def update(self, x) -> None:
        """Merge the rows of x [..., *shape] (any float dtype, on the device): Chan et al.'s pairwise update of (count, mean, M2) in
        float64 — the batch's own mean and M2 by two passes —, then `mean32` and `inv_std32` in place.  No host synchronisation."""
        nd = len(self.shape)
        if x.dim() < nd or tuple(x.shape[x.dim() - nd:]) != self.shape:
            raise ValueError(f"x must have shape [..., {', '.join(map(str, self.shape))}], got {tuple(x.shape)}")
        rows = x.to(device=self.device, dtype=torch.float64).reshape((-1,) + self.shape)
        nb = rows.shape[0]
        if nb == 0:
            return
        bmean = rows.mean(dim=0)
        bm2 = ((rows - bmean) ** 2).sum(dim=0)
        tot = self.count + nb
        delta = bmean - self.mean
        self.mean += delta * (nb / tot)
        self.m2 += bm2 + delta * delta * (self.count * nb / tot)
        self.count.copy_(tot)
        self.mean32.copy_(self.mean)
        self.inv_std32.copy_(torch.rsqrt(self.var + self.eps))
