"""The reference side of the UNet training tests (CPU): inputs, the oracle network
(oracle/ref_unet.py) with optionally bf16-rounded weights, and its autograd gradients.  Shared by
tests/test_unet_train_host.py and tests/test_gpu_unet_train.py; each result is computed once."""
import functools

import torch

from oracle import ref_cpu as R
from oracle import ref_unet as U

WEIGHT_SUFFIXES = (".w", ".w1", ".w2", ".ws", ".p")


def is_weight(name: str) -> bool:
    """Conv and linear weights (what the bf16 mode stores in bf16); biases stay fp32."""
    return name.endswith(WEIGHT_SUFFIXES) or name.startswith("W")


def make_inputs(D: int, T: int, B: int, seed: int = 77):
    """x0, eps [B, D] fp32 and mixed t int64 [B] that includes 0 and T - 1."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, D, generator=g) * 0.5
    eps = torch.randn(B, D, generator=g)
    t = torch.randint(0, T, (B,), generator=g)
    t[0], t[-1] = 0, T - 1
    return x0, t, eps


def oracle_params(D, C, TE, HT, seed, dtype=torch.float64, rounded=False) -> U.UNetParams:
    up = U.make_unet_params(D, C, TE, HT, seed=seed)
    if rounded:
        up = up.map(lambda v: v)
        for k in list(up.p):
            if is_weight(k):
                up.p[k] = up.p[k].float().bfloat16().double()
    return up.map(lambda v: v.to(dtype))


def oracle_loss(up: U.UNetParams, tab, emb, x0, t, eps) -> torch.Tensor:
    dt = up.p["Wt1"].dtype
    xt = R.q_sample(tab, x0.to(dt), eps.to(dt), t)
    return R.eps_mse_loss(U.unet_forward(up, xt, t, emb.to(dt)), eps.to(dt))


@functools.lru_cache(maxsize=None)
def oracle_grads(D, C, TE, HT, T, B, dtype=torch.float64, rounded=False, seed=2468):
    """({name: dL/dparam}, loss) by autograd on the oracle in ``dtype``."""
    up = oracle_params(D, C, TE, HT, seed, dtype, rounded)
    for v in up.p.values():
        v.requires_grad_(True)
    tab = R.ddpm_tables(T)
    emb = torch.from_numpy(R.timestep_embedding_table(T, TE)).double()
    x0, t, eps = make_inputs(D, T, B)
    loss = oracle_loss(up, tab, emb, x0, t, eps)
    loss.backward()
    return {k: v.grad.detach() for k, v in up.p.items()}, float(loss.detach())
