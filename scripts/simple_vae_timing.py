"""Time forward + backward of SimpleVAE.forward() + loss_function (sum mse + sum nll, every parameter's gradient) at
Physionet's widths, D = 37 inputs, L = 16 latent dims, hidden (300, 30), for B = 80, 256, 4096, 40960 rows:
  fused    lvae_amd.SimpleVAE on its fused route (mlp_vae.hip: one launch per half forward, two backward);
  stock    the same network restated with torch.nn.Linear / F.relu / torch.sigmoid and the loss in plain torch ops, fp32
           on the same GPU: what a user has without this model;
  layered  lvae_amd.SimpleVAE sent to its layered route (fused_max_rows = 0: hipBLASLt GEMMs + the bias / ReLU passes), for
           the record.
Device events around blocks of ITERS iterations, 3 warm-up blocks, the median of 9 blocks per case, the cases
alternating in one process, clocks as found; the largest difference of the fused case's loss and gradients from the
stock case's is reported with the times.  DESIGN.md and profiles/simple_vae_timing.json hold a run.

    python scripts/simple_vae_timing.py [out.json]
"""
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "longitudinal-vae_amd")]
import lvae_amd as la  # noqa: E402

DEV = "cuda"
D, L, HIDDEN = 37, 16, (300, 30)
ROWS = (80, 256, 4096, 40960)
WARMUP, BLOCKS = 3, 9


class StockVAE(nn.Module):
    """SimpleVAE in stock torch.nn (the reference's VAE.py:165-273 with an eps argument)"""

    def __init__(self, model):
        super().__init__()
        self.num_dim = model.num_dim
        self._log_vy = nn.Parameter(model._log_vy.detach().clone())
        for name in ("fc1", "fc21", "fc211", "fc221", "fc3", "fc31", "fc4"):
            src = getattr(model, name)
            fc = nn.Linear(src.in_features, src.out_features)
            fc.load_state_dict(src.state_dict())
            setattr(self, name, fc)

    def forward(self, x, eps):
        h2 = F.relu(self.fc21(F.relu(self.fc1(x))))
        mu, log_var = self.fc211(h2), self.fc221(h2)
        z = mu + eps * torch.exp(0.5 * log_var)
        return torch.sigmoid(self.fc4(F.relu(self.fc31(F.relu(self.fc3(z)))))), mu, log_var

    def loss_function(self, recon_x, x, mask):
        se = (recon_x - x) ** 2 * mask
        msum = mask.sum(1)
        msum = torch.where(msum == 0, torch.ones_like(msum), msum)
        nll = se / (2 * torch.exp(self._log_vy)) + 0.5 * (math.log(2 * math.pi) + self._log_vy)
        return se.sum(1) / msum, nll.sum(1)


def step(model, x, mask, eps):
    for p in model.parameters():
        p.grad = None
    recon, mu, log_var = model(x, eps)
    mse, nll = model.loss_function(recon, x, mask)
    loss = mse.sum() + nll.sum() + 0.1 * (mu ** 2).sum() + 0.05 * log_var.sum()
    loss.backward()
    return loss.detach()


def timed_block(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(B, seed=7):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, D, generator=gen).to(DEV)
    mask = (torch.rand(B, D, generator=gen) < 0.75).float().to(DEV)
    eps = torch.randn(B, L, generator=gen).to(DEV)
    torch.manual_seed(seed)
    fused = la.SimpleVAE(L, D, hidden=HIDDEN).to(DEV)
    layered = la.SimpleVAE(L, D, hidden=HIDDEN).to(DEV)
    layered.load_state_dict(fused.state_dict())
    stock = StockVAE(fused).to(DEV)

    layered.fused_max_rows = 0   # (every batch above 0 rows: the layered route)
    cases = {c: (lambda m=m: step(m, x, mask, eps)) for c, m in (("fused", fused), ("stock", stock),
                                                                   ("layered", layered))}
    iters = max(20, min(100, 2000000 // B))
    ms = {c: [] for c in cases}
    for rep in range(WARMUP + BLOCKS):
        for c, fn in cases.items():
            t = timed_block(fn, iters)
            if rep >= WARMUP:
                ms[c].append(t)
    res = dict(B=B, D=D, L=L, iters_per_block=iters, routes=dict(fused=fused.last_route, layered=layered.last_route))
    for c, v in ms.items():
        res[f"{c}_ms_median"], res[f"{c}_ms_min"], res[f"{c}_ms_max"] = statistics.median(v), min(v), max(v)
    res["stock_over_fused"] = res["stock_ms_median"] / res["fused_ms_median"]
    lf, ls = cases["fused"](), cases["stock"]()
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))
    res["fused_vs_stock_loss"] = rel(lf, ls)
    res["fused_vs_stock_grads"] = max(rel(p.grad, q.grad) for (_, p), (_, q) in
                                      zip(sorted(fused.named_parameters()), sorted(stock.named_parameters())))
    return res


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("simple_vae_timing: no GPU visible; nothing is measured without one")
    results = [measure(B) for B in ROWS]
    for r in results:
        print(json.dumps(r), flush=True)
    for a in sys.argv[1:]:
        if a.endswith(".json"):
            with open(a, "w") as f:
                f.write("\n".join(json.dumps(r) for r in results) + "\n")
