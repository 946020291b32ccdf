"""Golden vectors for TripletLoss under the non-cosine measures (forward + autograd), produced by
running the REFERENCE's own module on the CPU:

  LINAS-engine/loss.py:13-73    order / euclidean / L1 / L1_norm / L2 / L2_norm / jaccard sims
  LINAS-engine/loss.py:83-153   TripletLoss(measure=...) forward, torch autograd backward

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_triplet_measures.py /root/reference
Writes tests/golden/triplet_measures.npz.  torch.Tensor.cuda is patched to identity (loss.py:146-148
calls .cuda() on its zero terms), as make_golden_model.py does.

Per measure: one input pair (B = 33, D = 37: D crosses the kernels' 32-deep K slab; positive inputs for
jaccard, l2-normalised rows for the rest) and four configurations at margin 0.2.  Each configuration
runs through the reference module twice, in fp32 and with .double() inputs; stored are the inputs, the
fp64 loss and gradients, and the fp32 run's max-abs error against them (loss, ds, dim) -- the tests'
tolerance is a multiple of that error.

Conditioning is a condition, not a tolerance: the seed of each measure is searched until
  * every off-diagonal fp64 hinge argument |margin + S_ij - S_dd| is at least 16 x the fp32 run's own
    max score error max|S32 - S64|, and
  * under max_violation every row's / column's positive winning cost leads its runner-up by that much,
so neither the reference's fp32 rounding nor a port's can flip a hinge or an argmax.

The tie / zero-distance cases are hand-made at 2 x 2 x 3 and recorded from the same module (fp64, with their
fp64 score matrices; the fp32 run has its NaN in the same positions -- asserted).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

MEASURES = ["order", "euclidean", "jaccard", "l1", "l2", "l1_norm", "l2_norm"]
SIMS = {"order": "order_sim", "euclidean": "euclidean_sim", "jaccard": "jaccard_sim", "l1": "L1_sim", "l2": "L2_sim",
        "l1_norm": "L1_sim_norm", "l2_norm": "L2_sim_norm"}
# (name, max_violation, cost_style, direction)
CONFIGS = [("mv_sum_all", True, "sum", "all"), ("mean_all", False, "mean", "all"), ("mv_sum_t2v", True, "sum", "t2v"),
           ("sum_v2t", False, "sum", "v2t")]
MARGIN = 0.2
B, D = 33, 37
GUARD = 16.0

# tie rules (2 x 2 x 3): order has two pairs at distance exactly 0 (NaN where s_jk == im_ik), jaccard and l1
# have equal components (min / max halve the gradient there, abs gives 0)
TIES = {
    "order": ([[1, 2, 3], [0, 0, 0]], [[0, 2, 1], [1, 1, 1]]),
    "jaccard": ([[1, 2, 3], [2, 2, 1]], [[1, 3, 2], [2, 1, 1]]),
    "l1": ([[1, 2, 3], [0.5, 0, -1]], [[0.5, 0, -2], [1, 2, 2.5]]),  # (the off-diagonal pairs tie, and are active)
}


def make_inputs(measure, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, D, generator=g)
    im = torch.randn(B, D, generator=g)
    if measure == "jaccard":
        return s.abs(), im.abs()
    return torch.nn.functional.normalize(s, dim=1), torch.nn.functional.normalize(im, dim=1)


def well_conditioned(L, measure, s, im):
    sim = getattr(L, SIMS[measure])
    S64 = sim(im.double(), s.double()).numpy()
    S32 = sim(im, s).numpy().astype(np.float64)
    guard = GUARD * np.abs(S32 - S64).max()
    off = ~np.eye(B, dtype=bool)
    diag = np.diag(S64)
    for dd, axis in ((diag[:, None], 1), (diag[None, :], 0)):  # cost_s (max over dim 1), cost_im (dim 0)
        h = MARGIN + S64 - dd
        if np.abs(h[off]).min() < guard:
            return False
        cost = np.where(off, np.maximum(h, 0.0), 0.0)
        top2 = np.sort(cost, axis=axis)
        top2 = top2[:, -2:] if axis == 1 else top2[-2:, :].T
        lead = top2[:, 1] - top2[:, 0]
        if (lead[top2[:, 1] > 0] < guard).any():
            return False
    return True


def run(L, measure, mv, cs, dr, s, im):
    s = s.clone().requires_grad_(True)
    im = im.clone().requires_grad_(True)
    loss = L.TripletLoss(margin=MARGIN, measure=measure, max_violation=mv, cost_style=cs, direction=dr)(s, im)
    loss.backward()
    return loss.item(), s.grad.numpy(), im.grad.numpy()


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "LINAS-engine"))
    import loss as L  # noqa
    torch.Tensor.cuda = lambda self, *a, **k: self  # CPU-only container: keep tensors where they are

    out = {"measures": np.array(MEASURES), "configs": np.array([c[0] for c in CONFIGS]), "margin": np.array(MARGIN)}
    for m in MEASURES:
        for seed in range(1000):
            s, im = make_inputs(m, seed)
            if well_conditioned(L, m, s, im):
                break
        else:
            raise AssertionError(f"{m}: no well-conditioned seed")
        assert well_conditioned(L, m, s, im)
        out[f"{m}_s"], out[f"{m}_im"], out[f"{m}_seed"] = s.numpy(), im.numpy(), np.array(seed)
        for name, mv, cs, dr in CONFIGS:
            l32, ds32, dim32 = run(L, m, mv, cs, dr, s, im)
            l64, ds64, dim64 = run(L, m, mv, cs, dr, s.double(), im.double())
            assert np.isfinite(ds64).all() and np.isfinite(dim64).all()
            k = f"{m}_{name}"
            out[f"{k}_loss"], out[f"{k}_ds"], out[f"{k}_dim"] = np.array(l64), ds64, dim64
            out[f"{k}_err"] = np.array([abs(l32 - l64), np.abs(ds32 - ds64).max(), np.abs(dim32 - dim64).max()])
            print(k, "seed", seed, "loss", l64, "max|ds|", np.abs(ds64).max(), "fp32 err", out[f"{k}_err"])
    for m, (im, s) in TIES.items():
        s, im = torch.tensor(s, dtype=torch.float32), torch.tensor(im, dtype=torch.float32)
        l32, ds32, dim32 = run(L, m, False, "sum", "all", s, im)
        l64, ds64, dim64 = run(L, m, False, "sum", "all", s.double(), im.double())
        assert np.array_equal(np.isnan(ds32), np.isnan(ds64)) and np.array_equal(np.isnan(dim32), np.isnan(dim64))
        out[f"tie_{m}_s"], out[f"tie_{m}_im"] = s.numpy(), im.numpy()
        out[f"tie_{m}_loss"], out[f"tie_{m}_ds"], out[f"tie_{m}_dim"] = np.array(l64), ds64, dim64
        out[f"tie_{m}_S"] = getattr(L, SIMS[m])(im.double(), s.double()).numpy()  # (the scale of the loss's rounding)
        print("tie", m, "loss", l64, "ds", ds64.tolist(), "dim", dim64.tolist())
    assert np.array_equal(np.isnan(out["tie_order_dim"][0]), [True, True, False]) and out["tie_order_dim"][0, 2] == 0
    path = os.path.join(HERE, "triplet_measures.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
