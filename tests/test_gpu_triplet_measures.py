"""TripletLoss under the non-cosine measures, forward and backward (K10 + K6 + K17), against the reference
module's fp64 run (tests/golden/triplet_measures.npz, made by tests/golden/make_golden_triplet_measures.py).

Tolerance of the golden comparisons: max(4 x the fixture's recorded fp32-reference error, 4 x eps32 x max|value|).
The fixture's inputs are conditioned so that no rounding can flip a hinge or an argmax (the generator asserts
it), so the port and the fp32 reference differ from the fp64 run by rounding alone; the reference's recorded
error is one sample of that noise, hence the factor 4, and an fp32 result cannot be closer than its own ulp.
A wrong or missing term moves a gradient by ~1/B of its maximum, orders above either.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEASURES = ["order", "euclidean", "jaccard", "l1", "l2", "l1_norm", "l2_norm"]
CONFIGS = {"mv_sum_all": (True, "sum", "all"), "mean_all": (False, "mean", "all"),
           "mv_sum_t2v": (True, "sum", "t2v"), "sum_v2t": (False, "sum", "v2t")}
EPS32 = float(np.finfo(np.float32).eps)


def _run(measure, s, im, mv=False, cs="sum", dr="all", margin=0.2, s_grad=True, im_grad=True):
    from cmve.linas import loss as L
    s = torch.as_tensor(s).cuda().requires_grad_(s_grad)
    im = torch.as_tensor(im).cuda().requires_grad_(im_grad)
    loss = L.TripletLoss(margin=margin, measure=measure, max_violation=mv, cost_style=cs, direction=dr)(s, im)
    loss.backward()
    return loss.detach(), s.grad, im.grad


def _close(name, got, want, ref_err, tol=None):
    got = got.double().cpu().numpy()
    if tol is None:
        tol = max(4.0 * float(ref_err), 4.0 * EPS32 * float(np.nanmax(np.abs(want))))
    err = float(np.nanmax(np.abs(got - want)))
    print(f"{name}: port err {err:.3e}  reference fp32 err {float(ref_err):.3e}  tol {tol:.3e}")
    np.testing.assert_allclose(got, want, rtol=0.0, atol=tol, equal_nan=True, err_msg=name)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("measure", MEASURES)
def test_loss_and_grads_match_reference_fp64(golden, measure, config):
    g = golden("triplet_measures")
    assert float(g["margin"]) == 0.2
    mv, cs, dr = CONFIGS[config]
    loss, ds, dim = _run(measure, g[f"{measure}_s"], g[f"{measure}_im"], mv, cs, dr)
    k = f"{measure}_{config}"
    e_loss, e_ds, e_dim = g[f"{k}_err"]
    assert ds.dtype == torch.float32 and dim.dtype == torch.float32
    _close(k + " loss", loss, g[f"{k}_loss"], e_loss)
    _close(k + " ds", ds, g[f"{k}_ds"], e_ds)
    _close(k + " dim", dim, g[f"{k}_dim"], e_dim)


@pytest.mark.parametrize("measure", ["order", "jaccard", "l1"])
def test_ties_and_zero_distance_follow_torch_autograd(golden, measure):
    """min / max halve the gradient at a_k == b_k, abs gives 0, and an order pair at distance exactly 0
    contributes NaN where s_jk == im_ik and exactly 0 elsewhere.  The gradients are sums of a few exactly
    representable weights times fp64-evaluated partials, rounded once: 4 ulp of the largest.  The loss is a sum
    of 2 B (B - 1) = 4 hinges margin + S_ij - S_dd that cancel scores of magnitude max|S|, each evaluated in fp32
    from fp32 scores: its rounding scales with the scores, not with the (small) loss, so the bound is
    4 x eps32 x (2 max|S| + margin) -- one ulp of the operands per hinge."""
    g = golden("triplet_measures")
    loss, ds, dim = _run(measure, g[f"tie_{measure}_s"], g[f"tie_{measure}_im"])
    for name, got, want in (("ds", ds, g[f"tie_{measure}_ds"]), ("dim", dim, g[f"tie_{measure}_dim"])):
        assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want)), (name, got, want)
        _close(f"tie {measure} {name}", got, want, 0.0)
    top = float(np.abs(g[f"tie_{measure}_S"]).max())
    _close(f"tie {measure} loss", loss, g[f"tie_{measure}_loss"], 0.0, tol=4 * EPS32 * (2 * top + 0.2))
    if measure == "order":
        d = dim.cpu().numpy()
        assert np.isnan(d[0, 0]) and np.isnan(d[0, 1]) and d[0, 2] == 0.0


# ---- the C entry on rectangular shapes, against torch fp64 autograd of the formulas written out here ----
def _f(metric, a, b):
    a, b = a[:, None, :], b[None, :, :]
    if metric == "sq_l2":
        return (a - b).pow(2).sum(-1)
    if metric == "l1":
        return (a - b).abs().sum(-1)
    if metric == "order":
        return (b - a).clamp(min=0).pow(2).sum(-1).sqrt()
    return torch.min(a, b).sum(-1) / torch.max(a, b).sum(-1)


def _code(metric):
    from cmve import _lib
    return {"sq_l2": _lib.PW_SQ_L2, "l1": _lib.PW_L1, "order": _lib.PW_ORDER, "jaccard": _lib.PW_JACCARD}[metric]


def _rect_case(metric, na, nb, d, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.round(torch.randn(na, d, generator=gen, dtype=torch.float64) * 4) / 4  # 0.25 grid: plenty of ties
    b = torch.round(torch.randn(nb, d, generator=gen, dtype=torch.float64) * 4) / 4
    if metric == "jaccard":
        a, b = a.abs() + 0.25, b.abs() + 0.25
    ds = torch.randn(na, nb, generator=gen, dtype=torch.float64).float().double()
    ds = ds * (torch.rand(na, nb, generator=gen) < 0.5)  # about half exactly 0
    return a, b, ds


@pytest.mark.parametrize("metric", ["sq_l2", "l1", "order", "jaccard"])
def test_pairwise_bwd_rectangular_edges(metric):
    """Tile / slab edges (1, 63, 64, 65, 130, 200 rows; d = 1, 31, 33, 515), lda > d, zero coefficients, ties.
    Tolerance: the forward's own in test_pairwise_kernel_edges (rtol 1e-5, atol 1e-5 x max|want|)."""
    from cmve import engine
    alpha = 0.5
    for seed, (na, nb, d) in enumerate([(1, 1, 1), (63, 65, 31), (64, 130, 33), (200, 7, 515)]):
        a, b, ds = _rect_case(metric, na, nb, d, seed)
        a.requires_grad_(True)
        b.requires_grad_(True)
        ((alpha * _f(metric, a, b)) * ds).sum().backward()
        ta = torch.full((na, d + 3), 7.0, dtype=torch.float32).cuda()[:, :d]
        ta.copy_(a.detach())
        assert ta.stride(0) == d + 3  # lda > d
        tb, tds = b.detach().float().cuda(), ds.float().cuda()
        da, db = engine.pairwise_bwd(ta, tb, _code(metric), alpha, tds)
        for name, got, want in (("dA", da, a.grad.numpy()), ("dB", db, b.grad.numpy())):
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
            top = np.nanmax(np.abs(want)) if np.isfinite(want).any() else 0.0
            np.testing.assert_allclose(got.double().cpu().numpy(), want, rtol=1e-5, atol=1e-5 * top, equal_nan=True,
                                       err_msg=f"{metric} {name} {(na, nb, d)}")
        # one side only: the other is not computed, the requested one is the same bits
        da1, none_b = engine.pairwise_bwd(ta, tb, _code(metric), alpha, tds, need_b=False)
        none_a, db1 = engine.pairwise_bwd(ta, tb, _code(metric), alpha, tds, need_a=False)
        assert none_a is None and none_b is None
        assert torch.equal(da1.view(torch.int32), da.view(torch.int32))
        assert torch.equal(db1.view(torch.int32), db.view(torch.int32))
    # na = 0: an empty dA, and a zero dB
    da, db = engine.pairwise_bwd(torch.zeros((0, 8), device="cuda"), torch.ones((5, 8), device="cuda"), _code(metric),
                                 alpha, torch.zeros((0, 5), device="cuda"))
    assert da.shape == (0, 8) and db.shape == (5, 8) and not db.any()


def test_pairwise_bwd_refuses_metrics_without_a_backward():
    from cmve import _lib, engine
    x = torch.ones((4, 8), device="cuda")
    for metric in (_lib.PW_L2, _lib.PW_DOT):
        with pytest.raises(_lib.CmveError, match="no backward"):
            engine.pairwise_bwd(x, x, metric, 1.0, torch.ones((4, 4), device="cuda"))


def test_pairwise_bwd_checks_its_arguments():
    """House-style argument checks of the C entry: nothing is launched on a refused call."""
    from cmve import _lib, engine
    x = torch.ones((4, 8), device="cuda")
    ds, out = torch.ones((4, 4), device="cuda"), torch.empty((4, 8), device="cuda")
    need = engine.pairwise_bwd_workspace(4, 4, _lib.PW_JACCARD)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    h, p = engine.handle(x.device), engine._ptr

    def call(a=x, lda=8, d=8, ldd=4, da=out, ldda=8, w=ws, wb=need, metric=_lib.PW_JACCARD):
        return _lib.lib.cmve_pairwise_bwd(h, p(a), lda, 4, p(x), 8, 4, d, metric, 1.0, p(ds), ldd, p(da), ldda,
                                          None, 8, p(w), wb)
    assert call() == 0
    for kw, msg in ((dict(a=None), b"NULL"), (dict(lda=7), b"bad shape"), (dict(ldd=3), b"bad shape"),
                    (dict(d=0), b"bad shape"), (dict(ldda=7), b"leading dimension"), (dict(metric=9), b"unknown metric"),
                    (dict(wb=need - 1), b"workspace too small"), (dict(w=None), b"workspace too small")):
        assert call(**kw) < 0, kw
        assert msg in _lib.lib.cmve_last_error(), (kw, _lib.lib.cmve_last_error())
    torch.cuda.synchronize()


def _batch(B, D, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, generator=gen).abs(), torch.randn(B, D, generator=gen).abs()


def test_backward_is_deterministic():
    s, im = _batch(130, 70, 3)
    _, ds1, dim1 = _run("jaccard", s, im)
    _, ds2, dim2 = _run("jaccard", s, im)
    assert ds1.abs().max() > 0 and dim1.abs().max() > 0
    assert torch.equal(ds1.view(torch.int32), ds2.view(torch.int32))
    assert torch.equal(dim1.view(torch.int32), dim2.view(torch.int32))


@pytest.mark.parametrize("measure", ["jaccard", "order", "l1"])
def test_no_b_b_d_buffer(measure):
    """B = 256, D = 1024: one B x B x D fp32 temporary is 256 MiB; the step may allocate an eighth of that
    (the design needs ~5 MB: S, dS, the coefficient workspace and two gradients)."""
    from cmve.linas import loss as L
    B, D = 256, 1024
    s, im = _batch(B, D, 4)
    s, im = s.cuda().requires_grad_(True), im.cuda().requires_grad_(True)
    crit = L.TripletLoss(margin=0.2, measure=measure, max_violation=False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    crit(s, im).backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"{measure}: peak grew by {grown / 2**20:.2f} MiB")
    assert s.grad is not None and im.grad is not None
    assert grown < B * B * D * 4 // 8


def test_unknown_measure_is_cosine():
    gen = torch.Generator().manual_seed(5)
    s = torch.nn.functional.normalize(torch.randn(48, 40, generator=gen), dim=1)
    im = torch.nn.functional.normalize(torch.randn(48, 40, generator=gen), dim=1)
    want = _run("cosine", s, im, mv=True)
    got = _run("no-such-measure", s, im, mv=True)
    for w, g_ in zip(want, got):
        assert torch.equal(w.view(torch.int32), g_.view(torch.int32))


def test_input_without_requires_grad_gets_none():
    s, im = _batch(40, 37, 6)
    _, ds, dim = _run("l1_norm", s, im)
    _, ds_none, dim_only = _run("l1_norm", s, im, s_grad=False)
    _, ds_only, dim_none = _run("l1_norm", s, im, im_grad=False)
    assert ds_none is None and dim_none is None
    assert torch.equal(dim_only.view(torch.int32), dim.view(torch.int32))
    assert torch.equal(ds_only.view(torch.int32), ds.view(torch.int32))


@pytest.mark.parametrize("measure", ["l1", "order"])
def test_trainer_step_with_a_non_cosine_criterion(measure):
    """GTTrainer takes the criterion as an object: nothing on its path assumes cosine.  Seven steps with a
    non-cosine TripletLoss, eager and as a captured graph (no host synchronisation in K10 / K6 / K17), from the
    same weights and dropout seed: the same kernels in the same order, so the same trajectory -- the bounds are
    those of test_graphed_step_equals_eager_step -- and the heads do move."""
    from cmve.linas.model import Latent_mapping
    from cmve.linas.loss import TripletLoss
    from cmve.linas import train as T
    torch.manual_seed(2)
    init = [Latent_mapping([96, 64], 0.2).cuda(), Latent_mapping([80, 64, 64], 0.2).cuda()]
    batches = [(torch.randn(32, 96, device="cuda"), torch.randn(32, 80, device="cuda")) for _ in range(3)]
    runs = []
    for graph in (False, True):
        heads = [Latent_mapping([96, 64], 0.2).cuda(), Latent_mapping([80, 64, 64], 0.2).cuda()]
        for h, h0 in zip(heads, init):
            h.load_state_dict(h0.state_dict())
        tr = T.GTTrainer(heads[0], heads[1], TripletLoss(0.2, measure, True, 'sum', 'all'), learning_rate=1e-3,
                         grad_clip=2.0, graph=graph)
        tr.train_start()
        T.manual_seed(77)
        losses = [tr.train_emb(*batches[i % 3])[1] for i in range(7)]
        runs.append((losses, [p.detach().clone() for p in tr.params]))
    assert np.isfinite(runs[0][0]).all() and all(l > 0 for l in runs[0][0])
    np.testing.assert_allclose(runs[1][0], runs[0][0], rtol=1e-6)
    for a, b in zip(runs[1][1], runs[0][1]):
        torch.testing.assert_close(a, b, rtol=0, atol=1e-6)
    moved = [float((p - p0.detach()).abs().max()) for p, p0 in zip(runs[0][1], [q for h in init for q in h.parameters()])]
    assert max(moved) > 1e-4, moved
