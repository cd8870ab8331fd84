"""GPU: L2 adversarial training (TrainPipeline(pgd=dict(..., norm=2))) against the composed oracle, eager against graph replay,
and the random start inside training (num_random_init=1: keyed by the model's device step counter)."""
import numpy as np
import pytest
import torch

import lp_attacks_ref as L
from helpers import build_model, dev, load_params, read_params
from oracle import constraints_ref as R, mlp_ref as P

pytestmark = pytest.mark.gpu


def _spec():
    return [P.LayerSpec(s.n_in, s.n_out, s.bn, 0.0, s.nonneg) for s in P.vd_constrained_spec()]


def _data(n=96, seed=41):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 880)).astype(np.float32)  # standardised features
    y = P.to_categorical(rng.integers(0, 10, n), 10).astype(np.float32)
    return x, y


@pytest.mark.parametrize("compute", ("float32", "float16x2"))
def test_l2_adversarial_training_steps_match_the_composed_oracle(cuda, compute):
    """(On both training arithmetics, at the same bounds: the fp16 two-plane mode claims those of exact fp32; the attack runs on
    exact fp32 in either.)  Three L2 adversarial-training steps at batch 32, dropout off: PGD-20 (eps 0.5, eps_step 0.1, norm 2, the batch's labels,
    inference-mode network) -> training step on x_adv -> Adam + NonNeg -> simple_norm_constraint, against the same composition
    of the restatement and the oracle (lp_attacks_ref.pgd -> mlp_ref.train_step -> constraints_ref.simple_norm_constraint_pass),
    held to the terms of test_adversarial_training_steps_match_the_composed_oracle.  The oracle takes ITS training step from the
    device's x_adv, so that the parameter comparison measures the step's arithmetic.  Then the same three steps eagerly: bit
    for bit the graph-replayed run."""
    from lipasr.pipeline import TrainPipeline

    spec = _spec()
    p = P.init_params(spec, seed=10, dtype=np.float32, nonneg_init=True)
    x, y = _data()
    eps, eps_step, iters = 0.5, 0.1, 20
    runs = []
    for use_graph in (True, False):
        m = build_model(spec, max_batch=32, compute_dtype=compute)
        load_params(m, p)
        pipe = TrainPipeline(m, batch=32, rho=0.1, constraint="product", use_graph=use_graph,
                             pgd=dict(eps=eps, eps_step=eps_step, max_iter=iters, norm=2))
        p64, st = p.astype(np.float64), P.AdamState()
        solid = [None] * 6
        advs = []
        for k, s in enumerate(range(0, 96, 32)):
            yb = y[s:s + 32].astype(np.float64)
            pipe.step(None, dev(y[s:s + 32]), features=dev(x[s:s + 32]))
            pipe.synchronize()
            x_adv = pipe.x_adv.cpu().numpy().astype(np.float64)
            advs.append(pipe.x_adv.clone())
            if not use_graph:
                continue
            feats = x[s:s + 32].astype(np.float64)
            assert (np.sqrt(((x_adv - feats) ** 2).sum(axis=1)) <= eps * (1 + 1e-6)).all()
            ref_adv = L.pgd(spec, p64, feats, eps, eps_step, iters, norm=2, y=yb)
            close = np.sqrt(((x_adv - ref_adv) ** 2).sum(axis=1)) <= 1e-3 * eps
            assert close.mean() >= 0.99, (k, close.mean())

            def loss_at(z):
                return P.forward_backward(spec, p64, z, yb, training=False)["loss"]

            l_dev, l_ref, l_clean = loss_at(x_adv), loss_at(ref_adv), loss_at(feats)
            # (as in the L-inf test: after two projected steps the inference-mode output of this network may no longer depend on
            # its input, so equality is allowed from the second step on; the first step must be a real ascent)
            assert abs(l_dev - l_ref) <= 2e-3 * max(1.0, abs(l_ref)) and l_dev >= l_clean and (k > 0 or l_dev > l_clean), (k, l_dev, l_ref, l_clean)
            out = P.train_step(spec, p64, st, x_adv, yb)
            for l in range(6):
                g = np.abs(out["dW"][l])
                assert g.max() > 0, l
                ok = g > 1e-3 * g.max()
                solid[l] = ok if solid[l] is None else (solid[l] & ok)
            new_w, norms = R.simple_norm_constraint_pass([w.astype(np.float32) for w in p64.W], 0.1, [])
            p64.W = [w.astype(np.float64) for w in new_w]
        pipe.synchronize()
        assert int(m._step.item()) == 3
        if use_graph:
            after = read_params(m, spec)
            np.testing.assert_allclose(pipe.norms.cpu().numpy(), norms, rtol=2e-3)
            for l in range(6):
                d = np.abs(after.W[l] - p64.W[l]) / np.abs(p64.W[l]).max()
                assert solid[l].mean() > 0.05, (l, solid[l].mean())
                assert d[solid[l]].max() < 2e-3, (l, d[solid[l]].max())
                assert np.quantile(d, 0.999) < 2e-3 and d.max() < 5e-2, (l, np.quantile(d, 0.999), d.max())
        runs.append((m._params.clone(), m._bnstate.clone(), pipe.norms.clone(), advs))
        pipe.close()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][3], runs[1][3]))


def test_random_start_in_training(cuda):
    """num_random_init=1: the start is drawn from the eps ball keyed by the model's device step counter, so two steps on the
    same batch start apart, a replayed graph draws afresh each step, and two pipelines of the same seed reproduce each other
    (eager or graph).  max_iter=0 exposes the start itself in x_adv."""
    from lipasr.pipeline import TrainPipeline

    spec = _spec()
    p = P.init_params(spec, seed=12, dtype=np.float32, nonneg_init=True)
    x, y = _data(32, seed=43)
    xt, yt = dev(x), dev(y)

    def run(use_graph, iters, norm=2):
        m = build_model(spec, max_batch=32)
        load_params(m, p)
        pipe = TrainPipeline(m, batch=32, rho=0.1, constraint="product", use_graph=use_graph,
                             pgd=dict(eps=0.5, eps_step=0.1, max_iter=iters, norm=norm, num_random_init=1))
        starts = []
        for _ in range(3):  # the same batch every step
            pipe.step(None, yt, features=xt)
            pipe.synchronize()
            starts.append(pipe.x_adv.clone())
        out = (starts, m._params.clone())
        pipe.close()
        return out

    a, pa = run(True, 0)
    b, pb = run(True, 0)
    c, pc = run(False, 0)
    for s in a:
        d = (s - xt).double()
        assert float(d.norm(dim=1).max()) <= 0.5 * (1 + 1e-6) and float(d.norm(dim=1).min()) > 0
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2])
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and all(torch.equal(u, v) for u, v in zip(a, c))
    assert torch.equal(pa, pb) and torch.equal(pa, pc)
    # with iterations, in both norms: graph replay equals eager bit for bit
    for norm in (2, np.inf):
        g, pg = run(True, 20, norm)
        e, pe = run(False, 20, norm)
        assert all(torch.equal(u, v) for u, v in zip(g, e)) and torch.equal(pg, pe)
        lim = (g[0] - xt).abs().max(dim=1).values if norm == np.inf else (g[0] - xt).norm(dim=1)
        assert float(lim.max()) <= 0.5 * (1 + 1e-6) + 1e-6


def test_pgd_dict_validation(cuda):
    from lipasr.pipeline import TrainPipeline

    m = build_model(_spec(), max_batch=32)
    with pytest.raises(ValueError):
        TrainPipeline(m, batch=32, pgd=dict(eps=0.5, norm=3))
    with pytest.raises(ValueError):
        TrainPipeline(m, batch=32, pgd=dict(eps=0.5, num_random_init=2))
