"""Sampled softmax on the CPU: the torch composite against the formulas in
float64, the log-uniform sampler against its closed form, and the
num_sampled path of LM1BModel, alone and through the engine at world 1."""
import copy
import math

import pytest
import torch

from autodist_amd.models.lm1b import lm1b_small
from autodist_amd.ops.sampled_softmax import (LogUniformSampler,
                                              sampled_softmax_loss)
from tests.sampled_softmax_ref import make_inputs, reference


def test_composite_matches_float64():
    h, w, b, t, c, lq_t, lq_s = make_inputs(35, 200, 96, 300, seed=0)
    g = torch.rand(35) + 0.5
    ref = reference(h, w, b, t, c, lq_t, lq_s, g)
    h, w, b = (x.clone().requires_grad_(True) for x in (h, w, b))
    rows = sampled_softmax_loss(h, w, b, t, c, lq_t, lq_s, reduction="none")
    (rows * g).sum().backward()
    dense = torch.zeros(300, 96, dtype=torch.float64).index_add_(
        0, torch.cat([c, t]), ref["dW_rows"])
    for name, got, want in (("loss", rows, ref["loss"]),
                            ("dH", h.grad, ref["dH"]), ("dW", w.grad, dense),
                            ("db", b.grad, ref["db"])):
        torch.testing.assert_close(got.detach().double(), want, rtol=1e-4,
                                   atol=1e-4, msg=lambda m: f"{name}: {m}")


def test_sampler_logq_closed_form():
    R, S = 1000, 4096
    sampler = LogUniformSampler(R, S, seed=3)
    ids, logq = sampler.sample()
    assert ids.shape == (S,) and ids.dtype == torch.int64
    assert ids.min() >= 0 and ids.max() < R
    k = ids.double()
    want = torch.log(S * (torch.log(k + 2) - torch.log(k + 1))
                     / math.log(R + 1))
    torch.testing.assert_close(logq.double(), want, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(sampler.logq_true(ids.view(64, 64)).double(),
                               want.view(64, 64), rtol=1e-6, atol=1e-6)
    # log-uniform: about ln(11) / ln(R + 1) of the draws fall below 10
    share = (ids < 10).double().mean().item()
    assert abs(share - math.log(11) / math.log(R + 1)) < 0.05
    again = LogUniformSampler(R, S, seed=3).sample()[0]
    assert torch.equal(ids, again)


def test_lm1b_num_sampled():
    torch.manual_seed(0)
    model = lm1b_small(vocab_size=500, sparse=True, num_sampled=64,
                       dropout=0.0)
    toks = torch.randint(0, 500, (4, 6))
    tgts = torch.randint(0, 500, (4, 6))
    model.train()
    model.loss(toks, tgts).backward()
    grad = model.emb.weight.grad
    assert grad.is_sparse
    assert grad.coalesce().indices().size(1) <= 64 + 24 + 24
    assert model.out_bias.grad.count_nonzero() <= 64 + 24
    model.eval()
    logits, _ = model(toks)
    full = torch.nn.functional.cross_entropy(logits.reshape(-1, 500),
                                             tgts.reshape(-1))
    assert torch.equal(model.loss(toks, tgts), full)
    with pytest.raises(ValueError):
        lm1b_small(vocab_size=500, sharded_softmax=True, num_sampled=64)


def test_lm1b_num_sampled_engine_step_matches_torch():
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.parallel.engine import DistributedEngine
    from autodist_amd.resource_spec import ResourceSpec
    from autodist_amd.strategy import PS
    torch.manual_seed(1)
    m_ref = lm1b_small(vocab_size=500, sparse=True, num_sampled=64,
                       dropout=0.0, sampler_seed=5)
    m_eng = copy.deepcopy(m_ref)
    toks = torch.randint(0, 500, (4, 6))
    tgts = torch.randint(0, 500, (4, 6))

    opt = torch.optim.Adagrad(m_ref.parameters(), lr=0.05)
    opt.zero_grad()
    m_ref.loss(toks, tgts).backward()
    opt.step()

    g = GraphItem()
    g.extend_model(m_eng)
    opt = torch.optim.Adagrad(m_eng.parameters(), lr=0.05)
    g.extend_optimizer_info(opt)
    engine = DistributedEngine(g, PS().build(g, ResourceSpec()), rank=0,
                               world_size=1, device=torch.device("cpu"))
    engine.setup()
    opt.zero_grad()
    m_eng.loss(toks, tgts).backward()
    opt.step()
    engine.drain()
    engine.teardown()
    for (name, p1), p2 in zip(m_ref.named_parameters(), m_eng.parameters()):
        assert torch.allclose(p1, p2, atol=1e-6), \
            f"{name}: {(p1 - p2).abs().max()}"
