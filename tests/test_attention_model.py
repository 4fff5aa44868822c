"""CPU checks of the attention error model in tests/attention_ref.py.

The GPU tests assert |kernel - float64 reference| <= k * tol per element,
tol the first-order bound derived in tests/attention_ref.py. This module
shows, without a GPU, that the bound is neither too tight nor too loose:

  * `emulate` (fp32 torch with bf16 casts at the kernels' rounding points)
    stays inside k * tol on every bounded case and all four outputs;
  * each planted bug in MUTANTS leaves k * tol in at least one output of at
    least one case;
  * the two exact input families give bit-exact results under `emulate`,
    which guards their construction, and the numpy hash replica has the
    threshold and seed-truncation properties the kernels rely on.

The margin k. R_EMU is the emulation's worst err / tol over all CASES and
outputs at k = 1, measured on CPU inputs (test_margin_is_derived prints the
per-case figures and fails if the recorded value no longer matches):

    R_EMU = 1.83  (worst: dK of peaky-D128-S96; randn cases 0.6-1.35,
                  spiked-key ones up to 1.6, inputs x3 1.5-1.8)
    K_MARGIN = ceil(2 * R_EMU) = 4

The factor 2 is for what the emulation does not share with the kernels: the
MFMA accumulation order and the last-ulp behaviour of v_exp_f32.
"""
import math

import pytest
import torch

from tests import attention_ref as ar

R_EMU = 1.83


def _keep_for(case):
    if not case.p_drop:
        return None
    return ar.drop_keep(case.B, case.H, case.S, case.p_drop, case.seed)


@pytest.fixture(scope="module")
def table():
    """case id -> (inputs, keep, emulated outputs, reference); computed
    once, shared and left unchanged by every test here."""
    out = {}
    for case in ar.CASES:
        x = ar.make_inputs(case, "cpu")
        keep = _keep_for(case)
        emu = ar.emulate(x.q, x.k, x.v, x.dout, x.scale, x.add_mask, keep,
                         x.p_drop)
        ref = ar.reference(x.q, x.k, x.v, x.dout, x.scale, x.add_mask, keep,
                           x.p_drop, o_in=emu["O"])
        out[case.id] = (x, keep, emu, ref)
    return out


def test_case_table_covers_the_issue():
    ids = {c.id for c in ar.CASES}
    assert len(ids) == len(ar.CASES)
    for D, S in ar.SHAPES:
        assert f"plain-D{D}-S{S}" in ids
    for variant in ("plain", "drop", "mask", "mask_drop", "peaky", "spike"):
        cs = [c for c in ar.CASES if c.variant == variant]
        assert any(c.D == 64 and ar.fwd_rb(c.S) == 1 for c in cs), variant
        assert any(c.D == 64 and ar.fwd_rb(c.S) == 2 for c in cs), variant
        assert any(c.D == 128 for c in cs), variant
    assert {c.p_drop for c in ar.CASES if c.variant == "drop"} == {0.1, 0.5}


def test_margin_is_derived(table):
    worst = 0.0
    for cid, (_, _, emu, ref) in table.items():
        r = ar.ratios(emu, ref)
        print(cid, " ".join(f"{n}={r[n]:.2f}" for n in ar.OUTPUTS))
        worst = max(worst, max(r.values()))
    print(f"r_emu = {worst:.3f}")
    assert math.isfinite(worst)
    # fp32 matmul summation order may move the figure in the second decimal
    assert abs(worst - R_EMU) < 0.15, (
        f"measured r_emu {worst:.3f}, module header records {R_EMU}")
    assert ar.K_MARGIN == math.ceil(2 * R_EMU) == math.ceil(2 * worst)


@pytest.mark.parametrize("case", ar.CASES, ids=lambda c: c.id)
def test_emulation_within_bound(table, case):
    _, _, emu, ref = table[case.id]
    for name in ar.OUTPUTS:
        err = (emu[name].double() - ref.out[name]).abs()
        tol = ar.K_MARGIN * ref.tol[name]
        bad = ~(err <= tol)
        assert not bad.any(), (
            f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound")
        assert torch.isfinite(emu[name].float()).all()


def _applies(mutant, case):
    if mutant in ("no_fwd_rescale", "keep_transposed_bwd"):
        return case.p_drop > 0
    if mutant == "mask_of_batch0":
        return case.add_mask is not None
    return True


@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_mutant_is_rejected(table, mutant):
    """A planted bug must leave k * tol somewhere; where it applies it is
    in fact rejected on EVERY case, which is reported in the message."""
    killed, applied = [], 0
    for case in ar.CASES:
        x, keep, emu, _ = table[case.id]
        if not _applies(mutant, x):
            continue
        applied += 1
        bad = ar.emulate(x.q, x.k, x.v, x.dout, x.scale, x.add_mask, keep,
                         x.p_drop, mutant=mutant)
        # the backward under test is handed ITS OWN forward output
        ref = ar.reference(x.q, x.k, x.v, x.dout, x.scale, x.add_mask, keep,
                           x.p_drop, o_in=bad["O"])
        r = ar.ratios(bad, ref)
        if max(r.values()) > ar.K_MARGIN:
            killed.append((case.id, max(r, key=r.get), max(r.values())))
    assert applied >= 3
    print(mutant, f"rejected on {len(killed)} of {applied} cases; weakest "
          f"rejection {min(k[2] for k in killed) if killed else 0:.1f} x tol")
    assert killed, f"{mutant} survives the bound on all {applied} cases"


@pytest.mark.parametrize("D,S", ar.SELECT_SHAPES)
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
def test_selection_family_is_exact(D, S, p_drop):
    B, H = 2, 3
    q, k, v, dout, pi = ar.selection_inputs(B, H, S, D, "cpu")
    # the construction's claim: runner-up >= 161 below in the log2 domain
    lg = (q.double() @ k.double().transpose(-1, -2)) * ar.SELECT_SCALE \
        * ar.LOG2E
    top2 = lg.topk(2, dim=-1)
    assert torch.equal(top2.indices[..., 0], pi)
    assert float((top2.values[..., 0] - top2.values[..., 1]).min()) >= 161
    keep = ar.drop_keep(B, H, S, p_drop, 4242) if p_drop else None
    emu = ar.emulate(q, k, v, dout, ar.SELECT_SCALE, None, keep, p_drop)
    O, dV = ar.selection_expected(v, dout, pi, keep)
    assert torch.equal(emu["O"], O)
    assert torch.equal(emu["dV"], dV)
    assert torch.equal(emu["dQ"], torch.zeros_like(q))
    assert torch.equal(emu["dK"], torch.zeros_like(q))
    if keep is not None:    # both branches of keep[i, pi(i)] are present
        sel = torch.gather(keep, 3, pi[..., None])
        assert 0 < int(sel.sum()) < sel.numel()


@pytest.mark.parametrize("S,live", ar.UNIFORM_SHAPES)
def test_uniform_family_is_exact(S, live):
    B, H, D = 2, 3, 64
    q, k, v, dout, mask, alive = ar.uniform_inputs(B, H, S, D, live, "cpu")
    n = alive.sum(1)
    assert all(int(x) & (int(x) - 1) == 0 for x in n)
    emu = ar.emulate(q, k, v, dout, 0.125, mask)
    O, dV = ar.uniform_expected(v, dout, alive)
    assert torch.equal(emu["O"], O)
    assert torch.equal(emu["dV"], dV)
    assert torch.equal(emu["dK"], torch.zeros_like(q))
    ref = ar.reference(q, k, v, dout, 0.125, mask, o_in=emu["O"])
    assert ar.ratios(emu, ref)["dQ"] <= ar.K_MARGIN
    assert float(emu["dQ"].float().abs().max()) > 0


def test_drop_keep_properties():
    B, H, S = 2, 3, 96
    # seed truncation: (unsigned)(uint64_t)seed
    assert torch.equal(ar.drop_keep(B, H, S, 0.5, 2 ** 32 + 5),
                       ar.drop_keep(B, H, S, 0.5, 5))
    assert not torch.equal(ar.drop_keep(B, H, S, 0.5, 2 ** 31 + 7),
                           ar.drop_keep(B, H, S, 0.5, 7))
    # threshold: keep rate 1 - p within 5 sigma of a fair Bernoulli
    for p in (0.1, 0.5, 0.999):
        keep = ar.drop_keep(B, H, S, p, 12345)
        rate, n = keep.float().mean().item(), keep.numel()
        assert abs(rate - (1 - p)) < 5 * math.sqrt(p * (1 - p) / n), (p, rate)
    # one known value, worked by hand from the hash definition
    x = 12345 ^ 0 ^ 0 ^ 0
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(ar.drop_keep(1, 1, 32, 0.5, 12345)[0, 0, 0, 0]) == \
        int(x >= 2 ** 31)
    # heads differ (bh enters the hash), and the mask is not symmetric
    keep = ar.drop_keep(B, H, S, 0.5, 12345)
    assert not torch.equal(keep[:, 0], keep[:, 1])
    assert not torch.equal(keep, keep.transpose(-1, -2))
