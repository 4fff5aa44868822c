"""Joint backward of the two-BN tail y = relu(bn3(z) + bn_ds(zd)) whose dy
arrives as two addends.

The two-BN signature of bn_bwd_mask_join(z, dy_a, dy_b, mask, stats, weight,
ws, zd, stats_d, weight_d, ws_d) runs one reduce over z, zd, dy_a, dy_b and
the mask (bn_bwd_reduce_join2_kernel) and one apply over z, zd and the masked
sum (bn_bwd_apply2_kernel). The reference is what it replaces, run in the same
build: the one-BN bn_bwd_mask_join on z, then the mask-less bn_bwd on zd with
the dym that call returned. The joint reduce keeps the grid, the rows per
thread, the order and the expressions of those two reduces, and the joint
apply the arithmetic of their apply, so every output must be torch.equal: dz,
dzd, dym, both dweight and both dbias.
"""
import functools

import pytest
import torch

from tests.test_bn_geometry_gpu import (  # noqa: F401 - ext is a fixture
    EPS, _geom, _inputs, _make_ws, _nhwc, ext)
from tests.test_bn_grad_join_gpu import _chain_grads, _make_chain

pytestmark = pytest.mark.gpu

# M = 3: less than one block; 257: a ragged second block at C = 8; 6149: the
# reduce's grid-stride loop with a tail (C = 64: 193 block-rows on 64 blocks)
CS, MS = (8, 64, 2056), (3, 257, 6149)
assert _geom(64, 6149)["rows"] == 193 and _geom(64, 6149)["gm"] == 64
assert _geom(2056, 6149)["grid_c"] == 2 and _geom(8, 257)["rows"] == 2


@functools.lru_cache(maxsize=None)
def _case(C, M, dtype):
    """The tail's forward (mask, statistics of both BNs) and three pairs of
    gradient addends, computed once per shape and shared read-only."""
    from autodist_amd.ops import api
    e = api.ext()
    z, zd, _, w, b, rm, rv = _inputs(C, M, dtype, True, seed=C + M)
    g = torch.Generator(device="cuda").manual_seed(C + M + 3)
    wd = torch.rand(C, generator=g, device="cuda") + 0.5
    bd = torch.randn(C, generator=g, device="cuda")
    _, mask, sm, sr, smd, srd = e.bn_fwd_train_add_bn(
        _nhwc(z), _nhwc(zd), w, b, rm.clone(), rv.clone(), EPS, 0.1, None,
        wd, bd, rm.clone(), rv.clone(), EPS, 0.1, None)
    rnd = lambda: torch.randn(M, C, generator=g, device="cuda")  # noqa: E731
    a = rnd().to(dtype)
    # ties and zeros: a third of the sums is a plus half a bf16 ulp of a
    # (a = m * 2^ex with m in [0.5, 1): the ulp is 2^(ex - 8)), halfway
    # between two bf16 values; a third is a - a = 0; the rest is random
    pick = torch.randint(0, 3, (M, C), generator=g, device="cuda")
    ex = torch.frexp(a.float())[1]
    tie = (torch.ldexp(torch.ones_like(a, dtype=torch.float32), ex - 9)
           * torch.sign(a.float())).to(dtype)
    b_tz = torch.where(pick == 0, tie, torch.where(pick == 1, -a,
                                                   rnd().to(dtype)))
    grads = {"randn": (a, rnd().to(dtype), mask),
             "ties+zeros": (a, b_tz, mask),
             "zero-mask": (a, rnd().to(dtype), torch.zeros_like(mask))}
    if dtype == torch.bfloat16 and M * C >= 1000:
        exact = a.float() + b_tz.float()
        low = exact.view(torch.int32) & 0xFFFF
        assert (low == 0x8000).float().mean().item() > 0.25, "too few ties"
        assert (exact == 0).float().mean().item() > 0.25, "too few zeros"
    if M * C >= 1000:
        assert 0 < int(mask.ne(0).sum()) and int(mask.ne(0xFF).sum()) > 0
    return dict(z=z, zd=zd, w=w, wd=wd, sm=sm, sr=sr, smd=smd, srd=srd,
                grads=grads)


NAMES = ("dz", "dweight", "dbias", "dym", "dzd", "dweight_d", "dbias_d")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("C", CS)
def test_joint_backward_equals_join_then_bn_bwd(ext, C, M, dtype):
    f = _case(C, M, dtype)
    z4, zd4 = _nhwc(f["z"]), _nhwc(f["zd"])
    for kind, (a, b, mask) in f["grads"].items():
        a4, b4 = _nhwc(a), _nhwc(b)
        ref = list(ext.bn_bwd_mask_join(z4, a4, b4, mask, f["sm"], f["sr"],
                                        f["w"], _make_ws(C, "persistent")[1]))
        ref += ext.bn_bwd(zd4, ref[3], ref[3], f["smd"], f["srd"], f["wd"],
                          False, False, _make_ws(C, "persistent")[1])
        # NaN-filled workspaces of its own for each branch, and none at all
        for ws, wsd in ((_make_ws(C, "persistent")[1],
                         _make_ws(C, "persistent")[1]), (None, None)):
            out = ext.bn_bwd_mask_join(z4, a4, b4, mask, f["sm"], f["sr"],
                                       f["w"], ws, zd4, f["smd"], f["srd"],
                                       f["wd"], wsd)
            assert len(out) == 7
            for name, got, want in zip(NAMES, out, ref):
                assert got.shape == want.shape and got.dtype == want.dtype
                assert torch.equal(got, want), (kind, name, ws is None)
        if kind == "zero-mask":
            assert not ref[3].any() and not ref[0].any() and not ref[4].any()
        else:
            assert ref[3].any()


def test_joint_backward_rejects_mismatched_branches(ext):
    f = _case(64, 257, torch.bfloat16)
    a, b, mask = f["grads"]["randn"]
    z4, zd4, a4, b4 = (_nhwc(t) for t in (f["z"], f["zd"], a, b))
    head = (mask, f["sm"], f["sr"], f["w"])
    tail = (f["smd"], f["srd"], f["wd"])
    ws = _make_ws(64, "persistent")[1]
    with pytest.raises(RuntimeError):  # one workspace for both branches
        ext.bn_bwd_mask_join(z4, a4, b4, *head, ws, zd4, *tail, ws)
    with pytest.raises(RuntimeError):  # zd of another dtype
        ext.bn_bwd_mask_join(z4, a4, b4, *head, None, zd4.float(), *tail,
                             None)
    with pytest.raises(RuntimeError):  # zd of another shape
        ext.bn_bwd_mask_join(z4, a4, b4, *head, None, _nhwc(f["zd"][:-1]),
                             *tail, None)


# ------------------------------------------------------------- model level
class _ArgCounts:
    """Records the argument count of every ext.bn_bwd_mask_join call."""

    def __init__(self, e):
        self.e, self.orig, self.seen = e, e.bn_bwd_mask_join, []

    def __enter__(self):
        def recorded(*args):
            self.seen.append(len(args))
            return self.orig(*args)
        self.e.bn_bwd_mask_join = recorded
        return self

    def __exit__(self, *exc):
        self.e.bn_bwd_mask_join = self.orig


def test_two_block_chain_equals_split_path(ext):
    """A downsample Bottleneck, then an identity one, through forward_pair.
    The first block's output has two consumers, so its tail's backward is the
    two-BN call; the second block's output has one. With SPLIT_PATH the same
    chain runs the separate kernels and autograd's add."""
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(3)
        chain3, out_ch = _make_chain("bottleneck")
        chain = torch.nn.ModuleList(list(chain3)[:2])
        state = {k: v.clone() for k, v in chain.state_dict().items()}
        x = torch.randn(4, 32, 10, 10, device="cuda").contiguous(
            memory_format=torch.channels_last)
        dy = torch.randn(4, out_ch, 5, 5, device="cuda").to(
            torch.bfloat16).contiguous(memory_format=torch.channels_last)
        with _ArgCounts(ext) as n_new:
            new = _chain_grads(ext, chain, x, dy, split=False)
        chain.load_state_dict(state)
        with _ArgCounts(ext) as n_old:
            old = _chain_grads(ext, chain, x, dy, split=True)
    finally:
        torch.backends.cudnn.deterministic = det
    assert n_new.seen == [13] and n_old.seen == [], (n_new.seen, n_old.seen)
    assert torch.equal(new[0], old[0]), "output"
    assert torch.equal(new[1], old[1]), "dx"
    for (name, _), a, c in zip(chain.named_parameters(), new[2], old[2]):
        assert torch.equal(a, c), name
    for k in new[3]:
        assert torch.equal(new[3][k], old[3][k]), k
