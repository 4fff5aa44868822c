"""The streaming BN apply kernels hold U rows in flight: a row's result must
not depend on the slot, the loop (U-row trips or the one-row loop behind them)
or the block it lands in.

Every input is P = 7 distinct random rows tiled to M rows (7 is odd and
coprime to every stride gm * rows_per_blk used here, which _rows_geom
asserts, so a thread's rows run through all seven), so
whatever the batch statistics are, output row m must be torch.equal to output
row m mod 7: y, the packed mask, dx, dres, dz, both branches of the two-BN
tail. A wrong row offset in one slot, in the tail loop or in a ragged block
breaks that. The values themselves are checked against the float64 reference
and the error model of tests/test_bn_geometry_gpu.py (its _check_forward /
_check_backward: integer dy, exact dbias, bounds from the number formats).

_rows_geom mirrors bn_apply_gm in csrc/ext.hip and the kernels' loops, and
each case states which (U-row trips, single rows) a thread runs. U comes from
the extension (BN_APPLY_FWD_U, BN_APPLY_BWD_U, BN_APPLY2_U); a family built
with U = 1 runs its one-row loop only and the statements about trips are
skipped for it.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_bn_geometry_gpu import (  # noqa: F401 - ext is a fixture
    BLOCK, BN_VEC, EPS, _check_backward, _check_forward, _flat, _geom,
    _inputs, _nhwc, ext)

pytestmark = pytest.mark.gpu

P = 7


def _rows_geom(C, M, U):
    """Mirror of bn_apply_gm and of the apply kernels' loops: the set of
    (U-row trips, single rows) over the threads that own a row."""
    tx = min(C // BN_VEC, BLOCK)
    rpb = BLOCK // tx
    grid_c = -(-(C // BN_VEC) // tx)
    rows = -(-M // rpb)
    cap = max(4096 // grid_c, 1)
    if U == 1:
        gm = min(rows, cap)
    else:
        trips = -(-rows // (U * cap))
        gm = -(-rows // (U * trips))
    bx = np.arange(gm)[:, None]
    ty = np.arange(rpb)[None, :]
    first = bx * rpb + ty
    n = np.maximum(0, -(-(M - first) // (gm * rpb)))
    n = n[n > 0]
    assert n.sum() == M
    # a thread's rows must run through all residues mod P
    assert np.gcd(gm * rpb, P) == 1, (gm, rpb)
    return dict(tx=tx, rpb=rpb, grid_c=grid_c, rows=rows, gm=gm, cap=cap,
                leftover=BLOCK - tx * rpb,
                loops={(int(k) // U, int(k) % U) for k in np.unique(n)})


# name -> (C, M as a function of U, what the geometry must look like)
CASES = {
    # fewer block-rows than one trip: single rows only
    "below-one-trip": (8, lambda U: 3, lambda g, U: g["loops"] == {(0, 1)}),
    # every thread runs exactly one U-row trip; tx_count = 1
    "exactly-U": (8, lambda U: 256 * 2 * U, lambda g, U: g["tx"] == 1
                  and g["loops"] == {(1, 0)}),
    # one row more: the grid grows by a block, thread (0, 0) runs a trip that
    # ends in the ragged last block-row, all others U - 1 single rows
    "U-plus-one": (64, lambda U: 32 * 3 * U + 1, lambda g, U:
                   g["loops"] == {(1, 0), (0, U - 1)}),
    # ragged last block and tx_count = 3, which does not divide 256
    "ragged-tx3": (24, lambda U: 85 * 3 * U - 20, lambda g, U: g["tx"] == 3
                   and g["leftover"] == 1
                   and g["loops"] == {(1, 0), (0, U - 1)}),
    # grid_c = 2, one live thread column in the second block column
    "grid-c-2": (2056, lambda U: 18 * U - 1, lambda g, U: g["grid_c"] == 2
                 and g["loops"] == {(1, 0), (0, U - 1)}),
}
# the grid cap is hit (rows > U * 4096): several U-row trips per thread, and
# the last blocks end in single rows. ~34 M elements: one case.
BIG = (2048, 16507, lambda g, U: g["rows"] > U * g["cap"]
       and any(a >= 1 and b >= 1 for a, b in g["loops"])
       and max(a for a, _ in g["loops"]) >= 2)


def _forces(ext, attr, C, M, forces):
    U = getattr(ext, attr)
    g = _rows_geom(C, M, U)
    if U > 1:
        assert forces(g, U), f"case no longer forces its loops: U={U} {g}"
    return g


def _tile(t, M):
    return t.repeat(-(-M // P), 1)[:M].contiguous()


def _assert_tiled(name, t4d_or_2d):
    t = _flat(t4d_or_2d) if t4d_or_2d.dim() == 4 else t4d_or_2d
    assert torch.equal(t, _tile(t[:P], t.size(0))), \
        f"{name}: a row differs from the row 7 before it"


@functools.lru_cache(maxsize=None)
def _data(C, M, dtype):
    """P random rows tiled to M; dy holds small integers (exact sums)."""
    x, res, dy, w, b, rm, rv = _inputs(C, P, dtype, True, seed=C + M)
    zd, _, dy_b, wd, bd, _, _ = _inputs(C, P, dtype, True, seed=C + M + 1)
    t = {k: _tile(v, M) for k, v in dict(x=x, res=res, dy=dy, zd=zd,
                                         dy_b=dy_b).items()}
    t.update(w=w, b=b, wd=wd, bd=bd, rm=rm, rv=rv)
    return t


def _forward_family(ext, C, M, dtype):
    d = _data(C, M, dtype)
    geo = _geom(C, M)
    x4, r4 = _nhwc(d["x"]), _nhwc(d["res"])
    outs = {}
    for relu, res in ((False, None), (True, None), (True, r4), (False, r4)):
        rm, rv = d["rm"].clone(), d["rv"].clone()
        y, sm, sr = ext.bn_fwd_train(x4, d["w"], d["b"], rm, rv, res, EPS,
                                     0.1, relu, None)
        _assert_tiled(f"y relu={relu} res={res is not None}", y)
        _check_forward(geo, d["x"], d["res"] if res is not None else None,
                       d["w"], d["b"], d["rm"], d["rv"], 0.1, relu, _flat(y),
                       sm, sr, rm, rv)
        outs[(relu, res is not None)] = y
    for res in (None, r4):
        y, sm, sr, mask = ext.bn_fwd_train_mask(
            x4, d["w"], d["b"], d["rm"].clone(), d["rv"].clone(), res, EPS,
            0.1, True, None)
        assert torch.equal(y, outs[(True, res is not None)])
        _assert_tiled("mask", mask)
        bits = (_flat(y) > 0).reshape(M, C // 8, 8).to(torch.int32)
        want = (bits << torch.arange(8, device="cuda")).sum(-1)
        assert torch.equal(mask.to(torch.int32), want), "mask != y > 0"


def _add_bn_family(ext, C, M, dtype):
    d = _data(C, M, dtype)
    geo = _geom(C, M)
    z4, zd4 = _nhwc(d["x"]), _nhwc(d["zd"])
    rm, rv = d["rm"].clone(), d["rv"].clone()
    rmd, rvd = d["rm"].clone(), d["rv"].clone()
    y, mask, sm, sr, smd, srd = ext.bn_fwd_train_add_bn(
        z4, zd4, d["w"], d["b"], rm, rv, EPS, 0.1, None, d["wd"], d["bd"],
        rmd, rvd, EPS, 0.1, None)
    _assert_tiled("y", y)
    _assert_tiled("mask", mask)
    # the identity the kernel rounds to T in registers, as the plain kernel
    # stores it; then the tail is the residual form with that identity
    ident, _, _ = ext.bn_fwd_train(zd4, d["wd"], d["bd"], d["rm"].clone(),
                                   d["rv"].clone(), None, EPS, 0.1, False,
                                   None)
    _check_forward(geo, d["zd"], None, d["wd"], d["bd"], d["rm"], d["rv"],
                   0.1, False, _flat(ident), smd, srd, rmd, rvd)
    _check_forward(geo, d["x"], _flat(ident), d["w"], d["b"], d["rm"],
                   d["rv"], 0.1, True, _flat(y), sm, sr, rm, rv)


def _backward_family(ext, C, M, dtype):
    d = _data(C, M, dtype)
    geo = _geom(C, M)
    x4, r4, dy4 = _nhwc(d["x"]), _nhwc(d["res"]), _nhwc(d["dy"])
    y, sm, sr, mask = ext.bn_fwd_train_mask(
        x4, d["w"], d["b"], d["rm"].clone(), d["rv"].clone(), r4, EPS, 0.1,
        True, None)
    # <none>, <y> and <mask>, each without and with dres
    for relu, dres, fn, sign in (
            (False, False, ext.bn_bwd, y), (False, True, ext.bn_bwd, y),
            (True, False, ext.bn_bwd, y), (True, True, ext.bn_bwd, y),
            (True, False, ext.bn_bwd_mask, mask),
            (True, True, ext.bn_bwd_mask, mask)):
        out = fn(x4, dy4, sign, sm, sr, d["w"], relu, dres, None)
        tag = f"{fn.__name__} relu={relu} dres={dres}"
        _assert_tiled("dx " + tag, out[0])
        if dres:
            _assert_tiled("dres " + tag, out[3])
        _check_backward(geo, d["x"], d["dy"], _flat(y), sm, sr, d["w"], relu,
                        _flat(out[0]), out[1], out[2],
                        _flat(out[3]) if dres else None)
    # the join: <none> apply on the dz its reduce wrote
    dx, dw, db, dz = ext.bn_bwd_mask_join(x4, dy4, _nhwc(d["dy_b"]), mask, sm,
                                          sr, d["w"], None)
    _assert_tiled("join dx", dx)
    _assert_tiled("join dz", dz)
    _check_backward(geo, d["x"], d["dy"] + d["dy_b"], _flat(y), sm, sr,
                    d["w"], True, _flat(dx), dw, db, _flat(dz))


def _joint_family(ext, C, M, dtype):
    d = _data(C, M, dtype)
    geo = _geom(C, M)
    z4, zd4 = _nhwc(d["x"]), _nhwc(d["zd"])
    y, mask, sm, sr, smd, srd = ext.bn_fwd_train_add_bn(
        z4, zd4, d["w"], d["b"], d["rm"].clone(), d["rv"].clone(), EPS, 0.1,
        None, d["wd"], d["bd"], d["rm"].clone(), d["rv"].clone(), EPS, 0.1,
        None)
    dz, dw, db, dym, dzd, dwd, dbd = ext.bn_bwd_mask_join(
        z4, _nhwc(d["dy"]), _nhwc(d["dy_b"]), mask, sm, sr, d["w"], None, zd4,
        smd, srd, d["wd"], None)
    for name, t in (("dz", dz), ("dzd", dzd), ("dym", dym)):
        _assert_tiled(name, t)
    s = d["dy"] + d["dy_b"]
    _check_backward(geo, d["x"], s, _flat(y), sm, sr, d["w"], True, _flat(dz),
                    dw, db, _flat(dym))
    _check_backward(geo, d["zd"], s, _flat(y), smd, srd, d["wd"], True,
                    _flat(dzd), dwd, dbd, None)


FAMILIES = {
    "fwd": ("BN_APPLY_FWD_U", _forward_family),
    "fwd_add_bn": ("BN_APPLY_FWD_U", _add_bn_family),
    "bwd": ("BN_APPLY_BWD_U", _backward_family),
    "bwd_two_bn": ("BN_APPLY2_U", _joint_family),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_apply_rows(ext, family, case, dtype):
    attr, run = FAMILIES[family]
    C, m_of_u, forces = CASES[case]
    M = m_of_u(max(getattr(ext, attr), 2))
    _forces(ext, attr, C, M, forces)
    run(ext, C, M, dtype)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_apply_rows_grid_cap(ext, family):
    attr, run = FAMILIES[family]
    C, M, forces = BIG
    _forces(ext, attr, C, M, forces)
    run(ext, C, M, torch.bfloat16)
