"""BSELL-ST without a GPU: the builder's structure and refusals, the
torch_ref SpMV against the long-double oracle, and the mutants of the
kernel's steps that the oracle bound must reject."""

import numpy as np
import pytest
import torch

import kernel_oracle as ko
import symtile_systems as ss
from acg_amd.ops import symtile, torch_ref

CPU = "cpu"
KERNEL_CASES = [(g, dof, o) for g in ss.CUBES for dof in ss.DOFS
                for o in ss.ORDERS]


def _tensors(st):
    return {k: v for k, v in vars(st).items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("shape,dof,order", KERNEL_CASES + [(ss.STRIP, 3, "brick")])
def test_ref_spmv_bsell_st(shape, dof, order):
    st = ss.build(shape, dof, order)
    assert st is not None and st.tile == 256 and st.qmax == 8
    for dotslot in (-1, ko.S_PT):
        got = ss.run_spmv(torch_ref, st, shape, dof, CPU, dotslot=dotslot)
        ko.assert_accepts(ss.expect(shape, dof, dotslot), got,
                          f"{shape} dof{dof} {order} dot{dotslot}")
    # the numpy replay of the kernel's steps computes the same thing
    ko.assert_accepts(ss.expect(shape, dof), ss.emulate(st, shape, dof),
                      "emulate")


@pytest.mark.parametrize("shape,dof,order", [(3, 3, "natural"), (5, 2, "brick"),
                                             (5, 4, "natural")])
def test_stored_operator_is_the_permuted_matrix(shape, dof, order):
    """Own blocks plus implied transposes give P A P^T bit for bit."""
    s = ss.system(shape, dof)
    st = ss.build(shape, dof, order)
    vp = st.vperm.numpy()
    want = s.Af.toarray()[np.ix_(vp, vp)]
    assert ko._bits_equal(ss.dense_from_st(st), want)


@pytest.mark.parametrize("shape,dof,order", [(5, 3, "brick"), (12, 3, "brick"),
                                             (12, 2, "natural"), (ss.STRIP, 4, "brick")])
def test_builder_structure(shape, dof, order):
    s = ss.system(shape, dof)
    st = ss.build(shape, dof, order)
    d2 = dof * dof
    nsl = (s.nnodes + 63) // 64
    ar = torch.arange(s.nnodes)
    # permutation: a bijection, composed with its inverse the identity
    assert torch.equal(st.perm[st.iperm], ar) and torch.equal(st.iperm[st.perm], ar)
    assert torch.equal(st.vperm.view(-1, dof)[:, 0], st.perm * dof)
    # tile membership is the hint's: the in-tile sort moves no node out
    order0 = ss.node_order(shape, order)
    order0 = ar if order0 is None else torch.from_numpy(order0)
    pos0 = torch.empty_like(ar)
    pos0[order0] = ar
    assert torch.equal(pos0[st.perm] // st.tile, ar // st.tile)
    # inside a tile stored counts descend
    node, col, vals, q = ss.decode(st)
    cnt = np.bincount(node[(vals != 0).any(axis=1)], minlength=s.nnodes)
    for t in range(st.ntiles):
        c = cnt[t * st.tile:(t + 1) * st.tile]
        assert np.all(np.diff(c) <= 0)
    # stored bytes equal the formula and the arrays' own sizes
    blen = (st.sptr[1:] - st.sptr[:-1]) // 64
    nslot = int(((blen - st.spl) * 64).sum())
    stotal = int(st.sptr[-1])
    assert st.svals.numel() == stotal * d2 and st.scol.numel() == stotal
    assert st.sq.numel() == stotal and st.nrecv.numel() == nsl * 64
    formula = (stotal * (8 * d2 + 4) + nslot + nsl * 64 + (nsl + 1) * 8 + nsl * 4)
    sizes = (st.svals.numel() * 8 + st.scol.numel() * 4 + nslot
             + st.nrecv.numel() + st.sptr.numel() * 8 + st.spl.numel() * 4)
    assert st.stored_bytes == formula == sizes
    bptr = ss.bsell(shape, dof)[0]
    assert st.bsell_bytes == int(bptr[-1]) * (8 * d2 + 4) + (nsl + 1) * 8
    assert st.ratio == st.stored_bytes / st.bsell_bytes
    # slots: a receiver's slots are 0 .. nrecv-1, each written once, by a
    # node of its own tile; nobody exceeds the cap
    snd = q != symtile.NOSEND
    assert np.all(node[snd] // st.tile == col[snd] // st.tile)
    nr = st.nrecv.numpy()[:s.nnodes]
    assert nr.max() <= st.qmax and not st.nrecv.numpy()[s.nnodes:].any()
    cell = col[snd] * 256 + q[snd]
    assert len(np.unique(cell)) == len(cell)
    assert np.array_equal(np.bincount(col[snd], minlength=s.nnodes), nr)
    assert np.all(q[snd] < nr[col[snd]])
    # two builds are bitwise equal
    again = _tensors(ss.build(shape, dof, order))
    for k, v in _tensors(st).items():
        assert torch.equal(v, again[k]), k


def test_tile_boundary_cuts_a_brick():
    """12^3 in 8 x 8 x 4 bricks: partial bricks shift the 256-node tiles,
    so some brick lies in two tiles."""
    st = ss.build(12, 3, "brick")
    old = st.perm.numpy()
    z, y, x = old // 144, (old // 12) % 12, old % 12
    brick = ((z // 4) * 2 + y // 8) * 2 + x // 8
    tile = np.arange(len(old)) // 256
    assert max(len(set(tile[brick == b])) for b in range(brick.max() + 1)) >= 2


def test_cap_pushes_pairs_back_to_two_plain_blocks():
    shape, dof = 5, 3
    st = ss.build(shape, dof, "brick", qmax=2)
    nr = st.nrecv.numpy()[:st.nnodes]
    assert nr.max() == 2 and (nr == 2).any()
    over = ss.overcap_pairs(st)
    assert over, "no pair was pushed over the cap"
    node, col, vals, q = ss.decode(st)
    k = over[0]  # both directions stored, both plain, nothing sent
    back = np.nonzero((node == col[k]) & (col == node[k]))[0]
    assert len(back) == 1 and q[back[0]] == symtile.NOSEND
    s = ss.system(shape, dof)
    vp = st.vperm.numpy()
    assert ko._bits_equal(ss.dense_from_st(st), s.Af.toarray()[np.ix_(vp, vp)])
    got = ss.run_spmv(torch_ref, st, shape, dof, CPU, dotslot=ko.S_PT)
    ko.assert_accepts(ss.expect(shape, dof, ko.S_PT), got, "qmax2")


@pytest.mark.parametrize("kw", [dict(qmax=0), dict(tile=1)])
def test_no_receives_anywhere(kw):
    """A one-node tile (or a zero cap) has no pairs: plain BSELL in the
    permuted order."""
    st = ss.build(5, 3, "brick", **kw)
    assert not st.nrecv.any() and st.npaired == 0
    assert (ss.decode(st)[3] == symtile.NOSEND).all()
    got = ss.run_spmv(torch_ref, st, 5, 3, CPU)
    ko.assert_accepts(ss.expect(5, 3), got, str(kw))


def test_refuses_one_ulp_off_the_transpose():
    shape, dof = 5, 3
    s = ss.system(shape, dof)
    bptr, bcol, bvals = ss.bsell(shape, dof)
    # an off-diagonal block of node 0 (natural order: nodes 0 and 1 share
    # tile 0): its (0, 1) element one ulp up
    blk = next(j for j in range(8) if int(bcol[j * 64]) == 1)
    idx = int(symtile.val_index(torch.tensor([blk * 64]), torch.tensor([0]),
                                dof * dof)[0, 1])
    assert bvals[idx] != 0
    bad = bvals.clone()
    bad[idx] = torch.nextafter(bad[idx], torch.tensor(float("inf"), dtype=torch.float64))
    assert ss.build(shape, dof, "natural", arrays=(bptr, bcol, bvals)) is not None
    assert ss.build(shape, dof, "natural", arrays=(bptr, bcol, bad)) is None
    # the same block pair split over two tiles is no intra-tile pair:
    # a one-node tile accepts the perturbed operator
    assert ss.build(shape, dof, "natural", arrays=(bptr, bcol, bad), tile=1) is not None
    assert s.nnodes == 125


def test_byte_gate_decides():
    # the default gate (0.9): bricks pass, a zero cap stores everything
    st = ss.build(12, 3, "brick", gate=symtile.GATE)
    assert st is not None and st.ratio <= 0.9
    assert ss.build(12, 3, "brick", gate=symtile.GATE, qmax=0) is None
    free = ss.build(12, 3, "brick", qmax=0)
    assert free.ratio > 0.9
    # just under / just over the ratio the build reaches
    assert ss.build(12, 3, "brick", gate=st.ratio * (1 + 1e-12)) is not None
    assert ss.build(12, 3, "brick", gate=st.ratio * (1 - 1e-6)) is None


def test_builder_argument_errors():
    bptr, bcol, bvals = ss.bsell(3, 2)
    with pytest.raises(TypeError):
        symtile.bsell_st_build(bptr, bcol, bvals.float(), 27, 2)
    with pytest.raises(ValueError):
        symtile.bsell_st_build(bptr, bcol, bvals, 27, 2, np.zeros(27, np.int64))
    with pytest.raises(ValueError):
        symtile.bsell_st_build(bptr, bcol, bvals, 27, 2, qmax=255)
    with pytest.raises(ValueError):
        symtile.bsell_st_build(bptr, bcol, bvals, 91, 2)


@pytest.mark.parametrize("mutant", ss.MUTANTS)
@pytest.mark.parametrize("shape,dof", [(5, 3), (12, 2)])
def test_mutants_are_rejected(shape, dof, mutant):
    """Each wrong step, replayed on the inputs the kernels see, leaves the
    oracle bound; the unmutated replay stays inside."""
    qmax = 2 if mutant == "overcap_dropped" else 8
    st = ss.build(shape, dof, "brick", qmax=qmax)
    e = ss.expect(shape, dof)
    assert ko.accepts(e, ss.emulate(st, shape, dof))
    assert not ko.accepts(e, ss.emulate(st, shape, dof, mutant)), mutant
