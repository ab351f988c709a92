"""tests/pgraph_ref.py (the references of tests/test_gpu_pgraph_ops.py and tests/test_gpu_rpn_loss.py) pinned from outside the
code under test: adjacency and soft-max against the CPU oracle's own lines for one group (oracle/detector.py: bbox_overlaps with
a unit diagonal > 0, D M D, ((1 - M) * sim).softmax(-1)), the RPN sums against torch's loss operators on targets from the
project's coder."""
import pytest
import torch
import torch.nn.functional as F

import pgraph_ref as R

D64 = torch.float64
COUNTS = [0, 1, 2, 17, 40, 64]          # ragged groups in a padding of 64, an empty and a one-box group among them


def close64(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


def padded_groups(gen, counts, npad):
    """boxes (G, npad, 4) float64 with NaN in the padding; clustered so that about half the pairs overlap"""
    G = len(counts)
    c = torch.rand(G, npad, 2, generator=gen, dtype=D64) * 100
    wh = torch.rand(G, npad, 2, generator=gen, dtype=D64) * 40 + 2
    boxes = torch.cat([c - wh / 2, c + wh / 2], -1)
    boxes[~R.below(counts, npad)] = float('nan')
    return boxes


def test_adjacency_and_softmax_are_the_oracle_lines_per_group():
    from oracle import boxes as B
    gen = torch.Generator().manual_seed(3)
    npad = 64
    boxes = padded_groups(gen, COUNTS, npad)
    boxes[3, 5] = boxes[3, 4]                                                   # a duplicate
    boxes[3, 6] = torch.tensor([1000., 1000., 1001., 1001.], dtype=D64)          # overlaps nothing: degree 1
    sim = torch.randn(len(COUNTS), npad, npad, generator=gen, dtype=D64) * 3
    pad = ~(R.below(COUNTS, npad)[:, :, None] & R.below(COUNTS, npad)[:, None, :])
    sim[pad] = float('nan')
    sim.requires_grad_()
    A_local = R.local_adjacency(boxes, COUNTS)
    A_glob = R.global_softmax(sim, A_local, COUNTS)
    assert A_local.shape == A_glob.shape == (len(COUNTS), npad, npad)
    assert torch.isfinite(A_local).all() and torch.isfinite(A_glob).all()
    gA = torch.randn(A_glob.shape, generator=gen, dtype=D64)
    gsim, = torch.autograd.grad(A_glob, sim, gA)
    A_glob = A_glob.detach()
    for g, c in enumerate(COUNTS):
        assert float(A_local[g, c:].abs().max() if c < npad else 0) == 0 and float(A_local[g, :, c:].abs().max() if c < npad else 0) == 0
        assert float(A_glob[g, c:].abs().sum()) == 0 and float(A_glob[g, :, c:].abs().sum()) == 0
        assert float(gsim[g, c:].abs().sum()) == 0 and float(gsim[g, :, c:].abs().sum()) == 0
        if c == 0:
            continue
        rois_ = boxes[g, :c]
        sim_ = sim.detach()[g, :c, :c].clone().requires_grad_()
        M = B.bbox_overlaps(rois_, rois_).fill_diagonal_(1.)
        M = (M > 0).to(D64)
        D = torch.diag(M.sum(-1).pow(-0.5))
        close64(A_local[g, :c, :c], torch.mm(torch.mm(D, M), D))
        assert torch.equal(R.local_mask(boxes, COUNTS)[g, :c, :c], M.bool())
        ref = ((1. - M) * sim_).softmax(-1)
        close64(A_glob[g, :c, :c].detach(), ref.detach())
        gref, = torch.autograd.grad(ref, sim_, gA[g, :c, :c])
        close64(gsim[g, :c, :c], gref)
        assert float((gsim[g, :c, :c] * M).abs().max()) == 0                    # local pairs: logit 0 whatever sim is
    assert float(A_local[1, 0, 0]) == 1.0 and float(A_glob[1, 0, 0]) == 1.0     # the one-box group
    assert float(A_local[3, 6, 6]) == 1.0 and float(A_local[3, 6].sum()) == 1.0


def test_adjacency_computes_in_the_dtype_of_its_inputs():
    gen = torch.Generator().manual_seed(4)
    boxes = padded_groups(gen, COUNTS, 64)
    a64, a32 = R.local_adjacency(boxes, COUNTS), R.local_adjacency(boxes.float(), COUNTS)
    assert a64.dtype == D64 and a32.dtype == torch.float32
    torch.testing.assert_close(a32.double(), a64, rtol=1e-6, atol=1e-7)


def test_bgemm_nt_is_the_per_group_mm():
    gen = torch.Generator().manual_seed(5)
    a, b = torch.randn(3, 5, 8, generator=gen, dtype=D64), torch.randn(3, 7, 8, generator=gen, dtype=D64)
    c = R.bgemm_nt(a, b)
    for g in range(3):
        close64(c[g], torch.mm(a[g], b[g].t()))
    assert torch.equal(R.below([0, 2, 5], 4), torch.tensor([[0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1]]).bool())


@pytest.mark.parametrize('beta,pos_weight', [(1. / 9., -1.), (1.0, 2.5), (None, -1.), (None, 2.5)])
def test_rpn_loss_is_torch_bce_and_smooth_l1_on_coder_targets(beta, pos_weight):
    from htd_amd.core.bbox import bbox2delta
    gen = torch.Generator().manual_seed(7)
    Bn, A, K = 2, 300, 3
    means, stds = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
    c = torch.rand(A, 2, generator=gen, dtype=D64) * 200
    wh = torch.rand(A, 2, generator=gen, dtype=D64) * 60 + 8
    anchors = torch.cat([c - wh / 2, c + wh / 2], 1).float().double()           # fp32 values: the coder computes in fp32
    gc = torch.rand(Bn, K, 2, generator=gen, dtype=D64) * 200
    gwh = torch.rand(Bn, K, 2, generator=gen, dtype=D64) * 80 + 8
    gts = torch.cat([gc - gwh / 2, gc + gwh / 2], -1).float().double()
    u = torch.rand(Bn, A, generator=gen)
    pos, neg = u < 0.1, (u > 0.08) & (u < 0.4)                                  # rows flagged both: 0.08 < u < 0.1
    assert int((pos & neg).sum()) > 0
    assigned = torch.where(pos, torch.randint(1, K + 1, (Bn, A), generator=gen), torch.randint(-1, 1, (Bn, A), generator=gen))
    cls = torch.randn(Bn, A, generator=gen, dtype=D64) * 4
    reg = torch.randn(Bn, A, 4, generator=gen, dtype=D64) * 0.5
    cls[~(pos | neg)] = float('nan')
    reg[~pos] = float('nan')
    cls.requires_grad_()
    reg.requires_grad_()
    s_cls, s_box = R.rpn_loss(cls, reg, anchors, gts, assigned, pos, neg, means, stds, beta, pos_weight)
    g_cls, g_reg = torch.autograd.grad(s_cls + s_box, (cls, reg))

    sampled = pos | neg
    x = cls.detach()[sampled].clone().requires_grad_()
    t = pos[sampled].double()
    w = torch.where(pos[sampled], torch.tensor(pos_weight if pos_weight > 0 else 1., dtype=D64), torch.tensor(1., dtype=D64))
    ref_cls = F.binary_cross_entropy_with_logits(x, t, weight=w, reduction='sum')
    close64(s_cls.detach(), ref_cls.detach())
    assert float(g_cls[~sampled].abs().sum()) == 0
    close64(g_cls[sampled], torch.autograd.grad(ref_cls, x)[0])

    b_idx, a_idx = pos.nonzero(as_tuple=True)
    pa, pg = anchors[a_idx], gts[b_idx, assigned[pos] - 1]
    tgt32 = bbox2delta(pa, pg, means, stds)                                     # the project's coder: fp32 arithmetic
    assert tgt32.dtype == torch.float32
    tgt64 = (R.rpn_targets(anchors, gts, assigned, pos) - torch.tensor(means, dtype=D64)) / torch.tensor(stds, dtype=D64)
    torch.testing.assert_close(tgt64, tgt32.double(), rtol=2e-6, atol=2e-6)     # a few fp32 roundings of O(1) deltas / std 0.1
    p = reg.detach()[pos].clone().requires_grad_()
    for tgt, tol in ((tgt64, 1e-12), (tgt32.double(), 1e-5)):
        ref_box = F.l1_loss(p, tgt, reduction='sum') if beta is None else F.smooth_l1_loss(p, tgt, beta=beta, reduction='sum')
        torch.testing.assert_close(s_box.detach(), ref_box.detach(), rtol=tol, atol=tol)
    ref_box = F.l1_loss(p, tgt64, reduction='sum') if beta is None else F.smooth_l1_loss(p, tgt64, beta=beta, reduction='sum')
    assert float(g_reg[~pos].abs().sum()) == 0
    close64(g_reg[pos], torch.autograd.grad(ref_box, p)[0])
