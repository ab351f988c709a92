"""Plain tensor formulations of the PGraph kernels of csrc/pgraph.hip, of the batched NT product (htd_bgemm_nt, htd_bgemm_nt_counts)
and of the fused RPN loss (htd_rpn_loss, htd_rpn_loss_l1 of csrc/box_ops.hip): the references tests/test_gpu_pgraph_ops.py and
tests/test_gpu_rpn_loss.py hold the kernels to.  No HIP and no C ABI in here; backward passes come from autograd on these formulas.
tests/test_pgraph_ref.py pins every function to the CPU oracle's own lines and to torch's loss operators, so the references
cannot drift with the code under test.

Every function computes in the dtype of its inputs (the tests pass float64; passing float32 gives the "same formula in fp32"
figure that the float checks scale their bound by).  Groups are padded as the kernels see them: group g holds counts[g] real
entries in slots 0..counts[g]-1 of npad; what the padding holds (the tests put NaN there) is never read."""
import torch


def _overlap_mask(bx):
    """(IoU with unit diagonal) > 0 of (n, 4) boxes with the arithmetic of bbox_overlaps (iou2d_calculator.py:148-150)."""
    n = bx.size(0)
    lt = torch.max(bx[:, None, :2], bx[None, :, :2])
    rb = torch.min(bx[:, None, 2:], bx[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
    union = torch.max(area[:, None] + area[None, :] - inter, bx.new_tensor([1e-6]))
    return (inter / union > 0) | torch.eye(n, dtype=torch.bool)


def local_mask(boxes, counts):
    """M of every group as a bool (G, npad, npad), False in the padding."""
    G, npad = boxes.shape[:2]
    M = torch.zeros(G, npad, npad, dtype=torch.bool)
    for g, c in enumerate(int(c) for c in counts):
        M[g, :c, :c] = _overlap_mask(boxes[g, :c])
    return M


def local_adjacency(boxes, counts):
    """boxes (G, npad, 4), counts (G,) -> A_local = D^-1/2 M D^-1/2 (G, npad, npad), M = (IoU with unit diagonal) > 0,
    D = rowsum(M) (htd_bbox_head.py:207-210); zeros in the padding."""
    M = local_mask(boxes, counts).to(boxes.dtype)
    dinv = M.sum(-1).clamp(min=1).pow(-0.5)                  # padded rows: degree 0, any finite factor
    return dinv[:, :, None] * M * dinv[:, None, :]


def global_softmax(sim, A_local, counts):
    """A_glob = softmax_row((1 - M) * sim) over the counts[g] valid columns of every valid row, M = A_local > 0
    (htd_bbox_head.py:211,214-215: local pairs keep logit 0); rows and columns of the padding are zeros."""
    out = sim.new_zeros(sim.shape)
    for g, c in enumerate(int(c) for c in counts):
        if c:
            M = (A_local[g, :c, :c] > 0).to(sim.dtype)
            out[g, :c, :c] = ((1. - M) * sim[g, :c, :c]).softmax(-1)
    return out


def bgemm_nt(a, b):
    """c[g] = a[g] @ b[g]^T: a (G, M, K), b (G, N, K) -> (G, M, N)."""
    return a @ b.transpose(1, 2)


def below(counts, n):
    """(G, n) bool: slot < counts[g], the validity of a padded axis."""
    return torch.arange(n)[None, :] < torch.as_tensor(counts)[:, None]


def rpn_targets(anchors, gts, assigned, pos):
    """bbox2delta (delta_xywh_bbox_coder.py:100-118, before means / stds) of the positive rows, in its order of operations:
    anchors (A, 4), gts (B, K, 4), assigned (B, A) = 1 + the gt of the row -> (P, 4) in the row order of pos.nonzero()."""
    b, a = pos.nonzero(as_tuple=True)
    p, g = anchors[a], gts[b, assigned[b, a] - 1]
    px, py, pw, ph = (p[:, 0] + p[:, 2]) * 0.5, (p[:, 1] + p[:, 3]) * 0.5, p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    gx, gy, gw, gh = (g[:, 0] + g[:, 2]) * 0.5, (g[:, 1] + g[:, 3]) * 0.5, g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    return torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph)], -1)


def rpn_loss(cls, reg, anchors, gts, assigned, pos, neg, means, stds, beta, pos_weight):
    """AnchorHead.loss_single summed over the batch with the targets of _get_targets_single (anchor_head.py:172-269,373-418):
         sum_cls = sum over the sampled rows (pos | neg) of w * BCEWithLogits(cls, t), t = 1 on positives, w = pos_weight on
                   positives when pos_weight > 0, else 1;
         sum_box = sum over the positives and the 4 components of SmoothL1_beta(reg - target) (beta None: |reg - target|),
                   target = (bbox2delta(anchor, gt[assigned - 1]) - means) / stds.
    cls (B, A), reg (B, A, 4), pos / neg (B, A) bool.  Rows outside the sums are selected away, never multiplied by zero: what
    cls holds on unsampled rows and reg on non-positive rows does not matter.  -> (sum_cls, sum_box)"""
    pos, neg = pos.bool(), neg.bool()
    sampled = pos | neg
    x, t = cls[sampled], pos[sampled].to(cls.dtype)
    w = torch.where(pos[sampled], cls.new_tensor(pos_weight if pos_weight > 0 else 1.), cls.new_tensor(1.))
    sum_cls = (w * (x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs())))).sum()
    tgt = (rpn_targets(anchors, gts, assigned, pos) - reg.new_tensor(means).view(1, 4)) / reg.new_tensor(stds).view(1, 4)
    d = (reg[pos] - tgt).abs()
    if beta is None:
        sum_box = d.sum()
    else:
        sum_box = torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta).sum()
    return sum_cls, sum_box


def check_float(name, out, ref64, cpu32, run):
    """The FLOAT rule of tests/test_gpu_glue_ops.py: e = max |out - ref64| / max |ref64| <= F x max(e_cpu, 2^-23),
    F = max(8, sqrt(run)); prints the figures before it asserts.  -> e / bound"""
    from glue_ref import float_bound, rel_err
    e, e_cpu = rel_err(out, ref64), rel_err(cpu32, ref64)
    bound = float_bound(e_cpu, run)
    print(f'{name}: e_kernel {e:.3e}  e_cpu {e_cpu:.3e}  R {run}  bound {bound:.3e}  ratio {e / bound:.3f}')
    assert e <= bound, f'{name}: e_kernel {e:.3e} > bound {bound:.3e} (e_cpu {e_cpu:.3e}, R {run})'
    return e / bound


def check_exact(name, out, ref64):
    """EXACT: the device result must torch.equal the float64 one cast to fp32."""
    ref = ref64.detach().to(torch.float32)
    out = out.detach().cpu()
    assert out.shape == ref.shape, (name, tuple(out.shape), tuple(ref.shape))
    assert torch.equal(out, ref), \
        f'{name}: {int((out != ref).sum())} of {ref.numel()} differ, max |diff| {float((out - ref).abs().max()):.3e}'
