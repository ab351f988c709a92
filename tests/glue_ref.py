"""Plain float64 tensor formulations of the small fused operators of csrc/roi_ops.hip and of the two coder kernels of
csrc/box_ops.hip: the references tests/test_gpu_glue_ops.py holds the kernels to.  No HIP and no C ABI in here; backward
passes come from autograd on these formulas.  tests/test_glue_ref.py pins every function to torch's own operators, to the CPU
oracle and to the recorded answers of the reference project, so the references cannot drift with the code under test.

Every function computes in the dtype of its inputs (the tests pass float64; passing float32 gives the "same formula in fp32"
figure that the float checks scale their bound by).  Layout is logical NCHW throughout."""
import numpy as np
import torch


def group_norm_relu(x, gamma, beta, G, eps=1e-5, relu=True):
    """GroupNorm(G) [+ ReLU] on (n, C, h, w): the GN + ReLU of the regression branch and of ConvModule(norm_cfg=GN),
    htd_bbox_head.py:48,89,111.  -> y, mean (n, G), rstd (n, G); biased variance, statistics over (C / G, h, w)."""
    n, C, h, w = x.shape
    xg = x.reshape(n, G, C // G * h * w)
    mean = xg.mean(2)
    var = ((xg - mean[:, :, None]) ** 2).mean(2)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = ((xg - mean[:, :, None]) * rstd[:, :, None]).reshape(n, C, h, w)
    y = xh * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)
    return (torch.relu(y) if relu else y), mean, rstd


def fuse_global(x, rois, g, extra=None, alpha=1.0):
    """HTDRoIHead._fuse_global, htd_roi_head.py:133-141: every RoI tile gets the global feature of its image added,
    image = rois[:, 0]; with `extra` the x_reg + g + alpha * enhanced of htd_bbox_head.py:163,184.
    x (n, C, h, w), rois (n, 5), g (B, C, 1, 1) or (B, C)."""
    B, C = g.shape[:2]
    out = x + g.reshape(B, C)[rois[:, 0].long()].view(-1, C, 1, 1)
    return out if extra is None else out + alpha * extra


def plain_and_fused(x, rois, g):
    """(2n, C, h, w): rows [0, n) = x, rows [n, 2n) = x + g[image of the RoI], the two batches of htd_bbox_head.py:198,201."""
    return torch.cat([x, fuse_global(x, rois, g)], 0)


def ba_fuse(att, lvl, border, edge):
    """AdptRoIExtractor.forward, adaptative_roi_extractor.py:76-91: softmax over the levels of the attention logits att (L, n),
    weighted sum of the per-level tiles lvl[l] (n, C, ph, pw), plus `border` with its interior zeroed AS THE REFERENCE ZEROES IT
    (:88), a slice assignment [edge:-edge, edge:-edge] = 0 on a copy: the slice is empty at edge = 0 and once edge reaches half
    the tile, so the whole border tile is added there."""
    w = att.softmax(0)
    fused = sum(w[l].view(-1, 1, 1, 1) * lvl[l] for l in range(len(lvl)))
    mask = torch.ones(border.shape[2:], dtype=border.dtype)
    mask[edge:-edge, edge:-edge] = 0
    return fused + border * mask


def global_avg_pool(x):
    """nn.AdaptiveAvgPool2d(1): global_context_head.py:372,386, adaptative_roi_extractor.py:38, htd_bbox_head.py:122,188."""
    n, C, h, w = x.shape
    return x.reshape(n, C, h * w).sum(2).div(h * w).view(n, C, 1, 1)


def bn_fold(w, gamma, beta, mean, var, eps=1e-5):
    """Convolution followed by BatchNorm2d on frozen statistics (backbones/resnet.py:640-650: norm_eval keeps every BN in eval mode; the
    `_bn_eval` of the oracle) as ONE convolution: s = gamma / sqrt(var + eps), w' = w * s[co], b' = beta - mean * s.
    -> w' (Co, Ci, kh, kw), b' (Co,), wT (Ci, taps, Co) with wT[ci][taps - 1 - t][co] = w'[co][ci][t], t = r * kw + s: the
    flipped, transposed image the data gradient convolves with."""
    Co, Ci, kh, kw = w.shape
    s = gamma / torch.sqrt(var + eps)
    wf = w * s.view(Co, 1, 1, 1)
    bf = beta - mean * s
    wT = wf.reshape(Co, Ci, kh * kw).flip(2).permute(1, 2, 0)
    return wf, bf, wT


def sgd_momentum(p, g, m, lr, mom, wd, gscale=1.0):
    """One torch.optim.SGD step (momentum, weight decay, no dampening, no Nesterov) on the gradient g * gscale:
    d = g * gscale + wd * p;  m' = mom * m + d;  p' = p - lr * m'.  -> p', m'"""
    d = g * gscale + wd * p
    m2 = mom * m + d
    return p - lr * m2, m2


def delta2bbox_clip(rois, deltas, means, stds, lim_wh=None, keep=None, rows_per_img=None, wh_ratio_clip=16 / 1000):
    """delta2bbox, delta_xywh_bbox_coder.py:171-203, in its order of operations, for (N, 4) deltas: denormalise, clamp dw / dh to
    +-|log(wh_ratio_clip)|, centre / size of the RoI, scale by exp, shift, corners, clamp to [0, W] x [0, H].  lim_wh (B, 2)
    holds [W, H] of the image of row i // rows_per_img (the reference decodes image by image, :199-202 with max_shape = (H, W));
    rows with keep == 0 come back as zeros (the static-shape train path's unused slots)."""
    n = rois.size(0)
    means, stds = deltas.new_tensor(means).view(1, 4), deltas.new_tensor(stds).view(1, 4)
    d = deltas * stds + means
    dx, dy, dw, dh = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    max_ratio = float(np.abs(np.log(wh_ratio_clip)))
    dw, dh = dw.clamp(min=-max_ratio, max=max_ratio), dh.clamp(min=-max_ratio, max=max_ratio)
    px, py = (rois[:, 0] + rois[:, 2]) * 0.5, (rois[:, 1] + rois[:, 3]) * 0.5
    pw, ph = rois[:, 2] - rois[:, 0], rois[:, 3] - rois[:, 1]
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = px + pw * dx, py + ph * dy
    x1, y1, x2, y2 = gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5
    if lim_wh is not None:
        img = torch.arange(n) // int(rows_per_img or max(n, 1))
        W, H = lim_wh.to(x1.dtype)[img, 0], lim_wh.to(x1.dtype)[img, 1]
        x1, x2 = torch.minimum(x1.clamp(min=0), W), torch.minimum(x2.clamp(min=0), W)
        y1, y2 = torch.minimum(y1.clamp(min=0), H), torch.minimum(y2.clamp(min=0), H)
    out = torch.stack([x1, y1, x2, y2], -1)
    if keep is not None:
        out = torch.where(keep.bool().view(n, 1), out, torch.zeros_like(out))
    return out


def roi_targets(boxes, gt_boxes, gt_labels, is_pos, valid, num_classes, means, stds):
    """BBoxHead._get_target_single (bbox_heads/bbox_head.py:85-114) on fixed sample slots, with bbox2delta
    (delta_xywh_bbox_coder.py:100-118) in its order of operations.  Slot i: positive -> its gt label, the encoded target and box
    weight 1; negative -> label num_classes (background), zero target, box weight 0; label weight 1 on every valid slot, 0 on
    the unused ones.  -> labels (N,) int64, label_weights (N,), bbox_targets (N, 4), bbox_weights (N, 4)"""
    n = boxes.size(0)
    pos = is_pos.bool()
    labels = torch.where(pos, gt_labels.long(), torch.full((n, ), int(num_classes), dtype=torch.int64))
    lw = valid.bool().to(boxes.dtype)
    p, g = boxes[pos], gt_boxes[pos]
    px, py, pw, ph = (p[:, 0] + p[:, 2]) * 0.5, (p[:, 1] + p[:, 3]) * 0.5, p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    gx, gy, gw, gh = (g[:, 0] + g[:, 2]) * 0.5, (g[:, 1] + g[:, 3]) * 0.5, g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    d = torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph)], -1)
    d = (d - boxes.new_tensor(means).view(1, 4)) / boxes.new_tensor(stds).view(1, 4)
    bt = boxes.new_zeros(n, 4)
    bt[pos] = d
    bw = pos.to(boxes.dtype).view(n, 1).expand(n, 4).contiguous()
    return labels, lw, bt, bw


def rel_err(out, ref):
    """The float checks' metric: max |out - ref| / max |ref| (ref in float64); 0 for an empty or all-zero reference that the
    output reproduces exactly."""
    out, ref = out.detach().double().cpu(), ref.detach().double()
    assert out.shape == ref.shape, (tuple(out.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.abs().max())
    diff = float((out - ref).abs().max())
    if scale == 0.0:
        return 0.0 if diff == 0.0 else float('inf')
    return diff / scale


def float_bound(e_cpu, R):
    """F x max(e_cpu, 2^-23), F = max(8, sqrt(R)): e_cpu is the error of the same formula evaluated in fp32 on the CPU, R the
    longest run of terms one thread of the kernel adds sequentially."""
    return max(8.0, float(R) ** 0.5) * max(float(e_cpu), 2.0 ** -23)
