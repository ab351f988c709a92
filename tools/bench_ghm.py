#!/usr/bin/env python3
"""Cost of the GHM losses (RetinaNet with GHMC + GHMR), four tables:

  kernel   htd_ghm_head_loss on the five levels of a B = 4 1344 x 800 batch (4 x 201 600 anchors x 80 classes): its three launches
           one by one (htd_ghm_head_loss_launches) and together, beside the HBM floor of their mandatory traffic -- the logits read
           by the histogram pass; read again and their gradient written by the loss pass -- at the rate a float4 copy of the same
           size reaches in this process, beside a plain read pass (a sum) of the logits, and beside htd_retina_loss on the same maps
  matrix   htd_ghmc_loss on the same 806 400 x 80 logits as one matrix, beside htd_sigmoid_focal_loss
  head     RetinaHead.loss forward + backward with GHMC + GHMR on the same maps: the fused path against the tensor path
           (fused_loss = False), legs alternated, and the host reads of each
  step     the RetinaNet-GHM R50 fp32 B = 4 1333 x 800 synthetic train step with the fused loss and with the tensor-path loss,
           beside the focal RetinaNet step, one process, legs alternated step by step

Warm-up first, device events around every timed call, medians.  One JSON line per table.  A library built with
HTD_EXTRA_HIPCC=-DHTD_GHM_HIST_PLAIN and selected by HTD_AMD_LIB times the per-element form of the histogram (one LDS atomic per
element instead of one per distinct bin of a wavefront).
usage: bench_ghm.py [kernel] [matrix] [head] [step] [--steps K] [--warmup W] [--reps R] [--batch B]"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_dense as D  # noqa: E402
from bench_dense import SIZES, alternated, capi  # noqa: E402


def head_and_inputs(dev, batch, ghm=True):
    from htd_amd.configs import retinanet_config, retinanet_ghm_config
    from htd_amd.runner import synthetic_batch
    head, data = D.head_from_config(retinanet_ghm_config if ghm else retinanet_config, dev), synthetic_batch(batch, device=dev, seed=0)
    # logits of a freshly initialised head (prior 0.01: bias -4.6) with some spread, so most elements fall into bin 0
    return (head, data, *D.seeded_maps(((720, lambda t, l: t - 4.0), (36, lambda t, l: 0.3 * t)), batch, dev))


def bench_kernel(dev, reps, warmup, batch):
    from htd_amd import mmcv_ops as M
    from htd_amd.core.bbox import batched_max_iou_assign, pad_gt_batch
    head, data, cls, reg = head_and_inputs(dev, batch)
    flat_anchors, inside = head._anchors_inside([c.shape[-2:] for c in cls], data['img_metas'], dev)
    gts, gt_valid, labels = pad_gt_batch(data['gt_bboxes'], data['gt_labels'])
    assigned, _ = batched_max_iou_assign(head.assigner, flat_anchors, inside, gts, gt_valid)
    num_pos, avg = M.retina_avg_factor(assigned)
    B, A = assigned.shape
    L = len(cls)
    ct, cs, pix = M._level_tables(cls, 'bench_ghm')
    rt, rs, _ = M._level_tables(reg, 'bench_ghm')
    gcls, greg = [torch.empty_like(c) for c in cls], [torch.empty_like(r) for r in reg]
    gct, _, _ = M._level_tables(gcls, 'bench_ghm')
    grt, _, _ = M._level_tables(greg, 'bench_ghm')
    partial = torch.empty(capi.lib().htd_focal_loss_partial_rows(), 2, device=dev)
    means, stds = (ctypes.c_float * 4)(0, 0, 0, 0), (ctypes.c_float * 4)(1, 1, 1, 1)
    stream = capi.current_stream_ptr()
    lc, lb = head.loss_cls, head.loss_bbox
    ws = M.ghm_workspace(L, dev)

    def ghm(launches):
        def run():
            capi.call('htd_ghm_head_loss_launches', ct, cs, rt, rs, pix, L, B, 9, 80, capi.ptr(flat_anchors), capi.ptr(gts),
                      capi.ptr(labels), capi.ptr(assigned), A, gts.size(1), means, stds, capi.ptr(lc.edges), lc.bins,
                      float(lc.momentum), capi.ptr(lc.acc_sum), capi.ptr(lb.edges), lb.bins, float(lb.momentum),
                      capi.ptr(lb.acc_sum), float(lb.mu), 1.0, 10.0, capi.ptr(ws), capi.ptr(partial), gct, grt, launches, stream)
        return run

    def focal():
        capi.call('htd_retina_loss', ct, cs, rt, rs, pix, L, B, 9, 80, capi.ptr(flat_anchors), capi.ptr(gts), capi.ptr(labels),
                  capi.ptr(assigned), A, gts.size(1), means, stds, 2.0, 0.25, -1.0, 1, 0.0, capi.ptr(avg), 1.0, 1.0,
                  capi.ptr(partial), gct, grt, stream)
    x = torch.cat([c.permute(0, 2, 3, 1).reshape(-1) for c in cls]).contiguous()
    y = torch.empty_like(x)
    legs = dict(histogram=ghm(1), weights=ghm(2), loss=ghm(4), htd_ghm_head_loss=ghm(7), htd_retina_loss=focal,
                float4_copy=lambda: y.copy_(x), plain_read=lambda: x.sum())
    ghm(7)()
    counts = M.ghm_workspace_views(ws)[0][0, 0, :lc.bins].tolist()
    out = dict(table='kernel', batch=B, anchors=A, classes=80, positives=int(num_pos.sum()), logits_MB=round(x.numel() * 4 / 1e6, 1),
               share_of_bin0_level0=round(counts[0] / max(sum(counts), 1), 3), lib=os.path.basename(capi.LIB_PATH))
    out.update(alternated(legs, reps, warmup))
    copy_tbs = 2 * x.numel() * 4 / out['float4_copy']['median_us'] / 1e6
    reg_bytes, as_bytes = B * A * 4 * 4, B * A * 8
    floor_hist = (x.numel() * 4 + as_bytes) / copy_tbs / 1e6
    floor_loss = (2 * x.numel() * 4 + 2 * reg_bytes + as_bytes) / copy_tbs / 1e6
    out.update(copy_TBs=round(copy_tbs, 2), hbm_floor_us=dict(histogram=round(floor_hist, 1), loss=round(floor_loss, 1)),
               fraction_of_floor=dict(histogram=round(floor_hist / out['histogram']['median_us'], 3),
                                      loss=round(floor_loss / out['loss']['median_us'], 3),
                                      whole=round((floor_hist + floor_loss) / out['htd_ghm_head_loss']['median_us'], 3),
                                      htd_retina_loss=round(floor_loss / out['htd_retina_loss']['median_us'], 3)),
               histogram_over_plain_read=round(out['histogram']['median_us'] / out['plain_read']['median_us'], 2))
    return out


def bench_matrix(dev, reps, warmup, batch):
    from htd_amd import mmcv_ops as M
    from htd_amd.detector.losses import GHMC
    g = torch.Generator().manual_seed(0)
    N = batch * 9 * sum(h * w for h, w in SIZES)
    x = (torch.randn(N, 80, generator=g) - 4.0).to(dev)
    lab = torch.full((N, ), 80, dtype=torch.int64, device=dev)
    lab[::97] = 3
    w = torch.ones(N, device=dev)
    mod = GHMC(bins=30, momentum=0.75).to(dev)
    gx = torch.empty_like(x)
    ws = M.ghm_workspace(1, dev)
    p2 = torch.empty(capi.lib().htd_focal_loss_partial_rows(), 2, device=dev)
    p1 = torch.empty(capi.lib().htd_focal_loss_partial_rows(), device=dev)
    stream = capi.current_stream_ptr()

    def ghmc():
        capi.call('htd_ghmc_loss', capi.ptr(x), capi.ptr(lab), capi.ptr(w), N, 80, capi.ptr(mod.edges), 30, 0.75, capi.ptr(mod.acc_sum),
                  1.0, capi.ptr(ws), capi.ptr(p2), capi.ptr(gx), stream)

    def focal():
        capi.call('htd_sigmoid_focal_loss', capi.ptr(x), capi.ptr(lab), capi.ptr(w), N, 80, 2.0, 0.25, None, capi.ptr(p1), capi.ptr(gx),
                  stream)
    out = dict(table='matrix', rows=N, classes=80)
    out.update(alternated(dict(htd_ghmc_loss=ghmc, htd_sigmoid_focal_loss=focal), reps, warmup))
    return out


class HostReads:
    """Counts .item() / .tolist() / bool() / float() / int() of tensors while active."""
    NAMES = ('item', 'tolist', '__bool__', '__float__', '__int__')

    def __enter__(self):
        self.n, self.real = 0, {k: getattr(torch.Tensor, k) for k in self.NAMES}
        for k, fn in self.real.items():
            def counted(t, *a, _fn=fn, **kw):
                self.n += 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, counted)
        return self

    def __exit__(self, *exc):
        for k, fn in self.real.items():
            setattr(torch.Tensor, k, fn)


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg = head_and_inputs(dev, batch)

    def run_loss():
        c, r = [t.detach().requires_grad_() for t in cls], [t.detach().requires_grad_() for t in reg]
        losses = head.loss(c, r, data['gt_bboxes'], data['gt_labels'], data['img_metas'])
        (sum(losses['loss_cls']) + sum(losses['loss_bbox'])).backward()

    def host_reads(out, step):
        for name, fused in (('fused', True), ('tensor_path', False)):
            with HostReads() as hr:
                step(fused)()
            out[name]['host_reads'] = hr.n
    return D.head_table(head, run_loss, reps, warmup, after=host_reads, batch=batch, anchors=9 * sum(h * w for h, w in SIZES))


def bench_step(dev, steps, warmup, batch):
    return D.step_table(dev, 'retinanet_ghm_r50_fpn', (('ghm_fused', 'retinanet_ghm', True), ('ghm_tensor_path', 'retinanet_ghm', False),
                                                       ('focal_fused', 'retinanet', True)),
                        (('ghm_fused', 'ghm_tensor_path'), ), steps, warmup, batch)


if __name__ == '__main__':
    D.main('bench_ghm.py', dict(kernel=(bench_kernel, D.KERNEL), matrix=(bench_matrix, D.KERNEL), head=(bench_head, D.HEAD),
                                step=(bench_step, D.STEP)))
