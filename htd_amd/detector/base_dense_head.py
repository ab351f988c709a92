"""BaseDenseHead: what the anchor-based (detector/anchor_heads.py) and the anchor-free (detector/anchor_free_heads.py) dense
heads share.

Reference: dense_heads/base_dense_head.py:22-59 (forward_train), dense_test_mixins.py (simple_test).  A head gives `forward`,
`loss` and `get_bboxes`; the step plumbing and the cache of constants of the pyramid's map shapes are written once, here, and
so is get_bboxes of the heads that predict one box and one centerness per location (FCOSHead from points and distances, ATSSHead
from anchors and deltas): `_ctr_get_bboxes` with the head's priors and its decode.
"""
import torch
import torch.nn as nn


class BaseDenseHead(nn.Module):
    def forward_train(self, x, img_metas, gt_bboxes, gt_labels=None, gt_bboxes_ignore=None, proposal_cfg=None, **kwargs):
        """base_dense_head.py:22-59."""
        outs = self(x)
        if gt_labels is None:
            losses = self.loss(*outs, gt_bboxes, img_metas, gt_bboxes_ignore=gt_bboxes_ignore)
        else:
            losses = self.loss(*outs, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=gt_bboxes_ignore)
        if proposal_cfg is None:
            return losses
        return losses, self.get_bboxes(*outs, img_metas, cfg=proposal_cfg, **kwargs)

    def simple_test(self, feats, img_metas, rescale=False):
        return self.get_bboxes(*self(feats), img_metas, rescale=rescale)

    def aug_test(self, feats, img_metas, rescale=False):
        raise NotImplementedError('test-time augmentation of dense heads is not part of this package')

    # ------------------------------------------------------------------ constants of the map shapes
    @staticmethod
    def _shape_key(featmap_sizes):
        """Cache key of whatever is computed from the pyramid's map sizes: the (h, w) pairs themselves, never their products --
        a portrait and a landscape batch have the same number of anchors on every level and different anchors."""
        return tuple(tuple(int(v) for v in f) for f in featmap_sizes)

    def _cached(self, name, cap, key, make):
        """self.<name>[key], made by make() on a miss; a cache that has grown past `cap` entries is emptied first."""
        cache = self.__dict__.setdefault(name, {})
        if key not in cache:
            if len(cache) > cap:
                cache.clear()
            cache[key] = make()
        return cache[key]

    # ------------------------------------------------------------------ boxes of a head with a centerness map
    # One prediction per location (the device forms; several anchors per location take the tensor forms) and a centerness map (fcos_head.py:255-401, atss_head.py:316-469).  `strides`: the pyramid's;
    # `mlvl_priors()` -> per level the (n_l, 2 or 4) points or anchors, `flat_priors()` -> the same concatenated (a head caches
    # it); `decode(priors, preds, img_shape)` -> boxes clamped to the image.
    def _ctr_get_bboxes(self, cls_scores, bbox_preds, centernesses, img_metas, cfg, rescale, with_nms, strides, mlvl_priors,
                        flat_priors, decode):
        """-> list (per image) of (dets (k, 5), labels (k,)).  GPU fp32 maps with hard NMS take the batched form; everything
        else the per-image loop."""
        from .. import mmcv_ops as M
        cfg = self.test_cfg if cfg is None else cfg
        assert len(cls_scores) == len(bbox_preds) == len(centernesses)
        nms_pre = cfg.get('nms_pre', -1)
        Ns = [int(c.shape[2] * c.shape[3]) for c in cls_scores]
        maps = list(cls_scores) + list(bbox_preds) + list(centernesses)
        batched = with_nms and cls_scores[0].is_cuda and len(cls_scores) <= 8 and all(t.dtype == torch.float32 for t in maps) and \
            getattr(self, 'num_anchors', 1) == 1 and \
            cfg.nms.get('type', 'nms') == 'nms' and (nms_pre <= 0 or nms_pre <= M.TOPK_KMAX) and \
            getattr(self, 'batched_get_bboxes', True) and (nms_pre > 0 or max(Ns) <= M.TOPK_KMAX)
        if batched:
            return self._ctr_bboxes_batched(cls_scores, bbox_preds, centernesses, flat_priors(), decode, strides, img_metas, cfg,
                                            rescale)
        priors = mlvl_priors()
        out = []
        for b, meta in enumerate(img_metas):
            out.append(self._ctr_bboxes_single([c[b].detach() for c in cls_scores], [r[b].detach() for r in bbox_preds],
                                               [t[b].detach() for t in centernesses], priors, decode, strides, meta['img_shape'],
                                               meta['scale_factor'], cfg, rescale, with_nms))
        return out

    def _ctr_level_keys(self, cls_score_list, centerness_list, strides):
        """per level (n_l,) max_c sigmoid(score) * sigmoid(centerness): htd_fcos_keys on the GPU (the same launch form as the
        batched path, so the two rank identically), the reference's tensor operations elsewhere."""
        from .. import mmcv_ops as M
        if cls_score_list[0].is_cuda and cls_score_list[0].dtype == torch.float32 and len(cls_score_list) <= 8 and \
                getattr(self, 'num_anchors', 1) == 1:
            keys = M.fcos_keys([c[None] for c in cls_score_list], [t[None] for t in centerness_list], strides)[0]
            return list(keys.split([int(c.shape[1] * c.shape[2]) for c in cls_score_list]))
        out = []
        for c, t in zip(cls_score_list, centerness_list):
            s = c.permute(1, 2, 0).reshape(-1, self.cls_out_channels).sigmoid()
            out.append((s * t.permute(1, 2, 0).reshape(-1).sigmoid()[:, None]).max(dim=1)[0])
        return out

    def _ctr_bboxes_single(self, cls_scores, bbox_preds, centernesses, mlvl_priors, decode, strides, img_shape, scale_factor, cfg,
                           rescale=False, with_nms=True):
        """fcos_head.py:315-401 / atss_head.py:379-469 for one image."""
        from ..core.post_processing import multiclass_nms
        cfg = self.test_cfg if cfg is None else cfg
        assert len(cls_scores) == len(bbox_preds) == len(mlvl_priors)
        nms_pre = cfg.get('nms_pre', -1)
        keys = self._ctr_level_keys(cls_scores, centernesses, strides) \
            if nms_pre > 0 and any(p.size(0) > nms_pre for p in mlvl_priors) else None
        mlvl_bboxes, mlvl_scores, mlvl_centerness = [], [], []
        for lvl, (cls_score, bbox_pred, centerness, priors) in enumerate(zip(cls_scores, bbox_preds, centernesses, mlvl_priors)):
            assert cls_score.size()[-2:] == bbox_pred.size()[-2:]
            scores = cls_score.permute(1, 2, 0).reshape(-1, self.cls_out_channels).sigmoid()
            centerness = centerness.permute(1, 2, 0).reshape(-1).sigmoid()
            bbox_pred = bbox_pred.permute(1, 2, 0).reshape(-1, 4)
            if nms_pre > 0 and scores.shape[0] > nms_pre:
                # the first nms_pre of the stable descending order (equal keys: lower location index first)
                topk_inds = keys[lvl].sort(descending=True, stable=True)[1][:nms_pre]
                priors, bbox_pred = priors[topk_inds, :], bbox_pred[topk_inds, :]
                scores, centerness = scores[topk_inds, :], centerness[topk_inds]
            mlvl_bboxes.append(decode(priors, bbox_pred, img_shape))
            mlvl_scores.append(scores)
            mlvl_centerness.append(centerness)
        mlvl_bboxes = torch.cat(mlvl_bboxes)
        if rescale:
            mlvl_bboxes = mlvl_bboxes / mlvl_bboxes.new_tensor(scale_factor)
        mlvl_scores = torch.cat(mlvl_scores)
        mlvl_scores = torch.cat([mlvl_scores, mlvl_scores.new_zeros(mlvl_scores.shape[0], 1)], dim=1)
        mlvl_centerness = torch.cat(mlvl_centerness)
        if with_nms:
            return multiclass_nms(mlvl_bboxes, mlvl_scores, cfg.score_thr, cfg.nms, cfg.max_per_img, score_factors=mlvl_centerness)
        return mlvl_bboxes, mlvl_scores, mlvl_centerness

    def _ctr_bboxes_batched(self, cls_scores, bbox_preds, centernesses, priors, decode, strides, img_metas, cfg, rescale):
        """The whole batch on the GPU: one key launch (htd_fcos_keys) and one segmented top-k give every (image, level) cut to
        nms_pre, one gather, one multiclass NMS over all images with the centerness as score factor; the decode stays the
        head's own, image by image, so the result is bit-identical to the per-image loop."""
        from .. import mmcv_ops as M
        from ..core.post_processing import multiclass_nms_images
        B, L = cls_scores[0].size(0), len(cls_scores)
        dev = cls_scores[0].device
        C = self.cls_out_channels
        nms_pre = cfg.get('nms_pre', -1)
        Ns = [int(c.shape[2] * c.shape[3]) for c in cls_scores]
        ks = [n if nms_pre <= 0 else min(nms_pre, n) for n in Ns]
        offs = [sum(Ns[:l]) for l in range(L)]
        total = sum(Ns)
        cls_scores = [c.detach() for c in cls_scores]
        centernesses = [t.detach() for t in centernesses]
        cut = [l for l in range(L) if ks[l] < Ns[l]]
        pieces = [torch.arange(offs[l], offs[l] + Ns[l], device=dev)[None].expand(B, Ns[l]) for l in range(L)]
        if cut:
            # every (image, level) cut of the call in one key launch and one segmented top-k; a level that is not cut keeps its
            # locations in their own order, as the per-image form does
            keys = M.fcos_keys(cls_scores, centernesses, strides)                     # (B, total)
            top_idx, _ = M.segmented_topk(keys, [(b * total + offs[l], Ns[l], ks[l]) for b in range(B) for l in cut])
            top_idx, at = top_idx.view(B, -1), 0
            for l in cut:
                pieces[l] = top_idx[:, at:at + ks[l]] + offs[l]
                at += ks[l]
        gidx = torch.cat(pieces, 1)
        K = gidx.size(1)
        logits = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1, C) for c in cls_scores], 1)
        preds = torch.cat([r.detach().permute(0, 2, 3, 1).reshape(B, -1, 4) for r in bbox_preds], 1)
        ctrs = torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1) for t in centernesses], 1)
        scores = torch.gather(logits, 1, gidx[..., None].expand(B, K, C)).sigmoid()
        preds = torch.gather(preds, 1, gidx[..., None].expand(B, K, 4))
        ctrs = torch.gather(ctrs, 1, gidx).sigmoid()
        boxes = torch.stack([decode(priors[gidx[b]], preds[b], img_metas[b]['img_shape']) for b in range(B)])
        if rescale:
            boxes = torch.stack([boxes[b] / boxes.new_tensor(img_metas[b]['scale_factor']) for b in range(B)])
        scores = torch.cat([scores, scores.new_zeros(B, K, 1)], dim=2)
        img_of = torch.arange(B, device=dev).repeat_interleave(K)
        dets, labels = multiclass_nms_images(boxes.reshape(B * K, 4), scores.reshape(B * K, C + 1), img_of, B, cfg.score_thr,
                                             cfg.nms, cfg.max_per_img, score_factors=ctrs.reshape(B * K))
        return list(zip(dets, labels))
