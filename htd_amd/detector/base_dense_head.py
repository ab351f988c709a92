"""BaseDenseHead: what the anchor-based (detector/anchor_heads.py) and the anchor-free (detector/anchor_free_heads.py) dense
heads share.

Reference: dense_heads/base_dense_head.py:22-59 (forward_train), dense_test_mixins.py (simple_test), and the get_bboxes /
_get_bboxes_single pair that anchor_head.py, fcos_head.py, atss_head.py, gfl_head.py, vfnet_head.py and fovea_head.py each
restate.  A head gives `forward`, `loss` and `get_bboxes`; the step plumbing, the cache of constants of the pyramid's map shapes,
the two convolution towers and get_bboxes are written once, here.

The towers of RetinaHead, ATSSHead, GFLHead, AnchorFreeHead / FCOSHead and VFNetHead are built by `_build_towers` (in each head's
own seeded order), initialised by `_init_towers` and run by `_run_towers`; FoveaHead builds its plain towers with the first and
keeps its own forward order.  `_fused_maps_ok` is the one statement of what the fused loss kernels ask of the maps; a head's
`_fused_loss_ok` is its own loss modules' conditions beside one call of it.

`_get_bboxes` is the whole inference path of RetinaHead, FCOSHead, ATSSHead, GFLHead, VFNetHead and FoveaHead: the dispatch, the
reference's per-image loop (`_get_bboxes_single`) and the batched form (`_get_bboxes_batched`: one key launch and one segmented
top-k give every (image, level) cut to nms_pre, one gather, one multiclass NMS over all images).  The decode and the rescale stay
tensor operations applied image by image, and the loop ranks by the launch form of the batched path, so the two agree bit for
bit.  A head contributes its priors (`_bbox_priors`, and `_prior_deps` if they depend on more than the map shapes), its decode
(`_bbox_decode`), `strides`, and -- GFLHead alone -- its own `_keys_and_preds`; a head with a centerness branch passes those maps
as `score_factors`.
"""
import torch
import torch.nn as nn

from .. import mmcv_ops as M
from .bricks import ConvModule, normal_init


def _channels_last(maps):
    """The key kernels read channels_last maps: any other layout (NCHW-contiguous maps) is converted, not refused."""
    return [m if M.nhwc_channel_stride(m) is not None else m.contiguous(memory_format=torch.channels_last) for m in maps]


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

    # ------------------------------------------------------------------ towers
    conv_bias = 'auto'                  # what ConvModule takes when no bias is passed (AnchorFreeHead: a constructor kwarg)
    dcn_on_last_conv = False            # (AnchorFreeHead: a constructor kwarg)

    def _build_towers(self, *names, interleaved=False):
        """self.<name> for every name: a ModuleList of stacked_convs ConvModules, the last one a DCNv2 under dcn_on_last_conv
        (anchor_free_head.py:85-123, retina_head.py:61-84).  A ConvModule draws from the RNG when it is built, so the order is
        part of a seeded head: tower by tower (the anchor-free heads), or `interleaved` layer by layer (the anchor heads)."""
        towers = [nn.ModuleList() for _ in names]
        layers = range(self.stacked_convs)
        for tower, i in ([(t, i) for i in layers for t in towers] if interleaved else [(t, i) for t in towers for i in layers]):
            chn = self.in_channels if i == 0 else self.feat_channels
            dcn = self.dcn_on_last_conv and i == self.stacked_convs - 1
            try:
                tower.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1,
                                        conv_cfg=dict(type='DCNv2') if dcn else self.conv_cfg, norm_cfg=self.norm_cfg,
                                        bias=self.conv_bias))
            except (KeyError, TypeError) as e:
                if not dcn:
                    raise
                raise NotImplementedError(f"dcn_on_last_conv: a ConvModule with conv_cfg=dict(type='DCNv2') does not build "
                                          f'({e})') from e
        for name, tower in zip(names, towers):
            setattr(self, name, tower)

    def _init_towers(self):
        for m in list(self.cls_convs) + list(self.reg_convs):
            if isinstance(m.conv, nn.Conv2d):
                normal_init(m.conv, std=0.01)

    def _run_towers(self, x):
        """One level's map through cls_convs and through reg_convs -> (cls_feat, reg_feat)."""
        if x.dtype != torch.float32:             # a bf16 pyramid: the towers and all box / loss arithmetic stay fp32
            x = x.float()
        cls_feat = reg_feat = x
        for layer in self.cls_convs:
            cls_feat = layer(cls_feat)
        for layer in self.reg_convs:
            reg_feat = layer(reg_feat)
        return cls_feat, reg_feat

    # ------------------------------------------------------------------ the fused losses' rule on the maps
    @staticmethod
    def _fused_maps_ok(*groups):
        """The fused loss kernels of every dense head read fp32 channels_last GPU maps (or channel slices of them) of at most 8
        levels where they are; any other layout, NCHW-contiguous maps included, takes the tensor path."""
        return len(groups[0]) <= 8 and \
            all(t.is_cuda and t.dtype == torch.float32 and M.nhwc_channel_stride(t) is not None for g in groups for t in g)

    # ------------------------------------------------------------------ boxes
    num_anchors = 1                     # predictions per location (AnchorHead: its generator's base anchors)
    use_sigmoid_cls = True              # (AnchorHead: its classification loss's)
    _prior_deps = ()                    # what the priors depend on besides the map shapes, their dtype and the device

    def _bbox_priors(self, featmap_sizes, dtype, device):
        """-> per level the (n_l, k) prior rows that `_bbox_decode` takes, one per prediction."""
        raise NotImplementedError

    def _bbox_decode(self, priors, preds, img_shape):
        """(n, k) prior rows and their (n, 4) regression rows -> (n, 4) boxes clamped to the image."""
        raise NotImplementedError

    def _level_cuts(self, cls_scores, nms_pre):
        """Per level: its number of predictions, how many of them the cut to nms_pre keeps (all when nms_pre <= 0) and its first
        column in the level-concatenated order."""
        Ns = [int(c.shape[2] * c.shape[3]) * self.num_anchors for c in cls_scores]
        ks = [n if nms_pre <= 0 else min(nms_pre, n) for n in Ns]
        return Ns, ks, [sum(Ns[:l]) for l in range(len(Ns))]

    def _device_keys_ok(self, cls_scores, bbox_preds, score_factors):
        """htd_retina_keys and htd_fcos_keys take fp32 GPU maps of at most 8 levels under a sigmoid, htd_fcos_keys with one
        prediction per location; anything else ranks by the tensor operations."""
        return cls_scores[0].is_cuda and len(cls_scores) <= 8 and self.use_sigmoid_cls and \
            all(t.dtype == torch.float32 for t in list(cls_scores) + list(score_factors or [])) and \
            (score_factors is None or self.num_anchors == 1)

    def _keys_and_preds(self, cls_scores, bbox_preds, score_factors, want_keys):
        """-> (B, total) ranking keys, level-major (None unless want_keys: no level is cut), and the (B, total, 4) regression
        rows.  The keys are max_c sigmoid(score) (softmax heads: of the foreground classes' softmax), times sigmoid(score factor)
        where there is one: one launch on the GPU, the reference's tensor operations elsewhere."""
        B, C = cls_scores[0].size(0), self.cls_out_channels
        preds = torch.cat([r.permute(0, 2, 3, 1).reshape(B, -1, 4) for r in bbox_preds], 1)
        if not want_keys:
            return None, preds
        if self._device_keys_ok(cls_scores, bbox_preds, score_factors):
            if score_factors is None:
                return M.retina_keys(_channels_last(cls_scores), self.num_anchors, C), preds
            return M.fcos_keys(_channels_last(cls_scores), _channels_last(score_factors), self.strides), preds
        keys = []
        for lvl, c in enumerate(cls_scores):
            s = c.permute(0, 2, 3, 1).reshape(B, -1, C)
            s = s.sigmoid() if self.use_sigmoid_cls else s.softmax(-1)[..., :-1]
            if score_factors is not None:
                s = s * score_factors[lvl].permute(0, 2, 3, 1).reshape(B, -1, 1).sigmoid()
            keys.append(s.max(dim=-1)[0])
        return torch.cat(keys, 1), preds

    def _get_bboxes(self, cls_scores, bbox_preds, score_factors, img_metas, cfg, rescale, with_nms):
        """-> list (per image) of (dets (k, 5), labels (k,)); with_nms=False: of (boxes, scores[, score factors]).  Sigmoid
        heads on the GPU with fp32 maps and hard NMS take the batched form; everything else the per-image loop."""
        cfg = self.test_cfg if cfg is None else cfg
        maps = [None if g is None else [t.detach() for t in g] for g in (cls_scores, bbox_preds, score_factors)]
        assert all(g is None or len(g) == len(cls_scores) for g in maps)
        dev = cls_scores[0].device
        featmap_sizes = [c.shape[-2:] for c in cls_scores]
        nms_pre = cfg.get('nms_pre', -1)
        Ns = self._level_cuts(cls_scores, nms_pre)[0]
        key = (self._shape_key(featmap_sizes), str(dev), bbox_preds[0].dtype, self._prior_deps)
        priors = self._cached('_prior_cache', 32, key,
                              lambda: torch.cat(self._bbox_priors(featmap_sizes, bbox_preds[0].dtype, dev)))
        assert priors.size(0) == sum(Ns)
        batched = with_nms and self._device_keys_ok(*maps) and all(t.dtype == torch.float32 for g in maps if g for t in g) and \
            cfg.nms.get('type', 'nms') == 'nms' and (nms_pre <= 0 or nms_pre <= M.TOPK_KMAX) and \
            getattr(self, 'batched_get_bboxes', True) and (nms_pre > 0 or max(Ns) <= M.TOPK_KMAX)
        if batched:
            return self._get_bboxes_batched(*maps, priors, img_metas, cfg, rescale)
        return [self._get_bboxes_single(*[g and [t[b:b + 1] for t in g] for g in maps], priors, meta['img_shape'],
                                        meta['scale_factor'], cfg, rescale, with_nms) for b, meta in enumerate(img_metas)]

    def _get_bboxes_single(self, cls_scores, bbox_preds, score_factors, priors, img_shape, scale_factor, cfg, rescale=False,
                           with_nms=True):
        """The reference's _get_bboxes_single, level by level, for one image: its maps as batches of one."""
        from ..core.post_processing import multiclass_nms
        nms_pre = cfg.get('nms_pre', -1)
        Ns, ks, offs = self._level_cuts(cls_scores, nms_pre)
        keys, preds = self._keys_and_preds(cls_scores, bbox_preds, score_factors, ks != Ns)
        mlvl = []
        for lvl, cls_score in enumerate(cls_scores):
            assert cls_score.size()[-2:] == bbox_preds[lvl].size()[-2:]
            at = slice(offs[lvl], offs[lvl] + Ns[lvl])
            scores = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
            rows = [priors[at], preds[0, at], scores.sigmoid() if self.use_sigmoid_cls else scores.softmax(-1)]
            if score_factors is not None:
                rows.append(score_factors[lvl].permute(0, 2, 3, 1).reshape(-1).sigmoid())
            if ks[lvl] < Ns[lvl]:
                # the first nms_pre of the stable descending order (equal keys: lower index first)
                topk_inds = keys[0, at].sort(descending=True, stable=True)[1][:nms_pre]
                rows = [r[topk_inds] for r in rows]
            rows[0] = self._bbox_decode(rows[0], rows[1], img_shape)
            mlvl.append(rows)
        mlvl_bboxes = torch.cat([r[0] for r in mlvl])
        if rescale:
            mlvl_bboxes = mlvl_bboxes / mlvl_bboxes.new_tensor(scale_factor)
        mlvl_scores = torch.cat([r[2] for r in mlvl])
        if self.use_sigmoid_cls:
            mlvl_scores = torch.cat([mlvl_scores, mlvl_scores.new_zeros(mlvl_scores.shape[0], 1)], dim=1)
        mlvl_factors = None if score_factors is None else torch.cat([r[3] for r in mlvl])
        if with_nms:
            return multiclass_nms(mlvl_bboxes, mlvl_scores, cfg.score_thr, cfg.nms, cfg.max_per_img, score_factors=mlvl_factors)
        return (mlvl_bboxes, mlvl_scores) if score_factors is None else (mlvl_bboxes, mlvl_scores, mlvl_factors)

    def _get_bboxes_batched(self, cls_scores, bbox_preds, score_factors, priors, img_metas, cfg, rescale):
        """The whole batch on the GPU: one key launch and one segmented top-k give every (image, level) cut to nms_pre, one
        gather, one multiclass NMS over all images; the decode stays the head's own, image by image, so the result is
        bit-identical to the per-image loop."""
        from ..core.post_processing import multiclass_nms_images
        B, L = cls_scores[0].size(0), len(cls_scores)
        dev = cls_scores[0].device
        C = self.cls_out_channels
        Ns, ks, offs = self._level_cuts(cls_scores, cfg.get('nms_pre', -1))
        total = sum(Ns)
        cut = [l for l in range(L) if ks[l] < Ns[l]]
        keys, preds = self._keys_and_preds(cls_scores, bbox_preds, score_factors, bool(cut))
        pieces = [torch.arange(offs[l], offs[l] + Ns[l], device=dev)[None].expand(B, Ns[l]) for l in range(L)]
        if cut:
            # every (image, level) cut of the call in one segmented top-k; a level that is not cut keeps its predictions in their
            # own order, as the per-image form does
            top_idx, _ = M.segmented_topk(keys, [(b * total + offs[l], Ns[l], ks[l]) for b in range(B) for l in cut])
            top_idx, at = top_idx.view(B, -1), 0
            for l in cut:
                pieces[l] = top_idx[:, at:at + ks[l]] + offs[l]
                at += ks[l]
        gidx = torch.cat(pieces, 1)
        K = gidx.size(1)
        logits = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1, C) for c in cls_scores], 1)
        scores = torch.gather(logits, 1, gidx[..., None].expand(B, K, C)).sigmoid()
        preds = torch.gather(preds, 1, gidx[..., None].expand(B, K, 4))
        factors = None
        if score_factors is not None:
            factors = torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1) for t in score_factors], 1)
            factors = torch.gather(factors, 1, gidx).sigmoid().reshape(B * K)
        boxes = torch.stack([self._bbox_decode(priors[gidx[b]], preds[b], img_metas[b]['img_shape']) for b in range(B)])
        if rescale:
            boxes = torch.stack([boxes[b] / boxes.new_tensor(img_metas[b]['scale_factor']) for b in range(B)])
        scores = torch.cat([scores, scores.new_zeros(B, K, 1)], dim=2)
        img_of = torch.arange(B, device=dev).repeat_interleave(K)
        dets, labels = multiclass_nms_images(boxes.reshape(B * K, 4), scores.reshape(B * K, C + 1), img_of, B, cfg.score_thr,
                                             cfg.nms, cfg.max_per_img, score_factors=factors)
        return list(zip(dets, labels))
