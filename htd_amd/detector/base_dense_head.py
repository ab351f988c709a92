"""BaseDenseHead: what the anchor-based (detector/anchor_heads.py) and the anchor-free (detector/anchor_free_heads.py) dense
heads share.

Reference: dense_heads/base_dense_head.py:22-59 (forward_train), dense_test_mixins.py (simple_test).  A head gives `forward`,
`loss` and `get_bboxes`; the step plumbing and the cache of constants of the pyramid's map shapes are written once, here.
"""
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
