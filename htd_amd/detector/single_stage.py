"""SingleStageDetector, RetinaNet, FCOS, ATSS, GFL, VFNet and FOVEA.

Reference: detectors/single_stage.py:9-149 (extract_feat :52-57, forward_train :68-96, simple_test :98-124),
detectors/retinanet.py:5-17, detectors/fcos.py:5-17, detectors/atss.py:5-17, detectors/gfl.py:5-16, detectors/vfnet.py:5-16, detectors/fovea.py:5-17.  The dense head does the work
(detector/anchor_heads.py, anchor_free_heads.py, vfnet_head.py, fovea_head.py); results of a batch leave the device in one copy (core.bbox.bbox2result_many).
"""
from ..core.bbox import bbox2result_many
from ..registry import DETECTORS, build_backbone, build_head, build_neck
from .two_stage import BaseDetector


@DETECTORS.register_module()
class SingleStageDetector(BaseDetector):
    def __init__(self, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        self.backbone = build_backbone(backbone)
        if neck is not None:
            self.neck = build_neck(neck)
        bbox_head = dict(bbox_head)
        bbox_head.update(train_cfg=train_cfg, test_cfg=test_cfg)
        self.bbox_head = build_head(bbox_head)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.init_weights(pretrained=pretrained)

    with_bbox = True
    with_rpn = False

    def init_weights(self, pretrained=None):
        self.backbone.init_weights(pretrained=pretrained)
        if self.with_neck:
            self.neck.init_weights()
        self.bbox_head.init_weights()

    def forward_dummy(self, img):
        return self.bbox_head(self.extract_feat(img))

    def forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None):
        self._begin_train_step(img)
        x = self.extract_feat(img)
        return self.bbox_head.forward_train(x, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore)

    def simple_test(self, img, img_metas, rescale=False):
        self._drop_step_caches(img)
        x = self.extract_feat(img)
        bbox_list = self.bbox_head.get_bboxes(*self.bbox_head(x), img_metas, rescale=rescale)
        return bbox2result_many([d for d, _ in bbox_list], [l for _, l in bbox_list], self.bbox_head.num_classes)

    def aug_test(self, imgs, img_metas, rescale=False):
        raise NotImplementedError('test-time augmentation of single-stage detectors is not part of this package')


@DETECTORS.register_module()
class RetinaNet(SingleStageDetector):
    """detectors/retinanet.py:5-17."""

    def __init__(self, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__(backbone, neck, bbox_head, train_cfg, test_cfg, pretrained)


@DETECTORS.register_module()
class FCOS(SingleStageDetector):
    """detectors/fcos.py:5-17."""

    def __init__(self, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__(backbone, neck, bbox_head, train_cfg, test_cfg, pretrained)


@DETECTORS.register_module()
class ATSS(SingleStageDetector):
    """detectors/atss.py:5-17."""

    def __init__(self, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__(backbone, neck, bbox_head, train_cfg, test_cfg, pretrained)


@DETECTORS.register_module()
class GFL(SingleStageDetector):
    """detectors/gfl.py:5-16."""

    def __init__(self, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__(backbone, neck, bbox_head, train_cfg, test_cfg, pretrained)


@DETECTORS.register_module()
class VFNet(SingleStageDetector):
    """detectors/vfnet.py:5-16."""

    def __init__(self, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__(backbone, neck, bbox_head, train_cfg, test_cfg, pretrained)


@DETECTORS.register_module()
class FOVEA(SingleStageDetector):
    """detectors/fovea.py:5-17."""

    def __init__(self, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__(backbone, neck, bbox_head, train_cfg, test_cfg, pretrained)
