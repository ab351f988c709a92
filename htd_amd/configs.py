"""The HTD model / train / test configuration as data (configs/htd/htd_resnet50_1x.py:5-168 and its
R101 / R101-DCN siblings htd_resnet101_2x.py, htd_resnet101_dcn_2x_mstrain.py:139-150), produced
programmatically so the package carries no config files of its own.  The reference's config *files*
load unchanged through `htd_amd.Config.fromfile` (same `type=` names and kwargs).

The two baselines HTD is measured against come the same way: faster_rcnn_config (configs/faster_rcnn/
faster_rcnn_r50_fpn_1x_coco.py) and cascade_rcnn_config (configs/cascade_rcnn/cascade_rcnn_r50_fpn_1x_coco.py), with
their `_base_` chains merged, and so do the single-stage baselines retinanet_config (configs/retinanet/
retinanet_r50_fpn_1x_coco.py), its GHM variant retinanet_ghm_config (configs/ghm/retinanet_ghm_r50_fpn_1x_coco.py) and
fcos_config (the two configs/fcos/fcos_*_r50_caffe_fpn_gn-head_4x4_1x_coco.py), atss_config (configs/atss/
atss_r50_fpn_1x_coco.py and its R101 sibling), gfl_config (configs/gfl/gfl_r50_fpn_1x_coco.py and the mstrain 2x schedule
of gfl_r101_fpn_mstrain_2x_coco.py) and vfnet_config (configs/vfnet/vfnet_r50_fpn_1x_coco.py and the mstrain 2x schedule of
vfnet_r101_fpn_mstrain_2x_coco.py) and fovea_config (the eight configs/foveabox/fovea_*_4x4_*_coco.py).
"""
import copy

from .registry import ConfigDict


def _bbox_head(kind, stds, **extra):
    d = dict(type=kind, in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=80,
             bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.], target_stds=stds),
             reg_class_agnostic=True,
             loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
             loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    d.update(extra)
    return d


def _rcnn(thr):
    return dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=thr, neg_iou_thr=thr, min_pos_iou=thr,
                              match_low_quality=False, ignore_iof_thr=-1),
                sampler=dict(type='RandomSampler', num=512, pos_fraction=0.25, neg_pos_ub=-1,
                             add_gt_as_proposals=True),
                pos_weight=-1, debug=False)


def htd_model(depth=50, dcn=False, resnext=False):
    backbone = dict(type='ResNet', depth=depth, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                    norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch')
    if resnext:                                    # htd_resnetx101_dcn_2x_mstrain.py:138-150 (64x4d)
        backbone.update(type='ResNeXt', groups=64, base_width=4)
    if dcn:
        backbone.update(dcn=dict(type='DCN', deform_groups=1, fallback_on_stride=False),
                        stage_with_dcn=(False, True, True, True))
    roi_layer = dict(type='RoIAlign', output_size=7, sampling_ratio=0)
    return dict(
        type='FasterRCNN', pretrained=None, backbone=backbone,
        neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5),
        rpn_head=dict(type='RPNHead', in_channels=256, feat_channels=256,
                      anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0],
                                            strides=[4, 8, 16, 32, 64]),
                      bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0],
                                      target_stds=[1.0, 1.0, 1.0, 1.0]),
                      loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                      loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)),
        roi_head=dict(type='HTDRoIHead', num_stages=2, with_global=True, stage_loss_weights=[1, 0.5],
                      bbox_roi_extractor=[
                          dict(type='SingleRoIExtractor', roi_layer=dict(roi_layer), out_channels=256,
                               featmap_strides=[4, 8, 16, 32]),
                          dict(type='AdptRoIExtractor', edge=1, roi_layer=dict(roi_layer), out_channels=256,
                               featmap_strides=[4, 8, 16, 32])],
                      bbox_head=[_bbox_head('Shared2FCBBoxHead', [0.1, 0.1, 0.2, 0.2]),
                                 _bbox_head('HTDBBoxHead', [0.05, 0.05, 0.1, 0.1], relpace=False, edge=1)]))


def htd_train_cfg():
    return dict(
        rpn=dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3,
                               match_low_quality=True, ignore_iof_thr=-1),
                 sampler=dict(type='RandomSampler', num=256, pos_fraction=0.5, neg_pos_ub=-1,
                              add_gt_as_proposals=False),
                 allowed_border=0, pos_weight=-1, debug=False),
        rpn_proposal=dict(nms_across_levels=False, nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.7,
                          min_bbox_size=0),
        rcnn=[_rcnn(0.5), _rcnn(0.6)])


def htd_test_cfg(soft_nms=False):
    nms = dict(type='soft_nms', iou_thr=0.5, min_score=0.05) if soft_nms else dict(type='nms', iou_threshold=0.5)
    return dict(rpn=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=1000, nms_thr=0.7,
                         min_bbox_size=0),
                rcnn=dict(score_thr=0.05, nms=nms, max_per_img=100))


def _baseline_model(kind, depth, roi_head, rpn_loss_bbox):
    model = htd_model(depth)
    model.update(type=kind, pretrained=f'torchvision://resnet{depth}', roi_head=roi_head)
    model['rpn_head']['loss_bbox'] = rpn_loss_bbox
    return model


def _single_extractor():
    return dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
                featmap_strides=[4, 8, 16, 32])


def faster_rcnn_model(depth=50):
    """configs/_base_/models/faster_rcnn_r50_fpn.py: L1 regression in the RPN and in a class-specific Shared2FCBBoxHead."""
    l1 = dict(type='L1Loss', loss_weight=1.0)
    head = _bbox_head('Shared2FCBBoxHead', [0.1, 0.1, 0.2, 0.2], reg_class_agnostic=False, loss_bbox=dict(l1))
    return _baseline_model('FasterRCNN', depth, dict(type='StandardRoIHead', bbox_roi_extractor=_single_extractor(),
                                                     bbox_head=head), dict(l1))


def cascade_rcnn_model(depth=50):
    """configs/_base_/models/cascade_rcnn_r50_fpn.py: three class-agnostic stages with tightening target_stds."""
    heads = [_bbox_head('Shared2FCBBoxHead', stds) for stds in ([0.1, 0.1, 0.2, 0.2], [0.05, 0.05, 0.1, 0.1],
                                                                [0.033, 0.033, 0.067, 0.067])]
    return _baseline_model('CascadeRCNN', depth,
                           dict(type='CascadeRoIHead', num_stages=3, stage_loss_weights=[1, 0.5, 0.25],
                                bbox_roi_extractor=_single_extractor(), bbox_head=heads),
                           dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0))


def _baseline_config(model, train_cfg, depth):
    if depth not in (50, 101):
        raise ValueError(f'baseline configs exist for ResNet-50 and ResNet-101, got depth={depth!r}')
    return ConfigDict(
        model=model, train_cfg=train_cfg, test_cfg=htd_test_cfg(False), data=htd_data(50),
        evaluation=dict(interval=1, metric='bbox'),
        optimizer=dict(type='SGD', lr=0.02, momentum=0.9, weight_decay=0.0001), optimizer_config=dict(grad_clip=None),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=0.001, step=[8, 11]), total_epochs=12)


def faster_rcnn_config(depth=50):
    """faster_rcnn_r{depth}_fpn_1x_coco: the RPN ignores no border anchors (allowed_border=-1) and hands on 1000 proposals."""
    train_cfg = htd_train_cfg()
    train_cfg['rpn']['allowed_border'] = -1
    train_cfg['rpn_proposal'].update(nms_post=1000, max_num=1000)
    train_cfg['rcnn'] = _rcnn(0.5)
    return _baseline_config(faster_rcnn_model(depth), train_cfg, depth)


def cascade_rcnn_config(depth=50):
    """cascade_rcnn_r{depth}_fpn_1x_coco: IoU thresholds 0.5 / 0.6 / 0.7 over the three stages."""
    train_cfg = htd_train_cfg()
    train_cfg['rcnn'] = [_rcnn(0.5), _rcnn(0.6), _rcnn(0.7)]
    return _baseline_config(cascade_rcnn_model(depth), train_cfg, depth)


def faster_rcnn_gn_ws_model(depth=50):
    """configs/gn+ws/faster_rcnn_r50_fpn_gn_ws-all_1x_coco.py over faster_rcnn_model: weight-standardised convolutions and
    GroupNorm(32) in the backbone, the neck and a Shared4Conv1FCBBoxHead."""
    conv_cfg, norm_cfg = dict(type='ConvWS'), dict(type='GN', num_groups=32, requires_grad=True)
    model = faster_rcnn_model(depth)
    model['pretrained'] = f'open-mmlab://jhu/resnet{depth}_gn_ws'
    model['backbone'].update(conv_cfg=dict(conv_cfg), norm_cfg=dict(norm_cfg))
    model['neck'].update(conv_cfg=dict(conv_cfg), norm_cfg=dict(norm_cfg))
    model['roi_head']['bbox_head'].update(type='Shared4Conv1FCBBoxHead', conv_out_channels=256, conv_cfg=dict(conv_cfg),
                                          norm_cfg=dict(norm_cfg))
    return model


def faster_rcnn_gn_ws_config(depth=50):
    """faster_rcnn_r{depth}_fpn_gn_ws-all_1x_coco: faster_rcnn_config with the GN+WS model."""
    cfg = faster_rcnn_config(depth)
    cfg.model = ConfigDict(faster_rcnn_gn_ws_model(depth))
    return cfg


def retinanet_model(depth=50):
    """configs/_base_/models/retinanet_r50_fpn.py: P3-P7 (P6, P7 by stride-2 convolutions from C5), nine anchors per position,
    focal loss on 80 sigmoid classes and L1 on the deltas."""
    model = htd_model(depth)
    return dict(
        type='RetinaNet', pretrained=f'torchvision://resnet{depth}', backbone=model['backbone'],
        neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1, add_extra_convs='on_input',
                  num_outs=5),
        bbox_head=dict(type='RetinaHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
                       anchor_generator=dict(type='AnchorGenerator', octave_base_scale=4, scales_per_octave=3,
                                             ratios=[0.5, 1.0, 2.0], strides=[8, 16, 32, 64, 128]),
                       bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0],
                                       target_stds=[1.0, 1.0, 1.0, 1.0]),
                       loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                       loss_bbox=dict(type='L1Loss', loss_weight=1.0)))


def retinanet_config(depth=50):
    """retinanet_r{depth}_fpn_1x_coco: every anchor is a sample (no sampler), lr 0.01."""
    cfg = _baseline_config(
        retinanet_model(depth),
        dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1),
             allowed_border=-1, pos_weight=-1, debug=False), depth)
    cfg.test_cfg = ConfigDict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5),
                              max_per_img=100)
    cfg.optimizer.lr = 0.01
    return cfg


def retinanet_ghm_model(depth=50):
    """configs/ghm/retinanet_ghm_r{depth}_fpn_1x_coco.py: retinanet_model with GHMC (30 bins, momentum 0.75) in place of the focal
    loss and GHMR (mu 0.02, 10 bins, momentum 0.7, weight 10) in place of L1."""
    model = retinanet_model(depth)
    model['bbox_head'].update(
        loss_cls=dict(type='GHMC', bins=30, momentum=0.75, use_sigmoid=True, loss_weight=1.0),
        loss_bbox=dict(type='GHMR', mu=0.02, bins=10, momentum=0.7, loss_weight=10.0))
    return model


def retinanet_ghm_config(depth=50):
    """retinanet_ghm_r{depth}_fpn_1x_coco: retinanet_config with the GHM model and gradients clipped at norm 35.
    (`python -m htd_amd.train` refuses grad_clip: apis.check_supported; Trainer.train_step and `python -m htd_amd.test` take the
    config as it is.)"""
    cfg = retinanet_config(depth)
    cfg.model = ConfigDict(retinanet_ghm_model(depth))
    cfg.optimizer_config = ConfigDict(grad_clip=dict(max_norm=35, norm_type=2))
    return cfg


FCOS_VARIANTS = ('gn-head', 'center-normbbox-centeronreg-giou')


def fcos_model(depth=50, variant='gn-head'):
    """configs/fcos/fcos_r50_caffe_fpn_gn-head_4x4_1x_coco.py: a caffe-style backbone with frozen BN, P3-P7 with P6 / P7 by
    convolutions on the ReLU of the output P5, a GroupNorm(32) FCOSHead with IoULoss.  variant 'center-normbbox-centeronreg-giou'
    (configs/fcos/fcos_center-normbbox-centeronreg-giou_r50_caffe_fpn_gn-head_4x4_1x_coco.py): centre sampling, stride-normalised
    distances, the centerness on the regression tower, conv biases and GIoULoss."""
    if variant not in FCOS_VARIANTS:
        raise ValueError(f'fcos_model: variant must be one of {FCOS_VARIANTS}, got {variant!r}')
    tricks = variant != 'gn-head'
    head = dict(type='FCOSHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
                strides=[8, 16, 32, 64, 128],
                loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                loss_bbox=dict(type='GIoULoss' if tricks else 'IoULoss', loss_weight=1.0),
                loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0))
    if tricks:
        head.update(norm_on_bbox=True, centerness_on_reg=True, dcn_on_last_conv=False, center_sampling=True, conv_bias=True)
    return dict(
        type='FCOS', pretrained=f"open-mmlab://{'detectron2' if tricks else 'detectron'}/resnet{depth}_caffe",
        backbone=dict(type='ResNet', depth=depth, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                      norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True, style='caffe'),
        neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1, add_extra_convs=True,
                  extra_convs_on_inputs=False, num_outs=5, relu_before_extra_convs=True),
        bbox_head=head)


def fcos_config(depth=50, variant='gn-head'):
    """The two FCOS configs of fcos_model, 4 images per GPU, lr 0.01 with doubled, undecayed biases (paramwise_cfg); the plain
    one clips gradients at norm 35 and warms up at a constant third of the rate, the other warms up linearly without clipping.
    (`python -m htd_amd.train` refuses paramwise_cfg, grad_clip and constant warm-up: apis.check_supported.)"""
    cfg = _baseline_config(
        fcos_model(depth, variant),
        dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1),
             allowed_border=-1, pos_weight=-1, debug=False), depth)
    tricks = variant != 'gn-head'
    cfg.test_cfg = ConfigDict(nms_pre=1000, min_bbox_size=0, score_thr=0.05,
                              nms=dict(type='nms', iou_threshold=0.6 if tricks else 0.5), max_per_img=100)
    cfg.optimizer = ConfigDict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001,
                               paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.))
    cfg.optimizer_config = ConfigDict(grad_clip=None if tricks else dict(max_norm=35, norm_type=2))
    cfg.lr_config = ConfigDict(policy='step', warmup='linear' if tricks else 'constant', warmup_iters=500, warmup_ratio=1.0 / 3,
                               step=[8, 11])
    return cfg


def atss_model(depth=50):
    """configs/atss/atss_r50_fpn_1x_coco.py: P3-P7 with P6 / P7 by convolutions on the output P5, one square anchor of 8 strides
    per location, a GroupNorm(32) ATSSHead with a centerness-weighted GIoULoss of weight 2 on decoded boxes."""
    return dict(
        type='ATSS', pretrained=f'torchvision://resnet{depth}', backbone=htd_model(depth)['backbone'],
        neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1, add_extra_convs='on_output',
                  num_outs=5),
        bbox_head=dict(type='ATSSHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
                       anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                             strides=[8, 16, 32, 64, 128]),
                       bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0],
                                       target_stds=[0.1, 0.1, 0.2, 0.2]),
                       loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                       loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
                       loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)))


def atss_config(depth=50):
    """atss_r{depth}_fpn_1x_coco: ATSSAssigner with the nine nearest anchors per level and gt, every anchor a sample, lr 0.01, no
    gradient clipping, the linear warm-up of schedule_1x: `python -m htd_amd.train` takes it as it is."""
    cfg = _baseline_config(atss_model(depth),
                           dict(assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1, pos_weight=-1, debug=False), depth)
    cfg.test_cfg = ConfigDict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6),
                              max_per_img=100)
    cfg.optimizer.lr = 0.01
    return cfg


def gfl_model(depth=50):
    """configs/gfl/gfl_r50_fpn_1x_coco.py: ATSS's backbone, neck and one-anchor pyramid under a GFLHead -- QualityFocalLoss on the
    joint class / quality score, 17 bins per side (reg_max 16) under DistributionFocalLoss of weight 0.25, GIoULoss of weight 2
    on the integral-decoded boxes."""
    return dict(
        type='GFL', pretrained=f'torchvision://resnet{depth}', backbone=htd_model(depth)['backbone'],
        neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1, add_extra_convs='on_output',
                  num_outs=5),
        bbox_head=dict(type='GFLHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
                       anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                             strides=[8, 16, 32, 64, 128]),
                       loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0),
                       loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25), reg_max=16,
                       loss_bbox=dict(type='GIoULoss', loss_weight=2.0)))


def gfl_config(depth=50, mstrain=False):
    """gfl_r{depth}_fpn_1x_coco, or with mstrain gfl_r{depth}_fpn_mstrain_2x_coco: ATSS's training and test settings and lr 0.01;
    the multi-scale schedule trains 24 epochs with steps at 16 / 22 on a short side drawn from [480, 800] (Resize in `range`
    mode): `python -m htd_amd.train` takes either as it is."""
    cfg = _baseline_config(gfl_model(depth),
                           dict(assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1, pos_weight=-1, debug=False), depth)
    cfg.test_cfg = ConfigDict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6),
                              max_per_img=100)
    cfg.optimizer.lr = 0.01
    if mstrain:
        cfg.lr_config.step = [16, 22]
        cfg.total_epochs = 24
        resize = cfg.data.train.pipeline[2]
        assert resize['type'] == 'Resize'
        cfg.data.train.pipeline[2] = ConfigDict(type='Resize', img_scale=[(1333, 480), (1333, 800)], multiscale_mode='range',
                                                keep_ratio=True)
    return cfg


def vfnet_model(depth=50):
    """configs/vfnet/vfnet_r50_fpn_1x_coco.py: ATSS's backbone, FCOS's neck (P6 / P7 by convolutions on the ReLU of the output
    P5), a VFNetHead of three tower convolutions -- VarifocalLoss on the IoU-aware score, GIoULoss of weight 1.5 on the initial
    and of weight 2 on the refined box, ATSS targets."""
    return dict(
        type='VFNet', pretrained=f'torchvision://resnet{depth}', backbone=htd_model(depth)['backbone'],
        neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1, add_extra_convs=True,
                  extra_convs_on_inputs=False, num_outs=5, relu_before_extra_convs=True),
        bbox_head=dict(type='VFNetHead', num_classes=80, in_channels=256, stacked_convs=3, feat_channels=256,
                       strides=[8, 16, 32, 64, 128], center_sampling=False, dcn_on_last_conv=False, use_atss=True, use_vfl=True,
                       loss_cls=dict(type='VarifocalLoss', use_sigmoid=True, alpha=0.75, gamma=2.0, iou_weighted=True,
                                     loss_weight=1.0),
                       loss_bbox=dict(type='GIoULoss', loss_weight=1.5), loss_bbox_refine=dict(type='GIoULoss', loss_weight=2.0)))


def vfnet_config(depth=50, mstrain=False):
    """vfnet_r{depth}_fpn_1x_coco, or with mstrain vfnet_r{depth}_fpn_mstrain_2x_coco: ATSS's training and test settings, lr 0.01
    with doubled, undecayed biases (paramwise_cfg) and a linear warm-up from a tenth of the rate; the multi-scale schedule trains
    24 epochs with steps at 16 / 22 on a short side drawn from [480, 960] (Resize in `range` mode).
    (`python -m htd_amd.train` refuses paramwise_cfg: apis.check_supported.)"""
    cfg = _baseline_config(vfnet_model(depth),
                           dict(assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1, pos_weight=-1, debug=False), depth)
    cfg.test_cfg = ConfigDict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6),
                              max_per_img=100)
    cfg.optimizer = ConfigDict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001,
                               paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.))
    cfg.lr_config = ConfigDict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=0.1, step=[8, 11])
    if mstrain:
        cfg.lr_config.step = [16, 22]
        cfg.total_epochs = 24
        resize = cfg.data.train.pipeline[2]
        assert resize['type'] == 'Resize'
        cfg.data.train.pipeline[2] = ConfigDict(type='Resize', img_scale=[(1333, 480), (1333, 960)], multiscale_mode='range',
                                                keep_ratio=True)
    return cfg


def fovea_model(depth=50, align=False):
    """configs/foveabox/fovea_r50_fpn_4x4_1x_coco.py: RetinaNet's backbone and neck under a FoveaHead -- focal loss with gamma 1.5
    and alpha 0.4, SmoothL1Loss (beta 0.11) on log distances, scale ranges of two octaves around each level's base edge.  align:
    the fovea_align_*_gn-head configs -- the classification tower behind a FeatureAlign of 4 deformable groups, GroupNorm(32)."""
    head = dict(type='FoveaHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256, strides=[8, 16, 32, 64, 128],
                base_edge_list=[16, 32, 64, 128, 256], scale_ranges=((1, 64), (32, 128), (64, 256), (128, 512), (256, 2048)),
                sigma=0.4, with_deform=bool(align),
                loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=1.50, alpha=0.4, loss_weight=1.0),
                loss_bbox=dict(type='SmoothL1Loss', beta=0.11, loss_weight=1.0))
    if align:
        head['norm_cfg'] = dict(type='GN', num_groups=32, requires_grad=True)
    return dict(
        type='FOVEA', pretrained=f'torchvision://resnet{depth}', backbone=htd_model(depth)['backbone'],
        neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1, num_outs=5,
                  add_extra_convs='on_input'),
        bbox_head=head)


def fovea_config(depth=50, align=False, mstrain=False, schedule='1x'):
    """fovea[_align]_r{depth}_fpn[_gn-head][_mstrain_640-800]_4x4_{schedule}_coco: an empty train_cfg (the head needs no assigner),
    lr 0.01 and the linear warm-up of schedule_1x; '2x' trains 24 epochs with steps at 16 / 22; mstrain (2x only) draws the
    short side from {640, 800} (Resize in `value` mode).  fovea_align_r50_fpn_gn-head_4x4_2x_coco alone clips gradients at norm
    35, as the reference's file does (`python -m htd_amd.train` refuses grad_clip: apis.check_supported)."""
    if schedule not in ('1x', '2x'):
        raise ValueError(f"fovea_config: schedule must be '1x' or '2x', got {schedule!r}")
    if mstrain and schedule != '2x':
        raise ValueError('fovea_config: the multi-scale configs train the 2x schedule')
    cfg = _baseline_config(fovea_model(depth, align), dict(), depth)
    cfg.test_cfg = ConfigDict(nms_pre=1000, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
    cfg.optimizer.lr = 0.01
    if schedule == '2x':
        cfg.lr_config.step = [16, 22]
        cfg.total_epochs = 24
    if align and depth == 50 and schedule == '2x' and not mstrain:
        cfg.optimizer_config = ConfigDict(grad_clip=dict(max_norm=35, norm_type=2))
    if mstrain:
        resize = cfg.data.train.pipeline[2]
        assert resize['type'] == 'Resize'
        cfg.data.train.pipeline[2] = ConfigDict(type='Resize', img_scale=[(1333, 640), (1333, 800)], multiscale_mode='value',
                                                keep_ratio=True)
    return cfg


IMG_NORM_CFG = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def htd_data(depth=50, resnext=False, data_root='data/coco/'):
    """The `data` section: R50 1x trains at (1333, 800); the 2x(-mstrain) configs train at a random scale in
    [(1600, 400), (1600, 1400)]; every config tests at (1333, 800) but the ResNeXt one, at (1600, 800)."""
    if depth == 50 and not resnext:
        train_resize = dict(type='Resize', img_scale=(1333, 800), keep_ratio=True)
    else:
        train_resize = dict(type='Resize', img_scale=[(1600, 400), (1600, 1400)], multiscale_mode='range',
                            keep_ratio=True)
    train_pipeline = [
        dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True), train_resize,
        dict(type='RandomFlip', flip_ratio=0.5), dict(type='Normalize', **IMG_NORM_CFG),
        dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
        dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
    test_pipeline = [
        dict(type='LoadImageFromFile'),
        dict(type='MultiScaleFlipAug', img_scale=(1600, 800) if resnext else (1333, 800), flip=False,
             transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                         dict(type='Normalize', **IMG_NORM_CFG), dict(type='Pad', size_divisor=32),
                         dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]

    def split(name, pipeline):
        return dict(type='CocoDataset', ann_file=data_root + f'annotations/instances_{name}2017.json',
                    img_prefix=data_root + f'{name}2017/', pipeline=copy.deepcopy(pipeline))
    return dict(samples_per_gpu=2, workers_per_gpu=2, train=split('train', train_pipeline),
                val=split('val', test_pipeline), test=split('val', test_pipeline))


def voc0712_data(data_root='data/VOCdevkit/'):
    """configs/_base_/datasets/voc0712.py: train on VOC2007 + VOC2012 trainval (a list ann_file) repeated 3 times,
    test on VOC2007 test, at (1000, 600)."""
    train_pipeline = [
        dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
        dict(type='Resize', img_scale=(1000, 600), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
        dict(type='Normalize', **IMG_NORM_CFG), dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
        dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
    test_pipeline = [
        dict(type='LoadImageFromFile'),
        dict(type='MultiScaleFlipAug', img_scale=(1000, 600), flip=False,
             transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                         dict(type='Normalize', **IMG_NORM_CFG), dict(type='Pad', size_divisor=32),
                         dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]

    def test_split():
        return dict(type='VOCDataset', ann_file=data_root + 'VOC2007/ImageSets/Main/test.txt',
                    img_prefix=data_root + 'VOC2007/', pipeline=copy.deepcopy(test_pipeline))
    return dict(samples_per_gpu=2, workers_per_gpu=2,
                train=dict(type='RepeatDataset', times=3, dataset=dict(
                    type='VOCDataset', ann_file=[data_root + 'VOC2007/ImageSets/Main/trainval.txt',
                                                 data_root + 'VOC2012/ImageSets/Main/trainval.txt'],
                    img_prefix=[data_root + 'VOC2007/', data_root + 'VOC2012/'], pipeline=train_pipeline)),
                val=test_split(), test=test_split())


def htd_config(depth=50, dcn=False, soft_nms=None, resnext=False, dataset='coco'):
    """-> ConfigDict(model=..., train_cfg=..., test_cfg=..., data=..., evaluation=..., optimizer=..., lr_config=...).
    dataset='voc0712': both bbox heads with 20 classes, the voc0712 data section, mAP evaluation every epoch and the
    4-epoch schedule of the reference's VOC configs (lr step at 3)."""
    soft_nms = (depth == 101) if soft_nms is None else soft_nms        # htd_resnet101_2x.py:298
    cfg = ConfigDict(
        model=htd_model(depth, dcn, resnext), train_cfg=htd_train_cfg(), test_cfg=htd_test_cfg(soft_nms),
        data=htd_data(depth, resnext), evaluation=dict(interval=1 if depth == 50 else 24, metric='bbox'),
        optimizer=dict(type='SGD', lr=0.02 if depth == 50 else 0.015, momentum=0.9, weight_decay=0.0001),
        optimizer_config=dict(grad_clip=None),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=0.001,
                       step=[8, 11] if depth == 50 else [16, 22]),
        total_epochs=12 if depth == 50 else 24)
    if dataset == 'voc0712':
        for head in cfg.model.roi_head.bbox_head:
            head.num_classes = 20
        cfg.data = ConfigDict(voc0712_data())
        cfg.evaluation = ConfigDict(interval=1, metric='mAP')
        cfg.lr_config.step = [3]
        cfg.total_epochs = 4
    elif dataset != 'coco':
        raise ValueError(f"htd_config: dataset must be 'coco' or 'voc0712', got {dataset!r}")
    return cfg


def build_htd_detector(depth=50, dcn=False, cfg=None, bf16=False, resnext=False):
    """bf16=True: backbone stages, FPN and the RPN's shared conv run on the bf16 MFMA kernels (fp32 master weights, fp32
    accumulate); the stem, the RoI head and all box / loss arithmetic stay fp32 (BASELINE configs[2] precision map)."""
    from . import detector  # noqa: F401  (registers the components)
    from .registry import build_detector
    cfg = htd_config(depth, dcn, resnext=resnext) if cfg is None else cfg
    # the reference's mixed-precision switch is the config key `fp16 = dict(loss_scale=...)` (mmdet/apis/train.py:97-100,
    # Fp16OptimizerHook); MI355X's 16-bit training type is bf16 (fp32's exponent range: no loss scaling needed), so the key
    # selects this mode and its loss_scale is ignored
    if cfg.get('fp16', None) is not None:
        bf16 = True
    model = build_detector(copy.deepcopy(cfg.model.to_dict()), train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    if bf16:
        import os
        import torch
        if 'HTD_OVERLAP_WGRAD' not in os.environ:
            # weight gradients on a second stream: +2 % on the fp32 step, -6 % on the bf16 one (R101: 33.3 -> 35.4 ms; its
            # hundreds of 10-40 us kernels gain nothing from sharing the chip and pay for the cross-stream waits).  A
            # property of THIS model (runner.Trainer applies it around its steps), not of the process.
            model.overlap_wgrad = False
        model.backbone.compute_dtype = torch.bfloat16
        heads = model.roi_head.bbox_head if getattr(model, 'roi_head', None) is not None else []
        for head in (heads if isinstance(heads, (list, torch.nn.ModuleList)) else [heads]):      # the 12544->1024->1024 FC stacks of every stage
            head.compute_dtype = torch.bfloat16
            for m in getattr(head, 'convs', []):       # and the 3x3 stack of the regression branch (GroupNorm stays fp32)
                m.compute_dtype = torch.bfloat16
    return model


def build_baseline_detector(kind='faster_rcnn', depth=50, cfg=None, bf16=False):
    """kind = 'faster_rcnn' | 'cascade_rcnn' | 'faster_rcnn_gn_ws' | 'fcos' | 'fcos_center' | 'atss' | 'gfl' | 'vfnet' -> the
    detector of faster_rcnn_config / cascade_rcnn_config / faster_rcnn_gn_ws_config / fcos_config (its two variants) /
    atss_config / gfl_config / vfnet_config (or of `cfg`), with the `pretrained` URL of the
    reference's config dropped: weights come from a checkpoint or from init_weights.  bf16 as in build_htd_detector."""
    makers = dict(faster_rcnn=faster_rcnn_config, cascade_rcnn=cascade_rcnn_config, faster_rcnn_gn_ws=faster_rcnn_gn_ws_config,
                  fcos=fcos_config, fcos_center=lambda d: fcos_config(d, 'center-normbbox-centeronreg-giou'), atss=atss_config,
                  gfl=gfl_config, vfnet=vfnet_config)
    if cfg is None:
        if kind not in makers:
            raise ValueError(f'build_baseline_detector: kind must be one of {sorted(makers)}, got {kind!r}')
        cfg = makers[kind](depth)
    cfg = copy.deepcopy(cfg)
    if str(cfg.model.get('pretrained') or '').startswith(('torchvision://', 'open-mmlab://')):
        cfg.model.pretrained = None
    return build_htd_detector(cfg=cfg, bf16=bf16)


def build_retinanet_detector(depth=50, cfg=None, bf16=False):
    """The detector of retinanet_config(depth) (or of `cfg`), built like the two-stage baselines: the `pretrained` URL of the
    reference's config dropped.  The single-stage baseline has a builder of its own: the kinds of build_baseline_detector are
    the two-stage ones."""
    return build_baseline_detector(cfg=retinanet_config(depth) if cfg is None else cfg, bf16=bf16)


def build_retinanet_ghm_detector(depth=50, cfg=None, bf16=False):
    """The detector of retinanet_ghm_config(depth) (or of `cfg`); build_retinanet_detector with that config gives the same."""
    return build_baseline_detector(cfg=retinanet_ghm_config(depth) if cfg is None else cfg, bf16=bf16)


def build_fovea_detector(depth=50, align=False, cfg=None, bf16=False):
    """The detector of fovea_config(depth, align) (or of `cfg`), built like the other single-stage baselines: the `pretrained`
    URL of the reference's config dropped.  (The head's towers stay fp32 under bf16, as every dense head's do.)"""
    return build_baseline_detector(cfg=fovea_config(depth, align) if cfg is None else cfg, bf16=bf16)
