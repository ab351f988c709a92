"""Shared by tests/golden/make_golden_gn_ws.py, tests/test_gn_ws.py and tests/test_gpu_gn_ws.py: the weights and gradient keys
of the GN+WS Faster R-CNN fixture (tests/golden/gn_ws.npz), re-created from seeds so the fixture holds results only."""
import torch

from golden_util import load_seeded_

CONFIG = 'configs/gn+ws/faster_rcnn_r50_fpn_gn_ws-all_1x_coco.py'
CFG_JSON = 'faster_rcnn_r50_fpn_gn_ws-all_1x_coco_cfg.json'
CFG_KEYS = ('model', 'train_cfg', 'test_cfg', 'evaluation', 'optimizer', 'optimizer_config', 'lr_config', 'total_epochs')
# one convolution and one GroupNorm parameter of the stem, of each stage, of the neck and of the head
GRAD_KEYS = ('backbone.conv1.weight', 'backbone.gn1.weight',
             'backbone.layer1.0.conv2.weight', 'backbone.layer1.0.downsample.1.bias',
             'backbone.layer2.0.conv1.weight', 'backbone.layer2.3.gn3.weight',
             'backbone.layer3.1.conv3.weight', 'backbone.layer3.1.gn2.bias',
             'backbone.layer4.2.conv2.weight', 'backbone.layer4.2.gn3.weight',
             'neck.lateral_convs.0.conv.weight', 'neck.lateral_convs.3.gn.weight', 'neck.fpn_convs.1.conv.weight',
             'neck.fpn_convs.0.gn.bias',
             'rpn_head.rpn_conv.weight', 'rpn_head.rpn_reg.bias',
             'roi_head.bbox_head.shared_convs.0.conv.weight', 'roi_head.bbox_head.shared_convs.3.gn.weight',
             'roi_head.bbox_head.shared_fcs.0.bias', 'roi_head.bbox_head.fc_cls.weight', 'roi_head.bbox_head.fc_reg.weight')


FC_REG_SCALE = 0.25
GN3_SCALE = 0.25


def load_fixture_weights_(det, cls_scale, rpn_scale=1.0, rpn_bias=0.0, seed=1234):
    """load_seeded_(det, 'det.', seed) -- every GroupNorm weight 1 + 0.1 N(0, 1), every bias 0.05 N(0, 1) -- and then:
      * the last GroupNorm of every bottleneck (gn3) scaled by GN3_SCALE.  With gamma around 1 on all three norms of 16 residual
        blocks the seeded network amplifies rounding a thousandfold (the reference's fp32 and fp64 runs then keep different
        proposals); trained networks start from gamma3 = 0 (zero_init_residual) and stay well below 1.
      * the head's regressor scaled by FC_REG_SCALE (plainly seeded it throws the boxes across the image) and its classifier by
        cls_scale: plainly seeded, the 81 softmax scores of a RoI are nearly flat and the max_per_img cut falls among thousands
        of nearly equal scores.
      * the RPN's classifier scaled by rpn_scale and its bias lowered by rpn_bias.  Objectness scores s well below 1 put the
        relative gap of neighbouring scores at (1 - s) dz ~ dz, the gap of the logits, which grows with rpn_scale; around
        s = 0.8, where the plain seeds put them, the 200th of 3840 scores has its neighbour within 4e-4.
    cls_scale, rpn_scale, rpn_bias and seed are recorded in the fixture; the make script searches them for the margins."""
    load_seeded_(det, 'det.', seed)
    head = det.roi_head.bbox_head
    with torch.no_grad():
        for name, p in det.backbone.named_parameters():
            if name.endswith('gn3.weight'):
                p.mul_(GN3_SCALE)
        for m, f in ((head.fc_cls, cls_scale), (head.fc_reg, FC_REG_SCALE), (det.rpn_head.rpn_cls, rpn_scale)):
            m.weight.mul_(float(f))
            m.bias.mul_(float(f))
        det.rpn_head.rpn_cls.bias.sub_(float(rpn_bias))
    return det


def fixture_args(g):
    """The arguments of load_fixture_weights_ that the fixture g records."""
    return float(g['weight_scale']), float(g['rpn_scale']), float(g['rpn_bias']), int(g['seed'])
