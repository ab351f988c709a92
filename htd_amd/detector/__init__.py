"""Registers every component of the HTD path and of its Faster R-CNN / Cascade R-CNN / RetinaNet / FCOS / ATSS / GFL / VFNet / FoveaBox baselines under the reference's
registry names."""
from . import losses, resnet, fpn, rpn_head, roi_extractors, bbox_heads, global_context_head, htd_bbox_head  # noqa
from . import htd_roi_head, roi_heads, two_stage, anchor_heads, anchor_free_heads, vfnet_head, fovea_head, single_stage  # noqa: F401
from .fovea_head import FeatureAlign, FoveaHead  # noqa: F401
from .single_stage import FOVEA  # noqa: F401
from .. import dcn  # noqa: F401  ('DCN' / 'DCNv2' conv layers)
