"""Build libhtd_amd.so (gfx950) in-tree with hipcc.  Cross-compiles without a GPU.

    python -m htd_amd.csrc.build [--force]
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), 'libhtd_amd.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ARCH = 'gfx950'
COMMON = ['--offload-arch=' + ARCH, '-O3', '-fPIC', '-std=c++17', '-Wall', '-Wno-unused-function',
          '-fhip-fp32-correctly-rounded-divide-sqrt'] + os.environ.get('HTD_EXTRA_HIPCC', '').split()      # experiment builds (-D...)
# per-file extra flags: NMS keeps the CPU path's unfused arithmetic (bit-exact keep sets)
EXTRA = {'nms.hip': ['-ffp-contract=off'], 'box_ops.hip': ['-ffp-contract=off'],
         'image_pipeline.hip': ['-ffp-contract=off'], 'coco_eval.hip': ['-ffp-contract=off'],
         'voc_eval.hip': ['-ffp-contract=off'], 'fcos.hip': ['-ffp-contract=off'],
         'ghm_loss.hip': ['-ffp-contract=off'],     # its two passes must bin an element alike
         'atss.hip': ['-ffp-contract=off'],         # distances and IoUs one rounded operation at a time
         'gfl.hip': ['-ffp-contract=off'],          # centres, targets and IoU scores in the reference's fp32 order
         'vfnet.hip': ['-ffp-contract=off'],        # star offsets, target distances and both IoUs in that order too
         'fovea.hip': ['-ffp-contract=off']}        # the fovea rectangles one rounded operation at a time; offsets in channel order


# Every *.hip / *.cpp of this directory is a translation unit of the library; what each one replaces (include/htd_amd.h cites
# the reference interface per entry point):
#   focal_loss.hip   mmcv.ops.sigmoid_focal_loss (mmdet/models/losses/focal_loss.py:10-87) and AnchorHead.loss of a head without
#                    sampling over all pyramid levels (dense_heads/anchor_head.py:172-269,288-291,373-488, retina_head.py)
#   ghm_loss.hip     GHMC / GHMR (mmdet/models/losses/ghm_loss.py:20-172) and AnchorHead.loss with the pair (the level table,
#                    map decoding and box targets of focal_loss.hip, shared through retina_levels.h)
#   fcos.hip         FCOSHead's targets, loss and ranking keys (dense_heads/fcos_head.py:159-253,364-372,415-576)
#   atss.hip         ATSSAssigner over a batch with the centerness targets and averaging factors, and ATSSHead's loss
#                    (core/bbox/assigners/atss_assigner.py:33-178, dense_heads/atss_head.py:145-313)
#   gfl.hip          GFLHead's quality pass, loss (QFL, weighted IoU / GIoU, DFL) and inference decode
#                    (dense_heads/gfl_head.py:209-369,420-428, losses/gfocal_loss.py:8-74)
#   vfnet.hip        VFNetHead's star offsets with their backward, quality pass and loss (varifocal loss, two IoU-weighted
#                    IoU / GIoU losses) (dense_heads/vfnet_head.py:246-314,317-463, losses/varifocal_loss.py:8-53)
#   fovea.hip        FoveaHead's fovea-rectangle targets and loss (focal, smooth-L1 on log distances) and FeatureAlign's offsets
#                    with their backward (dense_heads/fovea_head.py:13-39,127-258)
# The seven share focal_elem.h (the element arithmetic) and loss_units.h (level search, VEC-wide units, matrix units).  The last
# five, the heads with one prediction per location, share point_maps.h (their map table and its checker, the loss grid and the
# float4 / lane-group decision, the decoding of a pixel row, the classification sweep of their loss kernels), point_scale.h
# (the kernel behind htd_fcos_grad_scale, htd_vfnet_grad_scale and htd_fovea_grad_scale) and, but for FCOS and FoveaBox,
# anchor_levels.h (the level table of htd_atss_targets' anchors, the box load, the reference's fp32 IoU): each of the five files
# holds only what its head alone does.
def sources():
    return sorted(f for f in os.listdir(HERE) if f.endswith('.hip') or f.endswith('.cpp'))


def _newest_dep():
    deps = [os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith(('.hip', '.cpp', '.h'))]
    deps.append(os.path.join(HERE, '..', '..', 'include', 'htd_amd.h'))
    return max(os.path.getmtime(d) for d in deps)


def _compile(src):
    obj = os.path.join(HERE, '_obj', src + '.o')
    hdr_time = max(os.path.getmtime(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith('.h'))
    hdr_time = max(hdr_time, os.path.getmtime(os.path.join(HERE, '..', '..', 'include', 'htd_amd.h')))
    if os.path.exists(obj) and os.path.getmtime(obj) > max(os.path.getmtime(os.path.join(HERE, src)), hdr_time):
        return obj
    cmd = [HIPCC] + COMMON + EXTRA.get(src, []) + ['-c', os.path.join(HERE, src), '-o', obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc failed for %s:\n%s\n%s' % (src, ' '.join(cmd), r.stderr[-6000:]))
    return obj


def build(force=False, verbose=False):
    os.makedirs(os.path.join(HERE, '_obj'), exist_ok=True)
    if force:
        for f in os.listdir(os.path.join(HERE, '_obj')):
            os.remove(os.path.join(HERE, '_obj', f))
    if not force and os.path.exists(LIB) and os.path.getmtime(LIB) > _newest_dep():
        return LIB
    with ThreadPoolExecutor(max_workers=6) as ex:
        objs = list(ex.map(_compile, sources()))
    cmd = [HIPCC, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-o', LIB] + objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('link failed:\n' + r.stderr[-4000:])
    if verbose:
        print('built', LIB)
    return LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv, verbose=True)
