"""The VOC workflow through the command lines on a small generated VOCdevkit: `python -m htd_amd.train` for two
epochs on RepeatDataset(ConcatDataset(VOC2007, VOC2012)) with spawned loader workers and mAP evaluation after each
epoch, then `python -m htd_amd.test CONFIG CKPT --eval mAP` on the VOC2007 test split."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable',
           'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')


def write_devkit(root, seed=0):
    """VOC2007 (trainval 4 images, test 3) and VOC2012 (trainval 3) with JPEGs, XML and ImageSets lists."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    splits = {2007: {'trainval': 4, 'test': 3}, 2012: {'trainval': 3}}
    for year, sets in splits.items():
        base = os.path.join(root, f'VOC{year}')
        for sub in ('Annotations', 'JPEGImages', 'ImageSets/Main'):
            os.makedirs(os.path.join(base, sub), exist_ok=True)
        n = 0
        for name, count in sets.items():
            ids = []
            for _ in range(count):
                img_id = f'{year}_{n:06d}'
                n += 1
                w, h = [(96, 64), (64, 96), (80, 80)][n % 3]
                Image.fromarray((rs.rand(h, w, 3) * 255).astype(np.uint8)).save(
                    os.path.join(base, 'JPEGImages', img_id + '.jpg'), quality=95)
                objs = []
                for k in range(rs.randint(1, 4)):
                    x1, y1 = rs.randint(1, w // 2), rs.randint(1, h // 2)
                    x2, y2 = rs.randint(x1 + 8, w), rs.randint(y1 + 8, h)
                    objs.append(f'<object><name>{CLASSES[rs.randint(0, 20)]}</name><difficult>{int(k == 2)}'
                                f'</difficult><bndbox><xmin>{x1}</xmin><ymin>{y1}</ymin><xmax>{x2}</xmax>'
                                f'<ymax>{y2}</ymax></bndbox></object>')
                with open(os.path.join(base, 'Annotations', img_id + '.xml'), 'w') as f:
                    f.write(f'<annotation><size><width>{w}</width><height>{h}</height><depth>3</depth></size>'
                            + ''.join(objs) + '</annotation>')
                ids.append(img_id)
            with open(os.path.join(base, 'ImageSets', 'Main', name + '.txt'), 'w') as f:
                f.write(''.join(i + '\n' for i in ids))
    return root + '/'


def voc_cfg(devkit, work_dir):
    from htd_amd.configs import htd_config, voc0712_data
    cfg = htd_config(50, dataset='voc0712')
    cfg.data = type(cfg)(voc0712_data(data_root=devkit))
    cfg.model.pretrained = None
    cfg.test_cfg.rcnn.score_thr = 0.0                 # a seeded (untrained) model: keep every detection
    cfg.train_cfg.rpn_proposal.update(nms_pre=200, nms_post=100, max_num=100)
    for r in cfg.train_cfg.rcnn:
        r.sampler.num = 48
    cfg.data.train.dataset.pipeline[2]['img_scale'] = (128, 128)
    for split in (cfg.data.val, cfg.data.test):
        split.pipeline[1]['img_scale'] = (128, 128)
    cfg.data.workers_per_gpu = 2                      # spawned loader workers over the wrapper stack
    cfg.total_epochs = 2
    cfg.log_config = dict(interval=3, hooks=[dict(type='TextLoggerHook')])
    cfg.work_dir = str(work_dir)
    cfg.seed = 1
    return cfg


def _cli(args, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_train_and_test_cli(tmp_path):
    from golden_util import load_seeded_
    from htd_amd.checkpoint import save_checkpoint
    from htd_amd.configs import build_htd_detector
    from htd_amd.datasets import ConcatDataset, GroupSampler, RepeatDataset, build_dataset
    devkit = write_devkit(str(tmp_path / 'VOCdevkit'))
    cfg = voc_cfg(devkit, tmp_path / 'unused')
    train_set = build_dataset(cfg.data.train.to_dict())
    assert isinstance(train_set, RepeatDataset) and isinstance(train_set.dataset, ConcatDataset)
    assert [d.year for d in train_set.dataset.datasets] == [2007, 2012] and len(train_set) == 21
    seeded = str(tmp_path / 'seeded.pth')
    save_checkpoint(load_seeded_(build_htd_detector(cfg=cfg), 'det.'), seeded)
    cfg.load_from = seeded
    cfg_file = tmp_path / 'htd_voc_tiny.py'
    cfg_file.write_text(''.join(f'{k} = {v!r}\n' for k, v in cfg.to_dict().items() if k != 'work_dir'))
    work = str(tmp_path / 'work')
    p = _cli(['-m', 'htd_amd.train', str(cfg_file), '--work-dir', work])
    assert p.returncode == 0, p.stderr[-4000:]
    (name, ) = [f for f in os.listdir(work) if f.endswith('.log.json')]
    with open(os.path.join(work, name)) as f:
        lines = [json.loads(x) for x in f]
    train = [x for x in lines if x.get('mode') == 'train']
    iters = len(GroupSampler(train_set, 2)) // 2
    assert [(x['epoch'], x['iter']) for x in train] == [(e, i) for e in (1, 2) for i in range(3, iters + 1, 3)]
    assert all(np.isfinite(x['loss']) for x in train)
    val = [x for x in lines if x.get('mode') == 'val']
    assert [x['epoch'] for x in val] == [1, 2] and all(set(x) >= {'mAP'} for x in val)
    assert all(0.0 <= x['mAP'] <= 1.0 for x in val)
    ck = torch.load(os.path.join(work, 'epoch_2.pth'), weights_only=True)
    assert ck['meta']['CLASSES'] == list(CLASSES) and ck['meta']['epoch'] == 2
    assert ck['state_dict']['roi_head.bbox_head.0.fc_cls.weight'].shape[0] == 21

    p = _cli(['-m', 'htd_amd.test', str(cfg_file), os.path.join(work, 'epoch_2.pth'), '--eval', 'mAP'])
    assert p.returncode == 0, p.stderr[-3000:]
    m = re.search(r"'mAP'(?::|,) ([^,)}]+)", p.stdout)
    assert m is not None, (p.stdout[-3000:], p.stderr[-3000:])
    assert round(float(m.group(1)), 5) == val[-1]['mAP'], (m.group(1), val[-1])
    assert 'aeroplane' in p.stdout                     # the summary table names the VOC07 classes
