#!/usr/bin/env python
"""Generate the dataset / sampler fixtures by running the REFERENCE's own datasets/custom.py, datasets/coco.py,
samplers/group_sampler.py and samplers/distributed_sampler.py (loaded by file path, with make_golden's mmcv stand-in
and the small pycocotools COCO stand-in below).  Only recorded outputs are written:

  tests/golden/coco_dataset.npz     CocoDataset on coco_dataset_ann.json (hand-made, committed beside it) for
                                    test_mode x filter_empty_gt x classes, and the samplers' index sequences
  tests/golden/htd_data_cfgs.json   the `data` / `evaluation` sections of the five configs/htd/*.py, without
                                    their file paths (settings only)

    python tests/golden/make_golden_dataset.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402

DATASETS_DIR = os.path.join(make_golden.REF, 'mmdet', 'datasets')
ANN = os.path.join(HERE, 'coco_dataset_ann.json')
CONFIGS = ('htd_resnet50_1x', 'htd_resnet101_2x', 'htd_resnet101_2x_mstrain', 'htd_resnet101_dcn_2x_mstrain',
           'htd_resnetx101_dcn_2x_mstrain')
SUBSET = ('dog', 'car')


class COCO:
    """The pycocotools.coco.COCO calls CocoDataset makes: index dicts in file order, per-image and per-category
    lists built in annotation order."""

    def __init__(self, annotation_file):
        with open(annotation_file) as f:
            self.dataset = json.load(f)
        self.anns, self.imgs, self.cats = {}, {}, {}
        self.imgToAnns, self.catToImgs = {}, {}
        for ann in self.dataset.get('annotations', []):
            self.imgToAnns.setdefault(ann['image_id'], []).append(ann)
            self.anns[ann['id']] = ann
        for img in self.dataset.get('images', []):
            self.imgs[img['id']] = img
        for cat in self.dataset.get('categories', []):
            self.cats[cat['id']] = cat
        for ann in self.dataset.get('annotations', []):
            self.catToImgs.setdefault(ann['category_id'], []).append(ann['image_id'])

    @property
    def cat_img_map(self):
        class _Map(dict):
            def __missing__(self, k):
                return []
        return _Map(self.catToImgs)

    def get_cat_ids(self, cat_names=()):
        cats = self.dataset['categories']
        return [c['id'] for c in cats if len(cat_names) == 0 or c['name'] in cat_names]

    def get_img_ids(self):
        return list(self.imgs.keys())

    def get_ann_ids(self, img_ids):
        return [a['id'] for i in img_ids for a in self.imgToAnns.get(i, [])]

    def load_anns(self, ids):
        return [self.anns[i] for i in ids]

    def load_imgs(self, ids):
        return [self.imgs[i] for i in ids]


def load_reference():
    make_golden.install_mmcv_standin()
    mmcv = sys.modules['mmcv']
    mmcv.list_from_file = lambda fn: [x.rstrip('\n\r') for x in open(fn)]
    sys.modules['mmcv.runner'].get_dist_info = lambda: (0, 1)
    pyc = types.ModuleType('pycocotools')
    pyc.__version__ = '12.0.2'
    pyc_coco, pyc_eval = types.ModuleType('pycocotools.coco'), types.ModuleType('pycocotools.cocoeval')
    pyc_coco.COCO, pyc_eval.COCOeval = COCO, None
    tt = types.ModuleType('terminaltables')
    tt.AsciiTable = None
    core = types.ModuleType('mmdet.core')
    core.eval_map = core.eval_recalls = None
    mmdet = types.ModuleType('mmdet')
    mmdet.__path__ = []
    mmdet.core = core
    pkg = types.ModuleType('ref_datasets')
    pkg.__path__ = [DATASETS_DIR]
    builder = types.ModuleType('ref_datasets.builder')
    builder.DATASETS = make_golden.Registry('dataset')
    pipelines = types.ModuleType('ref_datasets.pipelines')

    class Compose:                 # the transforms are not under test here: a sample is its input dict
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, results):
            return results
    pipelines.Compose = Compose
    sys.modules.update({'pycocotools': pyc, 'pycocotools.coco': pyc_coco, 'pycocotools.cocoeval': pyc_eval,
                        'terminaltables': tt, 'mmdet': mmdet, 'mmdet.core': core, 'ref_datasets': pkg,
                        'ref_datasets.builder': builder, 'ref_datasets.pipelines': pipelines})
    mods = {}
    for name, path in [('custom', 'custom.py'), ('coco', 'coco.py'), ('group_sampler', 'samplers/group_sampler.py'),
                       ('distributed_sampler', 'samplers/distributed_sampler.py')]:
        spec = importlib.util.spec_from_file_location('ref_datasets.' + name, os.path.join(DATASETS_DIR, path))
        m = importlib.util.module_from_spec(spec)
        sys.modules['ref_datasets.' + name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods


def dataset_cases(mods, out):
    for test_mode in (True, False):
        for filter_empty_gt in (True, False):
            for cname, classes in (('all', None), ('subset', SUBSET)):
                key = f'{int(test_mode)}{int(filter_empty_gt)}_{cname}'
                ds = mods['coco'].CocoDataset(ANN, [], classes=classes, test_mode=test_mode,
                                              filter_empty_gt=filter_empty_gt)
                out[key + '/img_ids'] = np.array(ds.img_ids, np.int64)
                out[key + '/cat_ids'] = np.array(ds.cat_ids, np.int64)
                out[key + '/kept_ids'] = np.array([d['id'] for d in ds.data_infos], np.int64)
                out[key + '/flag'] = getattr(ds, 'flag', np.zeros(0, np.uint8))
                anns = [ds.get_ann_info(i) for i in range(len(ds))]
                for f in ('bboxes', 'labels', 'bboxes_ignore'):
                    out[f'{key}/{f}'] = np.concatenate([a[f] for a in anns]) if anns else np.zeros(0)
                    out[f'{key}/{f}_n'] = np.array([len(a[f]) for a in anns], np.int64)
                out[key + '/cat_of'] = np.array([len(ds.get_cat_ids(i)) for i in range(len(ds))], np.int64)


class _Flagged:
    def __init__(self, flag):
        self.flag = np.asarray(flag, np.uint8)

    def __len__(self):
        return len(self.flag)


FLAGS = {'mixed': [1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1], 'one_group': [1] * 7, 'zeros': [0] * 5}


def sampler_cases(mods, out):
    gs, ds = mods['group_sampler'], mods['distributed_sampler']
    for fname, flag in FLAGS.items():
        data = _Flagged(flag)
        for spg in (1, 2, 3):
            for seed in (0, 1, 7):
                np.random.seed(seed)
                out[f'group/{fname}/{spg}/{seed}'] = np.array(list(gs.GroupSampler(data, spg)), np.int64)
            for world in (1, 2, 3):
                for rank in range(world):
                    for epoch in (0, 1, 5):
                        s = gs.DistributedGroupSampler(data, spg, world, rank)
                        s.set_epoch(epoch)
                        out[f'dgroup/{fname}/{spg}/{world}/{rank}/{epoch}'] = np.array(list(s), np.int64)
    for n in (5, 7, 10):
        for world in (1, 2, 3):
            for rank in range(world):
                s = ds.DistributedSampler(list(range(n)), world, rank, shuffle=False)
                out[f'dist/{n}/{world}/{rank}'] = np.array(list(s), np.int64)


def data_cfgs():
    from htd_amd.registry import Config
    out = {}
    for name in CONFIGS:
        cfg = Config.fromfile(os.path.join(make_golden.REF, 'configs', 'htd', name + '.py'))
        data = cfg.data.to_dict()
        for split in ('train', 'val', 'test'):          # the authors' local paths are not settings
            data[split].pop('ann_file')
            data[split].pop('img_prefix')
        out[name] = dict(data=data, evaluation=cfg.get('evaluation').to_dict())
    return json.loads(json.dumps(out))


def main():
    mods = load_reference()
    out = {}
    dataset_cases(mods, out)
    sampler_cases(mods, out)
    np.savez_compressed(os.path.join(HERE, 'coco_dataset.npz'), **out)
    with open(os.path.join(HERE, 'htd_data_cfgs.json'), 'w') as f:
        json.dump(data_cfgs(), f, indent=1, sort_keys=True)
    print('coco_dataset.npz:', len(out), 'arrays;', torch.__version__)


if __name__ == '__main__':
    main()
