"""Data for the test and train loops: the COCO and Pascal VOC datasets, the dataset wrappers, the samplers and the data
loader, without pycocotools or mmcv.

`CocoDataset` behaves like the reference's (datasets/custom.py, datasets/coco.py): the same constructor arguments, the
same index orders (images in file order, the file's categories whose names are in CLASSES, each image's annotations in
file order), the same filters, the same parsed annotations and the same `np.random` use.  The samplers consume random
numbers exactly as the reference's do (samplers/group_sampler.py, samplers/distributed_sampler.py), so a seed gives the
same index sequence.  XMLDataset / VOCDataset (datasets/xml_style.py, voc.py) and the wrappers ConcatDataset,
RepeatDataset and ClassBalancedDataset (dataset_wrappers.py, builder.py) follow the reference in the same way.

Samples are planned on the host.  The loader's collate function hands over the list of `Collect` dicts unchanged, and
the caller turns a batch into device tensors with `pipelines.collate(samples, device)` in the main process: one upload
of uint8 pixels and one launch of htd_image_batch_pipeline.  Loader workers are started with `spawn` and never touch the
GPU: they decode with PIL and run the planning transforms only.
"""
import bisect
import copy
import json
import math
import os.path as osp
import random
import tempfile
import warnings
import xml.etree.ElementTree as ET
from collections import OrderedDict, defaultdict
from functools import partial

import numpy as np
import torch
from torch.utils.data import ConcatDataset as TorchConcatDataset
from torch.utils.data import DataLoader, Dataset, Sampler

from .coco import COCO_CLASSES, CocoEvaluator
from .pipelines import Compose
from .registry import Registry, build_from_cfg

DATASETS = Registry('dataset')


def get_dist_info():
    """(rank, world size) of the default process group, (0, 1) without one."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _concat_dataset(cfg, default_args=None):
    """A config whose ann_file is a list: one dataset per entry (img_prefix / seg_prefix / proposal_file lists are
    taken entry by entry) in a ConcatDataset with the config's separate_eval (default True)."""
    ann_files = cfg['ann_file']
    img_prefixes, seg_prefixes = cfg.get('img_prefix', None), cfg.get('seg_prefix', None)
    proposal_files = cfg.get('proposal_file', None)
    datasets = []
    for i in range(len(ann_files)):
        part = copy.deepcopy(dict(cfg))
        part.pop('separate_eval', None)
        part['ann_file'] = ann_files[i]
        for key, val in (('img_prefix', img_prefixes), ('seg_prefix', seg_prefixes), ('proposal_file', proposal_files)):
            if isinstance(val, (list, tuple)):
                part[key] = val[i]
        datasets.append(build_dataset(part, default_args))
    return ConcatDataset(datasets, cfg.get('separate_eval', True))


def build_dataset(cfg, default_args=None):
    """A dataset from its config dict (datasets/builder.py): a list of configs, ConcatDataset, RepeatDataset and
    ClassBalancedDataset configs, and a list ann_file are wrapped; anything else names a DATASETS entry."""
    if isinstance(cfg, (list, tuple)):
        return ConcatDataset([build_dataset(c, default_args) for c in cfg])
    if cfg['type'] == 'ConcatDataset':
        return ConcatDataset([build_dataset(c, default_args) for c in cfg['datasets']], cfg.get('separate_eval', True))
    if cfg['type'] == 'RepeatDataset':
        return RepeatDataset(build_dataset(cfg['dataset'], default_args), cfg['times'])
    if cfg['type'] == 'ClassBalancedDataset':
        return ClassBalancedDataset(build_dataset(cfg['dataset'], default_args), cfg['oversample_thr'])
    if isinstance(cfg.get('ann_file'), (list, tuple)):
        return _concat_dataset(cfg, default_args)
    return build_from_cfg(cfg, DATASETS, default_args)


class CocoIndex:
    """What CocoDataset reads of a COCO annotation file, in pycocotools' orders: `imgs` / `anns` / `cats` keyed by id
    in file order, `img_anns[image_id]` = that image's annotations in file order, `cat_img_map[category_id]` = the image
    id of every annotation of the category (repeats included)."""

    def __init__(self, data):
        self.dataset = data
        self.imgs = {im['id']: im for im in data.get('images', [])}
        self.cats = {c['id']: c for c in data.get('categories', [])}
        self.anns, self.img_anns, self.cat_img_map = {}, {}, {}
        for a in data.get('annotations', []):
            self.anns[a['id']] = a
            self.img_anns.setdefault(a['image_id'], []).append(a)
            self.cat_img_map.setdefault(a['category_id'], []).append(a['image_id'])

    def cat_ids_named(self, names):
        """Ids of the categories whose name is in `names` (all of them when `names` is empty), in file order."""
        return [c['id'] for c in self.dataset.get('categories', []) if not len(names) or c['name'] in names]

    def anns_of(self, img_id):
        """The image's annotations, looked up by annotation id as COCO.loadAnns(getAnnIds(imgIds=[img_id])) does."""
        return [self.anns[a['id']] for a in self.img_anns.get(img_id, [])]


class CustomDataset(Dataset):
    """What CocoDataset and XMLDataset share (datasets/custom.py): paths under data_root, CLASSES, the train-mode image
    filter and aspect-ratio `flag`, the pipeline, and re-drawing a refused train sample from its group."""

    CLASSES = None

    def __init__(self, ann_file, pipeline, classes=None, data_root=None, img_prefix='', seg_prefix=None,
                 proposal_file=None, test_mode=False, filter_empty_gt=True):
        if proposal_file is not None:
            raise ValueError(f'{type(self).__name__}: proposal_file is not supported, HTD computes its proposals '
                             'with its RPN')
        self.data_root, self.proposal_file = data_root, None
        self.test_mode, self.filter_empty_gt = test_mode, filter_empty_gt
        self.CLASSES = self.get_classes(classes)

        def under_root(path):          # relative paths are taken from data_root when it is given
            return path if data_root is None or path is None or osp.isabs(path) else osp.join(data_root, path)
        self.ann_file, self.img_prefix, self.seg_prefix = under_root(ann_file), under_root(img_prefix), \
            under_root(seg_prefix)
        self.data_infos = self.load_annotations(self.ann_file)
        self.proposals = None
        if not test_mode:
            kept = self._filter_imgs()
            self.data_infos = [self.data_infos[i] for i in kept]
            self._set_group_flag()
        self.pipeline = Compose(pipeline)

    def __len__(self):
        return len(self.data_infos)

    @classmethod
    def get_classes(cls, classes=None):
        """None: cls.CLASSES; a str: a file with one name per line; a tuple / list: those names."""
        if classes is None:
            return cls.CLASSES
        if isinstance(classes, str):
            with open(classes) as f:
                return [line.rstrip('\n\r') for line in f]
        if isinstance(classes, (tuple, list)):
            return classes
        raise ValueError(f'Unsupported type {type(classes)} of classes.')

    def _set_group_flag(self):
        self.flag = np.array([int(info['width'] / info['height'] > 1) for info in self.data_infos], dtype=np.uint8)

    def pre_pipeline(self, results):
        results.update(img_prefix=self.img_prefix, seg_prefix=self.seg_prefix, proposal_file=self.proposal_file,
                       bbox_fields=[], mask_fields=[], seg_fields=[])

    def _rand_another(self, idx):
        return np.random.choice(np.flatnonzero(self.flag == self.flag[idx]))

    def __getitem__(self, idx):
        if self.test_mode:
            return self.prepare_test_img(idx)
        data = self.prepare_train_img(idx)
        while data is None:                # a pipeline may refuse a sample: try another of the same group
            idx = self._rand_another(idx)
            data = self.prepare_train_img(idx)
        return data

    def prepare_train_img(self, idx):
        results = dict(img_info=self.data_infos[idx], ann_info=self.get_ann_info(idx))
        self.pre_pipeline(results)
        return self.pipeline(results)

    def prepare_test_img(self, idx):
        results = dict(img_info=self.data_infos[idx])
        self.pre_pipeline(results)
        return self.pipeline(results)


@DATASETS.register_module()
class CocoDataset(CustomDataset):
    """A COCO-format detection dataset.  In train mode (test_mode=False) images smaller than 32 px, and with
    filter_empty_gt images without an annotation of CLASSES, are dropped, and `flag` groups the rest by aspect ratio
    (1 where w / h > 1).  `evaluate` / `results2json` / `format_results` / `fast_eval_recall` run through CocoEvaluator,
    built from the index in memory over this dataset's `img_ids`."""

    CLASSES = COCO_CLASSES

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._evaluator = None

    def load_annotations(self, ann_file):
        with open(ann_file) as f:
            self.coco = CocoIndex(json.load(f))
        self.cat_ids = self.coco.cat_ids_named(self.CLASSES)
        self.cat2label = {c: label for label, c in enumerate(self.cat_ids)}
        self.img_ids = list(self.coco.imgs)
        for info in self.coco.imgs.values():
            info['filename'] = info['file_name']
        return [self.coco.imgs[i] for i in self.img_ids]

    def get_ann_info(self, idx):
        info = self.data_infos[idx]
        return self._parse_ann_info(info, self.coco.anns_of(info['id']))

    def get_cat_ids(self, idx):
        return [a['category_id'] for a in self.coco.anns_of(self.data_infos[idx]['id'])]

    def _filter_imgs(self, min_size=32):
        """-> indices of the images kept; self.img_ids becomes their ids."""
        annotated = {a['image_id'] for a in self.coco.anns.values()}
        with_class = set()
        for c in self.cat_ids:
            with_class.update(self.coco.cat_img_map.get(c, ()))
        with_class &= annotated
        kept = [i for i, (img_id, info) in enumerate(zip(self.img_ids, self.data_infos))
                if not (self.filter_empty_gt and img_id not in with_class)
                and min(info['width'], info['height']) >= min_size]
        self.img_ids = [self.img_ids[i] for i in kept]
        return kept

    def _parse_ann_info(self, img_info, ann_info):
        """-> dict(bboxes (n, 4) f32 xyxy, labels (n,) i64, bboxes_ignore (k, 4) f32 crowd boxes, seg_map).  Skipped:
        `ignore` annotations, boxes with no overlap with the image, area <= 0, w < 1 or h < 1, other categories."""
        boxes, labels, crowd = [], [], []
        W, H = img_info['width'], img_info['height']
        for a in ann_info:
            if a.get('ignore', False):
                continue
            x, y, w, h = a['bbox']
            overlap_w = max(0, min(x + w, W) - max(x, 0))
            overlap_h = max(0, min(y + h, H) - max(y, 0))
            if overlap_w * overlap_h == 0 or a['area'] <= 0 or w < 1 or h < 1 or a['category_id'] not in self.cat_ids:
                continue
            if a.get('iscrowd', False):
                crowd.append([x, y, x + w, y + h])
            else:
                boxes.append([x, y, x + w, y + h])
                labels.append(self.cat2label[a['category_id']])

        def as_boxes(rows):
            return np.array(rows, dtype=np.float32) if rows else np.zeros((0, 4), dtype=np.float32)
        return dict(bboxes=as_boxes(boxes), labels=np.array(labels, dtype=np.int64), bboxes_ignore=as_boxes(crowd),
                    seg_map=img_info['filename'].replace('jpg', 'png'))

    # ------------------------------------------------------------------------------------------------ evaluation
    @property
    def evaluator(self):
        if self._evaluator is None:
            data = dict(self.coco.dataset, images=[self.coco.imgs[i] for i in self.img_ids])
            self._evaluator = CocoEvaluator(data, classes=self.CLASSES)
        return self._evaluator

    def results2json(self, results, outfile_prefix):
        return self.evaluator.results2json(results, outfile_prefix)

    def fast_eval_recall(self, results, proposal_nums, iou_thrs, logger=None):
        return self.evaluator.fast_eval_recall(results, proposal_nums, iou_thrs, logger=logger)

    def format_results(self, results, jsonfile_prefix=None, **kwargs):
        """-> (result files, tmp_dir): tmp_dir is the TemporaryDirectory holding them when no prefix is given."""
        assert isinstance(results, list), 'results must be a list'
        assert len(results) == len(self), \
            f'The length of results is not equal to the dataset len: {len(results)} != {len(self)}'
        tmp_dir = None
        if jsonfile_prefix is None:
            tmp_dir = tempfile.TemporaryDirectory()
            jsonfile_prefix = osp.join(tmp_dir.name, 'results')
        return self.results2json(results, jsonfile_prefix), tmp_dir

    def evaluate(self, results, metric='bbox', logger=None, jsonfile_prefix=None, classwise=False,
                 proposal_nums=(100, 300, 1000), iou_thrs=None, metric_items=None):
        """results: bbox2result lists, (k, 5) proposal arrays, or the (dets, labels, dataset index) triple of
        apis.results_to_tensors."""
        return self.evaluator.evaluate(results, metric=metric, logger=logger, jsonfile_prefix=jsonfile_prefix,
                                       classwise=classwise, proposal_nums=proposal_nums, iou_thrs=iou_thrs,
                                       metric_items=metric_items)


@DATASETS.register_module()
class VOCDataset_coco(CocoDataset):
    """Pascal VOC converted to COCO format (the reference's datasets/voc_coco.py)."""
    CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable',
               'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')


@DATASETS.register_module()
class DHD_Traffic(CocoDataset):
    """The DHD traffic set in COCO format (the reference's datasets/dhd_traffic.py)."""
    CLASSES = ('Pedestrian', 'Cyclist', 'Car', 'Truck', 'Van')


@DATASETS.register_module()
class EADDataset(CocoDataset):
    """EndoCV2019 artefact detection in COCO format (the reference's datasets/endocv19.py)."""
    CLASSES = ('specularity', 'saturation', 'artifact', 'blur', 'contrast', 'bubbles', 'instrument')


@DATASETS.register_module()
class XMLDataset(CustomDataset):
    """A Pascal-VOC-style dataset (datasets/xml_style.py): `ann_file` lists image ids, image `id` is
    JPEGImages/{id}.jpg under img_prefix and Annotations/{id}.xml holds its objects.  Boxes are int(float(text)) - 1
    as float32; `difficult` objects and (train mode only) boxes narrower or lower than min_size are ignored boxes;
    objects of other classes are skipped."""

    def __init__(self, min_size=None, **kwargs):
        super().__init__(**kwargs)
        self.cat2label = {cat: i for i, cat in enumerate(self.CLASSES)}
        self.min_size = min_size

    def _xml(self, img_id):
        return ET.parse(osp.join(self.img_prefix, 'Annotations', f'{img_id}.xml')).getroot()

    def load_annotations(self, ann_file):
        with open(ann_file) as f:
            img_ids = [line.rstrip('\n\r') for line in f]
        infos = []
        for img_id in img_ids:
            size = self._xml(img_id).find('size')
            if size is not None:
                width, height = int(size.find('width').text), int(size.find('height').text)
            else:
                from PIL import Image
                with Image.open(osp.join(self.img_prefix, 'JPEGImages', f'{img_id}.jpg')) as img:
                    width, height = img.size
            infos.append(dict(id=img_id, filename=f'JPEGImages/{img_id}.jpg', width=width, height=height))
        return infos

    def _filter_imgs(self, min_size=32):
        kept = []
        for i, info in enumerate(self.data_infos):
            if min(info['width'], info['height']) < min_size:
                continue
            if self.filter_empty_gt and not any(o.find('name').text in self.CLASSES
                                                for o in self._xml(info['id']).findall('object')):
                continue
            kept.append(i)
        return kept

    def get_ann_info(self, idx):
        bboxes, labels, bboxes_ignore, labels_ignore = [], [], [], []
        for obj in self._xml(self.data_infos[idx]['id']).findall('object'):
            name = obj.find('name').text
            if name not in self.CLASSES:
                continue
            label = self.cat2label[name]
            difficult = int(obj.find('difficult').text)
            bnd = obj.find('bndbox')
            bbox = [int(float(bnd.find(k).text)) for k in ('xmin', 'ymin', 'xmax', 'ymax')]
            ignore = False
            if self.min_size:
                if self.test_mode:
                    raise AssertionError('XMLDataset: min_size is a train-mode setting')
                ignore = bbox[2] - bbox[0] < self.min_size or bbox[3] - bbox[1] < self.min_size
            if difficult or ignore:
                bboxes_ignore.append(bbox)
                labels_ignore.append(label)
            else:
                bboxes.append(bbox)
                labels.append(label)

        def as_boxes(rows):
            return (np.array(rows, ndmin=2) - 1).astype(np.float32) if rows else np.zeros((0, 4), np.float32)
        return dict(bboxes=as_boxes(bboxes), labels=np.array(labels, dtype=np.int64),
                    bboxes_ignore=as_boxes(bboxes_ignore), labels_ignore=np.array(labels_ignore, dtype=np.int64))

    def get_cat_ids(self, idx):
        return [self.cat2label[o.find('name').text] for o in self._xml(self.data_infos[idx]['id']).findall('object')
                if o.find('name').text in self.CLASSES]


@DATASETS.register_module()
class VOCDataset(XMLDataset):
    """Pascal VOC 2007 / 2012 (datasets/voc.py).  `evaluate` scores 'mAP' with the device eval_map (VOC07's 11-point
    AP when img_prefix names VOC2007, the area under the curve for VOC2012) or 'recall' with the device eval_recalls."""

    CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable',
               'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if 'VOC2007' in self.img_prefix:
            self.year = 2007
        elif 'VOC2012' in self.img_prefix:
            self.year = 2012
        else:
            raise ValueError('Cannot infer dataset year from img_prefix')

    def evaluate(self, results, metric='mAP', logger=None, proposal_nums=(100, 300, 1000), iou_thr=0.5,
                 scale_ranges=None):
        """results: bbox2result lists or the (dets, labels, dataset index) triple for 'mAP'; proposal arrays for
        'recall'.  scale_ranges is accepted and, as in the reference, not used."""
        from .core.evaluation import eval_map, eval_recalls
        if not isinstance(metric, str):
            assert len(metric) == 1
            metric = metric[0]
        if metric not in ('mAP', 'recall'):
            raise KeyError(f'metric {metric} is not supported')
        annotations = [self.get_ann_info(i) for i in range(len(self))]
        eval_results = OrderedDict()
        if metric == 'mAP':
            assert isinstance(iou_thr, float)
            ds_name = 'voc07' if self.year == 2007 else self.CLASSES
            mean_ap, _ = eval_map(results, annotations, scale_ranges=None, iou_thr=iou_thr, dataset=ds_name,
                                  logger=logger, num_classes=len(self.CLASSES))
            eval_results['mAP'] = mean_ap
        else:
            gt_bboxes = [ann['bboxes'] for ann in annotations]
            if isinstance(iou_thr, float):
                iou_thr = [iou_thr]
            recalls = eval_recalls(gt_bboxes, results, proposal_nums, iou_thr, logger=logger)
            for i, num in enumerate(proposal_nums):
                for j, iou in enumerate(iou_thr):
                    eval_results[f'recall@{num}@{iou}'] = recalls[i, j]
            if recalls.shape[1] > 1:
                ar = recalls.mean(axis=1)
                for i, num in enumerate(proposal_nums):
                    eval_results[f'AR@{num}'] = ar[i]
        return eval_results


# ---------------------------------------------------------------------------------------------------- wrappers
def _is_triple(results):
    return isinstance(results, tuple) and len(results) == 3 and isinstance(results[0], torch.Tensor)


def _results_slice(results, start, end):
    """Results of dataset samples start..end-1: a list slice, or for the (dets, labels, index) triple the rows whose
    index falls there, re-indexed from 0."""
    if not _is_triple(results):
        return results[start:end]
    dets, labels, index = results
    keep = ((index >= start) & (index < end)).nonzero().squeeze(1)
    return dets[keep], labels[keep], index[keep] - start


@DATASETS.register_module()
class ConcatDataset(TorchConcatDataset):
    """torch's ConcatDataset plus the concatenated group `flag` (dataset_wrappers.py).  separate_eval=True evaluates
    each part and prefixes its keys with its position; False evaluates the whole as the first part would, which
    COCO-format parts and mixed types refuse."""

    def __init__(self, datasets, separate_eval=True):
        super().__init__(datasets)
        self.CLASSES = datasets[0].CLASSES
        self.separate_eval = separate_eval
        if not separate_eval:
            self._check_whole()
        if hasattr(datasets[0], 'flag'):
            self.flag = np.concatenate([d.flag for d in datasets])

    def _check_whole(self):
        if any(isinstance(d, CocoDataset) for d in self.datasets):
            raise NotImplementedError('Evaluating concatenated CocoDataset as a whole is not supported! Please set '
                                      '"separate_eval=True"')
        if len({type(d) for d in self.datasets}) != 1:
            raise NotImplementedError('All the datasets should have same types')

    def get_cat_ids(self, idx):
        if idx < 0:
            if -idx > len(self):
                raise ValueError('absolute value of index should not exceed dataset length')
            idx = len(self) + idx
        part = bisect.bisect_right(self.cumulative_sizes, idx)
        return self.datasets[part].get_cat_ids(idx - (self.cumulative_sizes[part - 1] if part else 0))

    def evaluate(self, results, logger=None, **kwargs):
        from .core.evaluation import print_log
        if not _is_triple(results):
            assert len(results) == self.cumulative_sizes[-1], \
                f'Dataset and results have different sizes: {self.cumulative_sizes[-1]} v.s. {len(results)}'
        for d in self.datasets:
            assert hasattr(d, 'evaluate'), f'{type(d)} does not implement evaluate function'
        if self.separate_eval:
            out, start = {}, 0
            for i, (end, d) in enumerate(zip(self.cumulative_sizes, self.datasets)):
                part = _results_slice(results, start, end)
                print_log(f'\nEvaluateing {d.ann_file} with {len(part)} images now', logger=logger)
                for k, v in d.evaluate(part, logger=logger, **kwargs).items():
                    out[f'{i}_{k}'] = v
                start = end
            return out
        self._check_whole()
        first = self.datasets[0]
        infos = first.data_infos
        first.data_infos = sum([d.data_infos for d in self.datasets], [])
        try:
            return first.evaluate(results, logger=logger, **kwargs)
        finally:
            first.data_infos = infos


@DATASETS.register_module()
class RepeatDataset:
    """The dataset `times` over (dataset_wrappers.py): index i is sample i % len(dataset)."""

    def __init__(self, dataset, times):
        self.dataset, self.times = dataset, times
        self.CLASSES = dataset.CLASSES
        if hasattr(dataset, 'flag'):
            self.flag = np.tile(dataset.flag, times)
        self._ori_len = len(dataset)

    def __getitem__(self, idx):
        return self.dataset[idx % self._ori_len]

    def get_cat_ids(self, idx):
        return self.dataset.get_cat_ids(idx % self._ori_len)

    def __len__(self):
        return self.times * self._ori_len


@DATASETS.register_module()
class ClassBalancedDataset:
    """Repeat-factor sampling (dataset_wrappers.py, LVIS): image I appears ceil(max over its categories c of
    max(1, sqrt(oversample_thr / f(c)))) times, f(c) the fraction of images holding c; with filter_empty_gt=False an
    image without objects counts as the background class len(CLASSES)."""

    def __init__(self, dataset, oversample_thr, filter_empty_gt=True):
        self.dataset, self.oversample_thr, self.filter_empty_gt = dataset, oversample_thr, filter_empty_gt
        self.CLASSES = dataset.CLASSES
        factors = self._get_repeat_factors(dataset, oversample_thr)
        self.repeat_indices = [i for i, f in enumerate(factors) for _ in range(math.ceil(f))]
        flags = []
        if hasattr(dataset, 'flag'):
            for flag, f in zip(dataset.flag, factors):
                flags.extend([flag] * int(math.ceil(f)))
            assert len(flags) == len(self.repeat_indices)
        self.flag = np.asarray(flags, dtype=np.uint8)

    def _cats(self, idx):
        cats = set(self.dataset.get_cat_ids(idx))
        if not cats and not self.filter_empty_gt:
            cats = {len(self.CLASSES)}
        return cats

    def _get_repeat_factors(self, dataset, repeat_thr):
        n = len(dataset)
        freq = defaultdict(int)
        for idx in range(n):
            for c in self._cats(idx):
                freq[c] += 1
        rep = {c: max(1.0, math.sqrt(repeat_thr / (v / n))) for c, v in freq.items()}
        out = []
        for idx in range(n):
            cats = self._cats(idx)
            out.append(max({rep[c] for c in cats}) if cats else 1)
        return out

    def __getitem__(self, idx):
        return self.dataset[self.repeat_indices[idx]]

    def __len__(self):
        return len(self.repeat_indices)


def replace_ImageToTensor(pipelines):
    """A copy of a pipeline config with every ImageToTensor (inside MultiScaleFlipAug too) replaced by
    DefaultFormatBundle, for batched inference."""
    def swap(t):
        if t['type'] == 'MultiScaleFlipAug':
            assert 'transforms' in t
            return dict(t, transforms=[swap(x) for x in t['transforms']])
        if t['type'] == 'ImageToTensor':
            warnings.warn('"ImageToTensor" pipeline is replaced by "DefaultFormatBundle" for batch inference. It is '
                          'recommended to manually replace it in the test data pipeline in your config file.',
                          UserWarning)
            return {'type': 'DefaultFormatBundle'}
        return t
    return [swap(t) for t in copy.deepcopy(pipelines)]


# ---------------------------------------------------------------------------------------------------- samplers
def _round_up(n, m):
    return -(-int(n) // m) * m


class GroupSampler(Sampler):
    """Batches of samples_per_gpu indices from one `flag` group each, in random order, on the global np.random: per
    non-empty group a shuffle and a draw of the indices that fill its last batch, then a permutation of the batches."""

    def __init__(self, dataset, samples_per_gpu=1):
        assert hasattr(dataset, 'flag')
        self.dataset, self.samples_per_gpu = dataset, samples_per_gpu
        self.flag = dataset.flag.astype(np.int64)
        self.group_sizes = np.bincount(self.flag)
        self.num_samples = sum(_round_up(n, samples_per_gpu) for n in self.group_sizes)

    def __iter__(self):
        spg = self.samples_per_gpu
        parts = []
        for g, n in enumerate(self.group_sizes):
            if n == 0:
                continue
            members = np.flatnonzero(self.flag == g)
            np.random.shuffle(members)
            fill = np.random.choice(members, _round_up(n, spg) - n)
            parts.append(np.concatenate([members, fill]))
        batches = np.concatenate(parts).reshape(-1, spg)
        order = np.random.permutation(len(batches))
        out = batches[order].reshape(-1).astype(np.int64).tolist()
        assert len(out) == self.num_samples
        return iter(out)

    def __len__(self):
        return self.num_samples


class DistributedGroupSampler(Sampler):
    """The distributed GroupSampler: a torch.Generator seeded with the epoch permutes each non-empty group, which is
    then padded cyclically to a multiple of samples_per_gpu * num_replicas; a second permutation orders the batches
    and rank r takes the r-th contiguous num_samples of them."""

    def __init__(self, dataset, samples_per_gpu=1, num_replicas=None, rank=None):
        own_rank, own_world = get_dist_info()
        self.dataset, self.samples_per_gpu = dataset, samples_per_gpu
        self.num_replicas = own_world if num_replicas is None else num_replicas
        self.rank = own_rank if rank is None else rank
        self.epoch = 0
        assert hasattr(dataset, 'flag')
        self.flag = dataset.flag
        self.group_sizes = np.bincount(self.flag)
        self.num_samples = sum(int(math.ceil(n * 1.0 / samples_per_gpu / self.num_replicas)) * samples_per_gpu
                               for n in self.group_sizes)
        self.total_size = self.num_samples * self.num_replicas

    def __iter__(self):
        gen = torch.Generator()
        gen.manual_seed(self.epoch)
        spg, world = self.samples_per_gpu, self.num_replicas
        pool = []
        for g, n in enumerate(self.group_sizes):
            if n == 0:
                continue
            members = np.flatnonzero(self.flag == g)[torch.randperm(int(n), generator=gen).numpy()]
            target = int(math.ceil(n * 1.0 / spg / world)) * spg * world
            pool.append(np.resize(members, target))          # cyclic repetition up to the padded size
        pool = np.concatenate(pool)
        assert len(pool) == self.total_size
        order = torch.randperm(len(pool) // spg, generator=gen).numpy()
        out = pool.reshape(-1, spg)[order].reshape(-1)
        out = out[self.num_samples * self.rank:self.num_samples * (self.rank + 1)].astype(np.int64).tolist()
        assert len(out) == self.num_samples
        return iter(out)

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


class DistributedSampler(Sampler):
    """Every num_replicas-th index from `rank`, after padding the (optionally epoch-seeded, permuted) index list to
    num_replicas * ceil(len / num_replicas) by repeating its head."""

    def __init__(self, dataset, num_replicas=None, rank=None, shuffle=True):
        own_rank, own_world = get_dist_info()
        self.dataset, self.shuffle, self.epoch = dataset, shuffle, 0
        self.num_replicas = own_world if num_replicas is None else num_replicas
        self.rank = own_rank if rank is None else rank
        self.num_samples = int(math.ceil(len(dataset) / self.num_replicas))
        self.total_size = self.num_samples * self.num_replicas

    def __iter__(self):
        n = len(self.dataset)
        if self.shuffle:
            gen = torch.Generator()
            gen.manual_seed(self.epoch)
            base = torch.randperm(n, generator=gen).numpy()
        else:
            base = np.arange(n)
        padded = np.resize(base, self.total_size)
        return iter(padded[self.rank::self.num_replicas].astype(np.int64).tolist())

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


# ---------------------------------------------------------------------------------------------------- loader
def host_collate(batch):
    """The loader's collate_fn: the batch's `Collect` dicts as they are (pipelines.collate makes the device batch)."""
    return batch


def worker_init_fn(worker_id, num_workers, rank, seed):
    """Seeds np.random and random of a loader worker with num_workers * rank + worker_id + seed."""
    s = num_workers * rank + worker_id + seed
    np.random.seed(s)
    random.seed(s)


def build_dataloader(dataset, samples_per_gpu, workers_per_gpu, num_gpus=1, dist=True, shuffle=True, seed=None,
                     **kwargs):
    """A DataLoader whose batches are lists of `Collect` dicts.  dist=True: DistributedGroupSampler (shuffle) or
    DistributedSampler, samples_per_gpu per batch.  dist=False: GroupSampler (shuffle) or file order, num_gpus *
    samples_per_gpu per batch.  Workers are spawned, never forked from a process that may hold a HIP context."""
    rank, world_size = get_dist_info()
    if dist:
        sampler = DistributedGroupSampler(dataset, samples_per_gpu, world_size, rank) if shuffle else \
            DistributedSampler(dataset, world_size, rank, shuffle=False)
        batch_size, num_workers = samples_per_gpu, workers_per_gpu
    else:
        sampler = GroupSampler(dataset, samples_per_gpu) if shuffle else None
        batch_size, num_workers = num_gpus * samples_per_gpu, num_gpus * workers_per_gpu
    init_fn = None if seed is None else partial(worker_init_fn, num_workers=num_workers, rank=rank, seed=seed)
    if num_workers > 0:
        kwargs.setdefault('multiprocessing_context', 'spawn')
    return DataLoader(dataset, batch_size=batch_size, sampler=sampler, num_workers=num_workers,
                      collate_fn=host_collate, pin_memory=False, worker_init_fn=init_fn, **kwargs)
