#!/usr/bin/env python
"""Generate the Pascal VOC fixtures by running the REFERENCE's own core/evaluation/mean_ap.py, bbox_overlaps.py,
class_names.py and datasets/custom.py, xml_style.py, voc.py, dataset_wrappers.py and builder.py (loaded by file path,
with make_golden's mmcv stand-in, make_golden_dataset's stubs, a stub `terminaltables` and a serial stand-in for
multiprocessing.Pool).  Only recorded outputs and data files are written:

  tests/golden/voc_mini/      a small VOCdevkit (VOC2007 and VOC2012): XML files, ImageSets lists and the one JPEG
                              of the image whose XML has no <size>; difficult, small and out-of-class objects
  tests/golden/voc_dataset.npz  what the reference's VOCDataset, wrappers and build_dataset make of voc_mini: infos,
                              annotation arrays, kept images, flags, cat ids, wrapper lengths / flags / index maps,
                              ClassBalancedDataset repeat indices for several thresholds
  tests/golden/voc0712_cfg.json  the reference's htd_resnet50_1x.py with voc0712.py's data / evaluation, 20-class
                              heads and the VOC schedule, merged as INTEGRATION.md's recipe does it

  tests/golden/voc_eval.npz   eval_map on seeded sets with distinct scores: 'area' and VOC07 '11points' modes, ignored
                              ground truths, images without ground truth, a class without detections and one without
                              ground truth, two scale ranges in both modes, iou_thr 0.5 and 0.7; the inputs too

    python tests/golden/make_golden_voc.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
from voc_eval_np import drop_class, pack_inputs, pack_result, synthetic_voc  # noqa: E402

EVAL_DIR = os.path.join(make_golden.REF, 'mmdet', 'core', 'evaluation')
DATASETS_DIR = os.path.join(make_golden.REF, 'mmdet', 'datasets')


class _SerialPool:
    def __init__(self, *a, **k):
        pass

    def starmap(self, fn, args):
        return [fn(*a) for a in args]

    def close(self):
        pass


def load_reference_mean_ap():
    make_golden.install_mmcv_standin()
    sys.modules['mmcv'].is_str = lambda x: isinstance(x, str)
    tt = types.ModuleType('terminaltables')
    tt.AsciiTable = lambda data: types.SimpleNamespace(table='')
    sys.modules['terminaltables'] = tt
    pkg = types.ModuleType('ref_evaluation')
    pkg.__path__ = [EVAL_DIR]
    sys.modules['ref_evaluation'] = pkg
    mods = {}
    for name in ('bbox_overlaps', 'class_names', 'mean_ap'):
        spec = importlib.util.spec_from_file_location('ref_evaluation.' + name, os.path.join(EVAL_DIR, name + '.py'))
        m = importlib.util.module_from_spec(spec)
        sys.modules['ref_evaluation.' + name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    mods['mean_ap'].Pool = _SerialPool
    return mods


CASES = {
    # name: (synthetic_voc kwargs, drop_class kwargs, eval_map kwargs)
    'area': (dict(n_img=40, n_cls=6, dets_per_img=30, seed=1, empty_every=7), dict(no_dets=(4,), no_gts=(5,)),
             dict()),
    'voc07': (dict(n_img=40, n_cls=6, dets_per_img=30, seed=1, empty_every=7), dict(no_dets=(4,), no_gts=(5,)),
              dict(dataset='voc07')),
    'area_iou07': (dict(n_img=30, n_cls=5, dets_per_img=40, seed=2, empty_every=5), dict(), dict(iou_thr=0.7)),
    'voc07_iou07': (dict(n_img=30, n_cls=5, dets_per_img=40, seed=2, empty_every=5), dict(), dict(iou_thr=0.7,
                                                                                                  dataset='voc07')),
    'area_scales': (dict(n_img=30, n_cls=5, dets_per_img=40, seed=3, empty_every=6), dict(no_dets=(2,)),
                    dict(scale_ranges=[(0, 96), (96, 1e5)])),
    'voc07_scales': (dict(n_img=30, n_cls=5, dets_per_img=40, seed=3, empty_every=6), dict(no_dets=(2,)),
                     dict(scale_ranges=[(0, 96), (96, 1e5)], dataset='voc07')),
    'no_ignore_key': (dict(n_img=12, n_cls=3, dets_per_img=20, seed=4, ignore_frac=0.0), dict(), dict()),
}


# (image id, size or None, [(name, difficult, xmin, ymin, xmax, ymax)])
VOC_MINI = {
    2007: {'trainval': [
        ('000005', (500, 375), [('chair', 0, 263, 211, 324, 339), ('chair', 0, 165, 264, 253, 372),
                                ('chair', 1, 5, 244, 67, 374), ('unicorn', 0, 1, 1, 40, 40)]),
        ('000007', (500, 333), [('car', 0, 141.5, 50.2, 500, 330.9)]),
        ('000009', None, [('horse', 0, 69, 172, 270, 330), ('person', 0, 150, 141, 229, 284),
                          ('person', 0, 285, 201, 327, 331), ('person', 0, 258, 198, 297, 329)]),
        ('000012', (500, 20), [('car', 0, 156, 1, 351, 19)]),
        ('000016', (334, 500), [('bicycle', 0, 92, 72, 305, 473), ('bird', 0, 10, 10, 22, 60)]),
        ('000017', (480, 364), [('unicorn', 0, 185, 62, 279, 199)]),
        ('000019', (500, 375), [('cat', 0, 231, 88, 483, 256), ('cat', 0, 11, 113, 266, 259)])],
        'test': [('000001', (353, 500), [('dog', 0, 48, 240, 195, 371), ('person', 0, 8, 12, 352, 498)]),
                 ('000002', (335, 500), [('train', 1, 139, 200, 207, 301)])]},
    2012: {'trainval': [
        ('2008_000002', (500, 375), [('tvmonitor', 0, 34, 11, 448, 293)]),
        ('2008_000003', (500, 333), [('train', 0, 46, 11, 500, 333), ('person', 1, 62, 190, 83, 243)]),
        ('2008_000007', (500, 375), [('bus', 0, 1, 74, 500, 375)]),
        ('2008_000008', (442, 500), [('horse', 0, 53, 87, 471, 420), ('person', 0, 158, 44, 289, 167)])]},
}
NO_SIZE_JPEG = (40, 30)


def write_voc_mini(root):
    from PIL import Image
    for year, sets in VOC_MINI.items():
        base = os.path.join(root, f'VOC{year}')
        for sub in ('Annotations', 'JPEGImages', 'ImageSets/Main'):
            os.makedirs(os.path.join(base, sub), exist_ok=True)
        for split, items in sets.items():
            with open(os.path.join(base, 'ImageSets', 'Main', split + '.txt'), 'w') as f:
                f.write(''.join(i + '\n' for i, _, _ in items))
            for img_id, size, objs in items:
                xml = ['<annotation>', f'  <filename>{img_id}.jpg</filename>']
                if size is None:
                    Image.new('RGB', NO_SIZE_JPEG, (90, 120, 30)).save(
                        os.path.join(base, 'JPEGImages', img_id + '.jpg'), quality=75)
                else:
                    xml.append(f'  <size><width>{size[0]}</width><height>{size[1]}</height><depth>3</depth></size>')
                for name, diff, x1, y1, x2, y2 in objs:
                    xml.append(f'  <object><name>{name}</name><difficult>{diff}</difficult><bndbox><xmin>{x1}</xmin>'
                               f'<ymin>{y1}</ymin><xmax>{x2}</xmax><ymax>{y2}</ymax></bndbox></object>')
                xml.append('</annotation>')
                with open(os.path.join(base, 'Annotations', img_id + '.xml'), 'w') as f:
                    f.write('\n'.join(xml) + '\n')


def load_reference_datasets():
    import make_golden_dataset
    mods = make_golden_dataset.load_reference()
    sys.modules['mmcv'].is_str = lambda x: isinstance(x, str)
    samplers = types.ModuleType('ref_datasets.samplers')
    samplers.GroupSampler = mods['group_sampler'].GroupSampler
    samplers.DistributedGroupSampler = mods['group_sampler'].DistributedGroupSampler
    samplers.DistributedSampler = mods['distributed_sampler'].DistributedSampler
    sys.modules['ref_datasets.samplers'] = samplers
    stub_builder = sys.modules['ref_datasets.builder']
    for name in ('xml_style', 'voc', 'dataset_wrappers'):
        spec = importlib.util.spec_from_file_location('ref_datasets.' + name,
                                                      os.path.join(DATASETS_DIR, name + '.py'))
        m = importlib.util.module_from_spec(spec)
        sys.modules['ref_datasets.' + name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    spec = importlib.util.spec_from_file_location('ref_datasets.builder_real', os.path.join(DATASETS_DIR, 'builder.py'))
    real = importlib.util.module_from_spec(spec)
    real.__package__ = 'ref_datasets'
    spec.loader.exec_module(real)
    real.DATASETS = stub_builder.DATASETS               # the registry the loaded dataset modules registered into
    mods['builder'] = real
    return mods


def _pack_ds(out, key, ds):
    out[key + '/ids'] = np.array([d['id'] for d in ds.data_infos])
    out[key + '/wh'] = np.array([[d['width'], d['height']] for d in ds.data_infos], np.int64).reshape(-1, 2)
    out[key + '/filenames'] = np.array([d['filename'] for d in ds.data_infos])
    out[key + '/flag'] = getattr(ds, 'flag', np.zeros(0, np.uint8))
    anns = [ds.get_ann_info(i) for i in range(len(ds))]
    for f in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
        out[f'{key}/{f}'] = np.concatenate([a[f] for a in anns])
        out[f'{key}/{f}_n'] = np.array([len(a[f]) for a in anns], np.int64)
    cats = [ds.get_cat_ids(i) for i in range(len(ds))]
    out[key + '/cat_ids'] = np.array(sum(cats, []), np.int64)
    out[key + '/cat_ids_n'] = np.array([len(c) for c in cats], np.int64)


def dataset_cases(mods, root, out):
    VOC = mods['voc'].VOCDataset
    for year in (2007, 2012):
        for test_mode in (True, False):
            for filt in (True, False):
                for cname, classes in (('all', None), ('subset', ('person', 'car', 'chair'))):
                    for min_size in ((None, 32) if not test_mode else (None, )):
                        ds = VOC(ann_file=f'{root}/VOC{year}/ImageSets/Main/trainval.txt', pipeline=[],
                                 img_prefix=f'{root}/VOC{year}/', test_mode=test_mode, filter_empty_gt=filt,
                                 classes=classes, min_size=min_size)
                        _pack_ds(out, f'{year}/{int(test_mode)}{int(filt)}_{cname}_{min_size}', ds)
    build = mods['builder'].build_dataset
    train = dict(type='VOCDataset', ann_file=[f'{root}/VOC2007/ImageSets/Main/trainval.txt',
                                              f'{root}/VOC2012/ImageSets/Main/trainval.txt'],
                 img_prefix=[f'{root}/VOC2007/', f'{root}/VOC2012/'], pipeline=[])
    rep = build(dict(type='RepeatDataset', times=3, dataset=train))
    cat = rep.dataset
    out['repeat/len'] = np.array(len(rep))
    out['repeat/flag'] = rep.flag
    out['repeat/ids'] = np.array([rep[i]['img_info']['id'] for i in range(len(rep))])
    out['repeat/cat_ids'] = np.array(sum([rep.get_cat_ids(i) for i in range(len(rep))], []), np.int64)
    out['concat/len'] = np.array(len(cat))
    out['concat/cumulative_sizes'] = np.array(cat.cumulative_sizes, np.int64)
    out['concat/flag'] = cat.flag
    out['concat/ids'] = np.array([cat[i]['img_info']['id'] for i in range(len(cat))])
    idx = list(range(-len(cat), len(cat)))
    out['concat/cat_idx'] = np.array(idx, np.int64)
    out['concat/cat_ids'] = np.array(sum([cat.get_cat_ids(i) for i in idx], []), np.int64)
    out['concat/cat_ids_n'] = np.array([len(cat.get_cat_ids(i)) for i in idx], np.int64)
    listed = build([dict(train, ann_file=train['ann_file'][i], img_prefix=train['img_prefix'][i]) for i in range(2)])
    out['list/ids'] = np.array([listed[i]['img_info']['id'] for i in range(len(listed))])
    base = VOC(ann_file=f'{root}/VOC2007/ImageSets/Main/trainval.txt', pipeline=[], img_prefix=f'{root}/VOC2007/',
               filter_empty_gt=False)
    CB = mods['dataset_wrappers'].ClassBalancedDataset
    for thr in (0.05, 0.2, 0.4, 0.7, 1.0):
        for filt in (True, False):
            cb = CB(base, thr, filter_empty_gt=filt)
            out[f'cb/{thr}/{int(filt)}/repeat_indices'] = np.array(cb.repeat_indices, np.int64)
            out[f'cb/{thr}/{int(filt)}/flag'] = cb.flag
    cb = build(dict(type='ClassBalancedDataset', oversample_thr=0.4, dataset=dict(
        type='VOCDataset', ann_file=f'{root}/VOC2007/ImageSets/Main/trainval.txt', img_prefix=f'{root}/VOC2007/',
        pipeline=[])))
    out['cb_built/repeat_indices'] = np.array(cb.repeat_indices, np.int64)


def voc0712_cfg():
    """INTEGRATION.md's recipe over the reference's own config files -> the merged settings (the reference's local
    data_root replaced by data/VOCdevkit/)."""
    from htd_amd.registry import Config
    cfg = Config.fromfile(os.path.join(make_golden.REF, 'configs', 'htd', 'htd_resnet50_1x.py'))
    voc = Config.fromfile(os.path.join(make_golden.REF, 'configs', '_base_', 'datasets', 'voc0712.py'))
    for head in cfg.model.roi_head.bbox_head:
        head.num_classes = 20
    cfg.data, cfg.evaluation = voc.data, voc.evaluation
    cfg.lr_config.step, cfg.total_epochs = [3], 4
    text = json.dumps(cfg._cfg_dict.to_dict()).replace(voc.data_root, 'data/VOCdevkit/')
    return json.loads(text)


def main():
    root = os.path.join(HERE, 'voc_mini')
    write_voc_mini(root)
    dmods = load_reference_datasets()
    dout = {}
    dataset_cases(dmods, root, dout)
    np.savez_compressed(os.path.join(HERE, 'voc_dataset.npz'), **dout)
    with open(os.path.join(HERE, 'voc0712_cfg.json'), 'w') as f:
        json.dump(voc0712_cfg(), f, indent=1, sort_keys=True)
    print('voc_dataset.npz:', len(dout), 'arrays')
    mods = load_reference_mean_ap()
    out = {}
    for name, (syn, drop, kw) in CASES.items():
        dets, anns = drop_class(*synthetic_voc(**syn), **drop)
        if name == 'no_ignore_key':
            anns = [dict(bboxes=a['bboxes'], labels=a['labels']) for a in anns]
            packed = pack_inputs(dets, [dict(a, bboxes_ignore=np.zeros((0, 4), np.float32),
                                             labels_ignore=np.zeros(0, np.int64)) for a in anns], name + '/')
            packed[name + '/no_ignore_key'] = np.array(True)
        else:
            packed = pack_inputs(dets, anns, name + '/')
        out.update(packed)
        res = mods['mean_ap'].eval_map(dets, anns, logger='silent', **kw)
        out.update(pack_result(*res, prefix=name + '/'))
        out[name + '/kwargs'] = np.array(repr(kw))
        print(name, res[0])
    out['voc_classes'] = np.array(mods['class_names'].get_classes('voc07'))
    out['coco_classes'] = np.array(mods['class_names'].get_classes('coco'))
    np.savez_compressed(os.path.join(HERE, 'voc_eval.npz'), **out)


if __name__ == '__main__':
    main()
