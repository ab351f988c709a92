"""CPU: the Pascal VOC datasets (XMLDataset, VOCDataset), the fork's COCO-format types, the dataset wrappers and
build_dataset on a small VOCdevkit written by the test, and htd_config(dataset='voc0712')."""
import math
import os

import numpy as np
import pytest

PIPE = []
# (image id, size or None, [(name, difficult, xmin, ymin, xmax, ymax)])
VOC07 = [
    ('000001', (353, 500), [('dog', 0, 48, 240, 195, 371), ('person', 0, 8, 12, 352, 498)]),
    ('000002', (335, 500), [('train', 0, 139, 200, 207, 301)]),
    ('000003', None, [('sofa', 0, 123, 155, 215, 195), ('chair', 1, 239, 156, 307, 205),
                      ('chair', 0, 255.7, 150.2, 290.9, 199.8)]),
    ('000004', (20, 500), [('car', 0, 5, 5, 15, 15)]),                 # too narrow: dropped in train mode
    ('000005', (500, 375), [('unicorn', 0, 1, 1, 50, 50)]),            # no object of CLASSES
    ('000006', (500, 333), [('bird', 0, 10, 10, 18, 60), ('bird', 0, 100, 100, 300, 300)]),
]
VOC12 = [
    ('2008_000001', (500, 375), [('cat', 0, 30, 40, 200, 300), ('cat', 1, 1, 1, 30, 30)]),
    ('2008_000002', (375, 500), [('horse', 0, 50, 60, 250, 400)]),
]


def _write_split(root, year, items):
    from PIL import Image
    base = os.path.join(root, f'VOC{year}')
    for sub in ('Annotations', 'JPEGImages', 'ImageSets/Main'):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    for img_id, size, objs in items:
        xml = ['<annotation>', f'<filename>{img_id}.jpg</filename>']
        if size is not None:
            xml.append(f'<size><width>{size[0]}</width><height>{size[1]}</height><depth>3</depth></size>')
        else:
            Image.new('RGB', (400, 300), (90, 120, 30)).save(os.path.join(base, 'JPEGImages', f'{img_id}.jpg'))
        for name, diff, x1, y1, x2, y2 in objs:
            xml.append(f'<object><name>{name}</name><difficult>{diff}</difficult><bndbox><xmin>{x1}</xmin>'
                       f'<ymin>{y1}</ymin><xmax>{x2}</xmax><ymax>{y2}</ymax></bndbox></object>')
        xml.append('</annotation>')
        with open(os.path.join(base, 'Annotations', f'{img_id}.xml'), 'w') as f:
            f.write('\n'.join(xml))
    with open(os.path.join(base, 'ImageSets/Main/trainval.txt'), 'w') as f:
        f.write(''.join(i + '\n' for i, _, _ in items))
    return base


@pytest.fixture()
def devkit(tmp_path):
    root = str(tmp_path / 'VOCdevkit')
    _write_split(root, 2007, VOC07)
    _write_split(root, 2012, VOC12)
    return root + '/'


def voc(devkit, year=2007, **kw):
    from htd_amd.datasets import build_dataset
    cfg = dict(type='VOCDataset', ann_file=f'{devkit}VOC{year}/ImageSets/Main/trainval.txt',
               img_prefix=f'{devkit}VOC{year}/', pipeline=PIPE)
    cfg.update(kw)
    return build_dataset(cfg)


def test_infos_and_filters(devkit):
    ds = voc(devkit, test_mode=True)
    assert [d['id'] for d in ds.data_infos] == [i for i, _, _ in VOC07]
    assert ds.data_infos[0] == dict(id='000001', filename='JPEGImages/000001.jpg', width=353, height=500)
    assert (ds.data_infos[2]['width'], ds.data_infos[2]['height']) == (400, 300)     # no <size>: from the JPEG
    assert ds.year == 2007 and not hasattr(ds, 'flag')
    tr = voc(devkit)
    assert [d['id'] for d in tr.data_infos] == ['000001', '000002', '000003', '000006']
    assert tr.flag.dtype == np.uint8 and tr.flag.tolist() == [0, 0, 1, 1]
    keep_empty = voc(devkit, filter_empty_gt=False)
    assert [d['id'] for d in keep_empty.data_infos] == ['000001', '000002', '000003', '000005', '000006']


def test_annotations(devkit):
    ds = voc(devkit, test_mode=True)
    a = ds.get_ann_info(2)
    assert a['bboxes'].dtype == np.float32 and a['labels'].dtype == np.int64
    assert a['bboxes'].tolist() == [[122, 154, 214, 194], [254, 149, 289, 198]]     # int(float(text)) - 1
    assert a['labels'].tolist() == [ds.CLASSES.index('sofa'), ds.CLASSES.index('chair')]
    assert a['bboxes_ignore'].tolist() == [[238, 155, 306, 204]] and a['labels_ignore'].tolist() == [8]
    e = ds.get_ann_info(4)                                       # only an object outside CLASSES
    assert e['bboxes'].shape == (0, 4) and e['bboxes'].dtype == np.float32 and e['labels'].dtype == np.int64
    assert e['bboxes_ignore'].shape == (0, 4) and e['labels_ignore'].shape == (0,)
    assert ds.get_cat_ids(0) == [11, 14] and ds.get_cat_ids(4) == []
    small = voc(devkit, min_size=20)
    b = small.get_ann_info(3)                                    # 000006: the 8-px-wide bird is ignored
    assert b['bboxes'].tolist() == [[99, 99, 299, 299]] and b['bboxes_ignore'].tolist() == [[9, 9, 17, 59]]
    with pytest.raises(AssertionError):
        voc(devkit, min_size=20, test_mode=True).get_ann_info(0)


def test_classes_year_and_refusals(devkit, tmp_path):
    ds = voc(devkit, test_mode=True, classes=('dog', 'bird'))
    assert ds.CLASSES == ('dog', 'bird')
    assert ds.get_ann_info(0)['labels'].tolist() == [0] and ds.get_cat_ids(5) == [1, 1]
    assert voc(devkit, year=2012, test_mode=True).year == 2012
    with pytest.raises(ValueError):
        voc(devkit, proposal_file='p.pkl')
    os.symlink(devkit + 'VOC2007', devkit + 'VOCother')
    from htd_amd.datasets import build_dataset
    with pytest.raises(ValueError, match='year'):
        build_dataset(dict(type='VOCDataset', ann_file=f'{devkit}VOCother/ImageSets/Main/trainval.txt',
                           img_prefix=f'{devkit}VOCother/', pipeline=PIPE))


def test_data_root(devkit):
    ds = voc(devkit, data_root=devkit, ann_file='VOC2007/ImageSets/Main/trainval.txt', img_prefix='VOC2007/')
    assert ds.img_prefix == devkit + 'VOC2007/' and len(ds) == 4


def test_list_ann_file_repeat_and_samplers(devkit):
    from htd_amd.datasets import ConcatDataset, GroupSampler, RepeatDataset, build_dataset
    cfg = dict(type='RepeatDataset', times=3, dataset=dict(
        type='VOCDataset', ann_file=[f'{devkit}VOC2007/ImageSets/Main/trainval.txt',
                                     f'{devkit}VOC2012/ImageSets/Main/trainval.txt'],
        img_prefix=[f'{devkit}VOC2007/', f'{devkit}VOC2012/'], pipeline=PIPE))
    ds = build_dataset(cfg)
    assert isinstance(ds, RepeatDataset) and isinstance(ds.dataset, ConcatDataset)
    cat = ds.dataset
    assert [d.year for d in cat.datasets] == [2007, 2012] and cat.separate_eval
    assert len(cat) == 6 and len(ds) == 18 and ds.CLASSES == cat.CLASSES == cat.datasets[0].CLASSES
    assert cat.flag.tolist() == [0, 0, 1, 1, 1, 0]
    assert ds.flag.tolist() == cat.flag.tolist() * 3
    assert cat.get_cat_ids(4) == [7, 7] and cat.get_cat_ids(-1) == [12] and ds.get_cat_ids(10) == [7, 7]
    with pytest.raises(ValueError):
        cat.get_cat_ids(-7)
    np.random.seed(0)
    order = list(GroupSampler(ds, 2))
    assert sorted(set(order)) == list(range(18)) and len(order) == 20          # each group of 9 padded to 10
    listed = build_dataset([dict(cfg['dataset'], ann_file=cfg['dataset']['ann_file'][i],
                                 img_prefix=cfg['dataset']['img_prefix'][i]) for i in range(2)])
    assert isinstance(listed, ConcatDataset) and len(listed) == 6


def test_concat_whole_refusals(devkit):
    from htd_amd.datasets import ConcatDataset, CocoDataset
    a, b = voc(devkit), voc(devkit, year=2012)
    whole = ConcatDataset([a, b], separate_eval=False)
    assert len(whole) == 6
    coco = CocoDataset.__new__(CocoDataset)
    coco.CLASSES = a.CLASSES
    coco.flag = a.flag
    coco.data_infos = a.data_infos
    with pytest.raises(NotImplementedError):
        ConcatDataset([a, coco], separate_eval=False)


def test_fork_coco_types():
    from htd_amd.datasets import DATASETS
    from htd_amd.core.evaluation import voc_classes
    assert tuple(voc_classes()) == DATASETS.get('VOCDataset_coco').CLASSES == DATASETS.get('VOCDataset').CLASSES
    assert DATASETS.get('DHD_Traffic').CLASSES == ('Pedestrian', 'Cyclist', 'Car', 'Truck', 'Van')
    assert DATASETS.get('EADDataset').CLASSES == ('specularity', 'saturation', 'artifact', 'blur', 'contrast',
                                                  'bubbles', 'instrument')
    for name in ('VOCDataset_coco', 'DHD_Traffic', 'EADDataset'):
        assert issubclass(DATASETS.get(name), DATASETS.get('CocoDataset'))


def test_voc_evaluate_refusals(devkit):
    ds = voc(devkit, test_mode=True)
    with pytest.raises(KeyError):
        ds.evaluate([], metric='bbox')


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MINI = os.path.join(GOLDEN, 'voc_mini')


@pytest.fixture(scope='module')
def ref():
    return np.load(os.path.join(GOLDEN, 'voc_dataset.npz'))


def _check_ds(z, key, ds):
    assert [d['id'] for d in ds.data_infos] == list(z[key + '/ids'])
    assert [[d['width'], d['height']] for d in ds.data_infos] == z[key + '/wh'].tolist()
    assert [d['filename'] for d in ds.data_infos] == list(z[key + '/filenames'])
    flag = getattr(ds, 'flag', np.zeros(0, np.uint8))
    assert flag.dtype == z[key + '/flag'].dtype and np.array_equal(flag, z[key + '/flag'])
    anns = [ds.get_ann_info(i) for i in range(len(ds))]
    for f in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
        got = np.concatenate([a[f] for a in anns])
        assert got.dtype == z[f'{key}/{f}'].dtype and np.array_equal(got, z[f'{key}/{f}']), (key, f)
        assert [len(a[f]) for a in anns] == z[f'{key}/{f}_n'].tolist(), (key, f)
        assert all(a[f].dtype == got.dtype for a in anns)
    cats = [ds.get_cat_ids(i) for i in range(len(ds))]
    assert sum(cats, []) == z[key + '/cat_ids'].tolist() and [len(c) for c in cats] == z[key + '/cat_ids_n'].tolist()


@pytest.mark.parametrize('year', [2007, 2012])
@pytest.mark.parametrize('test_mode,filt,min_size', [(True, True, None), (True, False, None), (False, True, None),
                                                     (False, False, None), (False, True, 32), (False, False, 32)])
@pytest.mark.parametrize('cname,classes', [('all', None), ('subset', ('person', 'car', 'chair'))])
def test_voc_dataset_equals_reference(ref, year, test_mode, filt, min_size, cname, classes):
    from htd_amd.datasets import VOCDataset
    ds = VOCDataset(ann_file=f'{MINI}/VOC{year}/ImageSets/Main/trainval.txt', pipeline=[],
                    img_prefix=f'{MINI}/VOC{year}/', test_mode=test_mode, filter_empty_gt=filt, classes=classes,
                    min_size=min_size)
    _check_ds(ref, f'{year}/{int(test_mode)}{int(filt)}_{cname}_{min_size}', ds)


def test_wrappers_equal_reference(ref):
    from htd_amd.datasets import build_dataset
    train = dict(type='VOCDataset', ann_file=[f'{MINI}/VOC2007/ImageSets/Main/trainval.txt',
                                              f'{MINI}/VOC2012/ImageSets/Main/trainval.txt'],
                 img_prefix=[f'{MINI}/VOC2007/', f'{MINI}/VOC2012/'], pipeline=[])
    rep = build_dataset(dict(type='RepeatDataset', times=3, dataset=train))
    cat = rep.dataset
    assert len(rep) == int(ref['repeat/len']) and np.array_equal(rep.flag, ref['repeat/flag'])
    assert [rep[i]['img_info']['id'] for i in range(len(rep))] == list(ref['repeat/ids'])
    assert sum([rep.get_cat_ids(i) for i in range(len(rep))], []) == ref['repeat/cat_ids'].tolist()
    assert len(cat) == int(ref['concat/len']) and cat.cumulative_sizes == ref['concat/cumulative_sizes'].tolist()
    assert cat.flag.dtype == ref['concat/flag'].dtype and np.array_equal(cat.flag, ref['concat/flag'])
    assert [cat[i]['img_info']['id'] for i in range(len(cat))] == list(ref['concat/ids'])
    idx = ref['concat/cat_idx'].tolist()
    assert sum([cat.get_cat_ids(i) for i in idx], []) == ref['concat/cat_ids'].tolist()
    assert [len(cat.get_cat_ids(i)) for i in idx] == ref['concat/cat_ids_n'].tolist()
    listed = build_dataset([dict(train, ann_file=train['ann_file'][i], img_prefix=train['img_prefix'][i])
                            for i in range(2)])
    assert [listed[i]['img_info']['id'] for i in range(len(listed))] == list(ref['list/ids'])


@pytest.mark.parametrize('thr', [0.05, 0.2, 0.4, 0.7, 1.0])
@pytest.mark.parametrize('filt', [True, False])
def test_class_balanced_equals_reference(ref, thr, filt):
    from htd_amd.datasets import ClassBalancedDataset, VOCDataset
    base = VOCDataset(ann_file=f'{MINI}/VOC2007/ImageSets/Main/trainval.txt', pipeline=[],
                      img_prefix=f'{MINI}/VOC2007/', filter_empty_gt=False)
    cb = ClassBalancedDataset(base, thr, filter_empty_gt=filt)
    assert cb.repeat_indices == ref[f'cb/{thr}/{int(filt)}/repeat_indices'].tolist()
    assert cb.flag.dtype == np.uint8 and np.array_equal(cb.flag, ref[f'cb/{thr}/{int(filt)}/flag'])
    assert len(cb) == len(cb.repeat_indices)


def test_class_balanced_built_equals_reference(ref):
    from htd_amd.datasets import build_dataset
    cb = build_dataset(dict(type='ClassBalancedDataset', oversample_thr=0.4, dataset=dict(
        type='VOCDataset', ann_file=f'{MINI}/VOC2007/ImageSets/Main/trainval.txt', img_prefix=f'{MINI}/VOC2007/',
        pipeline=[])))
    assert cb.repeat_indices == ref['cb_built/repeat_indices'].tolist()


def _voc0712_ref():
    import json
    with open(os.path.join(GOLDEN, 'voc0712_cfg.json')) as f:
        return json.load(f)


def test_htd_config_voc0712_equals_reference_merge():
    import json
    from htd_amd.configs import htd_config
    want = _voc0712_ref()
    cfg = json.loads(json.dumps(htd_config(50, dataset='voc0712').to_dict()))       # tuples as JSON lists
    assert cfg['data'] == want['data']
    assert cfg['evaluation'] == want['evaluation']
    assert cfg['model']['roi_head']['bbox_head'] == want['model']['roi_head']['bbox_head']
    assert cfg['lr_config']['step'] == want['lr_config']['step'] == [3]
    assert cfg['total_epochs'] == want['total_epochs'] == 4


def test_integration_recipe_builds(tmp_path, monkeypatch):
    """INTEGRATION.md's VOC recipe, run over stand-ins of the reference's two config files, writes a config that
    loads back to the reference merge and builds a 20-class detector."""
    from htd_amd.configs import build_htd_detector, htd_data
    from htd_amd.registry import Config
    from htd_amd.train import dump_config
    want = _voc0712_ref()
    root = os.path.dirname(GOLDEN.rstrip('/'))
    with open(os.path.join(os.path.dirname(root), 'INTEGRATION.md')) as f:
        text = f.read()
    code = text.split('<!-- voc0712-recipe -->\n```python\n', 1)[1].split('```', 1)[0]
    os.makedirs(tmp_path / 'configs' / 'htd')
    os.makedirs(tmp_path / 'configs' / '_base_' / 'datasets')
    coco = {k: v for k, v in want.items() if k not in ('data', 'evaluation')}
    coco['model'] = _with_classes(coco['model'], 80)
    coco.update(data=htd_data(50), evaluation=dict(interval=1, metric='bbox'),
                lr_config=dict(coco['lr_config'], step=[8, 11]), total_epochs=12)
    dump_config(Config(coco), str(tmp_path / 'configs' / 'htd' / 'htd_resnet50_1x.py'))
    dump_config(Config(dict(data=want['data'], evaluation=want['evaluation'], data_root='data/VOCdevkit/')),
                str(tmp_path / 'configs' / '_base_' / 'datasets' / 'voc0712.py'))
    monkeypatch.chdir(tmp_path)
    exec(compile(code, 'INTEGRATION.md', 'exec'), {})
    got = Config.fromfile(str(tmp_path / 'configs' / 'htd' / 'htd_resnet50_voc0712.py'))
    assert got._cfg_dict.to_dict() == want
    got.model.pretrained = None                        # no ImageNet weights to fetch here
    det = build_htd_detector(cfg=got)
    assert [h.num_classes for h in det.roi_head.bbox_head] == [20, 20]
    assert [type(h).__name__ for h in det.roi_head.bbox_head] == ['Shared2FCBBoxHead', 'HTDBBoxHead']


def _with_classes(model, n):
    import copy
    model = copy.deepcopy(model)
    for h in model['roi_head']['bbox_head']:
        h['num_classes'] = n
    return model


def test_htd_config_voc0712():
    from htd_amd.configs import htd_config
    cfg = htd_config(50, dataset='voc0712')
    assert [h.num_classes for h in cfg.model.roi_head.bbox_head] == [20, 20]
    assert cfg.evaluation == dict(interval=1, metric='mAP')
    assert cfg.lr_config.step == [3] and cfg.total_epochs == 4
    tr = cfg.data.train
    assert tr.type == 'RepeatDataset' and tr.times == 3 and tr.dataset.type == 'VOCDataset'
    assert [os.path.basename(os.path.dirname(p.rstrip('/'))) for p in tr.dataset.img_prefix] == ['VOCdevkit'] * 2
    assert [p.split('/')[-2] for p in tr.dataset.img_prefix] == ['VOC2007', 'VOC2012']
    assert [p.split('/')[-4:] for p in tr.dataset.ann_file] == [['VOC2007', 'ImageSets', 'Main', 'trainval.txt'],
                                                               ['VOC2012', 'ImageSets', 'Main', 'trainval.txt']]
    assert tr.dataset.pipeline[2]['type'] == 'Resize' and tr.dataset.pipeline[2]['img_scale'] == (1000, 600)
    for split in ('val', 'test'):
        s = cfg.data[split]
        assert s.type == 'VOCDataset' and s.ann_file.endswith('VOC2007/ImageSets/Main/test.txt')
        assert s.pipeline[1]['img_scale'] == (1000, 600)
    assert cfg.data.samples_per_gpu == 2 and cfg.data.workers_per_gpu == 2
    coco = htd_config(50)
    assert coco.data.train.type == 'CocoDataset' and coco.evaluation.metric == 'bbox'
    assert [h.num_classes for h in coco.model.roi_head.bbox_head] == [80, 80]
    with pytest.raises(ValueError):
        htd_config(50, dataset='nope')
