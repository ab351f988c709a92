"""CocoDataset, the samplers, the data loader's workers, the `data` section of htd_config and the test CLI's argument
checks (CPU).  The recorded values come from the reference's own dataset and sampler code
(tests/golden/make_golden_dataset.py)."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ANN = os.path.join(GOLDEN, 'coco_dataset_ann.json')
SUBSET = ('dog', 'car')


@pytest.fixture(scope='module')
def rec():
    return np.load(os.path.join(GOLDEN, 'coco_dataset.npz'))


def _split(flat, counts):
    return np.split(flat, np.cumsum(counts)[:-1]) if len(counts) else []


@pytest.mark.parametrize('test_mode', [True, False])
@pytest.mark.parametrize('filter_empty_gt', [True, False])
@pytest.mark.parametrize('cname', ['all', 'subset'])
def test_coco_dataset_matches_reference(rec, test_mode, filter_empty_gt, cname):
    from htd_amd.datasets import CocoDataset
    key = f'{int(test_mode)}{int(filter_empty_gt)}_{cname}'
    ds = CocoDataset(ANN, [], classes=SUBSET if cname == 'subset' else None, test_mode=test_mode,
                     filter_empty_gt=filter_empty_gt)
    assert ds.img_ids == rec[key + '/img_ids'].tolist()
    assert ds.cat_ids == rec[key + '/cat_ids'].tolist()
    assert [d['id'] for d in ds.data_infos] == rec[key + '/kept_ids'].tolist()
    if test_mode:
        assert not hasattr(ds, 'flag')
    else:
        assert ds.flag.dtype == np.uint8 and np.array_equal(ds.flag, rec[key + '/flag'])
    anns = [ds.get_ann_info(i) for i in range(len(ds))]
    for f in ('bboxes', 'labels', 'bboxes_ignore'):
        want = _split(rec[f'{key}/{f}'], rec[f'{key}/{f}_n'])
        assert len(want) == len(anns)
        for a, w in zip(anns, want):
            assert a[f].dtype == (np.int64 if f == 'labels' else np.float32)
            assert a[f].shape[0] == w.shape[0] and np.array_equal(a[f].reshape(w.shape), w), (f, a[f], w)
    assert [len(ds.get_cat_ids(i)) for i in range(len(ds))] == rec[key + '/cat_of'].tolist()
    assert ds.evaluator.img_ids == ds.img_ids and ds.evaluator.cat_ids == ds.cat_ids


def test_coco_dataset_paths_classes_and_samples(tmp_path):
    from htd_amd.datasets import CocoDataset, build_dataset
    names = tmp_path / 'names.txt'
    names.write_text('dog\ncar\n')
    ds = build_dataset(dict(type='CocoDataset', ann_file='coco_dataset_ann.json', data_root=GOLDEN + '/',
                            img_prefix='imgs/', classes=str(names), pipeline=[]))
    assert ds.ann_file == ANN and ds.img_prefix == GOLDEN + '/imgs/' and list(ds.CLASSES) == list(SUBSET)
    ds2 = CocoDataset(ANN, [], data_root='/elsewhere', img_prefix='/abs/')
    assert ds2.img_prefix == '/abs/' and ds2.ann_file == ANN
    s = ds[0]                                   # an empty pipeline returns the prepared dict
    assert s['img_prefix'] == GOLDEN + '/imgs/' and s['bbox_fields'] == [] and s['img_info']['filename'] == '000042.jpg'
    assert np.array_equal(s['ann_info']['bboxes'], ds.get_ann_info(0)['bboxes'])
    t = CocoDataset(ANN, [], test_mode=True)[3]
    assert 'ann_info' not in t and t['img_info']['id'] == 5
    with pytest.raises(ValueError, match='proposal_file'):
        CocoDataset(ANN, [], proposal_file='p.pkl')
    with pytest.raises(ValueError):
        CocoDataset(ANN, [], classes=3)


def test_train_mode_retries_refused_samples():
    """A sample the pipeline refuses is replaced by a random one of the same flag group (np.random)."""
    from htd_amd.datasets import CocoDataset

    class RefuseFirst:
        def __call__(self, results):
            return None if results['img_info']['id'] == 42 else results
    ds = CocoDataset(ANN, [RefuseFirst()], test_mode=False)
    np.random.seed(3)
    out = ds[0]
    np.random.seed(3)
    pool = np.flatnonzero(ds.flag == ds.flag[0])
    expect = None
    while expect is None or expect == 0:
        expect = int(np.random.choice(pool))
    assert ds.flag[0] == 1 and out['img_info']['id'] == ds.data_infos[expect]['id']


class _Flagged:
    def __init__(self, flag):
        self.flag = np.asarray(flag, np.uint8)

    def __len__(self):
        return len(self.flag)


FLAGS = {'mixed': [1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1], 'one_group': [1] * 7, 'zeros': [0] * 5}


@pytest.mark.parametrize('fname', sorted(FLAGS))
@pytest.mark.parametrize('spg', [1, 2, 3])
def test_samplers_match_reference(rec, fname, spg):
    from htd_amd.datasets import DistributedGroupSampler, GroupSampler
    data = _Flagged(FLAGS[fname])
    for seed in (0, 1, 7):
        np.random.seed(seed)
        s = GroupSampler(data, spg)
        got = list(s)
        assert got == rec[f'group/{fname}/{spg}/{seed}'].tolist() and len(s) == len(got)
    for world in (1, 2, 3):
        for rank in range(world):
            s = DistributedGroupSampler(data, spg, world, rank)
            for epoch in (0, 1, 5):
                s.set_epoch(epoch)
                got = list(s)
                assert got == rec[f'dgroup/{fname}/{spg}/{world}/{rank}/{epoch}'].tolist() and len(s) == len(got)


def test_distributed_sampler_matches_reference(rec):
    from htd_amd.datasets import DistributedSampler
    for n in (5, 7, 10):
        for world in (1, 2, 3):
            for rank in range(world):
                s = DistributedSampler(list(range(n)), world, rank, shuffle=False)
                got = list(s)
                assert got == rec[f'dist/{n}/{world}/{rank}'].tolist() and len(s) == len(got)


# ------------------------------------------------------------------------------------------- loader workers
class Probe:
    """Last transform: what the process that ran the pipeline sees of the GPU."""

    def __call__(self, data):
        with open('/proc/self/maps') as f:
            lib_mapped = 'libhtd_amd.so' in f.read()
        data['probe'] = dict(pid=os.getpid(), cuda_init=torch.cuda.is_initialized(), lib_mapped=lib_mapped)
        return data


def write_png_set(root, shapes, seed=0):
    """PNG images of the given (h, w) and a COCO json over them (one person box per image, the 80 COCO categories);
    -> ann file path."""
    from PIL import Image
    from htd_amd.coco import COCO_CLASSES
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, 'imgs'), exist_ok=True)
    images, anns = [], []
    for i, (h, w) in enumerate(shapes):
        name = f'{i:06d}.png'
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, 'imgs', name))
        images.append(dict(id=i + 1, file_name=name, width=w, height=h))
        anns.append(dict(id=100 + i, image_id=i + 1, category_id=1, bbox=[2.0, 3.0, w / 2, h / 3], area=w * h / 6.0,
                         iscrowd=0))
    path = os.path.join(root, 'ann.json')
    with open(path, 'w') as f:
        json.dump(dict(images=images, annotations=anns,
                       categories=[dict(id=i + 1, name=c) for i, c in enumerate(COCO_CLASSES)]), f)
    return path


def png_test_pipeline(scale=(96, 64)):
    from htd_amd.configs import IMG_NORM_CFG
    return [dict(type='LoadImageFromFile'),
            dict(type='MultiScaleFlipAug', img_scale=scale, flip=False,
                 transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                             dict(type='Normalize', **IMG_NORM_CFG), dict(type='Pad', size_divisor=32),
                             dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]


def _same_sample(a, b):
    assert a['img_metas'][0]['filename'] == b['img_metas'][0]['filename']
    for x, y in zip(a['img'], b['img']):
        assert np.array_equal(x.raw, y.raw) and x.out_hw == y.out_hw and x.pad_hw == y.pad_hw and x.norm[2] == y.norm[2]
    for ma, mb in zip(a['img_metas'], b['img_metas']):
        assert ma.keys() == mb.keys()
        for k in ma:
            assert np.array_equal(np.asarray(ma[k]), np.asarray(mb[k])) if k != 'img_norm_cfg' else True


def test_spawned_workers_yield_the_same_samples_and_never_touch_the_gpu(tmp_path):
    from htd_amd.datasets import build_dataloader, build_dataset
    ann = write_png_set(str(tmp_path), [(40, 60), (60, 40), (50, 50), (33, 70), (70, 33)])
    ds = build_dataset(dict(type='CocoDataset', ann_file=ann, img_prefix=str(tmp_path / 'imgs'),
                            pipeline=png_test_pipeline(), test_mode=True))
    ds.pipeline.transforms.append(Probe())
    inline = [b for b in build_dataloader(ds, 2, 0, dist=False, shuffle=False)]
    spawned = [b for b in build_dataloader(ds, 2, 2, dist=False, shuffle=False)]
    assert [len(b) for b in inline] == [len(b) for b in spawned] == [2, 2, 1]
    for bi, bs in zip(inline, spawned):
        for a, b in zip(bi, bs):
            _same_sample(a, b)
            assert b['probe']['pid'] != os.getpid()
            assert not b['probe']['cuda_init'] and not b['probe']['lib_mapped']
    assert {b['probe']['pid'] for batch in spawned for b in batch}.__len__() == 2


def test_train_loader_seeds_and_groups(tmp_path):
    from htd_amd.datasets import GroupSampler, build_dataloader, build_dataset, worker_init_fn
    ann = write_png_set(str(tmp_path), [(40, 60), (60, 40), (50, 50), (33, 70), (70, 33), (44, 66)])
    ds = build_dataset(dict(type='CocoDataset', ann_file=ann, img_prefix=str(tmp_path / 'imgs'), pipeline=[]))
    dl = build_dataloader(ds, 2, 0, dist=False, shuffle=True, seed=5)
    assert isinstance(dl.sampler, GroupSampler)
    np.random.seed(11)
    batches = [[s['img_info']['id'] for s in b] for b in dl]
    for b in batches:                                       # one aspect-ratio group per batch
        assert len({int(ds.flag[ds.img_ids.index(i)]) for i in b}) == 1
    worker_init_fn(1, num_workers=4, rank=2, seed=5)
    a = np.random.rand()
    np.random.seed(4 * 2 + 1 + 5)
    assert a == np.random.rand()


# ------------------------------------------------------------------------------------------- config / CLI
def _without_paths(data):
    data = json.loads(json.dumps(data))
    for split in ('train', 'val', 'test'):
        data[split].pop('ann_file')
        data[split].pop('img_prefix')
    return data


@pytest.mark.parametrize('name,kw', [('htd_resnet50_1x', dict(depth=50)), ('htd_resnet101_2x', dict(depth=101)),
                                     ('htd_resnet101_2x_mstrain', dict(depth=101)),
                                     ('htd_resnet101_dcn_2x_mstrain', dict(depth=101, dcn=True)),
                                     ('htd_resnetx101_dcn_2x_mstrain', dict(depth=101, dcn=True, resnext=True))])
def test_htd_config_data_section(name, kw):
    from htd_amd.configs import htd_config
    with open(os.path.join(GOLDEN, 'htd_data_cfgs.json')) as f:
        rec = json.load(f)[name]
    cfg = htd_config(**kw)
    assert _without_paths(cfg.data.to_dict()) == rec['data']
    assert json.loads(json.dumps(cfg.evaluation.to_dict())) == rec['evaluation']
    assert cfg.data.test.ann_file.endswith('instances_val2017.json')


def test_replace_image_to_tensor():
    from htd_amd.datasets import replace_ImageToTensor
    p = png_test_pipeline()
    with pytest.warns(UserWarning):
        q = replace_ImageToTensor(p)
    assert q[1]['transforms'][4] == {'type': 'DefaultFormatBundle'} and p[1]['transforms'][4]['type'] == 'ImageToTensor'
    assert q[1]['transforms'][:4] == p[1]['transforms'][:4] and q[0] == p[0]


def test_cli_arguments():
    from htd_amd.test import parse_args
    with pytest.raises(ValueError, match='--eval and --format_only'):
        parse_args(['c.py', 'm.pth', '--eval', 'bbox', '--format-only'])
    with pytest.raises(ValueError, match='pkl'):
        parse_args(['c.py', 'm.pth', '--out', 'r.json'])
    with pytest.raises(SystemExit):
        parse_args(['c.py', 'm.pth'])
    a = parse_args(['c.py', 'm.pth', '--eval', 'bbox', 'proposal_fast', '--eval-options', 'classwise=True',
                    'proposal_nums=(1,10)', 'jsonfile_prefix=/tmp/x', '--cfg-options', 'data.test.img_prefix=d/',
                    'data.workers_per_gpu=0'])
    assert a.eval == ['bbox', 'proposal_fast'] and a.launcher == 'none'
    assert a.eval_options == dict(classwise=True, proposal_nums=(1, 10), jsonfile_prefix='/tmp/x')
    assert a.cfg_options == {'data.test.img_prefix': 'd/', 'data.workers_per_gpu': 0}
