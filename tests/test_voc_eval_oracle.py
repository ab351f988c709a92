"""CPU: the numpy restatement of mean_ap.py:eval_map (tests/voc_eval_np.py) equals the reference's own output
(tests/golden/voc_eval.npz) bit for bit, and the host parts of htd_amd's VOC evaluation (class names, argument
refusals, the summary table)."""
import ast
import os

import numpy as np
import pytest

from voc_eval_np import assert_matches_packed, eval_map_np, unpack_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('area', 'voc07', 'area_iou07', 'voc07_iou07', 'area_scales', 'voc07_scales', 'no_ignore_key')


def load_case(name):
    z = np.load(os.path.join(GOLDEN, 'voc_eval.npz'))
    dets, anns = unpack_inputs(z, name + '/')
    if name + '/no_ignore_key' in z:
        anns = [dict(bboxes=a['bboxes'], labels=a['labels']) for a in anns]
    return z, dets, anns, ast.literal_eval(str(z[name + '/kwargs']))


@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_reference(name):
    z, dets, anns, kw = load_case(name)
    assert_matches_packed(eval_map_np(dets, anns, **kw), z, name + '/')


def test_scale_division_quirk_pinned():
    # mean_ap.py divides the whole ap array by 11 inside its loop over scales: scale 0 of two is divided twice
    z, dets, anns, kw = load_case('voc07_scales')
    _, res = eval_map_np(dets, anns, **kw)
    once = dict(kw, scale_ranges=kw['scale_ranges'][:1])
    _, single = eval_map_np(dets, anns, **once)
    for a, b in zip(res, single):
        assert a['ap'][0] == np.float32(b['ap'][0] / np.float32(11))


def test_class_names():
    from htd_amd.core.evaluation import get_classes, voc_classes
    z = np.load(os.path.join(GOLDEN, 'voc_eval.npz'))
    assert voc_classes() == list(z['voc_classes'])
    for alias in ('voc', 'voc07', 'voc12', 'pascal_voc'):
        assert get_classes(alias) == voc_classes()
    for alias in ('coco', 'mscoco', 'ms_coco'):
        assert get_classes(alias) == list(z['coco_classes'])
    with pytest.raises(NotImplementedError):
        get_classes('cityscapes')
    with pytest.raises(ValueError):
        get_classes('nope')
    with pytest.raises(TypeError):
        get_classes(['a'])


def test_refusals():
    from htd_amd.core.evaluation import eval_map
    _, dets, anns, _ = load_case('area')
    with pytest.raises(NotImplementedError):
        eval_map(dets, anns, tpfp_fn=lambda *a: None)
    for ds in ('det', 'vid'):
        with pytest.raises(NotImplementedError):
            eval_map(dets, anns, dataset=ds)


def test_summary_table(capsys):
    from htd_amd.core.evaluation import print_map_summary
    z, dets, anns, kw = load_case('voc07')
    mean_ap, res = eval_map_np(dets, anns, **kw)
    print_map_summary(mean_ap, res, dataset=('a', 'b', 'c', 'd', 'e', 'f'))
    out = capsys.readouterr().out
    assert out.splitlines()[1].split(' | ')[0].strip() == 'class'
    assert 'mAP' in out and f'{mean_ap:.3f}' in out
    print_map_summary(mean_ap, res, dataset='voc07')
    assert 'aeroplane' in capsys.readouterr().out
