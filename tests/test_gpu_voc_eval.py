"""Pascal VOC mean AP on the device (csrc/voc_eval.hip through htd_amd.core.evaluation.eval_map) against the
reference's own output (tests/golden/voc_eval.npz) and the numpy restatement (tests/voc_eval_np.py), bit for bit."""
import numpy as np
import pytest
import torch

from test_voc_eval_oracle import CASES, load_case
from voc_eval_np import assert_matches_packed, assert_same_result, eval_map_np, synthetic_voc

pytestmark = pytest.mark.gpu


def _triple(dets):
    from htd_amd.apis import results_to_tensors
    return tuple(t.cuda() for t in results_to_tensors(dets))


@pytest.mark.parametrize('name', CASES)
def test_reference_fixtures(name):
    from htd_amd.core.evaluation import eval_map
    z, dets, anns, kw = load_case(name)
    got = eval_map(dets, anns, logger='silent', **kw)
    assert_matches_packed(got, z, name + '/')
    assert_same_result(got, eval_map_np(dets, anns, **kw))
    K = len(dets[0])
    assert_same_result(eval_map(_triple(dets), anns, logger='silent', num_classes=K, **kw), got)


@pytest.mark.parametrize('seed,kw', [(11, dict()), (12, dict(dataset='voc07')), (13, dict(iou_thr=0.7)),
                                     (14, dict(scale_ranges=[(0, 64), (64, 128), (128, 1e5)])),
                                     (15, dict(scale_ranges=[(0, 64), (64, 1e5)], dataset='voc07'))])
def test_restatement_with_ties(seed, kw):
    from htd_amd.core.evaluation import eval_map
    dets, anns = synthetic_voc(500, 20, dets_per_img=60, seed=seed, ties=True, empty_every=9)
    scores = np.concatenate([a[:, 4] for r in dets for a in r])
    assert len(np.unique(scores)) < len(scores) // 10               # heavy ties, across and inside images
    got = eval_map(dets, anns, logger='silent', **kw)
    assert_same_result(got, eval_map_np(dets, anns, **kw))
    again = eval_map(_triple(dets), anns, logger='silent', num_classes=20, **kw)
    assert_same_result(again, got)


def test_deterministic_and_one_readback(monkeypatch):
    from htd_amd.core import evaluation
    dets, anns = synthetic_voc(200, 20, seed=21, ties=True)
    a = evaluation.map_device_arrays(dets, anns, 20)
    b = evaluation.map_device_arrays(dets, anns, 20)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    reads = []
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *args, **kw):
        reads.append(self.shape)
        return real_cpu(self, *args, **kw)
    monkeypatch.setattr(torch.Tensor, 'cpu', counting_cpu)
    evaluation.map_device_arrays(dets, anns, 20)
    assert len(reads) == 1, reads


def test_voc07_shaped_set():
    # 4952 images x 20 classes, 100 detections per image: the bench tool's set, against the restatement
    from htd_amd.core.evaluation import eval_map
    dets, anns = synthetic_voc(4952, 20, dets_per_img=100, seed=5)
    got = eval_map(_triple(dets), anns, logger='silent', dataset='voc07')
    assert_same_result(got, eval_map_np(dets, anns, dataset='voc07'))


def test_triple_out_of_range_raises_after_one_read():
    from htd_amd.core.evaluation import eval_map
    dets, anns = synthetic_voc(20, 5, seed=31)
    d, l, i = _triple(dets)
    for bad in ((d, l + 5, i), (d, l, i + 20), (d, l - 9, i)):
        with pytest.raises(ValueError, match='must lie'):
            eval_map(bad, anns, logger='silent', num_classes=5)
