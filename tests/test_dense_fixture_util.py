"""The one thing the two texts of a dense head's fixture weights used to promise each other, on the CPU: the state dict that
fixture_state() rebuilds from a fixture's key and shape lists IS the state dict of the detector that load_fixture_weights_()
edited -- the same keys in the same order, torch.equal values -- for every dense detector fixture.  (Both walk one table of
dense_fixture_util now; the GPU round-trip tests compare detections within a tolerance and would not see a small disagreement.)"""
import pytest
import torch

import atss_util
import fcos_util
import fovea_util
import gfl_util
import ghm_util
import retina_util
import vfnet_util

TWO = ('cls_scale', 'cls_bias_shift')
# case -> (util, fixture, key prefix, config function, its arguments, detector builder, the figures the fixture records)
CASES = dict(retinanet=(retina_util, 'retinanet', '', 'retinanet_config', {}, 'build_retinanet_detector', TWO[:1]),
             ghm=(ghm_util, 'ghm', '', 'retinanet_ghm_config', {}, 'build_retinanet_ghm_detector', TWO[:1]),
             fcos=(fcos_util, 'fcos', '', 'fcos_config', {}, 'build_baseline_detector', TWO),
             atss=(atss_util, 'atss', '', 'atss_config', {}, 'build_baseline_detector', TWO),
             gfl=(gfl_util, 'gfl', '', 'gfl_config', {}, 'build_baseline_detector', TWO),
             vfnet=(vfnet_util, 'vfnet', '', 'vfnet_config', {}, 'build_baseline_detector', TWO),
             fovea_plain=(fovea_util, 'fovea', 'plain.', 'fovea_config', fovea_util.CONFIG_ARGS['plain'], 'build_fovea_detector', TWO),
             fovea_align=(fovea_util, 'fovea', 'align.', 'fovea_config', fovea_util.CONFIG_ARGS['align'], 'build_fovea_detector', TWO))


@pytest.mark.parametrize('case', list(CASES))
def test_fixture_state_is_the_state_dict_the_loader_leaves(golden, case):
    from htd_amd import configs
    U, fixture, p, config, args, build, names = CASES[case]
    g = golden(fixture)
    figures = [float(g[p + n]) for n in names]
    torch.manual_seed(7)                                 # (whatever the constructor draws, the loader overwrites)
    det = U.load_fixture_weights_(getattr(configs, build)(cfg=getattr(configs, config)(**args)), *figures)
    mine = det.state_dict()
    ref = U.fixture_state(g[p + 'state_keys'], g[p + 'state_shapes'], *figures)
    assert list(mine) == list(ref)
    for k, v in ref.items():
        if k.endswith('num_batches_tracked'):
            assert v.dtype == torch.int64 and int(v) == 0 and int(mine[k]) == 0, k
        else:
            assert v.dtype == mine[k].dtype and v.shape == mine[k].shape and torch.equal(v, mine[k]), k
