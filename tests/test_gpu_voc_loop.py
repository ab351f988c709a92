"""A 20-class HTD on the device: a train step and simple_test against the CPU oracle, and VOCDataset.evaluate ('mAP'
and 'recall') on single_gpu_test output over a small VOCdevkit whose JPEGs the test writes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _seeded_20_class(train):
    from golden_util import load_seeded_
    from htd_amd.configs import build_htd_detector, htd_config
    cfg = htd_config(50, dataset='voc0712')
    cfg.train_cfg.rpn_proposal.update(nms_pre=200, nms_post=100, max_num=100)
    for r in cfg.train_cfg.rcnn:
        r.sampler.num = 48
    det = load_seeded_(build_htd_detector(cfg=cfg), 'det.').cuda()
    return det.train() if train else det.eval()


def test_20_class_train_step_and_simple_test_against_oracle():
    """The bounds of the 80-class test_gpu_detector.py tests: RPN end to end, the RoI head fed the oracle's proposals
    and sample picks; losses at rtol 5e-4, gradients (the 20-class fc_cls / fc_reg of both stages among them) at
    2e-3 of their scale; simple_test detections matched one to one within 1e-3."""
    from golden_util import demo_inputs, seeded_state_dict
    from test_gpu_detector import ReplaySampler
    from htd_amd.core import set_randperm
    from oracle import detector as D
    H, W, B = 96, 160, 3
    imgs, gts, labels = demo_inputs(B, H, W, np.random.RandomState(5), num_classes=20)
    imgs = (imgs - 0.5) * 4
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), ori_shape=(H, W, 3),
                  scale_factor=np.array([1, 1, 1, 1], dtype=np.float32), flip=False) for _ in range(B)]
    T = lambda a: torch.from_numpy(np.asarray(a))
    ocfg = D.htd_config(50)
    ocfg['num_classes'] = 20
    ocfg['train_cfg']['rpn_proposal'].update(nms_pre=200, nms_post=100, max_num=100)
    for r in ocfg['train_cfg']['rcnn']:
        r['sampler']['num'] = 48
    sd = {k: v.requires_grad_(v.dtype.is_floating_point and 'running' not in k)
          for k, v in seeded_state_dict(D.state_shapes(50, num_classes=20), prefix='det.').items()}
    torch.manual_seed(9)
    trace = {}
    ref_loss, ref_log = D.parse_losses(D.forward_train(sd, T(imgs), metas, [T(x) for x in gts],
                                                       [T(x) for x in labels], ocfg, trace))
    ref_loss.backward()
    det = _seeded_20_class(train=True)
    assert det.roi_head.bbox_head[0].num_classes == 20
    gts_d, labels_d = [T(x).cuda() for x in gts], [T(x).cuda() for x in labels]
    head = det.roi_head
    saved = list(head.bbox_sampler)
    set_randperm(lambda n, device: torch.randperm(n).to(device))       # the oracle's CPU draws for the RPN sampler
    try:
        torch.manual_seed(9)
        x = det.extract_feat(T(imgs).cuda())
        losses, _ = det.rpn_head.forward_train(x, metas, gts_d, proposal_cfg=det.train_cfg.rpn_proposal)
        head.bbox_sampler = [ReplaySampler(saved[i], trace['samples'][i]) for i in range(2)]
        losses.update(head.forward_train(x, metas, [p.cuda() for p in trace['proposals']], gts_d, labels_d))
    finally:
        head.bbox_sampler = saved
        set_randperm(None)
    loss, log = det._parse_losses(losses)
    for k, v in log.items():
        np.testing.assert_allclose(v, ref_log[k], rtol=5e-4, atol=1e-4, err_msg=k)
    det.zero_grad()
    loss.backward()
    params = dict(det.named_parameters())
    for k in ('roi_head.bbox_head.0.fc_cls.weight', 'roi_head.bbox_head.0.fc_cls.bias',
              'roi_head.bbox_head.0.fc_reg.weight', 'roi_head.bbox_head.1.fc_cls.weight',
              'roi_head.bbox_head.1.fc_cls.bias', 'roi_head.bbox_head.1.fc_reg.weight',
              'roi_head.bbox_head.1.graph_lvl1_cls.weight', 'roi_head.bbox_head.1.fcs.0.weight',
              'rpn_head.rpn_cls.weight', 'neck.fpn_convs.0.conv.weight'):
        a = params[k].grad.detach().cpu() if params[k].grad is not None else torch.zeros_like(params[k]).cpu()
        b = sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k])
        a = a.reshape(b.shape)
        scale = max(b.abs().max().item(), 1e-6)
        assert (a - b).abs().max().item() <= 2e-3 * scale + 1e-6, (k, (a - b).abs().max().item(), scale)

    det.eval()
    with torch.no_grad():
        ref_props, ref_res = D.simple_test({k: v.detach() for k, v in sd.items()}, T(imgs), metas, ocfg)
        feats = det.extract_feat(T(imgs).cuda())
        res = det.roi_head.simple_test(feats, [p.cuda() for p in ref_props], metas, rescale=False)
    assert len(res) == B and all(len(r) == 20 for r in res)
    for i in range(B):
        mine = np.concatenate([np.concatenate([r, np.full((len(r), 1), c, dtype=np.float32)], 1)
                               for c, r in enumerate(res[i])], 0)
        dets, labs = ref_res[i]
        ref = np.concatenate([dets.numpy(), labs.numpy()[:, None].astype(np.float32)], 1)
        assert mine.shape == ref.shape and len(ref) > 0
        assert labs.max().item() < 20
        used = np.zeros(len(mine), dtype=bool)
        for r in ref:
            d = np.abs(mine[:, :5] - r[:5]).max(1) + 1e3 * (mine[:, 5] != r[5]) + 1e3 * used
            j = int(d.argmin())
            assert d[j] <= 1e-3 + 1e-5 * np.abs(r[:4]).max(), (r, mine[j], d[j])
            used[j] = True


def test_voc_evaluate_on_simple_test_output(tmp_path):
    from PIL import Image
    from test_voc_dataset import VOC07, _write_split
    from voc_eval_np import eval_map_np
    from htd_amd.apis import single_gpu_test
    from htd_amd.configs import htd_config
    from htd_amd.core.evaluation import eval_recalls
    from htd_amd.datasets import build_dataloader, build_dataset
    root = str(tmp_path / 'VOCdevkit') + '/'
    base = _write_split(root, 2007, VOC07)
    rs = np.random.RandomState(0)
    for img_id, size, _ in VOC07:
        w, h = size or (400, 300)
        Image.fromarray((rs.rand(h, w, 3) * 255).astype(np.uint8)).save(f'{base}/JPEGImages/{img_id}.jpg')
    cfg = htd_config(50, dataset='voc0712').data.test.to_dict()
    cfg.update(ann_file=f'{base}/ImageSets/Main/trainval.txt', img_prefix=f'{base}/', test_mode=True)
    cfg['pipeline'][1]['img_scale'] = (320, 192)
    ds = build_dataset(cfg)
    loader = build_dataloader(ds, 1, 0, dist=False, shuffle=False)
    model = _seeded_20_class(train=False)
    results = single_gpu_test(model, loader)
    assert len(results) == len(ds) and all(len(r) == 20 for r in results)
    anns = [ds.get_ann_info(i) for i in range(len(ds))]
    out = ds.evaluate(results, metric='mAP', logger='silent')
    assert list(out) == ['mAP']
    assert out['mAP'] == eval_map_np(results, anns, dataset='voc07')[0]
    triple = tuple(t.cuda() for t in single_gpu_test(model, loader, return_tensors=True))
    assert ds.evaluate(triple, metric='mAP', logger='silent')['mAP'] == out['mAP']
    # ground truths as detections: every class present scores 1
    perfect = [[np.concatenate([a['bboxes'][a['labels'] == c], np.ones((int((a['labels'] == c).sum()), 1))], 1)
                .astype(np.float32) for c in range(20)] for a in anns]
    assert ds.evaluate(perfect, logger='silent')['mAP'] == 1.0
    props = [np.concatenate([x for x in r if len(x)] or [np.zeros((0, 5), np.float32)]) for r in results]
    rec = ds.evaluate(props, metric='recall', proposal_nums=(10, 100), iou_thr=[0.5, 0.7], logger='silent')
    want = eval_recalls([a['bboxes'] for a in anns], props, (10, 100), [0.5, 0.7], logger='silent')
    assert list(rec) == ['recall@10@0.5', 'recall@10@0.7', 'recall@100@0.5', 'recall@100@0.7', 'AR@10', 'AR@100']
    assert rec['recall@100@0.7'] == want[1, 1] and rec['AR@10'] == want[0].mean()
    from htd_amd.datasets import ConcatDataset
    both = ConcatDataset([ds, ds])
    sep = both.evaluate(perfect + perfect, logger='silent')
    assert sep == {'0_mAP': 1.0, '1_mAP': 1.0}
    from htd_amd.apis import results_to_tensors
    mixed = tuple(t.cuda() for t in results_to_tensors(results + perfect))
    assert both.evaluate(mixed, logger='silent') == {'0_mAP': out['mAP'], '1_mAP': 1.0}
