"""Result collection of multi_gpu_test (htd_amd.apis.collect_results) in a world-2 gloo run (CPU): the ranks hold
unequal shares, the sampler has padded, and rank 0 rebuilds exactly the single-process result lists."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

NUM_CLASSES = 4


def fake_result(i):
    """A bbox2result list for dataset index i: ragged per class, some classes and whole images empty."""
    rs = np.random.RandomState(100 + i)
    if i % 5 == 3:
        return [np.zeros((0, 5), np.float32) for _ in range(NUM_CLASSES)]
    return [rs.rand(rs.randint(0, 4), 5).astype(np.float32) * 100 for _ in range(NUM_CLASSES)]


def _same(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb) == NUM_CLASSES
        for x, y in zip(ra, rb):
            assert x.dtype == y.dtype == np.float32 and x.shape == y.shape and np.array_equal(x, y)


def test_tensor_round_trip():
    from htd_amd.apis import results_to_tensors, tensors_to_results
    res = [fake_result(i) for i in range(9)]
    dets, labels, index = results_to_tensors(res)
    assert dets.dtype == torch.float32 and labels.dtype == index.dtype == torch.int64
    assert dets.shape[0] == sum(r.shape[0] for x in res for r in x)
    _same(tensors_to_results(dets, labels, index, 9, NUM_CLASSES), res)
    perm = torch.randperm(dets.shape[0], generator=torch.Generator().manual_seed(0))
    shuffled = tensors_to_results(dets[perm], labels[perm], index[perm], 9, NUM_CLASSES)
    for ra, rb in zip(shuffled, res):          # rows of one (image, label) keep their relative order only
        for x, y in zip(ra, rb):
            assert np.array_equal(np.sort(x, axis=0), np.sort(y, axis=0))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, size, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from htd_amd.apis import collect_results
        from htd_amd.datasets import DistributedSampler
        mine = [fake_result(i) for i in DistributedSampler(list(range(size)), shuffle=False)]
        lists = collect_results(mine, size, NUM_CLASSES)
        triple = collect_results(mine, size, NUM_CLASSES, return_tensors=True)
        q.put((rank, len(mine), lists, None if triple is None else [t.numpy() for t in triple]))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_collect_equals_single_process():
    from htd_amd.coco import CocoEvaluator
    world, size = 2, 7                                # rank 0: 0 2 4 6, rank 1: 1 3 5 + the padding sample 0
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, size, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    for _ in range(world):
        rank, n, lists, triple = q.get(timeout=120)
        out[rank] = (n, lists, triple)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert out[0][0] == out[1][0] == 4
    assert out[1][1] is None and out[1][2] is None
    single = [fake_result(i) for i in range(size)]
    _same(out[0][1], single)
    dets, labels, index = out[0][2]
    ev = CocoEvaluator(dict(images=[dict(id=i + 1) for i in range(size)], annotations=[],
                            categories=[dict(id=c + 1, name=str(c)) for c in range(NUM_CLASSES)]),
                       classes=[str(c) for c in range(NUM_CLASSES)])
    a = ev._det_arrays((torch.from_numpy(dets), torch.from_numpy(labels), torch.from_numpy(index)))
    b = ev._det_arrays(single)
    for k in a:                                       # the triple is what the evaluator sees from the lists
        assert torch.equal(a[k], b[k]), k
