"""Test loops over a data loader: single_gpu_test, multi_gpu_test and the tensor form of their results.

A batch from `datasets.build_dataloader` is a list of host-side `Collect` dicts; `pipelines.collate` turns it into the
detector's keyword arguments on the model's device (one upload of uint8 pixels, one htd_image_batch_pipeline launch),
and the detector's own batched post-processing produces the per-image bbox2result lists.

Across ranks the results travel as numbers, not pickles: each rank packs its detections into a triple of tensors
(dets (N, 5) float32, labels (N,) int64, result index (N,) int64), the triples are all-gathered on the device (RCCL
under the `nccl` backend, gloo on the host), and rank 0 rebuilds the per-image lists.  CocoEvaluator takes the triple
directly, so a caller can also evaluate without rebuilding the lists.
"""
import numpy as np
import torch
import torch.distributed as dist

from .datasets import get_dist_info
from .pipelines import collate


def _model_device(model):
    return next(model.parameters()).device


def _num_classes(model):
    heads = model.roi_head.bbox_head
    return (heads[-1] if isinstance(heads, (list, tuple, torch.nn.ModuleList)) else heads).num_classes


def results_to_tensors(results, indices=None):
    """bbox2result lists -> (dets (N, 5) float32, labels (N,) int64, index (N,) int64) on the host.  Rows run image by
    image (indices[i] names image i, default i), label-major inside an image, in each array's row order."""
    indices = np.arange(len(results), dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64)
    arrs = [b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b) for r in results for b in r]
    lens = np.array([a.shape[0] if a.ndim == 2 else 0 for a in arrs], dtype=np.int64)
    rows = [a.reshape(-1, 5) for a, n in zip(arrs, lens) if n]
    dets = np.concatenate(rows).astype(np.float32, copy=False) if rows else np.zeros((0, 5), np.float32)
    per_img = [len(r) for r in results]
    labels = np.repeat(np.concatenate([np.arange(n, dtype=np.int64) for n in per_img] or [np.zeros(0, np.int64)]),
                       lens)
    index = np.repeat(np.repeat(indices, per_img), lens)
    return torch.from_numpy(dets), torch.from_numpy(labels), torch.from_numpy(index)


def tensors_to_results(dets, labels, index, num_images, num_classes):
    """The inverse of results_to_tensors: image i's list holds, for each label, its rows in the order given."""
    dets = dets.detach().cpu().numpy().astype(np.float32, copy=False).reshape(-1, 5)
    key = index.detach().cpu().numpy().astype(np.int64) * num_classes + labels.detach().cpu().numpy().astype(np.int64)
    order = np.argsort(key, kind='stable')
    counts = np.bincount(key, minlength=num_images * num_classes)
    parts = np.split(dets[order], np.cumsum(counts)[:-1])
    return [parts[i * num_classes:(i + 1) * num_classes] for i in range(num_images)]


def _run(model, data_loader):
    """-> the per-image bbox2result lists of every batch of the loader, in loader order."""
    model.eval()
    dev = _model_device(model)
    results = []
    for samples in data_loader:
        data = collate(samples, dev)
        with torch.no_grad():
            results.extend(model(return_loss=False, rescale=True, **data))
    return results


def single_gpu_test(model, data_loader, return_tensors=False):
    """Run `model` over every batch of `data_loader` -> one bbox2result list per sample, in loader order.
    return_tensors=True: the results_to_tensors triple instead."""
    results = _run(model, data_loader)
    return results_to_tensors(results) if return_tensors else results


def multi_gpu_test(model, data_loader, tmpdir=None, gpu_collect=True, return_tensors=False):
    """Every rank runs its share of the loader; rank 0 returns the results of the whole dataset in the interleaved
    order of DistributedSampler (sample k of rank r is result k * world + r), without the sampler's padding: sample
    k of rank r is kept if and only if k * world + r < len(dataset).  Other ranks return None.

    Collection always all-gathers tensors (on the device under `nccl`, on the host under gloo); `tmpdir` and
    `gpu_collect` are accepted for the reference's signature and have no effect.  return_tensors=True: rank 0 returns
    the (dets, labels, result index) triple instead of the lists."""
    results = _run(model, data_loader)
    return collect_results(results, len(data_loader.dataset), _num_classes(model), _model_device(model),
                           return_tensors)


def collect_results(results, size, num_classes, device=None, return_tensors=False):
    """This rank's results (in its sampler's order) -> on rank 0, the `size` results of the dataset in the interleaved
    order of multi_gpu_test (padding dropped); None on the other ranks.  The rows travel as tensors: on `device`
    under the `nccl` backend, on the host otherwise."""
    rank, world = get_dist_info()
    pos = np.arange(len(results), dtype=np.int64) * world + rank
    keep = pos < size
    dets, labels, index = results_to_tensors([r for r, k in zip(results, keep) if k], pos[keep])
    if world > 1:
        dev = torch.device(device) if dist.get_backend() == 'nccl' else torch.device('cpu')
        dets, labels, index = _gather(dets.to(dev), labels.to(dev), index.to(dev), world)
        if rank != 0:
            return None
    if return_tensors:
        return dets, labels, index
    return tensors_to_results(dets, labels, index, size, num_classes)


def _gather(dets, labels, index, world):
    """all_gather of ragged rows: lengths first, then the rows padded to the longest; -> the concatenation."""
    n = torch.tensor([dets.size(0)], dtype=torch.int64, device=dets.device)
    ns = [torch.empty_like(n) for _ in range(world)]
    dist.all_gather(ns, n)
    ns = [int(x) for x in torch.cat(ns).tolist()]
    m = max(ns)
    packed = torch.cat([dets.double(), labels.double()[:, None], index.double()[:, None]], 1)    # exact below 2**53
    packed = torch.nn.functional.pad(packed, (0, 0, 0, m - packed.size(0)))
    parts = [torch.empty_like(packed) for _ in range(world)]
    dist.all_gather(parts, packed)
    allp = torch.cat([p[:k] for p, k in zip(parts, ns)])
    return allp[:, :5].float(), allp[:, 5].long(), allp[:, 6].long()
