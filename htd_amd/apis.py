"""Test loops over a data loader: single_gpu_test, multi_gpu_test and the tensor form of their results.

A batch from `datasets.build_dataloader` is a list of host-side `Collect` dicts; `pipelines.collate` turns it into the
detector's keyword arguments on the model's device (one upload of uint8 pixels, one htd_image_batch_pipeline launch),
and the detector's own batched post-processing produces the per-image bbox2result lists.

Across ranks the results travel as numbers, not pickles: each rank packs its detections into a triple of tensors
(dets (N, 5) float32, labels (N,) int64, result index (N,) int64), the triples are all-gathered on the device (RCCL
under the `nccl` backend, gloo on the host), and rank 0 rebuilds the per-image lists.  CocoEvaluator takes the triple
directly, so a caller can also evaluate without rebuilding the lists.
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from .datasets import get_dist_info
from .pipelines import collate


def _model_device(model):
    return next(model.parameters()).device


def _num_classes(model):
    if getattr(model, 'roi_head', None) is None:        # single-stage detectors
        return model.bbox_head.num_classes
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


# ================================================================================================ training
# What mmdet/apis/train.py:train_detector sets up around mmcv's EpochBasedRunner, with the hooks it registers, run in the
# reference's order: LrUpdaterHook (by epoch, inside Trainer's schedule), OptimizerHook (Trainer.train_step),
# CheckpointHook, IterTimerHook, DistSamplerSeedHook, EvalHook / DistEvalHook, TextLoggerHook.

RUNTIME_DEFAULTS = dict(checkpoint_config=dict(interval=1), log_config=dict(interval=50, hooks=[dict(type='TextLoggerHook')]),
                        workflow=[('train', 1)], load_from=None, resume_from=None)   # configs/_base_/default_runtime.py
_EVAL_RUNNER_KEYS = ('interval', 'tmpdir', 'start', 'gpu_collect', 'save_best', 'rule')


def apply_runtime_defaults(cfg):
    """Fill the keys of configs/_base_/default_runtime.py that `cfg` lacks (htd_config carries none of them); -> cfg."""
    import copy
    for k, v in RUNTIME_DEFAULTS.items():
        if k not in cfg:
            setattr(cfg, k, copy.deepcopy(v))
    return cfg


def check_supported(cfg):
    """NotImplementedError naming the key for what this runner does not do (no HTD config uses any of it)."""
    for phase in cfg.get('workflow') or []:
        if phase[0] != 'train':
            raise NotImplementedError(f'workflow: a {phase[0]!r} phase is not supported, only [("train", 1)]')
    if cfg.get('custom_hooks'):
        raise NotImplementedError('custom_hooks: user-defined hooks are not supported')
    grad_clip = (cfg.get('optimizer_config') or {}).get('grad_clip')
    if grad_clip is not None:
        raise NotImplementedError(f'optimizer_config.grad_clip: only None is supported, got {grad_clip!r}')
    paramwise = (cfg.get('optimizer') or {}).get('paramwise_cfg')
    if paramwise:
        raise NotImplementedError(f'optimizer.paramwise_cfg: per-parameter rates and decays are not supported, got {paramwise!r}')
    for hook in (cfg.get('log_config') or {}).get('hooks', []):
        if hook.get('type') != 'TextLoggerHook':
            raise NotImplementedError(f"log_config.hooks: {hook.get('type')!r} is not supported, only TextLoggerHook")


def set_random_seed(seed, deterministic=False):
    """mmdet/apis/train.py:set_random_seed: python, numpy, torch and every HIP device."""
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    if deterministic:
        torch.backends.cudnn.deterministic = True
        torch.backends.cudnn.benchmark = False


def rng_state():
    """The python, numpy, torch CPU and HIP generator states as tensors and plain numbers (a checkpoint's meta stays
    readable by load_checkpoint's weights_only path)."""
    import random
    version, keys, gauss = random.getstate()
    _, mt, pos, has_gauss, cached = np.random.get_state()
    st = dict(python=torch.tensor(keys, dtype=torch.int64), python_version=int(version), python_gauss=gauss,
              numpy=torch.from_numpy(mt.astype(np.int64)), numpy_pos=int(pos), numpy_has_gauss=int(has_gauss),
              numpy_gauss=float(cached), torch=torch.get_rng_state())
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        st['hip'] = torch.cuda.get_rng_state()
    return st


def set_rng_state(st):
    import random
    random.setstate((st['python_version'], tuple(int(x) for x in st['python'].tolist()), st['python_gauss']))
    np.random.set_state(('MT19937', st['numpy'].numpy().astype(np.uint32), st['numpy_pos'], st['numpy_has_gauss'],
                         st['numpy_gauss']))
    torch.set_rng_state(st['torch'])
    if 'hip' in st and torch.cuda.is_available():
        torch.cuda.set_rng_state(st['hip'])


def env_info():
    """collect_env's essentials: python, torch, HIP / ROCm versions and the device name."""
    import sys
    info = dict(sys=sys.platform, Python=sys.version.replace('\n', ''), PyTorch=torch.__version__,
                HIP=getattr(torch.version, 'hip', None), GPU=None)
    if torch.cuda.is_available():
        info['GPU'] = torch.cuda.get_device_name(torch.cuda.current_device())
    return '\n'.join(f'{k}: {v}' for k, v in info.items())


def get_root_logger(log_file=None, log_level='INFO'):
    """mmdet.utils.get_root_logger: the `htd_amd` logger; rank 0 prints and writes `log_file`, other ranks only errors."""
    import logging
    logger = logging.getLogger('htd_amd')
    rank, _ = get_dist_info()
    if not any(getattr(h, '_htd', False) for h in logger.handlers):
        h = logging.StreamHandler()
        h._htd = True
        logger.addHandler(h)
    fmt = logging.Formatter('%(asctime)s - %(name)s - %(levelname)s - %(message)s')
    for h in logger.handlers:
        h.setFormatter(fmt)
    if rank == 0 and log_file is not None and not any(getattr(h, 'baseFilename', None) == os.path.abspath(log_file)
                                                      for h in logger.handlers):
        fh = logging.FileHandler(log_file, 'w')
        fh.setFormatter(fmt)
        logger.addHandler(fh)
    logger.setLevel(log_level if rank == 0 else 'ERROR')
    logger.propagate = False
    return logger


class NonFiniteLossError(FloatingPointError):
    """The total loss of iteration `iter` (1-based, counted over the whole run) was not finite."""

    def __init__(self, it, epoch, inner, per_epoch):
        self.iter = it
        super().__init__(f'loss is not finite at iteration {it} (epoch {epoch}, iter {inner}/{per_epoch}); training '
                         'stopped before any checkpoint of the affected weights was written')


class EvalHook:
    """EvalHook / DistEvalHook (core/evaluation/eval_hooks.py): after every `interval` epochs run the test loop over the
    validation loader (built once, kept), evaluate on rank 0 and hand the metrics to the logger.  The model goes back to
    train mode, and the python / numpy / torch / HIP generators are put back as they were: evaluating does not change
    what training draws next."""

    def __init__(self, dataloader, distributed=False, start=None, interval=1, **eval_kwargs):
        if interval <= 0:
            raise ValueError(f'interval must be positive, but got {interval}')
        self.dataloader, self.distributed, self.start, self.interval = dataloader, distributed, start, interval
        self.eval_kwargs = {k: v for k, v in eval_kwargs.items() if k not in _EVAL_RUNNER_KEYS}
        self.initial = True

    def due(self, epoch):
        """After 0-based epoch `epoch`?"""
        if self.start is None:
            return (epoch + 1) % self.interval == 0
        return epoch + 1 >= self.start and (epoch + 1 - self.start) % self.interval == 0

    def __call__(self, model):
        """-> the metric dict on rank 0, None elsewhere."""
        state = rng_state()
        try:
            if self.distributed:
                results = multi_gpu_test(model, self.dataloader)
            else:
                results = single_gpu_test(model, self.dataloader)
        finally:
            set_rng_state(state)
            model.train()
        if get_dist_info()[0] != 0:
            return None
        return self.dataloader.dataset.evaluate(results, **self.eval_kwargs)


def _round_float(v):
    return round(v, 5) if isinstance(v, float) else v


class EpochRunner:
    """mmcv's EpochBasedRunner.train with the hooks of train_detector, over `Trainer`:

      * per iteration: `batch_fn(samples, device)` -> Trainer.train_step -> ONE htd_log_accumulate launch that adds
        num_samples * log_vars (the packed device vector of _parse_losses) into fp64 sums and latches the first
        non-finite total loss; nothing is read back (the step stays free of host/device synchronisation);
      * every `log_interval` inner iterations: one read of the sums -> a text line and a json line (LogBuffer averages
        weighted by num_samples, mmcv's ignore_last=True: a partial tail is not logged); a non-finite loss stops the run
        there (and at the end of an epoch, before its checkpoint) with NonFiniteLossError;
      * every `checkpoint_interval` epochs: epoch_{n}.pth and latest.pth on rank 0 (meta: the caller's meta, CLASSES,
        epoch, iter and the generator states, so that `resume` continues the same random streams);
      * then the EvalHook, whose metrics become a `val` line.
    """

    def __init__(self, trainer, data_loader, work_dir, max_epochs, logger=None, meta=None, timestamp=None,
                 checkpoint_interval=1, log_interval=50, eval_hook=None, batch_fn=collate, distributed=False):
        import time
        self.trainer, self.model, self.data_loader = trainer, trainer.model, data_loader
        self.work_dir, self.max_epochs, self.meta = work_dir, max_epochs, dict(meta or {})
        self.timestamp = timestamp or time.strftime('%Y%m%d_%H%M%S', time.localtime())
        self.logger = logger or get_root_logger()
        self.checkpoint_interval, self.log_interval = checkpoint_interval, log_interval
        self.eval_hook, self.batch_fn, self.distributed = eval_hook, batch_fn, distributed
        self.device = _model_device(self.model)
        self.rank, self.world = get_dist_info()
        self.epoch = trainer.epoch
        self.inner_iter = 0
        self.json_log = os.path.join(work_dir, f'{self.timestamp}.log.json')
        self.log_history = []                 # every logged record, unrounded (the json lines round floats to 5 digits)
        # host seconds waiting on the loader, in the hooks, and (part of hooks_s) in the reads of the log sums, which wait
        # for the device to finish the steps queued before them
        self.timing = dict(loader_s=0.0, hooks_s=0.0, sync_s=0.0, iters=0)
        self._acc = self._keys = None
        self._times = []
        if self.rank == 0:
            os.makedirs(work_dir, exist_ok=True)
            header = {k: v for k, v in self.meta.items() if k in ('env_info', 'config', 'seed', 'exp_name')}
            if header:
                self._dump(header)

    @property
    def iter(self):
        return self.trainer.iter

    # ------------------------------------------------------------------------------------------ resume / load
    def resume(self, filename):
        """runner.resume: weights, optimizer state, epoch, iteration and (when the file has them) the generators."""
        ckpt = self.trainer.resume(filename, map_location='cpu')
        meta = ckpt.get('meta', {})
        self.epoch = int(meta.get('epoch', self.trainer.epoch))
        if 'rng' in meta:
            set_rng_state(meta['rng'])
        self.logger.info(f'resumed epoch {self.epoch}, iter {self.iter}')
        return ckpt

    def load_checkpoint(self, filename):
        self.logger.info(f'load checkpoint from {filename}')
        return self.trainer.load_checkpoint(filename, map_location='cpu', strict=False)

    # ------------------------------------------------------------------------------------------ the loop
    def run(self):
        import time
        t0 = time.time()
        if self.eval_hook is not None and self.eval_hook.initial:
            self.eval_hook.initial = False
            if self.eval_hook.start is not None and self.epoch >= self.eval_hook.start:
                self._evaluate()
        while self.epoch < self.max_epochs:
            self.train_epoch()
        self.timing['run_s'] = self.timing.get('run_s', 0.0) + time.time() - t0

    def train_epoch(self):
        import time
        self.model.train()
        sampler = getattr(self.data_loader, 'sampler', None)
        if self.distributed and hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(self.epoch)                     # DistSamplerSeedHook
        self._reset_log()
        n = len(self.data_loader)
        t = time.time()
        for i, samples in enumerate(self.data_loader):
            self.inner_iter = i
            data_time = time.time() - t
            self.run_iter(samples)
            now = time.time()
            self._times.append((now - t, data_time))
            self.timing['loader_s'] += data_time
            self.timing['iters'] += 1
            t = now
            if (i + 1) % self.log_interval == 0:
                self._log_train(n)
                self.timing['hooks_s'] += time.time() - t
        a = time.time()
        self._check_finite(n)                                 # the unlogged tail too, before any checkpoint
        if self.checkpoint_interval and (self.epoch + 1) % self.checkpoint_interval == 0:
            self.save_checkpoint()
        if self.eval_hook is not None and self.eval_hook.due(self.epoch):
            self._evaluate()
        self._reset_log()
        self.epoch += 1
        self.timing['hooks_s'] += time.time() - a

    def run_iter(self, samples):
        """One iteration without its hooks: the batch to the device, Trainer.train_step, the log buffer's one launch."""
        it = self.trainer.iter
        out = self.trainer.train_step(self.batch_fn(samples, self.device))
        self._accumulate(out, it)
        return out

    # ------------------------------------------------------------------------------------------ log buffer
    def _reset_log(self):
        self._acc = self._keys = None
        self._times = []

    def _accumulate(self, out, it):
        from . import mmcv_ops as M
        log_vars = out['log_vars']
        keys = list(log_vars.keys())
        packed = getattr(log_vars, '_packed', None)
        if packed is None:
            packed = torch.stack([torch.as_tensor(log_vars[k], dtype=torch.float32).reshape(()) for k in keys])
            packed = packed.to(self.device)
        if self._acc is None:
            self._keys = keys
            self._acc = M.log_accumulator(len(keys), packed.device)
        elif keys != self._keys:
            raise ValueError(f'log_vars changed inside a log interval: {self._keys} -> {keys}')
        M.log_accumulate_(self._acc, packed.detach().float().contiguous(), out.get('num_samples', 1), it,
                          loss_index=keys.index('loss') if 'loss' in keys else -1)

    def _read(self):
        """-> (averages by key, first bad iteration or None); the one host read of a log interval."""
        import time
        if self._acc is None:
            return None, None
        t = time.time()
        vals = self._acc.tolist()
        self.timing['sync_s'] += time.time() - t
        n = len(self._keys)
        bad = int(vals[n + 1]) if vals[n + 1] >= 0 else None
        return {k: vals[i] / vals[n] for i, k in enumerate(self._keys)}, bad

    def _raise_if_bad(self, bad):
        if bad is not None:
            per = self.trainer.schedule.iters_per_epoch
            raise NonFiniteLossError(bad + 1, bad // per + 1, bad % per + 1, per)

    def _check_finite(self, n):
        _, bad = self._read()
        self._raise_if_bad(bad)

    def _max_memory(self):
        mem = torch.cuda.max_memory_allocated(self.device) // (1024 * 1024)
        if self.distributed:
            t = torch.tensor([mem], dtype=torch.int64, device=self.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            mem = int(t.item())
        return int(mem)

    def _log_train(self, n):
        avg, bad = self._read()
        self._raise_if_bad(bad)
        times = self._times[-self.log_interval:]
        rec = dict(mode='train', epoch=self.epoch + 1, iter=self.inner_iter + 1,
                   lr=self.trainer.schedule.lr(self.trainer.iter - 1))
        if self.device.type == 'cuda':
            rec['memory'] = self._max_memory()
        rec['time'] = sum(x for x, _ in times) / len(times)
        rec['data_time'] = sum(x for _, x in times) / len(times)
        rec.update(avg)
        self._emit(rec, n)
        self._reset_log()

    def _evaluate(self):
        metrics = self.eval_hook(self.model)
        if self.rank == 0 and metrics is not None:
            rec = dict(mode='val', epoch=self.epoch + 1, iter=len(self.data_loader),
                       lr=self.trainer.schedule.lr(max(self.trainer.iter - 1, 0)))
            rec.update(metrics)
            self._emit(rec, len(self.data_loader))

    def _emit(self, rec, n):
        """TextLoggerHook: one text line (logger) and one json line (rank 0)."""
        self.log_history.append(rec)
        if rec['mode'] == 'train':
            head = f"Epoch [{rec['epoch']}][{rec['iter']}/{n}]\tlr: {rec['lr']:.3e}, "
            head += f"time: {rec['time']:.3f}, data_time: {rec['data_time']:.3f}, "
            if 'memory' in rec:
                head += f"memory: {rec['memory']}, "
        else:
            head = f"Epoch({rec['mode']}) [{rec['epoch']}][{rec['iter']}]\t"
        items = [f'{k}: {v:.4f}' if isinstance(v, float) else f'{k}: {v}' for k, v in rec.items()
                 if k not in ('mode', 'epoch', 'iter', 'lr', 'time', 'data_time', 'memory')]
        self.logger.info(head + ', '.join(items))
        if self.rank == 0:
            self._dump({k: _round_float(v) for k, v in rec.items()})

    def _dump(self, rec):
        import json
        with open(self.json_log, 'a+') as f:
            json.dump(rec, f)
            f.write('\n')

    # ------------------------------------------------------------------------------------------ checkpoint
    def save_checkpoint(self):
        """CheckpointHook on rank 0: epoch_{n}.pth, latest.pth -> epoch_{n}.pth (a link, as mmcv makes it)."""
        if self.rank != 0:
            return None
        meta = dict(self.meta, rng=rng_state())
        path = os.path.join(self.work_dir, f'epoch_{self.epoch + 1}.pth')
        self.trainer.save_checkpoint(path, meta=meta)
        latest = os.path.join(self.work_dir, 'latest.pth')
        if os.path.lexists(latest):
            os.remove(latest)
        try:
            os.symlink(os.path.basename(path), latest)
        except OSError:
            import shutil
            shutil.copy(path, latest)
        return path


def train_detector(model, dataset, cfg, distributed=False, validate=False, timestamp=None, meta=None, batch_fn=collate):
    """mmdet/apis/train.py:train_detector for a model already on its device (the CLI moves it there): the loader of
    `dataset` (shuffled, seeded with cfg.seed, persistent workers), a Trainer from cfg.optimizer / cfg.lr_config with
    the loader's length as the epoch, the hooks, cfg.resume_from / cfg.load_from, then cfg.total_epochs epochs.
    batch_fn(samples, device) makes the step's input from a loader batch (default: pipelines.collate).
    -> the EpochRunner (its log_history and timing)."""
    from .datasets import build_dataloader, build_dataset, replace_ImageToTensor
    from .runner import Trainer
    apply_runtime_defaults(cfg)
    check_supported(cfg)
    datasets = dataset if isinstance(dataset, (list, tuple)) else [dataset]
    if len(datasets) != 1:
        raise NotImplementedError('workflow: only one (train) dataset is supported')
    dataset = datasets[0]
    if get_dist_info()[0] == 0:
        os.makedirs(cfg.work_dir, exist_ok=True)
    logger = get_root_logger(os.path.join(cfg.work_dir, f'{timestamp}.log') if timestamp else None,
                             cfg.get('log_level', 'INFO'))
    workers = cfg.data.workers_per_gpu
    loader = build_dataloader(dataset, cfg.data.samples_per_gpu, workers, 1, dist=distributed, shuffle=True,
                              seed=cfg.get('seed'), **(dict(persistent_workers=True) if workers > 0 else {}))
    trainer = Trainer(model, cfg=cfg, iters_per_epoch=len(loader))
    meta = dict(meta or {})
    classes = getattr(dataset, 'CLASSES', None)
    if classes is not None:
        meta['CLASSES'] = list(classes)
    eval_hook = None
    if validate:
        val_cfg = cfg.data.val.to_dict()
        val_spg = val_cfg.pop('samples_per_gpu', 1)
        if val_spg > 1:
            val_cfg['pipeline'] = replace_ImageToTensor(val_cfg['pipeline'])
        val_cfg['test_mode'] = True
        val_set = build_dataset(val_cfg)
        val_loader = build_dataloader(val_set, val_spg, workers, dist=distributed, shuffle=False,
                                      **(dict(persistent_workers=True) if workers > 0 else {}))
        ev = dict(cfg.get('evaluation') or {})
        eval_hook = EvalHook(val_loader, distributed=distributed, **ev)
    ckpt_cfg = cfg.get('checkpoint_config')
    runner = EpochRunner(trainer, loader, cfg.work_dir, cfg.total_epochs, logger=logger, meta=meta, timestamp=timestamp,
                         checkpoint_interval=(ckpt_cfg or {}).get('interval', 1) if ckpt_cfg is not None else 0,
                         log_interval=cfg.log_config.get('interval', 50), eval_hook=eval_hook, batch_fn=batch_fn,
                         distributed=distributed)
    if cfg.get('resume_from'):
        runner.resume(cfg.resume_from)
    elif cfg.get('load_from'):
        runner.load_checkpoint(cfg.load_from)
    runner.run()
    return runner
