"""Train a detector: python -m htd_amd.train CONFIG [--work-dir DIR] [--resume-from FILE] [--no-validate]
                                            [--gpus N | --gpu-ids I ...] [--seed 1] [--deterministic]
                                            [--cfg-options k=v ...] [--launcher none|pytorch] [--local_rank R]

The counterpart of the reference's tools/train.py for HTD configs: merge the config, make the work directory (the
merged config, `<timestamp>.log`, `<timestamp>.log.json`, `epoch_{n}.pth`, `latest.pth`), seed, build the detector and
`data.train`, and run htd_amd.apis.train_detector.  One process drives one GPU: several GPUs are used through
`python -m torch.distributed.run --nproc-per-node N -m htd_amd.train CONFIG --launcher pytorch`.

`--resume-from` restores the weights, the optimizer state, the epoch and iteration and the python / numpy / torch / HIP
generators saved with the checkpoint, so a single-process run with `data.workers_per_gpu=0` continues exactly as if it
had not stopped.  With loader workers the resumed run draws its random flips from freshly seeded workers, as the
reference's does; in a distributed run every rank restores rank 0's generators.
"""
import argparse
import os
import os.path as osp
import sys
import time
import warnings

from .test import _DictAction


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Train a detector')
    p.add_argument('config', help='train config file path')
    p.add_argument('--work-dir', help='the dir to save logs and models')
    p.add_argument('--resume-from', help='the checkpoint file to resume from')
    p.add_argument('--no-validate', action='store_true', help='whether not to evaluate the checkpoint during training')
    gpus = p.add_mutually_exclusive_group()
    gpus.add_argument('--gpus', type=int, help='number of gpus to use (non-distributed training: 1)')
    gpus.add_argument('--gpu-ids', type=int, nargs='+', help='ids of gpus to use (non-distributed training: one id)')
    p.add_argument('--seed', type=int, default=1, help='random seed')
    p.add_argument('--deterministic', action='store_true', help='whether to set deterministic options for the backend')
    p.add_argument('--options', nargs='+', action=_DictAction, help='deprecated spelling of --cfg-options')
    p.add_argument('--cfg-options', nargs='+', action=_DictAction, help='key=value overrides merged into the config')
    p.add_argument('--launcher', choices=['none', 'pytorch'], default='none', help='job launcher')
    p.add_argument('--local_rank', type=int, default=0)
    args = p.parse_args(argv)
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(args.local_rank)
    if args.options and args.cfg_options:
        raise ValueError('--options and --cfg-options cannot be both specified, --options is deprecated in favor of '
                         '--cfg-options')
    if args.options:
        warnings.warn('--options is deprecated in favor of --cfg-options')
        args.cfg_options = args.options
    if args.launcher == 'none':
        n = args.gpus if args.gpus is not None else len(args.gpu_ids or [0])
        if n != 1:
            p.error(f'a non-distributed run trains on exactly one GPU, {n} were asked for; for several GPUs start one '
                    'process per GPU: python -m torch.distributed.run --nproc-per-node N -m htd_amd.train CONFIG '
                    '--launcher pytorch')
    return args


def work_dir_of(args, cfg):
    """The work directory in the reference's priority: --work-dir, then cfg.work_dir, then ./work_dirs/<config name>."""
    if args.work_dir is not None:
        return args.work_dir
    if cfg.get('work_dir', None) is not None:
        return cfg.work_dir
    return osp.join('./work_dirs', osp.splitext(osp.basename(args.config))[0])


def dump_config(cfg, filename):
    """One `key = repr(value)` line per top-level key: Config.fromfile reads the file back to the same dict."""
    with open(filename, 'w') as f:
        for k, v in cfg._cfg_dict.to_dict().items():
            f.write(f'{k} = {v!r}\n')
    with open(filename) as f:
        return f.read()


def load_config(args):
    """The merged config with the runtime keys a config may lack, checked for settings this runner does not have."""
    from .apis import apply_runtime_defaults, check_supported
    from .registry import Config
    cfg = Config.fromfile(args.config)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    apply_runtime_defaults(cfg)
    check_supported(cfg)
    cfg.work_dir = work_dir_of(args, cfg)
    if args.resume_from is not None:
        cfg.resume_from = args.resume_from
    return cfg


def main(argv=None):
    args = parse_args(argv)
    cfg = load_config(args)
    import torch
    import torch.distributed as dist

    from . import detector  # noqa: F401  (registers the model components)
    from .apis import env_info, get_root_logger, set_random_seed, train_detector
    from .datasets import build_dataset, get_dist_info
    from .registry import build_detector

    distributed = args.launcher != 'none'
    if distributed:
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', args.local_rank)))
        dist.init_process_group((cfg.get('dist_params') or {}).get('backend', 'nccl'))
        cfg.gpu_ids = list(range(get_dist_info()[1]))
    else:
        cfg.gpu_ids = list(args.gpu_ids or [0])
        torch.cuda.set_device(cfg.gpu_ids[0])
    rank, _ = get_dist_info()
    timestamp = time.strftime('%Y%m%d_%H%M%S', time.localtime())
    if distributed:                                   # one timestamp for every rank's file names
        stamp = [timestamp]
        dist.broadcast_object_list(stamp, src=0)
        timestamp = stamp[0]
    cfg.seed = args.seed
    config_text = None
    if rank == 0:
        os.makedirs(osp.abspath(cfg.work_dir), exist_ok=True)
        config_text = dump_config(cfg, osp.join(cfg.work_dir, osp.basename(args.config)))
    logger = get_root_logger(osp.join(cfg.work_dir, f'{timestamp}.log'), cfg.get('log_level', 'INFO'))
    info = env_info()
    dash = '-' * 60 + '\n'
    logger.info('Environment info:\n' + dash + info + '\n' + dash)
    logger.info(f'Distributed training: {distributed}')
    logger.info(f'Config:\n{config_text}')
    logger.info(f'Set random seed to {args.seed}, deterministic: {args.deterministic}')
    set_random_seed(args.seed, deterministic=args.deterministic)
    meta = dict(env_info=info, config=config_text or '', seed=args.seed, exp_name=osp.basename(args.config))

    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    model = build_detector(cfg.model.to_dict(), train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    dataset = build_dataset(cfg.data.train.to_dict())
    model.CLASSES = dataset.CLASSES
    model = model.to(torch.device('cuda', torch.cuda.current_device()))
    train_detector(model, [dataset], cfg, distributed=distributed, validate=not args.no_validate, timestamp=timestamp,
                   meta=meta)
    if distributed:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
