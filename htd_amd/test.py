"""Score a checkpoint: python -m htd_amd.test CONFIG CHECKPOINT [--out FILE.pkl] [--eval bbox ...] [--format-only]
                                         [--eval-options k=v ...] [--cfg-options k=v ...] [--launcher none|pytorch]

The counterpart of the reference's tools/test.py for HTD configs: build `data.test`, load the checkpoint, run the
model over every image (htd_amd.apis) and evaluate or format the results.  With `--launcher pytorch` (under
`torch.distributed.run`) every rank tests its share and rank 0 collects, writes and evaluates.
"""
import argparse
import ast
import os
import pickle


def _value(text):
    """A --cfg-options / --eval-options value: a Python literal when it is one, a comma list, else the string."""
    try:
        return ast.literal_eval(text)
    except (ValueError, SyntaxError):
        pass
    if ',' in text:
        return [_value(v) for v in text.split(',') if v]
    return text


class _DictAction(argparse.Action):
    def __call__(self, parser, namespace, values, option_string=None):
        out = dict(getattr(namespace, self.dest, None) or {})
        for kv in values:
            if '=' not in kv:
                raise argparse.ArgumentError(self, f'expected key=value, got {kv!r}')
            k, v = kv.split('=', 1)
            out[k] = _value(v)
        setattr(namespace, self.dest, out)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Test (and evaluate) an HTD checkpoint on a COCO-format dataset')
    p.add_argument('config', help='test config file (e.g. configs/htd/htd_resnet50_1x.py)')
    p.add_argument('checkpoint', help='checkpoint file')
    p.add_argument('--out', help='write the results to this pickle file')
    p.add_argument('--format-only', action='store_true', help='write the result json files without evaluating')
    p.add_argument('--eval', type=str, nargs='+', help='metrics: bbox, proposal, proposal_fast (COCO); mAP, recall (VOC)')
    p.add_argument('--eval-options', nargs='+', action=_DictAction, help='key=value keyword arguments of '
                   'dataset.evaluate (or dataset.format_results with --format-only)')
    p.add_argument('--cfg-options', nargs='+', action=_DictAction, help='key=value overrides merged into the config, '
                   'e.g. data.test.ann_file=... data.test.img_prefix=...')
    p.add_argument('--launcher', choices=['none', 'pytorch'], default='none', help='job launcher')
    p.add_argument('--trust-checkpoint', action='store_true', help='allow a checkpoint whose meta holds pickled '
                   'objects beyond tensors and plain containers (unpickling runs code: trusted files only)')
    p.add_argument('--local_rank', type=int, default=0)
    args = p.parse_args(argv)
    if not (args.out or args.eval or args.format_only):
        p.error('specify at least one of --out, --eval and --format-only')
    if args.eval and args.format_only:
        raise ValueError('--eval and --format_only cannot be both specified')
    if args.out is not None and not args.out.endswith(('.pkl', '.pickle')):
        raise ValueError('The output file must be a pkl file.')
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch
    import torch.distributed as dist

    from . import detector  # noqa: F401  (registers the model components)
    from .apis import multi_gpu_test, single_gpu_test
    from .checkpoint import load_checkpoint
    from .datasets import build_dataloader, build_dataset, get_dist_info, replace_ImageToTensor
    from .registry import Config, build_detector

    cfg = Config.fromfile(args.config)
    if args.cfg_options:
        cfg.merge_from_dict(args.cfg_options)
    cfg.model.pretrained = None
    test_cfg = cfg.data.test
    test_cfg.test_mode = True
    distributed = args.launcher != 'none'
    if distributed:
        local_rank = int(os.environ.get('LOCAL_RANK', args.local_rank))
        torch.cuda.set_device(local_rank)
        dist.init_process_group('nccl')
    device = torch.device('cuda', torch.cuda.current_device())

    samples_per_gpu = test_cfg.pop('samples_per_gpu', 1)
    if samples_per_gpu > 1:
        test_cfg.pipeline = replace_ImageToTensor(test_cfg.pipeline)
    dataset = build_dataset(test_cfg.to_dict())
    loader = build_dataloader(dataset, samples_per_gpu=samples_per_gpu, workers_per_gpu=cfg.data.workers_per_gpu,
                              dist=distributed, shuffle=False)

    model = build_detector(cfg.model.to_dict(), train_cfg=None, test_cfg=cfg.get('test_cfg'))
    checkpoint = load_checkpoint(model, args.checkpoint, map_location='cpu', trusted=args.trust_checkpoint or None)
    meta = checkpoint.get('meta') or {}
    model.CLASSES = meta['CLASSES'] if 'CLASSES' in meta else dataset.CLASSES
    model = model.to(device)

    outputs = multi_gpu_test(model, loader) if distributed else single_gpu_test(model, loader)

    rank, _ = get_dist_info()
    if rank == 0:
        if args.out:
            print(f'\nwriting results to {args.out}')
            with open(args.out, 'wb') as f:
                pickle.dump(outputs, f)
        kwargs = dict(args.eval_options or {})
        if args.format_only:
            dataset.format_results(outputs, **kwargs)
        if args.eval:
            eval_kwargs = dict(cfg.get('evaluation') or {})
            for key in ('interval', 'tmpdir', 'start', 'gpu_collect', 'save_best', 'rule'):
                eval_kwargs.pop(key, None)
            eval_kwargs.update(dict(metric=args.eval, **kwargs))
            print(dataset.evaluate(outputs, **eval_kwargs))
    if distributed:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
