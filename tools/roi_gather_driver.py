#!/usr/bin/env python3
"""The gather-form RoIAlign backward entry points on one case, in a process of its own: HTD_ROI_BWD_SPLIT (how many wavefronts
share a tile: 1, 2 or 4) is read once per process, so the forced forms need a fresh one (tests/test_gpu_roi_align_ops.py starts this).

    HTD_ROI_BWD_SPLIT=4 python tools/roi_gather_driver.py case.npz out.npz [case2.npz out2.npz ...]

case.npz: rois (n, 5) f32, levels (n) i64, shapes (L, 4) = B, H, W, C per level, scales (L) f32, params = ph, pw, sampling_ratio,
aligned, grad0 .. grad{L-1} (n, ph, pw, C) f32.  out.npz: the gradient maps (B, H, W, C) of
  single             htd_roi_align_bwd_gather of grad0 on level 0's map, no level list
  levels{l}, levels_folded{l}   htd_roi_align_levels_bwd_gather(_folded) of grad0 by the level list
  all{l}, all_folded{l}         htd_roi_align_all_levels_bwd_gather(_folded) of grad{l}
every map NaN-filled before the launch (accumulate = 0 writes every pixel).
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from htd_amd import capi


def run(src, dst):
    case = np.load(src)
    dev = torch.device('cuda', 0)
    rois = torch.from_numpy(case['rois']).to(dev)
    levels = torch.from_numpy(case['levels']).to(dev)
    shapes = [tuple(int(v) for v in s) for s in case['shapes']]
    L = len(shapes)
    ph, pw, sr, aligned = (int(v) for v in case['params'])
    grads = [torch.from_numpy(case[f'grad{l}']).to(dev) for l in range(L)]
    n, (B, _, _, C) = rois.shape[0], shapes[0]
    lib = capi.lib()
    P, S = capi.ptr, capi.current_stream_ptr
    Hs, Ws = (ctypes.c_int * L)(*[s[1] for s in shapes]), (ctypes.c_int * L)(*[s[2] for s in shapes])
    sc, ac = (ctypes.c_float * L)(*[float(v) for v in case['scales']]), (ctypes.c_int * L)(*([0] * L))
    ws = torch.empty(L * lib.htd_roi_align_bwd_gather_workspace_bytes(n), dtype=torch.uint8, device=dev)
    fold = torch.empty(lib.htd_roi_align_fold_workspace_bytes(n, Hs, L, pw, C), dtype=torch.uint8, device=dev)

    def maps():
        return [torch.full(s, float('nan'), device=dev) for s in shapes]

    def table(ts):
        return (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])

    out = {}
    m = maps()[0]
    capi.call('htd_roi_align_bwd_gather', P(grads[0]), P(rois), None, 0, P(m), n, B, C, shapes[0][1], shapes[0][2], ph, pw,
              float(case['scales'][0]), sr, aligned, 0, P(ws), S())
    out['single'] = m
    ms = maps()
    capi.call('htd_roi_align_levels_bwd_gather', P(grads[0]), P(rois), P(levels), table(ms), Hs, Ws, sc, ac, L, n, B, C, ph, pw, sr,
              aligned, P(ws), S())
    out.update({f'levels{l}': t for l, t in enumerate(ms)})
    ms = maps()
    capi.call('htd_roi_align_levels_bwd_gather_folded', P(grads[0]), P(rois), P(levels), table(ms), Hs, Ws, sc, ac, L, n, B, C, ph, pw,
              sr, aligned, P(ws), P(fold), S())
    out.update({f'levels_folded{l}': t for l, t in enumerate(ms)})
    ms = maps()
    capi.call('htd_roi_align_all_levels_bwd_gather', table(grads), P(rois), table(ms), Hs, Ws, sc, ac, L, n, B, C, ph, pw, sr, aligned,
              P(ws), S())
    out.update({f'all{l}': t for l, t in enumerate(ms)})
    ms = maps()
    capi.call('htd_roi_align_all_levels_bwd_gather_folded', table(grads), P(rois), table(ms), Hs, Ws, sc, ac, L, n, B, C, ph, pw, sr,
              aligned, P(ws), P(fold), S())
    out.update({f'all_folded{l}': t for l, t in enumerate(ms)})
    torch.cuda.synchronize()
    np.savez(dst, **{k: v.cpu().numpy() for k, v in out.items()})


if __name__ == '__main__':
    for i in range(1, len(sys.argv) - 1, 2):
        run(sys.argv[i], sys.argv[i + 1])
