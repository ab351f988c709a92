"""The kernels that decide which anchors and proposals a two-stage model trains on, each against the independent numpy / Python
restatement of tests/select_ref.py (pinned on the CPU by tests/test_select_ref.py), at every path and edge of the kernels:

  csrc/topk.hip      htd_segmented_topk (radix select + LDS sort), htd_random_sample (RandomSampler for a batch)
  csrc/box_ops.hip   htd_max_iou_assign, htd_static_samples_finish, htd_rpn_heads_gather / _scatter

Every comparison is exact: equal indices, masks and counts, and equal bit patterns of the float outputs.  These kernels have no
tolerance: a wrong element draws a slightly different sample, which no loss tolerance downstream would notice."""
import ctypes

import numpy as np
import pytest
import torch

import select_ref as R

pytestmark = pytest.mark.gpu

CHUNK, KMAX = 4096, 2048           # keys per workgroup of the select passes, survivors per segment (csrc/topk.hip)
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bits(t):
    """int32 image of a float32 tensor / array (host)."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def from_bits(b):
    return T(np.asarray(b, dtype=np.uint32).view(np.float32))


# ====================================================================================================== segmented top-k
def layout(parts, ks):
    segs, off = [], 0
    for p, k in zip(parts, ks):
        segs.append((off, p.numel(), k))
        off += p.numel()
    keys = torch.cat([p.float() for p in parts]) if off else torch.zeros(0)
    return keys, segs


def check_topk(parts, ks, idx, val):
    idx, val = idx.cpu().numpy(), val.cpu()
    o = 0
    for i, (p, k) in enumerate(zip(parts, ks)):
        p = p.float().numpy()
        want = R.topk_ref(p, k)
        assert np.array_equal(idx[o:o + k], want), (i, k)
        assert np.array_equal(bits(val[o:o + k]), bits(p[want])), (i, k)       # a -0 comes back as -0, a NaN as the NaN it was
        o += k
    assert o == idx.size


def topk_case(dev, parts, ks):
    import htd_amd.mmcv_ops as M
    keys, segs = layout(parts, ks)
    idx, val = M.segmented_topk(keys.to(dev), segs)
    check_topk(parts, ks, idx, val)
    return idx, val


def distinct(n, seed):
    """n distinct keys in [0, 0.5) in random order (multiples of 2^-22, exact in fp32 for n <= 2^21)."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).float() * 2.0 ** -22


def test_topk_length_against_k(dev):
    """len == k (the selection is skipped), len == k + 1 (one key is dropped), k = 1 where the maximum is the only key of the
    segment's second chunk, and the largest k on segments of one chunk, one chunk and a key, two chunks, two chunks and a key."""
    g = torch.Generator().manual_seed(1)
    one = torch.rand(4097, generator=g)
    one[4096] = 2.0
    one2 = torch.rand(4097, generator=g)
    one2[4000] = 2.0
    parts = [torch.rand(100, generator=g), torch.rand(101, generator=g), one, one2, torch.rand(2048, generator=g),
             torch.rand(2048, generator=g), torch.rand(2049, generator=g), torch.rand(4096, generator=g),
             torch.rand(4097, generator=g), torch.rand(2, generator=g), torch.rand(65, generator=g)]
    ks = [100, 100, 1, 1, 2048, 2047, 2048, 2048, 2048, 1, 64]
    topk_case(dev, parts, ks)


def test_topk_sort_sizes_and_run_to_run_equality(dev):
    """k on both sides of the bitonic network's sizes (64, 1024; 2048 is the cap) on 5000 distinct keys: k - 1 keys above the
    threshold land in slots handed out by atomicAdd, so the call is made twice and must give the same bits."""
    import htd_amd.mmcv_ops as M
    ks = [63, 64, 65, 1023, 1024, 1025, 1, 2047]
    parts = [distinct(5000, 10 + i) - 0.25 for i in range(len(ks))]
    idx, val = topk_case(dev, parts, ks)
    keys, segs = layout(parts, ks)
    idx2, val2 = M.segmented_topk(keys.to(dev), segs)
    assert torch.equal(idx, idx2) and torch.equal(val.view(torch.int32), val2.view(torch.int32))


def test_topk_keys_that_differ_only_in_their_low_bits(dev):
    """Keys that share their top 22 bits (1 + j 2^-23, j < 1024, with duplicates: the last histogram pass alone discriminates),
    keys that share their top 11 bits and differ in bits 20..10 only (the middle pass alone), and both negated (the
    complemented images of negative floats)."""
    rng = np.random.RandomState(4)
    low = from_bits(0x3F800000 + rng.randint(0, 1024, 9000))                 # [1, 1 + 2^-13)
    mid = from_bits(0x3F800000 + (rng.randint(0, 2048, 9000) << 10))         # [1, 1.25): top 11 bits 0x3F8 | 00, low 10 bits zero
    assert low.unique().numel() <= 1024 and float(low.max()) < 1.0 + 2.0 ** -13 and mid.unique().numel() > 1500
    parts = [low, mid, -low, -mid, low[:4097], -mid[:4096]]
    topk_case(dev, parts, [500, 500, 500, 500, 2048, 7])


def test_topk_special_values(dev):
    """Denormals of both signs, +-inf, +-FLT_MAX, runs of -0 and +0 (equal keys: position decides, the sign bit comes back as
    it went in), a segment of negative keys only, and NaNs of either sign (largest, in position order)."""
    rng = np.random.RandomState(6)
    FMAX = 3.4028234663852886e38
    den = from_bits(rng.randint(1, 1 << 23, 6000).astype(np.uint32) | (rng.randint(0, 2, 6000).astype(np.uint32) << 31))
    assert float(den.abs().max()) < 1.1754944e-38 and bool((den != 0).all())
    zeros = torch.cat([-torch.zeros(30), torch.zeros(5000), -torch.zeros(30), torch.zeros(40)])
    zeros[rng.permutation(5100)[:9]] = 1e-45                                  # a few keys above the run of zeros
    special = torch.tensor([0.0, -0.0, float('inf'), -float('inf'), FMAX, -FMAX, 1e-45, -1e-45, 1.0, -1.0])
    mixed = torch.cat([torch.randn(4500, generator=torch.Generator().manual_seed(2)), special.repeat(3)])
    negative = -torch.rand(7000, generator=torch.Generator().manual_seed(3)) - 1e-3
    nans = torch.cat([torch.randn(4300, generator=torch.Generator().manual_seed(5)), torch.tensor([NAN, -NAN, float('inf')])])
    parts = [den, zeros, mixed, negative, torch.cat([den[:3000], zeros[:2000]]), nans, special]
    topk_case(dev, parts, [700, 50, 2048, 33, 2048, 10, 9])


def many_chunk_ties():
    """One segment of 1.5 M keys (367 chunks): the threshold value 0.75 sits at 2500 sparse positions, k = 2000 takes the five
    1.0 keys near the end and the first 1995 ties in position order.  A workgroup past chunk 256 counts the ties of MORE than
    256 earlier chunks, the second trip of the loop in topk_compact_kernel.  -> parts, ks of the call"""
    N, k = 367 * CHUNK - 1234, 2000
    keys = distinct(N, 7)
    tie_pos = torch.arange(2500) * 600 + 17
    assert int(tie_pos[-1]) < N - 100
    keys[tie_pos] = 0.75
    keys[N - 60:N - 10:10] = 1.0
    small = torch.rand(300, generator=torch.Generator().manual_seed(8))
    want = R.topk_ref(keys.numpy(), k)
    ties_taken = want[keys.numpy()[want] == 0.75]
    assert len(ties_taken) == k - 5 and int(ties_taken.max()) >= 256 * CHUNK            # the selection crosses chunk 256 ...
    assert int((ties_taken >= 256 * CHUNK).sum()) > 100 and int(tie_pos[-1]) > int(ties_taken.max())      # ... and stops inside
    return [small, keys, small], [10, k, 300]


def test_topk_ties_at_the_threshold_over_more_than_256_chunks(dev):
    topk_case(dev, *many_chunk_ties())


def test_topk_degenerate_segments_between_selecting_ones(dev):
    """A zero-length segment and a k = 0 segment between segments that select, a one-key segment as the last of the call."""
    g = torch.Generator().manual_seed(9)
    parts = [torch.rand(5000, generator=g), torch.zeros(0), torch.rand(9000, generator=g), torch.rand(300, generator=g),
             torch.randn(4100, generator=g), torch.tensor([-3.0])]
    topk_case(dev, parts, [100, 0, 2048, 0, 17, 1])


def raw_topk(dev, keys, segs, fill):
    """htd_segmented_topk through the C ABI with a workspace filled with `fill` and outputs filled with (-7, NaN)."""
    from htd_amd import capi
    rows, chunks, out = [], [], 0
    for s, (start, length, k) in enumerate(segs):
        rows.append((start, length, k, out))
        out += k
        chunks.extend((s, c) for c in range((length + CHUNK - 1) // CHUNK))
    seg_t = torch.tensor(rows, dtype=torch.int64, device=dev)
    tab_t = torch.tensor(chunks, dtype=torch.int32, device=dev)
    ws = torch.full((capi.lib().htd_segmented_topk_workspace_bytes(len(rows), len(chunks)), ), fill, dtype=torch.uint8, device=dev)
    idx = torch.full((out, ), -7, dtype=torch.int64, device=dev)
    val = torch.full((out, ), NAN, dtype=torch.float32, device=dev)
    capi.call('htd_segmented_topk', capi.ptr(keys), capi.ptr(seg_t), capi.ptr(tab_t), len(rows), len(chunks), capi.ptr(idx),
              capi.ptr(val), capi.ptr(ws), capi.current_stream_ptr())
    torch.cuda.synchronize()
    return idx, val


def test_topk_dirty_workspace_and_rejections(dev):
    """Only the zeroed prefix of the workspace may matter and the entry point zeroes it itself: a workspace full of 0xFF gives
    the result of a clean one.  Bad arguments raise and leave the outputs as they were."""
    g = torch.Generator().manual_seed(12)
    parts = [(torch.rand(9000, generator=g) * 32).floor() / 32, torch.rand(100, generator=g), torch.rand(5000, generator=g),
             torch.zeros(0), torch.rand(4097, generator=g)]
    ks = [1500, 100, 2048, 0, 1]
    keys, segs = layout(parts, ks)
    keys = keys.to(dev)
    clean = raw_topk(dev, keys, segs, 0)
    dirty = raw_topk(dev, keys, segs, 0xFF)
    check_topk(parts, ks, *dirty)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1].view(torch.int32), dirty[1].view(torch.int32))
    # S < 0, keys = NULL, chunks without their table: the outputs of a rejected call are filled before and untouched after
    from htd_amd import capi
    idx = torch.full((10, ), -7, dtype=torch.int64, device=dev)
    val = torch.full((10, ), NAN, dtype=torch.float32, device=dev)
    seg_t = torch.tensor([(0, 9000, 10, 0)], dtype=torch.int64, device=dev)
    tab_t = torch.tensor([(0, 0), (0, 1), (0, 2)], dtype=torch.int32, device=dev)
    ws = torch.zeros(capi.lib().htd_segmented_topk_workspace_bytes(1, 3), dtype=torch.uint8, device=dev)
    for args in ((capi.ptr(keys), capi.ptr(seg_t), capi.ptr(tab_t), -1, 3), (None, capi.ptr(seg_t), capi.ptr(tab_t), 1, 3),
                 (capi.ptr(keys), capi.ptr(seg_t), None, 1, 3)):
        with pytest.raises(ValueError):
            capi.call('htd_segmented_topk', *args, capi.ptr(idx), capi.ptr(val), capi.ptr(ws), capi.current_stream_ptr())
        torch.cuda.synchronize()
        assert bool((idx == -7).all()) and bool(torch.isnan(val).all())


# ====================================================================================================== random sampler
def check_sample(dev, assigned, keys, num, frac, ub, slots):
    """random_sample_device on the batch against random_sample_ref image by image: masks, counts, order[:n], order[n:] == 0."""
    from htd_amd.core import bbox as Bx
    B, A = assigned.shape
    pos, neg, counts, order = Bx.random_sample_device(assigned.to(dev), keys.to(dev), num, frac, ub, slots=slots)
    torch.cuda.synchronize()
    pos, neg, counts = pos.cpu().numpy(), neg.cpu().numpy(), counts.cpu().numpy()
    assert (order is None) == (slots == 0)
    drawn = []
    for b in range(B):
        rp, rn, ro = R.random_sample_ref(assigned[b].numpy(), keys[b].numpy(), num, frac, ub)
        print('image %d: drawn (pos, neg) = (%d, %d), reference (%d, %d)' % (b, counts[b, 0], counts[b, 1], len(rp), len(rn)))
        assert counts[b].tolist() == [len(rp), len(rn)], b
        assert np.flatnonzero(pos[b]).tolist() == rp and np.flatnonzero(neg[b]).tolist() == rn, b
        if order is not None:
            ob = order[b].cpu().tolist()
            n = min(len(ro), slots)
            assert ob[:n] == ro[:n] and not any(ob[n:]), b
        drawn.append((len(rp), len(rn)))
    return drawn


def rand_assigned(g, B, A, pos_rate, ignore_rate=0.1):
    a = torch.where(torch.rand(B, A, generator=g) < pos_rate, torch.randint(1, 9, (B, A), generator=g), torch.zeros(B, A, dtype=torch.long))
    return torch.where(torch.rand(B, A, generator=g) < ignore_rate, torch.full_like(a, -1), a)


@pytest.mark.parametrize('B,A,num,frac,ub,pos_rate,slots', [
    (3, 5000, 2048, 0.5, -1, 0.3, 2048),        # the largest sample: both rankings fill the LDS sort
    (2, 300, 512, 0.25, -1, 0.5, 512),          # fewer candidates than slots
    (2, 5000, 256, 0.0, -1, 0.2, 256),          # pos_fraction = 0: kpos = 0, negatives only
    (2, 5000, 256, 1.0, 3, 0.2, 256),           # pos_fraction = 1: positives may take every slot
    (3, 4097, 128, 0.5, 0, 0.05, 128),          # neg_pos_ub = 0: no negatives
    (3, 9000, 512, 0.25, 2, 0.002, 0),          # order = NULL; the bound decides
    (2, 5000, 200, 0.5, -1, 0.3, 37),           # slots < drawn
    (2, 5000, 200, 0.5, 1, 0.01, 333),          # slots > num
])
def test_random_sample_against_the_reference(dev, B, A, num, frac, ub, pos_rate, slots):
    g = torch.Generator().manual_seed(A + num + slots)
    assigned = rand_assigned(g, B, A, pos_rate)
    keys = torch.rand(B, A, generator=g)
    drawn = check_sample(dev, assigned, keys, num, frac, ub, slots)
    assert any(p + n > 0 for p, n in drawn)


def test_random_sample_one_candidate(dev):
    """A = 1: a positive, a negative and an ignored candidate, one per image."""
    assigned = torch.tensor([[3], [0], [-1]])
    keys = torch.tensor([[0.5], [0.25], [0.75]])
    assert check_sample(dev, assigned, keys, 4, 0.5, -1, 4) == [(1, 0), (0, 1), (0, 0)]
    assert check_sample(dev, assigned, keys, 1, 1.0, -1, 2) == [(1, 0), (0, 1), (0, 0)]
    assert check_sample(dev, assigned, keys, 1, 0.0, 0, 2) == [(0, 0), (0, 0), (0, 0)]


def test_random_sample_uniform_images_in_one_batch(dev):
    """Images that are all ignored, all positive, all negative and mixed share one call."""
    g = torch.Generator().manual_seed(21)
    A = 4500
    assigned = torch.stack([torch.full((A, ), -1), torch.full((A, ), 2), torch.zeros(A, dtype=torch.long), rand_assigned(g, 1, A, 0.1)[0]])
    keys = torch.rand(4, A, generator=g)
    assert check_sample(dev, assigned, keys, 512, 0.25, -1, 512)[:3] == [(0, 0), (128, 0), (0, 512)]
    assert check_sample(dev, assigned, keys, 512, 0.25, 3, 512)[:3] == [(0, 0), (128, 0), (0, 3)]


@pytest.mark.parametrize('ub,n_pos,n_neg', [(0.29, 100, 28), (0.7, 90, 62), (2.3, 50, 114)])
def test_random_sample_fractional_neg_pos_ub(dev, ub, n_pos, n_neg):
    """int(neg_pos_ub * n_pos) is a double product in the reference (base_sampler.py:90-92): 0.29 * 100 -> 28, 0.7 * 90 -> 62,
    2.3 * 50 -> 114.  The same product in fp32 rounds up to the next integer and draws one negative too many."""
    g = torch.Generator().manual_seed(n_pos)
    B, A, num = 2, 5000, 512
    assigned = torch.zeros(B, A, dtype=torch.long)
    for b in range(B):
        p = torch.randperm(A, generator=g)
        assigned[b, p[:n_pos]] = torch.randint(1, 9, (n_pos, ), generator=g)
        assigned[b, p[n_pos:n_pos + 400]] = -1
    keys = torch.rand(B, A, generator=g)
    assert int(ub * n_pos) == n_neg and int(num * 0.5) >= n_pos and num - n_pos >= n_neg + 1
    assert check_sample(dev, assigned, keys, num, 0.5, ub, num) == [(n_pos, n_neg)] * B


def test_random_sample_extreme_and_duplicate_keys(dev):
    """Keys of exactly 0.0 (negated to -0 by the staging kernel), of 1 - 2^-24 (the largest below 1) and heavy duplicates:
    equal keys are drawn by ascending index."""
    g = torch.Generator().manual_seed(31)
    B, A = 3, 6000
    assigned = rand_assigned(g, B, A, 0.3)
    table = torch.tensor([0.0, 1.0 - 2.0 ** -24, 0.5, 0.25, 2.0 ** -30, 0.75])
    keys = table[torch.randint(0, 6, (B, A), generator=g)]
    keys[1] = torch.where(torch.rand(A, generator=g) < 0.5, torch.zeros(A), torch.full((A, ), 1.0 - 2.0 ** -24))
    keys[2] = 0.0
    assert float(keys.max()) < 1.0 and int((keys == 0).sum()) > A
    check_sample(dev, assigned, keys, 512, 0.25, -1, 512)
    check_sample(dev, assigned, keys, 2048, 0.5, 1, 2048)


def test_random_sample_rejections(dev):
    from htd_amd import capi
    from htd_amd.core import bbox as Bx
    assigned = torch.zeros(1, 100, dtype=torch.long, device=dev)
    keys = torch.rand(1, 100, device=dev)
    with pytest.raises(ValueError):
        Bx.random_sample_device(assigned, keys, 2049, 0.5)             # num > 2048
    with pytest.raises(ValueError):
        Bx.random_sample_device(assigned, keys, 64, 1.5)               # max_pos > num
    segs = torch.tensor([(0, 100, 32, 0), (100, 100, 64, 32)], dtype=torch.int64, device=dev)
    tab = torch.tensor([(0, 0), (1, 0)], dtype=torch.int32, device=dev)
    pos, neg = torch.zeros(1, 100, dtype=torch.bool, device=dev), torch.zeros(1, 100, dtype=torch.bool, device=dev)
    counts = torch.full((1, 2), -7, dtype=torch.int64, device=dev)
    ws = torch.zeros(capi.lib().htd_random_sample_workspace_bytes(1, 100, 2), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):                                    # nchunks = 0
        capi.call('htd_random_sample', capi.ptr(assigned), capi.ptr(keys), 1, 100, 64, 32, -1.0, capi.ptr(segs), capi.ptr(tab), 0,
                  capi.ptr(pos), capi.ptr(neg), capi.ptr(counts), None, 0, capi.ptr(ws), capi.current_stream_ptr())
    torch.cuda.synchronize()
    assert counts.tolist() == [[-7, -7]]
    # the same call with its two chunks is accepted
    capi.call('htd_random_sample', capi.ptr(assigned), capi.ptr(keys), 1, 100, 64, 32, -1.0, capi.ptr(segs), capi.ptr(tab), 2,
              capi.ptr(pos), capi.ptr(neg), capi.ptr(counts), None, 0, capi.ptr(ws), capi.current_stream_ptr())
    torch.cuda.synchronize()
    assert counts.tolist() == [[0, 64]] and int(neg.sum()) == 64 and int(pos.sum()) == 0


# ====================================================================================================== MaxIoU assigner
RPN_THR = dict(pos=0.7, neg=0.3, min_pos=0.3)
RCNN_THR = dict(pos=0.5, neg=0.5, min_pos=0.5)


def rand_boxes(rng, shape, span=300., lo=2., hi=120.):
    xy = rng.rand(*shape, 2).astype(np.float32) * np.float32(span)
    wh = rng.rand(*shape, 2).astype(np.float32) * np.float32(hi - lo) + np.float32(lo)
    return np.concatenate([xy, xy + wh], -1)


def check_assign(dev, boxes, box_valid, gts, gt_valid, pos, neg, min_pos, low_quality):
    """batched_max_iou_assign on the device against max_iou_assign_ref image by image, both outputs bit for bit.
    boxes (A, 4) shared or (B, A, 4), numpy."""
    from htd_amd.core import bbox as Bx
    a = Bx.MaxIoUAssigner(pos_iou_thr=pos, neg_iou_thr=neg, min_pos_iou=min_pos, match_low_quality=low_quality, ignore_iof_thr=-1)
    got, ov = Bx.batched_max_iou_assign(a, T(boxes).to(dev), T(box_valid).to(dev), T(gts).to(dev), T(gt_valid).to(dev))
    torch.cuda.synchronize()
    got, ov = got.cpu().numpy(), ov.cpu().numpy()
    assert got.dtype == np.int64 and ov.dtype == np.float32
    for b in range(gt_valid.shape[0]):
        want, want_ov = R.max_iou_assign_ref(boxes if boxes.ndim == 2 else boxes[b], box_valid[b], gts[b], gt_valid[b], pos, neg,
                                             min_pos, low_quality)
        bad = np.flatnonzero(got[b] != want)
        assert bad.size == 0, (b, bad[:8], got[b][bad[:8]], want[bad[:8]])
        assert np.array_equal(bits(ov[b]), bits(want_ov)), b
    return got


def assign_inputs(rng, B, A, K, shared):
    """Random boxes and gts with duplicate gts, boxes equal to gts, zero-area boxes and gts, padded gts in image 1 and about a
    tenth of the boxes invalid."""
    boxes = rand_boxes(rng, (B, A))
    gts = rand_boxes(rng, (B, K), lo=4., hi=150.)
    if K > 1:
        gts[:, 1] = gts[:, 0]                                    # duplicate gts: the first wins the arg-max, the last the low-quality match
    if K > 4:
        gts[:, 4, 2:] = gts[:, 4, :2]                            # a gt of zero area
    m = min(A, K)
    boxes[:, :m] = gts[:, :m] if not shared else gts[:1, :m]     # boxes equal to gts: IoU exactly 1
    if A > K + 2:
        boxes[:, K + 1, 2:] = boxes[:, K + 1, :2]                # a box of zero area
        if K > 4:
            boxes[:, K + 2] = gts[:, 4]                          # ... and one equal to the zero-area gt
    gt_valid = np.ones((B, K), bool)
    if B > 1 and K > 1:
        gt_valid[1, K // 2:] = False                             # padded gts
    gts = gts * gt_valid[..., None]
    box_valid = rng.rand(B, A) > 0.1 if A > 1 else np.ones((B, A), bool)
    return (boxes[0] if shared else boxes), box_valid, gts, gt_valid


@pytest.mark.parametrize('shared', [True, False])
@pytest.mark.parametrize('low_quality', [True, False])
def test_max_iou_assign_at_the_block_and_chunk_boundaries(dev, shared, low_quality):
    """A in {1, 255, 256, 257} (one thread, one short of a workgroup, exactly one, one more) with K in {1, 127, 128, 129, 257}
    (around one and two chunks of 128 gts in LDS)."""
    rng = np.random.RandomState(40 + 2 * shared + low_quality)
    thr = RPN_THR if low_quality else RCNN_THR
    seen = set()
    for A in (1, 255, 256, 257):
        for K in (1, 127, 128, 129, 257):
            got = check_assign(dev, *assign_inputs(rng, 2, A, K, shared), low_quality=low_quality, **thr)
            seen |= set(np.sign(got).ravel().tolist())
    assert seen == {-1, 0, 1}


def test_max_iou_assign_best_boxes_past_256_workgroups(dev):
    """A = 70 000 (274 workgroups), K = 3, B = 2: in image 0 every gt's unique best box lies in a workgroup >= 256, which
    assign_gtmax_kernel reaches only in the second trip of its strided loop; its IoU (0.68) is below pos_iou_thr, so the
    low-quality match alone assigns it.  Image 1 holds the same best boxes and an exact duplicate of each below index 65 536:
    both copies are matched.  Then the same boxes shared by two images of which the second has gt 0's best box invalid."""
    rng = np.random.RandomState(50)
    B, A, K = 2, 70000, 3
    boxes = rand_boxes(rng, (B, A), span=600., lo=2., hi=100.)
    gts = np.array([[[40., 60., 190., 210.], [300., 100., 450., 250.], [150., 350., 300., 500.]],
                    [[80., 300., 230., 450.], [350., 350., 500., 500.], [200., 50., 350., 200.]]], np.float32)
    best = gts.copy()
    best[..., 2] = best[..., 0] + np.float32(0.68 * 150)                     # the gt's left 68 %: IoU 0.68
    far = np.array([66000, 67777, 69999])
    near = np.array([5, 30000, 65535])
    for b in range(B):
        boxes[b, far] = best[b]
    boxes[1, near] = best[1]
    box_valid, gt_valid = rng.rand(B, A) > 0.05, np.ones((B, K), bool)
    box_valid[:, far], box_valid[1, near] = True, True
    for b in range(B):                                                        # CPU-side: the path is entered
        iou = np.where(box_valid[b][None], R.iou_f32(gts[b], boxes[b]), np.float32(-1))
        top = iou.max(1)
        assert (top < 0.7).all() and (top > 0.6).all()
        for k in range(K):
            at = np.flatnonzero(iou[k] == top[k])
            assert at.tolist() == ([far[k]] if b == 0 else [near[k], far[k]]) and far[k] // 256 >= 256
    for low_quality in (True, False):
        got = check_assign(dev, boxes, box_valid, gts, gt_valid, low_quality=low_quality, **RPN_THR)
        if low_quality:
            assert got[0, far].tolist() == [1, 2, 3] and got[1, far].tolist() == [1, 2, 3] and got[1, near].tolist() == [1, 2, 3]
        else:
            assert (got[:, far] == -1).all()
    valid2 = np.stack([box_valid[0], box_valid[0]])
    valid2[1, far[0]] = False
    got = check_assign(dev, boxes[0], valid2, np.stack([gts[0], gts[0]]), gt_valid, low_quality=True, **RPN_THR)
    assert got[0, far[0]] == 1 and got[1, far[0]] == -1


@pytest.mark.parametrize('low_quality', [True, False])
def test_max_iou_assign_invalid_workgroups_and_images(dev, low_quality):
    """A workgroup whose 256 boxes are all invalid (its per-gt maxima must not win), an image with every box invalid, an image
    without gt, and padded gts in front of the real ones."""
    rng = np.random.RandomState(60)
    B, A, K = 4, 1000, 6
    boxes, box_valid, gts, gt_valid = assign_inputs(rng, B, A, K, False)
    box_valid[0, 256:512] = False
    boxes[0, 300] = gts[0, 2]                             # the best box of gt 2 would sit in the invalid workgroup
    box_valid[1] = False
    gt_valid[1] = True
    gt_valid[2] = False
    gts[2] = 0
    gt_valid[3, :3] = False                               # padding first
    gts[3, :3] = 0
    box_valid[3, :K] = True
    thr = RPN_THR if low_quality else RCNN_THR
    got = check_assign(dev, boxes, box_valid, gts, gt_valid, low_quality=low_quality, **thr)
    assert (got[1] == -1).all() and (got[2][box_valid[2]] == 0).all() and (got[0, 256:512] == -1).all()
    assert got[3].max() > 3 and not np.isin(got[3], (1, 2, 3)).any()


def test_max_iou_assign_min_pos_iou_zero_and_a_far_gt(dev):
    """min_pos_iou = 0 with a gt that overlaps nothing: its best IoU is 0, EVERY valid box has IoU 0 with it, and the
    reference's loop (max_iou_assigner.py:193-197) hands all of them to it; gts after it take their own best boxes back."""
    rng = np.random.RandomState(70)
    B, A, K = 2, 700, 4
    boxes, box_valid, gts, gt_valid = assign_inputs(rng, B, A, K, True)
    gts[:, 2] = [5000., 5000., 5040., 5030.]
    got = check_assign(dev, boxes, box_valid, gts, gt_valid, pos=0.5, neg=0.4, min_pos=0.0, low_quality=True)
    assert set(np.unique(got[0]).tolist()) == {-1, 3, 4}                    # invalid boxes, the far gt, the last gt's best box
    assert got[1].max() == 2 and (got[1] == 0).any()                        # gt 2 (the far one) and 3 of image 1 are padding
    far_last = gts.copy()
    far_last[0, [2, 3]] = far_last[0, [3, 2]]
    got = check_assign(dev, boxes, box_valid, far_last, gt_valid, pos=0.5, neg=0.4, min_pos=0.0, low_quality=True)
    assert set(np.unique(got[0]).tolist()) == {-1, 4}


def test_max_iou_assign_rejections(dev):
    from htd_amd import capi
    B, A, K = 1, 10, 2
    boxes, gts = torch.rand(A, 4, device=dev), torch.rand(B, K, 4, device=dev)
    bv, gv = torch.ones(B, A, dtype=torch.uint8, device=dev), torch.ones(B, K, dtype=torch.uint8, device=dev)
    assigned = torch.full((B, A), -7, dtype=torch.int64, device=dev)
    ov = torch.full((B, A), NAN, device=dev)
    ws = torch.zeros(capi.lib().htd_max_iou_assign_workspace_bytes(B, A, K), dtype=torch.uint8, device=dev)
    for k, low, w in ((0, 0, ws), (0, 1, ws), (K, 1, None)):       # K = 0; match_low_quality without a workspace
        with pytest.raises(ValueError):
            capi.call('htd_max_iou_assign', capi.ptr(boxes), 1, capi.ptr(bv), capi.ptr(gts), capi.ptr(gv), B, A, k, 0.7, 0.3, 0.3, low,
                      capi.ptr(assigned), capi.ptr(ov), capi.ptr(w), capi.current_stream_ptr())
        torch.cuda.synchronize()
        assert bool((assigned == -7).all()) and bool(torch.isnan(ov).all())
    capi.call('htd_max_iou_assign', capi.ptr(boxes), 1, capi.ptr(bv), capi.ptr(gts), capi.ptr(gv), B, A, K, 0.7, 0.3, 0.3, 0,
              capi.ptr(assigned), capi.ptr(ov), None, capi.current_stream_ptr())       # no workspace needed without it
    torch.cuda.synchronize()
    assert bool((assigned >= -1).all()) and not bool(torch.isnan(ov).any())


# ====================================================================================================== fixed-slot result
@pytest.mark.parametrize('add_gt,K,P,A,S,B', [
    (1, 3, 40, 50, 50, 3),        # A > K + P: slot entries point into the padding; B S = 150
    (0, 3, 40, 47, 100, 3),       # no gt candidates; B S = 300 crosses a workgroup
    (1, 1, 30, 31, 19, 2),        # K = 1
    (0, 1, 300, 300, 257, 2),
    (1, 2, 0, 7, 7, 2),           # P = 0, props = NULL: gts and padding only
    (0, 1, 0, 4, 5, 2),           # P = 0 without gt candidates: padding only
    (1, 5, 600, 605, 512, 2),     # the RoI head's size
])
def test_static_samples_finish_against_the_reference(dev, add_gt, K, P, A, S, B):
    """htd_static_samples_finish through the C ABI: an image with counts (0, 0), an image with all S slots used, slots of
    unused rows pointing anywhere (their boxes are the candidate's times 0: -0 where it is negative), every output compared as
    bits and pre-filled with a sentinel that no result contains."""
    from htd_amd import capi
    rng = np.random.RandomState(100 * K + P + S)
    gts = rand_boxes(rng, (B, K)) - np.float32(30)                # negative coordinates
    gvalid = rng.rand(B, K) > 0.3
    gvalid[:, 0] = True
    glabels = rng.randint(0, 80, (B, K)).astype(np.int64)
    props = rand_boxes(rng, (B, P)) - np.float32(30)
    assigned = rng.randint(-1, K + 1, (B, A)).astype(np.int64)
    if add_gt:
        assigned[:, :K] = np.where(gvalid, np.arange(1, K + 1), -1)
    order = rng.randint(0, A, (B, S)).astype(np.int64)
    counts = np.stack([rng.randint(0, S // 2 + 1, B), rng.randint(0, S // 2 + 1, B)], 1).astype(np.int64)
    counts[0] = (0, 0)
    counts[-1] = (S // 4, S - S // 4)
    d = lambda a: T(a).to(dev)
    t_gts, t_gv, t_gl, t_as, t_or, t_cn = d(gts), d(gvalid.astype(np.uint8)), d(glabels), d(assigned), d(order), d(counts)
    t_props = d(props) if P else None
    boxes, pgb = (torch.full((B, S, 4), NAN, device=dev) for _ in range(2))
    valid, is_pos, pig = (torch.full((B, S), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3))
    pgl = torch.full((B, S), -7, dtype=torch.int64, device=dev)
    capi.call('htd_static_samples_finish', capi.ptr(t_gts), capi.ptr(t_gv), capi.ptr(t_gl), capi.ptr(t_props), capi.ptr(t_as),
              capi.ptr(t_or), capi.ptr(t_cn), B, K, P, A, S, add_gt, capi.ptr(boxes), capi.ptr(valid), capi.ptr(is_pos), capi.ptr(pgb),
              capi.ptr(pgl), capi.ptr(pig), capi.current_stream_ptr())
    torch.cuda.synchronize()
    minus_zero = 0
    for b in range(B):
        want = R.static_samples_ref(gts[b], gvalid[b], glabels[b], props[b] if P else None, assigned[b], order[b], counts[b], S, add_gt)
        got = (boxes[b], valid[b], is_pos[b], pgb[b], pgl[b], pig[b])
        for name, x, y in zip(('boxes', 'valid', 'is_pos', 'pos_gt_boxes', 'pos_gt_labels', 'pos_is_gt'), got, want):
            x = x.cpu().numpy()
            if x.dtype == np.float32:
                x, y = bits(x), bits(y)
            assert x.shape == y.shape and np.array_equal(x, y), (b, name)
        minus_zero += int((bits(want[0]) == np.int32(-2 ** 31)).sum())
    assert minus_zero > 0 or P == 0


def test_static_samples_finish_rejections(dev):
    from htd_amd import capi
    z = torch.zeros(64, dtype=torch.int64, device=dev)
    p = capi.ptr(z)
    for B, K, P, A, S, add_gt, props in ((1, 0, 2, 4, 2, 0, p), (1, 1, 2, 2, 2, 1, p), (1, 1, 2, 4, 0, 0, p), (1, 1, 2, 4, 2, 0, None)):
        with pytest.raises(ValueError):        # K = 0; A < K + P; S = 0; P > 0 without props
            capi.call('htd_static_samples_finish', p, p, p, props, p, p, p, B, K, P, A, S, add_gt, p, p, p, p, p, p,
                      capi.current_stream_ptr())
    torch.cuda.synchronize()
    assert not bool(z.any())


# ====================================================================================================== RPN head maps
LEVELS = [(13, 17), (1, 1), (7, 9), (3, 5), (2, 1), (1, 1), (5, 3), (11, 1)]       # odd sizes: level boundaries inside a workgroup


def ptr_table(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def heads_gather(dev, ys, na):
    """ys: NHWC maps (B, h, w, C) on the device -> cls (B, A), reg (B, A, 4) from htd_rpn_heads_gather, NaN-filled before."""
    from htd_amd import capi
    B, C, L = ys[0].size(0), ys[0].size(3), len(ys)
    pix = [y.size(1) * y.size(2) for y in ys]
    A = na * sum(pix)
    cls, reg = torch.full((B, A), NAN, device=dev), torch.full((B, A, 4), NAN, device=dev)
    capi.call('htd_rpn_heads_gather', ptr_table(ys), (ctypes.c_int64 * L)(*pix), L, B, C, na, capi.ptr(cls), capi.ptr(reg),
              capi.current_stream_ptr())
    return cls, reg


def heads_scatter(dev, cls, reg, shapes, na, C):
    from htd_amd import capi
    B, L = cls.size(0), len(shapes)
    pix = [h * w for h, w in shapes]
    gys = [torch.full((B, h, w, C), NAN, device=dev) for h, w in shapes]
    capi.call('htd_rpn_heads_scatter', capi.ptr(cls), capi.ptr(reg), ptr_table(gys), (ctypes.c_int64 * L)(*pix), L, B, C, na,
              capi.current_stream_ptr())
    return gys


@pytest.mark.parametrize('C', [15, 16, 20])
def test_rpn_heads_gather_and_scatter_against_the_reference(dev, C):
    """na = 3 with no, one and five padding channels; one, five and eight levels, among them levels of one pixel; one and three
    images.  gather == permute / reshape / cat of the NCHW maps; scatter into NaN-filled maps == its transpose with zeros in the
    padding channels and no NaN left; scatter(gather(y)) gives y back on the first 5 na channels."""
    na = 3
    g = torch.Generator().manual_seed(C)
    for L in (1, 5, 8):
        for B in (1, 3):
            shapes = LEVELS[:L] if L > 1 else ([(9, 31)] if B == 3 else [(1, 1)])
            ys = [torch.randn(B, h, w, C, generator=g) for h, w in shapes]
            nchw = [y.permute(0, 3, 1, 2).numpy() for y in ys]
            want_cls, want_reg = R.rpn_flatten_ref(nchw, na)
            yd = [y.to(dev) for y in ys]
            cls, reg = heads_gather(dev, yd, na)
            assert np.array_equal(bits(cls), bits(want_cls)) and np.array_equal(bits(reg), bits(want_reg)), (L, B)
            back = heads_scatter(dev, cls, reg, shapes, na, C)
            for y, z in zip(ys, back):
                z = z.cpu()
                assert torch.equal(z[..., :5 * na], y[..., :5 * na]) and not bool(z[..., 5 * na:].any()), (L, B)
                assert np.array_equal(bits(z[..., 5 * na:]), np.zeros_like(bits(z[..., 5 * na:])))
            gc, gr = torch.randn(want_cls.shape, generator=g), torch.randn(want_reg.shape, generator=g)
            want_maps = R.rpn_unflatten_ref(gc.numpy(), gr.numpy(), shapes, na, C)
            for z, w in zip(heads_scatter(dev, gc.to(dev), gr.to(dev), shapes, na, C), want_maps):
                assert np.array_equal(bits(z.permute(0, 3, 1, 2)), bits(w)), (L, B)


def test_rpn_heads_rejections(dev):
    from htd_amd import capi
    ys = [torch.zeros(1, 1, 1, 16, device=dev) for _ in range(9)]
    cls, reg = torch.full((1, 27), NAN, device=dev), torch.full((1, 27, 4), NAN, device=dev)
    pix = (ctypes.c_int64 * 9)(*([1] * 9))
    for L, C, na in ((9, 16, 3), (2, 14, 3), (2, 16, 4), (0, 16, 3)):       # nine levels; C < 5 na twice; no level
        with pytest.raises(ValueError):
            capi.call('htd_rpn_heads_gather', ptr_table(ys), pix, L, 1, C, na, capi.ptr(cls), capi.ptr(reg), capi.current_stream_ptr())
        with pytest.raises(ValueError):
            capi.call('htd_rpn_heads_scatter', capi.ptr(cls), capi.ptr(reg), ptr_table(ys), pix, L, 1, C, na, capi.current_stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(cls).all()) and bool(torch.isnan(reg).all()) and not any(bool(y.any()) for y in ys)
