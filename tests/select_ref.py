"""Independent restatements of the selection operators of csrc/topk.hip (segmented top-k, RandomSampler) and csrc/box_ops.hip
(MaxIoUAssigner, the fixed-slot sampling result, the flat form of the RPN head maps): the references tests/test_gpu_select_ops.py
holds the kernels to.  Plain numpy and Python: no HIP, no C ABI and no import of the tensor formulations in htd_amd.core.bbox
that the first-generation tests compared the kernels with.  tests/test_select_ref.py pins every function from outside: to the
reference project's recorded assignments, to MaxIoUAssigner / RandomSampler on CPU tensors and to Python's own arithmetic.

Everything here is exact: indices, masks and counts are integers, and the two float outputs (max_overlaps, gathered boxes) are
the fp32 values the reference computes, so the GPU tests compare bit patterns."""
import numpy as np
import torch

F32 = np.float32


# ---------------------------------------------------------------------------------------------------- segmented top-k
def topk_ref(keys, k):
    """Positions of the k largest keys of one segment in descending order, equal keys by ascending position: the first k of
    `keys.sort(descending=True, stable=True)` (rpn_head.py:122-133).  NaN-free float32 keys go through float64 (exact, order
    preserving, -0 == +0) and numpy's stable argsort; a segment with a NaN keeps torch's stable sort on the CPU, which ranks
    every NaN first (numpy ranks them last)."""
    keys = np.asarray(keys, dtype=F32)
    if np.isnan(keys).any():
        return torch.from_numpy(keys).sort(descending=True, stable=True)[1][:k].numpy().astype(np.int64)
    return np.argsort(-keys.astype(np.float64), kind='stable')[:k].astype(np.int64)


# ---------------------------------------------------------------------------------------------------- MaxIoUAssigner
def iou_f32(gts, boxes):
    """bbox_overlaps(gts, boxes) of iou2d_calculator.py:43-158 in fp32, one operation at a time (numpy never contracts a
    multiply and an add): overlap / max(area_gt + area_box - overlap, 1e-6).  -> (K, A) float32"""
    g, b = np.asarray(gts, dtype=F32).reshape(-1, 4), np.asarray(boxes, dtype=F32).reshape(-1, 4)
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(np.minimum(g[:, None, 2], b[None, :, 2]) - np.maximum(g[:, None, 0], b[None, :, 0]), F32(0))
    h = np.maximum(np.minimum(g[:, None, 3], b[None, :, 3]) - np.maximum(g[:, None, 1], b[None, :, 1]), F32(0))
    overlap = w * h
    union = np.maximum(area_g[:, None] + area_b[None, :] - overlap, F32(1e-6))
    out = overlap / union
    assert out.dtype == F32
    return out


def max_iou_assign_ref(boxes, box_valid, gts, gt_valid, pos, neg, min_pos, low_quality):
    """MaxIoUAssigner.assign_wrt_overlaps with gt_max_assign_all (max_iou_assigner.py:124-212) for ONE image, statement by
    statement, on the image's real gts and real boxes, then written back into the padded layout under this project's
    conventions: a padded gt takes no part, an invalid box is -1 with overlap 0 and is no gt's best box, an image without gt
    has every valid box negative (0) with overlap 0.  boxes (A, 4), box_valid (A,), gts (K, 4), gt_valid (K,).
    -> assigned (A,) int64 (k + 1: gt k of the PADDED numbering), max_overlaps (A,) float32."""
    boxes, gts = np.asarray(boxes, dtype=F32), np.asarray(gts, dtype=F32)
    bi = np.flatnonzero(np.asarray(box_valid))           # the real boxes
    gi = np.flatnonzero(np.asarray(gt_valid))            # the real gts
    A = boxes.shape[0]
    assigned, max_ov = np.full(A, -1, dtype=np.int64), np.zeros(A, dtype=F32)
    num_gts, num_bboxes = len(gi), len(bi)
    if num_bboxes == 0:
        return assigned, max_ov
    if num_gts == 0:                                     # :145-161
        assigned[bi] = 0
        return assigned, max_ov
    overlaps = iou_f32(gts[gi], boxes[bi])               # (k, n)
    thr = lambda v: F32(v)                               # a Python float against a float32 tensor compares in fp32
    a = np.full(num_bboxes, -1, dtype=np.int64)          # 1. :141
    max_overlaps, argmax_overlaps = overlaps.max(axis=0), overlaps.argmax(axis=0)        # :165, first maximum
    gt_max_overlaps = overlaps.max(axis=1)               # :168
    a[(max_overlaps >= 0) & (max_overlaps < thr(neg))] = 0                               # 2. :173
    pos_inds = max_overlaps >= thr(pos)                  # 3. :181
    a[pos_inds] = argmax_overlaps[pos_inds] + 1
    if low_quality:                                      # :184-199
        for i in range(num_gts):
            if gt_max_overlaps[i] >= thr(min_pos):
                a[overlaps[i, :] == gt_max_overlaps[i]] = i + 1
    assigned[bi] = np.where(a > 0, gi[np.maximum(a - 1, 0)] + 1, a)
    max_ov[bi] = max_overlaps
    return assigned, max_ov


# ---------------------------------------------------------------------------------------------------- RandomSampler
def neg_bound(neg_pos_ub, n_pos):
    """base_sampler.py:90-92: int(neg_pos_ub * max(1, n_pos)) in Python's own (double) arithmetic."""
    return int(neg_pos_ub * max(1, n_pos))


def random_sample_ref(assigned, keys, num, pos_fraction, neg_pos_ub=-1):
    """RandomSampler.sample (base_sampler.py:82-97) for ONE image where "a random subset of size n" is the n candidates
    ranked first by (key, index).  assigned (A,) (> 0 positive, 0 negative, < 0 ignored), keys (A,) float32.
    -> (pos_inds ascending, neg_inds ascending, order = drawn positives then drawn negatives: SamplingResult.bboxes) as lists."""
    assigned, keys = np.asarray(assigned), np.asarray(keys, dtype=F32)

    def draw(cand, n):
        ranked = sorted((int(i) for i in cand), key=lambda i: (float(keys[i]), i))       # -0.0 == 0.0: the index decides
        return sorted(ranked[:max(n, 0)])
    max_pos = int(num * pos_fraction)
    pos_inds = draw(np.flatnonzero(assigned > 0), max_pos)
    num_expected_neg = num - len(pos_inds)
    if neg_pos_ub >= 0:
        num_expected_neg = min(num_expected_neg, neg_bound(neg_pos_ub, len(pos_inds)))
    neg_inds = draw(np.flatnonzero(assigned == 0), num_expected_neg)
    return pos_inds, neg_inds, pos_inds + neg_inds


# ---------------------------------------------------------------------------------------------------- fixed-slot result
def static_samples_ref(gts, gvalid, glabels, props, assigned, order, counts, S, add_gt):
    """SamplingResult (sampling_result.py:25-49) of ONE image laid out in S fixed slots.  Candidates are [gts (K, when add_gt) |
    props (P) | never-drawn padding up to A = len(assigned)] (base_sampler.py:73-80); order (S,) is the candidate of each slot,
    counts = (drawn positives, drawn negatives).  Slot s < n_pos + n_neg holds bboxes[order[s]]; every slot, used or not,
    carries the gt its candidate is assigned to (gt 0 when it has none) and that gt's label; pos_is_gt = gt_flags[order[s]] on
    the positive slots.  An unused slot's box is the candidate's box times 0.0, so a negative coordinate leaves -0.
    -> boxes (S, 4) f32, valid (S,) u8, is_pos (S,) u8, pos_gt_boxes (S, 4) f32, pos_gt_labels (S,) i64, pos_is_gt (S,) u8"""
    gts = np.asarray(gts, dtype=F32).reshape(-1, 4)
    K, A = gts.shape[0], len(assigned)
    props = np.zeros((0, 4), F32) if props is None else np.asarray(props, dtype=F32).reshape(-1, 4)
    head = [gts, props] if add_gt else [props]
    n_real = sum(len(h) for h in head)
    bboxes = np.concatenate(head + [np.zeros((A - n_real, 4), F32)])
    gt_flags = np.zeros(A, np.uint8)
    if add_gt:
        gt_flags[:K] = np.asarray(gvalid, dtype=np.uint8) != 0
    n_pos, n_neg = int(counts[0]), int(counts[1])
    boxes, pgb = np.zeros((S, 4), F32), np.zeros((S, 4), F32)
    valid, is_pos, pig = np.zeros(S, np.uint8), np.zeros(S, np.uint8), np.zeros(S, np.uint8)
    pgl = np.zeros(S, np.int64)
    for s in range(S):
        c = int(order[s])
        used = s < n_pos + n_neg
        boxes[s] = bboxes[c] * F32(1.0 if used else 0.0)
        valid[s], is_pos[s] = used, s < n_pos
        g = max(int(assigned[c]) - 1, 0)                 # pos_assigned_gt_inds, :34
        pgb[s], pgl[s] = gts[g], glabels[g]
        pig[s] = bool(gt_flags[c]) and s < n_pos
    return boxes, valid, is_pos, pgb, pgl, pig


# ---------------------------------------------------------------------------------------------------- RPN head maps
def rpn_flatten_ref(maps, na):
    """anchor_head.py:172-269 / rpn_head.py:78-168: every level's (B, na, h, w) objectness map and (B, 4 na, h, w) delta map
    go through permute(0, 2, 3, 1).reshape(B, -1[, 4]) and the levels are concatenated.  maps: per level the merged head's
    output (B, C, h, w), channels [0, na) the objectness, [na, 5 na) the deltas, the rest padding.
    -> cls (B, A), reg (B, A, 4), A = na * sum(h w)"""
    cls, reg = [], []
    for y in maps:
        y = np.asarray(y)
        B = y.shape[0]
        cls.append(y[:, :na].transpose(0, 2, 3, 1).reshape(B, -1))
        reg.append(y[:, na:5 * na].transpose(0, 2, 3, 1).reshape(B, -1, 4))
    return np.concatenate(cls, 1), np.concatenate(reg, 1)


def rpn_unflatten_ref(cls, reg, shapes, na, C):
    """The transpose of rpn_flatten_ref: the gradient maps (B, C, h, w) of every level, padding channels zero."""
    cls, reg = np.asarray(cls), np.asarray(reg)
    B, out, off = cls.shape[0], [], 0
    for h, w in shapes:
        n = h * w * na
        y = np.zeros((B, C, h, w), cls.dtype)
        y[:, :na] = cls[:, off:off + n].reshape(B, h, w, na).transpose(0, 3, 1, 2)
        y[:, na:5 * na] = reg[:, off:off + n].reshape(B, h, w, 4 * na).transpose(0, 3, 1, 2)
        out.append(y)
        off += n
    return out
