"""The PGraph kernels of csrc/pgraph.hip (htd_pgraph_adjacency, htd_pgraph_softmax_fwd, htd_pgraph_softmax_bwd) and the batched
NT products around them (htd_bgemm_nt, htd_bgemm_nt_counts, BatchedGemmNT.backward), each through the C ABI against its float64
reference in tests/pgraph_ref.py (pinned on the CPU by tests/test_pgraph_ref.py).  Every output buffer goes in filled with NaN,
so anything a kernel does not write shows; every padding slot of an input the kernels have no reason to read holds NaN too.

Two kinds of check, as in tests/test_gpu_glue_ops.py, so that no tolerance is tuned on the kernel.
EXACT: integer-valued operands in [-4, 4] (one bf16 piece each, sums <= 256 * 16 * 2 far below 2^24): the device result must
torch.equal the float64 one cast to fp32, whatever the tile, the slice length or the order of summation.
FLOAT: e = max |out - ref64| / max |ref64| <= F x max(e_cpu, 2^-23), F = max(8, sqrt(R)), e_cpu the same reference function in
fp32 on the CPU, R the longest run of terms one thread adds sequentially, counted from the kernels:
  pgraph_degree_kernel / pgraph_adjacency_kernel   no floating-point sum at all (the degree is a popcount of ballots, an entry is one
      product of two correctly rounded 1 / sqrt): R = 1
  pgraph_softmax_fwd_kernel   a lane adds its SM_MAX = 16 register slots one after the other, then six shuffle steps: R = 16
  pgraph_softmax_bwd_kernel   the same for the row's dot product: R = 16
so F = 8 everywhere.  Every float check prints e, e_cpu, R, the bound and their ratio before it asserts.

Which case reaches which loop (one launch holds the six groups of a line):
  npad   counts                      what they reach
  64     0, 1, 2, 33, 63, 64         degree loop: one 64-column pass, a partial one (33, 63) and a full one; softmax: register slot 0 only
  128    0, 1, 63, 64, 65, 128       degree loop's SECOND pass from count 65 on (one live lane at 65); softmax slots 0 and 1
  1024   0, 1, 65, 640, 1023, 1024   sixteen degree passes; ALL 16 softmax register slots (640 = ten full slots, 1023 = the last lane
                                     of the last slot dead, 1024 = none)
  count 0 and rows >= count          the padded-row early exit of both softmax kernels (zero rows), `vi` false in the adjacency
Boxes have coordinates on multiples of 1/4 in [0, 512): every product is exact in fp32, `inter > 0` is the same predicate in fp32 and
fp64, so the mask is compared exactly.  Each group with room (count >= 10) holds a duplicate pair, a nested pair, two boxes sharing
only an edge, two sharing only a corner (neither pair are neighbours), a zero-width box and a box that overlaps nothing (degree 1);
the edge, corner, zero-width and lone boxes sit in the LAST slots of the group, where the ragged lanes are.

Batched products (EXACT): PGraph's three contractions at small size with counts [0, 1, 129, 256] and [33, 128, 200, 255] (a count of
0, one inside the first tile, one past a tile edge by 1, the full size; counts that are no multiple of the K slice: 33, 200, 255,
129), operands zero beyond the count along every limited axis, which is the contract, so the expected result is a @ b^T:
  128 x 256 x 256  limit 6   feature x A_local      conv_igemm_kernel<32, ...> (bk = 32)
  256 x 256 x 40   limit 3   sam x sam^T            <8, ...>  (bk = 8)
  256 x 130 x 256  limit 5   A_glob x mixed         N % 4 != 0: the scalar tail of the dead-tile zero fill, the scalar epilogue
  128 x 256 x 48   limit 6                          <16, ...> (bk = 16)
  256 x 256 x 256  limits 0..7; count 0 with limit 4 alone runs no K slice and must still write zeros
  128 x 32 x 64, 128 x 64 x 64, and 16 groups of 1024 x 256 x 32: the launcher's own rule (choose_tile) takes configuration 1
      (128x32, N <= 32), 2 (128x64, N <= 64, fewer than 2048 rows) and 3 (128x128: 256 tiles fill the chip once) for them; every other
      case here scores highest on configuration 0 (64x64).  test_bgemm_cases_reach_the_tile_configurations asserts this from
      htd_conv2d_tile_query, so the claim cannot go stale.
  htd_bgemm_nt with G = 1, M in {1, 37, 200} x N in {1, 81, 130}: ragged row and column tiles, configurations 1 and 0.
Backward through dense.bgemm_nt for the three uses (the gram case `a is b` among them): integer upstream gradient, zero beyond the
count along the limited axes of c as every PGraph caller guarantees; ga, gb must equal the float64 autograd gradient times the
operand's validity mask exactly -- this is the remapping of the limit bits in BatchedGemmNT.backward.
One FLOAT case on normal operands in both arithmetics, held to the bounds of tests/test_gpu_conv.py::
test_split_bf16_products_are_fp32_accurate (imported from there, not restated)."""
import pytest
import torch

import pgraph_ref as R

pytestmark = pytest.mark.gpu
D64 = torch.float64
NAN = float('nan')

GROUPS = {64: [0, 1, 2, 33, 63, 64], 128: [0, 1, 63, 64, 65, 128], 1024: [0, 1, 65, 640, 1023, 1024]}
IDENTICAL = {64: 3, 128: 4, 1024: 2}            # softmax: the group (of 33 / 65 / 65 boxes) whose boxes are all the same
SOFTMAX_R = 16


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return torch.device('cuda:0')


def P_(t):
    from htd_amd import capi
    return capi.ptr(t)


def call(name, *args):
    from htd_amd import capi
    capi.call(name, *args, capi.current_stream_ptr())


def nan_like(shape, dev):
    return torch.full(shape, NAN, device=dev, dtype=torch.float32)


def quarter_boxes(gen, n):
    """n boxes on the 1/4 grid inside [0, 380): sides 2 .. 40"""
    c = torch.randint(4 * 20, 4 * 360, (n, 2), generator=gen).to(D64) / 4
    half = torch.randint(4, 4 * 20 + 1, (n, 2), generator=gen).to(D64) / 4
    return torch.cat([c - half, c + half], 1)


@pytest.fixture(scope='module')
def groups():
    """npad -> (boxes (6, npad, 4) float64 with NaN padding, counts); computed once, never modified"""
    out = {}
    for npad, counts in GROUPS.items():
        gen = torch.Generator().manual_seed(npad)
        boxes = torch.full((len(counts), npad, 4), NAN, dtype=D64)
        for g, c in enumerate(counts):
            b = quarter_boxes(gen, c)
            if c >= 2:
                b[1] = b[0]                                                          # duplicate pair
            if c >= 10:
                b[3] = b[2] + torch.tensor([0.5, 0.5, -0.5, -0.5], dtype=D64)        # nested pair
                b[c - 6] = torch.tensor([400., 400., 410., 410.], dtype=D64)         # these two share only an edge
                b[c - 5] = torch.tensor([410., 400., 420.25, 410.], dtype=D64)
                b[c - 4] = torch.tensor([430., 400., 440., 410.], dtype=D64)         # these two only a corner
                b[c - 3] = torch.tensor([440., 410., 450., 420.5], dtype=D64)
                b[c - 2] = torch.tensor([460., 400., 460., 410.], dtype=D64)         # zero width
                b[c - 1] = torch.tensor([480., 480., 500., 511.75], dtype=D64)       # overlaps nothing
            boxes[g, :c] = b
        out[npad] = (boxes, counts)
    return out


def pad_mask(counts, npad):
    v = R.below(counts, npad)
    return ~(v[:, :, None] & v[:, None, :])


# ------------------------------------------------------------------------------------------------ A. adjacency, softmax
@pytest.mark.parametrize('npad', [64, 128, 1024])
def test_adjacency(dev, groups, npad):
    boxes, counts = groups[npad]
    G = len(counts)
    ref = R.local_adjacency(boxes, counts)
    mask = R.local_mask(boxes, counts)
    for g, c in enumerate(counts):                      # the fixture holds what the docstring says
        if c >= 10:
            assert not mask[g, c - 6, c - 5] and not mask[g, c - 4, c - 3] and bool(mask[g, 0, 1]) and bool(mask[g, 2, 3])
            assert int(mask[g, c - 2].sum()) == 1 and int(mask[g, c - 1].sum()) == 1
    A, dinv = nan_like((G, npad, npad), dev), nan_like((G, npad), dev)
    bx, cnt = boxes.float().to(dev), torch.tensor(counts, device=dev)
    call('htd_pgraph_adjacency', P_(bx), P_(cnt), P_(A), P_(dinv), G, npad)
    A = A.cpu()
    assert torch.isfinite(A).all(), 'entries the kernel did not write'
    assert torch.equal(A > 0, mask)
    assert torch.equal(A, A.transpose(1, 2))
    assert float(A[pad_mask(counts, npad)].abs().sum()) == 0.0
    R.check_float(f'adjacency npad={npad}', A, ref, R.local_adjacency(boxes.float(), counts), 1)


def softmax_inputs(groups, npad, scale):
    """-> boxes, counts, A_local (float64), sim (float32 values held in float64, NaN in the padding), the big-logit position"""
    boxes, counts = groups[npad]
    boxes = boxes.clone()
    g0 = IDENTICAL[npad]
    boxes[g0, :counts[g0]] = boxes[g0, 4]               # every pair of this group is local: uniform rows
    A_local = R.local_adjacency(boxes, counts)
    gen = torch.Generator().manual_seed(npad + int(scale * 10))
    sim = (torch.randn(len(counts), npad, npad, generator=gen) * scale).to(D64)
    g1 = len(counts) - 1                                # the full group: one row with a single logit of 1e4 on a non-local pair
    i = counts[g1] // 2
    j = int((A_local[g1, i, :counts[g1]] == 0).nonzero()[-1])
    sim[g1, i, j] = 1e4
    sim[pad_mask(counts, npad)] = NAN
    return boxes, counts, A_local, sim, (g1, i, j)


@pytest.mark.parametrize('scale', [0.1, 30.])
@pytest.mark.parametrize('npad', [64, 128, 1024])
def test_softmax_forward(dev, groups, npad, scale):
    boxes, counts, A_local, sim, (g1, i, j) = softmax_inputs(groups, npad, scale)
    G = len(counts)
    ref = R.global_softmax(sim, A_local, counts)
    out = nan_like((G, npad, npad), dev)
    sd, Ad, cnt = sim.float().to(dev), A_local.float().to(dev), torch.tensor(counts, device=dev)
    call('htd_pgraph_softmax_fwd', P_(sd), P_(Ad), P_(cnt), P_(out), G, npad)
    out = out.cpu()
    assert torch.isfinite(out).all(), 'entries the kernel did not write'
    assert float(out[pad_mask(counts, npad)].abs().sum()) == 0.0
    g0, c0 = IDENTICAL[npad], counts[IDENTICAL[npad]]
    # all logits 0: exp(0) = 1, the sum is the integer c0, every entry the one rounding of 1 / c0
    assert torch.equal(out[g0, :c0, :c0], torch.full((c0, c0), 1.0, dtype=torch.float32) / torch.tensor(float(c0)))
    onehot = torch.zeros(counts[g1])
    onehot[j] = 1.0
    assert torch.equal(out[g1, i, :counts[g1]], onehot)
    R.check_float(f'softmax_fwd npad={npad} scale={scale}', out, ref, R.global_softmax(sim.float(), A_local.float(), counts), SOFTMAX_R)


def softmax_grads(sim, A_local, counts, gA, dtype):
    s = sim.detach().to(dtype).clone().requires_grad_()          # a copy: .to() of the same dtype returns sim itself
    A = R.global_softmax(s, A_local.to(dtype), counts)
    return torch.autograd.grad(A, s, torch.nan_to_num(gA).to(dtype))[0], A.detach()


@pytest.mark.parametrize('scale', [0.1, 30.])
@pytest.mark.parametrize('npad', [64, 128, 1024])
def test_softmax_backward(dev, groups, npad, scale):
    boxes, counts, A_local, sim, _ = softmax_inputs(groups, npad, scale)
    G = len(counts)
    pad = pad_mask(counts, npad)
    gen = torch.Generator().manual_seed(7 * npad)
    gA = torch.randn(G, npad, npad, generator=gen).to(D64)
    gA[pad] = NAN
    ref, A_glob = softmax_grads(sim, A_local, counts, gA, D64)
    cpu32, _ = softmax_grads(sim, A_local, counts, gA, torch.float32)
    out = nan_like((G, npad, npad), dev)
    cnt = torch.tensor(counts, device=dev)
    gd, Ad, Ld = gA.float().to(dev), A_glob.float().to(dev), A_local.float().to(dev)
    call('htd_pgraph_softmax_bwd', P_(gd), P_(Ad), P_(Ld), P_(cnt), P_(out), G, npad)
    out = out.cpu()
    assert torch.isfinite(out).all(), 'entries the kernel did not write'
    assert float(out[pad | (A_local > 0)].abs().sum()) == 0.0           # local pairs and the padding: exact zeros
    R.check_float(f'softmax_bwd npad={npad} scale={scale}', out, ref, cpu32, SOFTMAX_R)

    if scale == 0.1:        # the wrapper, forward and backward, with an upstream gradient that is not contiguous
        from htd_amd.detector.pgraph import _GlobalSoftmax
        sd = sim.detach().float().to(dev).requires_grad_()
        A = _GlobalSoftmax.apply(sd, Ld, cnt)
        up = gd.transpose(1, 2)
        assert not up.is_contiguous()
        A.backward(up)
        ref_t, _ = softmax_grads(sim, A_local, counts, gA.transpose(1, 2), D64)
        cpu_t, _ = softmax_grads(sim, A_local, counts, gA.transpose(1, 2), torch.float32)
        got = sd.grad.cpu()
        assert float(got[pad | (A_local > 0)].abs().sum()) == 0.0
        R.check_float(f'_GlobalSoftmax npad={npad}', got, ref_t, cpu_t, SOFTMAX_R)


def test_pgraph_kernels_reject_bad_sizes_and_null_pointers(dev):
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    f = [torch.zeros(2 * 64 * 64, device=dev) for _ in range(4)]
    entries = {'htd_pgraph_adjacency': [f[0], cnt, f[1], f[2]], 'htd_pgraph_softmax_fwd': [f[0], f[1], cnt, f[2]],
               'htd_pgraph_softmax_bwd': [f[0], f[1], f[2], cnt, f[3]]}
    for name, tensors in entries.items():
        for G, npad in ((2, 96), (2, 1088), (0, 64)):
            with pytest.raises(ValueError, match='bad sizes'):
                call(name, *[P_(t) for t in tensors], G, npad)
        for k in range(len(tensors)):
            with pytest.raises(ValueError, match='null pointer'):
                call(name, *[None if q == k else P_(t) for q, t in enumerate(tensors)], 2, 64)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ B. batched NT products
COUNTS_A, COUNTS_B = [0, 1, 129, 256], [33, 128, 200, 255]


def int_operands(gen, G, M, N, K, counts, limit):
    """a (G, M, K), b (G, N, K) float64 with integer entries in [-4, 4], zero beyond the count along every limited axis"""
    a = torch.randint(-4, 5, (G, M, K), generator=gen).to(D64)
    b = torch.randint(-4, 5, (G, N, K), generator=gen).to(D64)
    vm, vn, vk = R.below(counts, M), R.below(counts, N), R.below(counts, K)
    if limit & 1:
        a = a * vm[:, :, None]
    if limit & 2:
        b = b * vn[:, :, None]
    if limit & 4:
        a, b = a * vk[:, None, :], b * vk[:, None, :]
    return a, b


def run_counts(dev, a, b, counts, limit):
    G, M, K = a.shape
    N = b.size(1)
    c = nan_like((G, M, N), dev)
    ad, bd, cnt = a.float().to(dev), b.float().to(dev), torch.tensor(counts, device=dev)      # named: alive until the copy back
    call('htd_bgemm_nt_counts', P_(ad), P_(bd), P_(c), G, M, N, K, P_(cnt), limit)
    return c.cpu()


PRODUCTS = [(128, 256, 256, 6), (256, 256, 40, 3), (256, 130, 256, 5), (128, 256, 48, 6), (128, 32, 64, 7), (128, 64, 64, 7)]
BIG = (16, 1024, 256, 32)                       # G, M, N, K of the case that fills the chip with 128x128 tiles
BIG_COUNTS = [0, 1, 127, 128, 129, 255, 256, 300, 511, 512, 640, 777, 896, 1000, 1023, 1024]


@pytest.mark.parametrize('counts', [COUNTS_A, COUNTS_B])
@pytest.mark.parametrize('M,N,K,limit', PRODUCTS)
def test_bgemm_counts_exact(dev, M, N, K, limit, counts):
    gen = torch.Generator().manual_seed(M + N + K + counts[0])
    a, b = int_operands(gen, 4, M, N, K, counts, limit)
    R.check_exact(f'bgemm_nt_counts {M}x{N}x{K} limit {limit}', run_counts(dev, a, b, counts, limit), R.bgemm_nt(a, b))


@pytest.mark.parametrize('counts', [COUNTS_A, COUNTS_B])
@pytest.mark.parametrize('limit', range(8))
def test_bgemm_counts_every_limit(dev, limit, counts):
    gen = torch.Generator().manual_seed(limit)
    a, b = int_operands(gen, 4, 256, 256, 256, counts, limit)
    c = run_counts(dev, a, b, counts, limit)
    R.check_exact(f'bgemm_nt_counts limit {limit}', c, R.bgemm_nt(a, b))
    if limit and counts[0] == 0:                # the empty group; under limit 4 alone no tile is dead and no K slice runs
        assert float(c[0].abs().sum()) == 0.0
    if limit == 0:
        assert float(c[0].abs().sum()) > 0.0


def test_bgemm_counts_large_tiles(dev):
    G, M, N, K = BIG
    gen = torch.Generator().manual_seed(1)
    a, b = int_operands(gen, G, M, N, K, BIG_COUNTS, 7)
    R.check_exact('bgemm_nt_counts 16 x 1024x256x32', run_counts(dev, a, b, BIG_COUNTS, 7), R.bgemm_nt(a, b))


def test_bgemm_cases_reach_the_tile_configurations():
    """What the module docstring says of the tiles, from the launcher's own rule: batched products bypass the tuned table
    (epilogue code -1) and none of these reduction lengths is split."""
    from htd_amd import capi
    q = lambda G, M, N, K: capi.lib().htd_conv2d_tile_query(G * M, N, K, 1, -1)
    got = {(M, N, K): q(4, M, N, K) for M, N, K, _ in PRODUCTS}
    assert got[(128, 32, 64)] == 1 and got[(128, 64, 64)] == 2
    assert all(got[s] == 0 for s in ((128, 256, 256), (256, 256, 40), (256, 130, 256), (128, 256, 48)))
    assert q(4, 256, 256, 256) == 0
    assert q(*BIG) == 3
    assert [q(1, M, N, 72) for M in (1, 37, 200) for N in (1, 81, 130)] == [1, 0, 0] * 3


def test_bgemm_nt_single_group_ragged_tiles(dev):
    gen = torch.Generator().manual_seed(2)
    K = 72
    for M in (1, 37, 200):
        for N in (1, 81, 130):
            a, b = int_operands(gen, 1, M, N, K, [0], 0)
            c = nan_like((1, M, N), dev)
            ad, bd = a.float().to(dev), b.float().to(dev)
            call('htd_bgemm_nt', P_(ad), P_(bd), P_(c), 1, M, N, K)
            R.check_exact(f'bgemm_nt {M}x{N}x{K}', c.cpu(), R.bgemm_nt(a, b))


# the three PGraph uses: (M, N, K, limit, gram)
USES = {'feature x A_local': (128, 256, 256, 2 | 4, False), 'sam x sam^T': (256, 256, 40, 1 | 2, True), 'A_glob x mixed': (256, 128, 256, 1 | 4, False)}


@pytest.mark.parametrize('counts', [COUNTS_A, COUNTS_B])
@pytest.mark.parametrize('use', list(USES))
def test_bgemm_backward_exact(dev, use, counts):
    from htd_amd import dense
    M, N, K, limit, gram = USES[use]
    G = 4
    gen = torch.Generator().manual_seed(M + K + counts[0])
    a, b = int_operands(gen, G, M, N, K, counts, limit)
    if gram:
        b = a
    vm, vn, vk = R.below(counts, M), R.below(counts, N), R.below(counts, K)
    one = torch.ones(G, 1, dtype=torch.bool)
    gc = torch.randint(-4, 5, (G, M, N), generator=gen).to(D64)
    gc = gc * ((vm if limit & 1 else one)[:, :, None] & (vn if limit & 2 else one)[:, None, :])
    mask_a = (vm if limit & 1 else one)[:, :, None] & (vk if limit & 4 else one)[:, None, :]
    mask_b = (vn if limit & 2 else one)[:, :, None] & (vk if limit & 4 else one)[:, None, :]
    cnt = torch.tensor(counts, device=dev)
    ad = a.float().to(dev).requires_grad_()
    a64 = a.clone().requires_grad_()
    if gram:
        c = dense.bgemm_nt(ad, ad, cnt, limit)
        c.backward(gc.float().to(dev))
        R.bgemm_nt(a64, a64).backward(gc)
        R.check_exact(use + ': c', c, R.bgemm_nt(a, a))
        R.check_exact(use + ': ga', ad.grad, a64.grad * mask_a)
        return
    bd = b.float().to(dev).requires_grad_()
    b64 = b.clone().requires_grad_()
    c = dense.bgemm_nt(ad, bd, cnt, limit)
    c.backward(gc.float().to(dev))
    R.bgemm_nt(a64, b64).backward(gc)
    R.check_exact(use + ': c', c, R.bgemm_nt(a, b))
    R.check_exact(use + ': ga', ad.grad, a64.grad * mask_a)
    R.check_exact(use + ': gb', bd.grad, b64.grad * mask_b)


def test_bgemm_counts_float_is_fp32_accurate(dev):
    """Normal operands, both arithmetics, the bounds of test_split_bf16_products_are_fp32_accurate: error / accumulated
    magnitude below 1.5e-7 sqrt(K) for either, the split form's rms within RMS_BOUND and its largest error within MAX_BOUND
    (+ 2e-8) of the fp32-input MFMA's."""
    from htd_amd import capi, dense
    from test_gpu_conv import MAX_BOUND, RMS_BOUND
    G, M, N, K, limit = 4, 256, 256, 256, 7
    gen = torch.Generator().manual_seed(11)
    vm, vn, vk = R.below(COUNTS_B, M), R.below(COUNTS_B, N), R.below(COUNTS_B, K)
    a = torch.randn(G, M, K, generator=gen).to(D64) * vm[:, :, None] * vk[:, None, :]
    b = torch.randn(G, N, K, generator=gen).to(D64) * vn[:, :, None] * vk[:, None, :]
    ref, scale = R.bgemm_nt(a, b), R.bgemm_nt(a.abs(), b.abs())
    live = scale > 0
    L = capi.lib()
    prev = L.htd_conv2d_set_math(-1)
    err = {}
    try:
        for mode in (0, 1):
            L.htd_conv2d_set_math(mode)
            c = run_counts(dev, a, b, COUNTS_B, limit).double()
            assert float(c[~live].abs().sum()) == 0.0
            e = (c - ref).abs()[live] / scale[live]
            err[mode] = (float(e.max()), float(e.pow(2).mean().sqrt()))
    finally:
        L.htd_conv2d_set_math(prev)
        dense.new_step()
    (max0, rms0), (max1, rms1) = err[0], err[1]
    print(f'bgemm_nt_counts float K={K}: native max {max0:.3e} rms {rms0:.3e}  split-bf16 max {max1:.3e} rms {rms1:.3e}  '
          f'ratio rms {rms1 / rms0:.2f} max {max1 / max0:.2f}  absolute bound {1.5e-7 * K ** 0.5:.3e}')
    assert max0 < 1.5e-7 * K ** 0.5 and max1 < 1.5e-7 * K ** 0.5, err
    assert rms1 <= RMS_BOUND * rms0, err
    assert max1 <= MAX_BOUND * max0 + 2e-8, err


def test_bgemm_rejects_bad_arguments(dev):
    a, b, c = (torch.zeros(2 * 128 * 64, device=dev) for _ in range(3))
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        call('htd_bgemm_nt', P_(a), P_(b), P_(c), 1, 16, 16, 36)                        # K % 8
    with pytest.raises(ValueError):
        call('htd_bgemm_nt_counts', P_(a), P_(b), P_(c), 1, 128, 16, 36, P_(cnt), 1)
    with pytest.raises(ValueError):
        call('htd_bgemm_nt', P_(a), P_(b), P_(c), 2, 100, 16, 16)                       # M % 128 with G > 1
    with pytest.raises(ValueError):
        call('htd_bgemm_nt_counts', P_(a), P_(b), P_(c), 2, 100, 16, 16, P_(cnt), 1)
    with pytest.raises(ValueError):
        call('htd_bgemm_nt_counts', P_(a), P_(b), P_(c), 2, 128, 16, 16, P_(cnt), 8)     # limit
    with pytest.raises(ValueError):
        call('htd_bgemm_nt_counts', P_(a), P_(b), P_(c), 2, 128, 16, 16, None, 1)        # null counts
    with pytest.raises(ValueError):
        call('htd_bgemm_nt', None, P_(b), P_(c), 1, 16, 16, 16)
    torch.cuda.synchronize()
