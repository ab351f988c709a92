"""The kernel behind htd_fcos_grad_scale (FCOS and ATSS: maps of C, 4 and 1 channels) and htd_vfnet_grad_scale (C, 4 and 4), called
directly on hand-filled gradient maps: every kind of map is multiplied by its own factor over its own width and nothing else is
touched.  An fp32 multiply is the same operation on the CPU, so everything is compared bit for bit.

The pyramid is the smallest with a level of several rows, a level smaller than a wavefront and a level of one pixel; C = 3 takes
the 64-lane row loop once with most lanes idle, C = 80 twice; the padded maps are channel slices of wider channels_last maps
whose padding holds a sentinel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CL = torch.channels_last
B = 2
SIZES = ((3, 5), (2, 2), (1, 1))
STRIDES = (8, 16, 32)
SENTINEL = -7.25
ENTRIES = dict(htd_fcos_grad_scale=1, htd_vfnet_grad_scale=4)      # entry -> width of the third kind of map
FACTORS = [(2.0, 3.0, 5.0), (1.0, 3.0, 5.0), (2.0, 1.0, 5.0), (2.0, 3.0, 1.0)]


def _maps(width, pad, seed):
    """-> per level (the wide map on the device, the same on the CPU): values in `width` channels, the sentinel in `pad` more."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in SIZES:
        m = torch.full((B, width + pad, h, w), SENTINEL)
        m[:, :width] = torch.randn(B, width, h, w, generator=g)
        out.append((m.to(DEV).contiguous(memory_format=CL), m))
    return out


@pytest.mark.parametrize('factors', FACTORS, ids=lambda f: 'x'.join(str(int(v)) for v in f))
@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('C', [3, 80])
@pytest.mark.parametrize('entry', list(ENTRIES))
def test_each_kind_of_map_takes_its_own_factor_over_its_own_width(entry, C, padded, factors):
    from htd_amd import capi, mmcv_ops as M
    widths = (C, 4, ENTRIES[entry])
    pads = ((4 if C == 80 else 2), 4, 3) if padded else (0, 0, 0)
    kinds = [_maps(wd, pad, 10 * k + C) for k, (wd, pad) in enumerate(zip(widths, pads))]
    tables = []
    for maps, wd in zip(kinds, widths):
        table, strides, _ = M._level_tables([dev[:, :wd] for dev, _ in maps])
        assert list(strides) == [cpu.size(1) for _, cpu in maps]          # the slices are read where they lie
        tables += [table, strides]
    if entry == 'htd_fcos_grad_scale':
        levels = M._fcos_levels(SIZES, STRIDES)[:2]
    else:
        levels = (M._i64s([h * w for h, w in SIZES]), )
    scalars = [torch.tensor([f], device=DEV) for f in factors]
    capi.call(entry, *tables, *levels, len(SIZES), B, C, *[M._P(s) for s in scalars], M._S())
    torch.cuda.synchronize()
    for maps, wd, f in zip(kinds, widths, factors):
        for dev, cpu in maps:
            got = dev.cpu()
            assert torch.equal(got[:, :wd], cpu[:, :wd] * f)                 # also: a factor of 1 leaves the map as it was
            assert torch.equal(got[:, wd:], cpu[:, wd:])                      # the padding keeps its sentinel
