"""CPU: a PixelShuffle source read in place (slu_h8_src.shuffle).  The stored channel order (h8.shuffle_store_perm) plus the consumer's
record gather equals F.pixel_shuffle; the draw kernel's inverse index expression is that permutation; and a descriptor with the flag
gets, from the launch's own dispatch, the name of the same layer with a materialised shuffle -- or the launch's refusal."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from semanticlidarunc_amd import _lib, h8
from test_dispatch_names_cpu import PTR, SLU_EUNSUPPORTED, _h8_desc, _name
from test_gpu_dispatch_coverage import H8_CASES, _id


@pytest.mark.parametrize("c,h,w", [(64, 4, 6), (128, 2, 4), (256, 1, 2)])
def test_stored_order_plus_record_gather_is_pixel_shuffle(c, h, w):
    g = torch.Generator().manual_seed(c)
    t = torch.randn(2, c, h, w, generator=g)
    perm = h8.shuffle_store_perm(c)
    assert sorted(perm.tolist()) == list(range(c))
    stored = t[:, perm].reshape(2, c // 8, 8, h, w)                     # what the producer writes: [N][G][8][H][W]
    want = F.pixel_shuffle(t, 2)
    got = torch.empty_like(want)
    for y in range(2 * h):
        for x in range(2 * w):
            for go in range(c // 32):                                    # shuffled block go at (y, x) <- ONE stored record
                got[:, 8 * go:8 * go + 8, y, x] = stored[:, 4 * go + 2 * (y & 1) + (x & 1), :, y >> 1, x >> 1]
    assert torch.equal(got, want)


def test_draw_kernel_index_expression_is_the_permutation():
    for c in (32, 64, 256):
        p = torch.arange(c)
        assert torch.equal(32 * (p >> 5) + 4 * (p & 7) + ((p >> 3) & 3), h8.shuffle_store_perm(c))
    with pytest.raises(RuntimeError):
        h8.shuffle_store_perm(48)


needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libslu_hip.so not built")


def _shuffled(desc, g_stored, scale=True):
    desc.src[0].G, desc.src[0].shuffle, desc.src[0].scale = g_stored, 1, PTR if scale else None
    return desc


@needs_lib
@pytest.mark.parametrize("n,h,w", [(2, 64, 2048), (3, 48, 1000), (64, 64, 2048)])
def test_flagged_descriptor_gets_the_name_of_the_plain_layer(n, h, w):
    """The 80 -> 32 layer of UpBlock.conv1 at full resolution (test_gpu_h8.py::test_deep_ring_3x3_two_plain_sources names it): the same
    instantiation whether the 16 shuffled channels come materialised or in place, with or without multipliers."""
    opts = dict(scales=False, resid=False)
    plain = _name("slu_conv2d_h8_kernel_name", _h8_desc((3, 1, 1), (16, 64), 32, n, h, w, **opts))
    assert plain == (0, "ring3_h8_kernel<1, 1, 5, 1, 4>")
    for scale in (True, False):
        assert _name("slu_conv2d_h8_kernel_name", _shuffled(_h8_desc((3, 1, 1), (16, 64), 32, n, h, w, **opts), 8, scale)) == plain


@needs_lib
def test_what_the_in_place_forms_do_not_cover_is_refused():
    fam, parts = (3, 1, 1), (16, 64)
    base = dict(scales=False, resid=False)
    RING, ok = "ring3_h8_kernel<1, 1, 5, 1, 4>", lambda d: _name("slu_conv2d_h8_kernel_name", d)
    assert ok(_shuffled(_h8_desc(fam, parts, 32, 2, 64, 2048, **base), 8)) == (0, RING)
    # outside the deep-ring kernel a flagged source is read in place by the SCALED tiled kernels, i.e. only when some source carries multipliers
    for n, h, w in ((1, 16, 64), (300, 64, 2048)):               # too few tiles for ring3 / its [N][64] table does not fit in LDS
        rc, name = ok(_shuffled(_h8_desc(fam, parts, 32, n, h, w, **base), 8))
        assert rc == 0 and name.startswith("conv_h8_kernel<3, 1, 1,") and ", true, " in name, name
    assert ok(_shuffled(_h8_desc(fam, parts, 32, 1, 16, 64, **base), 8, scale=False))[0] == SLU_EUNSUPPORTED
    assert ok(_shuffled(_h8_desc(fam, parts, 32, 300, 64, 2048, **base), 8, scale=False)) == (0, RING)   # no table, no limit
    # more than one shuffled K-step also adds up to 80 -> 32, but ring3 multiplies K-step 0 only: never ring3
    for stored, skip in ((128, 48), (192, 32), (256, 16)):
        rc, name = ok(_shuffled(_h8_desc(fam, (stored // 4, skip), 32, 2, 64, 2048, **base), stored // 8, True))
        assert rc == 0 and name.startswith("conv_h8_kernel<3, 1, 1,"), (stored, name)
        assert ok(_shuffled(_h8_desc(fam, (stored // 4, skip), 32, 2, 64, 2048, **base), stored // 8, False))[0] == SLU_EUNSUPPORTED
    d = _shuffled(_h8_desc(fam, parts, 32, 2, 64, 2048, **base), 8)
    d.src[1].scale = PTR                                            # multipliers on the skip: the tiled kernel, not ring3
    assert ok(d)[0] == 0 and ok(d)[1].startswith("conv_h8_kernel<3, 1, 1,")
    assert ok(_shuffled(_h8_desc((1, 1, 0), parts, 32, 2, 64, 2048, **base), 8))[0] == SLU_EUNSUPPORTED   # never a 1x1 kernel
    assert ok(_shuffled(_h8_desc((3, 2, 2), parts, 32, 2, 64, 2048, **base), 8))[0] == SLU_EUNSUPPORTED   # nor a dilated one
    # one multiplier record per STORED block of source 0 plus one per block of the others: 64 records
    assert ok(_shuffled(_h8_desc(fam, (64, 256), 128, 8, 8, 256, **base), 32))[0] == 0                    # 32 + 32
    assert ok(_shuffled(_h8_desc(fam, (64, 264), 128, 8, 8, 256, **base), 32))[0] == SLU_EUNSUPPORTED     # 32 + 33
    for bad in (dict(G=4), dict(H=63), dict(W=2047)):                                                    # partial group of 64 / odd sizes
        d = _shuffled(_h8_desc(fam, parts, 32, 2, 64, 2048, **base), 8)
        if "G" in bad:
            d.src[0].G = bad["G"]
        else:
            setattr(d, *next(iter(bad.items())))
        assert ok(d)[0] == -1
    assert h8.conv_shuffle_in_place_kernel(2, 64, 2048, 64, 64, 32, 3, 1, 1, True) == RING
    assert h8.conv_shuffle_in_place_supported(2, 32, 1024, 128, 128, 64, 3, 1, 1, True, True)
    assert not h8.conv_shuffle_in_place_supported(2, 32, 1024, 128, 128, 64, 3, 1, 1, False, False)
    assert not h8.conv_shuffle_in_place_supported(2, 32, 1024, 96, 128, 64, 3, 1, 1, True, True)         # not whole groups of 64


SCALED_ROWS = [r for r in H8_CASES if r[7].get("scales") and tuple(r[1]) == (3, 1, 1) and len(r[2]) == 2 and r[2][0] % 16 == 0 and r[5] % 2 == 0 and r[6] % 2 == 0]
assert len({r[0] for r in SCALED_ROWS}) >= 4, "the SCALED 3x3 rows left the coverage table"


@needs_lib
@pytest.mark.parametrize("case", SCALED_ROWS, ids=_id)
def test_flagged_descriptor_gets_the_name_of_its_scaled_table_row(case):
    """UpBlock.conv1 of upBlock1-3: the layer of every SCALED 3x3 table row, with its first source flagged (4x the stored channels at half
    the size), selects the instantiation the row names -- the fold adds no instantiation and moves no layer to another one."""
    name, fam, parts, cout, n, h, w, opts = case
    assert _name("slu_conv2d_h8_kernel_name", _h8_desc(fam, parts, cout, n, h, w, **opts)) == (0, name)
    d = _shuffled(_h8_desc(fam, parts, cout, n, h, w, **opts), 4 * parts[0] // 8)
    g_in = sum((c + 7) // 8 for c in parts)
    want = (0, name) if 3 * parts[0] // 8 + g_in <= 64 else (SLU_EUNSUPPORTED, "")
    assert _name("slu_conv2d_h8_kernel_name", d) == want
