"""CPU: the restatement of the packed weight images (tests/afrag_restatement.py) against its own brute-force loops, the library's host-side size
functions against it, and the slu_cat2 record of the ABI: its size, where the two descriptors embed it, and the refusals that need no device."""
import ctypes

import numpy as np
import pytest

import afrag_restatement as A
from semanticlidarunc_amd import _lib


@pytest.mark.parametrize("rows,k,kc,taps", [(1, 1, 32, 1), (33, 13, 32, 1), (20, 10, 16, 1), (36, 10, 16, 9), (64, 32, 32, 1), (5, 17, 16, 9)])
def test_vectorised_image_equals_the_loops(rows, k, kc, taps):
    w = np.random.default_rng(rows + k).standard_normal((rows, k, taps)).astype(np.float32)
    got, want = A.afrag_image(w, kc), A.afrag_image_loops(w, kc)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (A.afrag_floats(rows, k, kc, taps),)
    assert np.array_equal(got, want)
    assert np.count_nonzero(want) == np.count_nonzero(w)      # every weight once, zero elsewhere


def test_a_3x3_weight_is_read_as_rows_k_taps():
    w3 = np.arange(2 * 3 * 9, dtype=np.float32).reshape(2, 3, 3, 3) + 1
    img = A.afrag_image(w3, 16).reshape(1, 9, 8, 64)
    for tap in range(9):
        assert img[0, tap, 1, 1] == w3[1, 2, tap // 3, tap % 3] and img[0, tap, 0, 32] == w3[0, 1, tap // 3, tap % 3]


def test_library_sizes_are_the_restatement_s():
    lib = _lib.load()
    for co, c in A.SHUFFLE_SHAPES + [(512, 488), (24, 64)]:
        assert lib.slu_shuffle_tail_packed_floats(co, c) == A.afrag_floats(co, c, A.TAIL_KC)
    for cin, s, e1, e3 in A.FIRE_SHAPES + [(512, 64, 256, 256)]:
        want = A.afrag_floats(s, cin, A.FIRE_SQUEEZE_KC) + A.afrag_floats(e1, s, A.FIRE_EXPAND_KC) + A.afrag_floats(e3, s, A.FIRE_EXPAND_KC, 9)
        assert lib.slu_fire_packed_floats(cin, s, e1, e3) == want


def test_cat2_record_and_where_the_descriptors_embed_it():
    """include/slu.h: two pointers and five int32, padded to 40 bytes, the first member of both descriptors."""
    assert _lib.ABI_VERSION >= 44
    assert ctypes.sizeof(_lib.Cat2) == 40
    assert [(n, getattr(_lib.Cat2, n).offset) for n, _ in _lib.Cat2._fields_] == [("src0", 0), ("src1", 8), ("ct0", 16), ("coff0", 20), ("c0", 24),
                                                                                  ("ct1", 28), ("c1", 32)]
    for desc, first_int, first_ptr, size in ((_lib.ShuffleTailDesc, "N", "wdw", 120), (_lib.FireDesc, "N", "wpack", 112)):
        assert desc.in_.offset == 0 and getattr(desc, first_int).offset == 40 and getattr(desc, first_ptr).offset == 72
        assert ctypes.sizeof(desc) == size
        d = desc()
        d.src0, d.ct0, d.coff0, d.c0, d.src1, d.ct1, d.c1 = 4096, 7, 1, 5, 8192, 3, 2      # the anonymous member's fields, by their own names
        assert (d.in_.src0, d.in_.ct0, d.in_.coff0, d.in_.c0, d.in_.src1, d.in_.ct1, d.in_.c1) == (4096, 7, 1, 5, 8192, 3, 2)


def test_cat2_refusals_come_before_any_device_call():
    lib = _lib.load()
    y = 4096      # never dereferenced: every call below is refused on the host
    for fn in (lib.slu_maxpool3s2_ceil_fwd, lib.slu_regnet_sample2):
        assert fn(None, y, 1, 4, 8, None) == -1
        for cat in (_lib.Cat2(None, None, 4, 0, 4, 0, 0),            # no source
                    _lib.Cat2(8192, None, 4, 1, 4, 0, 0),            # range past the tensor
                    _lib.Cat2(8192, None, 4, -1, 2, 0, 0),
                    _lib.Cat2(8192, None, 4, 0, 0, 0, 0),            # no channel
                    _lib.Cat2(8192, None, 4, 0, 4, 0, 1),            # channels of a missing second source
                    _lib.Cat2(8192, 16384, 4, 0, 4, 2, 3),           # more than the second source holds
                    _lib.Cat2(8192, 16384, 4, 0, 4, 2, 0)):          # a second source with no channel
            assert fn(ctypes.byref(cat), y, 1, 4, 8, None) == -1
        assert fn(ctypes.byref(_lib.Cat2(8192, None, 4, 0, 4, 0, 0)), None, 1, 4, 8, None) == -1
        assert fn(ctypes.byref(_lib.Cat2(8192, None, 4, 0, 4, 0, 0)), y, 0, 4, 8, None) == -1
    assert lib.slu_maxpool3s2_ceil_fwd(ctypes.byref(_lib.Cat2(8192, None, 4, 0, 4, 0, 0)), y, 1, 2, 8, None) == -1      # H = 2
