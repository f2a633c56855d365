"""rewriting_amd.resample on the host: the tables of Pillow's 8-bit bilinear resize, applied by the numpy twin of
tests/resize_checks.py, give PIL.Image.resize(size, BILINEAR)'s bytes -- array_equal, no tolerance: both are integer
arithmetic over the same fixed-point coefficients -- for every pair of lengths 1 .. 48, the large pairs of the UI
(1024 -> 256 among them) and mixed 2-D cases; the tables have the shape the kernel relies on; and what
hip.resize_bytes and rw_resize_bilinear_u8 refuse is refused before anything could be launched (no GPU here)."""
import math

import numpy as np
import pytest
import torch

from rewriting_amd import _lib, hip, resample
from tests import resize_checks as C

SMALL = range(1, 49)


def _rows(n, seed):
    """a 3-row picture (3, n, 3): noise, 0 / 255, other noise"""
    return np.concatenate([C.noise(1, n, seed), C.black_white(1, n, seed + 1), C.noise(1, n, seed + 2)])


def _check_axis(n, m):
    rows = _rows(n, seed=n)
    along_x = C.twin(rows, (m, 3))
    assert along_x.shape == (3, m, 3)
    assert np.array_equal(along_x, C.pil(rows, (m, 3))), ('x', n, m)
    cols = np.ascontiguousarray(rows.transpose(1, 0, 2))          # (n, 3, 3): the same samples down the columns
    along_y = C.twin(cols, (3, m))
    assert along_y.shape == (m, 3, 3)
    assert np.array_equal(along_y, C.pil(cols, (3, m))), ('y', n, m)
    assert np.array_equal(along_y, along_x.transpose(1, 0, 2))    # one definition for both axes


@pytest.mark.parametrize('n', SMALL)
def test_twin_is_pil_for_every_small_pair_of_lengths(n):
    for m in SMALL:
        _check_axis(n, m)


@pytest.mark.parametrize('n,m', C.LARGE_PAIRS, ids=lambda v: str(v))
def test_twin_is_pil_for_the_large_pairs(n, m):
    _check_axis(n, m)


@pytest.mark.parametrize('shape,out', C.PAIRS_2D, ids=lambda v: '%dx%d' % v)
@pytest.mark.parametrize('make', [C.noise, C.black_white], ids=['noise', 'black_white'])
def test_twin_is_pil_in_two_dimensions(shape, out, make):
    image = make(*shape)
    size = (out[1], out[0])                                       # PIL's size is (width, height)
    got = C.twin(image, size)
    assert got.shape == out + (3,) and np.array_equal(got, C.pil(image, size))


def _check_tables(n, m):
    k, bounds = resample.coefficients(n, m)
    K = 2 * math.ceil(max(1.0, n / m)) + 1
    assert k.shape == (m, K) and k.dtype == np.int32 and bounds.shape == (m, 2) and bounds.dtype == np.int32
    first, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (first >= 0).all() and (first + count <= n).all() and (count >= 1).all() and (count <= K).all()
    assert not k[np.arange(K)[None, :] >= count[:, None]].any()   # zero past count
    assert (np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)) <= count / 2).all()


def test_table_properties():
    for n in SMALL:
        for m in SMALL:
            _check_tables(n, m)
    for n, m in C.LARGE_PAIRS:
        _check_tables(n, m)
    for (h, w), (oh, ow) in C.PAIRS_2D:
        _check_tables(h, oh)
        _check_tables(w, ow)


def test_tables_are_cached_and_read_only():
    k, bounds = resample.coefficients(1024, 256)
    again = resample.coefficients(1024, 256)
    assert again[0] is k and again[1] is bounds
    with pytest.raises(ValueError):
        k[0, 0] = 1
    with pytest.raises(ValueError):
        resample.coefficients(0, 4)
    with pytest.raises(ValueError):
        resample.coefficients(4, 0)


@pytest.mark.parametrize('value', [0, 255])
def test_a_constant_picture_stays_constant(value):
    for (h, w), (oh, ow) in C.PAIRS_2D + [((64, 64), (16, 16)), ((2, 1000), (2, 7))]:
        got = C.twin(np.full((h, w, 3), value, np.uint8), (ow, oh))
        assert got.shape == (oh, ow, 3) and (got == value).all()


def test_size_is_width_then_height_as_pil_reads_it():
    image = C.noise(12, 20)
    got = C.twin(image, (7, 5))
    assert got.shape == (5, 7, 3) == C.pil(image, (7, 5)).shape
    assert np.array_equal(got, C.pil(image, (7, 5)))
    assert C.twin(image, (5, 7)).shape == (7, 5, 3)


# ---- what hip.resize_bytes refuses in Python, before the library is touched
def test_resize_bytes_refuses_before_the_library(monkeypatch):
    def touched():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(hip, 'lib', touched)
    monkeypatch.setattr(resample, 'device_coefficients', lambda *a: touched())
    good = torch.zeros(2, 4, 6, 3, dtype=torch.uint8)
    for size in [None, 5, (5,), (5, 6, 7), (0, 4), (4, 0), (-1, 4), (4.0, 4), ('4', 4), (True, 4), [4, None]]:
        with pytest.raises(RuntimeError, match='two positive integers'):
            hip.resize_bytes(good, size)
    with pytest.raises(RuntimeError, match='no CPU fallback'):                      # the wrong device
        hip.resize_bytes(good, (3, 2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):                      # even where nothing would change
        hip.resize_bytes(good, (6, 4))
    with pytest.raises(RuntimeError, match='contiguous'):                           # a view: read in place, never copied
        hip.resize_bytes(good.permute(0, 2, 1, 3), (3, 2))
    with pytest.raises(RuntimeError, match='contiguous'):
        hip.resize_bytes(good[:, :, ::2], (3, 2))
    with pytest.raises(RuntimeError):                                               # dtype (behind the device check here)
        hip.resize_bytes(good.float(), (3, 2))
    with pytest.raises(TypeError):
        hip.resize_bytes(np.zeros((2, 4, 6, 3), np.uint8), (3, 2))


# ---- what the C entry refuses: every case returns its code before anything is launched, so the placeholder pointers are
# never dereferenced.  As in tests/test_key_response_refusals.py the calls are skipped where a HIP device is visible.
BAD_ARGUMENT, UNSUPPORTED = 10001, 10002
P = 0x10000            # a placeholder for a device pointer: non-null, 4-byte aligned, never dereferenced
GOOD = dict(image=P, kx=P, bounds_x=P, ky=P, bounds_y=P, scratch=P, out=P, images=2, height=64, width=48,
            out_height=16, out_width=12, kx_width=9, ky_width=9, stream=None)
ORDER = ['image', 'kx', 'bounds_x', 'ky', 'bounds_y', 'scratch', 'out', 'images', 'height', 'width', 'out_height',
         'out_width', 'kx_width', 'ky_width', 'stream']
CASES = {
    'null_image': (dict(image=None), BAD_ARGUMENT),
    'null_out': (dict(out=None), BAD_ARGUMENT),
    'null_kx': (dict(kx=None), BAD_ARGUMENT),
    'null_bounds_x': (dict(bounds_x=None), BAD_ARGUMENT),
    'null_ky': (dict(ky=None), BAD_ARGUMENT),
    'null_bounds_y': (dict(bounds_y=None), BAD_ARGUMENT),
    'null_scratch_with_both_axes': (dict(scratch=None), BAD_ARGUMENT),
    'no_kx_width': (dict(kx_width=0), BAD_ARGUMENT),
    'no_ky_width': (dict(ky_width=0), BAD_ARGUMENT),
    'no_images': (dict(images=0), BAD_ARGUMENT),
    'negative_images': (dict(images=-1), BAD_ARGUMENT),
    'nothing_changes': (dict(out_height=64, out_width=48), BAD_ARGUMENT),
    'grid_past_31_bits': (dict(images=1 << 31), BAD_ARGUMENT),
    'no_height': (dict(height=0), UNSUPPORTED),
    'no_width': (dict(width=0), UNSUPPORTED),
    'no_out_height': (dict(out_height=0), UNSUPPORTED),
    'negative_out_width': (dict(out_width=-3), UNSUPPORTED),
    'picture_of_2_to_31_bytes': (dict(height=1 << 15, width=(1 << 16) // 3 + 1), UNSUPPORTED),
    'resized_picture_of_2_to_31_bytes': (dict(out_height=1 << 15, out_width=(1 << 16) // 3 + 1), UNSUPPORTED),
    'scratch_picture_of_2_to_31_bytes': (dict(height=1 << 20, width=4, out_height=2, out_width=1 << 10), UNSUPPORTED),
}


def test_the_entry_is_bound():
    assert 'rw_resize_bilinear_u8' in _lib.SIGNATURES and len(_lib.SIGNATURES['rw_resize_bilinear_u8'][1]) == len(ORDER)


@pytest.mark.parametrize('case', sorted(CASES))
def test_the_entry_refuses(case):
    if torch.cuda.is_available():
        pytest.skip('a HIP device is visible: a regressed refusal would launch on placeholder pointers')
    change, want = CASES[case]
    args = dict(GOOD, **change)
    status = int(_lib.load().rw_resize_bilinear_u8(*[args[n] for n in ORDER]))
    assert status == want, (case, status)
