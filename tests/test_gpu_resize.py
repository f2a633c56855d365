"""hip.resize_bytes on the device: byte-identical to PIL.Image.resize(size, BILINEAR) -- Pillow's 8-bit resampler is
integer arithmetic over the tables of rewriting_amd.resample, so there is no tolerance -- at shapes that take every path of
the two kernels (one axis or both, rows of a multiple of four bytes or not, more than one workgroup along a row and down
the rows, count 300, K = 287, up-scaling); a picture's bytes do not depend on its batch or the run; an equal size returns
the input itself; what is refused is refused before any launch; and the routes (gw.render_urls / gw.render_url /
pngwriter.as_urls with size=) decode to exactly PIL's resize of the full-size pictures.

The C entry's refusals run here on real device buffers (null pointers, counts and extents below 1, nothing to do); the
extents past 31 bits, which no small buffer could stand behind, are refused on placeholder pointers in
tests/test_resize_host.py, where no device is visible."""
import base64
import ctypes
import io

import numpy as np
import PIL.Image
import pytest
import torch

from rewriting_amd import hip, pngwriter, resample
from tests import resize_checks as C
from tests.search_checks import make_rewriter

pytestmark = pytest.mark.gpu

# (H, W) -> (OH, OW)
SHAPES = [((1, 1), (3, 2)), ((5, 9), (1, 1)), ((37, 53), (13, 29)), ((33, 65), (65, 33)),
          ((16, 16), (16, 7)),            # x only
          ((7, 16), (3, 16)),             # y only
          ((64, 64), (16, 16)),           # the app's ratio of 4
          ((64, 64), (24, 24)),
          ((300, 200), (1, 1)),           # count 300 on one axis
          ((2, 1000), (2, 7)),            # K = 287
          ((20, 20), (50, 50))]           # up-scaling


def _device(images):
    return torch.from_numpy(np.ascontiguousarray(images)).cuda()


def _batches(h, w):
    four = np.stack([C.noise(h, w, 1), np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8),
                     C.checkerboard(h, w)])
    three = np.stack([C.noise(h, w, seed) for seed in (2, 3, 4)])
    return four, three


@pytest.mark.parametrize('shape,out', SHAPES, ids=lambda v: '%dx%d' % v)
def test_resize_bytes_is_pil(shape, out):
    (h, w), (oh, ow) = shape, out
    size = (ow, oh)                                        # PIL's size is (width, height)
    for images in _batches(h, w):
        got = hip.resize_bytes(_device(images), size)
        assert got.shape == (len(images), oh, ow, 3) and got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous()
        got = got.cpu().numpy()
        for i, image in enumerate(images):
            want = C.pil(image, size)
            assert np.array_equal(got[i], want), 'picture %d: %d bytes differ' % (i, int((got[i] != want).sum()))
            assert np.array_equal(want, C.twin(image, size))


def test_alone_in_a_batch_and_twice():
    for (h, w), (oh, ow) in [((37, 53), (13, 29)), ((64, 64), (16, 16)), ((16, 16), (16, 7)), ((7, 16), (3, 16))]:
        images = _device(np.concatenate(_batches(h, w)))
        got = hip.resize_bytes(images, (ow, oh))
        assert torch.equal(hip.resize_bytes(images, (ow, oh)), got)             # the same bytes on a second run
        for i in range(len(images)):                                           # and alone: read in place, a slice
            assert torch.equal(hip.resize_bytes(images[i:i + 1], (ow, oh))[0], got[i])
        assert torch.equal(hip.resize_bytes(images[2:5], (ow, oh)), got[2:5])


def test_equal_size_returns_the_input_and_launches_nothing(monkeypatch):
    launched = []
    monkeypatch.setattr(hip.lib(), 'rw_resize_bilinear_u8', lambda *a: launched.append(a) or 0)
    images = _device(C.noise(6, 10)[None])
    assert hip.resize_bytes(images, (10, 6)) is images
    assert hip.resize_bytes(images, [10, 6]) is images
    assert launched == []
    empty = hip.resize_bytes(torch.empty(0, 6, 10, 3, dtype=torch.uint8, device='cuda'), (5, 3))
    assert empty.shape == (0, 3, 5, 3) and launched == []
    assert hip.resize_bytes(images, (6, 10)).shape == (1, 10, 6, 3) and len(launched) == 1    # (width, height)


def test_python_refusals_before_any_launch(monkeypatch):
    launched = []
    monkeypatch.setattr(hip.lib(), 'rw_resize_bilinear_u8', lambda *a: launched.append(a) or 0)
    good = _device(C.noise(4, 6)[None])
    for bad in (good.permute(0, 2, 1, 3), good[:, :, ::2], good.float(), good.cpu(), good[0], good[..., :2].contiguous(),
                torch.empty(1, 0, 6, 3, dtype=torch.uint8, device='cuda'),
                torch.empty(1, 4, 0, 3, dtype=torch.uint8, device='cuda')):
        with pytest.raises(RuntimeError):
            hip.resize_bytes(bad, (3, 2))
    for size in (None, 3, (3,), (3, 2, 1), (0, 2), (3, -2), (3.0, 2), (True, 2)):
        with pytest.raises(RuntimeError, match='two positive integers'):
            hip.resize_bytes(good, size)
    assert launched == []


def test_the_entry_refuses_without_a_launch():
    """Real buffers of the good call's sizes; out is filled with a mark that must still be there after the refusals."""
    BAD_ARGUMENT, UNSUPPORTED = 10001, 10002
    b, h, w, oh, ow = 2, 8, 12, 4, 6
    image = _device(np.stack([C.noise(h, w, 5), C.noise(h, w, 6)]))
    kx, bx = resample.device_coefficients(w, ow, image.device)
    ky, by = resample.device_coefficients(h, oh, image.device)
    scratch = torch.empty(b, h, ow, 3, dtype=torch.uint8, device='cuda')
    out = torch.full((b, oh, ow, 3), 77, dtype=torch.uint8, device='cuda')
    good = dict(image=image, kx=kx, bounds_x=bx, ky=ky, bounds_y=by, scratch=scratch, out=out, images=b, height=h,
                width=w, out_height=oh, out_width=ow, kx_width=kx.shape[1], ky_width=ky.shape[1])
    order = ['image', 'kx', 'bounds_x', 'ky', 'bounds_y', 'scratch', 'out', 'images', 'height', 'width', 'out_height',
             'out_width', 'kx_width', 'ky_width']
    cases = [(dict(image=None), BAD_ARGUMENT), (dict(out=None), BAD_ARGUMENT), (dict(kx=None), BAD_ARGUMENT),
             (dict(bounds_x=None), BAD_ARGUMENT), (dict(ky=None), BAD_ARGUMENT), (dict(bounds_y=None), BAD_ARGUMENT),
             (dict(scratch=None), BAD_ARGUMENT), (dict(kx_width=0), BAD_ARGUMENT), (dict(ky_width=-1), BAD_ARGUMENT),
             (dict(images=0), BAD_ARGUMENT), (dict(images=-2), BAD_ARGUMENT),
             (dict(out_height=h, out_width=w), BAD_ARGUMENT),
             (dict(height=0), UNSUPPORTED), (dict(width=0), UNSUPPORTED), (dict(out_height=0), UNSUPPORTED),
             (dict(out_width=-1), UNSUPPORTED)]
    for change, want in cases:
        args = dict(good, **change)
        values = [hip._p(args[n]) if n in order[:7] else args[n] for n in order]
        status = int(hip.lib().rw_resize_bilinear_u8(*values, ctypes.c_void_p(0)))
        assert status == want, (change, status)
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    # and the same buffers, unrefused, give the picture
    values = [hip._p(good[n]) if n in order[:7] else good[n] for n in order]
    assert int(hip.lib().rw_resize_bilinear_u8(*values, hip._stream())) == 0
    for i in range(b):
        assert np.array_equal(out[i].cpu().numpy(), C.pil(image[i].cpu().numpy(), (ow, oh)))


# ---- the routes
def _decode(url):
    assert url.startswith('data:image/png;base64,')
    return np.asarray(PIL.Image.open(io.BytesIO(base64.b64decode(url.split(',', 1)[1]))).convert('RGB'))


@pytest.fixture(scope='module')
def gw():
    return make_rewriter('cuda', 32, 10, 4, device_render=True)


def test_routes_resize_as_pil_does(gw):
    size = (20, 12)                                        # (width, height): not square
    key = torch.randn(gw.k_shape[1], generator=torch.Generator().manual_seed(0))
    key = key / key.norm()
    with torch.no_grad():
        zb = torch.cat([gw.get_z(n) for n in (0, 1, 2)])
        heat = gw._heat(zb, key, 0.0)
    level = float(heat.flatten().sort()[0][int(0.9 * heat.numel())])
    seeds = [0, 1, 2, 3]
    for args, kwargs in [((), {}), ((key, level), dict(border_color=[255, 255, 255], thickness=2))]:
        full = gw.render_urls(seeds, *args, **kwargs)
        small = gw.render_urls(seeds, *args, size=size, **kwargs)
        assert len(small) == len(full) == len(seeds)
        for a, b in zip(small, full):
            got = _decode(a)
            assert got.shape == (12, 20, 3) and np.array_equal(got, C.pil(_decode(b), size))
        # one picture: seed 3 is a batch of one in both calls (an image's noise row is its position in its batch of
        # three), so the URLs are the same strings; seed 0 against the picture render_image shows for it
        assert gw.render_url(seeds[3], *args, size=size, **kwargs) == small[3]
        assert gw.render_url(seeds[3], *args, **kwargs) == full[3]
        picture = np.asarray(gw.render_image(seeds[0], *args, **kwargs))
        assert np.array_equal(_decode(gw.render_url(seeds[0], *args, **kwargs)), picture)
        assert np.array_equal(_decode(gw.render_url(seeds[0], *args, size=size, **kwargs)), C.pil(picture, size))
        # size=None is the call without the keyword
        assert gw.render_urls(seeds, *args, size=None, **kwargs) == full
        assert gw.render_url(seeds[0], *args, size=None, **kwargs) == full[0]
    mask = torch.zeros(32, 32)
    mask[8:20, 4:30] = 1
    masked = gw.render_url(1, mask=mask, size=size, thickness=1)
    assert np.array_equal(_decode(masked), C.pil(_decode(gw.render_url(1, mask=mask, thickness=1)), size))
    assert gw.render_urls([], size=size) == []
    gw.device_render = False
    try:
        with pytest.raises(RuntimeError, match='device overlay route'):
            gw.render_urls([0], size=size)
        with pytest.raises(RuntimeError, match='device overlay route'):
            gw.render_url(0, size=size)
    finally:
        gw.device_render = True


def test_pngwriter_resizes_as_pil_does(gw):
    size = (12, 20)
    with torch.no_grad():
        images = gw.model(torch.cat([gw.get_z(n) for n in (0, 1, 2)])).detach().contiguous()
    full = pngwriter.as_urls(images)
    small = pngwriter.as_urls(images, size=size)
    for a, b in zip(small, full):
        got = _decode(a)
        assert got.shape == (20, 12, 3) and np.array_equal(got, C.pil(_decode(b), size))
    assert pngwriter.as_urls(images, size=None) == full
    assert pngwriter.encode(images, size=None) == pngwriter.encode(images) == hip.png_encode(hip.render_bytes(images))
    heat = torch.rand(3, 8, 8, device='cuda')
    overlay = dict(activations=heat, level=0.5, border_color=[255, 0, 0])
    for a, b in zip(pngwriter.as_urls(images, size=size, **overlay), pngwriter.as_urls(images, **overlay)):
        assert np.array_equal(_decode(a), C.pil(_decode(b), size))
