"""hip.png_encode on the device: byte-identical to tests/png_checks.py's numpy twin run with hip.png_segment_bytes() --
the format is fully specified and integer, so there is no tolerance -- at the small shapes of tests/test_png_host.py and
at the seams of the segments; an image's file does not depend on its batch or the run; what is refused is refused before
any launch; and the two user-facing routes (gw.render_urls, pngwriter.save_image_set) end in exactly the pixels of the
host route."""
import base64
import io
import os
import zlib

import numpy as np
import PIL.Image
import pytest
import torch

from rewriting_amd import hip, pngwriter
from rewriting_amd.utils import renormalize
from tests import png_checks as C
from tests.search_checks import make_rewriter

pytestmark = pytest.mark.gpu

S = 16384          # asserted below: the shapes at the seams are chosen for it


def _random(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) % 256], axis=2).astype(np.uint8)


def _smooth(h, w, seed):
    tile = C.lowpass_noise(128, seed)                      # tiled: smooth content with a seam every 128 pixels
    return np.ascontiguousarray(np.tile(tile, (-(-h // 128), -(-w // 128), 1))[:h, :w])


def _device(images):
    return torch.from_numpy(np.ascontiguousarray(images)).cuda()


def _check(images):
    """hip.png_encode of the batch against the twin, image by image; returns the files"""
    files = hip.png_encode(_device(images))
    assert len(files) == len(images) and all(type(f) is bytes for f in files)
    for image, got in zip(images, files):
        want, stream, _ = C.encode(image, hip.png_segment_bytes())
        assert got == want, 'first difference at byte %d of %d / %d' % (
            next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want))), len(got), len(want))
        assert zlib.decompress(C.idat_of(got)) == stream and np.array_equal(C.decode(got), image)
    return files


def test_segment_size():
    assert hip.png_segment_bytes() == S


@pytest.mark.parametrize('shape', [(1, 1), (1, 2), (2, 1), (3, 5), (7, 33)], ids=lambda s: '%dx%d' % s)
def test_small_shapes(shape):
    h, w = shape
    _check(np.stack([_random(h, w), np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), _ramp(h, w)]))


# H (1 + 3 W) = S - 1, S, S + 1, 2 S + 1; a row of 1 + 3 W bytes is no multiple of a thread's run of 64 in any of them
# but the second, where the one row IS the segment
@pytest.mark.parametrize('shape,length', [((3, 1820), S - 1), ((1, 5461), S), ((5, 1092), S + 1), ((99, 110), 2 * S + 1)],
                         ids=['S-1', 'S', 'S+1', '2S+1'])
def test_segment_seams(shape, length):
    h, w = shape
    assert h * (1 + 3 * w) == length
    _check(np.stack([_smooth(h, w, seed=3), _random(h, w, seed=4)]))


def test_pictures_and_code_length_limit():
    _check(C.lowpass_noise(64, seed=1)[None])
    fib = C.fibonacci_row()                                # a plain Huffman tree would be 16 deep
    files = _check(fib[None])
    assert max(C.encode(fib, S)[2]['lengths']) == 15 and np.array_equal(C.decode(files[0]), fib)


def test_batch_of_five_alone_and_twice():
    h, w = 40, 300                                         # 36 040 stream bytes: three segments, the last one short
    images = np.stack([np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), _ramp(h, w),
                       _random(h, w, seed=7), _smooth(h, w, seed=8)])
    files = _check(images)
    assert len(set(len(f) for f in files)) == 5            # five sizes of content
    assert hip.png_encode(_device(images)) == files        # the same bytes on a second run
    for i in (0, 3, 4):                                    # and alone
        assert hip.png_encode(_device(images[i:i + 1])) == [files[i]]
    # read in place: the middle of a larger batch
    big = _device(np.concatenate([_random(h, w, seed=1)[None], images]))
    assert hip.png_encode(big[2:5]) == files[1:4]


def test_refusals_before_any_launch(monkeypatch):
    launched = []
    real = hip.lib()
    for name in ('rw_png_filter_u8', 'rw_png_encode_u8', 'rw_png_compact_u8'):
        monkeypatch.setattr(real, name, lambda *a, _n=name: launched.append(_n) or 0)
    good = _device(_random(4, 6)[None])
    for bad in (good.permute(0, 2, 1, 3), good[:, :, ::2], good.float(), good.cpu(), good[0], good[..., :2].contiguous(),
                torch.empty(1, 0, 6, 3, dtype=torch.uint8, device='cuda'),
                torch.empty(1, 4, 0, 3, dtype=torch.uint8, device='cuda')):
        with pytest.raises(RuntimeError):
            hip.png_encode(bad)
    assert hip.png_encode(torch.empty(0, 4, 6, 3, dtype=torch.uint8, device='cuda')) == []
    assert launched == []


def test_render_urls_and_save_image_set(tmp_path):
    gw = make_rewriter('cuda', 32, 10, 4, device_render=True)
    key = torch.randn(gw.k_shape[1], generator=torch.Generator().manual_seed(0))
    key = key / key.norm()
    with torch.no_grad():
        zb = torch.cat([gw.get_z(n) for n in (0, 1, 2)])
        heat = gw._heat(zb, key, 0.0)
    level = float(heat.flatten().sort()[0][int(0.9 * heat.numel())])
    kwargs = dict(border_color=[255, 255, 255], thickness=2)
    urls = gw.render_urls([0, 1, 2], key, level, **kwargs)
    pictures = gw.render_image_batch([0, 1, 2], key, level, **kwargs)
    assert len(urls) == len(pictures) == 3
    shown = 0
    for url, picture in zip(urls, pictures):
        assert url.startswith('data:image/png;base64,')
        got = np.asarray(PIL.Image.open(io.BytesIO(base64.b64decode(url.split(',', 1)[1]))).convert('RGB'))
        assert got.shape == (32, 32, 3) and np.array_equal(got, np.asarray(picture))
        assert np.array_equal(np.asarray(renormalize.from_url(url, target='image')), np.asarray(picture))
        shown += int((got == 255).all(axis=2).sum())
    assert shown > 0                                       # the outline is in the pictures
    assert gw.render_urls([]) == [] and len(gw.render_urls([4, 5, 6, 7])) == 4
    gw.device_render = False
    with pytest.raises(RuntimeError, match='device overlay route'):
        gw.render_urls([0])
    gw.device_render = True

    model, seeds = gw.model, [3, 1, 4, 15, 9]
    paths = pngwriter.save_image_set(model, model, seeds, str(tmp_path / 'set'), batch=2, shard=None)
    assert [os.path.basename(p) for p in paths] == ['image_%d.png' % s for s in seeds]
    assert sorted(os.listdir(str(tmp_path / 'set'))) == sorted(os.path.basename(p) for p in paths)
    from rewriting_amd import samples
    from rewriting_amd.utils.stylegan2.models import noise_batch_period
    want = {}
    for chunk, images in samples.generate(model, model, seeds, batch=2, shard=None):
        want.update(zip(chunk, hip.render_bytes(images.contiguous()).cpu().numpy()))
    for seed, path in zip(seeds, paths):
        assert np.array_equal(np.asarray(PIL.Image.open(path).convert('RGB')), want[seed])
    # the shard of rank 1 of 2, a template of the caller's, an offset
    paths = pngwriter.save_image_set(model, model, range(5), str(tmp_path / 'half'), name_template='s{:03d}.png',
                                     shard=(1, 2), offset=100)
    assert [os.path.basename(p) for p in paths] == ['s001.png', 's003.png']
    with torch.no_grad(), noise_batch_period(1):
        z = samples.seed_latents(model, [1, 3], offset=100).cuda()
        want = hip.render_bytes(model(z).contiguous())[1].cpu().numpy()
    assert np.array_equal(np.asarray(PIL.Image.open(paths[1]).convert('RGB')), want)
    urls = pngwriter.as_urls(model(samples.seed_latents(model, [3]).cuda()).detach().contiguous())
    assert len(urls) == 1 and urls[0].startswith('data:image/png;base64,')
