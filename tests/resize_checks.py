"""The numpy twin of hip.resize_bytes: rewriting_amd.resample.coefficients applied with plain integer numpy, one pass at
a time (along x, rounded to bytes, then along y), and Pillow itself as the yardstick of both.  Shared by
tests/test_resize_host.py and tests/test_gpu_resize.py; every comparison made with these is array_equal."""
import numpy as np
import PIL.Image

from rewriting_amd import resample

BILINEAR = getattr(PIL.Image, 'Resampling', PIL.Image).BILINEAR

# one axis, n -> m: the large pairs of the issue
LARGE_PAIRS = [(1024, 256), (1024, 300), (1024, 1), (512, 257), (255, 1024), (1000, 7)]
# (H, W) -> (OH, OW), both axes
PAIRS_2D = [((5, 9), (1, 1)), ((37, 53), (13, 29)), ((33, 65), (65, 33)), ((16, 16), (16, 7)), ((20, 20), (50, 50))]


def resize_axis(a, m, axis):
    """a (..., n, ...) uint8 resized to m along `axis` with the tables of resample.coefficients: int32 sums, an
    arithmetic shift, a clamp to bytes"""
    n = a.shape[axis]
    k, bounds = resample.coefficients(n, m)
    src = np.moveaxis(a, axis, 0).astype(np.int32)
    out = np.empty((m,) + src.shape[1:], dtype=np.uint8)
    for o in range(m):
        first, count = int(bounds[o, 0]), int(bounds[o, 1])
        acc = np.full(src.shape[1:], 1 << 21, dtype=np.int32)
        for j in range(count):
            acc += k[o, j] * src[first + j]
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def twin(image, size):
    """image (H, W, 3) uint8 -> (size[1], size[0], 3): x first, then y; an axis that keeps its length is not touched"""
    width, height = size
    if width != image.shape[1]:
        image = resize_axis(image, width, 1)
    if height != image.shape[0]:
        image = resize_axis(image, height, 0)
    return image


def pil(image, size):
    """PIL.Image.resize(size, resample=BILINEAR) of image (H, W, 3) uint8, as renormalize.as_url(size=...) does it"""
    return np.asarray(PIL.Image.fromarray(image).resize(size, resample=BILINEAR))


def noise(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def black_white(h, w, seed=0):
    """every byte 0 or 255: the sums reach both ends of the clamp"""
    return (np.random.RandomState(seed).randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def checkerboard(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
