"""What tests/test_overlay_host.py (CPU) and tests/test_gpu_overlay.py (device) share: a NumPy restatement of the picture
rw_render_bytes_f32 defines (include/rewriting_hip.h) with the up-sampling in float64, the band of pixels whose
`up > level` float32 cannot decide, the comparison that leaves exactly those out, and the two tables of inputs.

The picture: s = trunc(clamp(x * 127.5f + 127.5f, 0, 255)) (float32, two roundings); inside = mask, or up(y, x) > level
with up bilinear over the heat map's pixel centres and zeros outside it; border = not inside and some pixel within
Chebyshev distance `thickness` is inside; border pixels show border_color, inside pixels s (or inside_color), the rest
trunc(clamp(outside_bright * s, 0, 255)).  Everything but the comparison `up > level` is integer-exact."""
import functools

import numpy as np
import torch

# (h, w, H, W): random heat maps; the comparison leaves out the undecided band (at most 2 % of an image)
BAND_SHAPES = [(8, 8, 64, 64), (4, 4, 64, 64), (6, 5, 20, 37), (32, 32, 256, 256), (16, 16, 16, 16), (7, 9, 130, 202),
               (32, 32, 1024, 1024)]
BAND_SEEDS = (0, 1, 2, 3, 4)
BAND_QUANTILES = (0.5, 0.9, 0.99)
# (h, w, H, W): 0/1 heat maps at level 0.5; the band is empty and the whole picture must be equal
EXACT_SHAPES = [(16, 16, 16, 16), (16, 16, 32, 32), (8, 8, 32, 32), (8, 8, 64, 64), (5, 7, 20, 28), (6, 5, 20, 37),
                (4, 4, 64, 64)]
EXACT_LEVEL = 0.5
MAX_EXCLUDED = 0.02
YELLOW = (255, 255, 0)


def band_heat(seed, h, w):
    return torch.randn(h, w, generator=torch.Generator().manual_seed(seed))


def band_level(a, q):
    return 0.75 * a.reshape(-1).sort()[0][int(a.numel() * q)].item()


def exact_heat(seed, h, w):
    return (torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) < 0.3).float()


def image_for(seed, H, W):
    """0.8 * randn: both clamps of the byte conversion occur"""
    return 0.8 * torch.randn(3, H, W, generator=torch.Generator().manual_seed(1000 + seed))


def _np(t, dtype):
    return np.ascontiguousarray((t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype))


def _axis(n_out, n_in):
    f = (np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5
    i0 = np.floor(f)
    return i0.astype(np.int64), f - i0


def upsample64(heat, H, W):
    """(up, corner): up (H, W) float64 = the bilinear up-sampling of heat (h, w) with zeros outside the map; corner =
    the largest |heat| among the four corners a pixel reads."""
    a = _np(heat, np.float64)
    h, w = a.shape
    padded = np.zeros((h + 2, w + 2))
    padded[1:-1, 1:-1] = a
    y0, ty = _axis(H, h)
    x0, tx = _axis(W, w)
    r0, r1, c0, c1 = (y0 + 1)[:, None], (y0 + 2)[:, None], (x0 + 1)[None, :], (x0 + 2)[None, :]
    ty, tx = ty[:, None], tx[None, :]
    v00, v01, v10, v11 = padded[r0, c0], padded[r0, c1], padded[r1, c0], padded[r1, c1]
    up = (v00 * (1 - tx) + v01 * tx) * (1 - ty) + (v10 * (1 - tx) + v11 * tx) * ty
    corner = np.maximum(np.maximum(np.abs(v00), np.abs(v01)), np.maximum(np.abs(v10), np.abs(v11)))
    return up, corner


def undecided(heat, level, H, W):
    """Pixels with |up64 - level| <= tau, tau = 2^-24 (16 (max(h, w) + 1) + 8) max(A, |level|), A the largest |heat| among
    the pixel's corners: at most four roundings on coordinates of size <= max(h, w) + 1 reach the weights, twice that
    the value, and eight more come from the products and sums.  A pixel whose four corners are all zero is decided
    whatever the level: its up is a sum of exact zeros, 0 in float32 and in float64 alike (this only narrows the band:
    a box of ones on zeros at level 0.0, render_object's, would otherwise have its whole outside in it)."""
    up, corner = upsample64(heat, H, W)
    h, w = heat.shape[-2:]
    tau = 2.0 ** -24 * (16 * (max(h, w) + 1) + 8) * np.maximum(corner, abs(float(level)))
    return (np.abs(up - float(level)) <= tau) & (corner > 0)


def grow(mask, thickness):
    """Pixels within Chebyshev distance `thickness` of a set pixel; pixels beyond the edge do not count."""
    out = mask.copy()
    for axis in (0, 1):
        src = out.copy()
        for d in range(1, thickness + 1):
            lo = [slice(None)] * 2
            hi = [slice(None)] * 2
            lo[axis], hi[axis] = slice(None, -d), slice(d, None)
            if d < src.shape[axis]:
                out[tuple(hi)] |= src[tuple(lo)]
                out[tuple(lo)] |= src[tuple(hi)]
    return out


def left_out(heat, level, H, W, thickness):
    """The pixels a comparison leaves out: the undecided ones and every pixel within `thickness` of one.  It depends
    on the inputs alone, never on the code under test."""
    return grow(undecided(heat, level, H, W), thickness)


def closed_form_border(mask, thickness):
    mask = _np(mask, bool)
    return ~mask & grow(mask, thickness)


def image_bytes(image):
    """renormalize.as_image's bytes: float32 product, float32 sum, clamp, truncation; NaN -> 0"""
    x = _np(image, np.float32)
    with np.errstate(invalid='ignore'):
        v = x * np.float32(127.5)
        v = v + np.float32(127.5)
        v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(255)))
    return v.astype(np.uint8)


def _colour(c):
    return np.array([int(min(max(float(v), 0.0), 255.0)) for v in c], dtype=np.uint8)


def picture(image, inside=None, thickness=1, border_color=None, outside_bright=0.5, inside_color=None):
    """(H, W, 3) uint8 of one image (3, H, W) and its inside mask (H, W) (None: the plain bytes)"""
    s = image_bytes(image).transpose(1, 2, 0)
    if inside is None:
        return s
    inside = _np(inside, bool)
    border = closed_form_border(inside, thickness)
    dim = np.clip(np.float32(outside_bright) * s.astype(np.float32), np.float32(0), np.float32(255)).astype(np.uint8)
    out = np.where(inside[:, :, None], s if inside_color is None else _colour(inside_color)[None, None, :], dim)
    return np.where(border[:, :, None], _colour(YELLOW if border_color is None else border_color)[None, None, :],
                    out).astype(np.uint8)


def inside64(heat, level, H, W):
    return upsample64(heat, H, W)[0] > float(level)


def render(images, activations=None, mask=None, level=None, thickness=1, border_color=None, outside_bright=0.5,
           inside_color=None):
    """hip.render_bytes restated: (B, H, W, 3) uint8 as a NumPy array"""
    H, W = images.shape[-2:]
    out = []
    for b in range(images.shape[0]):
        inside = None
        if activations is not None:
            inside = inside64(activations[b], level, H, W)
        elif mask is not None:
            inside = _np(mask[b], np.uint8) != 0
        out.append(picture(images[b], inside, thickness, border_color, outside_bright, inside_color))
    return np.stack(out)


def render_bytes_stand_in(images, activations=None, mask=None, level=None, thickness=1, border_color=None,
                          outside_bright=0.5, inside_color=None):
    """A torch stand-in for hip.render_bytes made from the restatement (the routing tests on the CPU)."""
    assert images.dim() == 4 and images.shape[1] == 3 and images.is_contiguous() and images.dtype == torch.float32
    assert 0 <= thickness <= 8
    if activations is not None:
        assert level is not None and activations.is_contiguous() and activations.shape[0] == images.shape[0]
        assert min(activations.shape[1:]) >= 2
    return torch.from_numpy(render(images, activations, mask, level, thickness, border_color, outside_bright,
                                   inside_color)).to(images.device)


def host_picture(image, heat=None, level=None, mask=None, **kwargs):
    """(H, W, 3) uint8 by the yardstick, ImageVisualizer.pytorch_masked_image on the CPU"""
    from rewriting_amd.utils import imgviz
    iv = imgviz.ImageVisualizer(tuple(image.shape[-2:]))
    image = image.detach().cpu()
    if mask is not None:
        got = iv.pytorch_masked_image(image, mask=torch.as_tensor(mask).cpu().bool(), **kwargs)
    else:
        got = iv.pytorch_masked_image(image, heat.detach().cpu(), level=level, **kwargs)
    return got.permute(1, 2, 0).numpy()


def compare(got, want, heat=None, level=None, thickness=0):
    """got, want (H, W, 3) uint8.  Left out: the undecided pixels of (heat, level) and every pixel within `thickness` of
    one -- at most 2 % of the image, asserted; everywhere else the bytes must be EQUAL.  heat None: the whole picture.
    Returns the share left out."""
    got, want = _np(got, np.uint8), _np(want, np.uint8)
    assert got.shape == want.shape and got.shape[2] == 3, (got.shape, want.shape)
    if heat is None:
        assert np.array_equal(got, want), _first_difference(got, want)
        return 0.0
    H, W = got.shape[:2]
    out = left_out(heat, level, H, W, thickness)
    share = out.mean()
    assert share <= MAX_EXCLUDED, 'the comparison leaves out %.2f %% of the image' % (100 * share)
    differ = (got != want).any(axis=2) & ~out
    assert not differ.any(), _first_difference(np.where(out[:, :, None], want, got), want)
    return float(share)


def assert_empty_band(heat, level, H, W):
    assert not undecided(heat, level, H, W).any()


def _first_difference(got, want):
    y, x = np.argwhere((got != want).any(axis=2))[0]
    return '%d pixels differ; first at (%d, %d): %s, wanted %s' % ((got != want).any(axis=2).sum(), y, x,
                                                                    got[y, x].tolist(), want[y, x].tolist())


@functools.lru_cache(maxsize=None)
def band_case(seed, q, h, w):
    a = band_heat(seed, h, w)
    return a, band_level(a, q)
