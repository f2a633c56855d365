"""The coefficient tables of Pillow's 8-bit bilinear resize: what ``renormalize.as_url(img, size=...)``
(utils/renormalize.py:22-32) does with ``PIL.Image.resize(size, resample=BILINEAR)``, as numbers a kernel can apply.

Pillow's 8-bit resampler is integer arithmetic over fixed-point coefficients that the host computes in double
(``precompute_coeffs`` + ``normalize_coeffs_8bpc``; bilinear filter, support 1).  For one axis of length n resized to m:

    scale = n / m;  fs = max(scale, 1.0);  support = fs;  K = 2 * ceil(support) + 1
    for o in 0 .. m - 1:
        center = (o + 0.5) * scale
        first  = max(int(center - support + 0.5), 0)
        count  = min(int(center + support + 0.5), n) - first
        w[j]   = tri((j + first - center + 0.5) * (1.0 / fs))  for j < count;  tri(v) = 1 - |v| if |v| < 1 else 0
        w[j]  /= w[0] + w[1] + ...        (summed in this order; left alone if the sum is 0)
        k[j]   = int(0.5 + w[j] * 2^22)   (int(-0.5 + ...) for a negative w[j]);  k[j] = 0 for count <= j < K
    out[o] = clamp((2^21 + sum_j k[j] * in[first + j]) >> 22, 0, 255)          (int32, arithmetic shift)

Everything above the last line is IEEE double in this operation order, int() truncates toward zero, and it lives HERE
only: rw_resize_bilinear_u8 (hip.resize_bytes) applies the tables on the device, tests/resize_checks.py with numpy.  The
columns below are vectorised over o; the operations of one o and their order are the scalar ones.
"""
import functools
import math

import numpy

PRECISION_BITS = 32 - 8 - 2          # Pillow's: 8 bits of data, 2 of headroom for the overshoot of other filters


@functools.lru_cache(maxsize=64)
def coefficients(n, m):
    """(k (m, K) int32, bounds (m, 2) int32 = first, count) for an axis of length n resized to m; read-only arrays."""
    n, m = int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError('resample.coefficients: lengths must be positive, not %d -> %d' % (n, m))
    scale = n / m
    fs = max(scale, 1.0)
    support = fs
    K = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    center = (numpy.arange(m, dtype=numpy.float64) + 0.5) * scale
    first = numpy.maximum((center - support + 0.5).astype(numpy.int64), 0)
    count = numpy.minimum((center + support + 0.5).astype(numpy.int64), n) - first
    w = numpy.zeros((m, K), dtype=numpy.float64)
    total = numpy.zeros(m, dtype=numpy.float64)
    for j in range(K):
        v = numpy.abs((j + first - center + 0.5) * ss)
        w[:, j] = numpy.where((v < 1.0) & (j < count), 1.0 - v, 0.0)
        total = total + w[:, j]                                        # + 0.0 past count: the running sum of count terms
    w = w / numpy.where(total != 0.0, total, 1.0)[:, None]
    fixed = w * float(1 << PRECISION_BITS)
    k = numpy.where(w < 0.0, -0.5 + fixed, 0.5 + fixed).astype(numpy.int64).astype(numpy.int32)
    bounds = numpy.stack([first, count], axis=1).astype(numpy.int32)
    k.setflags(write=False)
    bounds.setflags(write=False)
    return k, bounds


_device_tables = {}


def device_coefficients(n, m, device):
    """coefficients(n, m) as two int32 tensors on `device`, copied once per (n, m, device)"""
    import torch
    device = torch.device(device)
    key = (int(n), int(m), device.type, device.index)
    tables = _device_tables.get(key)
    if tables is None:
        k, bounds = coefficients(n, m)
        tables = (torch.from_numpy(k.copy()).to(device), torch.from_numpy(bounds.copy()).to(device))
        if len(_device_tables) >= 64:
            _device_tables.clear()
        _device_tables[key] = tables
    return tables
