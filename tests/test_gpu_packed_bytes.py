"""The bytes every packing function of rewriting_amd/hip.py returns, pinned against the 'packed' table of
tests/golden/hip_calls.json: SHA-256 of the tensor, its element count and the scale that rides on it (rw_u_inv).  Equal
device code gives equal bytes, so there is no tolerance.  A size a form does not pack is pinned by its error text.

Weights and the blur kernel come from integer arithmetic that is exact in fp32 (no generator, no libm).  Recorded at
the commit BEFORE a change to the packing code:

    python -m tests.test_gpu_packed_bytes --record
"""
import hashlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rewriting_amd import hip  # noqa: E402
from tests.test_gpu_hip_calls import _table, update_table  # noqa: E402

pytestmark = pytest.mark.gpu

CHANNELS = ((16, 16), (48, 32), (64, 16))        # (out_ch, in_ch); the last: one every form packs (F(2x2), bf16x3)
# name -> (pack function, takes the blur kernel, keyword arguments)
FORMS = {
    'pack_conv_weight mode 0': ('pack_conv_weight', False, dict(mode=0)),
    'pack_conv_weight mode 1': ('pack_conv_weight', False, dict(mode=1)),
    'pack_conv_weight_bf16x3': ('pack_conv_weight_bf16x3', False, {}),
    'pack_conv_weight_wino': ('pack_conv_weight_wino', False, {}),
    'pack_conv_weight_wino4': ('pack_conv_weight_wino4', False, {}),
    'pack_conv_weight_wino4 split': ('pack_conv_weight_wino4', False, dict(split=True)),
    'pack_conv_transpose_weight_wino': ('pack_conv_transpose_weight_wino', False, {}),
    'pack_conv_transpose_weight_wino split': ('pack_conv_transpose_weight_wino', False, dict(split=True)),
    'pack_conv_transpose_blur_weight_wino4': ('pack_conv_transpose_blur_weight_wino4', True, {}),
    'pack_conv_transpose_blur_weight_wino4 split': ('pack_conv_transpose_blur_weight_wino4', True, dict(split=True)),
    'pack_conv_weight_direct16': ('pack_conv_weight_direct16', False, {}),
    'pack_conv_transpose_blur_weight_direct16': ('pack_conv_transpose_blur_weight_direct16', True, {}),
}


def weight(out_ch, in_ch):
    """(1, out_ch, in_ch, 3, 3) multiples of 1/8 in [-1, 1], as the model stores a modulated weight."""
    o = torch.arange(out_ch).view(-1, 1, 1, 1)
    i = torch.arange(in_ch).view(1, -1, 1, 1)
    ky = torch.arange(3).view(1, 1, -1, 1)
    kx = torch.arange(3).view(1, 1, 1, -1)
    return (((7 * o + 13 * i + 3 * ky + 5 * kx) % 17 - 8).float() / 8)[None].cuda()


def blur_kernel():
    """outer([1, 3, 3, 1]) / 16: the generator's FIR times the upsampling factor 4, in sixteenths."""
    k = torch.tensor([1., 3., 3., 1.])
    return (k[:, None] * k[None, :] / 16).cuda()


def observe(form, out_ch, in_ch):
    fn, takes_k4, kwargs = FORMS[form]
    args = (weight(out_ch, in_ch),) + ((blur_kernel(),) if takes_k4 else ())
    try:
        t = getattr(hip, fn)(*args, **kwargs)
    except ValueError as e:
        return {'raises': str(e)}
    assert t.dtype == torch.float32 and t.ndim == 1 and t.is_contiguous()
    return {'sha256': hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest(), 'numel': t.numel(),
            'rw_u_inv': getattr(t, 'rw_u_inv', None)}


@pytest.mark.parametrize('channels', CHANNELS, ids=lambda c: '%dx%d' % c)
@pytest.mark.parametrize('form', sorted(FORMS))
def test_packed_bytes_are_the_recorded_ones(form, channels):
    want = _table()['packed']['%s %dx%d' % ((form,) + channels)]
    got = observe(form, *channels)
    print(form, channels, got)
    assert got == want


def test_the_table_covers_every_packing_function():
    assert {fn for fn, _, _ in FORMS.values()} == {n for n in dir(hip) if n.startswith('pack_')}
    assert set(_table()['packed']) == {'%s %dx%d' % ((form,) + c) for form in FORMS for c in CHANNELS}


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], __doc__
    update_table('packed', {'%s %dx%d' % ((form,) + c): observe(form, *c) for form in sorted(FORMS) for c in CHANNELS})
