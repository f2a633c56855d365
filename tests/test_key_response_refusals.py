"""What rw_key_response_f32 REFUSES (include/rewriting_hip.h): every case returns RW_ERR_BAD_ARGUMENT before anything
is launched, so the placeholder pointers are never dereferenced.  As in tests/test_abi_refusals.py the calls are
skipped where a HIP device is visible -- a refusal that regressed must not turn into a launch on placeholder
pointers."""
import pytest

from rewriting_amd import _lib

BAD_ARGUMENT = 10001
P = 0x10000            # a placeholder for a device pointer: non-null, never dereferenced
GOOD = dict(a=P, keys=P, heat=P, peak=P, images=2, channels=512, hw=1024, n_keys=3, stream=None)
ORDER = ['a', 'keys', 'heat', 'peak', 'images', 'channels', 'hw', 'n_keys', 'stream']

CASES = {
    'null_a': dict(a=None),
    'null_keys': dict(keys=None),
    'null_heat': dict(heat=None),
    'no_images': dict(images=0),
    'negative_images': dict(images=-1),
    'no_channels': dict(channels=0),
    'no_pixels': dict(hw=0),
    'no_keys': dict(n_keys=0),
    'nine_keys': dict(n_keys=9),
    'map_of_an_image_past_31_bits': dict(channels=512, hw=1 << 22),          # C * hw = 2^31
    'heat_of_an_image_past_31_bits': dict(channels=1, hw=1 << 28, n_keys=8),     # K * hw = 2^31, C * hw is not
    'null_a_and_null_peak': dict(a=None, peak=None),
}


def _device_visible():
    import torch
    return torch.cuda.is_available()


def test_the_limit_of_the_header_is_the_limit_of_the_wrapper():
    import os
    import re
    from rewriting_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'rewriting_hip.h')).read()
    assert int(re.search(r'#define RW_KEY_RESPONSE_MAX_KEYS (\d+)', text).group(1)) == hip.KEY_RESPONSE_MAX_KEYS == 8
    assert _lib.ABI_VERSION == 11 and 'rw_key_response_f32' in _lib.SIGNATURES


@pytest.mark.parametrize('case', sorted(CASES))
def test_key_response_refuses(case):
    if _device_visible():
        pytest.skip('a HIP device is visible: a regressed refusal would launch on placeholder pointers')
    args = dict(GOOD, **CASES[case])
    status = int(_lib.load().rw_key_response_f32(*[args[n] for n in ORDER]))
    assert status == BAD_ARGUMENT, (case, status)
