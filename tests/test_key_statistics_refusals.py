"""What the entries of the key statistics REFUSE (include/rewriting_hip.h), and the size of the split-K workspace.  Every
refused case returns before anything is launched, so the placeholder pointers are never dereferenced.  As in
tests/test_key_response_refusals.py the calls are skipped where a HIP device is visible -- a refusal that regressed must
not turn into a launch on placeholder pointers; the workspace size is a pure function and is checked everywhere."""
import pytest

from rewriting_amd import _lib
from tests import key_statistics_checks as K

BAD_ARGUMENT, UNSUPPORTED = 10001, 10002
P = 0x10000            # a placeholder for a device pointer: non-null, never dereferenced

MOMENT_ORDER = ['a', 'mom2', 'rows', 'channels', 'hw', 'layout', 'workspace', 'stream']
MOMENT_GOOD = dict(a=P, mom2=P, rows=2048, channels=512, hw=1024, layout=1, workspace=P, stream=None)
MOMENT_CASES = {
    'null_a': (dict(a=None), BAD_ARGUMENT),
    'null_mom2': (dict(mom2=None), BAD_ARGUMENT),
    'null_workspace': (dict(workspace=None), BAD_ARGUMENT),
    'null_a_as_rows': (dict(a=None, layout=0), BAD_ARGUMENT),
    'no_rows': (dict(rows=0), BAD_ARGUMENT),
    'negative_rows': (dict(rows=-16), BAD_ARGUMENT),
    'no_rows_as_rows': (dict(rows=0, layout=0, hw=0), BAD_ARGUMENT),
    'no_channels': (dict(channels=0), BAD_ARGUMENT),
    'layout_2': (dict(layout=2), BAD_ARGUMENT),
    'layout_minus_1': (dict(layout=-1), BAD_ARGUMENT),
    'rows_of_6_channels': (dict(layout=0, hw=0, channels=6), UNSUPPORTED),
    'rows_of_67_channels': (dict(layout=0, hw=0, channels=67), UNSUPPORTED),
    'map_of_35_pixels': (dict(hw=35, rows=70), UNSUPPORTED),
    'map_of_24_pixels': (dict(hw=24, rows=48), UNSUPPORTED),
    'rows_no_multiple_of_the_map': (dict(hw=1024, rows=2048 + 16), UNSUPPORTED),
}

SUMS_ORDER = ['a', 'sums', 'rows', 'channels', 'hw', 'layout', 'square_input', 'stream']
SUMS_GOOD = dict(a=P, sums=P, rows=2048, channels=512, hw=1024, layout=1, square_input=0, stream=None)
SUMS_CASES = {
    'null_a': dict(a=None),
    'null_sums': dict(sums=None),
    'null_a_as_rows': dict(a=None, layout=0),
    'null_sums_as_rows': dict(sums=None, layout=0),
    'rows_no_multiple_of_the_map': dict(rows=2048 + 1),
    'rows_no_multiple_of_an_odd_map': dict(hw=35, rows=71),
}


def _device_visible():
    import torch
    return torch.cuda.is_available()


@pytest.mark.parametrize('case', sorted(MOMENT_CASES))
def test_second_moment_refuses(case):
    if _device_visible():
        pytest.skip('a HIP device is visible: a regressed refusal would launch on placeholder pointers')
    change, want = MOMENT_CASES[case]
    args = dict(MOMENT_GOOD, **change)
    status = int(_lib.load().rw_second_moment_f32(*[args[n] for n in MOMENT_ORDER]))
    assert status == want, (case, status)


@pytest.mark.parametrize('entry', ['rw_channel_sums_f32', 'rw_channel_moments_f32'])
@pytest.mark.parametrize('case', sorted(SUMS_CASES))
def test_channel_sums_refuse(case, entry):
    if _device_visible():
        pytest.skip('a HIP device is visible: a regressed refusal would launch on placeholder pointers')
    args = dict(SUMS_GOOD, **SUMS_CASES[case])
    status = int(getattr(_lib.load(), entry)(*[args[n] for n in SUMS_ORDER]))
    assert status == BAD_ARGUMENT, (case, entry, status)


def expected_ksplit(channels, rows):
    """the rule of include/rewriting_hip.h (rw_second_moment_workspace_bytes), restated"""
    tile = 128 if channels >= 128 else 64
    tiles = -(-channels // tile)
    pairs = tiles * (tiles + 1) // 2
    chunks = -(-rows // 16)
    return max(1, min(512 // pairs, max(chunks // 8, 1)))


KNOWN_KSPLIT = {(4, 1): 1, (64, 17): 1, (132, 130): 1, (68, 2063): 16, (320, 1000): 7, (512, 4099): 32, (2048, 50): 1,
                (512, 10240): 51, (64, 16384): 128, (512, 2 ** 22 + 16): 51, (128, 1 << 20): 512}


def test_workspace_bytes_follow_the_rule_of_the_header():
    """ksplit * C^2 * 4 for every case of the suite; the slice counts the case comments of key_statistics_checks.py and
    the issue name are pinned by hand, so that the restated rule is itself checked"""
    shapes = {(c.channels, c.rows) for c in list(K.EXACT.values()) + list(K.ACCURACY.values())} | set(KNOWN_KSPLIT)
    size = _lib.load().rw_second_moment_workspace_bytes
    for channels, rows in sorted(shapes):
        ks = expected_ksplit(channels, rows)
        assert int(size(channels, rows)) == ks * channels * channels * 4, (channels, rows, ks)
    for (channels, rows), ks in KNOWN_KSPLIT.items():
        assert expected_ksplit(channels, rows) == ks, (channels, rows)
