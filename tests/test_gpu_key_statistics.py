"""The key statistics on the device -- rw_second_moment_f32 and the channel-sum kernels of csrc/rw_stats.hip behind
RunningSecondMoment, RunningVariance, samples.FeatureStatistics and tally.tally_second_moment -- against integer results
that must be met EXACTLY at the shapes where a tile, a tail or a slab can go wrong, and against float64 under the measure
whitening sees.  The cases, the measures and where every bar comes from: tests/key_statistics_checks.py (shared with the
host twin of this file, tests/test_key_statistics_emulated.py).

Every figure of the accuracy, FeatureStatistics and RunningVariance cases goes to key_statistics.json in the directory
RW_REPORT_DIR names (default: test_reports/ at the repository's root, which git ignores)."""
import json

import pytest
import torch

from tests import key_statistics_checks as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('name', list(K.EXACT))
def test_integer_maps_give_the_integer_result(name):
    bad = K.check_exact(name, DEV)
    assert not bad, (name, K.EXACT[name].why, bad)


def test_large_then_small_launches_share_the_workspace_and_a_side_stream_agrees():
    bad = K.check_sequence(DEV)
    assert not bad, bad


def test_a_map_of_more_than_2_31_elements():
    free = torch.cuda.mem_get_info()[0]
    if free < 24 << 30:
        pytest.skip('%.1f GB free on the device; the map takes 9 GB' % (free / 2 ** 30))
    bad = K.check_past_31_bits(DEV)
    torch.cuda.empty_cache()
    assert not bad, bad


@pytest.mark.parametrize('name', list(K.ACCURACY))
def test_second_moment_against_float64(name):
    fig, ok = K.check_accuracy(name, DEV)
    print(name, json.dumps(fig, sort_keys=True))
    K.report('second_moment.' + name, fig)
    assert ok, (name, fig)


@pytest.mark.parametrize('features', [2048, 2046])
def test_feature_statistics_against_numpy_cov(features):
    """2048: the kernel per batch; 2046: the float64 branch FeatureStatistics keeps for f % 4 != 0"""
    fig, ok = K.check_features(features, DEV)
    print(features, json.dumps(fig, sort_keys=True))
    K.report('feature_statistics.%d' % features, fig)
    assert ok, (features, fig)


def test_tally_second_moment_with_a_short_last_batch():
    bad = K.check_tally(DEV)
    assert not bad, bad


@pytest.mark.parametrize('square_input', [False, True])
@pytest.mark.parametrize('nchw', [True, False])
def test_running_variance_against_float64(nchw, square_input):
    fig, bad = K.check_variance(nchw, DEV, square_input)
    print(nchw, square_input, json.dumps(fig, sort_keys=True))
    K.report('running_variance.%s%s' % ('nchw' if nchw else 'rows', '.squared' if square_input else ''), fig)
    assert not bad, (bad, fig)
