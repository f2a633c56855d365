"""The checks of the key statistics (tests/key_statistics_checks.py) on the host, through the CPU branches of the package
and tests/hip_emulation.py: the integer references, the admissibility asserts, the yardsticks and the report writer, on a
machine without a GPU -- the references alone pass every bar -- and the proof that the checks bite: seeded faults, each
caught by the check aimed at it.  The map of more than 2^31 elements is a GPU test only."""
import json
import os

import pytest
import torch

from tests import hip_emulation
from tests import key_statistics_checks as K


@pytest.mark.parametrize('branch', ['emulation', 'cpu'])
@pytest.mark.parametrize('name', list(K.EXACT))
def test_integer_maps_give_the_integer_result(name, branch, request):
    if branch == 'emulation':
        request.getfixturevalue('emulated_hip')
        assert not K.check_exact(name, 'cpu')
    else:                       # the CPU branch of RunningSecondMoment: the class alone, no wrapper
        from rewriting_amd.utils import runningstats
        c = K.EXACT[name]
        a, want, _, _ = K.exact_problem(name)
        stat = runningstats.RunningSecondMoment()
        (stat.add_nchw if c.nchw else stat.add)(a)
        assert stat.count == c.rows and torch.equal(stat.mom2.double(), want.double())


def test_inadmissible_integer_cases_are_refused_before_anything_runs():
    K.assert_exact_admissible(2 ** 22 + 16, bound=1)
    K.assert_exact_admissible(207126, fourth=True)
    for kwargs in (dict(rows=2 ** 24, bound=1), dict(rows=1864136), dict(rows=932068, adds=2),
                   dict(rows=207127, fourth=True)):
        with pytest.raises(AssertionError):
            K.assert_exact_admissible(**kwargs)


def test_sequence_and_tally(emulated_hip):
    assert not K.check_sequence('cpu')
    assert not K.check_tally('cpu')


@pytest.mark.parametrize('name', list(K.ACCURACY))
def test_second_moment_against_float64(emulated_hip, name, tmp_path, monkeypatch):
    """the emulation is the float32 product of the CPU branch: e_hip = e_ref here.  The yardsticks themselves are
    bracketed (u = 2^-24): both between 1 u and 64 u on every shape, where float32 sums of these lengths belong."""
    monkeypatch.setenv('RW_REPORT_DIR', str(tmp_path))
    fig, ok = K.check_accuracy(name, 'cpu')
    assert ok, fig
    assert K.U < fig['e_ref'] < 64 * K.U and K.U < fig['e_seq'] < 64 * K.U, fig
    path = K.report('second_moment.' + name, fig)
    K.report('other', 1)
    assert os.path.dirname(path) == str(tmp_path)
    with open(path) as f:
        assert json.load(f) == {'second_moment.' + name: fig, 'other': 1}


@pytest.mark.parametrize('dtype,factor', [(torch.float16, 2.5), (torch.bfloat16, 25)])
@pytest.mark.parametrize('name', list(K.ACCURACY))
def test_reduced_precision_operands_miss_the_bar(emulated_hip, name, dtype, factor):
    """operands rounded to f16 miss the bar by more than 2.5 times on every shape, to bf16 by more than 25 times
    (measured: 4.7 and 31 times at the least, both on (16384, 64), where e_seq is largest)"""
    if dtype == torch.float16:
        a = K.accuracy_problem(name)[0]
        assert a.abs().max() < 65504, 'the data overflows f16: the case would prove nothing about rounding'
    fig, ok = K.check_accuracy(name, 'cpu', operand=lambda a: a.to(dtype).float())
    print(name, dtype, fig)
    assert not ok
    assert fig['ratio'] > factor * K.MARGIN, fig


FAULTS = {
    'dropped_row': lambda a: a[:-1],
    'doubled_row': lambda a: torch.cat([a, a[-1:]]),
    'dropped_channel_of_the_last_tile': lambda a: torch.cat([a[:, :-1], torch.zeros_like(a[:, -1:])], 1),
}


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_a_seeded_fault_changes_an_integer(emulated_hip, monkeypatch, fault):
    clean = hip_emulation.second_moment_accumulate

    def faulted(mom2, a, nchw=False):
        a = K.rows_of(a, nchw)
        return clean(mom2, FAULTS[fault](a), nchw=False)
    from rewriting_amd import hip
    monkeypatch.setattr(hip, 'second_moment_accumulate', faulted)
    for name in ('r17x64', 'r130x132', 'n3x67x4x8'):
        bad = K.check_exact(name, 'cpu')
        assert 'exact' in bad and 'exact_onto_nonzero' in bad, (fault, name, bad)


def test_a_stale_slab_changes_an_integer(emulated_hip, monkeypatch):
    """what check_sequence is for: a small launch that also sums a slab the large one left"""
    clean = hip_emulation.second_moment_accumulate
    left = {}

    def faulted(mom2, a, nchw=False):
        c = a.shape[1]
        if c in left:
            mom2 += left[c]
        clean(mom2, a, nchw=nchw)
        left[64] = torch.ones(64, 64)
        return mom2
    from rewriting_amd import hip
    monkeypatch.setattr(hip, 'second_moment_accumulate', faulted)
    assert 'r17x64@1' in K.check_sequence('cpu')


@pytest.mark.parametrize('features', [2048, 2046])
def test_feature_statistics_against_numpy_cov(emulated_hip, features):
    fig, ok = K.check_features(features, 'cpu')
    assert ok, fig


def test_feature_statistics_cpu_branch():
    fig, ok = K.check_features(2046, 'cpu')            # not emulated: float64 throughout, whatever f
    assert ok, fig


@pytest.mark.parametrize('square_input', [False, True])
@pytest.mark.parametrize('nchw', [True, False])
def test_running_variance_against_float64(emulated_hip, nchw, square_input):
    """the emulated device branch (one pass about the mean of the first samples) holds the bar; the host's own figures, which are
    the yardstick, sit where two-pass float32 arithmetic belongs: below 4 u in every channel"""
    fig, bad = K.check_variance(nchw, 'cpu', square_input)
    print(fig)
    assert not bad, (bad, fig)
    assert fig['variance_cpu'] < 4 * K.U, fig


@pytest.mark.parametrize('nchw', [True, False])
def test_raw_sums_miss_the_variance_bar(emulated_hip, monkeypatch, nchw):
    """sum v^2 - n mean^2 from float32 raw sums, the form the device branch had: off by (mean / std)^2 roundings"""
    from rewriting_amd import hip

    def raw(a, nchw=False, square_input=False):
        s = hip_emulation.channel_sums(a, nchw=nchw, square_input=square_input)
        return torch.stack([torch.zeros_like(s[0]), s[0], s[1]])
    monkeypatch.setattr(hip, 'channel_moments', raw)
    fig, bad = K.check_variance(nchw, 'cpu')
    print(fig)
    assert 'variance' in bad and 'count' not in bad, (bad, fig)
    assert fig['per_ratio']['100']['variance_hip'] > 1e-4 > fig['per_ratio']['1']['variance_hip'], fig
