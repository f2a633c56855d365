"""The host side of the device Frechet route: the round-robin schedule, the padding, the numpy twin of the block Jacobi
against the truths, the refusals, and the default route of samples.frechet_distance, unchanged.  No GPU."""
import inspect
import itertools
import warnings

import numpy
import pytest
import torch

from rewriting_amd import hip, samples
from tests import frechet_checks as C


@pytest.mark.parametrize('count', [2, 3, 4, 5, 10])
def test_round_robin_meets_every_pair_exactly_once_per_sweep(count):
    steps = C.schedule(count)
    assert len(steps) == count + (count & 1) - 1
    met = [p for step in steps for p in step]
    assert sorted(met) == sorted(itertools.combinations(range(count), 2))
    for step in steps:                                      # the pairs of one launch share no block
        blocks = [b for p in step for b in p]
        assert len(blocks) == len(set(blocks))
        assert len(step) == count // 2                      # an odd count: one block has a bye in every step


def test_padding():
    for b in (8, 16):
        for n, want in [(1, 2 * b), (2 * b, 2 * b), (2 * b + 1, 3 * b), (70, 72 if b == 8 else 80), (2048, 2048)]:
            assert C.padded_order(n, b) == hip.jacobi_padded_order(n, b) == want
    assert hip.jacobi_padded_order(70) == C.padded_order(70, hip.JACOBI_BLOCK)
    assert hip.JACOBI_BLOCK in (8, 16) and hip.JACOBI_MAX_SWEEPS == C.MAX_SWEEPS
    # the padding's columns are dropped again: eigenvalues and vectors of the order asked for
    lam, v, _ = C.eigh_twin(numpy.diag([3.0, 0.0, 1.0]), 8)
    assert sorted(lam) == [0.0, 1.0, 3.0] and v.shape == (3, 3)
    assert numpy.array_equal(numpy.abs(v[:, numpy.argsort(lam)]), numpy.eye(3)[:, [1, 2, 0]])


@pytest.mark.parametrize('kind', C.KINDS)
@pytest.mark.parametrize('n,b', [(16, 8), (32, 16), (44, 8), (70, 16)])
def test_twin_against_the_truths(kind, n, b):
    mu1, s1, mu2, s2, exact = C.make_case(kind, n)
    lam, v, sweeps = C.eigh_twin(s1, b)
    res, orth = C.eigen_measures(s1, lam, v)
    lres, lorth, llam = C.lapack_measures(s1)
    dlam = numpy.abs(numpy.sort(lam) - llam).max() / max(llam.max(), numpy.finfo(float).tiny)
    assert res <= C.EIGEN_MARGIN * max(lres, C.EPS)
    assert orth <= C.EIGEN_MARGIN * max(lorth, C.EPS)
    assert dlam <= C.EIGEN_MARGIN * max(lres, C.EPS)
    assert sweeps < C.MAX_SWEEPS
    if kind in ('diagonal', 'zero'):
        assert sweeps == 1 and res == 0 and orth == 0
    d2, (sw1, sw2) = C.frechet_twin(mu1, s1, mu2, s2, b)
    e = C.distance_error(d2, C.distance_truth(mu1, s1, mu2, s2, exact), s1, s2)
    # every eigenvalue of F^T S2 F is known to n eps mu_max, its root to sqrt(n eps mu_max) at worst (a null direction),
    # and sqrt(mu_max) <= (Tr S1 + Tr S2) / 2: n such terms
    assert e <= n * numpy.sqrt(n * C.EPS)
    assert numpy.isfinite(d2) and max(sw1, sw2) < C.MAX_SWEEPS
    if kind == 'zero':
        diff = mu1 - mu2
        assert d2 == diff.dot(diff) + numpy.trace(s1) + numpy.trace(s2)


def test_twin_scales_exactly():
    mu1, s1, mu2, s2, _ = C.make_case('rankdef', 40)
    d2, sweeps = C.frechet_twin(mu1, s1, mu2, s2, 8)
    for e in (60, -60):
        f = 2.0 ** e
        got, sw = C.frechet_twin(mu1 * 2.0 ** (e // 2), s1 * f, mu2 * 2.0 ** (e // 2), s2 * f, 8)
        assert got == d2 * f and sw == sweeps


def test_refusals():
    good = torch.eye(4, dtype=torch.float64)
    with pytest.raises(ValueError, match='square'):
        hip.eigh_psd_f64(torch.zeros(4, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match='square'):
        hip.eigh_psd_f64(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='float64'):
        hip.eigh_psd_f64(good.float())
    with pytest.raises(ValueError, match='contiguous'):
        hip.eigh_psd_f64(torch.zeros(8, 4, dtype=torch.float64)[::2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.eigh_psd_f64(good)
    with pytest.raises(TypeError):
        hip.eigh_psd_f64(good.numpy())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        samples.frechet_distance([0.0], [[1.0]], [1.0], [[2.0]], device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.frechet_distance_f64(torch.zeros(4, dtype=torch.float64), good, torch.zeros(4, dtype=torch.float64), good)


def _frechet_as_it_was(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """samples.frechet_distance before the device route was added (metrics/fid.py:137-187), word for word."""
    from scipy import linalg
    mu1, mu2 = numpy.atleast_1d(mu1), numpy.atleast_1d(mu2)
    sigma1, sigma2 = numpy.atleast_2d(sigma1), numpy.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape and sigma1.shape == sigma2.shape
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not numpy.isfinite(covmean).all():
        offset = numpy.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if numpy.iscomplexobj(covmean):
        if not numpy.allclose(numpy.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError('Imaginary component {}'.format(numpy.max(numpy.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff) + numpy.trace(sigma1) + numpy.trace(sigma2) - 2 * numpy.trace(covmean)


@pytest.mark.parametrize('kind', ['decay', 'rankdef', 'commute'])
def test_default_route_is_unchanged_bit_for_bit(kind):
    sig = inspect.signature(samples.frechet_distance)
    assert list(sig.parameters) == ['mu1', 'sigma1', 'mu2', 'sigma2', 'eps', 'device']
    assert sig.parameters['device'].default is None and sig.parameters['eps'].default == 1e-6
    mu1, s1, mu2, s2, _ = C.make_case(kind, 24)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = _frechet_as_it_was(mu1, s1, mu2, s2)
        assert samples.frechet_distance(mu1, s1, mu2, s2) == want
        # host tensors without device= are host inputs
        assert samples.frechet_distance(torch.from_numpy(mu1), torch.from_numpy(s1), mu2, s2) == want


def test_mean_cov_on_the_device_of_the_sums_is_mean_cov():
    torch.manual_seed(0)
    stats = samples.FeatureStatistics()
    stats.add(torch.randn(12, 5))
    stats.add(torch.randn(7, 5))
    mu, sigma = stats.mean_cov()
    tmu, tsigma = stats.mean_cov(device=True)
    assert isinstance(mu, numpy.ndarray) and isinstance(tmu, torch.Tensor) and tsigma.dtype == torch.float64
    assert numpy.array_equal(tmu.numpy(), mu) and numpy.array_equal(tsigma.numpy(), sigma)
