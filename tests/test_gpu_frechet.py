"""The Frechet distance on the device (rw_frechet.hip, hip.eigh_psd_f64, samples.frechet_distance(device=...)) against
LAPACK, the truths and today's host route, at the margins of tests/frechet_checks.py.  RW_FRECHET_RECORD=path writes
every measured figure there (the 'device' part of profiles/frechet_accuracy.json)."""
import functools
import json
import os
import warnings

import numpy
import pytest
import torch

from rewriting_amd import hip, samples
from tests import frechet_checks as C

pytestmark = pytest.mark.gpu

B = hip.JACOBI_BLOCK
ORDERS = tuple(k * B for k in C.ORDERS_IN_B) + C.ORDERS
RECORD = []


@pytest.fixture(scope='module', autouse=True)
def record_figures():
    yield
    path = os.environ.get('RW_FRECHET_RECORD')
    if path:
        with open(path, 'w') as f:
            json.dump(dict(block=B, cases=RECORD), f, indent=1)


def dev(x):
    return torch.from_numpy(numpy.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """The inputs with everything the host computes once: LAPACK's measures, the truth, today's host distance."""
    mu1, s1, mu2, s2, exact = C.make_case(kind, n)
    truth = C.distance_truth(mu1, s1, mu2, s2, exact)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        try:
            e_ref = C.distance_error(samples.frechet_distance(mu1, s1, mu2, s2), truth, s1, s2)
        except ValueError:                                  # "Imaginary component": the host route gives no value
            e_ref = 0.0
    return dict(inputs=(mu1, s1, mu2, s2), truth=truth, e_ref=float(e_ref), lapack=C.lapack_measures(s1))


@pytest.mark.parametrize('n', ORDERS)
@pytest.mark.parametrize('kind', C.KINDS)
def test_eigh_against_lapack(kind, n):
    c = case(kind, n)
    s1 = c['inputs'][1]
    lres, lorth, llam = c['lapack']
    lam, v, sweeps = hip.eigh_psd_f64(dev(s1))
    lam, v = lam.cpu().numpy(), v.cpu().numpy()
    assert lam.shape == (n,) and v.shape == (n, n) and numpy.all(numpy.diff(lam) >= 0) and lam[0] >= 0
    res, orth = C.eigen_measures(s1, lam, v)
    dlam = float(numpy.abs(lam - llam).max() / max(llam.max(), numpy.finfo(float).tiny))
    RECORD.append(dict(test='eigh', case='%s-%d-b%d' % (kind, n, B), residual=res, orthogonality=orth, eigenvalues=dlam,
                       lapack_residual=lres, lapack_orthogonality=lorth, sweeps=sweeps))
    print(RECORD[-1])
    # LAPACK's own measure on the same matrix (a measure below one rounding is an accident of the input) times the margin
    assert res <= C.EIGEN_MARGIN * max(lres, C.EPS)
    assert orth <= C.EIGEN_MARGIN * max(lorth, C.EPS)
    assert dlam <= C.EIGEN_MARGIN * max(lres, C.EPS)
    assert sweeps < hip.JACOBI_MAX_SWEEPS
    if kind in ('diagonal', 'zero'):
        assert sweeps == 1 and res == 0 and orth == 0
    # eigenvalues alone: the same numbers without the vectors
    lam0, none, sweeps0 = hip.eigh_psd_f64(dev(s1), vectors=False)
    assert none is None and sweeps0 == sweeps and numpy.array_equal(lam0.cpu().numpy(), lam)


@pytest.mark.parametrize('n', ORDERS)
@pytest.mark.parametrize('kind', C.KINDS)
def test_distance_against_the_truth(kind, n):
    c = case(kind, n)
    mu1, s1, mu2, s2 = c['inputs']
    parts = {}
    d2 = hip.frechet_distance_f64(dev(mu1), dev(s1), dev(mu2), dev(s2), parts=parts)
    assert isinstance(d2, float) and numpy.isfinite(d2)
    e = float(C.distance_error(d2, c['truth'], s1, s2))
    e_twin = C.TWIN_DISTANCE_ERROR['%s-%d-b%d' % (kind, n, B)]
    bar = max(4 * e_twin, c['e_ref'], n * C.EPS)
    RECORD.append(dict(test='distance', case='%s-%d-b%d' % (kind, n, B), e=e, e_twin=e_twin, e_reference=c['e_ref'], bar=bar,
                       sweeps=list(parts['sweeps'])))
    print(RECORD[-1])
    assert e <= bar
    assert max(parts['sweeps']) < hip.JACOBI_MAX_SWEEPS
    assert samples.frechet_distance(dev(mu1), dev(s1), dev(mu2), dev(s2)) == d2         # device tensors take the route
    if kind == 'zero':                                      # every column below the floor: d^2 = |dmu|^2 + Tr S2, no NaN
        diff = mu1 - mu2
        assert abs(d2 - (diff.dot(diff) + numpy.trace(s2))) <= n * C.EPS * (diff.dot(diff) + numpy.trace(s2))
    if kind == 'same':                                      # d^2 = |dmu|^2 to rounding
        diff = mu1 - mu2
        assert abs(d2 - diff.dot(diff)) <= bar * 2 * numpy.trace(s1) + 8 * C.EPS * (diff.dot(diff) + 2 * numpy.trace(s1))


def test_host_inputs_with_device_given_take_the_device_route():
    mu1, s1, mu2, s2 = case('decay', 70)['inputs']
    want = hip.frechet_distance_f64(dev(mu1), dev(s1), dev(mu2), dev(s2))
    assert samples.frechet_distance(mu1, s1, mu2, s2, device='cuda') == want
    assert samples.frechet_distance(torch.from_numpy(mu1), s1.tolist(), mu2, s2, device=torch.device('cuda', 0)) == want
    assert abs(samples.frechet_distance([1.0], [[4.0]], [3.0], [[9.0]], device='cuda') - (4 + 1)) < 1e-12


@pytest.mark.parametrize('kind,n', [('decay', 70), ('rankdef', 96), ('span13', 64)])
def test_powers_of_two_scale_the_result_exactly(kind, n):
    mu1, s1, mu2, s2 = case(kind, n)['inputs']
    parts = {}
    d2 = hip.frechet_distance_f64(dev(mu1), dev(s1), dev(mu2), dev(s2), parts=parts)
    lam, v, sweeps = hip.eigh_psd_f64(dev(s1))
    for e in (60, -60):
        f, parts_f = 2.0 ** e, {}
        got = hip.frechet_distance_f64(dev(mu1 * 2.0 ** (e // 2)), dev(s1 * f), dev(mu2 * 2.0 ** (e // 2)), dev(s2 * f),
                                       parts=parts_f)
        assert got == d2 * f and parts_f['sweeps'] == parts['sweeps']
        lam_f, v_f, sweeps_f = hip.eigh_psd_f64(dev(s1 * f))
        assert torch.equal(lam_f, lam * f) and torch.equal(v_f, v) and sweeps_f == sweeps


def test_two_runs_give_the_same_bits():
    mu1, s1, mu2, s2 = case('rankdef', 160)['inputs']
    runs = []
    for _ in range(2):
        lam, v, sweeps = hip.eigh_psd_f64(dev(s1))
        runs.append((lam.cpu().numpy().tobytes(), v.cpu().numpy().tobytes(), sweeps,
                     hip.frechet_distance_f64(dev(mu1), dev(s1), dev(mu2), dev(s2))))
    assert runs[0] == runs[1]


def test_refusals_on_the_device():
    s = dev(case('decay', 70)['inputs'][1])
    for bad in (float('nan'), float('inf')):
        t = s.clone()
        t[3, 5] = t[5, 3] = bad
        with pytest.raises(ValueError, match='non-finite'):
            hip.eigh_psd_f64(t)
    with pytest.raises(RuntimeError, match='did not converge in 1 sweeps'):
        hip.eigh_psd_f64(s, max_sweeps=1)
    with pytest.raises(RuntimeError, match='float64'):
        hip.eigh_psd_f64(s.float())
    with pytest.raises(ValueError, match='contiguous'):
        hip.eigh_psd_f64(s.t()[::2, ::2])
    with pytest.raises(ValueError, match='square'):
        hip.eigh_psd_f64(s[:4])
    lam, _, _ = hip.eigh_psd_f64(s)                         # and the matrix is as it was: the solver works on a copy
    assert torch.equal(s, dev(case('decay', 70)['inputs'][1])) and lam.shape == (70,)


@pytest.mark.parametrize('m,n,k', [(70, 33, 45), (128, 64, 16), (200, 72, 129)])
def test_gemm_f64_against_torch(m, n, k):
    g = torch.Generator().manual_seed(m + n + k)
    for ta in (False, True):
        for tb in (False, True):
            a = dev(torch.randn((k, m) if ta else (m, k), dtype=torch.float64, generator=g).numpy())
            b = dev(torch.randn((n, k) if tb else (k, n), dtype=torch.float64, generator=g).numpy())
            rs, cs = (dev(torch.randn(x, dtype=torch.float64, generator=g).numpy()) for x in (m, n))
            want = rs[:, None] * ((a.t() if ta else a) @ (b.t() if tb else b)) * cs[None, :]
            got = hip.gemm_f64(a, b, ta, tb, rs, cs)
            # k products of magnitude |a||b| per entry, one rounding each, and the two scales
            bound = (k + 2) * C.EPS * (rs.abs()[:, None] * ((a.t() if ta else a).abs() @ (b.t() if tb else b).abs()) * cs.abs()[None, :])
            assert bool(((got - want).abs() <= bound).all())
            assert torch.equal(got, hip.gemm_f64(a, b, ta, tb, rs, cs))
    plain = hip.gemm_f64(a, b, ta, tb)
    assert torch.equal(plain * cs[None, :], hip.gemm_f64(a, b, ta, tb, col_scale=cs))


def test_feature_statistics_feed_the_device_route():
    torch.manual_seed(3)
    sets = []
    for shift in (0.0, 0.4):
        st = samples.FeatureStatistics()
        for rows in (40, 24):                               # fewer samples than features: a singular product
            st.add((torch.randn(rows, 96) * torch.linspace(0.2, 2.0, 96) + shift).cuda())
        sets.append(st)
    (mu1, s1), (mu2, s2) = (st.mean_cov(device=True) for st in sets)
    assert s1.is_cuda and s1.dtype == torch.float64 and mu1.shape == (96,)
    d_dev = samples.frechet_distance(mu1, s1, mu2, s2)
    (hm1, hs1), (hm2, hs2) = (st.mean_cov() for st in sets)
    assert samples.frechet_distance(hm1, hs1, hm2, hs2, device='cuda') == d_dev          # bit for bit
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d_host = samples.frechet_distance(hm1, hs1, hm2, hs2)
    truth = C.distance_truth(hm1, hs1, hm2, hs2)
    e, e_ref = C.distance_error(d_dev, truth, hs1, hs2), C.distance_error(d_host, truth, hs1, hs2)
    e_twin = C.distance_error(C.frechet_twin(hm1, hs1, hm2, hs2, B)[0], truth, hs1, hs2)
    print(dict(e=e, e_reference=e_ref, e_twin=e_twin))
    assert e <= max(4 * e_twin, e_ref, 96 * C.EPS)
