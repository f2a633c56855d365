"""The glue ops that are one kernel body for float and double (csrc/rw_ops.hip): the fp32 entry against the fp64 entry on
the same inputs -- the fp32 inputs (tensors and scalars) are the fp64 ones rounded once to float.

Bars, computed from the inputs (u = 2^-24, the unit roundoff of fp32; ulp = the spacing of fp32 at the fp64 result):
* a sum of n products: (n + 3) u sum |term_i| -- n for the recursive sum, 3 for the rounded inputs and the product;
* element-wise, no sum: 2 ulp (style_mul: three roundings of at most u each; adjust_latent without avg: a copy);
* a sum under a reciprocal square root, f = g(S)^(-1/2) (pixel_norm, demod): |df/dS| x the sum's bar + 2 ulp for the
  roundings after the sum;
* an addition can cancel, and no fp32 evaluation of rounded inputs is then within ulps of the result: noise_add,
  x + nw noise, is held as the sum of its n = 2 terms, and adjust_latent with avg, a + psi (w - a), as the n = 3 terms
  a, psi w, psi a its evaluation adds.
The shapes are the smallest that reach every branch of the shared bodies (and the fp32-only branches beside them)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24


def _pair(gen, *shape):
    """a float64 tensor on the device and itself rounded once to float"""
    t = torch.randn(*shape, generator=gen, dtype=torch.float64).to(DEV)
    return t, t.float()


def _ulp(v):
    """the spacing of fp32 at |v| (float64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 23)


def _sum_bar(n, abs_terms):
    return (n + 3) * U * abs_terms


def _within(what, got32, got64, bar):
    assert got32.dtype == torch.float32 and got64.dtype == torch.float64 and got32.shape == got64.shape
    assert bool(torch.isfinite(got64).all()) and bool(torch.isfinite(got32).all())
    err = (got32.double() - got64).abs()
    worst = (err / bar.clamp_min(1e-300)).max().item()
    print('%s: max error / bar = %.3f, max error = %.3e' % (what, worst, err.max().item()))
    assert bool((err <= bar).all()), (what, worst)


@pytest.mark.parametrize('shape', [(3, 70), (5, 512)])
def test_pixel_norm(shape):
    from rewriting_amd import hip
    x64, x32 = _pair(torch.Generator().manual_seed(10), *shape)
    eps, n = 1e-8, shape[1]
    got64, got32 = hip.pixel_norm_f64(x64, eps), hip.pixel_norm(x32, eps)
    s = (x64 * x64).sum(1, keepdim=True)                     # every term is positive: sum |term| = S
    bar = got64.abs() * 0.5 / (s + n * eps) * _sum_bar(n, s) + 2 * _ulp(got64)      # y = x (S / n + eps)^(-1/2)
    _within('pixel_norm %s' % (shape,), got32, got64, bar)


@pytest.mark.parametrize('with_avg', [True, False])
def test_adjust_latent(with_avg):
    from rewriting_amd import hip
    gen = torch.Generator().manual_seed(11)
    w64, w32 = _pair(gen, 3, 70)
    a64, a32 = _pair(gen, 70)
    psi, n_latent = 0.7, 6
    got64 = hip.adjust_latent_f64(w64, a64 if with_avg else None, n_latent, psi)
    got32 = hip.adjust_latent(w32, a32 if with_avg else None, n_latent, psi)
    assert got64.shape == (3, n_latent, 70)
    if with_avg:
        bar = _sum_bar(3, a64.abs() + abs(psi) * (w64.abs() + a64.abs()))[:, None, :].expand_as(got64)
    else:
        bar = 2 * _ulp(got64)
    _within('adjust_latent avg=%s' % with_avg, got32, got64, bar)


@pytest.mark.parametrize('shape', [(2, 5, 3, 5), (2, 5, 4, 4)])      # hw = 15: the shared scalar branch; 16: fp32's 16-byte one
def test_style_mul_and_noise_add(shape):
    from rewriting_amd import hip
    gen = torch.Generator().manual_seed(12)
    b, c, h, w = shape
    x64, x32 = _pair(gen, *shape)
    s64, s32 = _pair(gen, b, c)
    got64, got32 = hip.style_mul_f64(x64, s64), hip.style_mul(x32, s32)
    _within('style_mul %s' % (shape,), got32, got64, 2 * _ulp(got64))
    nz64, nz32 = _pair(gen, b, 1, h, w)
    nw64, nw32 = _pair(gen, 1)
    got64, got32 = hip.noise_add_f64(x64, nz64, nw64), hip.noise_add(x32, nz32, nw32)
    _within('noise_add %s' % (shape,), got32, got64, _sum_bar(2, x64.abs() + (nw64 * nz64).abs()))


def test_weight_sqsum():
    from rewriting_amd import hip
    w64, w32 = _pair(torch.Generator().manual_seed(13), 40, 24, 3, 3)
    w_scale = 1.0 / (24 * 9) ** 0.5
    got64, got32 = hip.weight_sqsum_f64(w64, w_scale), hip.weight_sqsum(w32, w_scale)
    assert got64.shape == (40, 24)
    _within('weight_sqsum', got32, got64, _sum_bar(9, got64))           # nine squares: sum |term| = the sum


@pytest.mark.parametrize('batch, in_ch, out_ch', [(2, 24, 40), (3, 64, 48)])      # the butterfly form; fp32 takes the MFMA form
def test_demod(batch, in_ch, out_ch):
    from rewriting_amd import hip
    gen = torch.Generator().manual_seed(14)
    w64, _ = _pair(gen, out_ch, in_ch, 3, 3)
    wsq64 = hip.weight_sqsum_f64(w64, 1.0 / (in_ch * 9) ** 0.5)
    s64, s32 = _pair(gen, batch, in_ch)
    eps = 1e-8
    got64, got32 = hip.demod_f64(wsq64, s64, eps), hip.demod(wsq64.float(), s32, eps)
    s = (s64 * s64) @ wsq64.t()                              # wsq >= 0: sum |term| = S
    bar = got64 * 0.5 / (s + eps) * _sum_bar(in_ch, s) + 2 * _ulp(got64)         # d = (S + eps)^(-1/2)
    _within('demod %d x %d -> %d' % (batch, in_ch, out_ch), got32, got64, bar)


@pytest.mark.parametrize('with_bias_and_skip', [True, False])
def test_to_rgb(with_bias_and_skip):
    from rewriting_amd import hip
    gen = torch.Generator().manual_seed(15)
    b, c, h, w = 2, 24, 5, 7                                  # hw = 35: the scalar form
    x64, x32 = _pair(gen, b, c, h, w)
    wt64, wt32 = _pair(gen, 3, c)
    s64, s32 = _pair(gen, b, c)
    bias64, bias32 = _pair(gen, 3) if with_bias_and_skip else (None, None)
    skip64, skip32 = _pair(gen, b, 3, h, w) if with_bias_and_skip else (None, None)
    w_scale = 1.0 / c ** 0.5
    got64 = hip.to_rgb_f64(x64, wt64, s64, bias64, skip64, w_scale)
    got32 = hip.to_rgb(x32, wt32, s32, bias32, skip32, w_scale)
    terms = torch.einsum('oi,bi,bihw->bohw', (w_scale * wt64).abs(), s64.abs(), x64.abs())
    n = c
    if with_bias_and_skip:
        terms = terms + bias64.abs().view(1, 3, 1, 1) + skip64.abs()
        n += 2
    _within('to_rgb bias, skip=%s' % with_bias_and_skip, got32, got64, _sum_bar(n, terms))
