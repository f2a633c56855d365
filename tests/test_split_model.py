"""The float64 model of the split-operand kernels (tests/split_model.py) on its own, at the shapes of
test_gpu_split_range.py: one pixel of image 0 raised to 2^k times the map's former maximum, the error measured on the
outputs that pixel cannot reach (and on image 1, which shares image 0's bound).  No kernel is involved: this pins what
the documented arithmetic does to the far field -- at k = 0 inside each family's bar, growing with k as the shared power
of two pushes the far field's Vl, then Vh, into f16's denormals -- and that the far field is (nearly) the whole map."""
import functools

import pytest
import torch

from tests import hip_emulation as E
from tests import split_model as S


@functools.lru_cache(maxsize=None)
def far_errors(kind, shape):
    """{k: (far field of the batch, image 1 alone)}: relative l2 of the model against the float64 convolution"""
    x0, wt, style = S.inputs(kind, shape)
    s, k4 = S.w_scale_of(shape), S.blur_kernel()
    dm = E.demod(E.weight_sqsum(wt, s), style)
    far = S.far_field(kind, shape)
    out = {}
    for k in S.KS:
        x = S.raise_pixel(kind, x0, k)
        model, ref = S.model(kind, x, wt, style, dm, s, k4), S.reference(kind, x, wt, style, dm, s, k4)
        assert model.shape == ref.shape == (shape[0], shape[2]) + tuple(far.shape[2:])
        assert model.dtype == torch.float64 and torch.isfinite(model).all()
        out[k] = (S.far_rel(model, ref, far), S.far_rel(model, ref, far, image=1))
    return out


@pytest.mark.parametrize('kind,shape', S.PROBLEMS)
def test_far_field_is_nearly_the_whole_map(kind, shape):
    far = S.far_field(kind, shape)
    assert far[1].all()                                   # the batch neighbour
    assert 0.0 < S.excluded_share(kind, shape) <= 0.15
    # the raised pixel's own reach lies inside what is excluded: a unit impulse there, through the float64 reference
    x0, wt, style = S.inputs(kind, shape)
    imp = torch.zeros_like(x0)
    c, py, px = S.raised_pixel(kind)
    imp[0, c, py, px] = 1.0
    ones = torch.ones(shape[0], shape[2])
    reach = S.reference(kind, imp, wt.abs() + 1, torch.ones_like(style), ones, 1.0, S.blur_kernel())
    assert (reach * far).abs().max().item() == 0.0 and reach.abs().max().item() > 0.0


@pytest.mark.parametrize('kind,shape', S.PROBLEMS)
def test_model_far_field_error_is_inside_the_bar_at_k0_and_grows_with_k(kind, shape):
    errs = far_errors(kind, shape)
    print('split model %s %s: ' % (kind, shape)
          + ', '.join('k=%d far %.3g image1 %.3g' % (k, *errs[k]) for k in S.KS))
    for which in (0, 1):
        e = [errs[k][which] for k in S.KS]
        assert e[0] < S.BARS[kind][0], e
        assert e[0] < e[1] < e[2] < e[3], e
        # from 2^16 on, every further bit of the bound costs the far field about one bit
        assert e[3] > 8 * e[2] > 0, e


def _fp32_route(kind, x, wt, style, dm, s, k4):
    """a host stand-in for the family's fp32 sibling: the same algorithm (direct sums, or F(4x4,3x3)) summed in fp32"""
    if kind in ('wino4', 'wino4_up'):
        xs, w = x * style[:, :, None, None], wt[0]
        if kind == 'wino4':
            return S._scaled(E._wino4_sums(xs, w), s, dm)
        return E._pixel_shuffle_phases(S._scaled(E._wino4_sums(xs, E._phase_weights(w, k4)), s, dm, 4), w.shape[0])
    return S.reference(kind, x, wt, style, dm, s, k4, dtype=torch.float32)


@pytest.mark.parametrize('fault,ks', [('headroom', (20,)), ('flush', (12, 16, 20))])
@pytest.mark.parametrize('kind,shape', S.PROBLEMS)
def test_the_error_size_bound_sees_the_two_smallest_faults(kind, shape, fault, ks):
    """test_gpu_split_range.test_far_field_error_is_the_models holds a kernel to sqrt(2) || model - ref || + 4 || fp32
    sibling - ref || on the far field.  A model with one bit of headroom less (at k = 20), or with the f16 denormals of the
    input pair flushed (from k = 12 on), is outside that bound: the device test would fail for either."""
    x0, wt, style = S.inputs(kind, shape)
    s, k4 = S.w_scale_of(shape), S.blur_kernel()
    dm = E.demod(E.weight_sqsum(wt, s), style)
    far = S.far_field(kind, shape)
    for k in ks:
        x = S.raise_pixel(kind, x0, k)
        ref = S.reference(kind, x, wt, style, dm, s, k4)
        good, bad = S.model(kind, x, wt, style, dm, s, k4), S.model(kind, x, wt, style, dm, s, k4, fault=fault)
        sib = _fp32_route(kind, x, wt, style, dm, s, k4)
        for image in (None, 1):
            bound = 2 ** 0.5 * S.far_norm(good, ref, far, image) + 4 * S.far_norm(sib, ref, far, image)
            assert S.far_norm(bad, ref, far, image) > bound, (k, image, S.far_norm(bad, ref, far, image) / bound)
