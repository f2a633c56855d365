"""rw_key_response_f32 / hip.key_response on the device against the float64 einsum.

The error bar is derived, not tuned: a float32 sum of C products, in any order, with or without FMA, differs from the
exact sum by at most 1.01 * C * 2^-24 * sum_c |k_c * a_c| + 1e-30 (tests/search_checks.py: exact_response).  Dropping a
single channel moves a response by about sum / C, 60 times the bar at C = 512."""
import pytest
import torch

from tests.search_checks import exact_response

pytestmark = pytest.mark.gpu

# (images, C, H, W, K): maps smaller than a wave with several images per wave (4x4, 8x8), a row of 6x6 = 36 floats (nine
# 16-byte loads: images straddle waves), 5x5 and 7x7 (hw % 4 != 0: the form with one pixel per lane; the 4-byte aligned view
# below takes it too), the ordinary 32x32 map, one image over many workgroups (128x128),
# channel counts that leave every tail of the unrolled channel loop (3, 24, 32, 512), one key / an odd count / a full
# group, a single image / a pair / an odd batch
CASES = [
    (1, 3, 4, 4, 1),
    (11, 512, 4, 4, 8),
    (2, 24, 8, 8, 3),
    (11, 3, 6, 6, 1),
    (2, 512, 6, 6, 8),
    (2, 24, 5, 5, 3),
    (11, 512, 7, 7, 8),
    (1, 32, 32, 32, 3),
    (11, 24, 32, 32, 1),
    (11, 512, 32, 32, 8),
    (2, 8, 128, 128, 8),
    (1, 8, 128, 128, 3),
]


def _inputs(images, c, h, w, k, seed=0):
    gen = torch.Generator().manual_seed(seed + 1000 * c + h)
    acts = torch.randn(images, c, h, w, generator=gen)
    keys = torch.randn(k, c, generator=gen)
    return acts, keys


def _within(heat, acts, keys):
    want, bound = exact_response(acts, keys)
    err = (heat.double().cpu() - want).abs()
    worst = (err / bound).max().item()
    print('largest error / bound: %.3f' % worst)
    assert (err <= bound).all(), worst


@pytest.mark.parametrize('images,c,h,w,k', CASES)
def test_heat_within_the_bar_and_peak_is_its_maximum(images, c, h, w, k):
    from rewriting_amd import hip
    acts, keys = _inputs(images, c, h, w, k)
    heat, peak = hip.key_response(acts.cuda(), keys.cuda())
    assert heat.shape == (images, k, h, w) and peak.shape == (images, k)
    assert heat.dtype == peak.dtype == torch.float32
    _within(heat, acts, keys)
    assert torch.equal(peak, heat.flatten(2).amax(2))
    only_heat, no_peak = hip.key_response(acts.cuda(), keys.cuda(), want_peak=False)
    assert no_peak is None and torch.equal(only_heat, heat)


def test_all_negative_responses_have_negative_peaks():
    from rewriting_amd import hip
    acts, keys = _inputs(5, 24, 8, 8, 3)
    acts, keys = -acts.abs() - 0.01, keys.abs() + 0.01
    heat, peak = hip.key_response(acts.cuda(), keys.cuda())
    _within(heat, acts, keys)
    assert (peak < 0).all() and torch.equal(peak, heat.flatten(2).amax(2))


@pytest.mark.parametrize('h', [4, 6, 7, 16])
def test_a_row_does_not_depend_on_its_launch(h):
    """Image 7 alone is its row in the batch of 11; key 5 alone, and in slot 0, is its row among eight -- bit for bit."""
    from rewriting_amd import hip
    acts, keys = _inputs(11, 512, h, h, 8)
    acts, keys = acts.cuda(), keys.cuda()
    heat, peak = hip.key_response(acts, keys)
    h7, p7 = hip.key_response(acts[7:8].contiguous(), keys)
    assert torch.equal(h7[0], heat[7]) and torch.equal(p7[0], peak[7])
    h5, p5 = hip.key_response(acts, keys[5])
    assert h5.shape == (11, 1, h, h)
    assert torch.equal(h5[:, 0], heat[:, 5]) and torch.equal(p5[:, 0], peak[:, 5])
    moved = torch.cat([keys[5:6], keys[:5], keys[6:]])
    h0, p0 = hip.key_response(acts, moved)
    assert torch.equal(h0[:, 0], heat[:, 5]) and torch.equal(p0[:, 0], peak[:, 5])
    assert torch.equal(h0[:, 1:6], heat[:, 0:5])


def test_a_key_map_at_a_4_byte_aligned_address():
    from rewriting_amd import hip
    acts, keys = _inputs(3, 24, 8, 8, 3)
    aligned = acts.cuda()
    buf = torch.empty(acts.numel() + 1, device='cuda')
    shifted = buf[1:].view(acts.shape)
    shifted.copy_(aligned)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    heat, peak = hip.key_response(shifted, keys.cuda())
    _within(heat, acts, keys)
    want_heat, want_peak = hip.key_response(aligned, keys.cuda())
    assert torch.equal(heat, want_heat) and torch.equal(peak, want_peak)     # the same chain of fmaf's in both forms


def test_eleven_keys_are_a_group_of_eight_and_one_of_three():
    from rewriting_amd import hip
    acts, keys = _inputs(3, 32, 8, 8, 11)
    acts, keys = acts.cuda(), keys.cuda()
    heat, peak = hip.key_response(acts, keys)
    assert heat.shape == (3, 11, 8, 8) and peak.shape == (3, 11)
    h8, p8 = hip.key_response(acts, keys[:8])
    h3, p3 = hip.key_response(acts, keys[8:])
    assert torch.equal(heat, torch.cat([h8, h3], dim=1)) and torch.equal(peak, torch.cat([p8, p3], dim=1))
    _within(heat, acts.cpu(), keys.cpu())


def test_refused_tensors():
    from rewriting_amd import hip
    acts, keys = _inputs(2, 8, 4, 4, 2)
    with pytest.raises(RuntimeError, match='contiguous'):
        hip.key_response(acts.cuda().permute(0, 1, 3, 2), keys.cuda())
    with pytest.raises(RuntimeError, match='contiguous'):
        hip.key_response(acts.cuda()[:, ::2], keys.cuda()[:, ::2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.key_response(acts, keys.cuda())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.key_response(acts.cuda(), keys)
    with pytest.raises(RuntimeError, match='fp32 only'):
        hip.key_response(acts.cuda().half(), keys.cuda().half())
    with pytest.raises(RuntimeError, match='fp32 only'):
        hip.key_response(acts.cuda(), keys.cuda().double())
    with pytest.raises(RuntimeError, match='does not go with'):
        hip.key_response(acts.cuda(), keys.cuda()[:, :7])
