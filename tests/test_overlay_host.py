"""Device-side overlays, the part that needs no device: the restatement of tests/overlay_checks.py against the yardstick
(ImageVisualizer.pytorch_masked_image on the CPU) over both tables of inputs, the closed-form outline against
border_from_mask, what rw_render_bytes_f32 refuses, the constants, and the rewriter's device_render routing with
hip.render_bytes replaced by a torch stand-in made from the restatement.  The kernel itself is tested by
tests/test_gpu_overlay.py."""
import os
import re

import numpy as np
import PIL.Image
import pytest
import torch

from rewriting_amd import _lib
from tests import overlay_checks as oc
from tests.search_checks import make_rewriter

BAD_ARGUMENT, UNSUPPORTED = 10001, 10002
RED = (255, 0, 0)


def _against_the_yardstick(image, heat, level, exact):
    H, W = image.shape[-2:]
    inside = oc.inside64(heat, level, H, W)
    if exact:
        oc.assert_empty_band(heat, level, H, W)
    for thickness in (1, 2, 3):
        for inside_color in (None, RED):
            kw = dict(thickness=thickness, inside_color=inside_color)
            want = oc.host_picture(image, heat, level, **kw)
            got = oc.picture(image, inside, **kw)
            oc.compare(got, want, None if exact else heat, level, thickness)


@pytest.mark.parametrize('q', oc.BAND_QUANTILES)
@pytest.mark.parametrize('seed', oc.BAND_SEEDS)
@pytest.mark.parametrize('shape', oc.BAND_SHAPES, ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_restatement_is_the_host_picture_outside_the_band(shape, seed, q):
    h, w, H, W = shape
    heat, level = oc.band_case(seed, q, h, w)
    _against_the_yardstick(oc.image_for(seed, H, W), heat, level, exact=False)


@pytest.mark.parametrize('seed', oc.BAND_SEEDS)
@pytest.mark.parametrize('shape', oc.EXACT_SHAPES, ids=lambda s: '%dx%d_to_%dx%d' % s)
def test_restatement_is_the_host_picture_on_the_exact_rows(shape, seed):
    h, w, H, W = shape
    _against_the_yardstick(oc.image_for(seed, H, W), oc.exact_heat(seed, h, w), oc.EXACT_LEVEL, exact=True)


def test_restated_bytes_are_as_image():
    from rewriting_amd.utils import renormalize
    image = oc.image_for(0, 20, 37)
    image[0, 0, :6] = torch.tensor([1.5, -1.5, float('inf'), float('-inf'), 1.0, -1.0])
    want = np.asarray(renormalize.as_image(image))
    assert np.array_equal(oc.picture(image), want) and want.min() == 0 and want.max() == 255


@pytest.mark.parametrize('thickness', [0, 1, 2, 3, 5])
def test_closed_form_border_is_border_from_mask(thickness):
    from rewriting_amd.utils import imgviz
    for seed in range(4):
        mask = torch.rand(37, 53, generator=torch.Generator().manual_seed(seed)) < (0.02, 0.3, 0.7, 0.98)[seed]
        want = imgviz.border_from_mask(mask, thickness).numpy() if thickness else np.zeros((37, 53), bool)
        assert np.array_equal(oc.closed_form_border(mask, thickness), want)


# ---- the C entry's refusals, on placeholder pointers that are never dereferenced
P = 0x10000
GOOD = dict(image=P, selector=P, out=P, images=3, height=64, width=64, mode=1, sel_height=8, sel_width=8, level=0.5,
            thickness=1, border_rgb=0xffff, inside_rgb=-1, outside_bright=0.5, stream=None)
ORDER = ['image', 'selector', 'out', 'images', 'height', 'width', 'mode', 'sel_height', 'sel_width', 'level',
         'thickness', 'border_rgb', 'inside_rgb', 'outside_bright', 'stream']
REFUSED = {
    'null_image': (dict(image=None), BAD_ARGUMENT),
    'null_out': (dict(out=None), BAD_ARGUMENT),
    'no_images': (dict(images=0), BAD_ARGUMENT),
    'negative_images': (dict(images=-1), BAD_ARGUMENT),
    'no_rows': (dict(height=0), BAD_ARGUMENT),
    'no_columns': (dict(width=0), BAD_ARGUMENT),
    'image_past_31_bits': (dict(height=1 << 15, width=(1 << 16) // 3 + 1, mode=0), BAD_ARGUMENT),   # 3 H W = 2^31 + 65536
    'mode_3': (dict(mode=3), BAD_ARGUMENT),
    'mode_minus_1': (dict(mode=-1), BAD_ARGUMENT),
    'heat_without_selector': (dict(selector=None), BAD_ARGUMENT),
    'mask_without_selector': (dict(mode=2, selector=None, sel_height=64, sel_width=64), BAD_ARGUMENT),
    'mask_of_another_size': (dict(mode=2, sel_height=64, sel_width=32), BAD_ARGUMENT),
    'thickness_9': (dict(thickness=9), BAD_ARGUMENT),
    'negative_thickness': (dict(thickness=-1), BAD_ARGUMENT),
    'infinite_outside_bright': (dict(outside_bright=float('inf')), BAD_ARGUMENT),
    'nan_outside_bright': (dict(outside_bright=float('nan')), BAD_ARGUMENT),
    'heat_one_high': (dict(sel_height=1), UNSUPPORTED),
    'heat_one_wide': (dict(sel_width=1), UNSUPPORTED),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_render_bytes_entry_refuses(case):
    if torch.cuda.is_available():
        pytest.skip('a HIP device is visible: a regressed refusal would launch on placeholder pointers')
    change, want = REFUSED[case]
    args = dict(GOOD, **change)
    status = int(_lib.load().rw_render_bytes_f32(*[args[n] for n in ORDER]))
    assert status == want, (case, status)


def test_the_limit_of_the_header_is_the_limit_of_the_wrapper():
    from rewriting_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'rewriting_hip.h')).read()
    assert int(re.search(r'#define RW_RENDER_MAX_THICKNESS (\d+)', text).group(1)) == hip.RENDER_MAX_THICKNESS == 8
    assert _lib.ABI_VERSION == 11 and 'rw_render_bytes_f32' in _lib.SIGNATURES


# ---- the rewriter's routing
SIZE, NSEEDS, LAYER = 32, 10, 4


@pytest.fixture
def routed(emulated_hip, monkeypatch):
    from rewriting_amd import hip
    calls = []

    def spy(images, activations=None, mask=None, level=None, **kw):
        calls.append(dict(images=images.shape[0], activations=activations, mask=mask, level=level, **kw))
        return oc.render_bytes_stand_in(images, activations, mask, level, **kw)
    monkeypatch.setattr(hip, 'render_bytes', spy, raising=False)
    return calls


def _same_kind(got, want):
    assert type(got) is type(want) and got.mode == want.mode == 'RGB' and got.size == want.size


def test_device_render_is_a_constructor_keyword(emulated_hip):
    gw = make_rewriter('cpu', SIZE, NSEEDS, LAYER)
    assert gw.device_render is False
    assert make_rewriter('cpu', SIZE, NSEEDS, LAYER, device_render=True).device_render is True


def test_render_image_batch_routes_through_render_bytes(routed):
    gw = make_rewriter('cpu', SIZE, NSEEDS, LAYER, device_render=True)
    key = torch.randn(gw.k_shape[1], generator=torch.Generator().manual_seed(0))
    key = key / key.norm()
    seeds = list(range(7))
    with torch.no_grad():
        acts = gw.context_acts(gw.context_model(gw.get_z(0)))
    level = 0.75 * (acts * key[None, :, None, None]).sum(1).reshape(-1).sort()[0][int(acts.shape[2] * acts.shape[3] * 0.9)]
    level = level.item()
    got = gw.render_image_batch(seeds, key, level, border_color=[255, 255, 255])
    assert [c['images'] for c in routed] == [3, 3, 1]                 # the batches of three stay
    assert all(c['border_color'] == [255, 255, 255] and c['level'] == level for c in routed)
    heats = torch.cat([c['activations'] for c in routed])
    assert heats.shape == (7,) + tuple(gw.k_shape[2:])
    del routed[:]
    gw.device_render = False
    want = gw.render_image_batch(seeds, key, level, border_color=[255, 255, 255])
    assert not routed
    assert isinstance(got, list) and isinstance(want, list) and len(got) == len(want) == 7     # one picture per seed
    for j in range(7):
        _same_kind(got[j], want[j])
        oc.compare(np.asarray(got[j]), np.asarray(want[j]), heats[j], level, 1)
    # without a key: the plain bytes, still in threes, exact
    gw.device_render = True
    got = gw.render_image_batch(seeds[:4])
    assert [c['images'] for c in routed] == [3, 1] and all(c['activations'] is None for c in routed)
    gw.device_render = False
    want = gw.render_image_batch(seeds[:4])
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        _same_kind(g, w)
        assert np.array_equal(np.asarray(g), np.asarray(w))


def test_render_image_and_render_object_route_through_render_bytes(routed):
    gw = make_rewriter('cpu', SIZE, NSEEDS, LAYER, device_render=True)
    key = torch.randn(gw.k_shape[1], generator=torch.Generator().manual_seed(1))
    mask = torch.zeros(SIZE, SIZE, dtype=torch.bool)
    mask[5:20, 0:9] = True
    with torch.no_grad():
        target_output = gw.target_model(gw.context_model(gw.get_z(2)))
    box = (1, 2, gw.v_shape[2] - 2, gw.v_shape[3] - 1)

    def both(fn):
        pictures = []
        for flag in (True, False):
            gw.device_render = flag
            del routed[:]
            pictures.append(fn())
            assert len(routed) == (1 if flag else 0)
            if flag:
                call = dict(routed[0])
        _same_kind(*pictures)
        return np.asarray(pictures[0]), np.asarray(pictures[1]), call

    got, want, call = both(lambda: gw.render_image(3))
    assert call['activations'] is None and call['mask'] is None and np.array_equal(got, want)
    got, want, call = both(lambda: gw.render_image(3, mask=mask, thickness=2))
    assert call['mask'].shape == (1, SIZE, SIZE) and call['thickness'] == 2 and np.array_equal(got, want)
    got, want, call = both(lambda: gw.render_image(3, key, 0.1, thickness=2, inside_color=[0, 0, 255]))
    assert call['images'] == 1 and call['level'] == 0.1
    oc.compare(got, want, call['activations'][0], 0.1, 2)
    got, want, call = both(lambda: gw.render_object(target_output))
    assert call['activations'] is None and np.array_equal(got, want)
    got, want, call = both(lambda: gw.render_object(target_output, box=box))
    assert call['thickness'] == 3 and call['border_color'] == [255, 0, 0] and call['level'] == 0.0
    oc.compare(got, want, call['activations'][0], 0.0, 3)


def test_what_the_kernel_does_not_take_stays_on_the_host(routed):
    gw = make_rewriter('cpu', SIZE, NSEEDS, LAYER, device_render=True)
    key = torch.randn(gw.k_shape[1], generator=torch.Generator().manual_seed(2))
    pictures = gw.render_image_batch([0, 1], key, 0.1, thickness=9)
    assert not routed and len(pictures) == 2 and all(isinstance(p, PIL.Image.Image) for p in pictures)
    assert isinstance(gw.render_image(0, key, 0.1, thickness=9), PIL.Image.Image) and not routed
    gw.render_image_batch([0, 1], key, 0.1, thickness=8)
    assert [c['images'] for c in routed] == [2]
    # the flag off: nothing reaches render_bytes
    del routed[:]
    gw.device_render = False
    gw.render_image_batch([0, 1], key, 0.1)
    gw.render_image(0)
    assert not routed


def test_a_model_on_the_cpu_renders_on_the_host(monkeypatch):
    from rewriting_amd import hip

    def never(*a, **k):
        raise AssertionError('render_bytes was called for a model that is not on the device')
    monkeypatch.setattr(hip, 'render_bytes', never, raising=False)
    from rewriting_amd import synthetic
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import proggan, zdataset
    model = proggan.ProgressiveGenerator(resolution=32)
    synthetic.randomize_(model, seed=0, kind='proggan')
    model.eval()
    gw = ganrewrite.ProgressiveGanRewriter(model, zdataset.z_dataset_for_model(model, size=4), 4, device_render=True)
    assert gw.device_render and not gw._kernels()
    key = torch.randn(gw.k_shape[1])
    assert len(gw.render_image_batch([0, 1, 2, 3], key, 0.1)) == 4
    assert isinstance(gw.render_image(1), PIL.Image.Image)
