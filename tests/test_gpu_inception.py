"""The Inception-v3 pool3 features on the device (rw_inception.hip, rewriting_amd/inception.py) against float64 on the CPU.

The bar of every comparison is MARGIN = 8 times the error of the float32 CPU result on the same input;
a max pooling does no arithmetic and must equal torch bit for bit.  The measured ratios go to inception_accuracy.json in the
directory RW_REPORT_DIR names (default: test_reports/, which git ignores); profiles/inception_accuracy.json is a copy."""
import numpy
import pytest
import torch
import torch.nn.functional as F

from rewriting_amd import hip, inception, samples
from tests import inception_checks as K
from tests import perceptual_checks as P

pytestmark = pytest.mark.gpu
MARGIN = K.MARGIN
SENTINEL = -123456.78125                # exact in float32
REPORT = 'inception_accuracy.json'


def held(name, got, want64, ref32, figures=None):
    """asserts d_hip <= MARGIN d_ref and records both"""
    d_hip, d_ref = K.rel(got, want64), K.rel(ref32, want64)
    row = dict(d_hip=d_hip, d_ref=d_ref, ratio=(d_hip / d_ref if d_ref else (0.0 if d_hip == 0 else float('inf'))))
    print(name, row)
    if figures is not None:
        figures[name] = row
    assert d_hip <= MARGIN * d_ref, (name, d_hip, d_ref)
    return row


# (in_ch, out_ch, kernel, stride, padding, (h, w)): the smallest shapes at which each path of the kernel can go wrong
CONV_CASES = [
    (3, 32, (3, 3), 2, (0, 0), (9, 11)),            # K = 27: no multiple of the chunk or of an MFMA's k
    (32, 32, (3, 3), 1, (0, 0), (5, 7)),
    (64, 80, (1, 1), 1, (0, 0), (7, 5)),
    (48, 64, (5, 5), 1, (2, 2), (7, 5)),
    (48, 64, (5, 5), 1, (2, 2), (3, 3)),            # the padding reaches past the map
    (128, 160, (1, 7), 1, (0, 3), (17, 17)),
    (128, 160, (1, 7), 1, (0, 3), (3, 5)),
    (128, 160, (7, 1), 1, (3, 0), (17, 17)),
    (128, 160, (7, 1), 1, (3, 0), (3, 5)),
    (384, 384, (1, 3), 1, (0, 1), (8, 8)),
    (384, 384, (3, 1), 1, (1, 0), (8, 8)),
    (448, 384, (3, 3), 1, (1, 1), (8, 8)),          # the longest K: 4032
    (288, 384, (3, 3), 2, (0, 0), (7, 7)),
    (288, 384, (3, 3), 2, (0, 0), (8, 8)),          # the last row and column of the input are unused
    (80, 192, (3, 3), 1, (0, 0), (3, 3)),           # one output position
    # the threshold between the two tile forms, 256 workgroups of 128 positions (all cases above take the narrow form):
    (3, 32, (3, 3), 2, (0, 0), (211, 211)),         # batch 3: 33 075 positions, 259 workgroups, the wide form, ragged end
    (3, 32, (3, 3), 2, (0, 0), (209, 209)),         # batch 3: 32 448 positions, 254 workgroups, the narrow form
    (64, 80, (1, 1), 1, (0, 0), (75, 73)),          # batch 3: 129 x 2 workgroups, the wide form with a ragged out_ch tile
]


def _conv_id(case):
    i, o, k, s, p, hw = case
    return '%dto%d_k%dx%d_s%d_p%d%d_%dx%d' % (i, o, k[0], k[1], s, p[0], p[1], hw[0], hw[1])


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('case', CONV_CASES, ids=_conv_id)
def test_conv2d_against_float64(case, batch):
    i, o, k, s, p, (h, w) = case
    gen = torch.Generator().manual_seed(1000 * i + 10 * o + h + batch)
    x = torch.randn(batch, i, h, w, generator=gen)
    weight = torch.randn(o, i, *k, generator=gen) * (2.0 / (i * k[0] * k[1])) ** 0.5
    bias = 0.1 * torch.randn(o, generator=gen)
    want64 = F.conv2d(x.double(), weight.double(), bias.double(), s, p)
    ref32 = F.conv2d(x, weight, bias, s, p)
    xd, bd = x.cuda(), bias.cuda()
    wp = hip.conv2d_pack_weight(weight.cuda())
    figures = {}
    for relu in (False, True):
        act = F.relu if relu else (lambda t: t)
        got = hip.conv2d(xd, wp, weight.shape, bd, stride=s, padding=p, relu=relu)
        assert got.shape == want64.shape and got.dtype == torch.float32
        held('relu' if relu else 'plain', got, act(want64), act(ref32), figures)
        # the slice form, and a second run: the same bits, the other channels untouched
        wide = torch.full((batch, o + 12) + tuple(got.shape[2:]), SENTINEL, device='cuda')
        assert hip.conv2d(xd, wp, weight.shape, bd, stride=s, padding=p, relu=relu, out=wide, c_off=5) is wide
        assert torch.equal(wide[:, 5:5 + o], got)
        rest = torch.cat([wide[:, :5], wide[:, 5 + o:]], 1)
        assert torch.equal(rest, torch.full_like(rest, SENTINEL))
    # no bias
    got = hip.conv2d(xd, wp, weight.shape, None, stride=s, padding=p)
    held('no_bias', got, F.conv2d(x.double(), weight.double(), None, s, p), F.conv2d(x, weight, None, s, p), figures)
    P.report(REPORT, 'conv2d_%s_b%d' % (_conv_id(case), batch), figures)


def test_conv2d_tile_forms_give_the_same_bits():
    """an image's result does not depend on the batch it came in: batch 3 takes the wide tiles, batch 1 the narrow ones"""
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(3, 64, 75, 73, generator=gen).cuda()
    weight = (torch.randn(80, 64, 1, 1, generator=gen) / 8).cuda()
    wp = hip.conv2d_pack_weight(weight)
    whole = hip.conv2d(x, wp, weight.shape, relu=True)
    for b in range(3):
        assert torch.equal(whole[b:b + 1], hip.conv2d(x[b:b + 1].contiguous(), wp, weight.shape, relu=True))


def test_conv2d_refusals_on_the_device():
    x = torch.zeros(1, 4, 8, 8, device='cuda')
    wp = hip.conv2d_pack_weight(torch.zeros(6, 4, 3, 3, device='cuda'))
    with pytest.raises(ValueError, match='channels'):
        hip.conv2d(torch.zeros(1, 5, 8, 8, device='cuda'), wp, (6, 4, 3, 3))
    with pytest.raises(ValueError, match='packed weight'):
        hip.conv2d(x, wp[:-64], (6, 4, 3, 3))
    with pytest.raises(ValueError, match='c_off'):
        hip.conv2d(x, wp, (6, 4, 3, 3), out=torch.zeros(1, 8, 6, 6, device='cuda'), c_off=3)
    with pytest.raises(ValueError, match='out must be'):
        hip.conv2d(x, wp, (6, 4, 3, 3), out=torch.zeros(1, 8, 8, 8, device='cuda'))
    with pytest.raises(ValueError, match='7 x 7'):
        hip.conv2d_pack_weight(torch.zeros(2, 2, 9, 1, device='cuda'))
    # the entry itself refuses before any launch
    lib, null = hip.lib(), None
    args = (x.data_ptr(), wp.data_ptr(), null, x.data_ptr(), 1, 4, 8, 8, 6)
    assert lib.rw_conv2d_f32(*args, 3, 3, 3, 0, 0, 0, 0, 6, null) == 10002          # stride 3
    assert lib.rw_conv2d_f32(*args, 3, 3, 1, 3, 0, 0, 0, 6, null) == 10002          # padding >= kernel
    assert lib.rw_conv2d_f32(*args, 8, 3, 1, 0, 0, 0, 0, 6, null) == 10002          # kernel > 7
    assert lib.rw_conv2d_f32(*args, 3, 3, 1, 0, 0, 0, 1, 6, null) == 10001          # the slice leaves the output
    assert lib.rw_pool3x3_f32(x.data_ptr(), x.data_ptr(), 1, 4, 2, 8, 0, 0, 4, null) == 10002
    assert lib.rw_pool3x3_f32(x.data_ptr(), x.data_ptr(), 1, 4, 8, 8, 3, 0, 4, null) == 10001
    torch.cuda.synchronize()


@pytest.mark.parametrize('ch', [5, 288])
@pytest.mark.parametrize('size', [(7, 7), (8, 8), (3, 3)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('mode', ['max_s2', 'avg', 'max_s1'])
def test_pool3x3(mode, size, ch):
    gen = torch.Generator().manual_seed(ch + size[0])
    x = -(torch.rand(2, ch, *size, generator=gen) + 0.1)           # all negative: a padded zero would win every edge maximum
    xd = x.cuda()

    def torch_pool(t):
        if mode == 'max_s2':
            return F.max_pool2d(t, 3, 2)
        if mode == 'max_s1':
            return F.max_pool2d(t, 3, 1, 1)
        return F.avg_pool2d(t, 3, 1, 1, count_include_pad=False)
    got = hip.pool3x3(xd, mode)
    if mode == 'avg':
        row = held('avg', got, torch_pool(x.double()), torch_pool(x))
        P.report(REPORT, 'pool3x3_avg_%dx%d_c%d' % (size + (ch,)), row)
        # corners over 4 taps, edges over 6: a map of -1 stays -1 exactly
        ones = hip.pool3x3(torch.full_like(xd, -1.0), 'avg')
        assert torch.equal(ones, torch.full_like(ones, -1.0))
    else:
        assert torch.equal(got.cpu(), torch_pool(x))
        assert bool((got < 0).all())
    assert torch.equal(got, hip.pool3x3(xd, hip.POOL_MODES[mode]))
    wide = torch.full((2, ch + 9) + tuple(got.shape[2:]), SENTINEL, device='cuda')
    assert hip.pool3x3(xd, mode, out=wide, c_off=5) is wide
    assert torch.equal(wide[:, 5:5 + ch], got)
    rest = torch.cat([wide[:, :5], wide[:, 5 + ch:]], 1)
    assert torch.equal(rest, torch.full_like(rest, SENTINEL))


@pytest.mark.parametrize('size', [(1, 1), (8, 8), (3, 5)], ids=lambda s: '%dx%d' % s)
def test_global_avgpool(size):
    gen = torch.Generator().manual_seed(size[1])
    x = torch.randn(3, 2048, *size, generator=gen).relu()
    got = hip.global_avgpool(x.cuda())
    assert got.shape == (3, 2048)
    row = held('mean', got, x.double().mean((2, 3)), x.mean((2, 3)))
    P.report(REPORT, 'global_avgpool_%dx%d' % size, row)
    assert torch.equal(got, hip.global_avgpool(x.cuda()))


def test_inception_input():
    gen = torch.Generator().manual_seed(11)
    figures = {}
    for name, shape in (('up_64', (2, 3, 64, 64)), ('down_1024x512', (1, 3, 1024, 512))):
        x = 1.5 * torch.randn(shape, generator=gen)              # a third of it outside [-1, 1]: clamped first
        assert bool((x.abs() > 1).any())
        c = x.clamp(-1, 1)
        want64 = F.interpolate(c.double(), size=(299, 299), mode='bilinear', align_corners=False)
        ref32 = F.interpolate(c, size=(299, 299), mode='bilinear', align_corners=False)
        got = hip.inception_input(x.cuda())
        assert got.shape == (shape[0], 3, 299, 299) and bool((got.abs() <= 1).all())
        held(name, got, want64, ref32, figures)
        assert torch.equal(got, hip.inception_input(x.cuda()))
    P.report(REPORT, 'inception_input', figures)
    # 299 x 299 passes through with the same bits; so does any size with size=None
    x = K.images((2, 3, 299, 299), 12)
    assert torch.equal(hip.inception_input(x.cuda()).cpu(), x)
    x = 2 * K.images((1, 3, 75, 91), 13)
    assert torch.equal(hip.inception_input(x.cuda(), size=None).cpu(), x.clamp(-1, 1))
    # bytes (B, H, W, 3) equal the float route on x / 127.5 - 1 (divided on the host: a true division)
    raw = torch.randint(0, 256, (2, 50, 70, 3), generator=gen, dtype=torch.uint8)
    raw[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    as_float = (raw.permute(0, 3, 1, 2).float() / 127.5 - 1).contiguous()
    for size in (299, None, (80, 61)):
        assert torch.equal(hip.inception_input(raw.cuda(), size=size), hip.inception_input(as_float.cuda(), size=size))
    assert torch.equal(hip.inception_input(raw.cuda(), size=None).cpu(), as_float)


@pytest.fixture(scope='module')
def device_net():
    _, sd, _ = K.shared_twin()
    return inception.from_state_dict(sd).cuda()


@pytest.mark.parametrize('shape', [(2, 3, 75, 75), (1, 3, 107, 91)], ids=lambda s: '%dx%dx%d' % (s[0], s[2], s[3]))
def test_network_against_the_float64_twin(device_net, shape):
    twin32, _, twin64 = K.shared_twin()
    x = K.images(shape, shape[2])
    want64, ref32 = twin64(x.double()), twin32(x)
    assert torch.isfinite(want64).all() and (want64 != 0).double().mean().item() >= 0.4
    got = device_net(x.cuda(), resize=False)
    assert got.shape == (shape[0], inception.FEATURES) and got.dtype == torch.float32 and got.is_cuda
    row = held('features', got, want64, ref32)
    P.report(REPORT, 'network_%dx%dx%d' % (shape[0], shape[2], shape[3]), row)
    assert torch.equal(got, device_net(x.cuda(), resize=False))
    # the byte form of the same call
    raw = torch.randint(0, 256, (shape[0], shape[2], shape[3], 3), generator=torch.Generator().manual_seed(2),
                        dtype=torch.uint8)
    as_float = (raw.permute(0, 3, 1, 2).float() / 127.5 - 1).contiguous()
    assert torch.equal(device_net(raw.cuda(), resize=False), device_net(as_float.cuda(), resize=False))


def test_network_with_resize(device_net):
    twin32, _, twin64 = K.shared_twin()
    x = K.images((1, 3, 64, 64), 64)
    up64 = F.interpolate(x.double(), size=(299, 299), mode='bilinear', align_corners=False)
    up32 = F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False)
    got = device_net(x.cuda())
    row = held('features', got, twin64(up64), twin32(up32))
    P.report(REPORT, 'network_resize_1x64x64', row)


def test_network_refuses_a_live_parameter(device_net):
    p = device_net.Mixed_6a.branch3x3.bias
    p.requires_grad_(True)
    try:
        with pytest.raises(RuntimeError, match='Mixed_6a.branch3x3.bias'):
            device_net(torch.zeros(1, 3, 75, 75, device='cuda'), resize=False)
    finally:
        p.requires_grad_(False)


def test_routes(device_net):
    batches = [K.images((2, 3, 75, 75), seed).cuda() for seed in (21, 22, 23)]
    stats = samples.activation_statistics(batches, lambda im: device_net(im, resize=False))
    by_hand, fp32_block = samples.FeatureStatistics(exact=True), samples.FeatureStatistics()
    for b in batches:
        by_hand.add(device_net(b, resize=False))
        fp32_block.add(device_net(b, resize=False))
    assert stats.count == by_hand.count == 6 and stats.sum.is_cuda and stats.outer.shape == (2048, 2048)
    assert torch.equal(stats.sum, by_hand.sum) and torch.equal(stats.outer, by_hand.outer)
    assert torch.equal(stats.outer, stats.outer.t())
    # the default route of FeatureStatistics rounds each batch's products to float32: the same sums to 2^-24 of the largest
    assert torch.equal(fp32_block.sum, stats.sum)
    assert (fp32_block.outer - stats.outer).abs().max().item() <= 3 * 2.0 ** -23 * stats.outer.abs().max().item()
    feats = torch.cat([device_net(b, resize=False) for b in batches]).double().cpu().numpy()
    mu, sigma = stats.mean_cov()
    numpy.testing.assert_allclose(mu, feats.mean(0), rtol=1e-12, atol=1e-14)
    numpy.testing.assert_allclose(sigma, numpy.cov(feats, rowvar=False), rtol=1e-9, atol=1e-12)
    # a set against itself: six samples of 2048 features, a degenerate covariance (section 8.10's tested case)
    d = samples.fid(stats, stats)
    trace = stats.mean_cov(device=True)[1].diagonal().sum().item()
    print(dict(fid_self=d, trace=trace))
    assert trace > 0 and abs(d) <= 1e-6 * trace
