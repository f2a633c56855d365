"""The face parser on the device (rw_faceparse.hip, the residual form of rw_conv2d_f32, rewriting_amd/faceparse.py, the routes
of rewriting_amd/distances.py) against float64 on the CPU.

Arithmetic is held to MARGIN = 8 times the error of the float32 CPU result on the same input; what does
no arithmetic -- the max pooling, a pure gather, a map of the output's size, the arg-max of the entry's own samples, the
integer counts -- must be equal.  Labels of the whole network follow the label rule of tests/faceparse_checks.py.  The
measured ratios go to faceparse_accuracy.json in the directory RW_REPORT_DIR names (default: test_reports/, which git
ignores); profiles/faceparse_accuracy.json is a copy."""
import os

import numpy
import pytest
import torch
import torch.nn.functional as F

from rewriting_amd import distances, faceparse, hip
from tests import faceparse_checks as K
from tests import perceptual_checks as P
from tests.test_gpu_inception import held

pytestmark = pytest.mark.gpu
REPORT = 'faceparse_accuracy.json'


def _operands(i, o, k, h, w, batch, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, i, h, w, generator=gen)
    weight = torch.randn(o, i, k, k, generator=gen) * (2.0 / (i * k * k)) ** 0.5
    return x, weight, 0.1 * torch.randn(o, generator=gen), gen


# (in_ch, out_ch, kernel, stride, padding, (h, w))
ADD_CASES = [
    (64, 64, 3, 1, 1, (5, 7)),
    (64, 128, 3, 2, 1, (8, 8)),
    (64, 128, 3, 2, 1, (7, 7)),
    (512, 512, 3, 1, 1, (1, 1)),            # the padding reaches past the map; K = 4608, the longest
    (512, 512, 3, 1, 1, (2, 2)),
    (256, 256, 3, 1, 1, (4, 4)),
]
# the shapes the plain convolution meets in this network for the first time
PLAIN_CASES = [
    (3, 64, 7, 2, 3, (9, 11)),
    (64, 128, 1, 2, 0, (8, 8)),
    (64, 128, 1, 2, 0, (7, 7)),
    (512, 128, 1, 1, 0, (1, 1)),
    (256, 19, 1, 1, 0, (4, 4)),
]


def _case_id(case):
    i, o, k, s, p, (h, w) = case
    return '%dto%d_k%d_s%d_p%d_%dx%d' % (i, o, k, s, p, h, w)


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('case', ADD_CASES, ids=_case_id)
def test_conv2d_add_against_float64(case, batch):
    i, o, k, s, p, (h, w) = case
    x, weight, bias, gen = _operands(i, o, k, h, w, batch, 1000 * i + 10 * o + h + batch)
    conv64 = F.conv2d(x.double(), weight.double(), bias.double(), s, p)
    res = torch.randn(conv64.shape, generator=gen)
    want64, ref32 = conv64 + res.double(), F.conv2d(x, weight, bias, s, p) + res
    xd, bd, rd = x.cuda(), bias.cuda(), res.cuda()
    wp = hip.conv2d_pack_weight(weight.cuda())
    figures = {}
    for relu in (False, True):
        act = F.relu if relu else (lambda t: t)
        got = hip.conv2d_add(xd, wp, weight.shape, bd, rd, stride=s, padding=p, relu=relu)
        assert got.shape == want64.shape and got.dtype == torch.float32 and torch.equal(rd.cpu(), res)
        held('relu' if relu else 'plain', got, act(want64), act(ref32), figures)
        assert torch.equal(got, hip.conv2d_add(xd, wp, weight.shape, bd, rd, stride=s, padding=p, relu=relu))
        # in place: y is res
        over = rd.clone()
        assert hip.conv2d_add(xd, wp, weight.shape, bd, over, stride=s, padding=p, relu=relu, out=over) is over
        assert torch.equal(over, got)
    # the sum is (conv + bias) + res: the plain convolution's bits, then one more rounding
    plain = hip.conv2d(xd, wp, weight.shape, bd, stride=s, padding=p)
    assert torch.equal(hip.conv2d_add(xd, wp, weight.shape, bd, rd, stride=s, padding=p), plain + rd)
    P.report(REPORT, 'conv2d_add_%s_b%d' % (_case_id(case), batch), figures)


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('case', PLAIN_CASES, ids=_case_id)
def test_conv2d_at_the_networks_new_shapes(case, batch):
    i, o, k, s, p, (h, w) = case
    x, weight, bias, _ = _operands(i, o, k, h, w, batch, 77 * i + o + w + batch)
    wp = hip.conv2d_pack_weight(weight.cuda())
    figures = {}
    for relu in (False, True):
        act = F.relu if relu else (lambda t: t)
        got = hip.conv2d(x.cuda(), wp, weight.shape, bias.cuda(), stride=s, padding=p, relu=relu)
        held('relu' if relu else 'plain', got, act(F.conv2d(x.double(), weight.double(), bias.double(), s, p)),
             act(F.conv2d(x, weight, bias, s, p)), figures)
    P.report(REPORT, 'conv2d_%s_b%d' % (_case_id(case), batch), figures)


def test_conv2d_add_tile_forms_give_the_same_bits():
    """64 -> 64, 3 x 3 at 128 x 128: batch 2 is 32 768 positions, 256 workgroups of 128, the wide form; batch 1 the narrow"""
    x, weight, bias, gen = _operands(64, 64, 3, 128, 128, 2, 5)
    res = torch.randn(2, 64, 128, 128, generator=gen).cuda()
    x, bias = x.cuda(), bias.cuda()
    wp = hip.conv2d_pack_weight(weight.cuda())
    whole = hip.conv2d_add(x, wp, weight.shape, bias, res, padding=1, relu=True)
    for b in range(2):
        one = hip.conv2d_add(x[b:b + 1].contiguous(), wp, weight.shape, bias, res[b:b + 1].contiguous(), padding=1, relu=True)
        assert torch.equal(whole[b:b + 1], one)
    want = F.relu(F.conv2d(x.cpu().double(), weight.double(), bias.cpu().double(), 1, 1) + res.cpu().double())
    held('tile_forms', whole, want, F.relu(F.conv2d(x.cpu(), weight, bias.cpu(), 1, 1) + res.cpu()))


def test_conv2d_add_refusals_on_the_device():
    x = torch.zeros(1, 4, 8, 8, device='cuda')
    wp = hip.conv2d_pack_weight(torch.zeros(6, 4, 3, 3, device='cuda'))
    with pytest.raises(ValueError, match='res must be'):
        hip.conv2d_add(x, wp, (6, 4, 3, 3), None, torch.zeros(1, 6, 8, 8, device='cuda'))
    with pytest.raises(ValueError, match='out must be'):
        hip.conv2d_add(x, wp, (6, 4, 3, 3), None, torch.zeros(1, 6, 6, 6, device='cuda'), out=torch.zeros(1, 6, 8, 8, device='cuda'))
    with pytest.raises(TypeError):
        hip.conv2d_add(x, wp, (6, 4, 3, 3), None, None)
    args = (x.data_ptr(), wp.data_ptr(), None, None, x.data_ptr(), 1, 4, 8, 8, 6, 3, 3, 1, 0, 0, 0, None)
    assert hip.lib().rw_conv2d_add_f32(*args) == 10001                           # a null res


@pytest.mark.parametrize('size', [(1, 1), (2, 2), (3, 5), (7, 7), (8, 8)])
@pytest.mark.parametrize('ch', [5, 64])
def test_maxpool_equals_torch(size, ch):
    gen = torch.Generator().manual_seed(ch + size[0])
    x = torch.randn(2, ch, *size, generator=gen)
    for maps in (x, -x.abs() - 1):                                               # all negative: a padded tap is no zero
        got = hip.maxpool3x3s2p1(maps.cuda())
        assert torch.equal(got.cpu(), F.max_pool2d(maps, 3, 2, 1))


def _tables(h, w, oh, ow):
    return faceparse.device_nearest_table(h, oh, 'cuda'), faceparse.device_nearest_table(w, ow, 'cuda')


@pytest.mark.parametrize('sizes', [((3, 2), (5, 3)), ((2, 2), (3, 3)), ((5, 3), (9, 5)), ((4, 4), (8, 8)), ((8, 8), (4, 4)),
                                   ((45, 37), (64, 64)), ((6, 8), (6, 8)), ((6, 8), (9, 8))])
def test_gate_resample_as_a_gather_equals_interpolate(sizes):
    (h, w), (oh, ow) = sizes
    x = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(h * w))
    rows, cols = _tables(h, w, oh, ow)
    assert (rows is None) == (h == oh) and (cols is None) == (w == ow)
    got = hip.gate_resample(x.cuda(), rows=rows, cols=cols)
    assert torch.equal(got.cpu(), F.interpolate(x, size=(oh, ow)))


# (h, w) -> (oh, ow), the add: every use the network makes of the kernel
GATE_CASES = [((1, 1), (2, 2), 'vec'), ((3, 2), (5, 3), 'vec'), ((4, 4), (4, 4), 'map'), ((2, 3), (4, 5), 'map'),
              ((4, 8), (7, 8), 'map'), ((5, 3), (5, 3), 'self'), ((6, 8), (6, 8), 'self'), ((3, 4), (3, 4), None)]


@pytest.mark.parametrize('case', GATE_CASES, ids=lambda c: '%dx%d_%dx%d_%s' % (c[0] + c[1] + (c[2],)))
def test_gate_resample_against_float64(case):
    (h, w), (oh, ow), add = case
    gen = torch.Generator().manual_seed(h + 10 * w + oh)
    x, gate = torch.randn(3, 5, h, w, generator=gen), 2 * torch.randn(3, 5, generator=gen)
    add_map = torch.randn(3, 5, h, w, generator=gen) if add == 'map' else None
    add_vec = torch.randn(3, 5, 1, 1, generator=gen) if add == 'vec' else None
    rows, cols = _tables(h, w, oh, ow)
    cpu = dict(rows=None if rows is None else rows.cpu(), cols=None if cols is None else cols.cpu())

    def twin(cast):
        opt = lambda t: None if t is None else cast(t)               # noqa: E731
        return K.gate_resample(cast(x), cast(gate), cast(x) if add == 'self' else opt(add_map), opt(add_vec), **cpu)
    xd = x.cuda()
    got = hip.gate_resample(xd, gate.cuda(), xd if add == 'self' else (None if add_map is None else add_map.cuda()),
                            None if add_vec is None else add_vec.cuda(), rows, cols)
    assert got.shape == (3, 5, oh, ow)
    row = held('gate', got, twin(torch.Tensor.double), twin(lambda t: t))
    assert torch.equal(got, hip.gate_resample(xd, gate.cuda(), xd if add == 'self' else (None if add_map is None else add_map.cuda()),
                                              None if add_vec is None else add_vec.cuda(), rows, cols))
    P.report(REPORT, 'gate_resample_%dx%d_%dx%d_%s' % (h, w, oh, ow, add), row)


def test_gate_resample_saturated_gates_and_refusals():
    ones = torch.ones(1, 4, 3, 4, device='cuda')
    gate = torch.tensor([[100.0, -100.0, 0.0, 20.0]], device='cuda')
    s = hip.gate_resample(ones, gate=gate)
    assert torch.isfinite(s).all() and (s >= 0).all() and (s <= 1).all()
    assert (s[0, 0] == 1).all() and (s[0, 1] == 0).all() and (s[0, 2] == 0.5).all()
    with pytest.raises(ValueError, match='exclude'):
        hip.gate_resample(ones, add_map=ones, add_vec=gate)
    with pytest.raises(ValueError, match='gate must be'):
        hip.gate_resample(ones, gate=gate[:, :3])
    with pytest.raises(ValueError, match='add_map must be'):
        hip.gate_resample(ones, add_map=ones[:, :, :2].contiguous())
    with pytest.raises(RuntimeError, match='nothing is converted'):
        hip.gate_resample(ones, rows=torch.zeros(3, device='cuda', dtype=torch.int64))
    null, p = None, ones.data_ptr()
    lib = hip.lib()
    assert lib.rw_gate_resample_f32(p, null, null, null, null, null, p, 1, 4, 3, 4, 5, 4, null) == 10001      # no rows, 3 -> 5
    assert lib.rw_gate_resample_f32(p, null, p, p, null, null, p, 1, 4, 3, 4, 3, 4, null) == 10001            # both adds


def test_gate_resample_clamps_a_wrong_table():
    """entries outside the map change values only: they are clamped into it"""
    x = torch.randn(2, 3, 4, 8, generator=torch.Generator().manual_seed(3)).cuda()
    rows = torch.tensor([0, -5, 2, 99, 3], dtype=torch.int32, device='cuda')
    cols = torch.tensor([7, 8, -1, 0, 1 << 30, 3], dtype=torch.int32, device='cuda')
    for r, c in ((rows, cols), (rows, None)):                                    # scalar and 16-byte forms
        got = hip.gate_resample(x, rows=r, cols=c)
        want = K.gate_resample(x, rows=r.clamp(0, 3), cols=None if c is None else c.clamp(0, 7))
        assert torch.equal(got, want)


AC_CASES = [((1, 1), (4, 4)), ((2, 2), (5, 7)), ((4, 4), (32, 32)), ((9, 5), (72, 40))]


@pytest.mark.parametrize('sizes', AC_CASES, ids=lambda s: '%dx%d_%dx%d' % (s[0] + s[1]))
def test_bilinear_ac_against_float64(sizes):
    (h, w), size = sizes
    x = torch.randn(2, 5, h, w, generator=torch.Generator().manual_seed(h + w))
    tables = faceparse.device_ac_tables((h, w), size, 'cuda')
    got = hip.bilinear_ac(x.cuda(), size, *tables)
    row = held('bilinear', got, F.interpolate(x.double(), size, mode='bilinear', align_corners=True),
               F.interpolate(x, size, mode='bilinear', align_corners=True))
    assert torch.equal(got, hip.bilinear_ac(x.cuda(), size, *tables))
    P.report(REPORT, 'bilinear_ac_%dx%d_%dx%d' % ((h, w) + size), row)
    # a map of the output's size passes through
    big = torch.randn(1, 3, *size, generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(hip.bilinear_ac(big, size, *faceparse.device_ac_tables(size, size, 'cuda')), big)
    with pytest.raises(ValueError, match='device_ac_tables'):
        hip.bilinear_ac(x.cuda(), (size[0] + 1, size[1]), *tables)


@pytest.mark.parametrize('n', [1, 19, 64])
@pytest.mark.parametrize('sizes', AC_CASES, ids=lambda s: '%dx%d_%dx%d' % (s[0] + s[1]))
def test_seg_labels_equal_the_argmax_of_bilinear_ac(sizes, n):
    (h, w), size = sizes
    logits = torch.randn(2, n, h, w, generator=torch.Generator().manual_seed(n + h)).cuda()
    tables = faceparse.device_ac_tables((h, w), size, 'cuda')
    want = numpy.argmax(hip.bilinear_ac(logits, size, *tables).cpu().numpy(), axis=1)[:, None]
    got = hip.seg_labels(logits, size, *tables)
    assert got.dtype == torch.int64 and got.shape == (2, 1) + size
    assert numpy.array_equal(got.cpu().numpy(), want)
    assert n == 1 or len(numpy.unique(want)) > 1 or h * w == 1
    if size == (32, 32):
        for out in (45, 20):                                                     # read through the labels' resize
            rows = faceparse.device_nearest_table(32, out, 'cuda')
            picked = hip.seg_labels(logits, size, *tables, pick_rows=rows, pick_cols=rows)
            index = faceparse.nearest_table(32, out).astype('int64')
            assert numpy.array_equal(picked.cpu().numpy(), want[:, :, index][:, :, :, index])
            tall = hip.seg_labels(logits, size, *tables, pick_rows=rows)
            assert numpy.array_equal(tall.cpu().numpy(), want[:, :, index])


def test_seg_labels_ties_nans_and_refusals():
    size = (5, 7)
    tables = faceparse.device_ac_tables((2, 2), size, 'cuda')
    flat = torch.full((1, 19, 2, 2), 0.25, device='cuda')
    assert not hip.seg_labels(flat, size, *tables).any()                         # constant across the classes: class 0
    tied = torch.randn(1, 19, 2, 2, generator=torch.Generator().manual_seed(2)).cuda()
    tied[:, 7] = tied[:, 3] = tied.amax(1) + 1
    assert (hip.seg_labels(tied, size, *tables) == 3).all()                      # the lower of two that tie
    nan = tied.clone()
    nan[:, 11] = nan[:, 5] = float('nan')
    got = hip.seg_labels(nan, size, *tables)
    assert (got == 5).all()                                                      # a NaN wins, the first one first
    assert numpy.array_equal(got.cpu().numpy(), numpy.argmax(hip.bilinear_ac(nan, size, *tables).cpu().numpy(), axis=1)[:, None])
    with pytest.raises(ValueError, match='at most 64'):
        hip.seg_labels(torch.zeros(1, 65, 2, 2, device='cuda'), size, *tables)
    p = flat.data_ptr()
    assert hip.lib().rw_seg_labels_i64(p, p, 1, 65, 2, 2, 5, 7, p, p, None, None, 5, 7, None) == 10002


@pytest.mark.parametrize('size', [(1, 1), (7, 9), (65, 64)])
def test_seg_correct_counts_equal_the_formula(size):
    gen = torch.Generator().manual_seed(size[0])
    before = torch.randint(0, 21, (3, 3) + size, generator=gen)
    after = torch.randint(0, 21, (3, 3) + size, generator=gen)
    bd, ad = before.cuda(), after.cuda()
    sets = [((4,), (9,)), ((1, 7, 20), (0, 3, 5)), (tuple(range(16)), tuple(range(5, 21))), ((33,), (1,)), ((2, 2), (1, 1))]
    for src, tgt in sets:
        for srcc, tgtc in ((0, 0), (2, 0), (1, 2)):
            got = hip.seg_correct_counts(bd, ad, src, tgt, srcc, tgtc)
            assert got.dtype == torch.int64 and torch.equal(got.cpu(), K.correct_counts(before, after, src, tgt, srcc, tgtc))
        plain = hip.seg_correct_counts(bd[:, 1].contiguous(), ad[:, 0].contiguous(), src, tgt)          # the (B, H, W) form
        assert torch.equal(plain.cpu(), K.correct_counts(before, after, src, tgt, 1, 0))
        want = K.correct_counts(before, after, src, tgt, 2, 0).sum(0).tolist()
        assert distances.correct_modification(bd, ad, src, tgt, srcc=2, tgtc=0) == (want[0], want[1])
    assert hip.seg_correct_counts(bd, ad, (33,), (1,)).tolist() == [[0, 0]] * 3                         # nothing matches
    with pytest.raises(ValueError, match='channel'):
        hip.seg_correct_counts(bd, ad, (1,), (1,), srcc=3)
    with pytest.raises(ValueError, match='agree'):
        hip.seg_correct_counts(bd, ad[:2].contiguous(), (1,), (1,))
    with pytest.raises(RuntimeError, match='nothing is converted'):
        hip.seg_correct_counts(bd.int(), ad, (1,), (1,))


# ---- the network ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def net():
    _, sd, _ = K.shared_twin()
    return faceparse.from_state_dict(sd).cuda()


@pytest.mark.parametrize('shape,seed', [((2, 3, 32, 32), 11), ((1, 3, 72, 40), 12), ((1, 3, 64, 64), 14)],
                         ids=['2x32x32', '1x72x40', '1x64x64'])
def test_face_parser_by_the_label_rule(net, shape, seed):
    ref = K.reference(shape, seed)
    assert ref.is_decisive()
    x = K.images(shape, seed).cuda()
    scores = net(x)
    assert scores.shape == ref.scores64.shape and scores.dtype == torch.float32
    row = held('scores', scores, ref.scores64, ref.scores32)
    worst = (scores.cpu().double() - ref.scores64).abs().max().item()
    row.update(max_abs=worst, tau=ref.tau, undecided=ref.undecided.double().mean().item())
    print(row)
    P.report(REPORT, 'face_parser_%s' % 'x'.join(str(v) for v in shape), row)
    assert worst <= ref.tau
    labels = net.labels(x)
    K.assert_labels(labels, ref.labels, ref.undecided)
    # the labels are the arg-max of the scores the module itself returns, and a second run gives the same bits
    assert numpy.array_equal(labels.cpu().numpy(), numpy.argmax(scores.cpu().numpy(), axis=1)[:, None])
    assert torch.equal(net(x), scores) and torch.equal(net.labels(x), labels)


def test_segment_batch_by_the_label_rule(net):
    shape, seed, size = (2, 3, 45, 37), 13, (64, 64)
    ref = K.reference(shape, seed, size)
    assert ref.is_decisive()
    seg = faceparse.FaceSegmenter(net, size=size)
    x = K.images(shape, seed).cuda()
    got = seg.segment_batch(x)
    assert got.shape == (2, 1, 45, 37) and got.is_cuda
    K.assert_labels(got, *ref.resized((45, 37)))
    assert torch.equal(seg.segment_batch(x), got)
    # an image's labels do not depend on the batch it came in
    assert torch.equal(seg.segment_batch(x[1:].contiguous()), got[1:])
    # size=None parses at the images' own size
    own = K.reference(shape, seed)
    K.assert_labels(faceparse.FaceSegmenter(net, size=None).segment_batch(x), own.labels, own.undecided)


def test_segment_batch_at_the_default_working_size(net):
    shape, seed = (1, 3, 96, 80), 15
    ref = K.reference(shape, seed, faceparse.WORKING_SIZE)
    assert ref.is_decisive()
    got = faceparse.FaceSegmenter(net).segment_batch(K.images(shape, seed).cuda())
    K.assert_labels(got, *ref.resized((96, 80)))


def test_a_live_parameter_is_refused_by_name():
    _, sd, _ = K.shared_twin()
    live = faceparse.from_state_dict(sd).cuda()
    live.ffm_convblk.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='ffm_convblk.weight'):
        live(torch.zeros(1, 3, 32, 32, device='cuda'))
    with pytest.raises(RuntimeError, match='move the network'):
        faceparse.from_state_dict(sd)(torch.zeros(1, 3, 32, 32, device='cuda'))


# ---- the routes -----------------------------------------------------------------------------------------------------------

def test_compute_dl_with_a_segmenter_equals_the_pth_route(net, tmp_path):
    import PIL.Image
    seg = faceparse.FaceSegmenter(net, size=(64, 64))
    dirs = [str(tmp_path / name) for name in ('before', 'after', 'seg')]
    for d in dirs:
        os.makedirs(d)
    rng = numpy.random.RandomState(4)
    keys = [0, 1, 2, 3]
    for key in keys:
        for d in dirs[:2]:
            PIL.Image.fromarray(rng.randint(0, 256, (32, 32, 3)).astype(numpy.uint8)).save(os.path.join(d, '%d.png' % key))
    before = torch.stack([distances._load_image(os.path.join(dirs[0], '%d.png' % key)) for key in keys]).cuda()
    labels = seg.segment_batch(before)
    for key, one in zip(keys, labels.cpu()):
        torch.save(one, os.path.join(dirs[2], '%d.pth' % key))
    assert labels.unique().numel() >= 3
    common = [int(v) for v in labels.flatten().bincount().argsort(descending=True)[:2]]
    for src in (faceparse.SMILE_SRC, tuple(common)):
        kwargs = dict(src=src, srcc=0, mode='pixel', batch_size=4)
        want = distances.compute_dl(dirs[0], dirs[1], dirs[2], keys, **kwargs)
        got = distances.compute_dl(dirs[0], dirs[1], None, keys, segmenter=seg, **kwargs)
        assert isinstance(got[0], float) and isinstance(got[1], int) and got == want
    assert 0 < want[1] < 4 * 32 * 32                                             # the frequent labels mask something
    # the device-decoded route takes the segmenter too
    assert distances.compute_dl(dirs[0], dirs[1], None, keys, segmenter=seg, device_decode=True, **kwargs) == want
    # pixels correctly modified: a set against itself
    total, count = distances.correct_modification(labels, labels, common, common)
    assert total == count == int(sum((labels == v).sum() for v in common)) and count > 0
    assert distances.correct_modification(labels, labels, common[:1], common[1:]) == (0, int((labels == common[0]).sum()))
