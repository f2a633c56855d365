"""The host side of the face parser (rewriting_amd/faceparse.py, distances.correct_modification, compute_dl's segmenter
route): the twin's fitness for the label rule, the layout table, the loader's refusals, the two index tables, the module's
walk on CPU stand-ins, the checks made before any library call and the entries' refusals.  No GPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from rewriting_amd import _lib, distances, faceparse, hip, inception
from tests import faceparse_checks as K

SMALL_CASES = [((2, 3, 32, 32), 11), ((1, 3, 72, 40), 12)]


@pytest.mark.parametrize('shape,seed', SMALL_CASES)
def test_twin_is_alive_and_decisive(shape, seed):
    """the twin alone: finite scores, at most 1 % undecided pixels, at least 4 labels -- the label rule of the device tests
    cannot pass vacuously"""
    ref = K.reference(shape, seed)
    assert ref.scores64.shape == (shape[0], 19) + shape[2:] and torch.isfinite(ref.scores64).all()
    share, labels = ref.undecided.double().mean().item(), ref.labels.unique().numel()
    print('undecided share %.3g, %d labels, d_ref %.3g, tau %.3g' % (share, labels, ref.d_ref, ref.tau))
    assert share <= K.MAX_UNDECIDED and labels >= K.MIN_LABELS and ref.is_decisive()
    assert 0 < ref.d_ref < 1e-5
    # the float32 twin itself obeys the rule it is the yardstick of
    K.assert_labels(ref.scores32.argmax(1, keepdim=True), ref.labels, ref.undecided)


def test_layout_table_equals_the_twin():
    _, sd, _ = K.shared_twin()
    kept = {k: tuple(v.shape) for k, v in sd.items()
            if not k.startswith(('conv_out16.', 'conv_out32.')) and not k.endswith('num_batches_tracked')}
    assert faceparse.checkpoint_shapes(19) == kept
    layers = faceparse.conv_layers(19)
    assert len(layers) == 32 and len({op.name for op in layers}) == 32
    assert sum(1 for op in layers if op.bn) == 29
    assert [op.name for op in layers if not op.bn] == ['ffm.conv1', 'ffm.conv2', 'conv_out.conv_out']
    assert faceparse.conv_layers(7)[-1].out_ch == 7
    assert len(faceparse.ATTRIBUTES) == 18 and faceparse.SMILE_SRC == (12, 13, 11)
    assert [faceparse.ATTRIBUTES[i - 1] for i in faceparse.SMILE_SRC] == ['u_lip', 'l_lip', 'mouth']


def test_loader_accepts_the_twin_and_ignores_the_other_heads(tmp_path):
    _, sd, _ = K.shared_twin()
    assert any(k.startswith('conv_out16.') for k in sd) and any(k.startswith('conv_out32.') for k in sd)
    assert any(k.endswith('num_batches_tracked') for k in sd)
    net = faceparse.from_state_dict(sd)
    assert isinstance(net, faceparse.FaceParser) and not net.training and net.n_classes == 19
    assert not any(p.requires_grad for p in net.parameters())
    assert len(list(net.parameters())) == 2 * 32
    name = 'cp.resnet.layer3.0.downsample'
    w, b = inception.fold_batch_norm(sd[name + '.0.weight'], sd[name + '.1.weight'], sd[name + '.1.bias'],
                                     sd[name + '.1.running_mean'], sd[name + '.1.running_var'], eps=1e-5)
    mine = net.state_dict()
    assert torch.equal(mine['cp_resnet_layer3_0_downsample.weight'], w) and tuple(w.shape) == (256, 128, 1, 1)
    assert torch.equal(mine['cp_resnet_layer3_0_downsample.bias'], b)
    assert not torch.equal(w, inception.fold_batch_norm(sd[name + '.0.weight'], sd[name + '.1.weight'], sd[name + '.1.bias'],
                                                        sd[name + '.1.running_mean'], sd[name + '.1.running_var'])[0])
    assert torch.equal(mine['ffm_conv2.weight'], sd['ffm.conv2.weight'])            # no batch norm: as it is
    # a narrower head
    narrow = dict(sd)
    narrow['conv_out.conv_out.weight'] = sd['conv_out.conv_out.weight'][:5].clone()
    assert faceparse.from_state_dict(narrow).n_classes == 5
    # the file form, and the environment variable
    path = tmp_path / 'faceparse.pt'
    torch.save(sd, str(path))
    assert isinstance(faceparse.face_parser(str(path)), faceparse.FaceParser)


def test_default_weights(tmp_path, monkeypatch):
    monkeypatch.delenv(faceparse.WEIGHTS_ENV, raising=False)
    assert faceparse.WEIGHTS_ENV == 'RW_FACEPARSE_WEIGHTS' and faceparse.default_weights() is None
    path = tmp_path / 'w.pt'
    path.write_bytes(b'x')
    monkeypatch.setenv(faceparse.WEIGHTS_ENV, str(path))
    assert faceparse.default_weights() == str(path)
    monkeypatch.setenv(faceparse.WEIGHTS_ENV, str(tmp_path / 'none.pt'))
    assert faceparse.default_weights() is None


def test_loader_refusals_name_the_key():
    _, sd, _ = K.shared_twin()
    lacking = dict(sd)
    del lacking['cp.arm32.bn_atten.running_var']
    with pytest.raises(KeyError, match='cp.arm32.bn_atten.running_var'):
        faceparse.from_state_dict(lacking)
    headless = dict(sd)
    del headless['conv_out.conv_out.weight']
    with pytest.raises(KeyError, match='conv_out.conv_out.weight'):
        faceparse.from_state_dict(headless)
    wrong = dict(sd)
    wrong['cp.resnet.layer2.0.conv1.weight'] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(ValueError, match='cp.resnet.layer2.0.conv1.weight'):
        faceparse.from_state_dict(wrong)
    live = dict(sd)
    live['ffm.conv1.weight'] = sd['ffm.conv1.weight'].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match='ffm.conv1.weight'):
        faceparse.from_state_dict(live)
    stray = dict(sd)
    stray['sp.conv1.conv.weight'] = torch.zeros(1)
    with pytest.raises(KeyError, match='sp.conv1.conv.weight'):
        faceparse.from_state_dict(stray)


def test_nearest_table_equals_interpolate():
    pairs = [(i, o) for i in range(1, 41) for o in range(1, 81)] + [(178, 512), (218, 512), (512, 178), (512, 1024)]
    for n_in, n_out in pairs:
        table = faceparse.nearest_table(n_in, n_out)
        assert table.dtype.name == 'int32' and table.shape == (n_out,)
        want = F.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None], size=n_out)[0, 0]
        assert torch.equal(torch.from_numpy(table.copy()).float(), want), (n_in, n_out)


@pytest.mark.parametrize('n_in,n_out', [(1, 4), (2, 5), (4, 32), (9, 72), (64, 512)])
def test_align_corners_table_reproduces_interpolate(n_in, n_out):
    i0, i1, lam = faceparse.align_corners_table(n_in, n_out)
    assert i0.dtype.name == i1.dtype.name == 'int32' and i0.min() >= 0 and i1.max() <= n_in - 1
    assert ((lam >= 0) & (lam < 1)).all()
    ramp = torch.linspace(-1, 2, n_in, dtype=torch.float64) ** 2                 # no straight line: lam matters
    want = F.interpolate(ramp[None, None, None], size=(1, n_out), mode='bilinear', align_corners=True)[0, 0, 0]
    t0, t1, lm = (torch.from_numpy(a.astype('int64' if a.dtype.kind == 'i' else 'float64')) for a in (i0, i1, lam))
    got = (1 - lm) * ramp[t0] + lm * ramp[t1]
    assert (got - want).abs().max().item() <= 1e-6
    # the device form: rows then columns, lam rounded to float32
    idx, lam32 = faceparse.device_ac_tables((n_in, 3), (n_out, 2), 'cpu')
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (2 * n_out + 4,) and tuple(lam32.shape) == (n_out + 2,)
    assert torch.equal(idx[:n_out], torch.from_numpy(i0.copy())) and idx[2 * n_out:].tolist() == [0, 2, 1, 2]
    assert faceparse.device_ac_tables((n_in, 3), (n_out, 2), 'cpu')[0] is idx    # kept
    assert faceparse.device_nearest_table(7, 7, 'cpu') is None


@pytest.mark.parametrize('shape,seed', SMALL_CASES)
def test_emulated_walk_equals_the_twin(monkeypatch, shape, seed):
    """the walk, the slices and the uses of the tables, without a device"""
    K.emulate(monkeypatch)
    _, sd, _ = K.shared_twin()
    net = faceparse.from_state_dict(sd)
    ref = K.reference(shape, seed)
    x = K.images(shape, seed)
    scores = net(x)
    assert scores.shape == ref.scores32.shape
    d = K.rel(scores, ref.scores32)
    print('emulated walk against the float32 twin: %.3g' % d)
    assert d <= 1e-5
    K.assert_labels(net.labels(x), ref.labels, ref.undecided)


def test_emulated_segment_batch_equals_the_twins_pipeline(monkeypatch):
    K.emulate(monkeypatch)
    _, sd, _ = K.shared_twin()
    shape, seed, size = (2, 3, 45, 37), 13, (64, 64)
    ref = K.reference(shape, seed, size)
    assert ref.is_decisive()
    seg = faceparse.FaceSegmenter(faceparse.from_state_dict(sd), size=size)
    got = seg.segment_batch(K.images(shape, seed))
    assert got.shape == (2, 1, 45, 37)
    K.assert_labels(got, *ref.resized((45, 37)))
    # and the counts of the metric over them, by the stand-in formula
    assert distances.correct_modification(got, got, faceparse.SMILE_SRC, faceparse.SMILE_SRC)[0] == \
        int(sum((got == s).sum() for s in faceparse.SMILE_SRC))


def test_inputs_are_refused_before_any_library_call(monkeypatch, tmp_path):
    def no_library():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(hip, 'lib', no_library)
    net = faceparse.FaceParser()
    for call in (net, net.labels, faceparse.FaceSegmenter(net).segment_batch):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call(torch.zeros(1, 3, 32, 32))
        with pytest.raises(ValueError, match='B, 3, H, W'):
            call(torch.zeros(1, 4, 32, 32))
        with pytest.raises(ValueError, match='nothing is converted'):
            call(torch.zeros(1, 3, 32, 32, dtype=torch.float64))
        with pytest.raises(ValueError, match='B, 3, H, W'):
            call(torch.zeros(3, 32, 32))
    with pytest.raises(ValueError, match='n_classes'):
        faceparse.FaceParser(65)
    # the wrappers themselves
    fmap, table = torch.zeros(1, 3, 4, 4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.conv2d_add(fmap, torch.zeros(16 * 64), (8, 3, 1, 1), None, torch.zeros(1, 8, 4, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.maxpool3x3s2p1(fmap)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.gate_resample(fmap, rows=table, cols=table)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.bilinear_ac(fmap, (4, 4), torch.zeros(16, dtype=torch.int32), torch.zeros(8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.seg_labels(fmap, (4, 4), torch.zeros(16, dtype=torch.int32), torch.zeros(8))
    labels = torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.seg_correct_counts(labels, labels, (1,), (2,))
    # the routes
    for src, tgt in (((), (1,)), ((1,), ()), (tuple(range(17)), (1,)), ((1,), tuple(range(17)))):
        with pytest.raises(ValueError, match='1 .. 16'):
            distances.correct_modification(labels, labels, src, tgt)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        distances.correct_modification(labels, labels, (1,), (2,))
    with pytest.raises(ValueError, match='both'):
        distances.compute_dl(str(tmp_path), str(tmp_path), str(tmp_path), [0], segmenter=faceparse.FaceSegmenter(net))
    with pytest.raises(ValueError, match='neither'):
        distances.compute_dl(str(tmp_path), str(tmp_path), None, [0])


NAMES = ('rw_conv2d_add_f32', 'rw_maxpool3x3s2p1_f32', 'rw_gate_resample_f32', 'rw_bilinear_ac_f32', 'rw_seg_labels_i64',
         'rw_seg_correct_counts_i64')


def test_the_entries_are_bound_at_abi_11():
    assert _lib.ABI_VERSION == 11
    lib = _lib.load()
    assert lib.rw_abi_version() == 11
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert not name.endswith('_supported') and not name.startswith('rw_packed_')
    assert not [n for n in ('conv2d_add', 'maxpool3x3s2p1', 'gate_resample', 'bilinear_ac', 'seg_labels', 'seg_correct_counts')
                if not callable(getattr(hip, n)) or n.startswith('pack_')]


def test_the_entries_refuse_before_any_launch():
    """only cases that must refuse, on placeholder pointers that are never dereferenced; skipped where a HIP device is visible
    -- a refusal that regressed must not turn into a launch on them (the precaution of tests/test_abi_refusals.py)"""
    if torch.cuda.is_available():
        pytest.skip('a HIP device is visible: a regressed refusal would launch on placeholder pointers')
    lib = _lib.load()
    P, BAD, UNSUPPORTED = 0x10000, 10001, 10002
    conv = (1, 64, 8, 8, 64)                                         # batch, in_ch, h, w, out_ch
    assert lib.rw_conv2d_add_f32(P, P, P, None, P, *conv, 3, 3, 1, 1, 1, 1, None) == BAD                # no res
    assert lib.rw_conv2d_add_f32(None, P, P, P, P, *conv, 3, 3, 1, 1, 1, 1, None) == BAD
    assert lib.rw_conv2d_add_f32(P, P, P, P, P, *conv, 3, 3, 3, 1, 1, 1, None) == UNSUPPORTED           # stride 3
    assert lib.rw_conv2d_add_f32(P, P, P, P, P, *conv, 3, 3, 1, 3, 1, 1, None) == UNSUPPORTED           # padding >= kernel
    assert lib.rw_conv2d_add_f32(P, P, P, P, P, *conv, 8, 3, 1, 1, 1, 1, None) == UNSUPPORTED           # kernel > 7
    assert lib.rw_conv2d_add_f32(P, P + 4, P, P, P, *conv, 3, 3, 1, 1, 1, 1, None) == UNSUPPORTED       # wp not aligned
    assert lib.rw_maxpool3x3s2p1_f32(None, P, 1, 1, 4, 4, None) == BAD
    assert lib.rw_maxpool3x3s2p1_f32(P, P, 1, 1, 0, 4, None) == BAD
    assert lib.rw_maxpool3x3s2p1_f32(P, P, 1, 1, (1 << 20) + 1, 4, None) == UNSUPPORTED
    gate = (P, P, P, None, P, P, P, 1, 8, 4, 4, 6, 6)               # x gate add_map add_vec row col y, batch ch h w oh ow
    assert lib.rw_gate_resample_f32(*gate[:3], P, *gate[4:], None) == BAD                               # both adds
    assert lib.rw_gate_resample_f32(*gate[:4], None, *gate[5:], None) == BAD                            # no rows, 4 -> 6
    assert lib.rw_gate_resample_f32(*gate[:5], None, *gate[6:], None) == BAD                            # no cols, 4 -> 6
    assert lib.rw_gate_resample_f32(*gate[:6], None, *gate[7:], None) == BAD                            # no y
    assert lib.rw_gate_resample_f32(*gate[:11], 0, 6, None) == BAD
    assert lib.rw_gate_resample_f32(*gate[:11], (1 << 20) + 1, 6, None) == UNSUPPORTED
    assert lib.rw_bilinear_ac_f32(P, P, 1, 19, 4, 4, 32, 32, None, P, None) == BAD
    assert lib.rw_bilinear_ac_f32(P, P, 1, 19, 4, 4, 32, 32, P, None, None) == BAD
    assert lib.rw_bilinear_ac_f32(P, P, 1, 19, 4, 4, 32, (1 << 20) + 1, P, P, None) == UNSUPPORTED
    seg = (P, P, 1, 19, 4, 4, 32, 32, P, P)                          # logits labels batch n h w H W idx lam
    assert lib.rw_seg_labels_i64(*seg[:3], 65, *seg[4:], None, None, 32, 32, None) == UNSUPPORTED
    assert lib.rw_seg_labels_i64(*seg[:3], 0, *seg[4:], None, None, 32, 32, None) == BAD
    assert lib.rw_seg_labels_i64(*seg, None, P, 45, 45, None) == BAD                                    # no pick_row, 32 -> 45
    assert lib.rw_seg_labels_i64(*seg, P, None, 45, 45, None) == BAD
    assert lib.rw_seg_labels_i64(*seg[:8], None, P, None, None, 32, 32, None) == BAD
    one, many = (ctypes.c_int64 * 1)(3), (ctypes.c_int64 * 17)(*range(17))
    counts = lib.rw_seg_correct_counts_i64
    assert counts(P, P, 1, 16, 16, 16, one, 0, one, 1, P, None) == BAD                                  # an empty set
    assert counts(P, P, 1, 16, 16, 16, one, 1, None, 1, P, None) == BAD
    assert counts(P, P, 1, 16, 8, 16, one, 1, one, 1, P, None) == BAD                                   # stride below hw
    assert counts(P, None, 1, 16, 16, 16, one, 1, one, 1, P, None) == BAD
    assert counts(P, P, 1, 16, 16, 16, many, 17, one, 1, P, None) == UNSUPPORTED
    assert counts(P, P, 1, 16, 16, 16, one, 1, many, 17, P, None) == UNSUPPORTED
