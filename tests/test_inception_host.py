"""The host side of the Inception feature extractor (rewriting_amd/inception.py, samples.activation_statistics): the
batch-norm fold, the loader's refusals, the layout table and the checks made before any library call.  No GPU."""
import numpy
import pytest
import torch

from rewriting_amd import inception, samples
from tests import inception_checks as K


def test_twin_is_alive():
    """the float64 twin alone: finite features, at least 40 % of them non-zero -- a dead network passes nothing vacuously"""
    _, _, twin64 = K.shared_twin()
    f = twin64(K.images((2, 3, 75, 75), 1).double())
    assert f.shape == (2, 2048) and torch.isfinite(f).all()
    assert (f != 0).double().mean().item() >= 0.4


def test_fold_equals_the_float64_formula():
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(7, 5, 3, 1, generator=gen)
    gamma, var = torch.rand(7, generator=gen) + 0.5, torch.rand(7, generator=gen) + 0.5
    beta, mean = 0.1 * torch.randn(7, generator=gen), 0.1 * torch.randn(7, generator=gen)
    fw, fb = inception.fold_batch_norm(w, gamma, beta, mean, var)
    s = gamma.double() / (var.double() + 1e-3).sqrt()
    assert fw.dtype == fb.dtype == torch.float32
    assert torch.equal(fw, (w.double() * s[:, None, None, None]).float())
    assert torch.equal(fb, (beta.double() - mean.double() * s).float())
    # and it is the batch norm: conv + bn in float64 against the folded convolution in float64
    x = torch.randn(2, 5, 6, 4, generator=gen).double()
    bn = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, w.double()), mean.double(), var.double(),
                                        gamma.double(), beta.double(), False, 0.0, 1e-3)
    assert K.rel(torch.nn.functional.conv2d(x, fw.double(), fb.double()), bn) < 1e-6


def test_layout_table():
    out = {b.name: inception.block_out_channels(b) for b in inception.BLOCKS}
    assert [out[n] for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_7a', 'Mixed_7c')] == \
        [256, 288, 288, 768, 1280, 2048]
    assert all(out[n] == 768 for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e')) and out['Mixed_7b'] == 2048
    layers = inception.conv_layers()
    assert len(layers) == 94 and len({name for name, _ in layers}) == 94
    # every block reads what the one before wrote
    ch = 192
    for b in inception.BLOCKS:
        assert b.in_ch == ch, b.name
        ch = out[b.name]
    # weights, and the gamma / beta of every batch norm
    assert sum(op.out_ch * op.in_ch * op.kernel[0] * op.kernel[1] + 2 * op.out_ch for _, op in layers) == 21785568
    twin, sd, _ = K.shared_twin()
    assert {name + '.conv.weight' for name, _ in layers} == {k for k in sd if k.endswith('conv.weight')}


def test_loader_accepts_the_twin_and_ignores_the_heads():
    _, sd, _ = K.shared_twin()
    extra = dict(sd)
    extra['fc.weight'], extra['fc.bias'] = torch.zeros(1008, 2048), torch.zeros(1008)
    extra['AuxLogits.conv0.conv.weight'] = torch.zeros(128, 768, 1, 1)
    net = inception.from_state_dict(extra)
    assert isinstance(net, inception.FIDInception) and not net.training
    assert not any(p.requires_grad for p in net.parameters())
    assert len(list(net.parameters())) == 2 * 94
    name = 'Mixed_6c.branch7x7dbl_3'
    w, b = inception.fold_batch_norm(sd[name + '.conv.weight'], sd[name + '.bn.weight'], sd[name + '.bn.bias'],
                                     sd[name + '.bn.running_mean'], sd[name + '.bn.running_var'])
    assert torch.equal(net.state_dict()[name + '.weight'], w) and torch.equal(net.state_dict()[name + '.bias'], b)
    assert tuple(w.shape) == (160, 160, 1, 7)
    assert any(k.endswith('num_batches_tracked') for k in sd)       # the twin has them; they were ignored


def test_loader_refusals_name_the_key(tmp_path):
    _, sd, _ = K.shared_twin()
    lacking = dict(sd)
    del lacking['Mixed_7a.branch7x7x3_2.bn.running_var']
    with pytest.raises(KeyError, match='Mixed_7a.branch7x7x3_2.bn.running_var'):
        inception.from_state_dict(lacking)
    wrong = dict(sd)
    wrong['Mixed_5b.branch5x5_2.conv.weight'] = torch.zeros(64, 48, 3, 3)
    with pytest.raises(ValueError, match='Mixed_5b.branch5x5_2.conv.weight'):
        inception.from_state_dict(wrong)
    live = dict(sd)
    live['Conv2d_3b_1x1.bn.weight'] = sd['Conv2d_3b_1x1.bn.weight'].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match='Conv2d_3b_1x1.bn.weight'):
        inception.from_state_dict(live)
    stray = dict(sd)
    stray['Mixed_8a.branch1x1.conv.weight'] = torch.zeros(1)
    with pytest.raises(KeyError, match='Mixed_8a'):
        inception.from_state_dict(stray)
    # the file form
    path = tmp_path / 'inception.pt'
    torch.save(sd, str(path))
    assert isinstance(inception.fid_inception(str(path)), inception.FIDInception)


def test_inputs_are_refused_before_any_library_call(monkeypatch):
    from rewriting_amd import hip

    def no_library():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(hip, 'lib', no_library)
    net = inception.FIDInception()
    with pytest.raises(ValueError, match='75'):
        net(torch.zeros(1, 3, 74, 75), resize=False)
    with pytest.raises(ValueError, match='75'):
        net(torch.zeros(1, 80, 74, 3, dtype=torch.uint8), resize=False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(1, 3, 75, 75), resize=False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match='uint8'):
        net(torch.zeros(1, 4, 75, 75))
    with pytest.raises(ValueError, match='nothing is converted'):
        net(torch.zeros(1, 3, 75, 75, dtype=torch.float64))
    # the wrappers themselves
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.conv2d(torch.zeros(1, 3, 9, 9), torch.zeros(16 * 64), (8, 3, 1, 1))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.pool3x3(torch.zeros(1, 3, 9, 9), 'avg')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.global_avgpool(torch.zeros(1, 3, 9, 9))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.inception_input(torch.zeros(1, 3, 9, 9))


def test_conv2d_out_size_refuses_what_the_entry_refuses():
    from rewriting_amd import hip
    assert hip.conv2d_out_size(8, 8, (3, 3), 2, (0, 0)) == (3, 3)
    assert hip.conv2d_out_size(3, 5, (1, 7), 1, (0, 3)) == (3, 5)
    for kernel, stride, padding in (((9, 1), 1, (0, 0)), ((3, 3), 3, (0, 0)), ((3, 3), 1, (3, 0)), ((1, 1), 1, (0, 1))):
        with pytest.raises(ValueError):
            hip.conv2d_out_size(8, 8, kernel, stride, padding)
    with pytest.raises(ValueError, match='smaller'):
        hip.conv2d_out_size(2, 8, (3, 3), 1, (0, 0))


def test_activation_statistics_with_a_stub_extractor():
    gen = torch.Generator().manual_seed(5)
    proj = torch.randn(3 * 4 * 4, 12, generator=gen).double()

    def stub(images):
        return images.double().reshape(images.shape[0], -1) @ proj
    batches = [torch.randn(n, 3, 4, 4, generator=gen) for n in (5, 7, 4)]
    stats = samples.activation_statistics(batches, stub)
    assert isinstance(stats, samples.FeatureStatistics) and stats.count == 16
    act = torch.cat([stub(b) for b in batches]).numpy()
    mu, sigma = stats.mean_cov()
    numpy.testing.assert_allclose(mu, numpy.mean(act, axis=0), rtol=1e-12, atol=1e-12)
    numpy.testing.assert_allclose(sigma, numpy.cov(act, rowvar=False), rtol=1e-10, atol=1e-10)
    # the (seeds, images) pairs of samples.generate
    pairs = samples.activation_statistics([([0] * b.shape[0], b) for b in batches], stub)
    assert torch.equal(pairs.outer, stats.outer) and torch.equal(pairs.sum, stats.sum)
    with pytest.raises(ValueError, match='no batch'):
        samples.activation_statistics([], stub)
