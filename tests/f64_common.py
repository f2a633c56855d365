"""Shared by the float64-forward tests (test_f64_dispatch.py, test_gpu_f64_forward.py): the bar, and the reading of
every stage that oracle.restatement.generator_forward(collect=...) records through nethook hooks."""
import torch

from oracle import restatement as R
from rewriting_amd import synthetic
from rewriting_amd.utils import nethook, zdataset
from rewriting_amd.utils.stylegan2 import models


def deviation(got, want):
    """(max |got - want|, its bar 1e-9 max(1, max |want|)), both sides float64.  Derived, not measured: the rounding of a
    3x3 sum over <= 512 channels is bounded by 9 * 512 * 2^-53 = 5e-13 of the sum of |terms|, about twenty stages
    compound below 1e-10, and 1e-9 leaves a decade -- three orders below the 1e-6 of a float32 step anywhere."""
    assert got.dtype == torch.float64 and want.dtype == torch.float64, (got.dtype, want.dtype)
    assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
    err = (got.detach().cpu() - want).abs().max().item()
    return err, 1e-9 * max(1.0, want.abs().max().item())


def assert_close(got, want, what=''):
    err, lim = deviation(got, want)
    assert err <= lim, (what, err, lim)
    return err


def stage_source(stage):
    """(module name, DataBag field) that holds the restatement's stage `stage`."""
    if stage in ('style', 'latents'):
        return stage, 'latent'
    if stage.startswith(('to_rgb', 'up_rgb')):
        return stage, 'output'
    prefix, kind = stage.rsplit('.', 1)
    if kind == 'style':
        return prefix + '.mconv.modulation', 'style'
    if kind in ('adain', 'dconv', 'blur'):
        return prefix + '.mconv.' + kind, 'fmap'
    return prefix + '.' + kind, 'fmap'


def double_generator(size, batch, channel_multiplier=2, mconv='seq', device='cpu'):
    """(the .double() generator of synthetic weights (seed 0, truncation 0.5), its float64 state dict on the host,
    z.double() of standard_z_sample(seed=1))."""
    g = models.SeqStyleGAN2(size, 512, 8, channel_multiplier=channel_multiplier, truncation=0.5, mconv=mconv)
    synthetic.randomize_(g, seed=0)
    g = g.eval().double()
    sd = {k: v.detach().clone() for k, v in g.state_dict().items()}
    if mconv != 'seq':      # the restatement reads the 'seq' names
        sd = {k.replace('mconv.weight', 'mconv.dconv.weight') if k.endswith('mconv.weight') else k: v for k, v in sd.items()}
    z = zdataset.standard_z_sample(batch, 512, seed=1).double()
    return g.to(device), sd, z


def truth(sd, z, size):
    """(float64 image, {stage: float64 tensor}) of the restatement on the host."""
    stages = {}
    img = R.generator_forward(sd, z, size, truncation=0.5, collect=stages)
    return img, stages


def run_hooked(g, z, stages):
    """(image, {stage: tensor}) of g(z) with every stage of `stages` read through a nethook hook."""
    sources = {s: stage_source(s) for s in stages}
    with torch.no_grad(), nethook.InstrumentedModel(g) as inst:
        inst.retain_layers(sorted({m for m, _ in sources.values()}), detach=False)
        img = inst(z)
        got = {s: inst.retained_layer(m)[field] for s, (m, field) in sources.items()}
    return img, got
