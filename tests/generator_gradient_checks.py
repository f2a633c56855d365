"""TEST INFRASTRUCTURE -- the whole-generator gradient checks at the sizes where the forward and the backward leave the
routes of the 8^2 and 16^2 models, shared by the GPU test (tests/test_gpu_generator_gradients.py) and by its host twin on
the emulation (tests/test_generator_gradients.py).

The measure.  A generator forward evaluates a piecewise-linear function of its activations: each leaky ReLU takes one of
two branches per element.  A handful of the inputs lie within rounding of zero, and float32 and float64 -- or two float32
summation orders -- decide them differently; one flipped element moves a gradient tensor by 1e-4 and more, which no
margin over rounding error survives.  So the run under test records the branch it took at every leaky ReLU
(``decisions_of``) and BOTH host oracles, float64 (the truth) and float32 (the yardstick), are forced onto those branches
(oracle.restatement.Decisions): they then differentiate exactly the function the run evaluated, and what is left between
them is arithmetic.  No miss is allowed for.

Where each bar comes from (``failures``):

* MARGIN = 8 is the margin test_whole_generator_gradients_against_the_float64_oracle allows over the reference's own float32
  deviation; every yardstick below is measured on the reference (``d_ref`` = the float32 oracle against the float64 one,
  both under the run's decisions):
  - a tensor of more than one element:  d_hip(name) <= 8 d_ref(name), every tensor;
  - a one-element tensor (the noise strengths): a scalar's own d_ref is small or large by luck (4e-8 .. 7e-7 on the
    host), so the bar is 8 times the LARGEST d_ref among the one-element tensors of that run;
* the loss within 2e-6 relative and the image within 5e-5 L-infinity of the float64 oracle: the bars of the same test.

The decision hooks are ``register_forward_hook``s; routing looks only for nethook's planted ``forward`` attribute, so they
should change no launch -- ``recorded_run`` asserts that they did not, from the spy's record of the same run without them.
"""
import collections
import contextlib

import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests import grad_emulation as G

MARGIN = 8
LOSS_REL, IMAGE_LINF = 2e-6, 5e-5
OVERFIT_LOSS_REL = 1e-5           # test_all_weights_insert_at_16's bar for its first loss


# ---- the run under test -----------------------------------------------------------------------------------------------

@contextlib.contextmanager
def decisions_of(model):
    """[(module name, output > 0)] of every leaky ReLU of the forwards run inside, in call order.  The hooks sit on the
    styled-convolution BLOCKS and on the activated EqualLinears: a block's output map is its activation's output whether
    the block ran as one fused kernel or module by module (a hook on `activate` would miss the fused blocks), and the
    output has the sign of the activation's input."""
    from rewriting_amd.utils.stylegan2 import models
    seen, handles = [], []

    def hook(name):
        def record(module, args, output):
            t = output
            if isinstance(output, dict):
                if output.get('prescaled') is not None:
                    raise AssertionError('%s: the map carries the next layer\'s style: not the activation\'s output' % name)
                t = output['fmap'] if isinstance(module, models.StyledConvSeq) else output['latent']
            assert torch.is_tensor(t), (name, type(t))
            seen.append((name, t.detach() > 0))
        return record
    for name, m in model.named_modules():
        if isinstance(m, models.StyledConvSeq) or (isinstance(m, models.EqualLinear) and m.activation):
            handles.append(m.register_forward_hook(hook(name)))
    try:
        yield seen
    finally:
        for h in handles:
            h.remove()


def repack(model):
    """every recording packs its own weights"""
    for m in model.modules():
        if hasattr(m, '_derived'):
            m._derived.store.clear()


def forward_backward(model, z, target, z_grad=True):
    """The recipe on `model` (any device): (loss, image, {name: gradient or None} with 'z'), all detached."""
    dev = next(model.parameters()).device
    z = z.detach().clone().to(dev).requires_grad_(z_grad)       # a leaf of this run alone
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        out = model(z)
        loss = G.smooth_loss(out, target.to(dev))
        loss.backward()
    grads = {name: p.grad for name, p in model.named_parameters()}
    grads['z'] = z.grad
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return loss.detach(), out.detach(), grads


Run = collections.namedtuple('Run', 'loss image grads decisions launches')


def recorded_run(model, z, target, log, z_grad=True):
    """Forward and backward twice, every weight packed anew each time: first plain, then with the decision hooks
    planted.  `log`: the list route_spy.install_spies appends to.  Asserts that the hooks changed no launch; returns the
    hooked run (its gradients belong to its decisions)."""
    repack(model)
    del log[:]
    forward_backward(model, z, target, z_grad)
    plain = list(log)
    repack(model)
    del log[:]
    with decisions_of(model) as seen:
        loss, image, grads = forward_backward(model, z, target, z_grad)
    hooked = list(log)
    del log[:]
    assert plain, 'the spy recorded nothing'
    assert hooked == plain, 'the decision hooks changed the launches:\n%s' % '\n'.join(
        '%s | %s' % pair for pair in zip(plain, hooked) if pair[0] != pair[1])
    return Run(loss, image, grads, [(name, d.cpu()) for name, d in seen], hooked)


def launched(log, name, shape, impl=None, flags=()):
    """the recorded calls of wrapper `name` on an input of `shape` (a tuple), with this impl and these arguments given"""
    hits = []
    for call in log:
        n, s, _, i, on = call.split(' ')
        if (n == name and s == 'x'.join(map(str, shape)) and (impl is None or i == str(impl))
                and set(flags) <= set(on.split(','))):
            hits.append(call)
    return hits


def index_of(log, name, shape, **more):
    hits = launched(log, name, shape, **more)
    assert hits, (name, shape, more)
    return log.index(hits[0])


# ---- the oracles ------------------------------------------------------------------------------------------------------

def pinned_oracles(sd, names, z, target, size, truncation, decisions):
    """((loss, image, gradients) in float64, the same in float32), both on the branches `decisions` names."""
    pinned = [d for _, d in decisions]
    return tuple(G.oracle_gradients(sd, names, z, target, size, truncation, dtype, decisions=pinned)
                 for dtype in (torch.float64, torch.float32))


def pinning_report(sd, z, size, truncation, decisions):
    """{layer: how many of the run's decisions differ from the float64 oracle's own (unpinned)}, layers without a
    difference left out; 'of' = the number of decisions.  Reported, never asserted: it says how much the pinning mattered."""
    own = R.RecordDecisions()
    with torch.no_grad():
        R.generator_forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, z.double(), size,
                            truncation=truncation, decisions=own)
    assert len(own) == len(decisions)
    differ = {name: int((d != o).sum()) for (name, d), o in zip(decisions, own)}
    out = {name: n for name, n in differ.items() if n}
    out['total'] = sum(differ.values())
    out['of'] = sum(d.numel() for _, d in decisions)
    return out


# ---- the measure and the bar -------------------------------------------------------------------------------------------

def measure(got, g64, g32):
    """{tensor: d_hip = |got - g64| / |g64|, d_ref = |g32 - g64| / |g64| (2-norms), their ratio, the tensor's size} for
    every tensor of g64; g64, g32: the float64 and float32 host oracles under the run's own decisions."""
    fig = {}
    for name, want in g64.items():
        d_hip, d_ref = G.rel(got[name], want), G.rel(g32[name], want)
        fig[name] = dict(d_hip=d_hip, d_ref=d_ref, ratio=d_hip / d_ref if d_ref else float('inf'), numel=want.numel())
    return fig


def failures(fig):
    """[(tensor, d_hip, bar)] of the tensors over the bar (see the module's docstring); the bar is written into `fig`."""
    scalars = [f['d_ref'] for f in fig.values() if f['numel'] == 1]
    bad = []
    for name, f in fig.items():
        f['bar'] = MARGIN * (max(scalars) if f['numel'] == 1 else f['d_ref'])
        if not f['d_hip'] <= f['bar']:
            bad.append((name, f['d_hip'], f['bar']))
    return bad


def summary(fig):
    """what the report and DESIGN.md's table hold of one run"""
    multi = {n: f for n, f in fig.items() if f['numel'] > 1}
    single = {n: f for n, f in fig.items() if f['numel'] == 1}
    out = {}
    worst = max(multi, key=lambda n: multi[n]['ratio'])
    out.update(worst_ratio=multi[worst]['ratio'], worst_ratio_tensor=worst,
               largest_d_ref=max(f['d_ref'] for f in fig.values()), largest_d_hip=max(f['d_hip'] for f in fig.values()))
    if single:
        worst = max(single, key=lambda n: single[n]['d_hip'])
        out.update(worst_scalar_d_hip=single[worst]['d_hip'], worst_scalar=worst,
                   scalar_bar=single[worst]['bar'] if 'bar' in single[worst] else None,
                   worst_scalar_own_ratio=max(f['ratio'] for f in single.values()))
    return out


def check(run, sd, names, z, target, size, truncation):
    """The whole comparison of one run: (figures for the report, list of failed checks).  names: the tensors that must
    have received a gradient ('z' among them where the latent has one); every one of them is held at the bar."""
    params = [n for n in names if n != 'z']
    missing = [n for n in names if run.grads[n] is None]
    (loss64, image64, g64), (_, _, g32) = pinned_oracles(sd, params, z, target, size, truncation, run.decisions)
    g64 = {n: g64[n] for n in names}
    fig = measure({n: run.grads[n] for n in names if n not in missing}, {n: g64[n] for n in names if n not in missing}, g32)
    bad = [('no gradient', n) for n in missing] + failures(fig)
    loss_rel = abs(run.loss.item() - loss64.item()) / abs(loss64.item())
    image_linf = (run.image.double().cpu() - image64).abs().max().item()
    if not loss_rel <= LOSS_REL:
        bad.append(('loss', loss_rel, LOSS_REL))
    if not image_linf <= IMAGE_LINF:
        bad.append(('image', image_linf, IMAGE_LINF))
    figures = dict(summary(fig), loss_rel=loss_rel, image_linf=image_linf, tensors=fig,
                   pinned=pinning_report(sd, z, size, truncation, run.decisions))
    return figures, bad


def describe(tag, figures):
    f = figures
    line = '%s: worst ratio %.2f on %s, largest d_ref %.2e, d_hip %.2e' % (
        tag, f['worst_ratio'], f['worst_ratio_tensor'], f['largest_d_ref'], f['largest_d_hip'])
    if 'worst_scalar' in f:
        line += '; scalars: d_hip %.2e on %s (bar %.2e, worst ratio to its own d_ref %.2f)' % (
            f['worst_scalar_d_hip'], f['worst_scalar'], f['scalar_bar'], f['worst_scalar_own_ratio'])
    return line + '; loss rel %.2e, image Linf %.2e; %d of %d decisions differ from float64\'s own' % (
        f['loss_rel'], f['image_linf'], f['pinned']['total'], f['pinned']['of'])


# ---- scenarios B and C: which parameters train -------------------------------------------------------------------------

@contextlib.contextmanager
def only_trainable(model, names):
    """Inside: exactly the parameters `names` require a gradient; afterwards every parameter does, as a fresh model's."""
    from rewriting_amd.utils import nethook
    params = dict(model.named_parameters())
    nethook.set_requires_grad(False, model)
    try:
        if names:
            nethook.set_requires_grad(True, *[params[n] for n in names])
        yield
    finally:
        nethook.set_requires_grad(True, model)


def partly_frozen_names(model):
    """scenario C: the parameters of layer10 and to_rgb5"""
    return [n for n, _ in model.named_parameters() if n.startswith(('layer10.', 'to_rgb5.'))]


# ---- scenario D: the overfit loop, teacher-forced ----------------------------------------------------------------------

OVERFIT = dict(size=32, niter=6, bounds=(8, 8, 24, 24), lr=0.01)


def overfit_loss(sd, x, z, bounds, size, truncation, feature_net, dtype=torch.float64):
    """all_weights_insert's loss (rewrite/ganrewrite.py:300-331) of the restatement at the state `sd`, no decision pinned:
    the loss is continuous across the kinks."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    t, l, b, r = bounds
    with torch.no_grad():
        out = R.generator_forward(sd, z.to(dtype), size, truncation=truncation)
        gt, pred = x.to(dtype)[:, :, t:b, l:r], out[:, :, t:b, l:r]
        return (F.l1_loss(gt, pred) + 1e-2 * F.mse_loss(feature_net(gt), feature_net(pred))).item()


def install_pack_spy(monkeypatch, packs):
    """Appends (wrapper, data_ptr of the weight it was handed) for every pack_* wrapper of rewriting_amd.hip: the
    launch record of tests/route_spy.py names a weight by its shape alone, and every layer of the 32^2 model has one shape."""
    from rewriting_amd import hip
    from tests import route_spy
    for name in route_spy.launchers(hip):
        if not name.startswith('pack_'):
            continue

        def spied(weight, *args, _name=name, _fn=getattr(hip, name), **kwargs):
            packs.append((_name, weight.data_ptr()))
            return _fn(weight, *args, **kwargs)
        monkeypatch.setattr(hip, name, spied)


def teacher_forced_overfit(model, truncation, device, monkeypatch):
    """all_weights_insert on `model` (OVERFIT's recipe, perceptual network G.PooledMix()), the state copied to the host
    after every optimizer.step().  Returns (rows, failed checks, the packs of iteration 0): row `it` = the loss the loop reported at iteration it
    beside the float64 restatement's loss AT THE STATE THE LOOP WAS IN -- the initial one for it = 0, the snapshot of
    iteration it - 1 after -- so the trajectories cannot drift apart, and a packed weight that went stale after a step shows
    at it = 1.  Also held: every iteration packs every trained convolution weight exactly as iteration 0 (cold caches)
    did, each form once."""
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import zdataset
    from rewriting_amd.utils.stylegan2 import models
    size, niter, bounds, lr = (OVERFIT[k] for k in ('size', 'niter', 'bounds', 'lr'))
    zds = zdataset.z_dataset_for_model(model, size=4)
    gw = ganrewrite.SeqStyleGanRewriter(model, zds, 6, cachedir=None)
    z = gw.get_z(0)
    with torch.no_grad():
        x = gw.model(gw.get_z(1))
    net = G.PooledMix()             # the host's; the loop gets a copy of its own on `device`
    weights = {m.weight.data_ptr(): name for name, m in gw.model.named_modules()
               if isinstance(m, models.DemodulatedConv2dF)}
    states = [{k: v.detach().cpu().clone() for k, v in gw.model.state_dict().items()}]
    reported, packs, packs_of = [], [], []
    repack(gw.model)
    install_pack_spy(monkeypatch, packs)

    def after_step(it, loss):
        reported.append(loss.item())
        states.append({k: v.detach().cpu().clone() for k, v in gw.model.state_dict().items()})
        packs_of.append(collections.Counter((weights[ptr], name) for name, ptr in packs if ptr in weights))
        del packs[:]
    gw.all_weights_insert(x, z, bounds=bounds, niter=niter, lr=lr, feature_net=G.PooledMix().to(device),
                          update_callback=after_step)
    x, z = x.cpu(), z.cpu()
    rows, bad = [], []
    if len(reported) != niter:
        bad.append(('iterations', len(reported), niter))
    for it, got in enumerate(reported):
        want = overfit_loss(states[it], x, z, bounds, size, truncation, net)
        rows.append(dict(it=it, loss=got, oracle=want, rel=abs(got - want) / abs(want)))
        if not rows[-1]['rel'] <= OVERFIT_LOSS_REL:
            bad.append(('loss', it, got, want))
    first = packs_of[0]
    if set(layer for layer, _ in first) != set(weights.values()) or set(first.values()) != {1}:
        bad.append(('packs of iteration 0', dict(first)))
    for it, counted in enumerate(packs_of):
        if counted != first:
            bad.append(('packs', it, dict(counted)))
    return rows, bad, {('%s %s' % key): n for key, n in sorted(first.items())}
