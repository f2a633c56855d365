"""How the rewriter launches its four statistics sweeps (second moment, unit scales, unit quantiles, key ranking): what
reaches tally.tally_* -- batch_size, nchw, square_input, shard -- and the noise period in force while it runs.  The
goldens pin the results of these sweeps; this pins the launches.  CPU only, the kernel layer emulated where the model
is to count as on the device."""
import torch

from tests.search_checks import make_rewriter

SIZE, LAYER = 32, 4
TALLIES = ('tally_second_moment', 'tally_mean', 'tally_quantile', 'tally_topk_and_quantile')


def _spy_on_tallies(monkeypatch):
    """{tally name: [(keyword arguments, noise period at call time), ...]}, every call passed through."""
    from rewriting_amd.utils import tally
    from rewriting_amd.utils.stylegan2 import models
    calls = {name: [] for name in TALLIES}
    for name in TALLIES:
        def spy(*args, _real=getattr(tally, name), _seen=calls[name], **kwargs):
            _seen.append((dict(kwargs), models._noise_period[0]))
            return _real(*args, **kwargs)
        monkeypatch.setattr(tally, name, spy)
    return calls


def _run_every_sweep(gw):
    """The constructor has run collect_2nd_moment already."""
    gw.square_scales_for_units()
    gw.quantiles_for_units()
    gw.quantiles_for_covariance_adjusted_directions()
    key = torch.randn(gw.k_shape[1], generator=torch.Generator().manual_seed(0))
    gw.ranking_for_key(key / key.norm(), k=3)


def _assert_every_sweep_ran(calls):
    assert {name: len(seen) for name, seen in calls.items()} == dict(
        tally_second_moment=1, tally_mean=1, tally_quantile=2, tally_topk_and_quantile=1)


def test_a_periodic_dataset_is_swept_in_large_launches_with_period_10(emulated_hip, monkeypatch):
    from rewriting_amd import parallel
    from rewriting_amd.utils.stylegan2 import models
    calls = _spy_on_tallies(monkeypatch)
    before = models._noise_period[0]
    gw = make_rewriter('cpu', SIZE, 20, LAYER)
    assert gw._kernels() and gw._noise_periodic()
    _run_every_sweep(gw)
    _assert_every_sweep_ran(calls)
    for name in TALLIES:
        for kwargs, period in calls[name]:
            assert kwargs['batch_size'] == gw._sweep_batch(), name
            assert period == 10, name
    (kwargs, _), = calls['tally_second_moment']
    assert kwargs['nchw'] is True and 'shard' in kwargs and kwargs['shard'] == parallel.shard()
    (kwargs, _), = calls['tally_mean']
    assert kwargs['nchw'] is True and kwargs['square_input'] is True
    assert models._noise_period[0] == before


def test_a_ragged_dataset_is_swept_in_the_tally_default_batches(emulated_hip, monkeypatch):
    from rewriting_amd.utils.stylegan2 import models
    calls = _spy_on_tallies(monkeypatch)
    assert models._noise_period[0] == 0
    gw = make_rewriter('cpu', SIZE, 15, LAYER)
    assert gw._kernels() and not gw._noise_periodic()
    _run_every_sweep(gw)
    _assert_every_sweep_ran(calls)
    for name in TALLIES:
        for kwargs, period in calls[name]:
            assert 'batch_size' not in kwargs, name
            assert period == 0, name
    (kwargs, _), = calls['tally_second_moment']
    assert kwargs['nchw'] is True                         # the model counts as on the device
    (kwargs, _), = calls['tally_mean']
    assert kwargs['nchw'] is True and kwargs['square_input'] is True
    assert models._noise_period[0] == 0


def test_a_model_on_the_cpu_is_swept_in_rows(monkeypatch):
    from rewriting_amd import synthetic
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import proggan, runningstats, zdataset
    from rewriting_amd.utils.stylegan2 import models
    calls = _spy_on_tallies(monkeypatch)
    samples = []
    real_add = runningstats.RunningVariance.add

    def add(self, a, **kwargs):
        samples.append((a.clone(), dict(kwargs)))
        return real_add(self, a, **kwargs)
    monkeypatch.setattr(runningstats.RunningVariance, 'add', add)
    model = proggan.ProgressiveGenerator(resolution=32)
    synthetic.randomize_(model, seed=0, kind='proggan')
    model.eval()
    nseeds = 14                                            # a batch of 10 and a ragged one of 4
    gw = ganrewrite.ProgressiveGanRewriter(model, zdataset.z_dataset_for_model(model, size=nseeds), LAYER)
    assert not gw._kernels()
    _run_every_sweep(gw)
    _assert_every_sweep_ran(calls)
    for name in TALLIES:
        for kwargs, period in calls[name]:
            assert 'batch_size' not in kwargs, name
            assert period == 0, name
    (kwargs, _), = calls['tally_second_moment']
    assert kwargs['nchw'] is False
    (kwargs, _), = calls['tally_mean']
    assert kwargs['nchw'] is False and kwargs['square_input'] is False
    assert models._noise_period[0] == 0
    # what RunningVariance was handed: rows, already squared
    assert [s.shape[0] for s, _ in samples] == [10 * gw.k_shape[2] * gw.k_shape[3], 4 * gw.k_shape[2] * gw.k_shape[3]]
    assert all(not kw.get('nchw') and not kw.get('square_input') for _, kw in samples)
    with torch.no_grad():
        acts = gw.context_acts(gw.context_model(torch.stack([gw.zds[i][0] for i in range(10, nseeds)])))
    want = acts.permute(0, 2, 3, 1).reshape(-1, acts.shape[1]).pow(2)
    assert samples[1][0].shape == want.shape == (4 * gw.k_shape[2] * gw.k_shape[3], gw.k_shape[1])
    assert torch.equal(samples[1][0], want)
