"""Pins the travelling oracle (oracle/restatement.py, oracle/native_ops.c) against fixtures
produced by the reference's own files (oracle/make_golden.py), and this package's statistics caches
against what the reference wrote and read (tests/golden/reference_checks.npz)."""
import hashlib
import json
import os
import math

import numpy
import pytest
import torch

from oracle import native, restatement as R
from tests.conftest import (build_stylegan, golden_meta, load_golden, load_mask_request,
                            oracle_state_dict, subsample)

STAGE_ALIASES = [('.sconv.mconv.', '.sconv.'), ('.conv.mconv.', '.conv.')]


def test_native_ops_c_and_torch_restatements_match_reference_spec():
    g = load_golden('ops')
    ncase = len([k for k in g.files if k.startswith('upfirdn/') and k.endswith('/x')])
    assert ncase >= 7
    for ci in range(ncase):
        x, k, y = (torch.from_numpy(g['upfirdn/%d/%s' % (ci, n)]) for n in 'xky')
        up, down, p0, p1 = [int(v) for v in g['upfirdn/%d/cfg' % ci]]
        got = R.upfirdn2d(x, k, up=up, down=down, pad=(p0, p1))
        assert got.shape == y.shape
        assert (got - y).abs().max() < 1e-5
        b, c, h, w = x.shape
        gotc = native.upfirdn2d(x.reshape(-1, h, w, 1).numpy(), k.numpy(), up, up, down, down, p0, p1, p0, p1)
        assert numpy.abs(gotc.reshape(y.shape) - y.numpy()).max() < 1e-5
    x, b, y = (torch.from_numpy(g['lrelu/' + n]) for n in ('x', 'b', 'y'))
    assert torch.equal(R.fused_leaky_relu(x, b), y)
    assert numpy.array_equal(native.fused_bias_act(x.numpy(), b.numpy(), None, 3, 0, 0.2, 2 ** 0.5), y.numpy())
    go = torch.from_numpy(g['lrelu/go'])
    gx, gb = R.fused_leaky_relu_backward(go, y)
    # the golden went through torch autograd ((g*scale)*slope); the kernel order is (g*slope)*scale
    assert (gx - torch.from_numpy(g['lrelu/gx'])).abs().max() < 1e-6
    assert (gb - torch.from_numpy(g['lrelu/gb'])).abs().max() < 1e-5
    assert numpy.abs(native.fused_bias_act(go.numpy(), None, y.numpy(), 3, 1, 0.2, 2 ** 0.5)
                     - g['lrelu/gx']).max() < 1e-6
    assert numpy.array_equal(native.fused_bias_act(go.numpy(), None, y.numpy(), 3, 1, 0.2, 2 ** 0.5), gx.numpy())
    x2, b2 = torch.from_numpy(g['lrelu2/x']), torch.from_numpy(g['lrelu2/b'])
    assert torch.equal(R.fused_leaky_relu(x2, b2), torch.from_numpy(g['lrelu2/y']))


def test_upfirdn2d_adjoint_identity():
    """<A x, y> == <x, A^T y> for the adjoint algebra of op/upfirdn2d.py:100-115."""
    rs = numpy.random.RandomState(3)
    for up, down, pad, shape in [(1, 1, (1, 1), (1, 2, 9, 9)), (2, 1, (2, 1), (1, 2, 6, 6)),
                                 (1, 2, (2, 1), (1, 1, 12, 12))]:
        k = R.make_kernel([1, 3, 3, 1]) * up * up
        k[0, 2] += 0.05
        x = torch.from_numpy(rs.randn(*shape).astype('float32'))
        y = R.upfirdn2d(x, k, up=up, down=down, pad=pad)
        gy = torch.from_numpy(rs.randn(*y.shape).astype('float32'))
        gx = R.upfirdn2d_backward(gy, k, up, down, pad, x.shape)
        assert abs((y * gy).sum().item() - (x * gx).sum().item()) < 1e-3


@pytest.mark.parametrize('name', ['gen_s32_t05', 'gen_s64_cm1'])
def test_generator_restatement_matches_reference_golden(name):
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_stylegan(meta['size'], meta['truncation'], meta['channel_multiplier'])
    sd = oracle_state_dict(model)
    col = {}
    img = R.generator_forward(sd, torch.from_numpy(g['z']), meta['size'],
                              truncation=meta['truncation'], collect=col)
    assert (img - torch.from_numpy(g['image'])).abs().max() < 2e-5
    checked = 0
    for key in g.files:
        if not key.startswith('stage/') or not key.endswith('/sub'):
            continue
        lname = key[len('stage/'):-len('/sub')]
        short = lname
        for a, b in STAGE_ALIASES:
            short = short.replace(a, b)
        if short.endswith('.modulation') and not short.startswith('to_rgb'):
            short = short[:-len('modulation')] + 'style'
        if short == 'style.8':
            short = 'style'
        if short not in col:
            continue
        want = torch.from_numpy(g[key])
        got = subsample(col[short])
        assert got.shape == want.shape, lname
        assert (got - want).abs().max() < 3e-5 * max(1.0, want.abs().max().item()), lname
        checked += 1
    assert checked >= 40, checked


def _rewriter_pieces(g, meta):
    model = build_stylegan(meta['size'], meta['truncation'])
    sd = oracle_state_dict(model)
    zs = torch.from_numpy(numpy.random.RandomState(1).standard_normal(meta['nseeds'] * 512)
                          .reshape(meta['nseeds'], 512)).float()
    return sd, zs


def test_rewriter_restatement_matches_reference_golden_horsehat():
    g = load_golden('rw_s64_l8_horsehat')
    meta = golden_meta(g)
    sd, zs = _rewriter_pieces(g, meta)
    size, layer, trunc = meta['size'], meta['layernum'], meta['truncation']
    req = load_mask_request(meta['mask'], meta['nseeds'])
    # key statistics: batches of 10 in order (quirk Q1: noise row = position in the batch)
    keys = (R.context_forward(sd, zs[i:i + 10], size, layer, trunc)[0] for i in range(0, len(zs), 10))
    C, mom2, count = R.second_moment(keys)
    assert count == meta['nseeds'] * 32 * 32
    assert abs(C.double().norm().item() / float(g['c_matrix_norm']) - 1) < 1e-5
    assert (C[::4, ::4] - torch.from_numpy(g['c_matrix'])).abs().max() < 1e-4 * C.abs().max()
    Z = R.zca_from_cov(C)
    assert abs(Z.double().norm().item() / float(g['zca_norm']) - 1) < 1e-3
    # context direction from the golden-consistent Z
    obs, wts = [], []
    for imgnum, mask in req['key']:
        k, _, _ = R.context_forward(sd, zs[imgnum][None], size, layer, trunc)
        obs.append(k.permute(0, 2, 3, 1).reshape(-1, k.shape[1]))
        wts.append(R.mask_from_url(mask, (32, 32)).reshape(-1)[:, None])
    mkey, zk = R.multi_key_zca(obs, wts, Z, 1)
    want = torch.from_numpy(g['mkey'])
    assert zk.shape[0] == int(g['n_sel'])
    assert (mkey - want).abs().max() < 2e-3, (mkey - want).abs().max()
    # goal
    o_img, o_mask = req['object']
    p_img, p_mask = req['paste']
    ko, so, _ = R.context_forward(sd, zs[o_img][None], size, layer, trunc)
    vo = R.target_forward(sd, layer, ko, so)
    area = R.mask_from_url(o_mask, (32, 32))
    t, l, b, r = R.positive_bounding_box(area)
    assert [t, l, b, r] == list(g['obj_bounds'])
    kp, sp, _ = R.context_forward(sd, zs[p_img][None], size, layer, trunc)
    vp = R.target_forward(sd, layer, kp, sp)
    parea = R.mask_from_url(p_mask, (32, 32))
    tgt, bounds = R.paste_clip_at_center(vp, vo[:, :, t:b, l:r], R.centered_location(parea), area[t:b, l:r])
    assert list(bounds) == list(g['paste_bounds'])
    ck, cv, _, _ = R.crop_clip_to_bounds(kp, tgt, bounds)
    assert (ck - torch.from_numpy(g['goal_in_fmap'])).abs().max() < 1e-4
    assert (cv - torch.from_numpy(g['goal_out_fmap'])).abs().max() < 1e-4
    # the solve, explicit arithmetic vs the reference's autograd + torch.optim.Adam
    W0 = sd['layer%d.sconv.mconv.dconv.weight' % layer]
    _, losses, snaps = R.insert_explicit(
        W0, torch.from_numpy(g['goal_in_fmap']), torch.from_numpy(g['goal_in_style']),
        torch.from_numpy(g['goal_out_fmap']), sd['layer%d.sconv.activate.bias' % layer],
        sd['layer%d.sconv.noise.weight' % layer], want, niter=101, snapshots=(1, 10, 11, 100, 101))
    for n in (1, 10, 11, 100, 101):
        dW = (snaps[n] - W0)[0]
        ref_norm = float(g['dW_%d_norm' % n])
        cos = torch.einsum('oiyx,di->odyx', dW, want)
        rel = (cos - torch.from_numpy(g['dW_%d_cos' % n])).norm() / ref_norm
        assert abs(dW.double().norm().item() / ref_norm - 1) < 1e-4, n
        assert rel < 1e-4, (n, rel.item())
        assert (subsample(dW, 8192) - torch.from_numpy(g['dW_%d_sub' % n])).norm() / \
            torch.from_numpy(g['dW_%d_sub' % n]).norm() < 2e-4, n
    assert numpy.abs(numpy.array(losses) - g['losses']).max() < 1e-5


def test_proggan_restatement_matches_reference_golden():
    from rewriting_amd.utils import proggan
    from rewriting_amd import synthetic
    g = load_golden('pg64_l6_spire2tree')
    meta = golden_meta(g)
    model = proggan.ProgressiveGenerator(resolution=meta['resolution'])
    synthetic.randomize_(model, seed=0, kind='proggan')
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    z = torch.from_numpy(g['z0'])[None]
    img = R.proggan_forward(sd, z)
    assert (img - torch.from_numpy(g['image'])).abs().max() < 1e-4


def _recorded(g, prefix):
    """{name: array} of the fixture entries under `prefix` (reference_checks.npz)."""
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def _same_arrays(got, want, levels=False):
    """What this package writes now is what it wrote when the reference read it back (same keys, dtypes, values).
    levels=True: float arrays are retained samples of a random draw made on this host's cores -- compared as sorted
    columns to float32 rounding (the reference reads them order-free)."""
    got = {k: numpy.asarray(v) for k, v in got.items() if numpy.asarray(v).dtype != object}
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
        if levels and v.dtype.kind == 'f':
            a, b = (numpy.sort(t, axis=0) if t.ndim == 2 else t for t in (got[k], v))
            assert numpy.allclose(a, b, rtol=1e-5, atol=1e-6), k
        else:
            assert numpy.array_equal(got[k], v), k


def _reference_r2m(path):
    """Writes the reference's notebooks/masks/reflections/progan-kitchen/r2m.npz to `path` from its stored form (the
    upper triangle of the symmetric mom2, the other fields as they are) and returns `path`."""
    t = load_golden('r2m_progan_kitchen_triu')
    tri = t['mom2_triu']
    n = int(round(((8 * tri.size + 1) ** 0.5 - 1) / 2))
    iu = numpy.triu_indices(n)
    mom2 = numpy.zeros((n, n), tri.dtype)
    mom2[iu] = tri
    mom2.T[iu] = tri
    assert hashlib.sha256(mom2.tobytes()).hexdigest() == str(t['mom2_sha256'])
    numpy.savez(path, constructor=t['constructor'], count=t['count'], mom2=mom2,
                sample_size=numpy.array(None, dtype=object))
    return path


def test_restatement_against_live_reference():
    """The reference's forward of a 16^2 generator (truncation 0.7, weights seed 3, z seed 5), recorded by
    oracle/make_golden.py golden_reference_checks."""
    g = load_golden('reference_checks')
    sd = oracle_state_dict(build_stylegan(16, 0.7, seed=3))
    z = torch.from_numpy(g['restate/z'])
    got = R.generator_forward(sd, z, 16, truncation=0.7)
    assert (got - torch.from_numpy(g['restate/image'])).abs().max() < 1e-5


def test_statistics_cache_interoperates_with_the_reference(tmp_path):
    """the reference's own notebooks/masks/reflections/progan-kitchen/r2m.npz (a copy:
    tests/golden/r2m_progan_kitchen_triu.npz, rebuilt bit for bit by _reference_r2m) loads into this package's RunningSecondMoment and through
    tally.load_cached_state (utils/tally.py:703-718, utils/runningstats.py:1111-1120) and gives the moment the
    reference's class gives; a cache written here has the reference's keys and dtypes and is what the reference's
    RunningSecondMoment and tally cache branch read back correctly when the fixture was recorded."""
    import numpy
    from rewriting_amd.utils import runningstats, tally
    rec = load_golden('reference_checks')
    path = _reference_r2m(str(tmp_path / 'reference_r2m.npz'))
    theirs = numpy.load(path, allow_pickle=True)
    r = runningstats.RunningSecondMoment(state=theirs)
    assert r.count == int(theirs['count']) == 256000 and tuple(r.mom2.shape) == (512, 512)
    assert torch.equal(r.mom2, torch.from_numpy(theirs['mom2']))

    def is_reference_moment(m):
        return (str(m.dtype) == str(rec['r2m/moment_dtype']) and
                hashlib.sha256(m.numpy().tobytes()).hexdigest() == str(rec['r2m/moment_sha256']))
    assert is_reference_moment(r.moment())
    via_tally = tally.tally_second_moment(lambda z: None, torch.zeros(1, 1), sample_size=None, cachefile=path)
    assert is_reference_moment(via_tally.moment())                 # found, matched on sample_size, never swept
    # round trip: what this package writes has the reference's keys and dtypes ...
    mine = str(tmp_path / 'r2m.npz')
    tally.save_cached_state(mine, r, dict(sample_size=None))
    back = numpy.load(mine, allow_pickle=True)
    assert sorted(back.files) == sorted(theirs.files) == ['constructor', 'count', 'mom2', 'sample_size']
    for k in ('count', 'mom2'):
        assert back[k].dtype == theirs[k].dtype and back[k].shape == theirs[k].shape, k
    assert numpy.array_equal(back['mom2'], theirs['mom2']) and back['sample_size'].dtype == object
    # ... and reads back to the reference's moment (the reference itself read this file so when recording)
    assert is_reference_moment(runningstats.RunningSecondMoment(state=back).moment())
    # a statistic accumulated here (CPU reference path of the class) and cached: the reference accepted the file for
    # the arguments it was written with, refused it for others, and read the moment back identically
    # (the statistic is the recorded one, bit for bit: a matrix product on other host cores may round differently)
    fresh = runningstats.RunningSecondMoment()
    rows = torch.randn(300, 16, generator=torch.Generator().manual_seed(0))
    assert torch.equal(rows, torch.from_numpy(rec['cache/rows']))
    assert torch.allclose(rows.t() @ rows, torch.from_numpy(rec['cache/ours/mom2']), rtol=1e-5, atol=0)
    fresh.mom2, fresh.count = torch.from_numpy(rec['cache/ours/mom2']).clone(), 300
    tally.save_cached_state(str(tmp_path / 'b.npz'), fresh, dict(sample_size=7))
    _same_arrays(numpy.load(str(tmp_path / 'b.npz'), allow_pickle=True), _recorded(rec, 'cache/ours/'))
    assert bool(rec['cache/ref_accepts_7']) and not bool(rec['cache/ref_accepts_8'])     # args mismatch
    assert tally.load_cached_state(str(tmp_path / 'b.npz'), dict(sample_size=7)) is not None
    assert tally.load_cached_state(str(tmp_path / 'b.npz'), dict(sample_size=8)) is None
    assert torch.equal(torch.from_numpy(rec['cache/ref_moment']), fresh.moment())
    # RunningVariance (unit_rs.npz, used by the erase goal): both directions
    numpy.savez(str(tmp_path / 'rs.npz'), **_recorded(rec, 'rv/theirs/'))
    ours = runningstats.RunningVariance(state=numpy.load(str(tmp_path / 'rs.npz'), allow_pickle=True))
    rv_mean, rv_var = torch.from_numpy(rec['rv/mean']), torch.from_numpy(rec['rv/variance'])
    assert torch.allclose(ours.mean(), rv_mean) and torch.allclose(ours.variance(), rv_var)
    _same_arrays(ours.state_dict(), _recorded(rec, 'rv/ours/'))


def test_quantile_cache_interoperates_with_the_reference(tmp_path):
    """unit_rq.npz.  The reference's randomised sketch (utils/runningstats.py:269-620) written by
    its own tally.tally_quantile (recorded in reference_checks.npz with what the reference read out of it) loads here
    and reads out what the reference reads out of the same state; the statistic computed here is written in the
    reference's schema (:422-437), is the state the reference's class and tally cache branch read back when the
    fixture was recorded, and answers within the bound of the class docstring of the exact quantiles -- where the
    reference's own sketch is ~1e-3 away."""
    import numpy
    from rewriting_amd.utils import runningstats, tally
    rec = load_golden('reference_checks')
    gen = torch.Generator().manual_seed(3)
    units, n = 6, 40000
    x = torch.randn(n, units, generator=gen) * torch.linspace(0.5, 3, units) + torch.linspace(-1, 1, units)
    x[:, 2] = x[:, 2].exp()                                     # one skewed unit
    # the sample the fixture was recorded on (the float64 sum's order of additions depends on the host's threads)
    assert torch.equal(x[:16], torch.from_numpy(rec['rq/x_head'])) and abs(x.double().sum().item() - float(rec['rq/x_sum'])) < 1e-3
    data = torch.utils.data.TensorDataset(x)
    qs = torch.tensor([0.0, 1e-4, 0.01, 0.25, 0.5, 0.9, 0.99, 0.999, 1.0])
    exact = torch.from_numpy(numpy.quantile(x.double().numpy(), qs.numpy(), axis=0).T)
    scale = x.std(dim=0)[:, None].double()
    theirs_out = {k: torch.from_numpy(v) for k, v in _recorded(rec, 'rq/theirs_out/').items()}

    # --- theirs -> ours (r = 512: five levels of retained samples, weights 1 .. 16)
    theirs_file = str(tmp_path / 'theirs' / 'unit_rq.npz')
    levels = _recorded(rec, 'rq/theirs/data/')
    dat = dict({k: v for k, v in _recorded(rec, 'rq/theirs/').items() if not k.startswith('data/')},
               sample_size=None, r=512)                         # what utils/tally.py:721-730 saves; the ragged list
    ragged = numpy.empty(len(levels), dtype=object)             # of levels became an object array under the numpy
    ragged[:] = [levels[str(l)] for l in range(len(levels))]    # of the reference's time (numpy 2 refuses to guess)
    os.makedirs(os.path.dirname(theirs_file))
    numpy.savez(theirs_file, **dict(dat, data=ragged))
    st = numpy.load(theirs_file, allow_pickle=True)
    assert len(st['data']) > 2
    mine = tally.tally_quantile(lambda b: 1 / 0, data, batch_size=1000, r=512, cachefile=theirs_file)  # cache hit
    assert mine.size() == n and mine.depth == units
    # (the reference accumulates its cumulative weights in float32, this class in float64: ~1e-5 of the spread)
    close = lambda a, b, tol=1e-4: bool(((a.double() - b.double()).abs() / (scale + b.double().abs())).max() < tol)
    assert close(mine.quantiles(qs), theirs_out['quantiles']), (mine.quantiles(qs) - theirs_out['quantiles']).abs().max()
    assert torch.equal(mine.minmax(), theirs_out['minmax'])
    probe = x[:500].t().contiguous()
    assert torch.allclose(mine.normalize(probe), theirs_out['normalize'], rtol=0, atol=1e-5)
    assert torch.allclose(mine.mean(), theirs_out['mean'], rtol=1e-5, atol=1e-6)
    assert torch.allclose(mine.stdev(), theirs_out['stdev'], rtol=1e-5)
    # ... and written back out it is the same state
    again = mine.state_dict()
    assert sorted(again) == sorted(k for k in st.files if k not in ('sample_size', 'r'))
    for a, b in zip(again['data'], st['data']):
        assert numpy.array_equal(numpy.sort(a, axis=0), numpy.sort(numpy.asarray(b), axis=0))

    # --- ours -> theirs
    ours_file = str(tmp_path / 'ours' / 'unit_rq.npz')
    ours = tally.tally_quantile(lambda b: b, data, batch_size=1000, r=512, cachefile=ours_file)
    levels = ours.state_dict()['data']
    cap = len(levels) - 1
    assert cap == 6 and [len(lv) for lv in levels] == [64] * 6 + [562]     # 32 per tail and level, body in 64s
    assert sum(len(lv) << l for l, lv in enumerate(levels)) == n and sum(len(lv) for lv in levels) <= 1024
    whole = runningstats.RunningQuantile(r=512)
    whole.add(x)
    inner = (qs > 0) & (qs < 1)
    rank_err = lambda q, got: (whole.normalize(got).double() - q).abs()
    # body: below 2^(cap-1) ranks; tails: within 1/32 of the distance to the nearer end (+ half a rank)
    assert rank_err(qs[inner], ours.quantiles(qs[inner])).max() < 2.0 ** (cap - 1) / n + 1e-6
    tails = torch.tensor([2e-4, 1e-3, 3e-3, 0.01, 0.99, 0.997, 0.999, 0.9998])
    assert (rank_err(tails, ours.quantiles(tails)) <= torch.minimum(tails, 1 - tails) / 32 + 1.0 / n).all()
    assert torch.equal(ours.quantiles(torch.tensor([0.0, 1.0])), torch.stack([x.min(0)[0], x.max(0)[0]], dim=1))
    # the levels written are those the reference's tally cache branch read back when recording, and what it read
    _same_arrays({str(l): lv for l, lv in enumerate(levels)}, _recorded(rec, 'rq/ours/data/'), levels=True)
    assert int(rec['rq/back/size']) == n
    assert close(torch.from_numpy(rec['rq/back/quantiles']), ours.quantiles(qs))
    assert torch.allclose(torch.from_numpy(rec['rq/back/normalize']), ours.normalize(probe), rtol=0, atol=1e-5)
    served = tally.tally_quantile(lambda b: 1 / 0, data, batch_size=1000, r=512, cachefile=ours_file)
    assert torch.equal(served.quantiles(qs), ours.quantiles(qs))    # fresh == cached, bit for bit
    # how far each is from the whole sample's quantiles, measured in rank: in the body both are within the
    # reference's nominal 1e-3 (checked against ours' own bound above); in the tails ours is the closer one
    assert rank_err(tails, ours.quantiles(tails)).max() <= rank_err(tails, theirs_out['tails']).max()

    # --- a sample below the retained budget is kept whole: answers exact, and the reference reads the same
    small = runningstats.RunningQuantile(r=4096)
    small.add(x[:3000])
    want = small.quantiles(qs)
    small.compress_()
    assert torch.equal(small.quantiles(qs), want)
    numpy.savez(str(tmp_path / 'small.npz'), **small.state_dict())
    written = dict(numpy.load(str(tmp_path / 'small.npz'), allow_pickle=True))
    written.update({'data/%d' % l: numpy.asarray(lv) for l, lv in enumerate(written.pop('data'))})
    _same_arrays(written, _recorded(rec, 'rq/small/'), levels=True)
    assert close(torch.from_numpy(rec['rq/small_theirs/quantiles']), want)


def test_exact_trajectory_fixture_of_the_full_size_edit_is_consistent_with_the_reference_runs():
    """rw_s256_l8_horsehat_1000_exact.npz (oracle/make_golden.py golden_edit_full_exact): the float64 trajectory of
    configs[2]'s solve.  Checked here: the oracle's float32 arithmetic re-run on the fixture's goal reproduces its
    recorded distance from the exact update at 11 steps; the REFERENCE's own weights (rw_s256_l8_horsehat_1000.npz) are
    within 1e-5 of the exact update through 101 steps and 2.3e-3 / 2.6e-3 away at 2001 (the horizon at which its 8-thread
    and 1-thread runs differ by 2.2e-3 from each other): the bar of the GPU test is 1.5 x that."""
    g, ge = load_golden('rw_s256_l8_horsehat_1000'), load_golden('rw_s256_l8_horsehat_1000_exact')
    sd = oracle_state_dict(build_stylegan(256, 0.5))
    W0 = sd['layer8.sconv.mconv.dconv.weight'].clone()
    mkey = torch.from_numpy(g['mkey'])
    _, _, snaps = R.insert_explicit(W0, torch.from_numpy(g['goal_in_fmap']), torch.from_numpy(g['goal_in_style']),
                                    torch.from_numpy(g['goal_out_fmap']), sd['layer8.sconv.activate.bias'],
                                    sd['layer8.sconv.noise.weight'], mkey, niter=11, piter=10, snapshots=(1, 10, 11))
    for n in (1, 10, 11):
        cos = torch.einsum('oiyx,di->odyx', (snaps[n] - W0)[0].double(), mkey.double())
        d = ((cos - torch.from_numpy(ge['exact_dW_%d_cos' % n])).norm() / float(ge['exact_dW_%d_norm' % n])).item()
        # (the recorded figure is the distance of the WHOLE tensor; its component along the direction cannot be larger)
        assert d < 1e-4 and d <= float(ge['restatement_f32_vs_exact_%d' % n]) + 1e-7, (n, d)
        if n % 10 == 1:                      # a projection step (it % piter == 0): the update lies along the direction
            assert float(ge['exact_off_direction_%d' % n]) < 1e-6      # (the direction is unit in float32 only)
    for tag in ('1', '10', '11', '100', '101'):
        ref_cos = torch.from_numpy(g['dW_%s_cos' % tag]).double()
        d = ((ref_cos - torch.from_numpy(ge['exact_dW_%s_cos' % tag])).norm() / float(ge['exact_dW_%s_norm' % tag])).item()
        assert d < 1e-5 and abs(d - float(ge['reference_vs_exact_%s' % tag])) < 1e-9, (tag, d)
    d8, d1 = float(ge['reference_vs_exact_2001_t8']), float(ge['reference_vs_exact_2001_t1'])
    assert 1e-3 < d8 < 5e-3 and 1e-3 < d1 < 5e-3
    # the two reference runs are as far from each other as each is from the exact update: float32's chaos, not a bug
    assert abs(float(g['self_scatter_2001']) - 2.2e-3) < 1e-3
