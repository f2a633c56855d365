"""TEST INFRASTRUCTURE -- the checks of the key statistics (csrc/rw_stats.hip behind hip.second_moment_accumulate and
hip.channel_sums, utils/runningstats.py, samples.FeatureStatistics, tally.tally_second_moment), shared by the GPU test
(tests/test_gpu_key_statistics.py) and by its host twin on the emulation (tests/test_key_statistics_emulated.py).

Two kinds of case:

* exact     small integers in {-3 .. 3} stored as float32, with 9 rows < 2^24 (81 rows where fourth powers are summed)
  asserted before anything is launched: every product and every partial sum is then an integer below 2^24, exact in
  float32 in ANY order, so the result must EQUAL the integer result (torch.equal, no tolerance).  A dropped or doubled
  row, a wrong tail, tile or mirror, a stale slab of the split-K workspace: all of them change an integer.
* accuracy  what integers cannot see ({-3 .. 3} is exact in f16 and bf16 too): operands or accumulators of reduced
  precision.  Data of the key maps' own class (a leaky ReLU of a normal sample, times a per-channel gain exp(1.5 randn):
  the channels span orders of magnitude).  Measure: e = max_ij |got - want64| / sqrt(want_ii want_jj), the error whitening
  sees, which the large channels cannot hide.  Bar: e_hip <= 4 max(e_ref, e_seq), both yardsticks computed in float32 on
  the host from the same data -- e_ref torch's zeros.addmm_(a.t(), a) (the arithmetic of the CPU branch), e_seq a plain
  accumulation of 16-row blocks in row order (the least accurate order a correct float32 kernel could use; split-K only
  shortens it).  The margin of 4 allows for another order of summation within and across the chunks.  Operands rounded
  to f16 sit 4.7 to 260 times above that bar on these shapes, to bf16 31 to 2500 times (test_key_statistics_emulated.py
  seeds both and asserts 2.5 and 25 times).

RunningVariance: per channel, the relative error of variance() against the same class fed float64, bar 16 times the worst
of the same class fed the same float32 batches on the host (two passes: the reference's arithmetic).  16: the device
reads the map once and centres on a pivot p taken from the channel's first samples instead of the batch mean, which costs
a factor 1 + (mean - p)^2 / var -- about 10 for a single sample that lies three deviations out; the margin for a form
centred on the mean itself would be 4.  mean(): |d| / sqrt(mean^2 + var) <= 4 max(the host's worst, 2^-24) -- the floor
is one rounding of the result itself.
"""
import functools
import json
import os
import types

import numpy
import torch

U = 2.0 ** -24
MARGIN = 4
VARIANCE_MARGIN = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the report
def report(section, value):
    """key_statistics.json in the directory RW_REPORT_DIR names (default: test_reports/, which git ignores)"""
    directory = os.environ.get('RW_REPORT_DIR') or os.path.join(ROOT, 'test_reports')
    path = os.path.join(directory, 'key_statistics.json')
    os.makedirs(directory, exist_ok=True)
    data = {}
    if os.path.isfile(path):
        with open(path) as f:
            data = json.load(f)
    data[section] = value
    with open(path, 'w') as f:
        json.dump(data, f, indent=1, sort_keys=True)
    return path


# ------------------------------------------------------------------------------------------------ exact cases
def _case(shape, why):
    nchw = len(shape) == 4
    rows = shape[0] * shape[2] * shape[3] if nchw else shape[0]
    return types.SimpleNamespace(shape=tuple(shape), nchw=nchw, rows=rows, channels=shape[1], why=why)


EXACT = {
    # (rows, C)
    'r1x4': _case((1, 4), 'a single row (add of a 1-D key), one float4 of one tile'),
    'r15x64': _case((15, 64), 'one chunk, its last row zero-filled'),
    'r17x64': _case((17, 64), 'two chunks, the second holds one row'),
    'r130x132': _case((130, 132), '128-wide tiles, 4 channels in the last; chunks / 8 = 1'),
    'r2063x68': _case((2063, 68), '64-wide tiles, 4 channels in the last; 129 chunks over 16 uneven slices'),
    'r1000x320': _case((1000, 320), '128-wide tiles, half a tile last; 63 chunks over 7 slices'),
    'r4099x512': _case((4099, 512), '257 chunks over 32 slices, 3 rows in the last chunk'),
    'r50x2048': _case((50, 2048), '136 tile pairs, one slice'),
    'r33x6': _case((33, 6), 'C % 4 != 0: channels padded by the wrapper'),
    # (b, c, h, w), the kernel's own layout
    'n1x3x4x4': _case((1, 3, 4, 4), 'three channels, one chunk'),
    'n3x67x4x8': _case((3, 67, 4, 8), 'two 64-wide tiles, 3 channels in the second, C % 4 != 0'),
    'n2x130x4x4': _case((2, 130, 4, 4), 'two 128-wide tiles, 2 channels in the second'),
    'n2x192x8x6': _case((2, 192, 8, 6), 'half a 128-wide tile last; a chunk crosses rows of the image'),
    'n1x512x8x8': _case((1, 512, 8, 8), 'full tiles, 4 chunks'),
    # hw % 16 != 0: copied to rows by the wrapper
    'n2x8x5x7': _case((2, 8, 5, 7), 'the row-copy fallback'),
    'n2x6x5x7': _case((2, 6, 5, 7), 'the row-copy fallback with C % 4 != 0'),
}
SEQUENCE = ['r4099x512', 'r17x64', 'r130x132', 'r4099x512']


def assert_exact_admissible(rows, bound=3, adds=1, fourth=False):
    """every sum of ``adds`` maps of ``rows`` rows is an integer below 2^24"""
    term = bound ** 4 if fourth else bound ** 2
    assert term * rows * adds < 2 ** 24, (rows, bound, adds, fourth)


def rows_of(a, nchw):
    return a.permute(0, 2, 3, 1).reshape(-1, a.shape[1]) if nchw else a.reshape(-1, a.shape[-1])


@functools.lru_cache(maxsize=None)
def exact_problem(name):
    """(a float32, mom2 int64, channel sums int64 (2, C), the same of the squared input): computed once, never modified.
    The products are formed in float64, where integers below 2^53 are exact, and stored as int64."""
    c = EXACT[name]
    gen = torch.Generator().manual_seed(sum(c.shape) * 31 + len(c.shape))
    a = torch.randint(-3, 4, c.shape, generator=gen).float()
    r = rows_of(a, c.nchw).double()
    mom2 = (r.t() @ r).long()
    sq = r * r
    sums = torch.stack([r.sum(0), sq.sum(0)]).long()
    sums_sq = torch.stack([sq.sum(0), (sq * sq).sum(0)]).long()
    assert mom2.diagonal().equal(sums[1]) and int(sums_sq[1].max()) <= 81 * c.rows
    return a, mom2, sums, sums_sq


def _same(got, want_int):
    """float32 result == integer result, with no tolerance (the comparison itself in float64, which holds both)"""
    return torch.equal(got.detach().cpu().double(), want_int.double())


def _accumulate(a, nchw, device, mom2=None):
    from rewriting_amd import hip
    if mom2 is None:
        mom2 = torch.zeros(a.shape[1], a.shape[1], device=device)
    hip.second_moment_accumulate(mom2, a, nchw=nchw)
    return mom2


def check_exact(name, device):
    """the assertions of one exact case; returns the names of those that fail"""
    from rewriting_amd import hip
    from rewriting_amd.utils import runningstats
    c = EXACT[name]
    a, want, sums, sums_sq = exact_problem(name)
    assert_exact_admissible(c.rows, adds=2)
    assert_exact_admissible(c.rows, fourth=True)
    d = a.to(device)
    bad = []

    def hold(check, ok):
        if not ok:
            bad.append(check)
    # through the drop-in class: one add from zero, a second onto the now non-zero mom2, the count
    stat = runningstats.RunningSecondMoment()
    add = stat.add_nchw if c.nchw else stat.add
    add(d[0] if c.shape == (1, 4) else d)                 # (1, 4): as a 1-D key
    first = stat.mom2.clone()
    hold('exact', _same(first, want))
    hold('symmetric', torch.equal(first, first.t()))
    add(d)
    hold('exact_onto_nonzero', _same(stat.mom2, 2 * want))
    hold('count', stat.count == 2 * c.rows and stat.size() == 2 * c.rows)
    # moment() divides on the device, where a quotient by a scalar may be a product by its reciprocal: two roundings
    mean = want.double() / c.rows
    hold('moment', bool(((stat.moment().cpu().double() - mean).abs() <= 2.0 ** -23 * mean.abs()).all()))
    # two identical calls of the wrapper from zero
    again = _accumulate(d, c.nchw, device), _accumulate(d, c.nchw, device)
    hold('repeatable', torch.equal(again[0], again[1]) and torch.equal(again[0], first))
    # the channel sums, in this layout and in the other one
    other = rows_of(d, True).contiguous() if c.nchw else None
    for square, ref in ((False, sums), (True, sums_sq)):
        hold('sums_square%d' % square, _same(hip.channel_sums(d, nchw=c.nchw, square_input=square), ref))
        if other is not None:
            hold('sums_rows_square%d' % square, _same(hip.channel_sums(other, nchw=False, square_input=square), ref))
    return bad


def check_sequence(device):
    """Large, small, small, large on one device with no synchronise between them: the cached workspace is reused and the
    slabs of the large launch lie behind those of the small ones.  Then the same call on a side stream."""
    got = []
    for name in SEQUENCE:
        c = EXACT[name]
        assert_exact_admissible(c.rows)
        got.append(_accumulate(exact_problem(name)[0].to(device), c.nchw, device))
    bad = [name + '@%d' % i for i, (name, m) in enumerate(zip(SEQUENCE, got)) if not _same(m, exact_problem(name)[1])]
    if not torch.equal(got[0], got[-1]):
        bad.append('first_vs_last')
    if torch.device(device).type == 'cuda':
        a = exact_problem(SEQUENCE[0])[0].to(device)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = _accumulate(a, False, device)
            small = _accumulate(exact_problem('r17x64')[0].to(device), False, device)
        again = _accumulate(a, False, device)                   # the default stream, while the side stream may still run
        side.synchronize()
        if not (torch.equal(on_side, got[0]) and torch.equal(again, got[0]) and _same(small, exact_problem('r17x64')[1])):
            bad.append('side_stream')
    return bad


def check_past_31_bits(device):
    """A (2^22 + 16, 512) map of {-1, 0, 1}: more than 2^31 elements, every sum at most 2^22 + 16 < 2^24.  The whole map
    against the sum of its halves (each below 2^31 elements, the same kernel), and the diagonal against the count of the
    non-zero entries; no float64 product of the map is formed."""
    rows, channels = 2 ** 22 + 16, 512
    half = rows // 2
    assert rows * channels > 2 ** 31 > half * channels and rows - half == half
    assert_exact_admissible(rows, bound=1)
    a = torch.empty(rows, channels, device=device)
    halves = a[:half], a[half:]
    for h in halves:
        h.random_(-1, 2)
    whole = _accumulate(a, False, device)
    parts = [_accumulate(h, False, device) for h in halves]
    nonzero = sum((h != 0).sum(0) for h in halves)
    bad = []
    if not torch.equal(whole, parts[0] + parts[1]):
        bad.append('whole_vs_halves')
    if not _same(whole.diagonal(), nonzero.cpu()):
        bad.append('diagonal')
    if not (int(nonzero.min()) > rows // 2 and bool((parts[1].diagonal() > half // 2).all())):
        bad.append('data')          # two thirds of the entries are non-zero, in the upper half of the map as well
    return bad


# ------------------------------------------------------------------------------------------------ accuracy cases
ACCURACY = {
    'r10240x512': _case((10240, 512), 'the key map of the edited layer, as rows'),
    'n10x512x32x32': _case((10, 512, 32, 32), 'the same map as the generator leaves it'),
    'r2063x68': _case((2063, 68), 'partial 64-wide tile, uneven slices'),
    'r130x132': _case((130, 132), 'partial 128-wide tile, one or two slices'),
    'r50x2048': _case((50, 2048), 'Inception features, one slice'),
    'r16384x64': _case((16384, 64), 'one tile, the longest sums per slice'),
}


def key_like(shape, seed, channel_dim=1):
    """randn through a leaky ReLU (slope 0.2, gain sqrt 2), times a per-channel gain exp(1.5 randn)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.leaky_relu(torch.randn(shape, generator=gen), 0.2) * 2 ** 0.5
    gain = torch.exp(1.5 * torch.randn(shape[channel_dim], generator=gen))
    view = [1] * len(shape)
    view[channel_dim] = -1
    return (x * gain.view(view)).contiguous()


def product_ref(r):
    return torch.zeros(r.shape[1], r.shape[1]).addmm_(r.t(), r)


def product_seq(r, block=16):
    acc = torch.zeros(r.shape[1], r.shape[1])
    for i in range(0, r.shape[0], block):
        acc += r[i:i + block].t() @ r[i:i + block]
    return acc


def normalised_error(got, want):
    d = want.diagonal().sqrt()
    return ((got.detach().cpu().double() - want).abs() / torch.outer(d, d)).max().item()


def frobenius_error(got, want):
    return ((got.detach().cpu().double() - want).norm() / want.norm()).item()


@functools.lru_cache(maxsize=None)
def _accuracy_rows(shape):
    """(rows float32, want float64, e_ref, e_seq): once per data set, shared by the two layouts of the same map"""
    a = key_like(shape, seed=shape[0] + shape[1])
    r64 = a.double()
    want = r64.t() @ r64
    return a, want, normalised_error(product_ref(a), want), normalised_error(product_seq(a), want)


def accuracy_problem(name):
    """(the sample in the case's layout, want float64, e_ref, e_seq)"""
    c = ACCURACY[name]
    a, want, e_ref, e_seq = _accuracy_rows((c.rows, c.channels))
    if c.nchw:
        b, ch, h, w = c.shape
        a = a.reshape(b, h, w, ch).permute(0, 3, 1, 2).contiguous()
    return a, want, e_ref, e_seq


def judge(e_hip, e_ref, e_seq):
    return dict(e_hip=e_hip, e_ref=e_ref, e_seq=e_seq, ratio=e_hip / max(e_ref, e_seq))


def check_accuracy(name, device, operand=None):
    """(figures, passed).  ``operand``: a rounding applied to the sample before it is handed over -- how the host twin
    shows that reduced-precision operands miss the bar."""
    c = ACCURACY[name]
    a, want, e_ref, e_seq = accuracy_problem(name)
    d = a if operand is None else operand(a)
    got = _accumulate(d.to(device), c.nchw, device)
    fig = judge(normalised_error(got, want), e_ref, e_seq)
    fig['frobenius'] = frobenius_error(got, want)
    return fig, fig['e_hip'] <= MARGIN * max(e_ref, e_seq)


# ------------------------------------------------------------------------------------------------ FeatureStatistics
FEATURE_BATCHES = (50, 50, 37)


@functools.lru_cache(maxsize=None)
def feature_problem(features):
    """(rows float32, cov float64 by numpy.cov, e_ref, e_seq).  The yardsticks do what FeatureStatistics does on the
    device -- a float32 product per batch, float64 across the batches and in mean_cov -- with the two host products."""
    rows = key_like((sum(FEATURE_BATCHES), features), seed=features)
    r64 = rows.double()
    cov = torch.from_numpy(numpy.cov(r64.numpy(), rowvar=False))
    n = rows.shape[0]
    mu = r64.sum(0) / n

    def through(product):
        outer = sum(product(b).double() for b in rows.split(FEATURE_BATCHES))
        return normalised_error((outer - n * torch.outer(mu, mu)) / (n - 1), cov)
    return rows, cov, through(product_ref), through(product_seq)


def check_features(features, device):
    from rewriting_amd import samples
    rows, cov, e_ref, e_seq = feature_problem(features)
    stat = samples.FeatureStatistics()
    for b in rows.split(FEATURE_BATCHES):
        stat.add(b.to(device))
    mu, sigma = stat.mean_cov()
    assert stat.count == rows.shape[0] and sigma.dtype == numpy.float64
    fig = judge(normalised_error(torch.from_numpy(sigma), cov), e_ref, e_seq)
    fig['mean'] = float(numpy.abs(mu - rows.double().mean(0).numpy()).max() / rows.abs().max())
    if features % 4:
        # the float64 branch: sums of 137 products, each side of outer - n mu mu^T within rows * 2^-53 of its own
        # magnitude, which is <= 2 n sqrt(cov_ii cov_jj) for this data (E x^2 = 1.24 var); 16 covers both sides, the
        # factor 2, 1 / (n - 1) and numpy's own rounding
        return fig, fig['e_hip'] <= 16 * rows.shape[0] * 2.0 ** -53
    return fig, fig['e_hip'] <= MARGIN * max(e_ref, e_seq)


# ------------------------------------------------------------------------------------------------ tally_second_moment
def check_tally(device):
    from rewriting_amd.utils import tally
    gen = torch.Generator().manual_seed(25)
    maps = torch.randint(-3, 4, (25, 64, 4, 4), generator=gen).float()
    assert_exact_admissible(25 * 16)
    r = rows_of(maps, True).double()
    seen = []

    def compute(batch):
        seen.append(batch.shape[0])
        return batch.to(device)
    stat = tally.tally_second_moment(compute, maps, batch_size=10, nchw=True)
    assert seen == [10, 10, 5], seen
    bad = []
    if not _same(stat.mom2, (r.t() @ r).long()):
        bad.append('exact')
    if stat.count != 400:
        bad.append('count')
    if stat.mom2.device.type != 'cpu':
        bad.append('device')
    return bad


# ------------------------------------------------------------------------------------------------ RunningVariance
RATIOS = (0.0, 1.0, 10.0, 30.0, 100.0)
VARIANCE_BATCHES = {True: ((8, 32, 32), (8, 32, 32), (3, 32, 32)), False: ((8192,), (8192,), (3072,))}


@functools.lru_cache(maxsize=None)
def variance_problem(nchw, square_input=False):
    """(batches float32, mean and variance of the class fed float64, the worst errors of the class fed float32 on the
    host, per ratio).  Ten channels: every mean / std of RATIOS at two scales of std."""
    from rewriting_amd.utils import runningstats
    gen = torch.Generator().manual_seed(7 + nchw)
    ratio = torch.tensor(RATIOS + RATIOS)
    std = torch.tensor([1.0] * len(RATIOS) + [0.037] * len(RATIOS))
    batches = []
    for lead in VARIANCE_BATCHES[nchw]:
        x = torch.randn(int(numpy.prod(lead)), len(ratio), generator=gen)
        x = ((x + ratio) * std).float()
        if nchw:
            x = x.reshape(lead[0], lead[1], lead[2], -1).permute(0, 3, 1, 2).contiguous()
        batches.append(x)

    def through(dtype):
        # the CPU branch of the class, also while the emulation makes host tensors count as device tensors
        from rewriting_amd import hip
        seen, hip.on_device = hip.on_device, lambda t: bool(t.is_cuda)
        try:
            stat = runningstats.RunningVariance()
            for b in batches:
                stat.add(b.to(dtype), nchw=nchw, square_input=square_input)
        finally:
            hip.on_device = seen
        return stat.mean().double(), stat.variance().double()
    mean64, var64 = through(torch.float64)
    mean32, var32 = through(torch.float32)
    return batches, mean64, var64, variance_errors(mean32, var32, mean64, var64)


def variance_errors(mean, var, mean64, var64):
    """(per-channel normalised error of the mean, per-channel relative error of the variance)"""
    mean, var = mean.detach().cpu().double(), var.detach().cpu().double()
    return ((mean - mean64).abs() / (mean64 ** 2 + var64).sqrt()), ((var - var64).abs() / var64)


def check_variance(nchw, device, square_input=False):
    """(figures, failed checks): three batches through RunningVariance.add on ``device``"""
    from rewriting_amd.utils import runningstats
    batches, mean64, var64, (mean_cpu, var_cpu) = variance_problem(nchw, square_input)
    stat = runningstats.RunningVariance()
    for b in batches:
        stat.add(b.to(device), nchw=nchw, square_input=square_input)
    mean_dev, var_dev = variance_errors(stat.mean(), stat.variance(), mean64, var64)
    rows = sum(b.numel() // len(mean64) for b in batches)
    fig = {'mean_hip': mean_dev.max().item(), 'mean_cpu': mean_cpu.max().item(),
           'variance_hip': var_dev.max().item(), 'variance_cpu': var_cpu.max().item(),
           'variance_ratio': var_dev.max().item() / var_cpu.max().item(), 'per_ratio': {}}
    n = len(RATIOS)
    for i, r in enumerate(RATIOS):
        fig['per_ratio']['%g' % r] = dict(variance_hip=var_dev[[i, i + n]].max().item(),
                                          variance_cpu=var_cpu[[i, i + n]].max().item())
    bad = []
    if stat.size() != rows or stat.batchcount != len(batches):
        bad.append('count')
    if not fig['mean_hip'] <= MARGIN * max(fig['mean_cpu'], U):
        bad.append('mean')
    if not fig['variance_hip'] <= VARIANCE_MARGIN * fig['variance_cpu']:
        bad.append('variance')
    if not torch.equal(stat.stdev(), stat.variance().sqrt()):
        bad.append('stdev')
    return fig, bad
