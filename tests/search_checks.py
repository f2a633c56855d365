"""What tests/test_search_host.py (kernel layer emulated, CPU) and tests/test_gpu_search.py share: the rewriter under
test, the float64 reference of a key response with its derived error bar, and the tie-class form of a top-k check."""
import torch

from tests.conftest import build_stylegan


def make_rewriter(device, size, nseeds, layernum, **kw):
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import zdataset
    model = build_stylegan(size, 1.0, device=device)
    zds = zdataset.z_dataset_for_model(model, size=nseeds)
    return ganrewrite.SeqStyleGanRewriter(model, zds, layernum, cachedir=None, **kw)


def exact_response(acts, keys):
    """(heat, bound) in float64 on the CPU: heat[b][k] = sum_c keys[k][c] * acts[b][c] and, per element, the most a
    float32 sum of C products can differ from it in any order, with or without FMA:
    1.01 * C * 2^-24 * sum_c |k_c * a_c| + 1e-30."""
    a, k = acts.detach().double().cpu(), keys.detach().double().cpu().reshape(-1, acts.shape[1])
    heat = torch.einsum('kc,bchw->bkhw', k, a)
    bound = 1.01 * a.shape[1] * 2.0 ** -24 * torch.einsum('kc,bchw->bkhw', k.abs(), a.abs()) + 1e-30
    return heat, bound


def pixel_keys(maps, n):
    """n query keys (n, C): key-map vectors of spread-out pixels of spread-out seeds, scaled to unit length."""
    nseeds, _, h, w = maps.shape
    keys = torch.stack([maps[(7 * i + 1) % nseeds, :, (3 * i + 2) % h, (5 * i + 1) % w] for i in range(n)])
    return (keys / keys.norm(dim=1, keepdim=True)).contiguous()


def check_ranking(numbers, peaks, exact_peak, peak_bound, k):
    """numbers (k,) [and peaks (k,), or None] of one key against that key's exact per-seed peaks (N,) float64 and the
    error bar of each seed's peak, peak_bound (N,) = the largest bar among the seed's pixels (two maps that differ by at
    most e everywhere have maxima that differ by at most e).  Every returned peak is within its seed's bar of the exact
    one and the peaks come sorted; with kth the k-th largest exact peak and b the largest bar, the returned set holds
    every seed above kth + 2b and none below kth - 2b (seeds closer to kth are a tie class: float32 cannot order them)."""
    numbers = numbers.cpu()
    assert numbers.shape == (k,) and numbers.dtype == torch.int64
    assert len(set(numbers.tolist())) == k
    if peaks is not None:
        peaks = peaks.double().cpu()
        assert peaks.shape == (k,)
        err = (peaks - exact_peak[numbers]).abs()
        assert (err <= peak_bound[numbers]).all(), (err / peak_bound[numbers]).max()
        assert (peaks[:-1] >= peaks[1:]).all()
    b = peak_bound.max()
    kth = exact_peak.topk(k)[0][-1]
    must = set(torch.nonzero(exact_peak > kth + 2 * b).flatten().tolist())
    never = set(torch.nonzero(exact_peak < kth - 2 * b).flatten().tolist())
    got = set(numbers.tolist())
    assert must <= got, sorted(must - got)
    assert not (never & got), sorted(never & got)


def same_answer(x, y):
    """Two results of search(): identical seed numbers and peaks, equal quantiles."""
    q = [0.5, 0.99, 0.999]
    return (torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2].size() == y[2].size()
            and torch.equal(x[2].quantiles(q), y[2].quantiles(q)))
