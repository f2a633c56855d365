"""The device-side Search on the MI355X: SeqStyleGanRewriter at layer 6 of the 64^2 generator, 40 seeds (key maps
40 x 512 x 16 x 16, four launches of ten seeds), with the resident index and without, against float64 and against the
torch expression of ranking_for_key.

Rankings are checked in their tie-class form (tests/search_checks.py: check_ranking): on this model and seed set the
error bar b of a peak is 4e-4 to 8e-4 (by key) and neighbouring peaks among the top 14 are as close as 1.2e-4, so float32
cannot order them and an exact-order assertion would be wrong."""
import pytest
import torch

from tests.search_checks import check_ranking, exact_response, make_rewriter, pixel_keys, same_answer

pytestmark = pytest.mark.gpu

SIZE, NSEEDS, LAYER, TOPK, NKEYS = 64, 40, 6, 12, 3
Q = [0.5, 0.99, 0.999]


def _rewriter(**kw):
    gw = make_rewriter('cuda', SIZE, NSEEDS, LAYER, **kw)
    gw.sweep_batch = 10
    return gw


@pytest.fixture(scope='module')
def setup():
    """(rewriter with its index, keys, swept answer, indexed answer, exact peaks (N, K), their error bars (N, K))"""
    gw = _rewriter()
    assert gw.search_index is None
    index = gw.build_search_index()
    assert tuple(index.maps.shape) == (NSEEDS, 512, 16, 16) and index.maps.device == gw.device
    assert index.launches == [(0, 10), (10, 10), (20, 10), (30, 10)] and index.nbytes() == NSEEDS * 512 * 256 * 4
    keys = pixel_keys(index.maps, NKEYS)
    indexed = gw.search(keys, k=TOPK)
    assert gw.search_index is index
    gw.drop_search_index()
    swept = gw.search(keys, k=TOPK)
    gw.search_index = index
    heat, bound = exact_response(index.maps, keys)
    return gw, keys, swept, indexed, heat.flatten(2).amax(2), bound.flatten(2).amax(2)


def test_index_and_sweep_give_identical_answers(setup):
    gw, keys, swept, indexed, _, _ = setup
    assert torch.equal(indexed[0], swept[0]) and torch.equal(indexed[1], swept[1])
    assert torch.equal(indexed[2].quantiles(Q), swept[2].quantiles(Q))
    assert indexed[0].shape == indexed[1].shape == (NKEYS, TOPK) and not indexed[0].is_cuda
    assert indexed[2].size() == swept[2].size() == NSEEDS * 256 and indexed[2].depth == NKEYS


def test_search_against_float64(setup):
    gw, keys, swept, indexed, exact_peak, peak_bound = setup
    print('largest error bar of a peak: %.3g' % peak_bound.max().item())
    for j in range(NKEYS):
        check_ranking(indexed[0][j], indexed[1][j], exact_peak[:, j], peak_bound[:, j], TOPK)
    assert indexed[0][0, 0].item() == 1          # a pixel's own key finds its seed
    # the quantile statistic holds every response: its extremes are the extremes of the exact heat maps
    heat, bound = exact_response(gw.search_index.maps, keys)
    mm = indexed[2].minmax().double()
    for j in range(NKEYS):
        assert abs(mm[j, 1].item() - heat[:, j].max().item()) <= bound[:, j].max().item()
        assert abs(mm[j, 0].item() - heat[:, j].min().item()) <= bound[:, j].max().item()


def test_search_against_ranking_for_key(setup):
    gw, keys, swept, indexed, exact_peak, peak_bound = setup
    assert not gw.device_search
    for j in range(NKEYS):
        numbers, rq = gw.ranking_for_key(keys[j], k=TOPK)
        check_ranking(numbers, None, exact_peak[:, j], peak_bound[:, j], TOPK)
        b = peak_bound[:, j].max().item()
        assert rq.size() == indexed[2].size() == NSEEDS * 256
        # the largest response is the first peak: the two paths agree on it within 2b
        assert abs(rq.minmax()[0, 1].item() - indexed[1][j, 0].item()) <= 2 * b
        got, want = indexed[2].quantiles(Q)[j].double(), rq.quantiles(Q)[0].double()
        print('key %d: quantiles %s against %s, b = %.3g' % (j, got.tolist(), want.tolist(), b))


def test_device_search_answers_ranking_for_key(setup):
    gw, keys, swept, indexed, _, _ = setup
    ref_numbers, ref_rq = gw.ranking_for_key(keys[1], k=TOPK)
    gw.device_search = True
    try:
        numbers, rq = gw.ranking_for_key(keys[1], k=TOPK)
    finally:
        gw.device_search = False
    assert torch.equal(numbers, indexed[0][1]) and torch.equal(rq.quantiles(Q)[0], indexed[2].quantiles(Q)[1])
    assert numbers.shape == ref_numbers.shape == (TOPK,) and numbers.dtype == ref_numbers.dtype
    assert numbers.device == ref_numbers.device
    assert type(rq) is type(ref_rq) and rq.size() == ref_rq.size() and rq.depth == ref_rq.depth == 1
    assert rq.quantiles(Q).shape == ref_rq.quantiles(Q).shape and rq.quantiles(Q).dtype == ref_rq.quantiles(Q).dtype
    assert make_rewriter('cuda', SIZE, 10, LAYER, device_search=True).device_search


def test_the_index_survives_an_edit_and_is_dropped_with_the_context():
    gw = _rewriter()
    index = gw.build_search_index()
    keys = pixel_keys(index.maps, NKEYS)
    before = gw.search(keys, k=TOPK)
    with torch.no_grad():
        goal_in = gw.context_model(gw.get_z(0))
        goal_out = gw.target_model(gw.context_model(gw.get_z(1)))
    w0 = gw.target_weights().detach().clone()
    gw.insert(goal_in, goal_out, keys[:1], niter=1, piter=10, lr=0.05)
    assert not torch.equal(gw.target_weights().detach(), w0)
    assert same_answer(gw.search(keys, k=TOPK), before) and gw.search_index is index
    param = next(p for n, p in gw.context_model.named_parameters() if 'layer2' in n and p.dim() > 1)
    with torch.no_grad():
        param.mul_(1.25)
    after = gw.search(keys, k=TOPK)
    assert gw.search_index is None
    assert not same_answer(after, before)
    assert same_answer(after, gw.search(keys, k=TOPK))           # a fresh un-indexed search


def test_an_index_over_the_budget_is_refused():
    gw = _rewriter()
    with pytest.raises(ValueError, match=str(NSEEDS * 512 * 256 * 4)):
        gw.build_search_index(max_bytes=1 << 20)
    assert gw.search_index is None
