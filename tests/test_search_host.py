"""Host logic of the device-side Search (rewrite/search.py) on the CPU: the kernel layer is the emulation of
tests/hip_emulation.py plus a torch stand-in for hip.key_response defined here (key by key, so that a key's rows do
not depend on its neighbours -- the property the kernel documents).  The kernel itself is tested by
tests/test_gpu_key_response.py, the same host assertions on the device by tests/test_gpu_search.py."""
import pytest
import torch

from tests.search_checks import check_ranking, exact_response, make_rewriter, pixel_keys, same_answer

SIZE, NSEEDS, LAYER, TOPK = 32, 20, 4, 5


def _key_response(acts, keys, want_peak=True):
    assert acts.is_contiguous() and acts.dtype == torch.float32
    keys = keys.reshape(-1, acts.shape[1])
    heat = torch.stack([torch.einsum('c,bchw->bhw', key, acts) for key in keys], dim=1)
    return heat, (heat.flatten(2).amax(2) if want_peak else None)


@pytest.fixture
def emulated(emulated_hip, monkeypatch):
    from rewriting_amd import hip
    calls = []

    def spy(acts, keys, want_peak=True):
        calls.append(acts.shape[0])
        return _key_response(acts, keys, want_peak)
    monkeypatch.setattr(hip, 'key_response', spy, raising=False)
    return calls


def _rewriter(**kw):
    gw = make_rewriter('cpu', SIZE, NSEEDS, LAYER, **kw)
    gw.sweep_batch = 10          # two launches of ten seeds
    return gw


def _forwards(gw):
    count = []
    handle = gw.context_model.register_forward_hook(lambda *a: count.append(1))
    return count, handle


def test_index_and_sweep_give_the_same_answer(emulated):
    gw = _rewriter()
    assert gw.search_index is None and not gw.device_search
    index = gw.build_search_index()
    assert gw.search_index is index and index.launches == [(0, 10), (10, 10)]
    assert index.maps.shape == (NSEEDS,) + tuple(gw.k_shape[1:]) and index.nbytes() == index.maps.numel() * 4
    keys = pixel_keys(index.maps, 3)
    gw.drop_search_index()
    assert gw.search_index is None
    swept = gw.search(keys, k=TOPK)
    assert emulated == [10, 10]                         # the sweep's launches
    gw.build_search_index()
    count, handle = _forwards(gw)
    del emulated[:]
    indexed = gw.search(keys, k=TOPK)
    handle.remove()
    assert not count and emulated == [10, 10]           # no forward; the same pieces as the sweep
    assert gw.search_index is not None
    assert same_answer(indexed, swept)
    numbers, peaks, rq = indexed
    assert numbers.shape == peaks.shape == (3, TOPK) and numbers.dtype == torch.int64
    assert rq.size() == NSEEDS * gw.k_shape[2] * gw.k_shape[3] and rq.depth == 3
    heat, bound = exact_response(gw.search_index.maps, keys)
    for j in range(3):
        check_ranking(numbers[j], peaks[j], heat[:, j].flatten(1).amax(1), bound[:, j].flatten(1).amax(1), TOPK)
    # a pixel's own key finds its seed
    assert numbers[0, 0].item() == 1
    # a single key: the same row, without the key axis
    one = gw.search(keys[1], k=TOPK)
    assert torch.equal(one[0], numbers[1]) and torch.equal(one[1], peaks[1]) and one[2].depth == 1
    assert torch.equal(one[2].quantiles([0.5, 0.99]), rq.quantiles([0.5, 0.99])[1:2])


def test_more_keys_than_a_group(emulated):
    gw = _rewriter()
    gw.build_search_index()
    keys = pixel_keys(gw.search_index.maps, 11)
    all_ = gw.search(keys, k=TOPK)
    first, rest = gw.search(keys[:8], k=TOPK), gw.search(keys[8:], k=TOPK)
    assert all_[0].shape == (11, TOPK) and all_[2].depth == 11
    assert torch.equal(all_[0], torch.cat([first[0], rest[0]])) and torch.equal(all_[1], torch.cat([first[1], rest[1]]))
    q = [0.5, 0.99, 0.999]
    assert torch.equal(all_[2].quantiles(q), torch.cat([first[2].quantiles(q), rest[2].quantiles(q)]))


def test_an_edit_of_the_target_keeps_the_index_and_a_change_of_the_context_drops_it(emulated):
    gw = _rewriter()
    gw.build_search_index()
    keys = pixel_keys(gw.search_index.maps, 2)
    before = gw.search(keys, k=TOPK)
    with torch.no_grad():
        goal_in = gw.context_model(gw.get_z(0))
        goal_out = gw.target_model(gw.context_model(gw.get_z(1)))
    w0 = gw.target_weights().detach().clone()
    gw.insert(goal_in, goal_out, keys[:1], niter=1, piter=10, lr=0.05)
    assert not torch.equal(gw.target_weights().detach(), w0)
    count, handle = _forwards(gw)
    assert same_answer(gw.search(keys, k=TOPK), before)
    assert gw.search_index is not None and not count
    gw.zero(keys[:1])
    assert same_answer(gw.search(keys, k=TOPK), before)
    assert gw.search_index is not None and not count
    # an earlier layer changes in place: the next query drops the index and sweeps
    name, param = next((n, p) for n, p in gw.context_model.named_parameters() if 'layer2' in n and p.dim() > 1)
    with torch.no_grad():
        param.mul_(1.25)
    after = gw.search(keys, k=TOPK)
    handle.remove()
    assert gw.search_index is None and len(count) == 2, name
    assert not same_answer(after, before)
    assert same_answer(after, gw.search(keys, k=TOPK))
    gw.build_search_index()
    assert same_answer(after, gw.search(keys, k=TOPK)) and gw.search_index is not None


def test_an_index_over_the_budget_is_refused(emulated):
    gw = _rewriter()
    need = NSEEDS * 4
    for d in gw.k_shape[1:]:
        need *= d
    with pytest.raises(ValueError) as e:
        gw.build_search_index(max_bytes=need - 1)
    assert str(need) in str(e.value) and str(need - 1) in str(e.value)
    assert gw.search_index is None
    assert gw.build_search_index(max_bytes=need).nbytes() == need


def test_device_search_routes_ranking_for_key_through_search(emulated):
    gw = _rewriter(device_search=True)
    assert gw.device_search
    gw.build_search_index()
    key = pixel_keys(gw.search_index.maps, 1)[0]
    numbers, peaks, rq = gw.search(key, k=TOPK)
    del emulated[:]
    got_numbers, got_rq = gw.ranking_for_key(key, k=TOPK)
    assert emulated == [10, 10]
    assert torch.equal(got_numbers, numbers) and torch.equal(got_rq.quantiles([0.5, 0.99]), rq.quantiles([0.5, 0.99]))
    # the shapes and types of the default path
    gw.device_search = False
    del emulated[:]
    ref_numbers, ref_rq = gw.ranking_for_key(key, k=TOPK)
    assert not emulated
    assert got_numbers.shape == ref_numbers.shape and got_numbers.dtype == ref_numbers.dtype
    assert got_numbers.device == ref_numbers.device
    q = got_rq.quantiles([0.5, 0.99])
    assert type(got_rq) is type(ref_rq) and got_rq.size() == ref_rq.size() and got_rq.depth == ref_rq.depth
    assert q.shape == ref_rq.quantiles([0.5, 0.99]).shape and (q - ref_rq.quantiles([0.5, 0.99])).abs().max() < 1e-4
    assert numbers[0].item() == ref_numbers[0].item() == 1


def test_on_the_cpu_search_is_ranking_for_key():
    """No kernel layer at all (a ProgGAN, plain torch modules): search() computes the torch expression of
    ranking_for_key and feeds the same statistics, so the two agree exactly -- with an index (a CPU tensor here) as
    without."""
    from rewriting_amd import synthetic
    from rewriting_amd.rewrite import ganrewrite
    from rewriting_amd.utils import proggan, zdataset
    model = proggan.ProgressiveGenerator(resolution=32)
    synthetic.randomize_(model, seed=0, kind='proggan')
    model.eval()
    gw = ganrewrite.ProgressiveGanRewriter(model, zdataset.z_dataset_for_model(model, size=NSEEDS), 4)
    assert not gw._kernels()
    key = torch.randn(gw.k_shape[1])
    ref_numbers, ref_rq = gw.ranking_for_key(key, k=TOPK)
    q = [0.01, 0.5, 0.99, 0.999]
    for indexed in (False, True):
        if indexed:
            gw.build_search_index()
        numbers, peaks, rq = gw.search(key, k=TOPK)
        assert torch.equal(numbers, ref_numbers)
        assert rq.size() == ref_rq.size() and torch.equal(rq.quantiles(q), ref_rq.quantiles(q))
        assert peaks[0].item() == rq.minmax()[0, 1].item()
