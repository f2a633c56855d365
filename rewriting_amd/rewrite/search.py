"""The UI's Search on the device: the response of every seed's key map to a few query keys
(``ProgressiveGanRewriter.ranking_for_key``, rewrite/ganrewrite.py:582-594), and a resident index of the key maps.

The key maps of a rewriter depend neither on the query nor on the weights of the edited layer (the context model
ends in front of the target convolution), so ``KeyMapIndex`` computes them once and keeps them on the device; a query
is then one streaming pass of ``hip.key_response`` over them instead of a forward sweep over the dataset.

Indexed and un-indexed queries are the same numbers bit for bit:

* the index is filled in exactly the launches the sweeps use (``_sweep``: ``_sweep_batch()`` seeds under
  ``noise_batch_period(10)``) -- a seed's key map depends on its noise row and, through the f16-pair split scales that
  follow a launch's bounds, on the launch it was computed in;
* the kernel's sum of a pixel depends on (C, hw) only, not on the launch around it (include/rewriting_hip.h);
* both feed the same ``RunningTopK`` / ``RunningQuantile`` in the same pieces, launch by launch, in seed order.

Under ``torch.distributed`` every rank answers the whole query for itself, like ``tally.tally_topk_and_quantile``.
"""
import torch

from .. import hip
from ..utils import runningstats, tally


def _each_launch(visit, dataset, batch_size=10):
    """visit(z) for every launch of a sweep over ``dataset``, in seed order (the loader of utils/tally.py)."""
    for batch in tally.make_loader(dataset, None, batch_size):
        tally.call_compute(visit, batch)


def _stamp(model):
    """What a change of the context model cannot leave alone: where each parameter and buffer lives and how often it
    was written in place."""
    return tuple((name, t.data_ptr(), t._version)
                 for name, t in list(model.named_parameters()) + list(model.named_buffers()))


def index_bytes(gw):
    n = 4 * len(gw.zds)
    for d in tuple(gw.k_shape)[1:]:
        n *= int(d)
    return n


class KeyMapIndex:
    """The key maps of every seed of ``gw.zds``: ``maps`` (N, C, H, W) float32 on the rewriter's device, and the
    launches they were computed in (``launches``: (first seed, seeds) each)."""

    def __init__(self, gw):
        self.maps = torch.empty((len(gw.zds),) + tuple(gw.k_shape)[1:], dtype=torch.float32, device=gw.device)
        self.launches = []

        def keep(zbatch):
            acts = gw._key_map(zbatch)
            first = self.launches[-1][0] + self.launches[-1][1] if self.launches else 0
            self.maps[first:first + acts.shape[0]].copy_(acts)
            self.launches.append((first, acts.shape[0]))
        gw._sweep(_each_launch, keep, gw.zds)
        assert sum(n for _, n in self.launches) == len(gw.zds)
        self.stamp = _stamp(gw.context_model)

    def nbytes(self):
        return self.maps.numel() * self.maps.element_size()

    def fresh(self, gw):
        return self.stamp == _stamp(gw.context_model)

    def pieces(self):
        for first, n in self.launches:
            yield self.maps[first:first + n]


def build_index(gw, max_bytes=None):
    """All or nothing: the index of every seed, or ValueError (and no allocation) when it needs more than max_bytes."""
    need = index_bytes(gw)
    if max_bytes is not None and need > max_bytes:
        raise ValueError('the search index of %d seeds needs %d bytes, more than max_bytes = %d'
                         % (len(gw.zds), need, max_bytes))
    gw.search_index = None
    gw.search_index = KeyMapIndex(gw)
    return gw.search_index


def current_index(gw):
    """The rewriter's index if it still describes the context model, else None (a stale index is dropped)."""
    if gw.search_index is not None and not gw.search_index.fresh(gw):
        gw.search_index = None
    return gw.search_index


def _respond(gw, acts, keys):
    """heat (B, K, H, W), peak (B, K)"""
    if gw._kernels():
        return hip.key_response(acts.contiguous(), keys)
    heat = torch.stack([gw._response(acts, key) for key in keys], dim=1)
    return heat, heat.reshape(heat.shape[0], heat.shape[1], -1).max(2)[0]


def search(gw, keys, k=12):
    """Per key: the k seeds whose key map responds most (by descending peak), their peaks, and the RunningQuantile of
    all N*H*W responses.  keys (K, C) -> (numbers (K, k), peaks (K, k), quantiles of K units); a single key (C,) ->
    (numbers (k,), peaks (k,), quantiles of one unit), the statistics of ranking_for_key."""
    keys = keys.to(gw.device)
    single = keys.dim() == 1
    if single:
        keys = keys[None]
    rtk, rq = runningstats.RunningTopK(k=k), runningstats.RunningQuantile()

    def tally_piece(acts):
        heat, peak = _respond(gw, acts, keys)
        rtk.add(peak)
        rq.add(heat.permute(1, 0, 2, 3).reshape(heat.shape[1], -1).t())      # (samples, keys), stored as it lies
    index = current_index(gw)
    with torch.no_grad():
        if index is not None:
            for acts in index.pieces():
                tally_piece(acts)
        else:
            gw._sweep(_each_launch, lambda zbatch: tally_piece(gw._key_map(zbatch)), gw.zds)
    rtk.to_('cpu')
    rq.compress_()
    rq.to_('cpu')
    peaks, numbers = rtk.result()
    if single:
        return numbers[0], peaks[0], rq
    return numbers, peaks, rq
