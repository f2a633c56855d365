"""Sample-set generation and Frechet statistics -- the "next" rows SURVEY.md section 8f.3 marks
after the hot path: sharded per-seed generator passes (metrics/sample.py:32-37,
metrics/sample_edited.py:55-59) and the reduction + distance of metrics/fid.py:40-62,137-187.
The feature extractor stays pluggable: any callable images -> (B, F) features.  The one that ships
is ``inception.FIDInception`` (the pool3 features of the reference's Inception graph, on the HIP
kernels; its weights are the caller's file); ``activation_statistics`` runs an extractor over image
batches and ``fid`` takes two sets of statistics to their distance without leaving the device.
"""
import warnings

import numpy
import torch

from . import hip, parallel
from .utils import zdataset
from .utils.stylegan2.models import noise_batch_period


def seed_latents(model, seeds, offset=0):
    """The reference draws image n from ``z_sample_for_model(model, size=1, seed=n + offset)``
    (metrics/sample.py:33): one independent stream per image."""
    return torch.cat([zdataset.z_sample_for_model(model, size=1, seed=int(s) + offset) for s in seeds])


def generate(model_fn, model, seeds, batch=32, offset=0, device=None, shard=None):
    """Yields (seed list, images) with seed i handled by rank i mod world (no collective).  The
    reference generates these sets at batch 1, where every image takes noise row 0 (quirk Q1);
    ``noise_batch_period(1)`` keeps that row for every image of a larger launch."""
    shard = parallel.shard() if shard is None else shard
    seeds = list(seeds)
    if shard is not None:
        seeds = seeds[shard[0]::shard[1]]
    device = device or next(model.parameters()).device
    with torch.no_grad(), noise_batch_period(1):
        for i in range(0, len(seeds), batch):
            chunk = seeds[i:i + batch]
            z = seed_latents(model, chunk, offset).to(device)
            yield chunk, model_fn(z)


class FeatureStatistics:
    """Running sum f and sum f f^T of feature rows, kept in float64; ``allreduce_`` pools the raw sums
    of all ranks with one RCCL all-reduce (F=2048: 33.5 MB).

    ``exact=True`` (opt-in; ``activation_statistics`` takes it): device features are widened to float64 before their
    products, and a batch's f^T f is ``hip.gemm_f64`` (the f64 MFMA) instead of the fp32 MFMA block.  The fp32 block
    rounds every entry to 2^-24 of |f|^2, which is noise of that size in every eigenvalue of the covariance -- harmless
    for a full-rank set, but a set with fewer samples than features has a thousand eigenvalues that should be zero, and
    the matrix square root of the Frechet distance sees them: six 75 x 75 images against themselves gave d^2 = -3.6e-4
    on Tr S = 1.76 through the fp32 block."""

    def __init__(self, dim=None, exact=False):
        self.count = 0
        self.sum = None
        self.outer = None
        self._dim = dim
        self.exact = bool(exact)

    def add(self, feats):
        feats = feats.detach()
        if feats.dim() != 2:
            feats = feats.reshape(feats.shape[0], -1)
        f = feats.shape[1]
        if self.sum is None:
            self.sum = torch.zeros(f, dtype=torch.float64, device=feats.device)
            self.outer = torch.zeros(f, f, dtype=torch.float64, device=feats.device)
        if hip.on_device(feats) and self.exact:
            d = feats.double().contiguous()
            self.outer += hip.gemm_f64(d, d, trans_a=True)                          # f64 MFMA, a fixed order
        elif hip.on_device(feats) and feats.dtype == torch.float32 and f % 4 == 0:
            block = torch.zeros(f, f, dtype=torch.float32, device=feats.device)
            hip.second_moment_accumulate(block, feats.contiguous(), nchw=False)    # fp32 MFMA per batch
            self.outer += block.double()                                            # fp64 across batches
        else:
            d = feats.double()
            self.outer += d.t() @ d
        self.sum += feats.double().sum(0)
        self.count += feats.shape[0]

    def allreduce_(self):
        import torch.distributed as dist
        if parallel.shard() is None:
            return self
        dev = self.sum.device
        if dist.get_backend() == 'gloo':
            dev = torch.device('cpu')
        packed = torch.cat([self.sum.to(dev), self.outer.reshape(-1).to(dev),
                            torch.tensor([float(self.count)], dtype=torch.float64, device=dev)])
        dist.all_reduce(packed, op=dist.ReduceOp.SUM)
        f = self.sum.numel()
        self.sum = packed[:f].to(self.sum.device)
        self.outer = packed[f:f + f * f].reshape(f, f).to(self.outer.device)
        self.count = int(round(packed[-1].item()))
        return self

    def mean_cov(self, device=False):
        """(mu, sigma) as numpy float64, sigma unbiased like numpy.cov(act, rowvar=False)
        (metrics/fid.py:60-61).  ``device=True``: the same two as float64 tensors where the sums live -- what
        ``frechet_distance`` takes without a round trip through the host."""
        n = self.count
        mu = self.sum / n
        sigma = (self.outer - n * torch.outer(mu, mu)) / (n - 1)
        if device:
            return mu, sigma
        return mu.cpu().numpy(), sigma.cpu().numpy()


def activation_statistics(batches, net):
    """``fid.calculate_activation_statistics`` (metrics/fid.py:40-62) as running sums: every batch of ``batches`` -- an
    iterable of image tensors, or of the (seeds, images) pairs ``generate`` yields -- goes through ``net`` (any callable
    images -> (B, F) features, e.g. ``inception.FIDInception``) and its features into a ``FeatureStatistics(exact=True)``
    -- float64 products, as numpy.cov of the reference's float64 activations has them -- which is returned.  Images,
    features and sums stay where ``net`` leaves them."""
    stats = FeatureStatistics(exact=True)
    with torch.no_grad():
        for batch in batches:
            images = batch[1] if isinstance(batch, (tuple, list)) else batch
            stats.add(net(images))
    if stats.count == 0:
        raise ValueError('activation_statistics: no batch of images')
    return stats


def fid(stats_a, stats_b):
    """The Frechet distance of two ``FeatureStatistics`` on the device their sums live on: ``mean_cov(device=True)`` of
    both, then ``frechet_distance`` there (metrics/fid.py:196-210 behind the activations)."""
    mu_a, sigma_a = stats_a.mean_cov(device=True)
    mu_b, sigma_b = stats_b.mean_cov(device=True)
    return frechet_distance(mu_a, sigma_a, mu_b, sigma_b, device=mu_a.device)


def _frechet_distance_device(mu1, sigma1, mu2, sigma2, device):
    """The inputs as contiguous float64 tensors on ``device`` (or on the device the tensors among them share), then
    hip.frechet_distance_f64."""
    tensors = [t for t in (mu1, sigma1, mu2, sigma2) if isinstance(t, torch.Tensor)]
    if device is None:
        devices = {t.device for t in tensors}
        if len(devices) != 1:
            raise ValueError('the inputs are on %s: pass device=' % sorted(str(d) for d in devices))
        device = devices.pop()
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('rewriting_amd: frechet_distance(device=%s): the HIP kernels need a GPU (there is no CPU '
                           'fallback); leave device=None for the host route' % device)

    def put(x, dims):
        x = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(numpy.asarray(x, dtype=numpy.float64))
        x = x.to(device=device, dtype=torch.float64)
        x = x.reshape((1,) * (dims - x.dim()) + tuple(x.shape)) if x.dim() < dims else x     # atleast_1d / atleast_2d
        return x.contiguous()
    mu1, mu2, sigma1, sigma2 = put(mu1, 1), put(mu2, 1), put(sigma1, 2), put(sigma2, 2)
    assert mu1.shape == mu2.shape and sigma1.shape == sigma2.shape
    return hip.frechet_distance_f64(mu1, sigma1, mu2, sigma2)


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6, device=None):
    """d^2 = |mu1-mu2|^2 + Tr(S1 + S2 - 2 sqrt(S1 S2)) with the reference's singular-product retry and
    imaginary-part check (metrics/fid.py:137-187).

    With ``device=None`` and host inputs this is the scipy route, unchanged.  With device tensors, or with ``device=``
    given, the distance is computed on the device (hip.frechet_distance_f64: Tr sqrt(S1 S2) as the sum of the square
    roots of the eigenvalues of F^T S2 F, S1 = F F^T, by two block Jacobi solves) and returned as a Python float with
    one copy to the host.  ``eps`` and the imaginary-part check have no counterpart there: the eigenvalues are column
    norms, so the value is real and finite by construction for finite input, singular products included."""
    if device is not None or any(isinstance(t, torch.Tensor) and t.is_cuda for t in (mu1, sigma1, mu2, sigma2)):
        return _frechet_distance_device(mu1, sigma1, mu2, sigma2, device)
    from scipy import linalg
    mu1, mu2 = numpy.atleast_1d(mu1), numpy.atleast_1d(mu2)
    sigma1, sigma2 = numpy.atleast_2d(sigma1), numpy.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape and sigma1.shape == sigma2.shape
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not numpy.isfinite(covmean).all():
        warnings.warn('fid calculation produces singular product; adding %s to diagonal of cov estimates' % eps)
        offset = numpy.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if numpy.iscomplexobj(covmean):
        if not numpy.allclose(numpy.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError('Imaginary component {}'.format(numpy.max(numpy.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff) + numpy.trace(sigma1) + numpy.trace(sigma2) - 2 * numpy.trace(covmean)
