"""How much an edit disturbs the rest of the picture: the distances of the reference's edit tables (metrics/distances.py:96-136,
``compute_dl``) on the device.

Three modes, named as the reference's command line names them:

* ``'lpips'``       per image ``sum(LPIPS * mask) / sum(mask)`` with the spatial LPIPS map (lpips.LPIPS) and the mask of the
                    pixels whose segmentation is none of ``src`` (:110-121);
* ``'mask_lpips'``  the same with a weight of ones, i.e. the mean of the map (:123-129);
* ``'pixel'``       ``sum(mask * sum_c |after - before|)`` and ``sum(mask)`` (:131-133).

``edit_distance`` takes device tensors and a whole batch at once, where the reference loops image by image (the images of a
batch do not interact); ``compute_dl`` walks two directories of PNG files and one of segmentations, as the reference does,
and returns its ``(total, count)`` -- or, given a ``segmenter`` (faceparse.FaceSegmenter), segments the `before` images on
the device instead of reading a directory.  ``correct_modification`` is the "pixels correctly modified" count of
metrics/seg_correct_mod.py:40-65 over two batches of label maps.
"""
import os

import torch

from . import hip

MODES = ('lpips', 'mask_lpips', 'pixel')


def mask_of(seg, src):
    """(B, H, W) float32: the product over ``src`` of ``seg != index`` (metrics/distances.py:110-114)"""
    mask = torch.ones_like(seg, dtype=torch.float32)
    for index in src:
        mask = mask * (seg != index).to(torch.float32)
    return mask


def edit_distance(before, after, seg=None, src=(), mode='lpips', net=None):
    """(values, counts), two (B,) float32 tensors on the images' device, for images (B, 3, H, W) in [-1, 1] and the
    segmentation seg (B, H, W) of `before` (None: nothing is masked).  'lpips' / 'mask_lpips': values = the (masked) LPIPS of
    every pair, counts = ones -- net is a lpips.LPIPS on that device; 'pixel': values = the masked L1 sums, counts = the masks'
    sums.  compute_dl's total and count are their sums."""
    if mode not in MODES:
        raise ValueError('rewriting_amd: edit_distance: mode is one of %s, not %r' % (', '.join(MODES), mode))
    if not isinstance(before, torch.Tensor) or before.dim() != 4 or not isinstance(after, torch.Tensor) or after.shape != before.shape:
        raise ValueError('rewriting_amd: edit_distance takes two image batches (B, 3, H, W) of one shape')
    b, _, h, w = before.shape
    if seg is None:
        mask = torch.ones(1, h, w, device=before.device, dtype=torch.float32)
    else:
        if tuple(seg.shape) != (b, h, w) or seg.device != before.device:
            raise ValueError('rewriting_amd: edit_distance: the segmentation is %s on %s, the images %s on %s -- it must be (B, H, W)'
                             % (tuple(seg.shape), seg.device, tuple(before.shape), before.device))
        mask = mask_of(seg, src)
    if mode == 'pixel':
        sums = hip.masked_l1(after, before, mask)
        return sums[:, 0], sums[:, 1]
    if net is None:
        raise ValueError('rewriting_amd: edit_distance: mode %r needs net, a lpips.LPIPS (lpips.lpips_vgg()) on the images\' device'
                         % mode)
    weight = mask[:, None] if mode == 'lpips' else torch.ones(1, 1, h, w, device=before.device, dtype=torch.float32)
    return net(before, after, w=weight.contiguous()), torch.ones(b, device=before.device, dtype=torch.float32)


def _load_image(path):
    """a PNG as transforms.ToTensor + Normalize(0.5, 0.5) leave it (metrics/distances.py:67-70): (3, H, W) float32 in [-1, 1]"""
    import numpy
    import PIL.Image
    with PIL.Image.open(path) as im:
        data = numpy.asarray(im.convert('RGB'), dtype=numpy.uint8)
    return (torch.from_numpy(data.copy()).permute(2, 0, 1).to(torch.float32) / 255 - 0.5) / 0.5


def compute_dl(before_dir, after_dir, seg_dir, indices, src=(1708,), srcc=2, mode='lpips', batch_size=100, net=None,
               device='cuda', name_template='{}.png', device_decode=False, segmenter=None):
    """(total, count) of metrics/distances.py:96-136 over the pairs ``before_dir/<key>.png``, ``after_dir/<key>.png`` with the
    segmentations ``seg_dir/<key>.pth`` (a tensor whose row `srcc` is the (H, W) map) for key in indices -- `batch_size` pairs
    per device call.  total: the sum of the per-image distances (count: their number), or in 'pixel' mode the masked L1 sum
    (count: the masks' sum).  device_decode: the `before` and `after` files are decoded on the device (pngreader.read_batch,
    as_float) instead of by PIL, one file at a time, on the host; the images, and so (total, count), are the same bit for
    bit.  The segmentations are torch.load'ed either way -- unless seg_dir is None and `segmenter` is given: then the
    segmentation of a batch is ``segmenter.segment_batch(before)[:, srcc]`` on the device (faceparse.FaceSegmenter, the
    reference's metrics/seg_stats.py run ahead of time; srcc=0 for faces).  Exactly one of seg_dir and segmenter is given."""
    if (seg_dir is None) == (segmenter is None):
        raise ValueError('rewriting_amd: compute_dl takes the segmentations from seg_dir (.pth files) or from segmenter '
                         '(segment_batch on the device): pass exactly one of them, not %s' % ('both' if segmenter else 'neither'))
    if device_decode:
        from . import pngreader

        def load(dirname, chunk):
            return pngreader.as_float(pngreader.read_batch([os.path.join(dirname, name_template.format(k)) for k in chunk],
                                                           device=device))
    else:
        def load(dirname, chunk):
            return torch.stack([_load_image(os.path.join(dirname, name_template.format(k))) for k in chunk]).to(device)
    total, count = 0.0, 0
    keys = [int(k) for k in indices]
    for start in range(0, len(keys), batch_size):
        chunk = keys[start:start + batch_size]
        before, after = load(before_dir, chunk), load(after_dir, chunk)
        if segmenter is not None:
            seg = segmenter.segment_batch(before)[:, srcc]
        else:
            seg = torch.stack([torch.load(os.path.join(seg_dir, '%d.pth' % k), map_location='cpu')[srcc] for k in chunk]).to(device)
        values, counts = edit_distance(before, after, seg, src, mode, net)
        total += values.double().sum().item()
        count += int(round(counts.double().sum().item()))
    return total, count


def correct_modification(before_seg, after_seg, src, tgt, srcc=0, tgtc=0):
    """(total, count), two Python ints, of metrics/seg_correct_mod.py:51-62 for one batch: count = the pixels whose label in
    before_seg is one of ``src``, total = those of them whose label in after_seg is one of ``tgt``.  The maps are int64
    (B, H, W) or (B, C, H, W) on the device, of which the channels srcc / tgtc are read; src and tgt name 1 .. 16 labels
    each."""
    for name, labels in (('src', src), ('tgt', tgt)):
        if not 1 <= len(labels) <= hip.SEG_MAX_SET:
            raise ValueError('rewriting_amd: correct_modification: %s must name 1 .. %d labels, not %d'
                             % (name, hip.SEG_MAX_SET, len(labels)))
    sums = hip.seg_correct_counts(before_seg, after_seg, src, tgt, srcc, tgtc).sum(0).tolist()
    return int(sums[0]), int(sums[1])
