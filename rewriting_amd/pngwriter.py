"""PNG files from images that are on the device: data URLs for the UI and the sample-set writer.

What the reference does on the host, one PIL ``img.save`` per picture -- ``renormalize.as_url``
(utils/renormalize.py:22-32) for the twelve tiles of a repaint, ``SaveImagePool`` / ``SaveImageWorker``
(utils/imgsave.py:58-66) for the 1 000 - 50 000 files of metrics/sample.py, metrics/sample_edited.py and
metrics/make_watermark_images.py:99-131 -- goes through ``hip.render_bytes`` and ``hip.png_encode`` here: the bytes,
the filters and the Huffman coding run in kernels, the host frames the chunks and writes the files.  The files are
lossless and decode to exactly ``renormalize.as_image``'s pixels; they are coded with literals only (no LZ77 matches),
so photographic pictures come out about the size of PIL's default and flat pictures larger.
``as_url(size=...)``'s PIL resize has no counterpart here: resize first.
"""
import base64
import collections
import os
from concurrent.futures import ThreadPoolExecutor

from . import hip, samples

MAX_WRITERS = 16          # file-writing threads; never sized from os.cpu_count() (a shared machine shows all its CPUs)


def encode(images, **overlay_kwargs):
    """One PNG file (bytes) per image of images (B, 3, H, W) float32 on the device, in the generator's range; the
    overlay_kwargs are hip.render_bytes's (activations / mask, level, thickness, colours)."""
    return hip.png_encode(hip.render_bytes(images, **overlay_kwargs))


def as_url(png):
    return 'data:image/png;base64,%s' % base64.b64encode(png).decode('utf-8')


def as_urls(images, **overlay_kwargs):
    """``[renormalize.as_url(img) for img in images]`` for a batch on the device (no ``size``: resize first)"""
    return [as_url(png) for png in encode(images, **overlay_kwargs)]


def _write(path, make):
    with open(path, 'wb') as f:
        f.write(make())              # the framing (CRC-32 over the coded bytes) runs in the writer's thread


def save_image_set(model_fn, model, seeds, dirname, name_template='image_{}.png', batch=32, offset=0, device=None,
                   shard=None, writers=8):
    """Writes the image of every seed (of this rank's shard of them: samples.generate) to
    dirname/name_template.format(seed), as metrics/sample.py:32-37 does through SaveImagePool.  The PNGs of a batch are
    coded on the device while a small thread pool (writers <= MAX_WRITERS threads) writes the files of the batches
    before it.  Returns the paths in the order written."""
    writers = max(1, min(int(writers), MAX_WRITERS))
    os.makedirs(dirname, exist_ok=True)
    paths, pending = [], collections.deque()
    with ThreadPoolExecutor(max_workers=writers) as pool:
        for chunk, images in samples.generate(model_fn, model, seeds, batch=batch, offset=offset, device=device,
                                              shard=shard):
            files = hip.png_encode(hip.render_bytes(images.contiguous()), deferred=True)
            for seed, make in zip(chunk, files):
                path = os.path.join(dirname, name_template.format(seed))
                paths.append(path)
                pending.append(pool.submit(_write, path, make))
            while len(pending) > 4 * batch:          # at most four batches of coded bytes wait for their writers
                pending.popleft().result()
        for job in pending:
            job.result()             # an error of a writer surfaces here
    return paths
