"""PNG files to images that are on the device: the mirror of pngwriter.py.

What the reference does on the host, one PIL ``Image.open`` per picture on one thread -- the loader of the edit tables
(metrics/distances.py:67-70), ``renormalize.from_url`` (utils/renormalize.py) for a data URL, the image folders that a
sample-set statistic walks -- goes through ``hip.png_decode`` here: the host reads the chunks and checks what is
O(file) in C (``zlib.crc32``), the inflate and the filters run in kernels, and the pixels never
visit the host.  The kernels take 8-bit grey, truecolour and truecolour-with-alpha files that are not interlaced --
what PIL and ``pngwriter`` write for RGB, L and RGBA pictures.  Every other valid form (palette, 16 bits, fewer than 8
bits, grey with alpha, Adam7) is recognised and refused by name, or decoded by PIL on the host with ``fallback=True``.
"""
import base64
import collections
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import torch

from . import hip, pngcode

MAX_READERS = 16          # file-reading threads; never sized from os.cpu_count() (a shared machine shows all its CPUs)

Parsed = collections.namedtuple('Parsed', 'w h channels span adler')
Parsed.__doc__ = """A file the kernels take: width, height, channels (1, 3, 4), the raw deflate stream (a memoryview: the
IDAT payload between the zlib header and the Adler-32 trailer) and the value of that trailer"""
Unsupported = collections.namedtuple('Unsupported', 'w h form')
Unsupported.__doc__ = """The marker for a valid file of a form the kernels do not take; form names it"""

_CHANNELS = {0: 1, 2: 3, 6: 4}             # colour type -> bytes per pixel at 8 bits
_KNOWN_CRITICAL = (b'IHDR', b'PLTE', b'IDAT', b'IEND')


def parse(file_bytes):
    """Parsed(w, h, channels, deflate span, adler) of a PNG file (bytes), or Unsupported(w, h, form) for a valid file of
    a form the kernels do not take.  ValueError for a file that is not a valid PNG: a wrong signature, IHDR not first or
    not 13 bytes, a chunk that is cut short or whose CRC-32 is wrong, IDATs that are not consecutive, none at all, no
    IEND, an unknown critical chunk, a zlib header that is not deflate with a window of at most 32 KiB and no preset
    dictionary.  The Adler-32 trailer is returned, not checked: the kernels report the sums of what they produced."""
    data = memoryview(file_bytes).cast('B')
    if bytes(data[:8]) != pngcode.SIGNATURE:
        raise ValueError('not a PNG file: wrong signature')
    at, idats, header, ended, idat_done = 8, [], None, False, False
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError('PNG: a chunk is cut short at byte %d' % at)
        size, kind = struct.unpack('>I', data[at:at + 4])[0], bytes(data[at + 4:at + 8])
        if at + 12 + size > len(data):
            raise ValueError('PNG: chunk %r is cut short' % kind)
        body = data[at + 8:at + 8 + size]
        if struct.unpack('>I', data[at + 8 + size:at + 12 + size])[0] != zlib.crc32(body, zlib.crc32(kind)) & 0xffffffff:
            raise ValueError('PNG: wrong CRC-32 of chunk %r' % kind)
        if header is None:
            if kind != b'IHDR' or size != 13:
                raise ValueError('PNG: the first chunk is not an IHDR of 13 bytes')
            header = struct.unpack('>IIBBBBB', body)
        elif kind == b'IHDR':
            raise ValueError('PNG: a second IHDR')
        elif kind == b'IDAT':
            if idat_done:
                raise ValueError('PNG: the IDAT chunks are not consecutive')
            idats.append(body)
        elif kind == b'IEND':
            ended = True
            break
        elif not (kind[0] & 0x20) and kind not in _KNOWN_CRITICAL:
            raise ValueError('PNG: unknown critical chunk %r' % kind)
        if idats and kind != b'IDAT':
            idat_done = True
        at += 12 + size
    if header is None or not ended:
        raise ValueError('PNG: no IEND chunk')
    if not idats:
        raise ValueError('PNG: no IDAT chunk')
    w, h, depth, colour, compression, filtering, interlace = header
    if w < 1 or h < 1 or compression != 0 or filtering != 0 or interlace > 1 \
            or (colour, depth) not in [(c, d) for c, ds in ((0, (1, 2, 4, 8, 16)), (2, (8, 16)), (3, (1, 2, 4, 8)),
                                                             (4, (8, 16)), (6, (8, 16))) for d in ds]:
        raise ValueError('PNG: an IHDR that the specification does not allow: %r' % (header,))
    payload = idats[0] if len(idats) == 1 else memoryview(b''.join(idats))
    if len(payload) < 6:
        raise ValueError('PNG: the IDAT payload is shorter than a zlib header and trailer')
    cmf, flg = payload[0], payload[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31 or flg & 0x20:
        raise ValueError('PNG: the zlib header %02x %02x is not deflate, window <= 32 KiB, no dictionary' % (cmf, flg))
    if interlace:
        return Unsupported(w, h, 'interlaced')
    if colour == 3:
        return Unsupported(w, h, 'palette')
    if depth == 16:
        return Unsupported(w, h, '16-bit')
    if depth < 8:
        return Unsupported(w, h, 'depth below 8')
    if colour == 4:
        return Unsupported(w, h, 'grey with alpha')
    return Parsed(w, h, _CHANNELS[colour], payload[2:len(payload) - 4], struct.unpack('>I', payload[len(payload) - 4:])[0])


def _pil(file_bytes, device):
    import io
    import numpy
    import PIL.Image
    with PIL.Image.open(io.BytesIO(file_bytes)) as im:
        return torch.from_numpy(numpy.asarray(im.convert('RGB'), dtype=numpy.uint8).copy()).to(device)


def _decode_parsed(parsed, device, fallback, files=None):
    """decode() behind the parsing: parsed[i] a Parsed, an Unsupported or the ValueError of file i"""
    out = [None] * len(parsed)
    groups = collections.OrderedDict()
    for i, item in enumerate(parsed):
        if isinstance(item, Exception):
            raise ValueError('file %d: %s' % (i, item))
        if isinstance(item, Unsupported):
            if not fallback:
                raise ValueError('file %d: a valid PNG of a form the device decoder does not take (%s, %d x %d); '
                                 'fallback=True decodes it with PIL on the host' % (i, item.form, item.w, item.h))
            out[i] = _pil(files[i], device)
        else:
            groups.setdefault((item.h, item.w, item.channels), []).append(i)
    for (h, w, channels), members in groups.items():
        pixels, status = hip.png_decode([parsed[i].span for i in members], h, w, channels, device=device)
        for k, i in enumerate(members):
            code, produced, s1, s2 = (int(v) for v in status[k])
            if code != 0:
                raise ValueError('file %d: status %d (%s) after %d bytes of its stream'
                                 % (i, code, hip.PNG_STATUS[code] if code < len(hip.PNG_STATUS) else '?', produced))
            if pngcode.adler_fold([(produced, s1, s2)]) != parsed[i].adler:
                raise ValueError('file %d: the Adler-32 trailer %08x is not that of the stream (%08x)'
                                 % (i, parsed[i].adler, pngcode.adler_fold([(produced, s1, s2)])))
            out[i] = pixels[k]
    return out


def _try_parse(file_bytes):
    try:
        return parse(file_bytes)
    except ValueError as e:
        return e


def decode(files, device='cuda', fallback=False):
    """One (H, W, 3) uint8 tensor on `device` per PNG file (bytes) of `files`, in their order: the pixels of
    ``PIL.Image.open(...).convert('RGB')``.  The files are grouped by (height, width, channels): one hip.png_decode per
    group.  ValueError, naming the file's index and the status, for a file that is not a valid PNG or whose stream is
    defective; also for a valid file of a form the kernels do not take (parse), unless fallback=True: PIL decodes that one
    file on the host and it is uploaded."""
    files = list(files)
    return _decode_parsed([_try_parse(f) for f in files], device, fallback, files)


def _read(path):
    with open(path, 'rb') as f:
        data = f.read()
    return data, _try_parse(data)        # the chunk walk and the CRC-32 run in the reader's thread


def read_files(paths, device='cuda', fallback=False, readers=8):
    """decode() of the files at `paths`, read and parsed by a pool of readers <= MAX_READERS threads"""
    paths = list(paths)
    if not paths:
        return []
    readers = max(1, min(int(readers), MAX_READERS, len(paths)))
    with ThreadPoolExecutor(max_workers=readers) as pool:
        loaded = list(pool.map(_read, paths))
    try:
        return _decode_parsed([p for _, p in loaded], device, fallback, [d for d, _ in loaded])
    except ValueError as e:
        index = int(str(e).split(':', 1)[0].split()[1])
        raise ValueError('%s (%s)' % (e, paths[index])) from None


def read_batch(paths, device='cuda', fallback=False, readers=8):
    """(B, H, W, 3) uint8 on the device: the pictures at `paths`, which must have one shape (ValueError otherwise)"""
    images = read_files(paths, device=device, fallback=fallback, readers=readers)
    if not images:
        raise ValueError('read_batch: no paths')
    shapes = sorted(set(tuple(im.shape) for im in images))
    if len(shapes) != 1:
        raise ValueError('read_batch takes pictures of one shape, not %s' % (shapes,))
    return torch.stack(images)


_AS_FLOAT = {}


def as_float(bytes_bhwc):
    """(B, 3, H, W) float32 in [-1, 1] from bytes (B, H, W, 3) on the device: bit for bit what distances._load_image
    makes of the same pixels on the host.  The 256 values are computed once, on the host, by that very expression, and
    looked up on the device."""
    dev = bytes_bhwc.device
    if dev not in _AS_FLOAT:
        _AS_FLOAT[dev] = ((torch.arange(256, dtype=torch.uint8).to(torch.float32) / 255 - 0.5) / 0.5).to(dev)
    return _AS_FLOAT[dev][bytes_bhwc.permute(0, 3, 1, 2).long()].contiguous()


def from_urls(urls, device='cuda', fallback=False):
    """The pictures of data URLs (pngwriter.as_urls, renormalize.as_url): a list of (H, W, 3) uint8 device tensors"""
    files = []
    for i, url in enumerate(urls):
        head, _, body = url.partition(',')
        if not head.startswith('data:image/png') or not head.endswith(';base64'):
            raise ValueError('url %d is not a base64 data URL of a PNG' % i)
        files.append(base64.b64decode(body))
    return decode(files, device=device, fallback=fallback)


def load_image_set(dirname, seeds, name_template='image_{}.png', batch=32, device='cuda', fallback=False, readers=8):
    """Yields (chunk of seeds, bytes (len(chunk), H, W, 3) uint8 on the device) for the files
    dirname/name_template.format(seed), `batch` at a time: the way back from pngwriter.save_image_set, for statistics
    over a sample set."""
    seeds = list(seeds)
    for start in range(0, len(seeds), batch):
        chunk = seeds[start:start + batch]
        yield chunk, read_batch([os.path.join(dirname, name_template.format(s)) for s in chunk], device=device,
                                fallback=fallback, readers=readers)
