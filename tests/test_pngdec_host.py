"""PNG decoding, the host side (no GPU): the numpy / Python twin of the kernels (tests/pngdec_checks.py) equals zlib and PIL
on the whole corpus the device tests use, its builders make what they say, and pngreader's host logic -- the chunk walk
and its refusals, the grouping by shape, the fallback, the float conversion -- works with the twin in hip.png_decode's
place."""
import io
import zlib

import numpy as np
import PIL.Image
import pytest
import torch

from rewriting_amd import distances, pngcode, pngreader
from tests import pngdec_checks as D


@pytest.fixture(scope='module')
def corpus():
    return D.corpus()


@pytest.fixture
def twin(monkeypatch):
    calls = []

    def decode(spans, h, w, channels, device='cpu', timings=None):
        calls.append((len(spans), h, w, channels))
        return D.png_decode(spans, h, w, channels)
    monkeypatch.setattr(pngreader.hip, 'png_decode', decode)
    return calls


def test_twin_equals_zlib_and_pil_on_the_corpus(corpus):
    assert len(corpus) > 40
    kinds = set()
    for name, data in corpus:
        parsed = pngreader.parse(data)
        want = D.pil_pixels(data)
        assert (parsed.h, parsed.w) == want.shape[:2], name
        span = bytes(parsed.span)
        expect = parsed.h * (1 + parsed.channels * parsed.w)
        status, stream = D.inflate(span, expect)
        assert status == D.OK and stream == zlib.decompressobj(-15).decompress(span), name
        assert zlib.adler32(stream) & 0xffffffff == parsed.adler == pngcode.adler_fold([(len(stream),) + D.raw_sums(stream)]), name
        status, pixels = D.unfilter(stream, parsed.h, parsed.w, parsed.channels)
        assert status == D.OK and np.array_equal(pixels, want), name
        kinds.update((span[0] >> 1) & 3 for _ in [0])
        kinds.update('filter %d' % t for t in set(stream[::1 + parsed.channels * parsed.w]))
    assert {0, 1, 2} <= kinds and {'filter %d' % t for t in range(5)} <= kinds       # stored, fixed, dynamic; all filters


def test_corpus_has_the_streams_it_is_meant_to_have(corpus):
    files = dict(corpus)
    big = files['random 160x160']
    assert big.count(b'IDAT') >= 2 and len(pngreader.parse(big).span) > 65536                 # several IDATs and stored blocks
    assert len(zlib.decompressobj(-15).decompress(bytes(pngreader.parse(files['smooth 90x364']).span))) == 98370
    for h, w, length in D.EDGE_SHAPES:
        assert pngreader.parse(files['random %dx%d' % (h, w)])[:3] == (w, h, 3) and h * (1 + 3 * w) == length


def test_hand_made_streams_are_accepted_by_zlib_and_the_twin():
    streams = D.hand_streams()
    assert len(streams) == 12
    for name, stream, out in streams:
        assert zlib.decompressobj(-15).decompress(stream) == out, name
        assert D.inflate(stream, len(out)) == (D.OK, out), name
        assert D.inflate(stream, len(out) + 1)[0] == D.OUTPUT_UNDER and D.inflate(stream, len(out) - 1)[0] == D.OUTPUT_OVER, name


def test_defect_streams_have_one_defect_each():
    want = [D.BAD_BLOCK_TYPE, D.STORED_LENGTH, D.TRUNCATED, D.TRUNCATED, D.TRUNCATED, D.BAD_LITLEN_SET, D.BAD_LITLEN_SET,
            D.NO_END_OF_BLOCK, D.BAD_CODELEN_SET, D.BAD_CODELEN_SET, D.BAD_SYMBOL, D.BAD_SYMBOL, D.DISTANCE_TOO_FAR,
            D.OUTPUT_OVER, D.OUTPUT_UNDER]
    defects = D.defect_streams()
    assert [D.inflate(stream, 700)[0] for _, stream in defects] == want
    for name, stream in defects:
        unpacker = zlib.decompressobj(-15)
        try:
            accepted = len(unpacker.decompress(stream)) == 700 and unpacker.eof
        except zlib.error:
            accepted = False
        assert not accepted, name


def test_forced_filters_and_the_bad_filter_status():
    picture = D.smooth_image(7, 33, seed=4, period=16)
    for kind in range(5):
        stream = D.filter_stream(picture, [kind] * 7)
        assert set(stream[::100]) == {kind}
        assert D.unfilter(stream, 7, 33, 3)[0] == D.OK and np.array_equal(D.unfilter(stream, 7, 33, 3)[1], picture)
    status, _ = D.unfilter(D.filter_stream(picture, [0, 1, 5, 3, 4, 0, 1]), 7, 33, 3)
    assert status == D.BAD_FILTER


def test_decode_groups_by_shape_and_keeps_the_order(twin):
    pictures = [D.random_image(3, 5, seed=1), D.random_image(7, 33, seed=2), D.random_image(3, 5, seed=3),
                D.random_image(3, 5, 1, seed=4), D.random_image(7, 33, seed=5), D.random_image(3, 5, 4, seed=6)]
    files = [D.pil_file(p) for p in pictures]
    got = pngreader.decode(files, device='cpu')
    assert twin == [(2, 3, 5, 3), (2, 7, 33, 3), (1, 3, 5, 1), (1, 3, 5, 4)]                  # one call per shape class
    assert len(got) == 6 and all(g.dtype == torch.uint8 for g in got)
    for g, f in zip(got, files):
        assert np.array_equal(g.numpy(), D.pil_pixels(f))
    assert pngreader.decode([], device='cpu') == []


def _pil_mode_file(mode):
    buf = io.BytesIO()
    image = PIL.Image.fromarray(D.random_image(5, 6, seed=7)).convert(mode)
    image.save(buf, format='png')
    return buf.getvalue()


def test_fallback_on_and_off(twin):
    good = D.pil_file(D.random_image(5, 6, seed=8))
    for mode, form in (('P', 'palette'), ('LA', 'grey with alpha')):
        other = _pil_mode_file(mode)
        marker = pngreader.parse(other)
        assert isinstance(marker, pngreader.Unsupported) and marker.form == form and (marker.w, marker.h) == (6, 5)
        with pytest.raises(ValueError, match='file 1.*%s' % form):
            pngreader.decode([good, other], device='cpu')
        got = pngreader.decode([good, other, good], device='cpu', fallback=True)
        assert [np.array_equal(g.numpy(), D.pil_pixels(f)) for g, f in zip(got, [good, other, good])] == [True] * 3
    assert twin[-1] == (2, 5, 6, 3)                                                          # the fallback took one file only


def test_parse_refusals_and_markers():
    picture = D.random_image(4, 6, seed=9)
    good = D.png_file(picture)
    parsed = pngreader.parse(good)
    assert parsed[:3] == (6, 4, 3) and zlib.decompressobj(-15).decompress(bytes(parsed.span)) == D.filter_stream(
        picture, [0, 1, 2, 3])
    stream = D.filter_stream(picture, [0] * 4)
    idat = zlib.compress(stream)
    text = D.chunk(b'tEXt', b'key\0value')
    cases = {
        'signature': b'\x89PNX' + good[4:],
        'CRC': good[:40] + bytes([good[40] ^ 1]) + good[41:],
        'not consecutive': D.png_container(6, 4, idat, split=[10], between=text),
        'dictionary': D.png_container(6, 4, b'\x78\x20' + idat[2:]),
        'zlib header': D.png_container(6, 4, b'\x78\x02' + idat[2:]),
        'unknown critical': D.png_container(6, 4, idat, before=D.chunk(b'ABCD', b'')),
        'first chunk': good[:8] + text + good[8:],
        'no IEND': good[:-12],
        'cut short': good[:-3],
        'no IDAT': D.png_container(6, 4, b'', split=[])[:8 + 25] + D.chunk(b'IEND', b''),
    }
    for name, data in cases.items():
        with pytest.raises(ValueError, match=name):
            pngreader.parse(data)
    # what may stand between: ancillary chunks before and after the IDATs, several IDATs in a row
    assert bytes(pngreader.parse(D.png_container(6, 4, idat, split=[1, 7], before=text)).span) == idat[2:-4]
    for form, data in (('interlaced', D.png_container(6, 4, idat, interlace=1)),
                       ('16-bit', D.png_container(6, 4, idat, depth=16)),
                       ('palette', D.png_container(6, 4, idat, colour=3, before=D.chunk(b'PLTE', bytes(6)))),
                       ('depth below 8', D.png_container(6, 4, idat, colour=0, depth=4)),
                       ('grey with alpha', D.png_container(6, 4, idat, colour=4))):
        assert pngreader.parse(data) == pngreader.Unsupported(6, 4, form)


def test_a_defective_file_is_named(twin):
    picture = D.smooth_image(7, 33, seed=2, period=16)
    good = D.png_file(picture)
    stream = D.filter_stream(picture, [y % 5 for y in range(7)])
    with pytest.raises(ValueError, match=r'file 1: status 2 \(bad block type\)'):
        pngreader.decode([good, D.png_file(picture, deflate=b'\x07')], device='cpu')
    with pytest.raises(ValueError, match='file 0.*Adler'):
        pngreader.decode([D.png_file(picture, adler=(zlib.adler32(stream) ^ 1) & 0xffffffff), good], device='cpu')
    with pytest.raises(ValueError, match=r'file 2: status 12 \(bad filter type\)'):
        pngreader.decode([good, good, D.png_file(picture, types=[0, 1, 5, 3, 4, 0, 1])], device='cpu')
    with pytest.raises(ValueError, match='file 1.*signature'):
        pngreader.decode([good, b'not a png'], device='cpu')


def test_as_float_equals_load_image(tmp_path):
    picture = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)[:, :, ::-1].copy()
    picture[0, 0] = (0, 255, 128)
    path = str(tmp_path / 'all.png')
    PIL.Image.fromarray(picture).save(path)
    want = distances._load_image(path)
    got = pngreader.as_float(torch.from_numpy(picture)[None])
    assert got.shape == (1, 3, 16, 16) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got[0], want) and len(set(want.flatten().tolist())) == 256


def test_read_batch_and_load_image_set(tmp_path, twin):
    seeds = [3, 1, 4, 15, 9]
    pictures = {s: D.random_image(5, 6, seed=s) for s in seeds}
    for s in seeds:
        with open(str(tmp_path / ('image_%d.png' % s)), 'wb') as f:
            f.write(D.pil_file(pictures[s]))
    assert pngreader.MAX_READERS == 16
    chunks = list(pngreader.load_image_set(str(tmp_path), seeds, batch=2, device='cpu', readers=64))
    assert [c for c, _ in chunks] == [[3, 1], [4, 15], [9]]
    for chunk, images in chunks:
        assert tuple(images.shape) == (len(chunk), 5, 6, 3)
        for s, image in zip(chunk, images):
            assert np.array_equal(image.numpy(), pictures[s])
    with open(str(tmp_path / 'other.png'), 'wb') as f:
        f.write(D.pil_file(D.random_image(6, 5)))
    with pytest.raises(ValueError, match='one shape'):
        pngreader.read_batch([str(tmp_path / 'image_3.png'), str(tmp_path / 'other.png')], device='cpu')
    with open(str(tmp_path / 'bad.png'), 'wb') as f:
        f.write(b'junk')
    with pytest.raises(ValueError, match=r'file 1.*bad\.png'):
        pngreader.read_batch([str(tmp_path / 'image_3.png'), str(tmp_path / 'bad.png')], device='cpu')


def test_from_urls(twin):
    import base64
    files = [D.pil_file(D.random_image(3, 5, seed=s)) for s in (1, 2)]
    urls = ['data:image/png;base64,' + base64.b64encode(f).decode() for f in files]
    got = pngreader.from_urls(urls, device='cpu')
    assert all(np.array_equal(g.numpy(), D.pil_pixels(f)) for g, f in zip(got, files))
    with pytest.raises(ValueError, match='url 0'):
        pngreader.from_urls(['http://example/x.png'], device='cpu')
