"""PNG decoding on the device (hip.png_decode, rewriting_amd/pngreader.py): the pixels are PIL's, byte for byte -- the
format is fully specified and integer, so there is no tolerance -- on PIL-written files of every compression level, on
streams at the edge of the 32 KiB window and on hand-made streams no encoder writes; every defect gets the status the
numpy twin (tests/pngdec_checks.py) gives it, once, after the host program accepted the same list; a bad stream does not
disturb its neighbours; what is refused is refused before any launch; and the routes that use it (load_image_set,
compute_dl(device_decode=True)) end in exactly the values of the host route."""
import os
import zlib

import numpy as np
import PIL.Image
import pytest
import torch

from rewriting_amd import distances, hip, pngcode, pngreader, pngwriter
from tests import lpips_checks as L
from tests import pngdec_checks as D
from tests.search_checks import make_rewriter

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def decoded():
    """{name: (file, pixels from the device)}: the whole corpus in one pngreader.decode, one launch pair per shape"""
    files = D.corpus()
    pixels = pngreader.decode([f for _, f in files])
    return {name: (f, p.cpu().numpy()) for (name, f), p in zip(files, pixels)}


def _exact(decoded, wanted):
    names = [n for n in decoded if wanted(n)]
    for name in names:
        data, got = decoded[name]
        want = D.pil_pixels(data)
        assert got.shape == want.shape and np.array_equal(got, want), name
    return names


# ------------------------------------------------------------------------------------------ exactness against PIL
def test_small_shapes_at_every_level(decoded):
    names = _exact(decoded, lambda n: n.startswith('random') and '{' in n)
    assert len(names) == 5 * 4                             # 1x1, 1x2, 2x1, 3x5, 7x33 at compress_level 1, 6, 9 and optimize


def test_many_stored_blocks_and_idats(decoded):
    assert _exact(decoded, lambda n: n == 'random 160x160')


def test_smooth_content_dynamic_blocks_long_distances(decoded):
    assert len(_exact(decoded, lambda n: n.startswith('smooth 40x300'))) == 4


def test_flat_image_longest_matches_at_distance_one(decoded):
    assert _exact(decoded, lambda n: n == 'flat 40x300')


def test_three_window_wraps(decoded):
    assert _exact(decoded, lambda n: n == 'smooth 90x364')


@pytest.mark.parametrize('shape', D.EDGE_SHAPES, ids=lambda s: '%dx%d=%d' % s)
def test_stream_length_at_the_windows_edge(decoded, shape):
    h, w, _ = shape
    assert len(_exact(decoded, lambda n: n.endswith(' %dx%d' % (h, w)))) == 2             # random and smooth


def test_every_filter_type_and_channel_count(decoded):
    assert len(_exact(decoded, lambda n: n.startswith('filter'))) == 5
    assert len(_exact(decoded, lambda n: n.startswith('channels'))) == 6                  # grey, RGB, RGBA: PIL's and forced filters


# ------------------------------------------------------------------------------------------ hand-made streams
@pytest.mark.parametrize('case', D.hand_streams(), ids=lambda c: c[0])
def test_hand_made_stream(case):
    name, stream, out = case
    got, status = hip.png_inflate([stream], len(out))
    assert tuple(got.shape) == (1, -(-len(out) // 16) * 16)
    assert status.tolist() == [[D.OK, len(out)] + list(D.raw_sums(out))]
    assert got[0, :len(out)].cpu().numpy().tobytes() == out
    assert pngcode.adler_fold([tuple(status[0, 1:])]) == zlib.adler32(out) & 0xffffffff


# ------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize('shape', [(40, 300), (99, 110)], ids=lambda s: '%dx%d' % s)
def test_round_trip_through_png_encode(shape):
    h, w = shape
    images = np.stack([D.random_image(h, w, seed=1), D.smooth_image(h, w, seed=2), np.zeros((h, w, 3), np.uint8)])
    device = torch.from_numpy(images).cuda()
    files = hip.png_encode(device)
    back = torch.stack(pngreader.decode(files))
    assert torch.equal(back, device)
    # hip.png_decode takes whole files of the call's shape as well as bare streams, and refuses a file of another shape
    pixels, status = hip.png_decode(files, h, w, 3)
    assert torch.equal(pixels, device) and not status[:, 0].any()
    with pytest.raises(RuntimeError, match='file 1 is'):
        hip.png_decode([files[0], D.pil_file(D.random_image(3, 5))], h, w, 3)


def test_from_urls_inverts_as_urls():
    images = (torch.rand(3, 3, 20, 28, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    urls = pngwriter.as_urls(images)
    assert torch.equal(torch.stack(pngreader.from_urls(urls)), hip.render_bytes(images))


# ------------------------------------------------------------------------------------------ defects
def test_defects_get_the_twins_status(tmp_path, monkeypatch):
    h, w, channels = D.DEFECT_SHAPE
    defects = D.defect_streams()
    picture = D.smooth_image(h, w, seed=2, period=16)
    stream = D.filter_stream(picture, [y % 5 for y in range(h)])
    files = [D.png_file(picture, deflate=s) for _, s in defects]
    files.append(D.png_file(picture, adler=(zlib.adler32(stream) ^ 1) & 0xffffffff))       # a wrong Adler trailer
    files.append(D.png_file(picture, types=[0, 1, 5, 3, 4, 0, 1]))                         # filter type 5
    names = [n for n, _ in defects] + ['wrong Adler trailer', 'filter type 5']
    spans = [bytes(pngreader.parse(f).span) for f in files]
    # the host program first: the same core, the same list
    program = D.build_host_program(tmp_path, sanitize=False)
    on_host = D.run_host_program(program, [(s, 700) for s in spans], tmp_path)
    assert on_host == [D.twin_result(s, 700) for s in spans]
    # then the device, every stream once
    pixels, status = hip.png_decode(spans, h, w, channels)
    _, want = D.png_decode(spans, h, w, channels)
    for name, got, twin in zip(names, status.tolist(), want.tolist()):
        assert got == twin, name
    assert status[:15, 0].min() > 0 and status[15, 0] == D.OK and status[16, 0] == D.BAD_FILTER
    assert not pixels[:15].any() and np.array_equal(pixels[15].cpu().numpy(), picture)
    # pngreader names the file; the device's answers are replayed, not asked for again
    for k, name in enumerate(names):
        monkeypatch.setattr(hip, 'png_decode', lambda *a, _k=k, **kw: (pixels[_k:_k + 1], status[_k:_k + 1]))
        with pytest.raises(ValueError, match='file 0: (status %d|the Adler)' % status[k, 0]):
            pngreader.decode([files[k]])


def _mixed_batch():
    """70 files at 7 x 33 of mixed content and coded sizes; spans[35] is defective"""
    h, w = 7, 33
    files = []
    for k in range(70):
        if k % 5 == 0:
            image = D.random_image(h, w, seed=k)                                           # stored or nearly
        elif k % 5 == 1:
            image = D.smooth_image(h, w, seed=k, period=16)
        elif k % 5 == 2:
            image = np.full((h, w, 3), k, np.uint8)                                        # a few bytes
        elif k % 5 == 3:
            image = np.tile(D.random_image(1, 3, seed=k), (h, w // 3, 1))                  # matches
        else:
            image = (D.smooth_image(h, w, seed=k, period=16) // 32) * 32
        files.append(D.pil_file(image, **D.PIL_OPTIONS[k % 4]) if k % 2 else D.png_file(image, level=1 + k % 9))
    spans = [bytes(pngreader.parse(f).span) for f in files]
    spans[35] = dict(D.defect_streams())['distance one past the start']
    return files, spans


def test_a_bad_stream_among_good_ones():
    files, spans = _mixed_batch()
    assert len(set(len(s) for s in spans)) > 20
    pixels, status = hip.png_decode(spans, 7, 33, 3)
    code, out = D.inflate(spans[35], 700)
    assert status[35].tolist() == [code, len(out)] + list(D.raw_sums(out)) and code == D.DISTANCE_TOO_FAR
    assert not pixels[35].any()
    good = [k for k in range(70) if k != 35]
    assert not status[good, 0].any()
    for k in good:
        assert np.array_equal(pixels[k].cpu().numpy(), D.pil_pixels(files[k])), k
        alone, alone_status = hip.png_decode([spans[k]], 7, 33, 3)
        assert torch.equal(alone[0], pixels[k]) and np.array_equal(alone_status[0], status[k]), k
    again, again_status = hip.png_decode(spans, 7, 33, 3)
    assert torch.equal(again, pixels) and np.array_equal(again_status, status)
    # read in place from the middle of a larger buffer, the streams back to back at any alignment
    rng = np.random.RandomState(1)
    head, tail = bytes(rng.randint(0, 256, 1001, dtype=np.uint8)), bytes(rng.randint(0, 256, 77, dtype=np.uint8))
    offsets = np.cumsum([0] + [len(s) for s in spans[:-1]])
    big = torch.from_numpy(np.frombuffer(head + b''.join(spans) + tail, dtype=np.uint8).copy()).cuda()
    middle = big[len(head):len(big) - len(tail)]
    there, there_status = hip.png_decode((middle, np.stack([offsets, [len(s) for s in spans]], axis=1)), 7, 33, 3)
    assert torch.equal(there, pixels) and np.array_equal(there_status, status)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_before_any_launch(monkeypatch):
    launched = []
    real = hip.lib()
    for name in ('rw_png_inflate_u8', 'rw_png_unfilter_u8'):
        monkeypatch.setattr(real, name, lambda *a, _n=name: launched.append(_n) or 0)
    span = bytes(pngreader.parse(D.pil_file(D.random_image(4, 6))).span)
    coded = torch.from_numpy(np.frombuffer(span, dtype=np.uint8).copy()).cuda()
    whole = np.array([[0, len(span)]])
    for bad in ((coded.float(), whole), (coded.cpu(), whole), (coded[::2], whole), (coded[None], whole),
                (coded, np.array([[0, len(span) + 1]])), (coded, np.array([[5, len(span) - 4]])),
                (coded, np.array([[-1, 4]])), (coded, np.array([0, len(span)])), (coded, np.array([[0.0, 4.0]]))):
        with pytest.raises(RuntimeError):
            hip.png_decode(bad, 4, 6, 3)
    for h, w, channels in ((4, 6, 2), (4, 6, 0), (0, 6, 3), (4, 0, 3), (4, -1, 3), (2 ** 20, 2 ** 11, 1), (1, 16385, 3)):
        with pytest.raises(RuntimeError):
            hip.png_decode([span], h, w, channels)
    with pytest.raises(RuntimeError):
        hip.png_decode([span], 4, 6, 3, device='cpu')
    with pytest.raises(RuntimeError):
        hip.png_inflate([span], 0)
    out, status = hip.png_decode([], 4, 6, 3)
    assert tuple(out.shape) == (0, 4, 6, 3) and out.is_cuda and out.dtype == torch.uint8 and status.shape == (0, 4)
    out, status = hip.png_decode((coded, np.zeros((0, 2), dtype=np.int64)), 4, 6, 3)
    assert tuple(out.shape) == (0, 4, 6, 3) and status.shape == (0, 4)
    assert launched == []
    # the C entries themselves: nothing launched, the project's two codes
    monkeypatch.undo()
    BAD, UNSUPPORTED = 10001, 10002
    stream = torch.empty(1, 80, dtype=torch.uint8, device='cuda')
    st = torch.zeros(1, 4, dtype=torch.int32, device='cuda')
    spans = torch.tensor([[0, len(span)]], dtype=torch.int64, device='cuda')
    out = torch.empty(1, 4, 6, 3, dtype=torch.uint8, device='cuda')
    p, null = hip._p, hip._p(None)
    inflate, unfilter = real.rw_png_inflate_u8, real.rw_png_unfilter_u8
    assert inflate(null, p(spans), p(stream), 80, 76, p(st), 1, null) == BAD
    assert inflate(p(coded), p(spans), p(stream), 80, 76, p(st), 0, null) == BAD
    assert inflate(p(coded), p(spans), p(stream), 72, 76, p(st), 1, null) == BAD           # stride below expect
    assert inflate(p(coded), p(spans), p(stream), 80, 0, p(st), 1, null) == UNSUPPORTED
    assert inflate(p(coded), p(spans), p(stream), 2 ** 31, 2 ** 31, p(st), 1, null) == UNSUPPORTED
    assert unfilter(p(stream), 80, p(st), null, 1, 4, 6, 3, null) == BAD
    assert unfilter(p(stream), 80, p(st), p(out), 1, 4, 6, 2, null) == UNSUPPORTED
    assert unfilter(p(stream), 80, p(st), p(out), 1, 0, 6, 3, null) == UNSUPPORTED
    assert unfilter(p(stream), 80, p(st), p(out), 1, 2 ** 20, 2 ** 11, 1, null) == UNSUPPORTED
    assert unfilter(p(stream), 64, p(st), p(out), 1, 4, 6, 3, null) == BAD                 # stride below H (1 + 3 W)
    torch.cuda.synchronize()
    assert not st.any()


# ------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def rewriter():
    return make_rewriter('cuda', 32, 10, 4, device_render=True)


def test_load_image_set_inverts_save_image_set(tmp_path, rewriter):
    from rewriting_amd import samples
    model, seeds = rewriter.model, [3, 1, 4, 15, 9]
    pngwriter.save_image_set(model, model, seeds, str(tmp_path), batch=2, shard=None)
    want = {}
    for chunk, images in samples.generate(model, model, seeds, batch=2, shard=None):
        want.update(zip(chunk, hip.render_bytes(images.contiguous())))
    chunks = list(pngreader.load_image_set(str(tmp_path), seeds, batch=3))
    assert [c for c, _ in chunks] == [[3, 1, 4], [15, 9]]
    for chunk, images in chunks:
        assert images.is_cuda and tuple(images.shape) == (len(chunk), 32, 32, 3)
        for seed, image in zip(chunk, images):
            assert torch.equal(image, want[seed]), seed


@pytest.fixture(scope='module')
def pairs(tmp_path_factory, rewriter):
    """Two sets of 12 before / after pairs at 32 x 32 with segmentations: files written by PIL, and by save_image_set"""
    root = tmp_path_factory.mktemp('pairs')
    before, after, seg = L.edit_set(n=12, size=32)
    keys = list(range(100, 112))
    sets = {}
    for name in ('pil', 'device'):
        dirs = [str(root / name / d) for d in ('before', 'after', 'seg')]
        for d in dirs:
            os.makedirs(d)
        for k, key in enumerate(keys):
            torch.save(torch.stack([seg[k] * 0, seg[k] + 1, seg[k]]), os.path.join(dirs[2], '%d.pth' % key))
        sets[name] = dirs
    for images, d in ((before, sets['pil'][0]), (after, sets['pil'][1])):
        data = ((images.permute(0, 2, 3, 1) + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).numpy()
        for key, picture in zip(keys, data):
            PIL.Image.fromarray(picture).save(os.path.join(d, '%d.png' % key))
    model = rewriter.model
    pngwriter.save_image_set(model, model, keys, sets['device'][0], name_template='{}.png', batch=5, shard=None)
    pngwriter.save_image_set(model, model, keys, sets['device'][1], name_template='{}.png', batch=5, shard=None, offset=1000)
    return keys, sets


@pytest.mark.parametrize('writer', ['pil', 'device'])
@pytest.mark.parametrize('mode', distances.MODES)
def test_compute_dl_device_decode_is_bit_identical(pairs, mode, writer):
    from rewriting_amd import lpips
    keys, sets = pairs
    net = None if mode == 'pixel' else lpips.from_state_dicts(*L.weights()).to('cuda')
    before_dir, after_dir, seg_dir = sets[writer]
    kwargs = dict(src=(2, 3), srcc=2, mode=mode, batch_size=5, net=net)     # the changed region is class 1: it counts
    want = distances.compute_dl(before_dir, after_dir, seg_dir, keys, **kwargs)
    got = distances.compute_dl(before_dir, after_dir, seg_dir, keys, device_decode=True, **kwargs)
    print('compute_dl %s %s: %r' % (mode, writer, got))
    assert got == want and want[0] > 0 and want[1] > 0
