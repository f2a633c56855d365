"""How the wrappers of rewriting_amd/hip.py call the C ABI, pinned against tests/golden/hip_calls.json WITHOUT launching
anything: every rw_* entry a wrapper under test reaches is replaced on the loaded library by a recorder that returns 0.

One record per call of an entry: its name, the scalars by value and every pointer as a label -- the named input it is
("x", "latent+64": 64 bytes into it), "fresh0 (2, 32, 8, 64) float32" for a tensor the wrapper allocated (numbered in the
order the entries first see them), "null", or the fields of an epilogue struct.  What the wrapper returned is recorded
the same way, so that "the result is the buffer the entry wrote" and "out= comes back itself" are part of the record.
The pure functions (rw_packed_*, rw_*_supported, rw_bound_floats, rw_dconv3x3_rgb_partials) stay real.

The table is recorded with this module's own recorder at the commit BEFORE a change to the wrappers:

    python -m tests.test_gpu_hip_calls --record
"""
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rewriting_amd import _lib, hip  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = os.path.join(ROOT, 'tests', 'golden', 'hip_calls.json')
B, O, I, H, W = 2, 32, 16, 8, 64         # a non-square channel pair: a swapped in_ch / out_ch cannot cancel
GLUE = ('pixel_norm', 'equal_linear', 'adjust_latent', 'style_mul', 'weight_sqsum', 'demod', 'noise_add', 'to_rgb')
RECORDED = [
    'rw_absmax_f32', 'rw_conv3x3_f32', 'rw_conv3x3_to_rgb_f32', 'rw_conv3x3_wino_f32', 'rw_conv3x3_wino_to_rgb_f32',
    'rw_conv3x3_wino4_f32', 'rw_conv3x3_wino4h_f32', 'rw_conv3x3_wino4_to_rgb_f32', 'rw_conv3x3_wino4h_to_rgb_f32',
    'rw_conv3x3_bf16x6_f32', 'rw_conv_transpose3x3s2_f32', 'rw_conv_transpose3x3s2_wino_f32',
    'rw_conv_transpose3x3s2_winoh_f32', 'rw_conv_transpose3x3s2_blur_wino4_f32',
    'rw_conv_transpose3x3s2_blur_wino4h_f32', 'rw_dconv3x3_f32', 'rw_dconv3x3_rgb_partial_f32', 'rw_dconv3x3_to_rgb_f32',
    'rw_dconv_transpose3x3s2_blur_f32', 'rw_tconv_blur_f32', 'rw_conv3x3_f64', 'rw_conv_transpose3x3s2_f64',
] + ['rw_%s_%s' % (op, sfx) for op in GLUE for sfx in ('f32', 'f64')]


class Session:
    """The recorders, the named inputs of one case and the tensors the wrapper allocates during it."""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch
        self.calls, self.named, self.fresh, self.seen = [], [], [], []
        for name in RECORDED:
            monkeypatch.setattr(hip.lib(), name, lambda *a, _n=name: self.calls.append([_n] + [self.value(v) for v in a]) or 0)

    def tensor(self, name, *shape, dtype=torch.float32):
        t = torch.empty(*shape, device='cuda', dtype=dtype)
        self.named.append((name, t))
        return t

    def label(self, ptr):
        if not ptr:
            return 'null'
        if ptr == torch.cuda.current_stream().cuda_stream:
            return 'stream'
        for name, t in self.named:
            if 0 <= ptr - t.data_ptr() < t.numel() * t.element_size():
                return name if ptr == t.data_ptr() else '%s+%d' % (name, ptr - t.data_ptr())
        for t in self.fresh:
            if ptr == t.data_ptr():
                if not any(s is t for s in self.seen):
                    self.seen.append(t)
                k = [s is t for s in self.seen].index(True)
                return 'fresh%d %s %s' % (k, tuple(t.shape), str(t.dtype).replace('torch.', ''))
        return 'unknown pointer'

    def value(self, v):
        if isinstance(v, ctypes.c_void_p):
            return self.label(v.value)
        if hasattr(v, '_obj'):                                                  # ctypes.byref(struct)
            return {f: self.label(getattr(v._obj, f)) if c is ctypes.c_void_p else getattr(v._obj, f)
                    for f, c in v._obj._fields_}
        assert isinstance(v, (int, float)), v
        return v

    def returned(self, r):
        if r is None:
            return None
        if isinstance(r, tuple):
            return [self.returned(t) for t in r]
        return self.label(r.data_ptr())

    def run(self, fn, *args, **kwargs):
        """{'calls': ..., 'returned': ...} of fn(*args, **kwargs): its allocations are kept alive (no address is used
        twice) and labelled by shape."""
        self.calls, self.fresh, self.seen = [], [], []
        with pytest.MonkeyPatch.context() as mp:
            for alloc in ('empty', 'empty_like'):
                mp.setattr(torch, alloc, lambda *a, _real=getattr(torch, alloc), **k: self.fresh.append(_real(*a, **k)) or self.fresh[-1])
            r = fn(*args, **kwargs)
        return {'calls': self.calls, 'returned': self.returned(r)}


def packed(elems, split):
    t = torch.empty(int(elems), device='cuda')
    if split:
        t.rw_u_inv = 0.03125
    return t


def conv_cases(s):
    """{case: record} of the fourteen convolution wrappers, each bare (every optional operand absent, bounds measured)
    and full (every one given), with plain and with split weights where the wrapper takes both."""
    L = hip.lib()
    x = s.tensor('x', B, I, H, W)
    x8 = s.tensor('x8', B, I, 8, 8)
    k4 = s.tensor('k4', 4, 4)
    ep = dict(style=s.tensor('style', B, I), demod=s.tensor('demod', B, O), noise=s.tensor('noise', B, 1, H, W),
              noise_w=s.tensor('noise_w', 1), bias=s.tensor('bias', O), act=True)
    up_noise = dict(ep, noise=s.tensor('up_noise', B, 1, 2 * H, 2 * W))
    mod = dict(style=ep['style'], demod=ep['demod'])
    rgb_bare = (s.tensor('rgb_weight', 3, O), s.tensor('rgb_style', B, O), None, None, 0.125)
    rgb_full = rgb_bare[:2] + (s.tensor('rgb_bias', 3), s.tensor('rgb_skip', B, 3, H, W), 0.125)
    post = s.tensor('post_scale', B, O)
    x_amax = s.tensor('x_amax', hip.BOUND_LANES)
    y_amax = s.tensor('y_amax', hip.bound_floats(B * O * H * W))
    y_amax_up = s.tensor('y_amax_up', hip.bound_floats(B * O * 4 * H * W))
    out = s.tensor('out', B, O, 2 * H + 1, 2 * W + 1)
    out8 = s.tensor('out8', B, O, 17, 17)

    def w(name, entry, split=False, *extra):
        n = getattr(L, entry)(O, I, *extra)
        t = packed(n // 4 if entry.endswith('_bytes') else n, split)
        s.named.append((name, t))
        return t
    wp0, wp1 = w('wp', 'rw_packed_conv_weight_elems', False, 0), w('wp_up', 'rw_packed_conv_weight_elems', False, 1)
    wb = w('wb', 'rw_packed_conv_weight_bf16x3_bytes')
    wino = w('uf_wino', 'rw_packed_conv_weight_wino_elems')
    w4 = {'plain': w('uf_wino4', 'rw_packed_conv_weight_wino4_elems'),
          'split': w('uf_wino4h', 'rw_packed_conv_weight_wino4h_elems', True)}
    upw = {'plain': w('uf_up', 'rw_packed_conv_transpose_wino_elems'),
           'split': w('uf_uph', 'rw_packed_conv_transpose_winoh_elems', True)}
    upw4 = {'plain': w('uf_up4', 'rw_packed_conv_transpose_blur_wino4_elems'),
            'split': w('uf_up4h', 'rw_packed_conv_transpose_blur_wino4h_elems', True)}
    d16 = w('wp_d16', 'rw_packed_dconv_weight_elems', True)
    d16up = w('wp_d16up', 'rw_packed_dconv_transpose_blur_weight_elems', True)

    c = {}
    c['conv3x3 bare'] = s.run(hip.conv3x3, x, wp0, O, 0.5)
    c['conv3x3 full impl=3'] = s.run(hip.conv3x3, x, wp0, O, 0.5, impl=3, **ep)
    c['conv3x3_to_rgb bare'] = s.run(hip.conv3x3_to_rgb, x, wp0, O, 0.5, *rgb_bare)
    c['conv3x3_to_rgb full store_fmap'] = s.run(hip.conv3x3_to_rgb, x, wp0, O, 0.5, *rgb_full, store_fmap=True, **ep)
    c['conv3x3_wino bare'] = s.run(hip.conv3x3_wino, x, wino, O, 0.5)
    c['conv3x3_wino full'] = s.run(hip.conv3x3_wino, x, wino, O, 0.5, **ep)
    c['conv3x3_wino 8x8 style'] = s.run(hip.conv3x3_wino, x8, wino, O, 0.5, **mod)
    c['conv3x3_wino_to_rgb bare'] = s.run(hip.conv3x3_wino_to_rgb, x, wino, O, 0.5, *rgb_bare)
    c['conv3x3_wino_to_rgb full store_fmap'] = s.run(hip.conv3x3_wino_to_rgb, x, wino, O, 0.5, *rgb_full, store_fmap=True,
                                                     **ep)
    for form in ('plain', 'split'):
        c['conv3x3_wino4 %s bare' % form] = s.run(hip.conv3x3_wino4, x, w4[form], O, 0.5)
        c['conv3x3_wino4 %s full' % form] = s.run(hip.conv3x3_wino4, x, w4[form], O, 0.5, x_amax=x_amax, y_amax=y_amax, **ep)
        c['conv3x3_wino4_to_rgb %s bare' % form] = s.run(hip.conv3x3_wino4_to_rgb, x, w4[form], O, 0.5, *rgb_bare)
        c['conv3x3_wino4_to_rgb %s full' % form] = s.run(hip.conv3x3_wino4_to_rgb, x, w4[form], O, 0.5, *rgb_full,
                                                         x_amax=x_amax, **ep)
        c['conv_transpose3x3s2_wino %s bare' % form] = s.run(hip.conv_transpose3x3s2_wino, x, upw[form], O, 0.5)
        c['conv_transpose3x3s2_wino %s full' % form] = s.run(hip.conv_transpose3x3s2_wino, x, upw[form], O, 0.5, out=out,
                                                             x_amax=x_amax, **mod)
        c['conv_transpose3x3s2_wino %s 8x8 style' % form] = s.run(hip.conv_transpose3x3s2_wino, x8, upw[form], O, 0.5,
                                                                  out=out8, **mod)
        c['conv_transpose3x3s2_blur_wino4 %s bare' % form] = s.run(hip.conv_transpose3x3s2_blur_wino4, x, upw4[form], O, 0.5)
        c['conv_transpose3x3s2_blur_wino4 %s full' % form] = s.run(
            hip.conv_transpose3x3s2_blur_wino4, x, upw4[form], O, 0.5, post_scale=post, x_amax=x_amax, y_amax=y_amax_up,
            **up_noise)
    c['conv3x3_bf16x6 bare'] = s.run(hip.conv3x3_bf16x6, x, wb, O, 0.5)
    c['conv3x3_bf16x6 full'] = s.run(hip.conv3x3_bf16x6, x, wb, O, 0.5, **ep)
    c['conv_transpose3x3s2 bare'] = s.run(hip.conv_transpose3x3s2, x, wp1, O, 0.5)
    c['conv_transpose3x3s2 full impl=8 out'] = s.run(hip.conv_transpose3x3s2, x, wp1, O, 0.5, impl=8, out=out, **mod)
    c['conv3x3_direct16 bare'] = s.run(hip.conv3x3_direct16, x, d16, O, 0.5)
    c['conv3x3_direct16 full'] = s.run(hip.conv3x3_direct16, x, d16, O, 0.5, x_amax=x_amax, y_amax=y_amax, **ep)
    c['conv3x3_direct16_rgb_partial bare'] = s.run(hip.conv3x3_direct16_rgb_partial, x, d16, O, 0.5, *rgb_bare[:2], 0.125)
    c['conv3x3_direct16_rgb_partial full'] = s.run(hip.conv3x3_direct16_rgb_partial, x, d16, O, 0.5, *rgb_bare[:2], 0.125,
                                                   x_amax=x_amax, y_amax=y_amax, **ep)
    c['conv3x3_direct16_to_rgb bare'] = s.run(hip.conv3x3_direct16_to_rgb, x, d16, O, 0.5, *rgb_bare)
    c['conv3x3_direct16_to_rgb full'] = s.run(hip.conv3x3_direct16_to_rgb, x, d16, O, 0.5, *rgb_full, x_amax=x_amax, **ep)
    c['conv_transpose3x3s2_blur_direct16 bare'] = s.run(hip.conv_transpose3x3s2_blur_direct16, x, d16up, O, 0.5)
    c['conv_transpose3x3s2_blur_direct16 full'] = s.run(hip.conv_transpose3x3s2_blur_direct16, x, d16up, O, 0.5,
                                                        post_scale=post, x_amax=x_amax, y_amax=y_amax_up, **up_noise)
    c['conv_transpose3x3s2_blur_fused bare'] = s.run(hip.conv_transpose3x3s2_blur_fused, x, d16, k4, O, 0.5)
    c['conv_transpose3x3s2_blur_fused full'] = s.run(hip.conv_transpose3x3s2_blur_fused, x, d16, k4, O, 0.5,
                                                     post_scale=post, x_amax=x_amax, y_amax=y_amax_up, **up_noise)
    return c


def glue_cases(s, dtype):
    """{case: record} of the eight glue wrappers (and, in double, the two convolutions) on tensors of `dtype`."""
    sfx = '' if dtype == torch.float32 else '_f64'
    op = lambda name: getattr(hip, name + sfx)                          # noqa: E731

    def t(name, *shape):
        return s.tensor(name, *shape, dtype=dtype)
    x, style = t('x', B, I, H, W), t('style', B, I)
    latent, z = t('latent', B, 3, 24), t('z', B, 24)
    lin_w, lin_b = t('linear_weight', 40, 24), t('linear_bias', 40)
    weight = t('weight', 1, O, I, 3, 3)
    c = {}
    c['pixel_norm'] = s.run(op('pixel_norm'), z)
    c['pixel_norm eps'] = s.run(op('pixel_norm'), z, 1e-6)
    c['equal_linear bare'] = s.run(op('equal_linear'), z, lin_w, None, 0.25, 0.01)
    c['equal_linear full'] = s.run(op('equal_linear'), z, lin_w, lin_b, 0.25, 0.01, act=True, alpha=0.1, act_scale=1.5)
    c['equal_linear row view'] = s.run(op('equal_linear'), latent[:, 1], lin_w, lin_b, 0.25, 0.01)
    c['adjust_latent bare'] = s.run(op('adjust_latent'), z, None, 5, 1.0)
    c['adjust_latent avg'] = s.run(op('adjust_latent'), z, t('latent_avg', 24), 5, 0.75)
    c['style_mul'] = s.run(op('style_mul'), x, style)
    c['weight_sqsum'] = s.run(op('weight_sqsum'), weight, 0.5)
    c['demod'] = s.run(op('demod'), t('wsq', O, I), style)
    c['demod eps'] = s.run(op('demod'), t('wsq', O, I), style, 1e-6)
    c['noise_add'] = s.run(op('noise_add'), x, t('noise', B, 1, H, W), t('noise_w', 1))
    rgb_w, skip = t('rgb_weight', 1, 3, I, 1, 1), t('skip', B, 3, H, W)
    c['to_rgb bare'] = s.run(op('to_rgb'), x, rgb_w, style, None, None, 0.25)
    c['to_rgb full'] = s.run(op('to_rgb'), x, rgb_w, style, t('rgb_bias', 1, 3, 1, 1), skip, 0.25)
    if dtype == torch.float64:
        c['conv3x3_f64 bare'] = s.run(hip.conv3x3_f64, x, weight, 0.5)
        c['conv3x3_f64 full'] = s.run(hip.conv3x3_f64, x, weight, 0.5, style=style, demod=t('demod', B, O))
        c['conv_transpose3x3s2_f64 bare'] = s.run(hip.conv_transpose3x3s2_f64, x, weight, 0.5)
        c['conv_transpose3x3s2_f64 full'] = s.run(hip.conv_transpose3x3s2_f64, x, weight, 0.5, style=style,
                                                  demod=t('demod', B, O))
    return c


GROUPS = {'conv': conv_cases, 'glue_f32': lambda s: glue_cases(s, torch.float32),
          'glue_f64': lambda s: glue_cases(s, torch.float64)}


def observe(group, monkeypatch):
    with torch.cuda.stream(torch.cuda.Stream()):             # a stream of its own: its handle is not the null pointer
        got = GROUPS[group](Session(monkeypatch))
    return json.loads(json.dumps(got))                       # as the table stores it: tuples are lists


def _table():
    with open(TABLE) as f:
        return json.load(f)


@pytest.mark.parametrize('group', sorted(GROUPS))
def test_wrappers_call_the_abi_as_recorded(group, monkeypatch):
    got, want = observe(group, monkeypatch), _table()['calls'][group]
    assert sorted(got) == sorted(want)
    for case in want:
        assert 'unknown pointer' not in json.dumps(got[case]), (case, got[case])
        assert got[case] == want[case], '%s:\n now      %s\n recorded %s' % (case, got[case], want[case])


def test_every_recorded_entry_is_reached_and_declared(monkeypatch):
    assert set(RECORDED) <= set(_lib.SIGNATURES)
    reached = {call[0] for group in GROUPS for rec in observe(group, monkeypatch).values() for call in rec['calls']}
    assert reached == set(RECORDED)


@pytest.mark.parametrize('dtype', (torch.float32, torch.float64), ids=('f32', 'f64'))
def test_glue_ops_refuse_misshaped_operands_before_any_call(dtype, monkeypatch):
    """The kernels index style / noise / skip by the feature map's shape: an operand of another shape is a ValueError,
    in both dtypes, and no entry is reached."""
    s = Session(monkeypatch)
    sfx = '' if dtype == torch.float32 else '_f64'
    op = lambda name: getattr(hip, name + sfx)                          # noqa: E731

    def t(*shape):
        return s.tensor('operand', *shape, dtype=dtype)
    x, style, rgb_w = t(B, I, H, W), t(B, I), t(1, 3, I, 1, 1)
    for fn, args in ((op('style_mul'), (x, t(B, I + 1))),
                     (op('style_mul'), (x, t(B + 1, I))),
                     (op('demod'), (t(O, I), t(B, I + 1))),
                     (op('noise_add'), (x, t(B, 1, H, W - 1), t(1))),
                     (op('to_rgb'), (x, t(1, 3, I + 1, 1, 1), style, None, None, 0.25)),
                     (op('to_rgb'), (x, rgb_w, t(B, I + 1), None, None, 0.25)),
                     (op('to_rgb'), (x, rgb_w, style, None, t(B, 3, H, W + 1), 0.25)),
                     (op('equal_linear'), (t(B, 24), t(40, 25), None, 0.25, 0.01))):
        with pytest.raises(ValueError):
            fn(*args)
    assert s.calls == []


def update_table(key, value):
    table = _table() if os.path.exists(TABLE) else {}
    table[key] = value
    with open(TABLE, 'w') as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s of %s' % (key, TABLE))


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], __doc__
    with pytest.MonkeyPatch.context() as mp:
        calls = {group: observe(group, mp) for group in sorted(GROUPS)}
    assert 'unknown pointer' not in json.dumps(calls)
    update_table('calls', calls)
