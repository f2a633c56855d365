"""TEST INFRASTRUCTURE -- records WHICH kernel wrappers of ``rewriting_amd.hip`` a generator forward launches, in
order and with which arguments: the routing decisions of utils/stylegan2/models.py made visible.

``record(device)`` runs one model per size through every (context, switch setting) of ``CONTEXTS`` x ``SETTINGS`` with a
spy around every launching wrapper (conv*, pack_*, to_rgb, rgb_combine, blur_noise_act, noise_add, style_mul, absmax,
new_bound) and returns ``{'<size>/b<batch>/<context>/<switches>': [call, ...]}``; a call reads
``name input-shape out_ch impl further,arguments,that,are,not,None,or,False``.  tests/test_routes.py compares that with the tables
under tests/golden/ (``routes_cpu.json``: the emulated path; ``routes_gpu.json``: the real wrappers, which reach the
routes that need device streams).  After adding a route ON PURPOSE, regenerate them:

    python -m tests.route_spy cpu tests/golden/routes_cpu.json
    python -m tests.route_spy cuda tests/golden/routes_gpu.json

On the CPU the 64^2 model runs on tests/hip_emulation.py; 256^2 and 1024^2 run on shape-only stand-ins (``torch.empty``
of the right shape, a filled bound where one is asked for): the route depends on shapes, never on values.
"""
import inspect
import json
import os
import sys

import torch

BATCH = 2
CPU_SIZES = (64, 256, 1024)
GPU_SIZES = (256, 1024)
CONTEXTS = ('unhooked', 'hooked', 'nofuse', 'grad')     # hooked: layer7 retained; nofuse: RW_FUSE=0; grad: layer10's weight
SETTINGS = [
    {},
    {'RW_MM': 'f32'},
    {'RW_MM_DIRECT16': '0'},
    {'RW_MM_DIRECT16': '1'},
    {'RW_UP_FUSED2': '0'},
    {'RW_UP_FUSED': '0'},
    {'RW_UP_ALGO': 'direct'},
    {'RW_UP_ALGO': 'winograd4'},
    {'RW_CONV_ALGO': 'direct'},
    {'RW_CONV_ALGO': 'winograd'},
    {'RW_CONV_ALGO': 'winograd4'},
    {'RW_CONV_PRECISION': 'bf16x6'},
    {'RW_CONV_IMPL': 'generic'},
    {'RW_PRESCALE': '0'},
    {'RW_RGB_F4': '0'},
    {'RW_DIRECT16_SMALL': '0'},
    {'RW_DIRECT16_HOOKED': '0'},
    {'RW_MM_HOOKED': 'f32'},
    {'RW_UP_FUSED2_HOOKED': '0'},
    {'RW_UP_FUSED2_MAX_IN': '64'},
    {'RW_DCONV_WS_FWD': '0'},
    {'RW_MM_PARTS': 'w4'},
    {'RW_FUSE_FINAL_RGB': '0'},
    {'RW_MICRO_BATCH': '1:256'},
    {'RW_RGB_PARTIAL': '0'},
    {'RW_MM': 'split', 'RW_MM_PARTS': 'up'},
    {'RW_UP_FUSED2': '0', 'RW_MM_DIRECT16': '0'},
    # tests/test_gpu_zz_sequences.py CONFIGS (its first two are the default and RW_PRESCALE=0 above)
    {'RW_PRESCALE': '0', 'RW_UP_FUSED': '0', 'RW_RGB_F4': '0'},
    {'RW_PRESCALE': '0', 'RW_UP_FUSED': '0', 'RW_RGB_F4': '0', 'RW_CONV_ALGO': 'winograd'},
]
_EXTRA = ('to_rgb', 'rgb_combine', 'blur_noise_act', 'noise_add', 'style_mul', 'absmax', 'new_bound')


def launchers(hip):
    return sorted(n for n in dir(hip) if callable(getattr(hip, n)) and not n.endswith(('_supported', '_applicable'))
                  and (n.startswith(('conv', 'pack_')) or n in _EXTRA))


def key_of(size, context, env):
    return '%d/b%d/%s/%s' % (size, BATCH, context, ' '.join('%s=%s' % kv for kv in sorted(env.items())) or 'default')


def keys(sizes):
    return [key_of(s, c, e) for s in sizes for c in CONTEXTS for e in SETTINGS]


def _spy(name, fn, log):
    params = inspect.signature(fn).parameters
    named = [p for p in list(params)[1:] if p not in ('out_ch', 'impl')]

    def spied(*args, **kwargs):
        got = dict(zip(params, args), **kwargs)
        first = args[0] if args else None
        shape = 'x'.join(map(str, first.shape)) if torch.is_tensor(first) else str(first)
        on = sorted(p for p in named if got.get(p) is not None and got.get(p) is not False)
        log.append('%s %s %s %s %s' % (name, shape, got.get('out_ch', '-'), got.get('impl', '-'), ','.join(on) or '-'))
        return fn(*args, **kwargs)
    return spied


def install_spies(monkeypatch, log):
    from rewriting_amd import hip
    for name in launchers(hip):
        monkeypatch.setattr(hip, name, _spy(name, getattr(hip, name), log))


# ---- shape-only stand-ins for the emulated kernels (the large CPU sizes) -----------------------------------------

class _SplitPack:
    """what a pack_*(split=True) stand-in returns: the kernels measure their input when they are handed one"""


def _bounds(x, x_amax, y_amax, measures=True):
    from rewriting_amd import hip
    if measures and x_amax is None:
        hip.absmax(x)                       # hip._amax_in
    if y_amax is not None:
        y_amax[:64] = 1.0


def _stub_conv(scale_h=1, grow=0, always_split=False, takes_out=False):
    def stub(x, wp, *args, **kw):
        out_ch = kw['out_ch'] if 'out_ch' in kw else args[1] if always_split == 'fused' else args[0]
        b, _, h, w = x.shape
        if 'x_amax' in kw or 'y_amax' in kw or always_split:
            _bounds(x, kw.get('x_amax'), kw.get('y_amax'), measures=bool(always_split) or isinstance(wp, _SplitPack))
        if takes_out and kw.get('out') is not None:
            return kw['out']
        return torch.empty(b, out_ch, scale_h * h + grow, scale_h * w + grow)
    return stub


def _stub_pack(weight, *args, **kw):
    return _SplitPack() if kw.get('split') or (args and args[-1] is True) else torch.empty(1)


def _stub_blur_noise_act(x, k4, noise, noise_w, bias, post_scale=None, y_amax=None):
    _bounds(x, None, y_amax, measures=False)
    return torch.empty(x.shape[0], x.shape[1], x.shape[2] - 1, x.shape[3] - 1)


def _stub_upfirdn2d_major(x, k, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    n, h, w, c = x.shape
    return torch.empty(n, (h * up_y + py0 + py1 - k.shape[0]) // down_y + 1,
                       (w * up_x + px0 + px1 - k.shape[1]) // down_x + 1, c)


def _stub_absmax(x):
    return torch.ones(64 + 2048 + 1)


def install_stubs(monkeypatch):
    from rewriting_amd import hip
    same = lambda x, *a, **k: torch.empty(x.shape)
    stubs = {
        'conv3x3': _stub_conv(), 'conv3x3_wino': _stub_conv(), 'conv3x3_bf16x6': _stub_conv(),
        'conv3x3_wino4': _stub_conv(), 'conv3x3_direct16': _stub_conv(always_split=True),
        'conv_transpose3x3s2': _stub_conv(2, 1, takes_out=True), 'conv_transpose3x3s2_wino': _stub_conv(2, 1, takes_out=True),
        'conv_transpose3x3s2_blur_wino4': _stub_conv(2), 'conv_transpose3x3s2_blur_direct16': _stub_conv(2, always_split=True),
        'conv_transpose3x3s2_blur_fused': _stub_conv(2, always_split='fused'),
        'blur_noise_act': _stub_blur_noise_act, 'absmax': _stub_absmax,
        'to_rgb': lambda x, *a, **k: torch.empty(x.shape[0], 3, x.shape[2], x.shape[3]),
        'style_mul': same, 'noise_add': same, 'fused_bias_act': same, 'upfirdn2d_major': _stub_upfirdn2d_major,
    }
    for name in launchers(hip):
        if name.startswith('pack_'):
            stubs[name] = lambda *a, **k: _stub_pack(*a, **k)
    for name, fn in stubs.items():
        fn.__signature__ = inspect.signature(getattr(hip, name))       # what the spy reads argument names from
        monkeypatch.setattr(hip, name, fn)


# ---- the runs ----------------------------------------------------------------------------------------------------

def _forward(model, z, context):
    from rewriting_amd.utils import nethook
    if context == 'hooked':
        with torch.no_grad(), nethook.InstrumentedModel(model) as inst:
            inst.retain_layer('layer7', detach=False)
            inst(z)
    elif context == 'grad':
        weight = model.layer10.sconv.mconv.dconv.weight
        weight.requires_grad_(True)
        try:
            with torch.enable_grad():
                model(z)
        finally:
            weight.requires_grad_(False)
    else:
        with torch.no_grad():
            model(z)
    if z.is_cuda:
        torch.cuda.synchronize()


def record_size(monkeypatch, size, device, wanted=None):
    """{key: [call, ...]} of one size; monkeypatch: a pytest.MonkeyPatch that the caller undoes."""
    from rewriting_amd.utils import nethook
    from tests import hip_emulation
    from tests.conftest import build_stylegan
    for name in [n for n in os.environ if n.startswith('RW_')]:
        monkeypatch.delenv(name)
    if device == 'cpu':
        hip_emulation.install(monkeypatch)
        if size > 64:
            install_stubs(monkeypatch)
    log = []
    install_spies(monkeypatch, log)
    model = build_stylegan(size, 0.7, device=device)
    nethook.set_requires_grad(False, model)
    z = torch.randn(BATCH, 512, generator=torch.Generator().manual_seed(9)).to(device)
    table = {}
    for context in CONTEXTS:
        for env in SETTINGS:
            key = key_of(size, context, env)
            if wanted is not None and key not in wanted:
                continue
            with monkeypatch.context() as mp:
                for name, value in env.items():
                    mp.setenv(name, value)
                if context == 'nofuse':
                    mp.setenv('RW_FUSE', '0')
                for m in model.modules():           # every configuration packs its own weights
                    if hasattr(m, '_derived'):
                        m._derived.store.clear()
                del log[:]
                try:
                    _forward(model, z, context)
                except RuntimeError as e:           # the fused last layer of a sliced batch asks for the device's stream
                    if device != 'cpu' or 'No HIP GPUs' not in str(e):
                        raise
                    log.append('raised: no GPU')
                table[key] = list(log)
    return table


def save(table, path):
    calls = []
    index = {}
    routes = {}
    for key, log in table.items():
        routes[key] = [index.setdefault(c, len(index)) for c in log]
    calls = sorted(index, key=index.get)
    with open(path, 'w') as f:
        f.write('{"calls": [\n' + ',\n'.join(json.dumps(c) for c in calls) + '\n],\n"routes": {\n')
        f.write(',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in routes.items()))
        f.write('\n}}\n')


def load(path):
    with open(path) as f:
        data = json.load(f)
    return {key: [data['calls'][i] for i in idx] for key, idx in data['routes'].items()}


if __name__ == '__main__':
    import pytest
    device, path = sys.argv[1], sys.argv[2]
    import time
    t0 = time.time()
    table = {}
    for size in (CPU_SIZES if device == 'cpu' else GPU_SIZES):
        with pytest.MonkeyPatch.context() as mp:
            table.update(record_size(mp, size, device))
        print('recorded', size, len(table), time.time() - t0, flush=True)
    save(table, path)
