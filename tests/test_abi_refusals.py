"""What the C entries of the convolution families REFUSE -- the convolutions and the entries that measure and pack their
weights -- and the full tables of the pure shape / size functions, pinned against tests/golden/abi_refusals.json.

The table is recorded with this module's own recorder against a library built from the commit BEFORE a change to the
launchers (never from the changed tree):

    python -m tests.test_abi_refusals --record path/to/parent/librewriting_hip.so

A launching entry is only ever called with a case whose recorded status is RW_ERR_BAD_ARGUMENT (10001) or
RW_ERR_UNSUPPORTED (10002): nothing was launched, so the placeholder pointers are never dereferenced.  The recorder
refuses to write anything else.  Where a HIP device is visible the launching cases are skipped -- a refusal that
regressed must not turn into a launch on placeholder pointers; the pure-function tables run everywhere.
"""
import ctypes
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rewriting_amd import _lib  # noqa: E402

TABLE = os.path.join(ROOT, 'tests', 'golden', 'abi_refusals.json')
BAD_ARGUMENT, UNSUPPORTED = 10001, 10002
P = 0x10000            # a placeholder for a device pointer: non-null, never dereferenced (see the module docstring)

CHANNELS = (8, 16, 24, 32, 48, 64, 128, 512, 1024)
SIDES = (4, 8, 16, 24, 32, 33, 64, 128)

# ---- the launching entries.  Every entry: its arguments in order with values that pass every check (such a call is
# never made), the fields of its epilogue(s), and the change of shape that the entry does not support.
EP = dict(style=P, demod=P, noise=P, noise_w=P, bias=P, act=1)
EP_PLAIN = dict(style=P, demod=P, noise=None, noise_w=None, bias=P, act=0)     # rw_conv_transpose3x3s2_f32: no noise / act
RGB = dict(weight=P, style=P, bias=P, skip=P, out=P, scale=0.125)
SHAPE = [('batch', 1), ('in_ch', 32), ('out_ch', 32), ('h', 64), ('w', 64), ('w_scale', 1.0)]
SPLIT = [('u_inv', 1.0), ('x_amax', P)]
TOO_LARGE = dict(in_ch=512, h=1024, w=1024)       # in_ch * h * w * 4 bytes = 2^31: past the 31-bit offsets of a map

ENTRIES = {
    'rw_conv3x3_f32': dict(
        args=[('x', P), ('wp', P), ('y', P)] + SHAPE + [('ep', EP), ('impl', 3), ('stream', None)],
        unsupported=dict(in_ch=8)),
    'rw_conv3x3_to_rgb_f32': dict(
        args=[('x', P), ('wp', P), ('y', P)] + SHAPE + [('ep', EP), ('rgb', RGB), ('stream', None)],
        unsupported=dict(out_ch=16)),
    'rw_conv3x3_wino_f32': dict(
        args=[('x', P), ('uf', P), ('y', P)] + SHAPE + [('ep', EP), ('stream', None)],
        unsupported=dict(w=33)),
    'rw_conv3x3_wino_to_rgb_f32': dict(
        args=[('x', P), ('uf', P), ('y', P)] + SHAPE + [('ep', EP), ('rgb', RGB), ('stream', None)],
        unsupported=dict(w=33)),
    'rw_conv3x3_wino4_f32': dict(
        args=[('x', P), ('uf', P), ('y', P)] + SHAPE + [('ep', EP), ('stream', None)],
        unsupported=dict(w=63)),
    'rw_conv3x3_wino4h_f32': dict(
        args=[('x', P), ('uf', P), ('y', P)] + SHAPE + [('ep', EP)] + SPLIT + [('y_amax', P), ('stream', None)],
        unsupported=dict(w=63)),
    'rw_conv3x3_wino4_to_rgb_f32': dict(
        args=[('x', P), ('uf', P)] + SHAPE + [('ep', EP), ('rgb', RGB), ('stream', None)],
        unsupported=dict(w=63)),
    'rw_conv3x3_wino4h_to_rgb_f32': dict(
        args=[('x', P), ('uf', P)] + SHAPE + [('ep', EP), ('rgb', RGB)] + SPLIT + [('stream', None)],
        unsupported=dict(w=63)),
    'rw_conv_transpose3x3s2_f32': dict(
        args=[('x', P), ('wp', P), ('y', P)] + SHAPE + [('ep', EP_PLAIN), ('impl', 3), ('stream', None)],
        unsupported=dict(in_ch=8)),
    'rw_conv_transpose3x3s2_wino_f32': dict(
        args=[('x', P), ('uf', P), ('y', P)] + SHAPE + [('style', P), ('demod', P), ('stream', None)],
        unsupported=dict(w=33)),
    'rw_conv_transpose3x3s2_winoh_f32': dict(
        args=[('x', P), ('uf', P), ('y', P)] + SHAPE + [('style', P), ('demod', P)] + SPLIT + [('stream', None)],
        unsupported=dict(w=33)),
    'rw_conv_transpose3x3s2_blur_wino4_f32': dict(
        args=[('x', P), ('uf', P), ('y', P)] + SHAPE + [('ep', EP), ('post_scale', P), ('stream', None)],
        unsupported=dict(w=63)),
    'rw_conv_transpose3x3s2_blur_wino4h_f32': dict(
        args=[('x', P), ('uf', P), ('y', P)] + SHAPE + [('ep', EP), ('post_scale', P)] + SPLIT
        + [('y_amax', P), ('stream', None)],
        unsupported=dict(w=63)),
    'rw_dconv3x3_f32': dict(
        args=[('x', P), ('wp', P), ('y', P)] + SHAPE + [('ep', EP)] + SPLIT + [('y_amax', P), ('stream', None)],
        unsupported=dict(w=33), too_large=TOO_LARGE),
    'rw_dconv3x3_rgb_partial_f32': dict(
        args=[('x', P), ('wp', P), ('y', P)] + SHAPE + [('ep', EP), ('rgb', RGB)] + SPLIT
        + [('y_amax', P), ('stream', None)],
        unsupported=dict(w=33), too_large=TOO_LARGE),
    'rw_dconv_transpose3x3s2_blur_f32': dict(
        args=[('x', P), ('wp', P), ('y', P)] + SHAPE + [('ep', EP), ('post_scale', P)] + SPLIT
        + [('y_amax', P), ('stream', None)],
        unsupported=dict(w=33), too_large=TOO_LARGE),
    'rw_dconv3x3_to_rgb_f32': dict(
        args=[('x', P), ('wp', P)] + SHAPE + [('ep', EP), ('rgb', RGB)] + SPLIT + [('stream', None)],
        unsupported=dict(w=33), too_large=TOO_LARGE),
    'rw_tconv_blur_f32': dict(
        args=[('x', P), ('wp', P), ('k4', P), ('y', P)] + SHAPE + [('ep', EP), ('post_scale', P)] + SPLIT
        + [('y_amax', P), ('stream', None)],
        unsupported=dict(w=33), too_large=TOO_LARGE),
}




# ---- the entries that measure (rw_*_absmax_f32) and pack a weight: 32 x 32 channels every form packs, `dst` = the
# packed weight or the bound, and a channel pair the form does not pack
def _pack_entry(unpacked, k4=False, bound=False, u_scale=False):
    args = [('w', P)] + [('k4', P)] * k4 + [('dst', P)] * (not bound) + [('out_ch', 32), ('in_ch', 32)]
    return dict(args=args + [('dst', P)] * bound + [('u_scale', 0.5)] * u_scale + [('stream', None)], unpacked=unpacked)


PACK_ENTRIES = {
    'rw_pack_conv_weight_wino_f32': _pack_entry(dict(out_ch=48)),
    'rw_pack_conv_weight_wino4_f32': _pack_entry(dict(out_ch=24)),
    'rw_conv_weight_wino4h_absmax_f32': _pack_entry(dict(out_ch=24), bound=True),
    'rw_pack_conv_weight_wino4h_f32': _pack_entry(dict(out_ch=24), u_scale=True),
    'rw_pack_conv_transpose_wino_f32': _pack_entry(dict(out_ch=24)),
    'rw_conv_transpose_weight_winoh_absmax_f32': _pack_entry(dict(in_ch=12), bound=True),
    'rw_pack_conv_transpose_winoh_f32': _pack_entry(dict(in_ch=12), u_scale=True),
    'rw_pack_conv_transpose_blur_weight_wino4_f32': _pack_entry(dict(out_ch=6), k4=True),
    'rw_conv_transpose_blur_weight_wino4h_absmax_f32': _pack_entry(dict(out_ch=6), k4=True, bound=True),
    'rw_pack_conv_transpose_blur_weight_wino4h_f32': _pack_entry(dict(out_ch=6), k4=True, u_scale=True),
    'rw_dconv_weight_absmax_f32': _pack_entry(dict(in_ch=24), bound=True),
    'rw_pack_dconv_weight_f32': _pack_entry(dict(in_ch=24), u_scale=True),
    'rw_dconv_transpose_blur_weight_absmax_f32': _pack_entry(dict(in_ch=24), k4=True, bound=True),
    'rw_pack_dconv_transpose_blur_weight_f32': _pack_entry(dict(in_ch=24), k4=True, u_scale=True),
}
ENTRIES.update(PACK_ENTRIES)


def pack_entry_cases(name):
    spec = PACK_ENTRIES[name]
    names = [a for a, _ in spec['args']]
    cases = {'null_w': {'w': None}, 'null_dst': {'dst': None}, 'zero_out_ch': {'out_ch': 0},
             'negative_in_ch': {'in_ch': -32}, 'unpacked_channels': dict(spec['unpacked'])}
    if 'k4' in names:
        cases['null_k4'] = {'k4': None}
    if 'u_scale' in names:
        cases['zero_u_scale'] = {'u_scale': 0.0}
    # two defects at once: a bad argument is reported before channel counts the form does not pack
    last = 'zero_u_scale' if 'u_scale' in names else 'null_dst'
    for first in ('null_w', last):
        cases[first + '+unpacked_channels'] = dict(cases[first], **spec['unpacked'])
    return cases


def entry_cases(name):
    """{case name: {argument (or 'ep.field' / 'rgb.field'): value}} -- the defects of one entry."""
    if name in PACK_ENTRIES:
        return pack_entry_cases(name)
    spec = ENTRIES[name]
    names = [a for a, _ in spec['args']]
    cases = {'null_x': {'x': None}, 'unsupported_shape': dict(spec['unsupported'])}
    if 'ep' in names:
        cases['noise_without_noise_w'] = {'ep.noise': P, 'ep.noise_w': None}
        cases['act_without_bias'] = {'ep.act': 1, 'ep.bias': None}
    if 'x_amax' in names:
        cases['null_x_amax'] = {'x_amax': None}
        cases['zero_u_inv'] = {'u_inv': 0.0}
    if 'rgb' in names:
        cases['null_rgb'] = {'rgb': None}
        cases['null_rgb_out'] = {'rgb.out': None}
    if 'too_large' in spec:
        cases['too_large'] = dict(spec['too_large'])
    # two defects at once pin the order of the checks: a bad argument is reported before an unsupported shape, by the
    # first check of an entry and by its last one
    last = 'act_without_bias' if 'ep' in names else ('null_x_amax' if 'x_amax' in names else None)
    cases['null_x+unsupported_shape'] = dict(cases['null_x'], **spec['unsupported'])
    if last:
        cases[last + '+unsupported_shape'] = dict(cases[last], **spec['unsupported'])
    else:
        cases['null_uf+unsupported_shape'] = dict({'uf': None}, **spec['unsupported'])
    return cases


def call_entry(lib, name, defects):
    values, keep = [], []
    for arg, good in ENTRIES[name]['args']:
        if isinstance(good, dict):
            if arg in defects:                       # the whole struct is missing
                values.append(None)
                continue
            fields = dict(good)
            fields.update({k.split('.')[1]: v for k, v in defects.items() if k.startswith(arg + '.')})
            struct = (_lib.ConvEpilogue if arg == 'ep' else _lib.RgbEpilogue)(**fields)
            keep.append(struct)
            values.append(ctypes.byref(struct))
        else:
            values.append(defects.get(arg, good))
    unknown = [k for k in defects if k.split('.')[0] not in dict(ENTRIES[name]['args'])]
    assert not unknown, (name, unknown)
    return int(getattr(lib, name)(*values))


# ---- the pure functions: name -> the argument tuples of its table, in order
def _shapes(*tails):
    return [s + t for s in itertools.product(CHANNELS, CHANNELS, SIDES, SIDES) for t in (tails or [()])]


SUPPORTED = {n: _shapes() for n in (
    'rw_conv3x3_wino_supported', 'rw_conv3x3_wino4_supported', 'rw_conv3x3_wino4_to_rgb_supported',
    'rw_conv_transpose3x3s2_wino_supported', 'rw_conv_transpose3x3s2_winoh_supported',
    'rw_conv_transpose_blur_wino4_supported', 'rw_dconv3x3_supported', 'rw_dconv3x3_to_rgb_supported',
    'rw_dconv_transpose_blur_supported', 'rw_tconv_blur_supported')}
# (upsample, plain, constrained) / (rank, upsample, linear_insert)
SUPPORTED['rw_solve_supported'] = _shapes((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
SUPPORTED['rw_solve_run_supported'] = _shapes((1, 0, 0), (8, 0, 0), (9, 0, 0), (1, 1, 0), (1, 0, 1))

_PAIRS = list(itertools.product(CHANNELS, CHANNELS))
PACKED = {n: _PAIRS for n in (
    'rw_packed_conv_weight_bf16x3_bytes', 'rw_packed_conv_weight_wino_elems', 'rw_packed_conv_weight_wino4_elems',
    'rw_packed_conv_weight_wino4h_elems', 'rw_packed_conv_transpose_wino_elems', 'rw_packed_conv_transpose_winoh_elems',
    'rw_packed_conv_transpose_blur_wino4_elems', 'rw_packed_conv_transpose_blur_wino4h_elems',
    'rw_packed_dconv_weight_elems', 'rw_packed_dconv_transpose_blur_weight_elems')}
PACKED['rw_packed_conv_weight_elems'] = [p + (mode,) for p in _PAIRS for mode in (0, 1)]


def supported_table(lib, name):
    fn = getattr(lib, name)
    return ''.join(str(int(fn(*a))) for a in SUPPORTED[name])        # every answer is one digit: 0 / 1


def packed_table(lib, name):
    fn = getattr(lib, name)
    return [int(fn(*a)) for a in PACKED[name]]


def _table():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_covers_every_pure_function_of_the_header():
    names = set(_lib.SIGNATURES)
    assert {n for n in names if n.endswith('_supported')} == set(SUPPORTED)
    assert {n for n in names if n.startswith('rw_packed_')} == set(PACKED)
    t = _table()
    assert set(t['supported']) == set(SUPPORTED) and set(t['packed']) == set(PACKED)
    assert set(t['refusals']) == set(ENTRIES)
    for name in ENTRIES:
        assert set(t['refusals'][name]) == set(entry_cases(name)), name


@pytest.mark.parametrize('name', sorted(SUPPORTED))
def test_supported_tables(name):
    got, want = supported_table(_lib.load(), name), _table()['supported'][name]
    assert len(got) == len(want)
    diff = [(a, want[i], got[i]) for i, a in enumerate(SUPPORTED[name]) if got[i] != want[i]]
    assert not diff, '%s: %d answers changed, first (args, recorded, now): %r' % (name, len(diff), diff[:5])


@pytest.mark.parametrize('name', sorted(PACKED))
def test_packed_size_tables(name):
    got, want = packed_table(_lib.load(), name), _table()['packed'][name]
    diff = [(a, w, g) for a, w, g in zip(PACKED[name], want, got) if w != g]
    assert len(got) == len(want) and not diff, '%s: (args, recorded, now) %r' % (name, diff[:5])


def _device_visible():
    import torch
    return torch.cuda.is_available()


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_entries_refuse_as_recorded(name):
    if _device_visible():
        pytest.skip('a HIP device is visible: a regressed refusal would launch on placeholder pointers')
    recorded = _table()['refusals'][name]
    lib = _lib.load()
    for case, defects in entry_cases(name).items():
        want = recorded[case]
        assert want in (BAD_ARGUMENT, UNSUPPORTED), (name, case, want)       # anything else is never called
        got = call_entry(lib, name, defects)
        print('%s %s: %d' % (name, case, got))
        assert got == want, '%s, %s: status %d, recorded %d' % (name, case, got, want)


def record(lib_path):
    lib = ctypes.CDLL(lib_path)
    for n, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, n)
        fn.restype, fn.argtypes = restype, argtypes
    assert not _device_visible(), 'record on a machine without a HIP device'
    table = {'refusals': {}, 'supported': {}, 'packed': {}}
    for name in sorted(ENTRIES):
        table['refusals'][name] = {}
        for case, defects in entry_cases(name).items():
            status = call_entry(lib, name, defects)
            assert status in (BAD_ARGUMENT, UNSUPPORTED), \
                '%s, %s: status %d -- not a refusal, nothing is written' % (name, case, status)
            table['refusals'][name][case] = status
    for name in sorted(SUPPORTED):
        table['supported'][name] = supported_table(lib, name)
        assert set(table['supported'][name]) <= {'0', '1'}, name
    for name in sorted(PACKED):
        table['packed'][name] = packed_table(lib, name)
    with open(TABLE, 'w') as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s' % TABLE)


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--record', __doc__
    record(sys.argv[2])
