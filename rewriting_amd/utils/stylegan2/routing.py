"""Which kernel runs a styled convolution: the RW_* switches, read in ONE place, and one pure decision function per kind
of layer (snapshot of the switches, calling context, shape -> a record; only the ``hip.*_supported`` / ``*_applicable``
helpers are consulted).  models.py dispatches on the record and decides nothing itself: a new route is one branch here
and one row of ``DemodulatedConv2dF.KERNELS`` (the names are STRIDE1_KERNELS / UP_KERNELS below); ``StyledConvSeq`` reads
the records' flags only.  tests/test_routes.py holds every context and switch setting to the launches recorded under
tests/golden/."""
import os
from collections import namedtuple

from ... import hip

_CONV_IMPLS = {'auto': 0, 'mfma': 0, 'direct': 1, 'generic': 2, 'halo': 3, 'nosplitk': 5}
ONE_PASS_UP_MAX_IN = 64         # see upsample_route: the phase kernels pay up to here
FUSED_UP_MAX_IN = 512           # default of RW_UP_FUSED2_MAX_IN

Switches = namedtuple('Switches', [
    'fuse',               # RW_FUSE (off: '0'): an un-hooked StyledConv runs as one fused block, the generator on its streams
    'conv_impl',          # RW_CONV_IMPL auto|mfma|direct|generic|halo|nosplitk: rw_conv3x3_f32's impl (include/rewriting_hip.h);
                          #   auto = halo-tile MFMA kernel from 24 columns up, else im2col MFMA; 'direct' = the VALU cross-check
    'conv_precision',     # RW_CONV_PRECISION f32|bf16x6: bf16x6 (opt-in) = eligible stride-1 layers on the bf16 pipe, exact 3-way splits
    'conv_algo',          # RW_CONV_ALGO direct|winograd|winograd4: one stride-1 algorithm everywhere (unset: see conv_algo)
    'up_algo',            # RW_UP_ALGO winograd|direct|winograd4: the transposed convolutions (F(2,2) phases / direct / phase kernels forced)
    'mm',                 # RW_MM f32|split: one matrix pipe everywhere (unset: see matrix_mode)
    'mm_hooked_split',    # RW_MM_HOOKED (off: 'f32'): hooked / sliced models run their F(2,2) transposed convolutions in the split form
    'mm_parts',           # RW_MM_PARTS w4,up,up1 (diagnostics): restricts the split form to these kinds of kernel
    'mm_direct16',        # RW_MM_DIRECT16 auto|1|0|kinds: which of conv,up,rgb run as direct sums inside the split form (see _direct16)
    'micro_batch',        # RW_MICRO_BATCH "k" or "k:res": (images per slice, first resolution run in slices); 0 = whole batch
    'up_fused',           # RW_UP_FUSED (off: '0'): the one-pass phase kernels for upsampling layers
    'up_fused2',          # RW_UP_FUSED2 (on: '1' only): the fused transposed-conv + blur kernel (csrc/rw_tconv.hip)
    'up_fused2_hooked',   # RW_UP_FUSED2_HOOKED (on: '1' only): ... in hooked / sliced models too
    'up_fused2_max_in',   # RW_UP_FUSED2_MAX_IN: ... up to this many input channels
    'up_fused2_join',     # RW_UP_FUSED2_JOIN (on: '1'): the trunk waits for the RGB stream in front of the fused kernel (diagnostics)
    'direct16_small',     # RW_DIRECT16_SMALL (off: '0'): the 32^2 stride-1 layer of the un-hooked forward as a direct sum
    'direct16_hooked',    # RW_DIRECT16_HOOKED (on: '1' only): stride-1 layers from 32^2 up of hooked / sliced models as direct sums
    'dconv_ws_fwd',       # RW_DCONV_WS_FWD (off: '0'): the twelve-wave specialised direct sum takes its style on load (no pre-scaled map)
    'dconv_v',            # RW_DCONV_V (on: '1'): the one-role direct-sum kernels are forced (csrc/rw_dconv.hip): none is specialised
    'rgb_partial',        # RW_RGB_PARTIAL (off: '0'): the direct sums leave the channel sums of the ToRGB that reads them
    'rgb_f4',             # RW_RGB_F4 (off: '0'): the last layer + ToRGB on F(4x4,3x3)
    'rgb_stream',         # RW_RGB_STREAM (off: '0'): the RGB branch of the un-hooked forward on a second stream
    'strip_stream',       # RW_STRIP_STREAM (off: '0'): the border strips of a sliced / hooked model on the device's auxiliary stream
    'side_priority',      # RW_SIDE_PRIORITY: torch priority of the side streams (positive = below the trunk's)
    'prescale',           # RW_PRESCALE (off: '0'): an upsampling layer multiplies the next layer's style into its result
    'mm_no_handover',     # RW_MM_NO_HANDOVER (on: '1'): every split kernel measures its input, no bound is handed over (diagnostics)
    'prefetch_styles',    # RW_PREFETCH_STYLES (off: '0'): styles and demodulation factors computed up front on the auxiliary stream
    'fuse_final_rgb',     # RW_FUSE_FINAL_RGB (off: '0'): ToRGB in the epilogue of the last styled convolution
    'rgb_inline_up',      # RW_RGB_INLINE_UP (off: '0'): rgb_combine and the final F(4x4) ToRGB upsample the running image themselves
])


def switches():
    """The RW_* environment as it is NOW (tests and bench.py flip the variables inside one process)."""
    env = os.environ.get
    direct16 = env('RW_MM_DIRECT16', 'auto')
    parts = env('RW_MM_PARTS')
    k, _, res = env('RW_MICRO_BATCH', '0').partition(':')
    return Switches(
        fuse=env('RW_FUSE', '1') != '0',
        conv_impl=_CONV_IMPLS[env('RW_CONV_IMPL', 'auto')],
        conv_precision=env('RW_CONV_PRECISION', 'f32'),
        conv_algo=env('RW_CONV_ALGO'),
        up_algo=env('RW_UP_ALGO', 'winograd'),
        mm=env('RW_MM'),
        mm_hooked_split=env('RW_MM_HOOKED', 'split') != 'f32',
        mm_parts=None if parts is None else tuple(parts.split(',')),
        mm_direct16={'auto': ('conv', 'up'), '1': ('conv', 'up', 'rgb')}.get(direct16) or tuple(direct16.split(',')),
        micro_batch=(int(k or 0), int(res or 256)),
        up_fused=env('RW_UP_FUSED', '1') != '0',
        up_fused2=env('RW_UP_FUSED2', '1') == '1',
        up_fused2_hooked=env('RW_UP_FUSED2_HOOKED', '1') == '1',
        up_fused2_max_in=int(env('RW_UP_FUSED2_MAX_IN', FUSED_UP_MAX_IN)),
        up_fused2_join=env('RW_UP_FUSED2_JOIN') == '1',
        direct16_small=env('RW_DIRECT16_SMALL', '1') != '0',
        direct16_hooked=env('RW_DIRECT16_HOOKED', '1') == '1',
        dconv_ws_fwd=env('RW_DCONV_WS_FWD', '1') != '0',
        dconv_v=env('RW_DCONV_V') == '1',
        rgb_partial=env('RW_RGB_PARTIAL', '1') != '0',
        rgb_f4=env('RW_RGB_F4', '1') != '0',
        rgb_stream=env('RW_RGB_STREAM', '1') != '0',
        strip_stream=env('RW_STRIP_STREAM', '1') != '0',
        side_priority=int(env('RW_SIDE_PRIORITY', '0')),
        prescale=env('RW_PRESCALE', '1') != '0',
        mm_no_handover=env('RW_MM_NO_HANDOVER') == '1',
        prefetch_styles=env('RW_PREFETCH_STYLES', '1') != '0',
        fuse_final_rgb=env('RW_FUSE_FINAL_RGB', '1') != '0',
        rgb_inline_up=env('RW_RGB_INLINE_UP', '1') != '0',
    )


# How the layer is being run.  image_path: inside the un-hooked forward of a whole generator (image generation) -- every
# other way is a hooked model, a nethook.subsequence slice (key statistics, goal maps, the solve's context and its
# rendering) or RW_FUSE=0; capturing: the stream is being captured into a graph; rgb_stream / aux_stream: the running
# forward has its RGB / auxiliary side stream; weight_changes: the caller differentiates with respect to the weight.
Context = namedtuple('Context', 'image_path on_device capturing rgb_stream aux_stream weight_changes')

STRIDE1_KERNELS = ('direct16', 'wino4_split', 'wino4', 'wino', 'bf16x6', 'gemm')
# these run the layer's blur, noise and activation too; the other upsampling kernels leave the (2H+1) x (2W+1) map
WHOLE_LAYER_KERNELS = ('fused', 'one_pass_direct16', 'one_pass_wino4')
UP_KERNELS = WHOLE_LAYER_KERNELS + ('f22_strips', 'halo_strips', 'plain')

# kernel: one of STRIDE1_KERNELS; specialised: the twelve-wave direct sum that needs its style on load; rgb_partials: it
# also leaves the ToRGB channel sums; reads_bound / reports_bound: it takes a bound of |input| (measuring the map itself
# without one) / writes the bound of its result; prescaled: the layer in front may hand it a map already multiplied by
# its style.
Stride1Route = namedtuple('Stride1Route', 'kernel specialised rgb_partials reads_bound reports_bound prescaled')

# kernel: one of UP_KERNELS; split: the F(2,2) / phase kernel runs in the split form; side_strips: the border strips go
# to the auxiliary stream beside the tiles; reads_bound: ADVICE to the layer in front, inside the un-hooked forward, to
# leave a bound on its result (see there); runs_layer: the kernel is one of WHOLE_LAYER_KERNELS.
UpRoute = namedtuple('UpRoute', 'kernel split side_strips reads_bound runs_layer')

# kernel: one of STRIDE1_KERNELS, in its form with ToRGB in the epilogue; reads_bound: as Stride1Route's.  Nothing reads
# the result but ToRGB, so none of them reports a bound.
FinalRgbRoute = namedtuple('FinalRgbRoute', 'kernel reads_bound')


def _stride1(kernel, *flags):
    if kernel not in STRIDE1_KERNELS:
        raise ValueError(kernel)
    return Stride1Route(kernel, *flags)


def _up(kernel, *flags):
    if kernel not in UP_KERNELS:
        raise ValueError(kernel)
    return UpRoute(kernel, *flags, kernel in WHOLE_LAYER_KERNELS)


def _final_rgb(kernel, reads_bound):
    if kernel not in STRIDE1_KERNELS:
        raise ValueError(kernel)
    return FinalRgbRoute(kernel, reads_bound)


def conv_algo(sw, image_path):
    """Algorithm of the stride-1 3x3 convolutions where more than one exists.

    Without RW_CONV_ALGO the answer depends on HOW the modules are being run:
      * image_path: 'winograd4' = F(4x4,3x3) where hip.wino4_supported says so -- 4x fewer matrix FLOPs at ~1e-5
        relative error per layer, 3e-5 measured on the 1024^2 image against the reference (the path's image tolerance
        is 1e-3) -- and F(2x2,3x3) elsewhere;
      * every other way: 'winograd' = F(2x2,3x3) (hip.conv3x3_wino: 2.25x fewer matrix FLOPs, the fp32 error class of
        the direct sum) -- which runs BELOW 32^2 only: from 32^2 up these models' stride-1 layers are direct sums on the
        16-bit pipe (stride1_route, the hooked branch) and their upsampling layers the fused split kernel
        (upsample_route); the statistics goldens hold at 4e-6 - 5e-6 from the reference's.
    Consequence: model(z) and the same weights run through rewriter.sample_image_from_latent differ by 1e-5 .. 1e-4
    on the image.  RW_CONV_ALGO=direct|winograd|winograd4 forces one algorithm everywhere; shapes an algorithm does
    not take always run the next one down ('direct' = the implicit GEMM takes everything)."""
    return sw.conv_algo or ('winograd4' if image_path else 'winograd')


def matrix_mode(sw, image_path, kind=None):
    """Which matrix pipe multiplies inside the F(4x4,3x3) and F(2,2) kernels: 'f32' (fp32 MFMAs) or 'split' -- every
    transformed operand as an exact pair of f16 numbers, the piece products on the 16-bit pipe, fp32 accumulation
    (hip.pack_conv_weight_wino4(split=True) ...: per-product error <= 2^-21, the kernels pass their parity tests at
    the fp32 bars).  image_path: 'split' for every kind of kernel.  Hooked / sliced models run only their F(2,2)
    transposed convolutions (kind 'up') in the split form, which holds the DIRECT kernels' bars
    (test_transposed_conv_f22_...: 3e-6 relative) and is 1.4 - 1.5 x faster on the 64^2 ... 512^2 maps of a layer-10 /
    layer-14 sweep; RW_MM_HOOKED=f32 keeps them on fp32.  RW_MM=f32|split forces one everywhere."""
    if sw.mm:
        return sw.mm
    if image_path:
        return 'split'
    return 'split' if kind == 'up' and sw.mm_hooked_split else 'f32'


def _split_part(sw, image_path, kind):
    return matrix_mode(sw, image_path, kind) == 'split' and (sw.mm_parts is None or kind in sw.mm_parts)


def _plain(sw):
    """The default implicit-GEMM family in exact fp32: every specialised route asks for it."""
    return sw.conv_impl == 0 and sw.conv_precision == 'f32'


def _direct16(sw, kind, in_ch, out_ch, h, w):
    """Inside the split form: the DIRECT sums on the 16-bit matrix pipe (csrc/rw_dconv.hip) in place of the
    split-operand F(4x4,3x3) kernels, kind 'conv' / 'up' / 'rgb'.  RW_MM_DIRECT16 'auto' = 'conv,up', the two that
    measure faster INSIDE the forward of the 1024 generator (same box, batch 64, profiles/r05c_ab.jsonl: 1262 against
    1221 img/s; per launch the stride-1 layers 3.4 / 4.3 ms against 3.7 - 4.7, the one-pass upsampling layer 10.2
    against 10.4; the last layer + ToRGB is slower as a direct sum: 7.0 against 5.8).  (Round 4 left them opt-in
    because sequences of un-synced forwards were occasionally wrong with them -- the device scalars of that round's
    bound hand-over; tests/test_gpu_zz_sequences.py holds both selections to bit-identical sequences now.)"""
    if in_ch < 32 or kind not in sw.mm_direct16:
        return False
    if kind == 'up':
        return hip.dconv_transpose_blur_supported(out_ch, in_ch, h, w)
    if kind == 'rgb':
        return hip.dconv_to_rgb_supported(out_ch, in_ch, h, w)
    return hip.dconv_supported(out_ch, in_ch, h, w)


def stride1_route(sw, ctx, in_ch, out_ch, h, w):
    """The stride-1 3x3 convolution of a map of h x w.  Branches in order of precedence."""
    algo = conv_algo(sw, ctx.image_path)
    plain = _plain(sw)
    split = _split_part(sw, ctx.image_path, 'w4')
    if algo == 'winograd4' and plain and hip.wino4_supported(out_ch, in_ch, h, w):
        if split and _direct16(sw, 'conv', in_ch, out_ch, h, w):
            # rw_dconv.hip's dconv_ws_w2 kernels: one persistent twelve-wave workgroup per CU, 64 out-channels and 64
            # columns per tile; their staging waves apply the style themselves, so nobody pre-scales for them
            specialised = (ctx.image_path and sw.dconv_ws_fwd and not sw.dconv_v
                           and out_ch % 64 == 0 and h % 8 == 0 and w % 64 == 0)
            # the RGB stream then adds a few small images instead of re-reading the feature map (4.3 GB for layer 16 at
            # batch 64); without them ToRGB re-reads the map on the RGB stream
            partials = ctx.image_path and ctx.rgb_stream and sw.rgb_partial and out_ch % 32 == 0
            return _stride1('direct16', specialised, partials, True, True, sw.prescale and not specialised)
        return _stride1('wino4_split' if split else 'wino4', False, False, split, split, sw.prescale)
    if (ctx.image_path and split and sw.direct16_small and algo == 'winograd4' and plain and min(h, w) >= 32
            and _direct16(sw, 'conv', in_ch, out_ch, h, w)):
        # the 32^2 layer, too narrow for F(4x4,3x3): 0.8 against 1.4 ms on the fp32 F(2x2,3x3) kernel at batch 64, the
        # forward +1.7 % (same box, interleaved: profiles/r06aq).  The layer in front runs an fp32 kernel, so its blur
        # pass reports the bound
        return _stride1('direct16', False, False, True, True, False)
    if (not ctx.image_path and not ctx.weight_changes and not ctx.capturing and sw.direct16_hooked
            and sw.conv_algo is None and matrix_mode(sw, False, 'up') == 'split' and plain
            and _direct16(sw, 'conv', in_ch, out_ch, h, w)):
        # hooked / sliced models (statistics sweeps, goal maps, the solve's context): exact f16 operand pairs, fp32
        # accumulation, 4e-7 from the fp32 direct sum -- the error class these models are held to -- where their F(2,2)
        # transposed convolutions run in the split form too.  It measures its input itself: nobody hands a bound over
        # outside the un-hooked forward.  Not where the weight is being optimised (every re-packing reads the weights'
        # maximum back to the host, hip._split_scale: two launches and a sync per layer and iteration) and not while
        # the stream is captured (the read-back would fail)
        return _stride1('direct16', False, False, True, False, False)
    if algo in ('winograd', 'winograd4') and plain and hip.wino_supported(out_ch, in_ch, h, w):
        return _stride1('wino', False, False, False, False, False)
    if sw.conv_precision == 'bf16x6' and sw.conv_impl == 0 and hip.bf16x6_supported(out_ch, in_ch, w):
        return _stride1('bf16x6', False, False, False, False, False)
    return _stride1('gemm', False, False, False, False, False)


def upsample_route(sw, ctx, in_ch, out_ch, h, w, whole_layer):
    """The stride-2 transposed convolution of a map of h x w.  whole_layer: the caller runs the layer's blur ([1,3,3,1],
    pad (1, 1)), noise and activation too, so the kernels that do all of it in one pass are candidates."""
    plain = _plain(sw)
    one_pass = whole_layer and plain and sw.up_algo != 'direct'
    advice = plain and matrix_mode(sw, ctx.image_path) == 'split'
    # 1. hip.conv_transpose3x3s2_blur_fused (csrc/rw_tconv.hip): one pass at the transposed convolution's OWN multiply
    # count, the (2H+1)^2 map kept in LDS -- wherever the split form applies (w % 32 == 0, h % 16 == 0: 32^2 maps up),
    # in hooked / sliced models too (+13 - 16 % on the layer-10 / layer-14 sweeps).  Its first forms were +1.6 % and
    # stayed opt-in in round 5 because to_rgb_kernel on the second stream came back wrong beside them (its packed fp32
    # FMAs; the streaming kernels are compiled without packed fp32 math since: csrc/rw_ops.hip, first line; DESIGN.md
    # section 4.5); the persistent and one-workgroup-per-CU forms are +7 % (profiles/r05r)
    if (one_pass and sw.up_fused2 and in_ch <= sw.up_fused2_max_in
            and (_split_part(sw, True, 'up1') if ctx.image_path else _split_part(sw, False, 'up') and sw.up_fused2_hooked)
            and hip.tconv_blur_supported(out_ch, in_ch, h, w)):
        return _up('fused', True, False, advice)
    split = _split_part(sw, ctx.image_path, 'up')
    f22 = (sw.up_algo == 'winograd' and sw.conv_impl == 0 and hip.up_strips_applicable(out_ch, in_ch)
           and hip.conv_transpose_wino_supported(out_ch, in_ch, h, w))
    f22_split = f22 and split and hip.conv_transpose_wino_split_supported(out_ch, in_ch, h, w)
    # 2. the four output-parity phases as virtual channels of the F(4x4,3x3) / direct-sum kernel: 1.44x the matrix work
    # of F(2,2), but the (2H+1)^2 map and the blur pass are never written or read -- pays at <= 64 input channels
    # (layer 17 of the 1024 model: 12.4 -> 9.x ms) where F(4x4,3x3) runs at all; RW_UP_ALGO=winograd4 forces it
    if (one_pass and sw.up_fused and hip.conv_transpose_blur_wino4_supported(out_ch, in_ch, h, w)
            and (sw.up_algo == 'winograd4' or conv_algo(sw, ctx.image_path) == 'winograd4' and in_ch <= ONE_PASS_UP_MAX_IN)):
        split1 = _split_part(sw, ctx.image_path, 'up1')
        if split1 and _direct16(sw, 'up', in_ch, out_ch, h, w):
            return _up('one_pass_direct16', True, False, advice)
        # reads_bound stays the approximate predicate it was: with RW_MM_PARTS=up (not up1) the fp32 phase kernel
        # runs and ignores the bound that this advice makes the layer in front leave (one reduction launch)
        return _up('one_pass_wino4', split1, False, advice and (split1 or f22_split))
    # 3. two passes: quad tiles -- F(2,2) on the four phases (25 instead of 36 multiplies per 2x2 block of quads) or
    # the direct halo kernel -- beside the border row / column strips, then the blur pass
    side = ctx.aux_stream or (ctx.on_device and sw.strip_stream and not ctx.capturing)
    if f22:
        # reads_bound, approximate again: under RW_CONV_PRECISION=bf16x6 the split F(2,2) kernel runs and measures
        # its input itself (hip.absmax), because the advice is given in plain fp32 mode only
        return _up('f22_strips', f22_split, side, advice and f22_split)
    if sw.conv_impl == 0 and side and hip.up_halo_applicable(out_ch, in_ch, w):
        return _up('halo_strips', False, True, False)
    return _up('plain', False, False, False)


def final_rgb_route(sw, ctx, in_ch, out_ch, h, w):
    """The last styled convolution of the un-hooked generator with ToRGB in its epilogue: a FinalRgbRoute, or None."""
    if not (_plain(sw) and hip.to_rgb_fusable(out_ch, in_ch, w)):
        return None
    algo = conv_algo(sw, ctx.image_path)
    if algo == 'winograd4' and sw.rgb_f4 and hip.wino4_to_rgb_supported(out_ch, in_ch, h, w):
        if not _split_part(sw, ctx.image_path, 'w4'):
            return _final_rgb('wino4', False)
        return _final_rgb('direct16' if _direct16(sw, 'rgb', in_ch, out_ch, h, w) else 'wino4_split', True)
    if algo in ('winograd', 'winograd4') and out_ch == 32 and hip.wino_supported(out_ch, in_ch, h, w):
        return _final_rgb('wino', False)
    return _final_rgb('gemm', False)
