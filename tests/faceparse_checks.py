"""What the face-parsing tests share: a torch.nn twin of the BiSeNet layout (written out here layer by layer, not derived from
rewriting_amd.faceparse's table, so that a wrong table fails against it), its random weights, the label rule, and plain torch
stand-ins for the wrappers the module's walk calls, so that the walk runs on the CPU.

The label rule.  Arg-max is discontinuous, so labels are compared outside the pixels float32 cannot decide: with
tau = MARGIN * max |float32 twin - float64 twin| over the up-sampled scores of one input, a pixel is undecided when the float64
twin's two largest scores there differ by less than tau.  Labels must equal the float64 twin's at every other pixel; scores
must lie within tau of the float64 twin's."""
import copy

import torch
import torch.nn.functional as F
from torch import nn

MARGIN = 8                  # d_hip <= MARGIN * d_ref, DESIGN section 8.1
MAX_UNDECIDED = 0.01        # of a case's pixels
MIN_LABELS = 4              # distinct labels in a case


def rel(a, b):
    """|a - b| / |b| in float64."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


def nearest_index(n_in, n_out):
    """int64 (n_out,): what F.interpolate (nearest) of a float32 tensor reads -- taken from F.interpolate itself on a ramp.
    The float64 twin goes through this table too: F.interpolate of a float64 tensor rounds some pairs differently."""
    ramp = torch.arange(n_in, dtype=torch.float32)[None, None]
    return F.interpolate(ramp, size=n_out)[0, 0].long()


def nearest(x, size):
    return x[:, :, nearest_index(x.shape[2], size[0])][:, :, :, nearest_index(x.shape[3], size[1])]


class ConvBNReLU(nn.Module):
    def __init__(self, i, o, ks=3, stride=1, padding=1):
        super().__init__()
        self.conv = nn.Conv2d(i, o, ks, stride, padding, bias=False)
        self.bn = nn.BatchNorm2d(o)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class BasicBlock(nn.Module):
    def __init__(self, i, o, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(i, o, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(o)
        self.conv2 = nn.Conv2d(o, o, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(o)
        self.downsample = None
        if i != o or stride != 1:
            self.downsample = nn.Sequential(nn.Conv2d(i, o, 1, stride, bias=False), nn.BatchNorm2d(o))

    def forward(self, x):
        r = self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x)))))
        return F.relu((x if self.downsample is None else self.downsample(x)) + r)


class Resnet18(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.layer1 = nn.Sequential(BasicBlock(64, 64), BasicBlock(64, 64))
        self.layer2 = nn.Sequential(BasicBlock(64, 128, 2), BasicBlock(128, 128))
        self.layer3 = nn.Sequential(BasicBlock(128, 256, 2), BasicBlock(256, 256))
        self.layer4 = nn.Sequential(BasicBlock(256, 512, 2), BasicBlock(512, 512))

    def forward(self, x):
        x = self.layer1(F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1))
        feat8 = self.layer2(x)
        feat16 = self.layer3(feat8)
        return feat8, feat16, self.layer4(feat16)


class AttentionRefinement(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.conv = ConvBNReLU(i, o)
        self.conv_atten = nn.Conv2d(o, o, 1, bias=False)
        self.bn_atten = nn.BatchNorm2d(o)

    def forward(self, x):
        feat = self.conv(x)
        return feat * torch.sigmoid(self.bn_atten(self.conv_atten(feat.mean((2, 3), keepdim=True))))


class ContextPath(nn.Module):
    def __init__(self):
        super().__init__()
        self.resnet = Resnet18()
        self.arm16 = AttentionRefinement(256, 128)
        self.arm32 = AttentionRefinement(512, 128)
        self.conv_head32 = ConvBNReLU(128, 128)
        self.conv_head16 = ConvBNReLU(128, 128)
        self.conv_avg = ConvBNReLU(512, 128, 1, 1, 0)

    def forward(self, x):
        feat8, feat16, feat32 = self.resnet(x)
        avg = self.conv_avg(feat32.mean((2, 3), keepdim=True))
        up32 = self.conv_head32(nearest(self.arm32(feat32) + avg, feat16.shape[2:]))
        up16 = self.conv_head16(nearest(self.arm16(feat16) + up32, feat8.shape[2:]))
        return feat8, up16, up32


class FeatureFusion(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.convblk = ConvBNReLU(i, o, 1, 1, 0)
        self.conv1 = nn.Conv2d(o, o // 4, 1, bias=False)
        self.conv2 = nn.Conv2d(o // 4, o, 1, bias=False)

    def forward(self, fsp, fcp):
        feat = self.convblk(torch.cat([fsp, fcp], 1))
        atten = torch.sigmoid(self.conv2(F.relu(self.conv1(feat.mean((2, 3), keepdim=True)))))
        return feat * atten + feat


class Output(nn.Module):
    def __init__(self, i, mid, n):
        super().__init__()
        self.conv = ConvBNReLU(i, mid)
        self.conv_out = nn.Conv2d(mid, n, 1, bias=False)

    def forward(self, x):
        return self.conv_out(self.conv(x))


class Twin(nn.Module):
    """float (B, 3, H, W) -> the (B, n, H, W) class scores of the first head; state_dict() carries the key names of the
    face-parsing checkpoint, the two auxiliary heads (which the segmenter never runs) included."""

    def __init__(self, n_classes=19):
        super().__init__()
        self.cp = ContextPath()
        self.ffm = FeatureFusion(256, 256)
        self.conv_out = Output(256, 256, n_classes)
        self.conv_out16 = Output(128, 64, n_classes)
        self.conv_out32 = Output(128, 64, n_classes)

    def forward(self, x):
        feat8, cp8, _ = self.cp(x)
        return F.interpolate(self.conv_out(self.ffm(feat8, cp8)), x.shape[2:], mode='bilinear', align_corners=True)


def random_twin(seed=0, n_classes=19):
    """The twin in eval mode with kaiming-normal weights and batch-norm statistics gamma ~ U(0.5, 1.5), beta ~ N(0, 0.1),
    mean ~ N(0, 0.1), var ~ U(0.5, 1.5) from `seed`; frozen."""
    gen = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):     # the layers' default initialisation draws from the global generator: tests that
        net = Twin(n_classes)                   # run after this one find it where they would have without it
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, nonlinearity='relu', generator=gen)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
                m.running_var.copy_(torch.rand(m.bias.shape, generator=gen) + 0.5)
    return net.eval().requires_grad_(False)


_cache = {}


def shared_twin():
    """(twin float32, its state dict, twin float64): made once per process and left unchanged."""
    if 'twin' not in _cache:
        net = random_twin(0)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        _cache['twin'] = (net, sd, copy.deepcopy(net).double())
    return _cache['twin']


def images(shape, seed):
    """float32 images in [-1, 1]."""
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=gen) * 2 - 1


# ---- the label rule -------------------------------------------------------------------------------------------------------

class Reference:
    """What a case is compared against: the float64 twin's scores and labels, the float32 twin's scores, tau and the mask of
    the undecided pixels -- all at the size the scores are formed at."""

    def __init__(self, x):
        twin32, _, twin64 = shared_twin()
        with torch.no_grad():
            self.scores32, self.scores64 = twin32(x), twin64(x.double())
        self.d_ref = rel(self.scores32, self.scores64)
        self.tau = MARGIN * (self.scores32.double() - self.scores64).abs().max().item()
        top = self.scores64.topk(2, dim=1).values
        self.undecided = (top[:, :1] - top[:, 1:]) < self.tau              # (B, 1, H, W)
        self.labels = self.scores64.argmax(1, keepdim=True)

    def resized(self, size):
        """(labels, undecided) read through the nearest-neighbour resize of the label map to `size`"""
        return nearest(self.labels, size), nearest(self.undecided, size)

    def is_decisive(self):
        """the two conditions under which the label rule says anything: few undecided pixels, several labels"""
        return self.undecided.double().mean().item() <= MAX_UNDECIDED and self.labels.unique().numel() >= MIN_LABELS


_references = {}


def reference(shape, seed, size=None):
    """The Reference of images(shape, seed), resized (nearest, through the float32 index table) to `size` first where one is
    given; computed once per process."""
    key = (tuple(shape), seed, size)
    if key not in _references:
        x = images(shape, seed)
        _references[key] = Reference(x if size is None else nearest(x, size))
    return _references[key]


def assert_labels(got, want, undecided):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == torch.int64
    wrong = (got != want) & ~undecided
    assert not wrong.any(), '%d decided pixels differ, first at %s' % (int(wrong.sum()), wrong.nonzero()[0].tolist())


# ---- CPU stand-ins for the wrappers the walk calls -------------------------------------------------------------------------

def _gather(x, rows, cols):
    if rows is not None:
        x = x[:, :, rows.long()]
    if cols is not None:
        x = x[:, :, :, cols.long()]
    return x


def conv2d_pack_weight(weight):
    return weight.detach()


def conv2d(x, wp, weight_shape, bias=None, stride=1, padding=0, relu=False, out=None, c_off=0):
    assert tuple(wp.shape) == tuple(weight_shape)
    y = F.conv2d(x, wp, bias, stride, padding)
    y = F.relu(y) if relu else y
    if out is None:
        return y
    out[:, c_off:c_off + y.shape[1]] = y
    return out


def conv2d_add(x, wp, weight_shape, bias, res, stride=1, padding=0, relu=False, out=None):
    y = F.conv2d(x, wp, bias, stride, padding) + res
    y = F.relu(y) if relu else y
    if out is None:
        return y
    out.copy_(y)
    return out


def maxpool3x3s2p1(x):
    return F.max_pool2d(x, 3, 2, 1)


def global_avgpool(x):
    return x.mean((2, 3))


def gate_resample(x, gate=None, add_map=None, add_vec=None, rows=None, cols=None):
    b, c = x.shape[:2]
    y = _gather(x, rows, cols)
    if gate is not None:
        y = y * torch.sigmoid(gate.reshape(b, c, 1, 1))
    if add_map is not None:
        y = y + _gather(add_map, rows, cols)
    if add_vec is not None:
        y = y + add_vec.reshape(b, c, 1, 1)
    return y


def bilinear_ac(x, size, idx, lam):
    oh, ow = size
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (2 * oh + 2 * ow,) and tuple(lam.shape) == (oh + ow,)
    y0, y1, x0, x1 = (t.long() for t in idx.split([oh, oh, ow, ow]))
    lr, lc = lam[:oh].reshape(1, 1, oh, 1), lam[oh:].reshape(1, 1, 1, ow)
    top, bottom = x[:, :, y0], x[:, :, y1]
    return (1 - lr) * ((1 - lc) * top[:, :, :, x0] + lc * top[:, :, :, x1]) + \
        lr * ((1 - lc) * bottom[:, :, :, x0] + lc * bottom[:, :, :, x1])


def seg_labels(logits, size, idx, lam, pick_rows=None, pick_cols=None):
    return _gather(bilinear_ac(logits, size, idx, lam).argmax(1, keepdim=True), pick_rows, pick_cols)


def correct_counts(before, after, src, tgt, srcc=0, tgtc=0):
    """(B, 2) int64 by the formula of the metric, image by image: masks summed over the label sets, then counted"""
    before = before[:, srcc] if before.dim() == 4 else before
    after = after[:, tgtc] if after.dim() == 4 else after
    rows = []
    for b_map, a_map in zip(before, after):
        b_mask = sum((b_map == s).long() for s in src)
        mapped = a_map[b_mask > 0]
        a_mask = sum((mapped == t).long() for t in tgt)
        rows.append([int((a_mask > 0).sum()), int(mapped.shape[0])])
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)


def emulate(monkeypatch):
    """the six wrappers of the face-parsing entries and the four the walk shares with the Inception extractor, replaced by the
    stand-ins above: rewriting_amd.faceparse then runs on CPU tensors"""
    from rewriting_amd import hip
    for name, fn in (('conv2d_pack_weight', conv2d_pack_weight), ('conv2d', conv2d), ('conv2d_add', conv2d_add),
                     ('maxpool3x3s2p1', maxpool3x3s2p1), ('global_avgpool', global_avgpool), ('gate_resample', gate_resample),
                     ('bilinear_ac', bilinear_ac), ('seg_labels', seg_labels), ('seg_correct_counts', correct_counts),
                     ('on_device', lambda t: True)):
        monkeypatch.setattr(hip, name, fn)
