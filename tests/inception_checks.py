"""What the Inception tests share: a torch.nn twin of the FID Inception-v3 layout (written out here layer by layer, not
derived from rewriting_amd.inception's tables, so that a wrong table fails against it), its random weights, and the
figures the accuracy bars are made of."""
import torch
import torch.nn.functional as F
from torch import nn

MARGIN = 8                  # d_hip <= MARGIN * d_ref, DESIGN section 8.1


def rel(a, b):
    """|a - b| / |b| in float64."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


class BasicConv2d(nn.Module):
    def __init__(self, i, o, **kw):
        super().__init__()
        self.conv = nn.Conv2d(i, o, bias=False, **kw)
        self.bn = nn.BatchNorm2d(o, eps=1e-3)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _avg(x):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


class A(nn.Module):
    def __init__(self, i, pf):
        super().__init__()
        self.branch1x1 = BasicConv2d(i, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(i, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(i, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(i, pf, kernel_size=1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          self.branch_pool(_avg(x))], 1)


class B(nn.Module):
    def __init__(self, i):
        super().__init__()
        self.branch3x3 = BasicConv2d(i, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(i, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          F.max_pool2d(x, 3, 2)], 1)


class C(nn.Module):
    def __init__(self, i, c):
        super().__init__()
        self.branch1x1 = BasicConv2d(i, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(i, c, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c, c, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(i, c, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c, c, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c, c, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c, c, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(i, 192, kernel_size=1)

    def forward(self, x):
        d = self.branch7x7dbl_1(x)
        for m in (self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5):
            d = m(d)
        return torch.cat([self.branch1x1(x), self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x))), d,
                          self.branch_pool(_avg(x))], 1)


class D(nn.Module):
    def __init__(self, i):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(i, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(i, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        d = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), d, F.max_pool2d(x, 3, 2)], 1)


class E(nn.Module):
    def __init__(self, i, pool):
        super().__init__()
        self.pool = pool
        self.branch1x1 = BasicConv2d(i, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(i, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(i, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(i, 192, kernel_size=1)

    def forward(self, x):
        t = self.branch3x3_1(x)
        d = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        pooled = _avg(x) if self.pool == 'avg' else F.max_pool2d(x, 3, 1, 1)
        return torch.cat([self.branch1x1(x), self.branch3x3_2a(t), self.branch3x3_2b(t), self.branch3x3dbl_3a(d),
                          self.branch3x3dbl_3b(d), self.branch_pool(pooled)], 1)


class Twin(nn.Module):
    """float (B, 3, H, W) as the network sees it -> (B, 2048); state_dict() carries torchvision's Inception3 key names."""

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b, self.Mixed_5c, self.Mixed_5d = A(192, 32), A(256, 64), A(288, 64)
        self.Mixed_6a = B(288)
        self.Mixed_6b, self.Mixed_6c, self.Mixed_6d, self.Mixed_6e = C(768, 128), C(768, 160), C(768, 160), C(768, 192)
        self.Mixed_7a = D(768)
        self.Mixed_7b, self.Mixed_7c = E(1280, 'avg'), E(2048, 'max')

    def forward(self, x):
        x = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x)))
        x = F.max_pool2d(x, 3, 2)
        x = self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x))
        x = F.max_pool2d(x, 3, 2)
        for name in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e',
                     'Mixed_7a', 'Mixed_7b', 'Mixed_7c'):
            x = getattr(self, name)(x)
        return x.mean((2, 3))


def random_twin(seed=0):
    """The twin in eval mode with kaiming-normal weights and batch-norm statistics gamma ~ U(0.5, 1.5), beta ~ N(0, 0.1),
    mean ~ N(0, 0.1), var ~ U(0.5, 1.5) from `seed`; frozen."""
    gen = torch.Generator().manual_seed(seed)
    net = Twin()
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
        import copy
        _cache['twin'] = (net, sd, copy.deepcopy(net).double())
    return _cache['twin']


def images(shape, seed):
    """float32 images in [-1, 1]."""
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=gen) * 2 - 1
