"""References for the ResNet tests (a helper module, not a test file and not a conftest).

1. A plain torch.nn replica of the reference's models/resnet.py (torchvision is not importable in the test environment): the same
   classes, constructor arguments, module names, construction order and initialisation, with torch's own forward.  Sanity
   check of the replica (tests/test_resnet_host.py): resnet18 has 11 689 512 parameters, resnet50 25 557 032.
2. The oracle composition of a network or block: oracle.ref.conv2d_affine_act per conv (pointwise convs at stride 1 in the
   summation order F.conv1x1_k_slices states, everything else the single ascending (c, ky, kx) chain), torch's CPU max_pool2d
   for the padded pool, oracle.ref.adaptive_avgpool and oracle.ref.linear_bias_relu (order of F.linear_k_slices).
   The oracle takes neither dilation nor general groups:
     - a dilated conv runs on the zero-stuffed kernel (3x3 with dilation 2 and padding 2 = a 5x5 kernel with zeros at the odd
       taps, padding 2): the zero taps add x * 0 = +-0 to the chain, which changes no finite sum, so the comparison is by value
       (+0 == -0; inputs are finite);
     - a grouped conv runs per channel slice.
"""
import numpy as np
import torch
from torch import nn

from oracle import ref


# ------------------------------------------------------------------------------------------------ the torch.nn replica
def conv3x3(in_planes, out_planes, stride=1, groups=1, dilation=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, groups=groups, bias=False, dilation=dilation)


def conv1x1(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None):
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        # the reference raises NotImplementedError for dilation > 1; the replica follows the library's superset (both convs dilated)
        self.conv1 = conv3x3(inplanes, planes, stride, dilation=dilation)
        self.bn1 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes, dilation=dilation)
        self.bn2 = norm_layer(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None):
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        width = int(planes * (base_width / 64.0)) * groups
        self.conv1 = conv1x1(inplanes, width)
        self.bn1 = norm_layer(width)
        self.conv2 = conv3x3(width, width, stride, groups, dilation)
        self.bn2 = norm_layer(width)
        self.conv3 = conv1x1(width, planes * self.expansion)
        self.bn3 = norm_layer(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000, zero_init_residual=False, groups=1, width_per_group=64,
                 replace_stride_with_dilation=None, norm_layer=None):
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        self._norm_layer = norm_layer
        self.inplanes = 64
        self.dilation = 1
        if replace_stride_with_dilation is None:
            replace_stride_with_dilation = [False, False, False]
        if len(replace_stride_with_dilation) != 3:
            raise ValueError(f"replace_stride_with_dilation should be None or a 3-element tuple, got {replace_stride_with_dilation}")
        self.groups = groups
        self.base_width = width_per_group
        self.conv1 = nn.Conv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2, dilate=replace_stride_with_dilation[0])
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2, dilate=replace_stride_with_dilation[1])
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2, dilate=replace_stride_with_dilation[2])
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck) and m.bn3.weight is not None:
                    nn.init.constant_(m.bn3.weight, 0)
                elif isinstance(m, BasicBlock) and m.bn2.weight is not None:
                    nn.init.constant_(m.bn2.weight, 0)

    def _make_layer(self, block, planes, blocks, stride=1, dilate=False):
        norm_layer = self._norm_layer
        downsample = None
        previous_dilation = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride), norm_layer(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, previous_dilation, norm_layer)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width, dilation=self.dilation,
                                norm_layer=norm_layer))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = torch.flatten(self.avgpool(x), 1)
        return self.fc(x)


def resnet18(**kw):
    return ResNet(BasicBlock, [2, 2, 2, 2], **kw)


def resnet34(**kw):
    return ResNet(BasicBlock, [3, 4, 6, 3], **kw)


def resnet50(**kw):
    return ResNet(Bottleneck, [3, 4, 6, 3], **kw)


def wide_resnet50_2(**kw):
    return ResNet(Bottleneck, [3, 4, 6, 3], width_per_group=128, **kw)


# ------------------------------------------------------------------------------------------------ the oracle composition
AFFINE = {None: 0, "mul_add": 1, "fma": 2}


def zero_stuffed(w, dilation):
    """(cout, cg, kh, kw) -> (cout, cg, d*(kh-1)+1, d*(kw-1)+1) with the taps at multiples of `dilation` and zeros between."""
    if dilation == 1:
        return w
    cout, cg, kh, kw = w.shape
    out = np.zeros((cout, cg, dilation * (kh - 1) + 1, dilation * (kw - 1) + 1), np.float32)
    out[:, :, ::dilation, ::dilation] = w
    return out


def oracle_conv(x, w, bias=None, alpha=None, beta=None, res=None, stride=1, padding=0, dilation=1, groups=1, affine=0, act=None,
                pointwise_order=False):
    """ref.conv2d_affine_act for any dilation and groups (square stride / padding / dilation).  pointwise_order: a 1x1 stride-1
    conv in the order F.conv1x1_k_slices states (what F.conv_norm_act runs); otherwise the single chain."""
    x, w = np.ascontiguousarray(x, np.float32), zero_stuffed(np.ascontiguousarray(w, np.float32), dilation)
    cout = w.shape[0]
    if groups == 1:
        sl = 0
        if pointwise_order:
            from cpu_vision_amd import functional as F
            slices, slen = F.conv1x1_k_slices(x.shape[0], x.shape[1], x.shape[2], x.shape[3], cout)
            sl = slen if slices > 1 else 0
        return ref.conv2d_affine_act(x, w, bias, alpha, beta, res, stride, padding, 1, affine, act, slice_len=sl)
    cg, mg = x.shape[1] // groups, cout // groups
    cut = lambda a, g: None if a is None else np.ascontiguousarray(a[g * mg:(g + 1) * mg])  # noqa: E731
    parts = [ref.conv2d_affine_act(np.ascontiguousarray(x[:, g * cg:(g + 1) * cg]), np.ascontiguousarray(w[g * mg:(g + 1) * mg]),
                                   cut(bias, g), cut(alpha, g), cut(beta, g),
                                   None if res is None else np.ascontiguousarray(res[:, g * mg:(g + 1) * mg]), stride, padding, 1,
                                   affine, act) for g in range(groups)]
    return np.concatenate(parts, axis=1)


def folded(norm):
    """(alpha, beta, affine code) of a norm container: BatchNorm2d through the oracle's own fold, FrozenBatchNorm2d through the
    reference's tensor expressions (ops/misc.py:55-60)."""
    if isinstance(norm, nn.BatchNorm2d):
        a, b = ref.fold_batchnorm(norm.weight.detach().numpy(), norm.bias.detach().numpy(), norm.running_mean.numpy(),
                                  norm.running_var.numpy(), norm.eps)
        return a, b, 2
    scale = norm.weight * (norm.running_var + norm.eps).rsqrt()
    shift = norm.bias - norm.running_mean * scale
    return scale.numpy(), shift.numpy(), 1


def oracle_conv_norm(x, conv, norm, relu, res=None):
    a, b, code = folded(norm)
    assert conv.stride[0] == conv.stride[1] and conv.padding[0] == conv.padding[1] and conv.dilation[0] == conv.dilation[1]
    pointwise = conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.groups == 1
    return oracle_conv(x, conv.weight.detach().numpy(), None if conv.bias is None else conv.bias.detach().numpy(), a, b, res,
                       conv.stride[0], conv.padding[0], conv.dilation[0], conv.groups, code, "relu" if relu else None,
                       pointwise_order=pointwise)


def oracle_block(block, x):
    """A BasicBlock / Bottleneck (the library's or the replica's: same names) through the oracle."""
    identity = x if block.downsample is None else oracle_conv_norm(x, block.downsample[0], block.downsample[1], relu=False)
    out = oracle_conv_norm(x, block.conv1, block.bn1, relu=True)
    if hasattr(block, "conv3"):
        out = oracle_conv_norm(out, block.conv2, block.bn2, relu=True)
        return oracle_conv_norm(out, block.conv3, block.bn3, relu=True, res=identity)
    return oracle_conv_norm(out, block.conv2, block.bn2, relu=True, res=identity)


def padded_max_pool(x, k, stride, pad):
    """torch's CPU max_pool2d: the reference of the padded pool."""
    return torch.nn.functional.max_pool2d(torch.from_numpy(np.ascontiguousarray(x)), k, stride, pad).numpy()


def oracle_resnet(model, x):
    """The whole network (CPU-resident parameters) through the oracle -> logits."""
    from cpu_vision_amd import functional as F
    a = oracle_conv_norm(np.ascontiguousarray(x, np.float32), model.conv1, model.bn1, relu=True)
    mp = model.maxpool
    a = padded_max_pool(a, mp.kernel_size, mp.stride, mp.padding)
    for layer in (model.layer1, model.layer2, model.layer3, model.layer4):
        for block in layer:
            a = oracle_block(block, a)
    a = ref.adaptive_avgpool(a, 1, 1).reshape(a.shape[0], -1)
    fc = model.fc
    slices, sl = F.linear_k_slices(a.shape[0], fc.in_features, fc.out_features)
    return ref.linear_bias_relu(a, fc.weight.detach().numpy(), fc.bias.detach().numpy(), relu=False, slice_len=sl if slices > 1 else 0)


def randomize_norms(model, seed):
    """Non-trivial BN statistics and affine terms (the default 1 / 0 would hide a folding error), seeded, in module order."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if getattr(m, "running_var", None) is not None:
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.2 - 0.1)
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) * 0.4 - 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.0 + 0.5)
