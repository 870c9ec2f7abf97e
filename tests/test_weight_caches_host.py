"""The seven per-module caches of derived weights, on CPU tensors: _FoldedNorm (mobilenet.py), _SlicedConv (segmentation.py), the joint
head weights of RPNHead / RetinaNetHead / FastRCNNPredictor and the relaid transposed-conv weights of MaskRCNNPredictor /
KeypointRCNNPredictor.  All are keyed by mobilenet._tensor_versions; a stale hit gives silently wrong outputs.  After every way a
parameter is commonly updated the cached value must equal a fresh computation bit for bit, tensor by tensor (a key that leaves one
tensor out fails here); with nothing changed the second call returns the identical objects.  Writes through `p.data` are the one
update the key cannot see: refresh_parameters(module) follows them."""
import copy
from functools import partial

import pytest
import torch
from torch import nn

import cpu_vision_amd as mv
from cpu_vision_amd import functional as F
from cpu_vision_amd import mobilenet, segmentation
from cpu_vision_amd.mobilenet import FrozenBatchNorm2d

CPU = torch.device("cpu")


def _cat(*pairs):
    return tuple(torch.cat([t.detach() for t in pair]).to(torch.float32).contiguous() for pair in pairs)


class Case:
    """make() -> module; cached(m, device) -> what the module's cache returns; fresh(m, device) -> the same value computed without
    the module's cache; names -> the state_dict entries the value depends on."""

    def __init__(self, make, cached, fresh, names):
        self.make, self.cached, self.fresh, self.names = make, cached, fresh, names


def _norm_block(norm_layer):
    return mobilenet.Conv2dNormActivation(4, 6, norm_layer=norm_layer)


_NORM_NAMES = ("1.weight", "1.bias", "1.running_mean", "1.running_var")
CASES = {
    "folded_norm_batchnorm": Case(partial(_norm_block, nn.BatchNorm2d), lambda m, d: m._fold.get(m[1], d),
                                  lambda m, d: mobilenet._FoldedNorm().get(m[1], d), _NORM_NAMES),
    "folded_norm_frozen": Case(partial(_norm_block, FrozenBatchNorm2d), lambda m, d: m._fold.get(m[1], d),
                               lambda m, d: mobilenet._FoldedNorm().get(m[1], d), _NORM_NAMES),
    # 132 input channels: two slices, SLICE_CHANNELS and a remainder, both copies of the weight
    "sliced_conv": Case(lambda: segmentation.FCNHead(132, 3), lambda m, d: m._fold.get(m[0], m[1], d),
                        lambda m, d: segmentation._SlicedConv().get(m[0], m[1], d), ("0.weight",) + _NORM_NAMES),
    "rpn_joint": Case(lambda: mv.RPNHead(8, 3), lambda m, d: m.joint_pointwise(d),
                      lambda m, d: _cat((m.cls_logits.weight, m.bbox_pred.weight), (m.cls_logits.bias, m.bbox_pred.bias)),
                      ("cls_logits.weight", "cls_logits.bias", "bbox_pred.weight", "bbox_pred.bias")),
    "retinanet_joint": Case(lambda: mv.RetinaNetHead(8, 2, 3), lambda m, d: m.joint_first_layer(d),
                            lambda m, d: _cat(*[(getattr(m.classification_head.conv[0][0], t), getattr(m.regression_head.conv[0][0], t))
                                                for t in ("weight", "bias")]),
                            tuple(f"{h}.conv.0.0.{t}" for t in ("weight", "bias") for h in ("classification_head", "regression_head"))),
    "faster_rcnn_joint": Case(lambda: mv.FastRCNNPredictor(8, 3), lambda m, d: m.joint_linear(d),
                              lambda m, d: _cat((m.cls_score.weight, m.bbox_pred.weight), (m.cls_score.bias, m.bbox_pred.bias)),
                              ("cls_score.weight", "cls_score.bias", "bbox_pred.weight", "bbox_pred.bias")),
    "mask_rcnn_relaid": Case(lambda: mv.MaskRCNNPredictor(8, 4, 3), lambda m, d: m.relaid(d),
                             lambda m, d: F.conv_transpose2x2_relayout(m.conv5_mask.weight, m.conv5_mask.bias, d),
                             ("conv5_mask.weight", "conv5_mask.bias")),
    "keypoint_rcnn_relaid": Case(lambda: mv.KeypointRCNNPredictor(8, 3), lambda m, d: m.relaid(d),
                                 lambda m, d: F.conv_transpose4x4_relayout(m.kps_score_lowres.weight, m.kps_score_lowres.bias, d),
                                 ("kps_score_lowres.weight", "kps_score_lowres.bias")),
}


def _flat(value):
    out = []
    for v in value:
        out.extend(v if isinstance(v, (list, tuple)) else [v])
    return out


def _same(a, b, what):
    a, b = _flat(a), _flat(b)
    assert len(a) == len(b), what
    for i, (u, v) in enumerate(zip(a, b)):
        if isinstance(u, torch.Tensor):
            assert u.dtype == v.dtype and u.device == v.device and u.shape == v.shape and torch.equal(u, v), f"{what}: element {i}"
        else:
            assert u == v, f"{what}: element {i}"


def _differs(a, b):
    return any(isinstance(u, torch.Tensor) and not torch.equal(u, v) for u, v in zip(_flat(a), _flat(b)))


def _entry(module, name):
    """(owner module, attribute, tensor) of a state_dict entry."""
    path, attr = name.rsplit(".", 1)
    owner = module.get_submodule(path)
    return owner, attr, getattr(owner, attr)


def _module(case, seed):
    torch.manual_seed(seed)
    m = case.make().eval()
    with torch.no_grad():  # every entry random and distinct, variances positive
        for name, t in m.state_dict().items():
            if t.is_floating_point():
                t.copy_(torch.rand(t.shape) + 0.5)
    return m


def _new_values(t, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(t.shape, generator=g) + 0.25).to(t.dtype)


def _check_follows(case, m, before, what):
    got = case.cached(m, CPU)
    _same(got, case.fresh(m, CPU), what)
    assert _differs(got, before), f"{what}: the update did not change the derived value (vacuous)"
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_unchanged_parameters_return_the_identical_objects(name):
    case = CASES[name]
    m = _module(case, 1)
    first, second = _flat(case.cached(m, CPU)), _flat(case.cached(m, CPU))
    _same(first, case.fresh(m, CPU), name)
    assert len(first) == len(second) and all(a is b for a, b in zip(first, second))


@pytest.mark.parametrize("name", list(CASES))
def test_in_place_update_under_no_grad(name):
    case = CASES[name]
    m = _module(case, 2)
    value = case.cached(m, CPU)
    for k, entry in enumerate(case.names):
        t = _entry(m, entry)[2]
        with torch.no_grad():
            t.mul_(1.5).add_(0.125)
        value = _check_follows(case, m, value, f"{name}: {entry}.mul_().add_()")
        with torch.no_grad():
            t.copy_(_new_values(t, 20 + k))
        value = _check_follows(case, m, value, f"{name}: {entry}.copy_()")


@pytest.mark.parametrize("assign", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_load_state_dict(name, assign):
    case = CASES[name]
    m = _module(case, 3)
    value = case.cached(m, CPU)
    for k, entry in enumerate(case.names):  # one changed entry per load: every tensor of the key is seen on its own
        state = {n: t.clone() for n, t in m.state_dict().items()}
        state[entry] = _new_values(state[entry], 30 + k)
        m.load_state_dict(state, strict=True, assign=assign)
        value = _check_follows(case, m, value, f"{name}: load_state_dict(assign={assign}) with a new {entry}")


@pytest.mark.parametrize("name", list(CASES))
def test_replaced_parameter_object(name):
    case = CASES[name]
    m = _module(case, 4)
    value = case.cached(m, CPU)
    for k, entry in enumerate(case.names):
        owner, attr, t = _entry(m, entry)
        new = _new_values(t, 40 + k)
        setattr(owner, attr, nn.Parameter(new, requires_grad=t.requires_grad) if isinstance(t, nn.Parameter) else new)
        del t
        value = _check_follows(case, m, value, f"{name}: {entry} replaced")


@pytest.mark.parametrize("name", list(CASES))
def test_dtype_round_trip(name):
    case = CASES[name]
    m = _module(case, 5)
    case.cached(m, CPU)
    m.double()
    with torch.no_grad():
        for entry in case.names:  # a change made while the module is float64, exact in float32
            _entry(m, entry)[2].mul_(2.0)
    m.float()
    _same(case.cached(m, CPU), case.fresh(m, CPU), f"{name}: .double(), an update, .float()")
    m.double().float()
    _same(case.cached(m, CPU), case.fresh(m, CPU), f"{name}: .double().float()")


@pytest.mark.gpu  # the one test of this file that needs a second device in the process
@pytest.mark.parametrize("name", list(CASES))
def test_device_move(name):
    case = CASES[name]
    m = _module(case, 6)
    on_cpu = case.cached(m, CPU)
    dev = torch.device("cuda", torch.cuda.current_device())
    m.to(dev)
    got = case.cached(m, dev)
    _same(got, case.fresh(m, dev), f"{name}: moved to {dev}")
    _same([t.cpu() if isinstance(t, torch.Tensor) else t for t in _flat(got)], on_cpu, f"{name}: the same values on {dev}")
    m.to(CPU)
    _same(case.cached(m, CPU), on_cpu, f"{name}: moved back")


@pytest.mark.parametrize("name", list(CASES))
def test_data_writes_need_refresh_parameters(name):
    case = CASES[name]
    m = _module(case, 7)
    value = case.cached(m, CPU)
    for entry in case.names:
        _entry(m, entry)[2].data.mul_(2)
        assert mv.refresh_parameters(m) is m
        value = _check_follows(case, m, value, f"{name}: {entry}.data.mul_(2), then refresh_parameters")


def test_refresh_parameters_reaches_nested_modules_and_the_getter_plan():
    torch.manual_seed(8)
    body = nn.Sequential()
    body.add_module("conv1", nn.Conv2d(3, 4, 3, padding=1, bias=False))
    body.add_module("bn1", nn.BatchNorm2d(4))
    body.add_module("relu", nn.ReLU())
    getter = mv.IntermediateLayerGetter(body, {"relu": "0"})
    tree = nn.ModuleDict({"getter": getter, "heads": nn.ModuleList([mv.RPNHead(4, 2), segmentation.FCNHead(8, 2)])})
    folds = [c for step in getter._plan for c in step if isinstance(c, mobilenet._FoldedNorm)]
    assert len(folds) == 1
    before = folds[0].get(getter["bn1"], CPU)
    joint, sliced = tree["heads"][0].joint_pointwise(CPU), tree["heads"][1]._fold.get(tree["heads"][1][0], tree["heads"][1][1], CPU)
    for p in list(tree.parameters()) + list(tree.buffers()):
        if p.is_floating_point():
            p.data.mul_(2)
            p.data.add_(0.5)
    mv.refresh_parameters(tree)
    after = folds[0].get(getter["bn1"], CPU)
    _same(after, mobilenet._FoldedNorm().get(getter["bn1"], CPU), "the getter's plan")
    assert _differs(after, before)
    head, fcn = tree["heads"]
    assert _differs(head.joint_pointwise(CPU), joint)
    _same(head.joint_pointwise(CPU), _cat((head.cls_logits.weight, head.bbox_pred.weight), (head.cls_logits.bias, head.bbox_pred.bias)), "RPNHead")
    got = fcn._fold.get(fcn[0], fcn[1], CPU)
    _same(got, segmentation._SlicedConv().get(fcn[0], fcn[1], CPU), "FCNHead")
    assert _differs(got, sliced)


# ---- _SlicedConv: the zero shift follows the folded norm, the slices follow the weight ------------------------------------------------------
def test_sliced_conv_when_only_the_norm_changes():
    case = CASES["sliced_conv"]
    m = _module(case, 9)
    alpha, beta, mode, weights, zero = case.cached(m, CPU)
    m[1] = nn.BatchNorm2d(m[1].num_features, eps=1e-3).eval()  # another norm object, the conv untouched
    with torch.no_grad():
        m[1].running_var.copy_(torch.rand(m[1].num_features) + 0.5)
    got = case.cached(m, CPU)
    _same(got, case.fresh(m, CPU), "a replaced norm")
    assert all(a is b for a, b in zip(got[3], weights)), "the slices follow the weight alone"
    assert got[4].shape == got[1].shape and got[4].device == got[1].device and not got[4].any()
    assert _differs(got[:2], (alpha, beta))


def test_sliced_conv_with_x_on_another_device_than_the_weights():
    """The shift added to the slices after the first must lie where alpha and beta lie: on x's device.  The meta device stands
    for the second one, so this runs in a process with a single device too."""
    case = CASES["sliced_conv"]
    m = _module(case, 10)
    case.cached(m, CPU)
    other = torch.device("meta")
    alpha, beta, mode, weights, zero = case.cached(m, other)
    assert alpha.device == beta.device == zero.device == other and zero.shape == beta.shape
    back = case.cached(m, CPU)
    _same(back, case.fresh(m, CPU), "back on the weights' device")
    assert back[4].device == CPU and not back[4].any()


def test_deepcopy_does_not_share_a_cache():
    case = CASES["rpn_joint"]
    m = _module(case, 11)
    case.cached(m, CPU)
    twin = copy.deepcopy(m)
    with torch.no_grad():
        twin.cls_logits.weight.mul_(3.0)
    _same(case.cached(twin, CPU), case.fresh(twin, CPU), "the copy")
    _same(case.cached(m, CPU), case.fresh(m, CPU), "the original")
