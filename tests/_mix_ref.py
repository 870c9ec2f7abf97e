"""torchvision 0.20's MixUp / CutMix (transforms/v2/_augment.py) and RandomApply / RandomChoice / RandomOrder
(transforms/v2/_container.py), restated with torch CPU ops: the parameter draws in the reference's order of host RNG calls, the
image and label arithmetic, and the containers' control flow.  Nothing here imports the package under test."""
import math

import torch


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------------
def mixup_image(inpt, lam):
    return inpt.roll(1, 0).mul_(1.0 - lam).add_(inpt.mul(lam))


def cutmix_image(inpt, box):
    x1, y1, x2, y2 = box
    rolled = inpt.roll(1, 0)
    output = inpt.clone()
    output[..., y1:y2, x1:x2] = rolled[..., y1:y2, x1:x2]
    return output


def mixup_label(label, lam, num_classes=None):
    if label.ndim == 1:
        label = torch.nn.functional.one_hot(label, num_classes=num_classes)
    if not label.dtype.is_floating_point:
        label = label.float()
    return label.roll(1, 0).mul_(1.0 - lam).add_(label.mul(lam))


# ---- the parameter draws ----------------------------------------------------------------------------------------------------------
def beta(alpha):
    return torch.distributions.Beta(torch.tensor([alpha]), torch.tensor([alpha]))


def mixup_params(dist):
    return dict(lam=float(dist.sample(())))


def cutmix_params(dist, H, W):
    lam = float(dist.sample(()))
    r_x = torch.randint(W, size=(1,))
    r_y = torch.randint(H, size=(1,))
    r = 0.5 * math.sqrt(1.0 - lam)
    r_w_half = int(r * W)
    r_h_half = int(r * H)
    x1 = int(torch.clamp(r_x - r_w_half, min=0))
    y1 = int(torch.clamp(r_y - r_h_half, min=0))
    x2 = int(torch.clamp(r_x + r_w_half, max=W))
    y2 = int(torch.clamp(r_y + r_h_half, max=H))
    box = (x1, y1, x2, y2)
    lam_adjusted = float(1.0 - (x2 - x1) * (y2 - y1) / (W * H))
    return dict(box=box, lam=lam_adjusted)


# ---- the batch transforms on an (images, labels) pair ------------------------------------------------------------------------------
class MixUp:
    def __init__(self, alpha=1.0, num_classes=None):
        self.dist, self.num_classes = beta(alpha), num_classes

    def __call__(self, images, labels):
        lam = mixup_params(self.dist)["lam"]
        return mixup_image(images, lam), mixup_label(labels, lam, self.num_classes)


class CutMix:
    def __init__(self, alpha=1.0, num_classes=None):
        self.dist, self.num_classes = beta(alpha), num_classes

    def __call__(self, images, labels):
        params = cutmix_params(self.dist, images.shape[-2], images.shape[-1])
        return cutmix_image(images, params["box"]), mixup_label(labels, params["lam"], self.num_classes)


# ---- the containers -----------------------------------------------------------------------------------------------------------------
def _thread(transforms, inputs):
    needs_unpacking = len(inputs) > 1
    for transform in transforms:
        outputs = transform(*inputs)
        inputs = outputs if needs_unpacking else (outputs,)
    return outputs


def random_apply(transforms, p, *inputs):
    if torch.rand(1) >= p:
        return inputs if len(inputs) > 1 else inputs[0]
    return _thread(transforms, inputs)


def random_choice(transforms, p, *inputs):
    if p is None:
        p = [1] * len(transforms)
    total = sum(p)
    p = [prob / total for prob in p]
    idx = int(torch.multinomial(torch.tensor(p), 1))
    return transforms[idx](*inputs)


def random_order(transforms, *inputs):
    return _thread([transforms[idx] for idx in torch.randperm(len(transforms))], inputs)
