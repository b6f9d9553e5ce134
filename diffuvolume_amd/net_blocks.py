"""What the ACV (ReLU) and PCW (Mish) networks are built from, written once and parametrised by the activation:

  * the parameter containers under the reference's state_dict names -- ``cb2`` / ``cb3`` (convbn), ``BasicBlock``,
    ``stack``, ``head2d``, ``Mish`` and the 3-D ``Hourglass`` (with ACV's bottleneck window attention when ``heads`` is
    given);
  * ``walk``: a (nested) Sequential of the training graph, then ``+ skip`` and ``act`` -- the one place that decides what
    rides in a BatchNorm statement (``train_norm.bn_act`` / ``train_net2d.bn_act2d``) and which route a convolution takes;
  * the prepared inference layers of those containers: ``plan_cb2`` / ``plan_cb3`` / ``deconv_plan`` / ``plan_seq2d``,
    ``BasicBlockPlan``, ``HourglassPlan`` and ``PairPlan``.  A plan reads its activation off the module it prepares.

``acv_ddim``, ``pwcnet_ddim`` and ``train_net2d`` import from here; this module imports none of them."""
from __future__ import annotations

import math
from typing import Callable, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import train2d, train3d
from .submodule import ACT_NONE, Conv2dPlan, Conv3dPlan, Deconv3dPlan, window_attention
from .train_norm import ACTS, act_statement, bn_act


# --------------------------------------------------------------------------------------
# parameter containers (names = reference state_dict keys)
# --------------------------------------------------------------------------------------
class Mish(nn.Module):
    """x * tanh(softplus(x)) (KITTI12/models/submodule.py:11-18)."""

    def forward(self, x):
        return x * torch.tanh(F.softplus(x))


def act_module(act: str) -> nn.Module:
    """A fresh activation member of a container: ``"relu"`` (in place, as the reference has it) or ``"mish"``."""
    return {"relu": lambda: nn.ReLU(inplace=True), "mish": Mish}[act]()


def act_of(m: nn.Module) -> Optional[str]:
    """``"relu"`` / ``"mish"`` for an activation member, None for anything else."""
    return "relu" if isinstance(m, nn.ReLU) else "mish" if isinstance(m, Mish) else None


def cb2(cin, cout, k, stride, pad, dil):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, dil if dil > 1 else pad, dil, bias=False),
                         nn.BatchNorm2d(cout))


def cb3(cin, cout, k, stride, pad):
    return nn.Sequential(nn.Conv3d(cin, cout, k, stride, pad, bias=False), nn.BatchNorm3d(cout))


def head2d(cin, mid, cout, act="mish"):
    return nn.Sequential(cb2(cin, mid, 3, 1, 1, 1), act_module(act), nn.Conv2d(mid, cout, 1, bias=False))


class BasicBlock(nn.Module):
    """BasicBlock of the 2-D networks (SceneFlow/models/submodule.py:307-330 with ReLU, KITTI12/models/submodule.py:192-215
    with Mish): no activation behind the add."""

    def __init__(self, cin, planes, stride, downsample, pad, dil, act):
        super().__init__()
        self.conv1 = nn.Sequential(cb2(cin, planes, 3, stride, pad, dil), act_module(act))
        self.conv2 = cb2(planes, planes, 3, 1, pad, dil)
        self.downsample = downsample

    def forward(self, x):
        y = self.conv2(self.conv1(x))
        return y + (x if self.downsample is None else self.downsample(x))


def stack(inplanes, planes, blocks, stride, pad, dil, act):
    """``_make_layer`` of the reference: ``blocks`` BasicBlocks, the first behind a 1x1 downsample when the shape changes."""
    down = None
    if stride != 1 or inplanes != planes:
        down = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
    layers = [BasicBlock(inplanes, planes, stride, down, pad, dil, act)]
    layers += [BasicBlock(planes, planes, 1, None, pad, dil, act) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


class WindowAttention(nn.Module):
    """Parameters of attention_block (SceneFlow/models/submodule.py:383-396)."""

    def __init__(self, channels: int, num_heads: int):
        super().__init__()
        self.num_heads = num_heads
        self.qkv_3d = nn.Linear(channels, channels * 3, bias=True)
        self.final1x1 = nn.Conv3d(channels, channels, 1)


class Hourglass(nn.Module):
    """3-D encoder/decoder with skip convs (acv_ddim.py:56-93, pwcnet_ddim.py:208-248); ``heads``: ACV's bottleneck window
    attention, registered between ``conv4`` and ``conv5``, and ``attention(block, x)``, the function that runs it in
    training."""

    def __init__(self, c: int, act: str, heads: Optional[int] = None, attention: Optional[Callable] = None):
        super().__init__()
        if (heads is None) != (attention is None):
            raise ValueError("`heads` and `attention` go together")
        self.act, self.attention = act, attention
        self.conv1 = nn.Sequential(cb3(c, 2 * c, 3, 2, 1), act_module(act))
        self.conv2 = nn.Sequential(cb3(2 * c, 2 * c, 3, 1, 1), act_module(act))
        self.conv3 = nn.Sequential(cb3(2 * c, 4 * c, 3, 2, 1), act_module(act))
        self.conv4 = nn.Sequential(cb3(4 * c, 4 * c, 3, 1, 1), act_module(act))
        if heads is not None:
            self.attention_block = WindowAttention(4 * c, heads)
        self.conv5 = nn.Sequential(nn.ConvTranspose3d(4 * c, 2 * c, 3, padding=1, output_padding=1, stride=2, bias=False),
                                   nn.BatchNorm3d(2 * c))
        self.conv6 = nn.Sequential(nn.ConvTranspose3d(2 * c, c, 3, padding=1, output_padding=1, stride=2, bias=False),
                                   nn.BatchNorm3d(c))
        self.redir1 = cb3(c, c, 1, 1, 0)
        self.redir2 = cb3(2 * c, 2 * c, 1, 1, 0)

    def forward(self, x):
        """Training path (acv_ddim.py:88-93, pwcnet_ddim.py:235-248); eval runs ``HourglassPlan``."""
        c2 = walk(self.conv2, walk(self.conv1, x))
        c4 = walk(self.conv4, walk(self.conv3, c2))
        if self.attention is not None:
            c4 = self.attention(self.attention_block, c4)
        c5 = walk(self.conv5, c4, self.act, skip=walk(self.redir2, c2))
        return walk(self.conv6, c5, self.act, skip=walk(self.redir1, x))


def init_weights(model: nn.Module) -> None:
    """The reference's weight initialisation (acv_ddim.py:224-238, pwcnet_ddim.py:433-447), in ``modules()`` order."""
    for m in model.modules():
        if isinstance(m, (nn.Conv2d, nn.Conv3d)) and not isinstance(m, nn.ConvTranspose3d):
            n = m.out_channels
            for k in m.kernel_size:
                n *= k
            m.weight.data.normal_(0, math.sqrt(2.0 / n))
        elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
            m.weight.data.fill_(1)
            m.bias.data.zero_()
        elif isinstance(m, nn.Linear):
            m.bias.data.zero_()


# --------------------------------------------------------------------------------------
# the training walk
# --------------------------------------------------------------------------------------
def leaves(m: nn.Module):
    if isinstance(m, nn.Sequential):
        for c in m:
            yield from leaves(c)
    else:
        yield m


def walk(mod: nn.Module, x: torch.Tensor, act: str = "none", skip: Optional[torch.Tensor] = None,
         conv2d: Callable = train2d.conv2d_module, bn2d: Optional[Callable] = None) -> torch.Tensor:
    """``act(mod(x) + skip)`` for a (nested) Sequential, or a single module, of the training graph, leaf by leaf.

    A BatchNorm is one statement with what follows it: the ReLU or Mish behind it, or -- when it is the last leaf -- the
    caller's ``skip`` and ``act``, so that DV_TRAIN_NORM=hip runs them as one kernel.  (An activation that is the last leaf
    is not fused when the caller passed an ``act`` or a ``skip``: the BatchNorm runs alone, the activation module behind
    it, then ``+ skip``, then ``act``.)  A BatchNorm3d goes to ``train_norm.bn_act``; a BatchNorm2d to ``bn2d`` (the
    caller passes ``train_net2d.bn_act2d`` where the 2-D statement runs on HIP) or, without one, to its own forward.
    Conv3d / ConvTranspose3d run on ``train3d`` at the ambient train precision, a Conv2d on ``conv2d`` (``train2d``'s
    ``conv2d_module`` for refinenet3, ``Net2d.conv`` for the feature CNNs); any other module is called."""
    mods = list(leaves(mod))
    i, n = 0, len(mods)
    while i < n:
        m, step = mods[i], 1
        if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
            a, s = "none", None
            behind = act_of(mods[i + 1]) if i + 1 < n else None
            if i + 1 == n:
                a, s, act, skip = act, skip, "none", None
            elif behind is not None and (i + 2 < n or (act == "none" and skip is None)):
                a, step = behind, 2
            if isinstance(m, nn.BatchNorm3d):
                x = bn_act(m, x, a, s)
            elif bn2d is not None:
                x = bn2d(m, x, a, s)
            else:
                x = act_statement(m(x), a, s)
        elif isinstance(m, nn.ConvTranspose3d):
            x = train3d.conv_transpose3d_module(m, x)
        elif isinstance(m, nn.Conv3d):
            x = train3d.conv3d_module(m, x)
        elif isinstance(m, nn.Conv2d):
            x = conv2d(m, x)
        else:
            x = m(x)
        i += step
    return act_statement(x, act, skip)


# --------------------------------------------------------------------------------------
# prepared (device-resident, BN-folded, repacked) inference layers
# --------------------------------------------------------------------------------------
def act_code(m: nn.Module) -> int:
    """ACT_RELU / ACT_MISH of an activation member (ACT_NONE for anything else)."""
    return ACTS[act_of(m) or "none"]


def bn_of(bn: nn.Module):
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var)


def plan_cb2(seq: nn.Sequential, act: int, dil: Optional[int] = None) -> Conv2dPlan:
    """convbn 2-D (Conv2d + BatchNorm2d, submodule.py:21-24) -> fused plan (stride 1 or 2).  ``dil``: the dilation LEFT of
    the layer's own when its input is already de-interleaved into sub-images (`space_to_batch2`, level l: dil = dilation >> l)."""
    conv, bn = seq[0], seq[1]
    return Conv2dPlan(conv.weight, bn_of(bn), dilation=conv.dilation[0] if dil is None else dil, act=act, eps=bn.eps,
                      stride=conv.stride[0])


def plan_cb3(seq: nn.Sequential, stride: int, act: int) -> Conv3dPlan:
    return Conv3dPlan(seq[0].weight, bn_of(seq[1]), stride=stride, act=act, eps=seq[1].eps)


def plan_seq2d(seq: nn.Sequential) -> list:
    """The plans of a 2-D Sequential of convbn + activation members and bare Conv2d members (firstconv, the heads,
    layer_refine), in order."""
    members = list(seq)
    plans = []
    for i, m in enumerate(members):
        if isinstance(m, nn.Sequential):
            plans.append(plan_cb2(m, act_code(members[i + 1]) if i + 1 < len(members) else ACT_NONE))
        elif isinstance(m, nn.Conv2d):
            plans.append(Conv2dPlan(m.weight, None, act=ACT_NONE))
    return plans


def run_plans(plans, x: torch.Tensor) -> torch.Tensor:
    for p in plans:
        x = p(x)
    return x


def deconv_plan(seq: nn.Sequential, act: int, redir: Optional[nn.Sequential] = None) -> Deconv3dPlan:
    """ConvTranspose3d + BN [+ the 1x1x1 `redir` conv + BN of the skip tensor folded into the same launch]."""
    if redir is None:
        return Deconv3dPlan(seq[0].weight, bn_of(seq[1]), act=act, eps=seq[1].eps)
    return Deconv3dPlan(seq[0].weight, bn_of(seq[1]), act=act, eps=seq[1].eps,
                        redir=(redir[0].weight, bn_of(redir[1])), redir_eps=redir[1].eps)


class BasicBlockPlan:
    """BasicBlock: convbn + activation, convbn, `out += x` (x through the 1x1 downsample when the shape changes); the add
    rides in the second convolution's epilogue, no activation after it.  ``down_first``: the order of the two independent
    launches in front of it -- PCW launches the downsample before ``conv1``, ACV behind it; each keeps its own."""

    def __init__(self, blk: BasicBlock, dil: Optional[int] = None, down_first: bool = True):
        self.down_first = down_first
        self.dilation = blk.conv2[0].dilation[0]
        self.conv1 = plan_cb2(blk.conv1[0], act_code(blk.conv1[1]), dil)
        self.conv2 = plan_cb2(blk.conv2, ACT_NONE, dil)
        self.down = None if blk.downsample is None else plan_cb2(blk.downsample, ACT_NONE)

    def __call__(self, x, group=1):
        down = (lambda t: t) if self.down is None else self.down
        if self.down_first:
            skip, y = down(x), self.conv1(x, group=group)
        else:
            y, skip = self.conv1(x, group=group), down(x)
        return self.conv2(y, residual=skip, group=group)


class HourglassPlan:
    """``filtered``: also the members of a step's first hourglass, whose input is ``volume * filter`` (``in_scale``)."""

    def __init__(self, hg: Hourglass, filtered: bool = False):
        act = ACTS[hg.act]
        self.conv1 = plan_cb3(hg.conv1[0], 2, act)
        self.conv2 = plan_cb3(hg.conv2[0], 1, act)
        self.conv3 = plan_cb3(hg.conv3[0], 2, act)
        self.conv4 = plan_cb3(hg.conv4[0], 1, act)
        ab = getattr(hg, "attention_block", None)
        self.attn = None
        if ab is not None:
            self.heads = ab.num_heads
            self.attn = tuple(t.detach().float().contiguous() for t in
                              (ab.qkv_3d.weight, ab.qkv_3d.bias,
                               ab.final1x1.weight.reshape(ab.final1x1.weight.shape[0], -1), ab.final1x1.bias))
        # act(BN(deconv) + BN(redir(skip))): the 1x1x1 redir convolutions ride inside the transposed convolutions
        self.conv5 = deconv_plan(hg.conv5, act, hg.redir2)
        self.conv6 = deconv_plan(hg.conv6, act, hg.redir1)
        if filtered:
            self.conv6_plain = deconv_plan(hg.conv6, act)        # filtered skip (first hourglass of a step)
            self.redir1 = plan_cb3(hg.redir1, 1, ACT_NONE)

    def __call__(self, x, in_scale=None):
        """``in_scale`` is the [0,1] volume filter: the reference feeds ``volume * noise`` to conv1 AND to
        redir1 (pwcnet_ddim.py:472-474, :245), so both take the prologue."""
        c2 = self.conv2(self.conv1(x, in_scale=in_scale))
        c4 = self.conv4(self.conv3(c2))
        if self.attn is not None:
            c4 = window_attention(c4, *self.attn, heads=self.heads)
        c5 = self.conv5(c4, skip=c2)                                        # act(deconv + redir2(conv2))
        if in_scale is None:
            return self.conv6(c5, skip=x)                                   # act(deconv + redir1(x))
        return self.conv6_plain(c5, residual=self.redir1(x, in_scale=in_scale))


class PairPlan:
    """convbn-act-conv[bn][-act] stacks (dres0 / dres1 / classif*, acv_ddim.py:200-222)."""

    def __init__(self, seq: nn.Sequential):
        act, last = act_code(seq[1]), seq[2]
        self.a = plan_cb3(seq[0], 1, act)
        if isinstance(last, nn.Sequential):
            self.b = plan_cb3(last, 1, act_code(seq[3]) if len(seq) > 3 else ACT_NONE)
        else:
            self.b = Conv3dPlan(last.weight, None, stride=1, act=ACT_NONE)

    def __call__(self, x, in_scale=None, residual_self=False):
        y = self.a(x, in_scale=in_scale)
        return self.b(y, residual=x if residual_self else None)

    def second(self, y):
        return self.b(y)
