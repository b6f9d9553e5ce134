"""Deterministic synthetic weights and stereo inputs (no checkpoints or datasets ship with
the reference: README.md:8, .MISSING_LARGE_BLOBS).  Every tensor is drawn from its own
CPU generator seeded by crc32(key) ^ seed, so the values depend only on (seed, key, shape)
-- not on module construction order -- and are identical here and on the GPU box.  Used by
oracle/make_golden.py (loaded into the imported reference), the tests and bench.py."""
from __future__ import annotations

import math
import zlib
from typing import Dict, Mapping

import torch


def _gen(seed: int, key: str) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed((zlib.crc32(key.encode()) ^ (seed * 0x9E3779B1)) & 0x7FFFFFFF)
    return g


def synth_state_dict(template: Mapping[str, torch.Tensor], seed: int = 0, logit_gain: float = 1.0,
                     scale: Mapping[str, float] | None = None) -> Dict[str, torch.Tensor]:
    """Random but well-conditioned values for every entry of ``template`` (a state_dict):
    conv weights ~ N(0, sqrt(2/(k^3*Cout))) as the reference initialises them
    (acv_ddim.py:224-238), BatchNorm with NON-trivial affine and running statistics,
    xavier-uniform Linear weights.  float64 schedule buffers are kept.  ``logit_gain``
    scales the single-channel classifier heads (sharper or flatter softmax); ``scale`` multiplies
    named tensors."""
    keys = set(template.keys())
    out: Dict[str, torch.Tensor] = {}
    for key, ref in template.items():
        g = _gen(seed, key)
        shape = tuple(ref.shape)
        leaf = key.rsplit(".", 1)[-1]
        stem = key.rsplit(".", 1)[0]
        is_bn = (stem + ".running_mean") in keys
        if ref.dtype == torch.float64 or not ref.dtype.is_floating_point:
            out[key] = ref.clone()                       # schedule buffers, num_batches_tracked
        elif leaf == "running_mean":
            out[key] = torch.randn(shape, generator=g) * 0.1
        elif leaf == "running_var":
            out[key] = torch.rand(shape, generator=g) + 0.5
        elif is_bn and leaf == "weight":
            out[key] = torch.rand(shape, generator=g) * 0.4 + 0.8
        elif is_bn and leaf == "bias":
            out[key] = torch.randn(shape, generator=g) * 0.1
        elif leaf == "weight" and ref.dim() >= 3:        # Conv2d / Conv3d / ConvTranspose3d
            kprod = 1
            for s in shape[2:]:
                kprod *= s
            std = math.sqrt(2.0 / (kprod * shape[0]))
            w = torch.randn(shape, generator=g) * std
            if shape[0] == 1 and ref.dim() == 5:
                w = w * logit_gain
            out[key] = w
        elif leaf == "weight" and ref.dim() == 2:        # Linear
            a = math.sqrt(6.0 / (shape[0] + shape[1]))
            out[key] = (torch.rand(shape, generator=g) * 2 - 1) * a
        elif leaf == "bias":
            out[key] = torch.randn(shape, generator=g) * 0.02
        else:
            out[key] = torch.randn(shape, generator=g) * 0.1
        if scale and key in scale:
            out[key] = out[key] * scale[key]       # e.g. tame an untrained residual head
        out[key] = out[key].to(ref.dtype)
    return out


def synth_features(b: int, c: int, h: int, w: int, seed: int, shifts=(6, 24, 60)) -> Dict[str, torch.Tensor]:
    """Left/right feature maps with a real correlation ridge: right = left shifted by a
    per-image disparity (in feature pixels) plus noise."""
    g = _gen(seed, f"features{b}x{c}x{h}x{w}")
    left = torch.randn(b, c, h, w, generator=g)
    right = torch.empty_like(left)
    for i in range(b):
        d = shifts[i % len(shifts)] // 4 if w > 16 else 1
        right[i] = torch.roll(left[i], shifts=-d, dims=-1)
    right = right + 0.05 * torch.randn(b, c, h, w, generator=g)
    return {"left": left, "right": right}


def synth_stereo_batch(b: int, h: int, w: int, seed: int = 0, shifts=(6, 24, 60)) -> Dict[str, torch.Tensor]:
    """left = randn, right = left rolled by d0 px + noise, gt = d0 + randn clamped
    to (0,192), used = gt + 0.5 randn (stand-in for the origin network), disp = bilinear/4."""
    import torch.nn.functional as F
    g = _gen(seed, f"stereo{b}x{h}x{w}")
    left = torch.randn(b, 3, h, w, generator=g)
    right = torch.empty_like(left)
    gt = torch.empty(b, h, w)
    for i in range(b):
        d0 = shifts[i % len(shifts)]
        right[i] = torch.roll(left[i], shifts=-d0, dims=-1)
        gt[i] = d0 + torch.randn(h, w, generator=g)
    right = right + 0.05 * torch.randn(b, 3, h, w, generator=g)
    gt = gt.clamp(0.5, 191.0)
    used = (gt + 0.5 * torch.randn(b, h, w, generator=g)).clamp(0.0, 191.0)
    disp = F.interpolate(used.clamp(0, 191).unsqueeze(1), size=(h // 4, w // 4), mode="bilinear") / 4
    return {"left": left, "right": right, "gt": gt, "used": used, "disp": disp}


def synth_hot_inputs(batch: int, h: int, w: int, seed: int, shifts=(6, 24, 60)) -> Dict[str, torch.Tensor]:
    """Inputs of the hot path at quarter resolution h x w: 320-channel gwc features and 32-channel
    concat features with a real correlation ridge (right = left rolled by the pair's disparity + noise), attention
    logits, full-resolution ground truth, the origin network's stand-in ``used`` and its quarter-resolution
    encoding input ``dq``.  CPU tensors; bench.py and the full-size parity tests move them to the device."""
    import torch.nn.functional as F
    g = _gen(seed, f"bench{batch}x{h}x{w}")

    def pair(c):
        left = torch.randn(batch, c, h, w, generator=g)
        right = torch.stack([torch.roll(left[i], -(shifts[i % 3] // 4), dims=-1) for i in range(batch)])
        return left, right + 0.05 * torch.randn(batch, c, h, w, generator=g)

    fl, fr = pair(320)
    cl, cr = pair(32)
    att = torch.randn(batch, 1, 48, h, w, generator=g) * 2
    gt = torch.stack([shifts[i % 3] + torch.randn(4 * h, 4 * w, generator=g) for i in range(batch)]).clamp(0.5, 191)
    used = (gt + 0.5 * torch.randn(batch, 4 * h, 4 * w, generator=g)).clamp(0, 191)
    dq = F.interpolate(used.unsqueeze(1), size=(h, w), mode="bilinear") / 4
    return dict(fl=fl, fr=fr, cl=cl, cr=cr, att=att, gt=gt, used=used, dq=dq)


class NoiseTape:
    """Deterministic replacement for the DDIM loop's random draws (acv_ddim.py:354 'eps' =
    randn_like(img), :360 'fill' = rand_like): the k-th draw of each kind comes from its own
    seeded CPU generator in float64 and is cast to the requested dtype, so the reference
    (patched torch.randn_like / rand_like), the CPU oracle and the HIP path all see the same
    numbers whatever their device."""

    def __init__(self, seed: int):
        self.seed = seed
        self.count = {}

    def __call__(self, kind: str, shape, dtype) -> torch.Tensor:
        """kind 'fill' is uniform [0,1); every other kind ('eps', 'x_T', 'q', ...) is standard normal."""
        k = self.count.get(kind, 0)
        self.count[kind] = k + 1
        g = _gen(self.seed, f"{kind}{k}")
        fn = torch.rand if kind == "fill" else torch.randn
        return fn(tuple(shape), generator=g, dtype=torch.float64).to(dtype)


def toy_update_block(net_list, inp_list, corr=None, flow=None, iter32=True, iter16=True, iter08=True, update=True):
    """Deterministic stand-in for IGEV's ConvGRU update block (KITTI15/core/update.py:104-142, a 2-D module that
    is out of scope): same call signature and return convention, so the reference's and this build's DDIM
    loops can be driven with identical dynamics in the parity fixtures."""
    if not update:
        return net_list
    delta = 0.3 * torch.tanh(corr.mean(dim=1, keepdim=True)) - 0.02 * flow
    return net_list, torch.ones_like(flow), delta


def toy_upsample_disp(flow, up_mask, stem_2x):
    """Stand-in for IGEVStereo_ddim.upsample_disp (:206-214): x4 bilinear upsampling of 4*flow."""
    import torch.nn.functional as F
    return F.interpolate(flow * 4.0, scale_factor=4, mode="bilinear", align_corners=False)


def _stub_stage(cin, cout, stride):
    from torch import nn
    return nn.Sequential(nn.Conv2d(cin, cout, 3, stride, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU6())


class StubMobileNetV2(__import__("torch").nn.Module):
    """Stand-in for ``timm.create_model('mobilenetv2_100', features_only=True)`` (KITTI15/core/extractor.py:331): the
    attributes IGEV's ``Feature`` takes from it -- ``conv_stem`` / ``bn1`` / ``act1`` and seven ``blocks`` with
    MobileNetV2's channel counts and strides (16 @1/2, 24 @1/4, 32 @1/8, 64 + 96 @1/16, 160 @1/32, 320) -- each stage
    one 3x3 conv + BN + ReLU6.  Neither timm nor its pretrained weights exist offline; the goldens and the tests
    drive the reference and this build with this same module (weights from ``synth_state_dict``)."""

    def __init__(self):
        from torch import nn
        super().__init__()
        self.conv_stem = nn.Conv2d(3, 32, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(32)
        self.act1 = nn.ReLU6()
        self.blocks = nn.Sequential(_stub_stage(32, 16, 1), _stub_stage(16, 24, 2), _stub_stage(24, 32, 2),
                                    _stub_stage(32, 64, 2), _stub_stage(64, 96, 1), _stub_stage(96, 160, 2),
                                    _stub_stage(160, 320, 1))


# ---- the recurrent update block as a training workload (tools/make_golden_update_train.py, tests, tools/bench_update_train.py)

UPDATE_TRAIN_ARGS = dict(corr_levels=2, corr_radius=4, n_gru_layers=3, n_downsample=2)
UPDATE_TRAIN_HIDDEN = (128, 128, 128)


def update_train_inputs(seed: int, b: int, h: int, w: int, iters: int, dtype=torch.float32, device="cpu"):
    """Seeded inputs of an unrolled training loop of IGEV's update block at a 1/4 plane of h x w: hidden states ``net``
    (tanh of noise) and context terms ``inp`` (relu of noise) at the three scales -- leaves that require grad --, one
    correlation tensor per iteration (162 channels), the starting disparity, a ground truth and the weights ``m`` of the
    loss's mask-feature term."""
    def rnd(key, *shape):
        return torch.randn(*shape, generator=_gen(seed, key)).to(device=device, dtype=dtype)
    planes = [(h, w)]
    for _ in range(2):
        planes.append(((planes[-1][0] - 1) // 2 + 1, (planes[-1][1] - 1) // 2 + 1))
    cor_planes = UPDATE_TRAIN_ARGS["corr_levels"] * (2 * UPDATE_TRAIN_ARGS["corr_radius"] + 1) * 9
    net = [torch.tanh(rnd(f"net{i}", b, UPDATE_TRAIN_HIDDEN[2 - i], *p)).requires_grad_(True) for i, p in enumerate(planes)]
    inp = [[torch.relu(rnd(f"inp{i}{j}", b, UPDATE_TRAIN_HIDDEN[2 - i], *p)).requires_grad_(True) for j in range(3)]
           for i, p in enumerate(planes)]
    return dict(net=net, inp=inp, corr=[rnd(f"corr{t}", b, cor_planes, h, w) for t in range(iters)],
                disp=rnd("disp", b, 1, h, w).abs() * 4, gt=rnd("gt", b, 1, h, w).abs() * 4 + 1,
                m=rnd("m", b, 32, h, w))


def update_train_loop(block, x, slow_fast: bool = False):
    """The reference's training loop around the update block (KITTI15/core/igev_stereo_ddim.py:441-457: the disparity
    is detached before every call, the hidden states never) with a loss shaped like sequence_loss at 1/4 resolution:
    sum_i 0.9^(T-1-i) mean|disp_i - gt| + 0.1 mean(mask_feat_i * m).  Returns (loss, per-iteration disparities,
    per-iteration mask features, final hidden states)."""
    net, disp = list(x["net"]), x["disp"]
    iters = len(x["corr"])
    loss, disps, masks = 0.0, [], []
    for i in range(iters):
        disp = disp.detach()
        if slow_fast:
            net = block(net, x["inp"], iter16=True, iter08=False, iter04=False, update=False)
            net = block(net, x["inp"], iter16=True, iter08=True, iter04=False, update=False)
        net, mask_feat, delta = block(net, x["inp"], x["corr"][i], disp, iter16=True, iter08=True)
        disp = disp + delta
        loss = loss + 0.9 ** (iters - 1 - i) * (disp - x["gt"]).abs().mean() + 0.1 * (mask_feat * x["m"]).mean()
        disps.append(disp)
        masks.append(mask_feat)
    return loss, disps, masks, net


# ---- IGEV's cost-volume front as a training workload (tools/make_golden_igev_volume_train.py, tests,
# ---- tools/bench_igev_volume_train.py)

IGEV_VOLUME_TRAIN_WEIGHT_SEED = 91
IGEV_VOLUME_TRAIN_CASES = {"even": dict(seed=41, b=2, h=16, w=32, max_disp=64),
                           "tall": dict(seed=42, b=2, h=8, w=24, max_disp=192)}
IGEV_VOLUME_LEAVES = ("match_left", "match_right", "feat0", "feat1", "feat2", "feat3")


def igev_volume_train_inputs(seed: int, b: int, h: int, w: int, max_disp: int, dtype=torch.float32, device="cpu",
                             requires_grad: bool = True, shift: int = 3):
    """Seeded inputs of one training step of IGEV's cost-volume front at a 1/4 plane of h x w: the 96-channel match
    features with a correlation ridge (right = left rolled by ``shift`` plus noise), the left feature pyramid (96 / 64 /
    192 / 160 channels at 1/4 .. 1/32) -- six leaves that require grad unless ``requires_grad=False`` (a frozen
    backbone) --, a ground truth ``gt`` uniform in [0, D-1] and a standard-normal cotangent ``cot`` of the geometry
    volume, D = max_disp / 4."""
    d = max_disp // 4

    def leaf(t):
        return t.to(device=device, dtype=dtype).requires_grad_(requires_grad)
    ml = torch.randn(b, 96, h, w, generator=_gen(seed, "ml"))
    mr = torch.roll(ml, -shift, dims=-1) + 0.1 * torch.randn(b, 96, h, w, generator=_gen(seed, "mr"))
    feats = [torch.randn(b, c, h // s, w // s, generator=_gen(seed, f"feat{i}"))
             for i, (c, s) in enumerate(((96, 1), (64, 2), (192, 4), (160, 8)))]
    gt = torch.rand(b, 1, h, w, generator=_gen(seed, "gt")) * (d - 1)
    cot = torch.randn(b, 8, d, h, w, generator=_gen(seed, "cot"))
    return dict(match_left=leaf(ml), match_right=leaf(mr), features=[leaf(f) for f in feats],
                gt=gt.to(device=device, dtype=dtype), cot=cot.to(device=device, dtype=dtype))


def igev_volume_train_leaves(x):
    """The six leaves of ``igev_volume_train_inputs`` under the names of IGEV_VOLUME_LEAVES."""
    return dict(zip(IGEV_VOLUME_LEAVES, [x["match_left"], x["match_right"], *x["features"]]))


def igev_volume_train_loss(geo: torch.Tensor, init_disp: torch.Tensor, x) -> torch.Tensor:
    """The `init_disp` term of the reference's sequence_loss (KITTI15/train_stereo.py:33-62) at 1/4 resolution plus a
    linear functional of the geometry encoding volume, which stands for the GRU terms that reach the weights through the
    lookup: smooth_l1(init_disp, gt) + mean(geo * cot)."""
    import torch.nn.functional as F
    return F.smooth_l1_loss(init_disp, x["gt"]) + (geo * x["cot"]).mean()


# ---- IGEV's convex-upsampling head as a training workload (tools/make_golden_igev_upsample_train.py, tests,
# ---- tools/bench_upsample_train.py)

IGEV_UPSAMPLE_TRAIN_WEIGHT_SEED = 93
IGEV_UPSAMPLE_TRAIN_CASES = {"even": dict(seed=51, b=2, h=8, w=16, iters=3),
                             "odd": dict(seed=52, b=1, h=5, w=7, iters=2)}
IGEV_UPSAMPLE_LOGIT_HEADS = ("spx_gru.0.weight", "spx.0.weight")       # what ``logit_gain`` of the fixture scales


def igev_upsample_state_dict(template: Mapping[str, torch.Tensor], seed: int, logit_gain: float = 1.0):
    """``synth_state_dict`` for an IGEVUpsampler, the two 9-logit heads scaled by ``logit_gain``."""
    return synth_state_dict(template, seed=seed, scale={k: logit_gain for k in IGEV_UPSAMPLE_LOGIT_HEADS})


def igev_upsample_train_inputs(seed: int, b: int, h: int, w: int, iters: int, dtype=torch.float32, device="cpu",
                               requires_grad: bool = True):
    """Seeded inputs of one training step of IGEV's upsampling head at a 1/4 plane of h x w over ``iters`` GRU
    iterations: per iteration the update block's mask feature (relu of noise, 32 channels) and disparity, once per step
    the 1/2-resolution stem (32 channels), the 1/4-resolution left features (96 channels) and the initial disparity --
    leaves that require grad unless ``requires_grad=False`` -- and a full-resolution ground truth."""
    def rnd(key, *shape):
        return torch.randn(*shape, generator=_gen(seed, key))

    def leaf(t):
        return t.to(device=device, dtype=dtype).requires_grad_(requires_grad)
    return dict(mask_feat_4=[leaf(torch.relu(rnd(f"mask{i}", b, 32, h, w))) for i in range(iters)],
                disp=[leaf(rnd(f"disp{i}", b, 1, h, w).abs() * 4) for i in range(iters)],
                stem_2x=leaf(rnd("stem_2x", b, 32, 2 * h, 2 * w)), feat0=leaf(rnd("feat0", b, 96, h, w)),
                init_disp=leaf(rnd("init_disp", b, 1, h, w).abs() * 4),
                gt=(rnd("gt", b, 1, 4 * h, 4 * w).abs() * 16 + 1).to(device=device, dtype=dtype))


def igev_upsample_train_leaves(x):
    """The leaves of ``igev_upsample_train_inputs`` by name: mask_feat_4_<i>, disp_<i>, stem_2x, feat0, init_disp."""
    out = {}
    for i, (m, d) in enumerate(zip(x["mask_feat_4"], x["disp"])):
        out[f"mask_feat_4_{i}"], out[f"disp_{i}"] = m, d
    out.update(stem_2x=x["stem_2x"], feat0=x["feat0"], init_disp=x["init_disp"])
    return out


def igev_upsample_train_step(model, x):
    """The upsampling side of the reference's training forward (KITTI15/core/igev_stereo_ddim.py:390-393, :456-457, :462)
    on ``model`` -- ``model(disp, mask_feat_4, stem_2x)`` is `upsample_disp`, ``model.init_forward(feat0, stem_2x,
    init_disp)`` the upsampled initial disparity -- with a loss shaped like sequence_loss (KITTI15/train_stereo.py:33-62)
    at full resolution: mean|init_up - gt| + sum_i 0.9^(T-1-i) mean|disp_up_i - gt|.  Returns (loss, init_up, [disp_up_i])."""
    iters = len(x["disp"])
    ups = [model(x["disp"][i], x["mask_feat_4"][i], x["stem_2x"]) for i in range(iters)]
    init_up = model.init_forward(x["feat0"], x["stem_2x"], x["init_disp"])
    loss = (init_up - x["gt"]).abs().mean()
    for i, up in enumerate(ups):
        loss = loss + 0.9 ** (iters - 1 - i) * (up - x["gt"]).abs().mean()
    return loss, init_up, ups


# ---- IGEV's geometry lookup as a training workload (tools/make_golden_igev_lookup_train.py, tests,
# ---- tools/bench_lookup_train.py)

IGEV_LOOKUP_TRAIN_CASES = {"even": dict(seed=71, b=2, c=8, d=48, h=8, w=24, iters=3),
                           "odd": dict(seed=72, b=1, c=8, d=48, h=5, w=7, iters=2)}
IGEV_LOOKUP_LEAVES = ("fmap1", "fmap2", "geo")


def igev_lookup_train_inputs(seed: int, b: int, c: int, d: int, h: int, w: int, iters: int, feat: int = 96,
                             dtype=torch.float32, device="cpu", requires_grad: bool = True):
    """Seeded inputs of one training step of IGEV's geometry lookup at a 1/4 plane of h x w over ``iters`` GRU iterations:
    the geometry encoding volume [b,c,d,h,w] and the two matching-feature maps [b,feat,h,w] -- three leaves that require
    grad unless ``requires_grad=False`` --, the pixel columns ``coords``, and per iteration a disparity (uniform in
    [-3, d+3): both borders are crossed), a noise filter [b,d,h,w] and a standard-normal cotangent of the lookup's
    [b, 2*(9c+9), h, w] output -- none of which requires grad (the reference detaches them)."""
    def rnd(key, *shape):
        return torch.randn(*shape, generator=_gen(seed, key))

    def leaf(t):
        return t.to(device=device, dtype=dtype).requires_grad_(requires_grad)

    def const(t):
        return t.to(device=device, dtype=dtype)
    coords = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w).expand(b, 1, h, w).contiguous()
    return dict(geo=leaf(rnd("geo", b, c, d, h, w)), fmap1=leaf(rnd("fmap1", b, feat, h, w)),
                fmap2=leaf(rnd("fmap2", b, feat, h, w)), coords=const(coords),
                disp=[const(torch.rand(b, 1, h, w, generator=_gen(seed, f"disp{i}")) * (d + 6) - 3) for i in range(iters)],
                noisy=[const(rnd(f"noisy{i}", b, d, h, w)) for i in range(iters)],
                cot=[const(rnd(f"cot{i}", b, 2 * (9 * c + 9), h, w)) for i in range(iters)])


def igev_lookup_train_leaves(x):
    """The three leaves of ``igev_lookup_train_inputs`` under the names of IGEV_LOOKUP_LEAVES."""
    return {n: x[n] for n in IGEV_LOOKUP_LEAVES}


def igev_lookup_train_step(volume_cls, x):
    """The lookup side of the reference's training loop (KITTI15/core/igev_stereo_ddim.py:402, :441-443): one
    ``volume_cls(fmap1, fmap2, geo)`` and T lookups against it, each with its own detached disparity and noise, under a
    loss that is a linear functional of every lookup: sum_t mean(out_t * cot_t).  Returns (loss, [out_t])."""
    vol = volume_cls(x["fmap1"], x["fmap2"], x["geo"])
    outs = [vol(dsp, x["coords"], nz) for dsp, nz in zip(x["disp"], x["noisy"])]
    loss = 0.0
    for out, cot in zip(outs, x["cot"]):
        loss = loss + (out * cot).mean()
    return loss, outs


# ---- IGEV: the 2-D front and the whole training step (tools/make_golden_igev_front_train.py, ..._train_step.py) -------
IGEV_TRAIN_ARGS = dict(hidden_dims=[128, 128, 128], n_gru_layers=3, n_downsample=2, corr_levels=2, corr_radius=4,
                       slow_fast_gru=False, max_disp=192, mixed_precision=False, corr_implementation="reg",
                       shared_backbone=False)
IGEV_TRAIN_WEIGHT_SEED = 55
IGEV_FRONT_TRAIN_CASES = {"b1": dict(seed=109, b=1, h=32, w=64), "b2": dict(seed=426, b=2, h=32, w=64)}
IGEV_FRONT_MODULES = ("feature", "stem_2", "stem_4", "conv", "desc", "cnet", "context_zqr_convs")
IGEV_TRAIN_STEP_CASE = dict(seed=83, b=2, h=64, w=128, iters=3, t=400)


def igev_train_images(seed: int, b: int, h: int, w: int, dtype=torch.float32, device="cpu"):
    """A stereo pair in 0..255: random texture, the right image the left shifted by 6 pixels."""
    img1 = torch.rand(b, 3, h, w, generator=_gen(seed, "image1")) * 255
    return img1.to(device=device, dtype=dtype), torch.roll(img1, -6, dims=-1).to(device=device, dtype=dtype)


def igev_front_flat(out):
    """The outputs of the 2-D front (features_left, stem_2x, match_left, match_right, net_list, inp_list) as one list."""
    features_left, stem_2x, match_left, match_right, net_list, inp_list = out
    return [*features_left, stem_2x, match_left, match_right, *net_list, *(t for trio in inp_list for t in trio)]


def igev_front_train_loss(out, seed: int):
    """sum_i mean(out_i * cot_i) with seeded cotangents over every output of the front: a smooth loss."""
    loss = 0.0
    for i, t in enumerate(igev_front_flat(out)):
        cot = torch.randn(tuple(t.shape), generator=_gen(seed, f"cot{i}")).to(device=t.device, dtype=t.dtype)
        loss = loss + (t * cot).mean()
    return loss


def igev_train_step_inputs(seed: int, b: int, h: int, w: int, iters: int, t: int, dtype=torch.float32, device="cpu"):
    """Images, the full-resolution disparity and its quarter-resolution form, the valid mask, and the fixed draws of the
    train branch: the diffusion step ``t`` [1] and the q_sample noise [B,48,h/4,w/4]."""
    import torch.nn.functional as F
    img1, img2 = igev_train_images(seed, b, h, w, dtype, device)
    g = _gen(seed, "disp")
    flow_full = (6 + torch.randn(b, 1, h, w, generator=g)).clamp(0.5, 47)
    flow_gt = F.interpolate(flow_full, size=(h // 4, w // 4), mode="bilinear") / 4
    valid = (torch.rand(b, h, w, generator=g) > 0.1).float()
    noise = torch.randn(b, 48, h // 4, w // 4, generator=_gen(seed, "noise"))
    return dict(image1=img1, image2=img2, flow_full=flow_full.to(device=device, dtype=dtype),
                flow_gt=flow_gt.to(device=device, dtype=dtype), valid=valid.to(device),
                noise=noise.to(device=device, dtype=dtype), t=torch.tensor([t], dtype=torch.long, device=device),
                iters=iters)


def igev_sequence_loss_inputs(seed: int, b: int = 2, h: int = 16, w: int = 24, n: int = 3, dtype=torch.float32):
    """Seeded arguments of ``sequence_loss``: n predictions and the initial one around a ground truth that has pixels
    beyond max_disp and invalid ones, and errors on both sides of smooth-L1's knee."""
    g = _gen(seed, "sequence_loss")
    gt = torch.rand(b, 1, h, w, generator=g) * 230
    valid = (torch.rand(b, h, w, generator=g) > 0.2).float()
    preds = [(gt + torch.randn(b, 1, h, w, generator=g) * (3.0 / (i + 1))).to(dtype) for i in range(n)]
    init = (gt + torch.randn(b, 1, h, w, generator=g) * 1.5).to(dtype)
    return preds, init, gt.to(dtype), valid


LOSS_TRAIN_CASE = dict(seed=83, b=2, h=16, w=24, k=6)


def loss_train_inputs(seed: int, b: int = 2, h: int = 16, w: int = 24, k: int = 6, dtype=torch.float32):
    """Seeded arguments of the ``model_loss_*`` functions: k predictions [B,H,W] around a ground truth with pixels at 0 (no
    ground truth) and beyond 192, the mask ``(gt < 192) & (gt > 0)`` of the training scripts, errors on both sides of
    smooth-L1's knee, and prediction 0 equal to the ground truth at every 7th pixel (d == 0 exactly) -> (preds, gt, mask)."""
    g = _gen(seed, "loss_train")
    gt = torch.rand(b, h, w, generator=g) * 180 + 1
    bad = torch.rand(b, h, w, generator=g)
    gt[bad < 0.1] = 0.0
    gt[bad > 0.9] = 200.0
    preds = [gt + torch.randn(b, h, w, generator=g) * (2.5 / (i + 1)) for i in range(k)]
    preds[0].view(-1)[::7] = gt.view(-1)[::7]
    mask = (gt < 192) & (gt > 0)
    return [p.to(dtype) for p in preds], gt.to(dtype), mask
