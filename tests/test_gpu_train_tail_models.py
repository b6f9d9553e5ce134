"""ACVNet_DDIM and PWCNet_ddim training steps with their regression heads on the fused HIP tail (DV_TRAIN_TAIL=hip, the
default) and on the torch expression (DV_TRAIN_TAIL=torch), in one process on the fixtures of test_gpu_acv_train.py /
test_gpu_pcw_train.py (whose helpers are copied here: importing those modules would run their fixtures again).

The HIP route's predictions and sampled gradient entries are held to the torch route's with those modules' `within` form,
per tensor:
    rel(hip, f64) <= 2 * rel(torch route, f64) + 1e-6        (f64: the reference's float64 step in the fixture;
                                                              torch route: the worse of two steps, see below)
and both routes give a gradient to the same parameters.

Only the tail may differ between the two steps, so everything else is made to repeat.  MIOpen's default choice for the
stride-2 convolution `feature_extraction.layer5.0.conv1` of PWCNet_ddim does not give the same bits twice, on either
route; from there on the forward of two fresh models differs, and a gradient that is mostly amplified rounding
(`dispupsample.0.0.weight`, behind a BatchNorm over one input channel) lands anywhere within a factor of three.  The steps
therefore run with `torch.backends.cudnn.deterministic = True`, under which every stage output of the forward repeats bit
for bit on both routes.  MIOpen's backward-weights still does not repeat, so the yardstick of a tensor is the worse of two
torch-route steps: the reason test_gpu_acv_train.py gives for not resting a bar on a single float32 evaluation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from diffuvolume_amd import ACVNet_DDIM, PWCNet_ddim, model_loss_kitti12, model_loss_train
from diffuvolume_amd.synth import NoiseTape, _gen, synth_state_dict, synth_stereo_batch

pytestmark = pytest.mark.gpu

MODELS = {
    "acv": ("acv_train_step.npz", lambda: ACVNet_DDIM(192), model_loss_train),
    "pcw": ("pcw_train_step.npz", lambda: PWCNet_ddim(192), model_loss_kitti12),
}


def inputs(gold, which):
    b, h, w = (int(v) for v in gold["shape"])
    seed = int(gold["input_seed"])
    x = synth_stereo_batch(b, h, w, seed=seed)
    gt = x["gt"].clone()
    bad = torch.rand(b, h, w, generator=_gen(seed, "train_gt_invalid"))
    gt[bad < 0.05] = 0.0
    gt[bad > 0.97] = 200.0
    disp = x["disp"]
    if which == "pcw":                      # quarter-resolution disp_net (KITTI12/main.py:148-150)
        disp = F.interpolate(torch.clamp(gt, 0, 191).unsqueeze(1), size=(h // 4, w // 4), mode="bilinear") / 4
    return [t.cuda() for t in (x["left"], x["right"], disp, gt)]


def step(which, gold, route):
    """A fresh model's forward + loss + backward with the fixture's timestep and q_sample noise on the given tail route."""
    _, make, loss_fn = MODELS[which]
    model = make()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=int(gold["weight_seed"])), strict=True)
    model = model.cuda().train()
    left, right, disp, gt = inputs(gold, which)
    tape = NoiseTape(int(gold["tape_seed"]))
    t = int(gold["t_step"])
    real_randint = torch.randint
    with pytest.MonkeyPatch.context() as m:
        m.setenv("DV_TRAIN_TAIL", route)
        m.setattr(torch.backends.cudnn, "deterministic", True)     # MIOpen: algorithms whose bits repeat (see above)
        m.setattr(torch, "randint", lambda low, high, size, *a, device=None, **k:
                  real_randint(t, t + 1, size, device=device))
        m.setattr(torch, "randn_like", lambda x, *a, **k: tape("q", tuple(x.shape), x.dtype).to(x.device))
        outs = model(left, right, None, disp, None)
        loss = loss_fn(outs, gt, (gt < 192) & (gt > 0))
        loss.backward()
    torch.cuda.synchronize()
    return model, [o.detach() for o in outs]


def rel(a, ref):
    a, ref = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, ref))
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


@pytest.mark.parametrize("which", ["acv", "pcw"])
def test_hip_tail_trains_like_the_torch_expression(which):
    with np.load(GOLDEN / MODELS[which][0]) as z:
        gold = {k: z[k] for k in z.files}
    hip_model, hip_outs = step(which, gold, "hip")
    refs = [step(which, gold, "torch") for _ in range(2)]
    pix = torch.from_numpy(gold["pix_idx"]).cuda()

    def ratio(hip, yardsticks, f64):
        """The `within` form as a number: rel(hip, f64) over its bar 2 * (the worse yardstick's rel) + 1e-6."""
        return rel(hip, f64) / (2 * max(rel(y, f64) for y in yardsticks) + 1e-6)

    rows = []
    for i, a in enumerate(hip_outs):
        ys = [outs[i] for _, outs in refs]
        assert len(refs[0][1]) == len(hip_outs) and all(y.shape == a.shape for y in ys)
        rows.append((ratio(a.reshape(-1)[pix].cpu().numpy(), [y.reshape(-1)[pix].cpu().numpy() for y in ys],
                           gold[f"pred{i}_f64"]), f"pred{i}"))
    hip_p = dict(hip_model.named_parameters())
    ref_ps = [dict(m.named_parameters()) for m, _ in refs]
    for name in hip_p:
        for ref_p in ref_ps:
            assert (hip_p[name].grad is None) == (ref_p[name].grad is None), name
    for j, name in enumerate(gold["grad_names"]):
        idx = torch.from_numpy(gold["grad_idx"][j]).cuda()
        a = hip_p[str(name)].grad.reshape(-1)[idx].cpu().numpy()
        ys = [ref_p[str(name)].grad.reshape(-1)[idx].cpu().numpy() for ref_p in ref_ps]
        rows.append((ratio(a, ys, gold["grad_val_f64"][j]), str(name)))
    rows.sort(reverse=True)
    print(f"{which}: largest ratios of an error to its bar:", [(round(r, 3), n) for r, n in rows[:6]])
    over = [(round(r, 3), n) for r, n in rows if not r <= 1.0]
    assert not over, f"{len(over)} of {len(rows)} tensors over the bar: {over[:20]}"
