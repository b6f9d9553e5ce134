"""ACVNet_DDIM and PWCNet_ddim at train precision "f16" (``set_train_precision``), one training step at the shapes of
tests/golden/acv_train_step.npz / pcw_train_step.npz (the weights, inputs and draws of tests/test_gpu_acv_train.py and
tests/test_gpu_pcw_train.py, whose helpers are used as they are).

Every step here runs with ``DV_TRAIN_NET2D=hip`` and every other ``DV_TRAIN_*`` switch at its default, the setting under
which a step of either model repeats bit for bit everywhere (tests/test_gpu_net2d_train_models.py).  At the default
``DV_TRAIN_NET2D=torch`` the 2-D networks run on the nn.Modules, where convolution algorithms and atomics are MIOpen's and
ATen's choice: PWCNet_ddim's feature extraction (``feature_extraction.layer5`` onwards) then differs from run to run, and
behind fp16 roundings that spread moved the worst BatchNorm statistic (``dispupsample.0.1.running_var``, downstream of the
predictions) between 1.5e-4 and 3.3e-4 from step to step -- a single-step comparison of the two routes was a draw.  Pinned,
both routes see the same 2-D bits and each figure below is one step.

Accuracy.  The reference for mixed precision is what a reference user gets from autocast: the same step with
``DV_TRAIN_CONV3D=torch``, where the 3x3x3 stride-1 layers run ``F.conv3d`` under a real ``torch.autocast`` (operands AND
results rounded to fp16).  Per tensor class -- predictions (the loss and the sampled pixels of every output), weights
(sampled gradient entries of the parameters with more than one dimension), biases (those of the 1-D parameters) and
BatchNorm statistics -- the largest relative L2 error of the HIP route's ONE step against the fixture's float64 values is
at most twice that of the autocast route's ONE step: the project's "twice the reference's own error" bar
(tests/test_gpu_acv_train.py: the worst tensor of a kind against twice the reference's worst tensor of that kind).
Measured (relative L2 against float64, HIP route / autocast route):
    ACVNet_DDIM   pred 2.59e-3 / 3.37e-3   weights 1.49e-1 / 1.96e-1   biases 1.74e-1 / 1.74e-1   bn 2.30e-4 / 2.68e-4
    PWCNet_ddim   pred 3.55e-3 / 4.59e-3   weights 5.35e-2 / 5.84e-2   biases 6.38e-2 / 5.99e-2   bn 1.36e-4 / 1.86e-4

Bits.  Two "f32" steps from one state repeat in the loss, every output and every gradient (asserted: the yardstick has
to be whole); two "f16" steps then repeat in all of them too; a "f32" step after a round trip through "f16" has the bits
of a fresh model's; two threads training two replicas at different precisions get the bits of their serial runs; a
GradScaler step whose scale overflows the fp16 operands is skipped and leaves the weights as they were."""
import threading

import numpy as np
import pytest
import torch

import test_gpu_acv_train as ACV
import test_gpu_pcw_train as PCW
from conftest import GOLDEN
from diffuvolume_amd import _env
from diffuvolume_amd.synth import NoiseTape

pytestmark = pytest.mark.gpu

MODELS = {"acv": (ACV, "acv_train_step.npz"), "pcw": (PCW, "pcw_train_step.npz")}
_local = threading.local()


class Fixed:
    """The fixture's timestep and q_sample noise for every thread at once: torch.randint / torch.randn_like are patched
    for the whole block (the helpers' own ``step`` patches and restores around one call, which two threads would race
    on); each ``run`` starts a noise tape of its own.  And the switches of the module docstring: DV_TRAIN_NET2D=hip, every
    other DV_TRAIN_* at its default (the fixture below moves DV_TRAIN_CONV3D inside the block)."""

    def __init__(self, gold):
        self.gold, self.mp = gold, pytest.MonkeyPatch()

    def __enter__(self):
        t, real = int(self.gold["t_step"]), torch.randint
        for k in _env.KNOBS:
            if k.startswith("DV_TRAIN_"):
                self.mp.delenv(k, raising=False)
        self.mp.setenv("DV_TRAIN_NET2D", "hip")
        self.mp.setattr(torch, "randint", lambda low, high, size, *a, device=None, **k: real(t, t + 1, size, device=device))
        self.mp.setattr(torch, "randn_like", lambda x, *a, **k: _local.tape("q", tuple(x.shape), x.dtype).to(x.device))
        return self

    def __exit__(self, *exc):
        self.mp.undo()


def run(T, gold, model):
    """One step under ``Fixed``: (loss, outputs, gradients by name, BatchNorm statistics by name)."""
    left, right, disp, gt = T.inputs(gold)
    _local.tape = NoiseTape(int(gold["tape_seed"]))
    model.zero_grad(set_to_none=True)
    outs = model(left, right, None, disp, None)
    loss_fn = ACV.model_loss_train if T is ACV else PCW.model_loss_kitti12
    loss = loss_fn(outs, gt, (gt < 192) & (gt > 0))
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    bufs = {str(n): dict(model.named_buffers())[str(n)].clone() for n in gold["bn_names"]}
    return loss.detach().clone(), [o.detach().clone() for o in outs], grads, bufs


def class_errors(gold, loss, outs, grads, bufs):
    """tensor class -> largest relative L2 error against the fixture's float64 values."""
    rows = {"pred": [T_rel(float(loss), gold["loss_f64"])], "weights": [], "biases": [], "bn": []}
    pix = torch.from_numpy(gold["pix_idx"]).cuda()
    for i, p in enumerate(outs):
        rows["pred"].append(T_rel(p.reshape(-1)[pix].cpu().numpy(), gold[f"pred{i}_f64"]))
    for j, name in enumerate(gold["grad_names"]):
        g = grads[str(name)]
        kind = "weights" if g.dim() > 1 else "biases"
        rows[kind].append(T_rel(g.reshape(-1)[torch.from_numpy(gold["grad_idx"][j]).cuda()].cpu().numpy(), gold["grad_val_f64"][j]))
    for j, name in enumerate(gold["bn_names"]):
        v = bufs[str(name)].reshape(-1)[torch.from_numpy(gold["bn_idx"][j]).cuda()].cpu().numpy()
        rows["bn"].append(T_rel(v, gold["bn_val_f64"][j]))
    return {k: max(v) for k, v in rows.items()}


def T_rel(a, ref):
    return ACV.rel(a, ref)


@pytest.fixture(scope="module", params=sorted(MODELS))
def S(request):
    """Every step the tests below compare, run once per model."""
    T, fname = MODELS[request.param]
    with np.load(GOLDEN / fname) as z:
        gold = {k: z[k] for k in z.files}
    mp = pytest.MonkeyPatch()
    out = {"T": T, "gold": gold, "name": request.param}
    try:
        with Fixed(gold):
            m32 = T.fresh_model(gold)
            assert m32.train_precision == "f32"
            out["f32"] = run(T, gold, m32)
            out["f32_again"] = run(T, gold, T.fresh_model(gold))
            m16 = T.fresh_model(gold).set_train_precision("f16")
            assert m16.train_precision == "f16"
            out["f16"] = run(T, gold, m16)
            out["f16_again"] = run(T, gold, T.fresh_model(gold).set_train_precision("f16"))
            back = T.fresh_model(gold).set_train_precision("f16").set_train_precision("f32")
            out["f32_round_trip"] = run(T, gold, back)
            mp.setenv("DV_TRAIN_CONV3D", "torch")
            out["torch16"] = run(T, gold, T.fresh_model(gold).set_train_precision("f16"))
            mp.delenv("DV_TRAIN_CONV3D")
    finally:
        mp.undo()
    return out


def repeating(S):
    """What two "f32" steps from one state repeat bit for bit: (the loss?, the outputs' indices, the gradients' names) --
    with the 2-D networks on the HIP route that is the loss, every output and every gradient of both models, and this
    asserts it, so that nothing is dropped from the comparisons below."""
    (la, oa, ga, _), (lb, ob, gb, _) = S["f32"], S["f32_again"]
    loss = torch.equal(la, lb)
    outs = [i for i, (x, y) in enumerate(zip(oa, ob)) if torch.equal(x, y)]
    names = [n for n in ga if torch.equal(ga[n], gb[n])]
    print(f"AMP3D {S['name']}: repeats at f32: loss {loss}, outputs {outs} of {len(oa)}, {len(names)} of {len(ga)} gradients")
    assert loss and len(outs) == len(oa), (loss, outs)
    assert len(names) == len(ga) == {"acv": 291, "pcw": 452}[S["name"]], (len(names), len(ga))
    return loss, outs, names


def same_bits(a, b, what):
    loss, outs, names = what
    assert loss and torch.equal(a[0], b[0])
    for i in outs:
        assert torch.equal(a[1][i], b[1][i]), f"output {i}"
    assert sorted(a[2]) == sorted(b[2]) == sorted(names)
    for n in names:
        assert torch.equal(a[2][n], b[2][n]), n


def test_f16_step_within_twice_the_autocast_routes_error(S):
    """One step of each route (see the module docstring for why a single step is a fair draw here)."""
    gold = S["gold"]
    hip, ref = class_errors(gold, *S["f16"]), class_errors(gold, *S["torch16"])
    for c in sorted(hip):
        print(f"AMP3D {S['name']} {c}: HIP f16 route {hip[c]:.3e}, torch autocast route {ref[c]:.3e} (relative L2 against float64)")
    for c in hip:
        assert hip[c] <= 2 * ref[c], (c, hip[c], ref[c])
    # the f16 route is another computation than the f32 one
    assert not torch.equal(S["f16"][0], S["f32"][0])


def test_two_f16_steps_repeat_where_f32_repeats(S):
    same_bits(S["f16"], S["f16_again"], repeating(S))


def test_f32_after_a_round_trip_through_f16_has_a_fresh_models_bits(S):
    same_bits(S["f32"], S["f32_round_trip"], repeating(S))


def test_two_threads_at_different_precisions_match_their_serial_runs(S):
    T, gold = S["T"], S["gold"]
    models = {"f32": T.fresh_model(gold), "f16": T.fresh_model(gold).set_train_precision("f16")}
    got, errors = {}, []
    barrier = threading.Barrier(2)

    def work(precision):
        try:
            barrier.wait(timeout=60)
            got[precision] = run(T, gold, models[precision])
        except BaseException as e:                               # noqa: BLE001 (reported by the asserting thread)
            errors.append((precision, e))

    with Fixed(gold):
        threads = [threading.Thread(target=work, args=(p,)) for p in models]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors, errors
    names = repeating(S)
    same_bits(S["f32"], got["f32"], names)
    same_bits(S["f16"], got["f16"], names)


def test_grad_scaler_skips_a_step_whose_scale_overflows(S):
    T, gold = S["T"], S["gold"]
    model = T.fresh_model(gold).set_train_precision("f16")
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    left, right, disp, gt = T.inputs(gold)
    with Fixed(gold):
        _local.tape = NoiseTape(int(gold["tape_seed"]))
        outs = model(left, right, None, disp, None)
        loss = (ACV.model_loss_train if T is ACV else PCW.model_loss_kitti12)(outs, gt, (gt < 192) & (gt > 0))
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        torch.cuda.synchronize()
    assert scaler.get_scale() < 2.0 ** 40                         # the scaler saw Inf / NaN and backed off
    nonfinite = [n for n, p in model.named_parameters() if p.grad is not None and not torch.isfinite(p.grad).all()]
    assert nonfinite
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
