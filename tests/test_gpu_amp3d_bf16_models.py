"""ACVNet_DDIM and PWCNet_ddim at train precision "bf16" (``set_train_precision(torch.bfloat16)``), one training step at
the shapes of tests/golden/acv_train_step.npz / pcw_train_step.npz, on the harness of tests/test_gpu_amp3d_models.py (its
``Fixed``, ``run``, ``class_errors`` and ``same_bits`` are used as they are): every step runs with ``DV_TRAIN_NET2D=hip``
and every other ``DV_TRAIN_*`` switch at its default, the setting under which a step of either model repeats bit for bit.

Accuracy.  The reference for mixed precision is what a reference user gets from autocast: the same step with
``DV_TRAIN_CONV3D=torch``, where the 3x3x3 stride-1 layers run ``F.conv3d`` under a real
``torch.autocast("cuda", dtype=torch.bfloat16)`` (operands AND results rounded to bf16).  Per tensor class -- predictions,
weights, biases and BatchNorm statistics, all four asserted -- the largest relative L2 error of the HIP route's ONE step
against the fixture's float64 values is at most twice that of the autocast route's ONE step: the project's standing
"twice the reference's own error" bar.  Gradients of whole models are badly conditioned in float32 already (the fp16 run
shows 1.5e-1 on weights) and bf16 has three bits less, which is why the bar is relative to the autocast route.
Measured (relative L2 against float64, HIP route / autocast route):
    ACVNet_DDIM   pred 2.06e-2 / 2.67e-2   weights 5.42e-1 / 4.38e-1   biases 3.98e-1 / 4.89e-1   bn 1.56e-3 / 1.96e-3
    PWCNet_ddim   pred 2.62e-2 / 3.44e-2   weights 3.64e-1 / 3.56e-1   biases 2.44e-1 / 3.81e-1   bn 9.08e-4 / 1.14e-3
(0.64 .. 1.24 of the autocast route's; about eight times the "f16" figures, as three bits less make it.)

Bits.  Two "bf16" steps repeat in the loss, every output and all 291 / 452 gradients; an "f32" step after a round trip
through "bf16" has the bits of a fresh model's; two threads training two replicas at "f16" and "bf16" get the bits of
their serial runs.

No GradScaler.  Three SGD steps at "bf16" on a loss multiplied by 2^20 (a scale at which fp16 operands would overflow)
with the learning rate divided by the same factor: every gradient of every step is finite, the largest gradient entry of
every step lies beyond 65504 (measured 1.7e6 .. 1.2e8: the scale does what it is there for) and the weights change."""
import threading

import numpy as np
import pytest
import torch

import test_gpu_acv_train as ACV
import test_gpu_pcw_train as PCW
from conftest import GOLDEN
from diffuvolume_amd.synth import NoiseTape
from test_gpu_amp3d_models import MODELS, Fixed, _local, class_errors, run, same_bits

pytestmark = pytest.mark.gpu


def bf16_model(T, gold):
    m = T.fresh_model(gold).set_train_precision(torch.bfloat16)
    assert m.train_precision == "bf16"
    return m


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
            out["f32"] = run(T, gold, T.fresh_model(gold))
            out["f32_again"] = run(T, gold, T.fresh_model(gold))
            out["bf16"] = run(T, gold, bf16_model(T, gold))
            out["bf16_again"] = run(T, gold, bf16_model(T, gold))
            out["f16"] = run(T, gold, T.fresh_model(gold).set_train_precision(torch.float16))
            back = bf16_model(T, gold).set_train_precision(torch.float32)
            assert back.train_precision == "f32"
            out["f32_round_trip"] = run(T, gold, back)
            mp.setenv("DV_TRAIN_CONV3D", "torch")
            out["torch_bf16"] = run(T, gold, bf16_model(T, gold))
            mp.delenv("DV_TRAIN_CONV3D")
    finally:
        mp.undo()
    return out


def repeating(S):
    """(True, every output's index, every gradient's name), after asserting that two "f32" steps from one state repeat
    in all of them: the yardstick of the comparisons below has to be whole."""
    (la, oa, ga, _), (lb, ob, gb, _) = S["f32"], S["f32_again"]
    assert torch.equal(la, lb) and all(torch.equal(x, y) for x, y in zip(oa, ob))
    names = [n for n in ga if torch.equal(ga[n], gb[n])]
    assert len(names) == len(ga) == {"acv": 291, "pcw": 452}[S["name"]], (len(names), len(ga))
    return True, list(range(len(oa))), names


def test_bf16_step_within_twice_the_autocast_routes_error(S):
    gold = S["gold"]
    hip, ref = class_errors(gold, *S["bf16"]), class_errors(gold, *S["torch_bf16"])
    assert sorted(hip) == sorted(ref) == ["biases", "bn", "pred", "weights"]
    for c in sorted(hip):
        print(f"AMP3DBF16 {S['name']} {c}: HIP bf16 route {hip[c]:.3e}, torch autocast route {ref[c]:.3e} (relative L2 against float64)")
    for c in hip:
        assert hip[c] <= 2 * ref[c], (c, hip[c], ref[c])
    # the bf16 route is another computation than the f32 and the f16 ones
    assert not torch.equal(S["bf16"][0], S["f32"][0]) and not torch.equal(S["bf16"][0], S["f16"][0])


def test_two_bf16_steps_repeat(S):
    same_bits(S["bf16"], S["bf16_again"], repeating(S))


def test_f32_after_a_round_trip_through_bf16_has_a_fresh_models_bits(S):
    same_bits(S["f32"], S["f32_round_trip"], repeating(S))


def test_two_threads_at_f16_and_bf16_match_their_serial_runs(S):
    T, gold = S["T"], S["gold"]
    models = {"f16": T.fresh_model(gold).set_train_precision(torch.float16), "bf16": bf16_model(T, gold)}
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
    same_bits(S["f16"], got["f16"], names)
    same_bits(S["bf16"], got["bf16"], names)


def test_three_steps_without_a_grad_scaler_on_a_loss_scaled_by_2_to_the_20(S):
    T, gold = S["T"], S["gold"]
    scale = 2.0 ** 20
    model = bf16_model(T, gold)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = torch.optim.SGD(model.parameters(), lr=1e-2 / scale)
    left, right, disp, gt = T.inputs(gold)
    loss_fn = ACV.model_loss_train if T is ACV else PCW.model_loss_kitti12
    with Fixed(gold):
        for step in range(3):
            _local.tape = NoiseTape(int(gold["tape_seed"]))
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(model(left, right, None, disp, None), gt, (gt < 192) & (gt > 0)) * scale
            loss.backward()
            grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
            assert len(grads) == {"acv": 291, "pcw": 452}[S["name"]]
            nonfinite = [n for n, g in grads.items() if not torch.isfinite(g).all()]
            assert torch.isfinite(loss) and not nonfinite, (step, nonfinite[:5])
            big = max(float(g.abs().max()) for g in grads.values())
            print(f"AMP3DBF16 {S['name']} step {step}: scaled loss {float(loss.detach()):.4e}, largest |gradient| {big:.3e}")
            assert big > 65504                                     # what fp16 cannot hold passes through here
            opt.step()
        torch.cuda.synchronize()
    changed = [n for n, p in model.named_parameters() if n in grads and not torch.equal(p.detach(), before[n])]
    assert len(changed) > len(grads) // 2, (len(changed), len(grads))
    assert all(torch.isfinite(p).all() for p in model.parameters())
