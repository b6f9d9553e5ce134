"""Both feature CNNs and ACVNet_DDIM's `concatconv` alone in train mode, forward + backward, on the HIP route of
diffuvolume_amd/train_net2d.py (DV_TRAIN_NET2D=hip) and on the nn.Modules (DV_TRAIN_NET2D=torch).

Shapes: B = 2; 3 x 32 x 64 images for ACV, 3 x 64 x 128 for PCW (its 1/32 scale needs multiples of 32; BatchNorm needs
more than one value per channel there), [2,320,8,16] features for `concatconv`.  One fixed random cotangent per output.

Reference: a deep copy of the same nn.Modules in float64 on the CPU, called stack by stack.  Yardstick: the torch route on
the GPU in float32, the worse of two runs.  Bar per kind of tensor (outputs, input gradient, convolution-weight gradients,
BatchNorm weight / bias gradients, running statistics), as tests/test_gpu_acv_train.py's `Bar`:
    rel(hip) <= 2 * worst float32 error of the kind + 1e-6.
Per network the module runs the reference once, two steps on `hip` and two on `torch`; every test reads those."""
import copy

import pytest
import torch
from torch import nn

from diffuvolume_amd import ACVNet_DDIM, acv_ddim, pwcnet_ddim, train_net2d
from diffuvolume_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

FNS = ("ConvCatFnBackward", "BatchNormActFnBackward")


def rel(a, ref):
    a, ref = a.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((a - ref).norm() / max(float(ref.norm()), 1e-30))


def graph_names(outs):
    seen, stack = set(), [o.grad_fn for o in outs.values()]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        stack.extend(g for g, _ in f.next_functions)
    return {f.name() for f in seen}


class Net:
    """One of the three networks: the CPU master module, its input and how each route calls it."""

    def __init__(self, which):
        self.which = which
        gen = torch.Generator().manual_seed({"acv": 11, "pcw": 12, "concat": 13}[which])
        if which == "acv":
            self.master, self.owner_of = acv_ddim.FeatureExtraction(), lambda m: m
            self.x = torch.rand(2, 3, 32, 64, generator=gen)
        elif which == "pcw":
            self.master, self.owner_of = pwcnet_ddim.FeatureExtraction(True, 12), lambda m: m
            self.x = torch.rand(2, 3, 64, 128, generator=gen)
        else:
            self.master, self.owner_of = ACVNet_DDIM(192), lambda m: m
            self.x = torch.randn(2, 320, 8, 16, generator=gen)
        self.master.load_state_dict(synth_state_dict(self.master.state_dict(), seed=5), strict=True)
        self.master.train()
        self.cot = None

    def net_of(self, model):
        return model.concatconv if self.which == "concat" else model

    def modules_forward(self, net, x):
        """The nn.Modules stack by stack (what the float64 reference runs)."""
        if self.which == "concat":
            return {"concat": net(x)}
        if self.which == "pcw":
            return net._forward_modules(x)
        x = net.layer1(net.firstconv(x))
        l2 = net.layer2(x)
        l3 = net.layer3(l2)
        l4 = net.layer4(l3)
        return {"gwc_feature": torch.cat((l2, l3, l4), dim=1)}

    def route_forward(self, model, x):
        """What the models' train_forward runs on the route of DV_TRAIN_NET2D."""
        if self.which != "concat":
            return model(x)
        if train_net2d.route() == "hip":
            return {"concat": train_net2d.Net2d(model, ("concatconv.",)).seq(model.concatconv, x)}
        return {"concat": model.concatconv(x)}

    def cotangents(self, outs):
        if self.cot is None:
            gen = torch.Generator().manual_seed(77)
            self.cot = {k: torch.randn(v.shape, generator=gen) for k, v in sorted(outs.items())}
        return self.cot

    def collect(self, net, outs, x):
        params = dict(net.named_parameters())
        kinds = {}
        bn = {f"{n}.{k}" for n, m in net.named_modules() if isinstance(m, nn.BatchNorm2d) for k in ("weight", "bias")}
        for n, p in params.items():
            kinds[n] = "bn_grad" if n in bn else "wgrad"
        return dict(outs={k: v.detach() for k, v in outs.items()},
                    dx=None if x.grad is None else x.grad.detach(),
                    grads={n: (None if p.grad is None else p.grad.detach().clone()) for n, p in params.items()},
                    bufs={n: b.detach().clone() for n, b in net.named_buffers()}, kinds=kinds)

    def reference(self, prepare=None):
        model = copy.deepcopy(self.master).double()
        if prepare:
            prepare(self.net_of(model))
        net = self.net_of(model)
        x = self.x.double().requires_grad_(self.which == "concat")
        outs = self.modules_forward(net, x)
        cot = self.cotangents(outs)
        sum((outs[k] * cot[k].double()).sum() for k in outs).backward()
        return self.collect(net, outs, x)

    def run(self, route, prepare=None):
        model = copy.deepcopy(self.master).cuda().train()
        if prepare:
            prepare(self.net_of(model))
        net = self.net_of(model)
        x = self.x.cuda().requires_grad_(self.which == "concat")
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("DV_TRAIN_NET2D", route)
            for k in ("DV_TRAIN_NORM", "DV_TRAIN_CONV2D"):
                mp.delenv(k, raising=False)
            outs = self.route_forward(model, x)
            names = graph_names(outs)
            cot = self.cotangents(outs)
            sum((outs[k] * cot[k].cuda()).sum() for k in outs).backward()
            torch.cuda.synchronize()
        r = self.collect(net, outs, x)
        r["names"] = names
        return r


def rows(run, ref):
    """(kind, name, relative error against the float64 run) for every tensor the step leaves."""
    out = [("out", k, rel(v, ref["outs"][k])) for k, v in run["outs"].items()]
    if ref["dx"] is not None:
        out.append(("dx", "x", rel(run["dx"], ref["dx"])))
    for n, g in ref["grads"].items():
        if g is not None:
            out.append((ref["kinds"][n], n, rel(run["grads"][n], g)))
    for n, b in ref["bufs"].items():
        if not n.endswith("num_batches_tracked"):
            out.append(("stats", n, rel(run["bufs"][n], b)))
    return out


def hold(hip, yard_runs, ref, what):
    yard = [r for run in yard_runs for r in rows(run, ref)]
    bound = {k: 2 * max(e for kk, _, e in yard if kk == k) + 1e-6 for k in {k for k, _, _ in yard}}
    mine = rows(hip, ref)
    worst = {k: max(e for kk, _, e in mine if kk == k) for k in bound}
    print(f"{what}: worst hip error / bar per kind:", {k: (f"{worst[k]:.3g}", f"{bound[k]:.3g}") for k in sorted(bound)})
    bad = sorted(((e / bound[k], k, n) for k, n, e in mine if not e <= bound[k]), reverse=True)
    assert not bad, f"{what}: {len(bad)} of {len(mine)} tensors over the bar {bound}: {bad[:20]}"


@pytest.fixture(scope="module", params=["acv", "pcw", "concat"])
def runs(request):
    net = Net(request.param)
    ref = net.reference()
    return net, ref, {"hip": net.run("hip"), "hip2": net.run("hip"), "torch": net.run("torch"), "torch2": net.run("torch")}


def test_every_kind_holds_the_float32_bar(runs):
    net, ref, r = runs
    assert all(g is not None for n, g in ref["grads"].items() if net.which != "concat")
    for name in ("hip", "hip2"):
        assert sorted(n for n, g in r[name]["grads"].items() if g is not None) == \
            sorted(n for n, g in ref["grads"].items() if g is not None)
        hold(r[name], (r["torch"], r["torch2"]), ref, f"{net.which} {name}")


def test_batches_are_counted_as_on_the_torch_route(runs):
    _, _, r = runs
    tracked = {n: int(v) for n, v in r["hip"]["bufs"].items() if n.endswith("num_batches_tracked")}
    assert tracked and tracked == {n: int(v) for n, v in r["torch"]["bufs"].items() if n.endswith("num_batches_tracked")}


def test_two_hip_runs_give_the_same_bits(runs):
    net, _, r = runs
    a, b = r["hip"], r["hip2"]
    assert all(torch.equal(a["outs"][k], b["outs"][k]) for k in a["outs"])
    assert a["dx"] is None or torch.equal(a["dx"], b["dx"])
    differ = [n for n, g in a["grads"].items() if g is not None and not torch.equal(g, b["grads"][n])]
    assert not differ, f"{net.which}: {len(differ)} gradients differ: {differ[:10]}"
    assert all(torch.equal(v, b["bufs"][n]) for n, v in a["bufs"].items())


def test_the_functions_are_in_the_graph_on_hip_and_not_on_torch(runs):
    _, _, r = runs
    for fn in FNS:
        assert fn in r["hip"]["names"] and fn in r["hip2"]["names"], fn
        assert fn not in r["torch"]["names"], fn
    assert not any("ConvolutionBackward" in n or "NativeBatchNorm" in n or "CudnnBatchNorm" in n or "MiopenBatchNorm" in n
                   for n in r["hip"]["names"]), sorted(r["hip"]["names"])


FROZEN = {"acv": ("firstconv.0.0.weight", "firstconv.0.1.weight", "firstconv.0.1.bias", "layer2.1.conv1.0.0.weight",
                  "layer2.1.conv1.0.1.weight", "layer3.0.conv2.1.bias", "layer4.1.conv2.0.weight"),
          "pcw": ("firstconv.0.0.weight", "layer5.0.conv1.0.0.weight", "layer5.0.downsample.0.weight", "gw3.2.weight",
                  "layer_refine.2.1.weight"),
          "concat": ("0.0.weight", "2.weight")}


def test_frozen_parameters_get_no_gradient_and_leave_the_other_bits(runs):
    net, _, r = runs
    frozen = FROZEN[net.which]

    def freeze(m):
        params = dict(m.named_parameters())
        for n in frozen:
            params[n].requires_grad_(False)
    got = net.run("hip", freeze)
    for n, g in got["grads"].items():
        if n in frozen:
            assert g is None, n
        elif r["hip"]["grads"][n] is not None:
            assert g is not None and torch.equal(g, r["hip"]["grads"][n]), n
    assert all(torch.equal(got["outs"][k], r["hip"]["outs"][k]) for k in got["outs"])
    assert got["dx"] is None or torch.equal(got["dx"], r["hip"]["dx"])


def test_plans_are_packed_once_per_weight_state_and_follow_data_parallel_replicas(monkeypatch):
    """The packed convolution plans live in the owner's "net2d" slot under a key of the convolution weights alone: a second
    call (the right image; BatchNorm has rewritten its buffers in between) finds them, an in-place write to a weight
    rebuilds them, and a DataParallel replica -- whose weights are broadcast copies, not parameters -- builds its own and
    gives the module's bits, with the gradients arriving on the source's parameters."""
    monkeypatch.setenv("DV_TRAIN_NET2D", "hip")
    net = Net("acv")
    model = copy.deepcopy(net.master).cuda().train()
    x = net.x.cuda()
    cot = None

    def fwd_bwd(m):
        nonlocal cot
        y = m(x)["gwc_feature"]
        cot = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).cuda() if cot is None else cot
        for p in model.parameters():
            p.grad = None
        y.backward(cot)
        return y.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}

    twin = copy.deepcopy(model)
    y0, g0 = fwd_bwd(model)
    p0 = model.plans(train_net2d.SLOT)
    assert len(p0[1]) == 46
    fwd_bwd(model)
    assert model.plans(train_net2d.SLOT) is p0                     # buffers changed, weights did not
    with torch.no_grad():
        model.layer3[0].conv1[0][0].weight.mul_(1.0)
    fwd_bwd(model)
    assert model.plans(train_net2d.SLOT) is not p0                 # a weight was written in place
    replica = torch.nn.parallel.replicate(twin, [0])[0]
    assert replica is not twin and not list(replica.parameters())
    model = twin                                                     # the replica's gradients arrive on its source
    y1, g1 = fwd_bwd(replica)
    assert torch.equal(y0, y1)
    assert sorted(g0) == sorted(g1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    assert twin.__dict__["_replica_plans"] and twin.__dict__.get("_plan_slots", {}).get(train_net2d.SLOT) is None


EVAL_BN = {"acv": "layer2.2.conv2.1", "pcw": "layer7.1.conv1.0.1", "concat": "0.1"}


def test_a_batchnorm_in_eval_mode_keeps_the_statement(runs):
    net, _, r = runs
    name = EVAL_BN[net.which]

    def to_eval(m):
        m.get_submodule(name).eval()
    ref = net.reference(to_eval)
    hip, yard = net.run("hip", to_eval), net.run("torch", to_eval)
    hold(hip, (yard,), ref, f"{net.which} with {name} in eval mode")
    before = dict(net.net_of(net.master).named_buffers())
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        assert torch.equal(hip["bufs"][f"{name}.{k}"].cpu(), before[f"{name}.{k}"]), k
    assert any("BatchNorm" in n and "BatchNormActFn" not in n for n in hip["names"]), sorted(hip["names"])
