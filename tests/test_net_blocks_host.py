"""diffuvolume_amd/net_blocks.py without a GPU: the walk over every Sequential shape the ACV and PCW models contain computes
what the modules compute, and puts into each BatchNorm statement exactly what the table below says.

DV_TRAIN_CONV3D=torch and DV_TRAIN_CONV2D=torch and modules in eval(): every statement is a PyTorch one, CPU tensors are
legal, and a BatchNorm is deterministic (running statistics), so the comparisons are `torch.equal`."""
import pytest
import torch
from torch import nn

ACTIVATIONS = ("relu", "mish")


@pytest.fixture(autouse=True)
def torch_routes(monkeypatch):
    monkeypatch.setenv("DV_TRAIN_CONV3D", "torch")
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")


def _shapes(member):
    """name -> (module, input, skip) for one instance of every Sequential shape of the two models at 8 channels; `member`
    is the activation of the container's own members."""
    from diffuvolume_amd import net_blocks as nb
    torch.manual_seed(7)
    a = lambda: nb.act_module(member)
    x3, x2 = torch.randn(1, 8, 4, 4, 8), torch.randn(1, 8, 4, 8)
    s3, s2, up = torch.randn(1, 8, 4, 4, 8), torch.randn(1, 8, 4, 8), torch.randn(1, 8, 8, 8, 16)
    cb3, cb2 = (lambda: nb.cb3(8, 8, 3, 1, 1)), (lambda: nb.cb2(8, 8, 3, 1, 1, 1))
    shapes = {
        "cb3-act": (nn.Sequential(cb3(), a()), x3, s3),
        "cb3-act-cb3-act": (nn.Sequential(cb3(), a(), cb3(), a()), x3, s3),
        "cb3-act-cb3": (nn.Sequential(cb3(), a(), cb3()), x3, s3),
        "cb3-act-conv3d": (nn.Sequential(cb3(), a(), nn.Conv3d(8, 8, 3, 1, 1, bias=False)), x3, s3),
        "deconv-bn3d": (nn.Sequential(nn.ConvTranspose3d(8, 8, 3, padding=1, output_padding=1, stride=2, bias=False),
                                      nn.BatchNorm3d(8)), x3, up),
        "redir": (nb.cb3(8, 8, 1, 1, 0), x3, s3),
        "cb2-act": (nn.Sequential(cb2(), a()), x2, s2),
        "head2d": (nb.head2d(8, 8, 8, member), x2, s2),
        "layer_refine": (nn.Sequential(cb2(), a(), nb.cb2(8, 8, 1, 1, 0, 1), a()), x2, s2),
        "conv2d": (nn.Conv2d(8, 8, 3, 1, 1, bias=False), x2, s2),
    }
    for mod, _, _ in shapes.values():
        _randomise(mod)
    return shapes


def _blocks(member):
    """A BasicBlock without and with `downsample` (8 -> 8 and 8 -> 16 channels, stride 1)."""
    from diffuvolume_amd import net_blocks as nb
    torch.manual_seed(8)
    blocks = {"block": nb.stack(8, 8, 1, 1, 1, 1, member)[0], "block-downsample": nb.stack(8, 16, 1, 1, 1, 1, member)[0]}
    assert blocks["block"].downsample is None and blocks["block-downsample"].downsample is not None
    for blk in blocks.values():
        _randomise(blk)
    return blocks, torch.randn(1, 8, 4, 8)


def _randomise(mod):
    """Running statistics and affine parameters away from the identity, then eval()."""
    for m in mod.modules():
        if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
            m.running_mean.normal_(0, 0.5)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.5)
    mod.eval()


def _batchnorms(mod):
    return [m for m in mod.modules() if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d))]


@pytest.mark.parametrize("member", ACTIVATIONS)
def test_the_walk_computes_what_the_modules_compute(member):
    from diffuvolume_amd.net_blocks import walk
    from diffuvolume_amd.train_norm import act_statement
    with torch.no_grad():
        for name, (mod, x, skip) in _shapes(member).items():
            y = mod(x)
            assert torch.equal(walk(mod, x), y), name
            for act in ACTIVATIONS:
                assert torch.equal(walk(mod, x, act, skip), act_statement(y + skip, act)), (name, act)
            assert torch.equal(walk(mod, x, "none", skip), y + skip), name
    with pytest.raises(ValueError):
        walk(nn.Identity(), torch.zeros(1), "gelu")


# (index of the BatchNorm in modules() order, activation in its statement, skip in its statement); M = the members' own
# activation, A = the caller's.  "alone": the call without `act` and `skip`; "caller": with both.
M, A = "M", "A"
STATEMENTS = {
    # an activation that is the last leaf is not fused when the caller passed an act or a skip: BatchNorm alone, the
    # activation module, + skip, act
    "cb3-act": {"alone": [(0, M, False)], "caller": [(0, "none", False)]},
    "cb3-act-cb3-act": {"alone": [(0, M, False), (1, M, False)], "caller": [(0, M, False), (1, "none", False)]},
    # a BatchNorm that is the last leaf takes the caller's skip and act
    "cb3-act-cb3": {"alone": [(0, M, False), (1, "none", False)], "caller": [(0, M, False), (1, A, True)]},
    "cb3-act-conv3d": {"alone": [(0, M, False)], "caller": [(0, M, False)]},
    "deconv-bn3d": {"alone": [(0, "none", False)], "caller": [(0, A, True)]},
    "redir": {"alone": [(0, "none", False)], "caller": [(0, A, True)]},
    "cb2-act": {"alone": [(0, M, False)], "caller": [(0, "none", False)]},
    "head2d": {"alone": [(0, M, False)], "caller": [(0, M, False)]},
    "layer_refine": {"alone": [(0, M, False), (1, M, False)], "caller": [(0, M, False), (1, "none", False)]},
    "conv2d": {"alone": [], "caller": []},
}
# Net2d.block: downsample first (no activation, no skip), conv1 with its activation, conv2 with the block's skip
BLOCK_STATEMENTS = {"block": [(0, M, False), (1, "none", True)],
                    "block-downsample": [(2, "none", False), (0, M, False), (1, "none", True)]}


def _recorder(monkeypatch, log):
    """`bn_act` / `bn_act2d` replaced by a function that notes the statement and computes it in PyTorch."""
    from diffuvolume_amd import net_blocks, train_net2d
    from diffuvolume_amd.train_norm import act_statement

    def record(bn, x, act, skip=None):
        log.append((bn, act, skip is not None))
        return act_statement(bn(x), act, skip)
    monkeypatch.setattr(net_blocks, "bn_act", record)
    monkeypatch.setattr(train_net2d, "bn_act2d", record)


def _named(log, mod, member, caller):
    index = {id(m): i for i, m in enumerate(_batchnorms(mod))}
    name = {member: M, caller: A}
    return [(index[id(bn)], name.get(a, a), s) for bn, a, s in log]


@pytest.mark.parametrize("member,caller", [("relu", "mish"), ("mish", "relu")])
def test_what_rides_in_each_batchnorm_statement(monkeypatch, member, caller):
    """`member` and `caller` differ, so the table can tell the members' activation from the caller's."""
    from diffuvolume_amd import train2d, train_net2d
    from diffuvolume_amd.net_blocks import walk
    log = []
    _recorder(monkeypatch, log)
    monkeypatch.setenv("DV_TRAIN_NET2D", "hip")
    with torch.no_grad():
        for name, (mod, x, skip) in _shapes(member).items():
            for how, args in (("alone", ()), ("caller", (caller, skip))):
                del log[:]
                walk(mod, x, *args, conv2d=train2d.conv2d_module, bn2d=train_net2d.bn_act2d)
                assert _named(log, mod, member, caller) == STATEMENTS[name][how], (name, how)
        blocks, x = _blocks(member)
        n = train_net2d.Net2d(conv2d=train2d.conv2d_module)
        for name, blk in blocks.items():
            del log[:]
            n.block(blk, x)
            assert _named(log, blk, member, caller) == BLOCK_STATEMENTS[name], name


@pytest.mark.parametrize("member", ACTIVATIONS)
def test_a_basic_blocks_batchnorm2d_goes_to_bn_act2d_only_on_the_hip_route(monkeypatch, member):
    """refinenet3's statement, `Net2d(conv2d=train2d.conv2d_module).block`: under DV_TRAIN_NET2D=hip every BatchNorm2d
    goes to `bn_act2d`, under torch to the module's own forward; both compute the block."""
    from diffuvolume_amd import train2d, train_net2d
    blocks, x = _blocks(member)
    with torch.no_grad():
        want = {name: blk(x) for name, blk in blocks.items()}
        for route in ("hip", "torch"):                                   # the functions as they are (eval: the statement)
            monkeypatch.setenv("DV_TRAIN_NET2D", route)
            n = train_net2d.Net2d(conv2d=train2d.conv2d_module)
            for name, blk in blocks.items():
                assert torch.equal(n.block(blk, x), want[name]), (route, name)
        log, called = [], []
        _recorder(monkeypatch, log)
        for blk in blocks.values():
            for bn in _batchnorms(blk):
                bn.register_forward_hook(lambda m, i, o: called.append(m))
        for route in ("hip", "torch"):
            monkeypatch.setenv("DV_TRAIN_NET2D", route)
            n = train_net2d.Net2d(conv2d=train2d.conv2d_module)
            for name, blk in blocks.items():
                del log[:], called[:]
                assert torch.equal(n.block(blk, x), want[name]), (route, name)
                bns = _batchnorms(blk)
                assert len(called) == len(bns)                           # (the recorder calls the module too)
                assert len(log) == (len(bns) if route == "hip" else 0), (route, name)


def test_one_activation_statement_and_one_batchnorm_body():
    import torch.nn.functional as F
    from diffuvolume_amd import net_blocks, train_net2d, train_norm
    y, s = torch.randn(2, 3, 4), torch.randn(2, 3, 4)
    assert torch.equal(train_norm.act_statement(y, "none"), y)
    assert torch.equal(train_norm.act_statement(y, "relu", s), F.relu(y + s))
    assert torch.equal(train_norm.act_statement(y, "mish", s), (y + s) * torch.tanh(F.softplus(y + s)))
    assert torch.equal(net_blocks.Mish()(y), train_norm.act_statement(y, "mish"))
    with pytest.raises(ValueError):
        train_norm.act_statement(y, "gelu")
    assert net_blocks.act_of(net_blocks.Mish()) == "mish" and net_blocks.act_of(nn.ReLU()) == "relu"
    assert net_blocks.act_of(nn.Tanh()) is None
    # the two call sites differ in the rank they take into the kernel's case and in nothing else
    x4 = torch.randn(2, 3, 4, 5)
    for fn, rank in ((train_norm.bn_act, 5), (train_net2d.bn_act2d, 4)):
        bn, twin = nn.BatchNorm2d(3).eval(), nn.BatchNorm2d(3).eval()
        assert torch.equal(fn(bn, x4, "relu", x4), train_norm.bn_act_rank(rank, twin, x4, "relu", x4))
