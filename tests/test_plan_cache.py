"""submodule.PlanCache on toy modules: when plans are built, kept, dropped and shared with nn.DataParallel replicas."""
import torch
from torch import nn

from diffuvolume_amd.submodule import PlanCache


class Toy(PlanCache, nn.Module):
    def __init__(self, child=None):
        super().__init__()
        self.lin = nn.Linear(3, 3)
        self.bn = nn.BatchNorm1d(3)
        if child is not None:
            self.child = child
        self.builds = []

    def _build_plans(self, slot):
        self.builds.append(slot)
        return object()


def test_built_once_and_kept_across_eval_calls():
    m = Toy().eval()
    p = m.plans()
    assert m.plans() is p and m.prepare() is p and m.prepare(check_weights=True) is p and m._plans is p
    m.eval()
    assert m.plans() is p and m.builds == [None]


def test_train_toggle_drops_the_plans():
    m = Toy().eval()
    p = m.plans()
    m.train()
    m.eval()
    assert m._plans is None and m.plans() is not p and len(m.builds) == 2


def test_load_state_dict_drops_the_plans_directly_and_through_a_wrapper():
    m = Toy().eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    p = m.plans()
    m.load_state_dict(sd)
    q = m.plans()
    assert q is not p
    nn.DataParallel(m).load_state_dict({"module." + k: v for k, v in sd.items()})
    assert m.plans() is not q and len(m.builds) == 3


def test_to_dtype_drops_the_plans():
    m = Toy().eval()
    p = m.plans()
    m.to(torch.float64)
    assert m.plans() is not p


def test_in_place_write_is_noticed_by_refresh_only():
    m = Toy().eval()
    p = m.plans()
    with torch.no_grad():
        m.lin.weight.copy_(torch.randn(3, 3))
    assert m.plans() is p                      # a plain lookup does not look at the weights
    m.refresh_plans()
    assert m.plans() is not p and len(m.builds) == 2


def test_data_swap_is_noticed_by_refresh():
    m = Toy().eval()
    p = m.plans()
    other = torch.randn(3, 3)
    m.lin.weight.data = other                  # leaves _version alone: the storage address changes
    m.refresh_plans()
    assert m.plans() is not p


def test_refresh_without_a_change_keeps_the_plans():
    m = Toy(child=Toy()).eval()
    p, c = m.plans(), m.child.plans()
    m.refresh_plans()
    assert m.plans() is p and m.child.plans() is c


def test_parent_refresh_drops_the_plans_of_its_subtree():
    m = Toy(child=Toy()).eval()
    p, c = m.plans(), m.child.plans()
    with torch.no_grad():
        m.child.bn.running_mean.add_(1.0)
    m.refresh_plans()
    assert m.plans() is not p and m.child.plans() is not c


def test_slots_are_independent():
    m = Toy().eval()
    a, b = m.plans(), m.plans("f16")
    assert a is not b and m.plans() is a and m.plans("f16") is b and m.builds == [None, "f16"]
    m.train()
    m.eval()
    assert m.plans("f16") is not b


def test_replicas_reuse_the_plans_parked_on_the_source(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)      # what nn.DataParallel sets around each replica
    src = Toy().eval()
    s = src.plans()
    r1 = src._replicate_for_data_parallel()
    assert r1._plans is None and src._plans is s       # the replica does not share the source's cache
    p1 = r1.plans()
    assert p1 is not s
    r2 = src._replicate_for_data_parallel()
    assert r2.plans() is p1 and src.builds == [None, None]
    assert r2._replicate_for_data_parallel().plans() is p1       # a replica of a replica parks on the first source
    with torch.no_grad():
        src.lin.bias.add_(1.0)                 # new weights on the source: the parked plans are stale
    assert src._replicate_for_data_parallel().plans() is not p1
