"""Pin the SceneFlow oracle to the IMPORTED REFERENCE's outputs on the conditioned network (oracle/calibrate.py,
oracle/make_golden_acv_conditioned.py), at the contract's raw bars, and show that the network is well conditioned on the
fixtures -- which is what entitles tests/test_gpu_acv_conditioned.py to hold the HIP path to those bars."""
import pytest
import torch

from conftest import load_golden
from oracle import acv_oracle as O
from oracle import calibrate as C
from oracle import loop_parity as LP

FIXTURES = ["acv_conditioned_16x32", "acv_conditioned_24x32_b2"]


def _epe(disp, used):
    return float((disp - used).abs().mean())


@pytest.mark.parametrize("name", FIXTURES)
def test_conditioned_network_at_the_raw_bars(name):
    """Step 1 (model_predictions at t = 999) and every step of the 5-step loop of the fp32 oracle against the reference's
    own outputs: |d disp| <= 1e-3 px on 99.9 % of the pixels, |d EPE| < 1e-4.  Then the conditioning check of the
    generator, repeated: the reference's step 1 and every step of the oracle's trajectory within 1e-3 px of a float64
    evaluation of the oracle on EVERY pixel, with no renewal decision differing between fp32 and float64."""
    g = load_golden(name)
    sd = C.conditioned_acv_state_dict(g)
    x = C.conditioned_acv_inputs(g["batch"], g["h"], g["w"], g["seed"])
    vol, used = x["vol"], g["used"]
    assert torch.equal(x["used"], used)
    orc = O.ACVDiffusionOracle(sd)
    assert torch.equal(orc.encode_x_T(x["dq"]), g["x_T"])
    bar = max(LP.BAR_FRAC, 1.0 / g["disp"].numel())
    pn, xs, disp, prob = orc.model_predictions(vol, g["x_T"], g["t"])
    d = (disp - g["disp"]).abs()
    assert float((d > LP.BAR_PX).float().mean()) <= bar and float(d.mean()) < 1e-4, (float(d.mean()), float(d.max()))
    assert abs(_epe(disp, used) - _epe(g["disp"], used)) < LP.BAR_EPE
    assert float((O.disparity_uncertainty(disp, prob) - g["unc"]).abs().mean()) < 1e-3
    same = ((xs - g["x_start"]).abs() < 1e-3).all(dim=1)
    assert float(same.float().mean()) > 0.99
    sel = same.unsqueeze(1).expand_as(pn)
    torch.testing.assert_close(pn[sel], g["pred_noise"][sel], atol=1e-6, rtol=0)

    gate = C.acv_float64_gate(sd, vol, used, g["x_T"], g["tape_seed"])
    print(f"{name}: fp32 oracle vs float64 per step {gate['max_px']} px, flips {gate['flips']}")
    stack = gate["stack32"]
    assert stack.shape == g["stack"].shape and torch.equal(stack[0], used)
    for i in range(1, stack.shape[0]):
        di = (stack[i] - g["stack"][i]).abs()
        assert float((di > LP.BAR_PX).float().mean()) <= bar, (i, float(di.mean()), float(di.max()))
        assert abs(_epe(stack[i], used) - _epe(g["stack"][i], used)) < LP.BAR_EPE, i
    df = (gate["final32"] - g["final"]).abs()
    assert float((df > LP.BAR_PX).float().mean()) <= bar, (float(df.mean()), float(df.max()))
    # conditioning: every pixel of every step within 1e-3 px of float64, the reference's own step 1 too
    assert float((g["disp"].double() - gate["disp64"]).abs().max()) < LP.BAR_PX
    assert max(gate["max_px"]) < LP.BAR_PX and gate["final_max_px"] < LP.BAR_PX, gate["max_px"]
    assert gate["flips"] == 0
