"""Every export of the C ABI is either a row of the arena table (tests/test_gpu_abi_arena.py) or excluded here for a stated
reason, so that a new entry point cannot arrive without a decision about its pointer and bounds contract."""
from diffuvolume_amd import _lib
import test_gpu_abi_arena as T
from test_gpu_abi_arena import TABLE

SIZE_OR_CHOICE = "only returns a size, a version, a string or a choice: launches nothing"
PACKS = "only packs weights (its output is the `wpacked` operand of a row, produced through this call)"
HOOK = "process-wide test hook: launches nothing"


def TRAINED(test):
    return f"training entry whose misaligned-view test already exists: {test}"


EXCLUDED = {
    "dv_version": SIZE_OR_CHOICE,
    "dv_error_string": SIZE_OR_CHOICE,
    "dv_pointwise_expand_packed_floats": SIZE_OR_CHOICE,
    "dv_conv3d_packed_floats": SIZE_OR_CHOICE,
    "dv_conv3d_f16x3_packed_bytes": SIZE_OR_CHOICE,
    "dv_conv3d_wino_packed_floats": SIZE_OR_CHOICE,
    "dv_conv3d_wino3_packed_floats": SIZE_OR_CHOICE,
    "dv_conv3d_wino3_supported": SIZE_OR_CHOICE,
    "dv_conv3d_s2pp_supported": SIZE_OR_CHOICE,
    "dv_conv3d_s2pp_packed_floats": SIZE_OR_CHOICE,
    "dv_deconv3d_packed_floats": SIZE_OR_CHOICE,
    "dv_deconv3d_pl_supported": SIZE_OR_CHOICE,
    "dv_deconv3d_k4_packed_floats": SIZE_OR_CHOICE,
    "dv_conv2d_packed_floats": SIZE_OR_CHOICE,
    "dv_conv2d_auto_kslices": SIZE_OR_CHOICE,
    "dv_conv2d_wino_packed_floats": SIZE_OR_CHOICE,
    "dv_conv2d_wino_auto_kslices": SIZE_OR_CHOICE,
    "dv_conv2d_f16_packed_bytes": SIZE_OR_CHOICE,
    "dv_conv2d_f16_auto_kslices": SIZE_OR_CHOICE,
    "dv_geo_lookup_conv1x1_packed_floats": SIZE_OR_CHOICE,
    "dv_conv3d_wgrad_workspace_floats": SIZE_OR_CHOICE,
    "dv_deconv3d_k4s2_dgrad_packed_floats": SIZE_OR_CHOICE,
    "dv_deconv3d_k4s2_wgrad_workspace_floats": SIZE_OR_CHOICE,
    "dv_feature_gate_bwd_workspace_floats": SIZE_OR_CHOICE,
    "dv_conv2d_wgrad_workspace_floats": SIZE_OR_CHOICE,
    "dv_conv2d_wgrad_cat_workspace_floats": SIZE_OR_CHOICE,
    "dv_conv2d_wgrad_cat_f16_workspace_floats": SIZE_OR_CHOICE,
    "dv_deconv2d_k4s2_wgrad_workspace_floats": SIZE_OR_CHOICE,
    "dv_conv2d_fewin_wgrad_workspace_floats": SIZE_OR_CHOICE,
    "dv_pointwise_expand_pack_weights_f32": PACKS,
    "dv_conv3d_pack_weights_f32": PACKS,
    "dv_conv3d_f16x3_pack_weights": PACKS,
    "dv_conv3d_wino_pack_weights_f32": PACKS,
    "dv_conv3d_wino3_pack_weights_f32": PACKS,
    "dv_conv3d_s2pp_pack_weights_f32": PACKS,
    "dv_deconv3d_pack_weights_f32": PACKS,
    "dv_deconv3d_k4_pack_weights_f32": PACKS,
    "dv_conv2d_pack_weights_f32": PACKS,
    "dv_conv2d_wino_pack_weights_f32": PACKS,
    "dv_conv2d_f16_pack_weights": PACKS,
    "dv_geo_lookup_conv1x1_pack_weights_f32": PACKS,
    "dv_deconv3d_k4s2_dgrad_pack_weights_f32": PACKS,
    "dv_conv3d_set_s2_tile": HOOK,
    "dv_conv3d_set_c1z": HOOK,
    "dv_deconv3d_set_impl": HOOK,
    "dv_deconv3d_pl_set_max_blocks": HOOK,
    "dv_allpairs_corr_bwd_f32": TRAINED("test_gpu_allpairs_corr_bwd.py::test_gradients_writes_and_repeatability"),
    "dv_geo_filter_lookup_bwd_f32": TRAINED("test_gpu_geo_lookup_bwd.py::test_abi_writes_every_element_once_and_reproducibly"),
    "dv_deconv3d_k4s2_dgrad_f32": TRAINED("test_gpu_deconv3d_k4_bwd.py::test_misaligned_pointers_take_the_scalar_path"),
    "dv_gru_reset_mul_f32": TRAINED("test_gpu_update_train.py::test_gate_kernels_tails_and_misaligned_views"),
    "dv_gru_blend_f32": TRAINED("test_gpu_update_train.py::test_gate_kernels_tails_and_misaligned_views"),
    "dv_gru_gates_bwd_blend_f32": TRAINED("test_gpu_update_train.py::test_gate_kernels_tails_and_misaligned_views"),
    "dv_gru_gates_bwd_reset_f32": TRAINED("test_gpu_update_train.py::test_gate_kernels_tails_and_misaligned_views"),
    "dv_gru_reset_mul_f16": TRAINED("test_gpu_conv2d_wgrad_cat_f16.py::test_gate_kernels_match_torch_half_arithmetic"),
    "dv_gru_blend_f16": TRAINED("test_gpu_conv2d_wgrad_cat_f16.py::test_gate_kernels_match_torch_half_arithmetic"),
}


def test_every_export_is_a_row_or_an_exclusion():
    rows = {r.entry for r in TABLE}
    names = set(_lib.SIGNATURES)
    assert not rows - names, f"rows that name no export: {sorted(rows - names)}"
    assert not set(EXCLUDED) - names, f"exclusions that name no export: {sorted(set(EXCLUDED) - names)}"
    both = rows & set(EXCLUDED)
    assert not both, f"both a row and an exclusion: {sorted(both)}"
    missing = names - rows - set(EXCLUDED)
    assert not missing, ("exports with no decision: add a row to tests/test_gpu_abi_arena.py or an exclusion with its reason "
                         f"here: {sorted(missing)}")
    assert all(isinstance(v, str) and len(v) > 20 for v in EXCLUDED.values())


def test_no_weight_gradient_entry_is_excluded():
    assert not [n for n in EXCLUDED if "wgrad" in n and not n.endswith("_workspace_floats")]
    assert {n for n in _lib.SIGNATURES if "wgrad" in n and not n.endswith("_workspace_floats")} == set(T.WGRAD_REQUIRED)


def test_weight_gradient_rows_meet_their_shape_conditions():
    """The rows of a weight-gradient entry are there for stated shape conditions (channel tails, a second channel tile,
    plane tails, one split, a ragged split range, ...): every builder holds its own from the size entry -- which needs no
    GPU, so the rows are built here -- and between them the rows of an entry state all the entry asks for.  The pairs a
    row declares bit-equal must be placements the harness really runs and accepts."""
    from diffuvolume_amd import _build
    _build.build()
    met = {entry: set() for entry in T.WGRAD_REQUIRED}
    for r in TABLE:
        if r.entry not in T.WGRAD_REQUIRED:
            continue
        case = r.build()                                   # asserts r.build.claims
        met[r.entry] |= set(r.build.claims)
        assert set(case.outs) == ({"dw"} if r.entry == "dv_conv2d_1in_wgrad_f32" else {"dw", "workspace"}), r.name
        assert set(case.ref) == {"dw"} and not case.inout, r.name
        accepted = {label for label, _, want in T.variants_of(r, case) if want == T.OK}
        refused = {label for label, _, want in T.variants_of(r, case) if want != T.OK}
        assert accepted - {"a"} == {y for x, y in r.same_bits if x == "a"}, (r.name, sorted(accepted))
        assert bool(refused) == bool(r.refuse), r.name
    for entry, need in T.WGRAD_REQUIRED.items():
        assert need <= met[entry], (entry, sorted(need - met[entry]))


def test_the_named_tests_exist():
    """An exclusion that leans on another test names it: the file must exist and define that test."""
    from pathlib import Path
    here = Path(__file__).resolve().parent
    for name, reason in EXCLUDED.items():
        if "already exists: " in reason:
            fname, test = reason.split("already exists: ")[1].split("::")
            assert f"def {test}(" in (here / fname).read_text(), (name, reason)


def test_rows_cite_the_test_their_bar_comes_from():
    from pathlib import Path
    text = "".join(p.read_text() for p in Path(__file__).resolve().parent.glob("test_*.py"))
    for r in TABLE:
        assert r.cite, r.name
        if r.cite.startswith("test_"):
            assert f"def {r.cite}(" in text, (r.name, r.cite)
        assert set(r.variants) <= set("abc") and "a" in r.variants and "c" in r.variants, r.name
