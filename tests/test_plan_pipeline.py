"""The plan-time pipeline decision, case by case.

`choose_pipeline` (csrc/aa_model.hip) decides in one place which pipeline a model runs -- the tensor-product path, the
linear-layer path, the weight folds, the fused forward, the widened sizes -- from the configuration and the plan options
alone; `aa_model_plan_create_with_options` carries the decision out as the blob layout.  Each case of the table below is a
model configuration (built the way `allegro_amd.nn` builds it) plus options and names what it must get.  Plans only: no
weights, no graph, no step, so the same table runs on the CPU emulation build and on the GPU build.  Per case:
  * the whole `aa_model_plan_describe` dictionary is the recorded one, and agrees with the named pipeline
    as far as the dictionary shows it (it cannot tell the three per-edge tensor-product paths apart; the layout hash can);
  * `aa_model_plan_layout_hash`, `aa_model_weights_bytes` and the workspace size of a small force step are the recorded ones
    (the hash mixes the channel-minor flag, the chain pair, the operator chain and every blob offset; the workspace shows
    `embed_fused`), the hash is non-zero, and a second plan from the same inputs gives the same three numbers.
The expected values were recorded from the library of the commit BEFORE the selector was gathered into `choose_pipeline`
(that commit's emulation build, the same inputs), not from the code under test: the refactor must not move a decision.
The last test checks the table itself: every describe key takes both of its values, every option the selector reads is
toggled, and every tensor-product path x linear-layer path of DESIGN.md's table is reached."""
import ctypes as C
import json

import pytest
import torch

from allegro_amd import _lib
from allegro_amd.nn import HipAllegroModel

KEYS = ["fused_forward", "fold_embed_table", "fold_embed_output", "fold_latent_outputs", "fold_lat0_reverse", "fused_mfma_steps_executed",
        "fused_mfma_steps_reference", "chain_gemm", "moments", "operator_path", "slot_form", "fused_wide"]
COUNTS = ("fused_mfma_steps_executed", "fused_mfma_steps_reference")
# the tensor-product path x linear-layer path combinations that can occur
PIPELINES = {"general/single", "spec/single", "spec_chain/single", "moments/single", "moments/chains", "operator/single", "operator/slot",
             "operator/chains"}
OPTIONS = {"tp_generic": 1, "tp_no_chain": 1, "tp_no_moments": 1, "tp_no_operator": 1, "tp_force_operator": 1, "tp_prefer_moments": 1,
           "gemm_no_chain": 1, "gemm_fp32_mfma": 1, "gemm_valu": 1, "no_slot_form": 1, "op_proj_gemm": 2, "embed_no_fuse": 1,
           "fused_forward": 3, "fused_narrow": 1, "no_channel_padding": 1}
# BASELINE config C2 / C3 / C4: l_max 2, 2 layers, u = S = 64, every MLP one hidden layer of 64, one species, fp32
BASE = dict(type_names=["Si"], r_max=5.0, l_max=2, parity=True, num_layers=2, num_scalar_features=64, num_tensor_features=64,
            radial_chemical_embed=dict(_target_="allegro.nn.TwoBodyBesselScalarEmbed", num_bessels=8), radial_chemical_embed_dim=64,
            scalar_embed_mlp_hidden_layers_depth=1, scalar_embed_mlp_hidden_layers_width=64, allegro_mlp_hidden_layers_depth=1,
            allegro_mlp_hidden_layers_width=64, readout_mlp_hidden_layers_depth=1, readout_mlp_hidden_layers_width=64,
            avg_num_neighbors=28.0, tp_path_channel_coupling=True, seed=456)
W128 = dict(scalar_embed_mlp_hidden_layers_width=128, allegro_mlp_hidden_layers_width=128, readout_mlp_hidden_layers_width=128)
S128 = dict(num_scalar_features=128, radial_chemical_embed_dim=128, **W128)
C5 = dict(type_names=["O", "H"], l_max=3, num_layers=3, num_tensor_features=128, model_dtype="float64", **S128)
F64 = dict(model_dtype="float64")
MISH = dict(allegro_mlp_nonlinearity="mish")
SPLINE = dict(radial_chemical_embed=dict(_target_="allegro.nn.TwoBodySplineScalarEmbed", num_splines=16, spline_span=12))
# (name, model constructor overrides, plan options,
#  pipeline, describe values in KEYS order, layout hash, weight bytes, workspace bytes of a 64-atom / 1792-edge force step)
CASES = [
    # BASELINE configurations in their model dtypes
    ("c1", dict(l_max=1, num_tensor_features=32), {},
     "moments/chains", "1 1 1 1 1 22 30 1 1 0 0 1", 0xf2b8465cceee7a45, 2491648, 12333056),
    ("c1_one_layer", dict(l_max=1, num_tensor_features=32, num_layers=1), {},
     "spec/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0x49f1364d885a1c95, 1093632, 8929280),
    ("c1_f64", dict(l_max=1, num_tensor_features=32, **F64), {},
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0xe71513b6f6281af4, 7744000, 25415680),
    ("c2_c3_c4", {}, {},
     "moments/chains", "1 1 1 1 1 24 32 1 1 0 0 1", 0x1c500ed149be09ee, 2755840, 13557760),
    ("c5", C5, {},
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0xc083f9a8619aefb6, 56579072, 82694144),
    # the shapes the selector's comments name
    ("f32_u64_S128", S128, {},
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0x0d7306088ebb3ac6, 13215232, 23205888),
    ("f32_u64_S128_prefer_moments", S128, dict(tp_prefer_moments=1),
     "moments/single", "0 0 0 0 0 0 0 0 1 0 0 0", 0xc554c224d26c0c29, 6596096, 21749760),
    ("f64_u64_S64", F64, {},
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0x6cf8a1125c910775, 9091584, 29011968),
    ("f64_u64_S64_prefer_moments", F64, dict(tp_prefer_moments=1),
     "moments/single", "0 0 0 0 0 0 0 0 1 0 0 0", 0x59e63ee6e98e1628, 4078080, 26947584),
    ("f64_u64_S128", dict(S128, **F64), {},
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0xbda9b625ff1f995f, 26430464, 46374912),
    ("f32_S64_latents128", dict(allegro_mlp_hidden_layers_width=128), {},
     "moments/single", "0 0 0 0 0 0 0 0 1 0 0 0", 0xa6c32924c514741c, 2940160, 15327232),
    ("f32_S64_latents128_force_operator", dict(allegro_mlp_hidden_layers_width=128), dict(tp_force_operator=1),
     "operator/single", "0 0 0 0 0 0 0 0 1 1 0 0", 0xf5b946e8ec52bf96, 3972352, 16718848),
    ("f64_lmax3_u64", dict(l_max=3, **F64), {},
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0x6e78eb0ccf91b40d, 10441728, 34230272),
    ("f64_lmax3_u8_three_layers", dict(l_max=3, num_layers=3, num_tensor_features=8, **F64), {},
     "general/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0x721ec6cb301df79b, 4412416, 35098624),
    ("f64_lmax3_u64_no_operator", dict(l_max=3, **F64), dict(tp_no_operator=1),
     "general/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0x4248c5454cdfac6f, 5755904, 68636672),
    ("three_layers", dict(num_layers=3), {},
     "operator/chains", "0 0 0 0 0 0 0 1 1 1 0 0", 0x5483ef89798b83ab, 4063232, 18307072),
    ("three_layers_no_operator", dict(num_layers=3), dict(tp_no_operator=1),
     "spec/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0x22d4720ac3519a42, 3567616, 48569344),
    ("three_layers_u128", dict(num_layers=3, num_tensor_features=128), {},
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0xa2a4f4553d478168, 9408768, 26204160),
    ("deep_latents", dict(allegro_mlp_hidden_layers_depth=2), {},
     "moments/single", "0 0 0 0 0 0 0 0 1 0 0 0", 0xed92f2410d90a40a, 2268416, 14868480),
    # channel padding and hidden-width padding
    ("u32", dict(num_tensor_features=32), {},
     "moments/chains", "1 1 1 1 1 24 32 1 1 0 0 1", 0x654ce5be13551a8e, 2755840, 13557760),
    ("u32_no_padding", dict(num_tensor_features=32), dict(no_channel_padding=1),
     "spec_chain/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0x4bee213cbbd494de, 1898240, 12656640),
    ("u96", dict(num_tensor_features=96), {},
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0xd407ff71bfe0918e, 7023360, 20208640),
    ("u96_no_padding", dict(num_tensor_features=96), dict(no_channel_padding=1),
     "general/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0x6c12eb0e84388f15, 3163392, 33925120),
    ("u16_S32", dict(num_tensor_features=16, num_scalar_features=32, radial_chemical_embed_dim=32), {},
     "spec_chain/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0xc8c1b12bf0d68fa4, 896768, 8110080),
    ("readout32", dict(readout_mlp_hidden_layers_width=32), {},
     "moments/chains", "1 1 1 1 1 24 32 1 1 0 0 1", 0x1c500ed149be09ee, 2755840, 13557760),
    ("readout32_no_padding", dict(readout_mlp_hidden_layers_width=32), dict(no_channel_padding=1),
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0x5e94e5ca12411532, 4201728, 14065664),
    ("readout32_no_padding_no_operator", dict(readout_mlp_hidden_layers_width=32), dict(no_channel_padding=1, tp_no_operator=1),
     "moments/single", "0 0 0 0 0 0 0 0 1 0 0 0", 0xf2a618f00da1abc4, 1867008, 13033472),
    # nonlinearity, species, embedding
    ("mish_latents", MISH, {},
     "spec_chain/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0xf0a85129fece44b4, 2530560, 17162240),
    ("mish_latents_no_chain", MISH, dict(tp_no_chain=1),
     "spec/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0x3190a24e8469f69a, 2530560, 25419776),
    ("species2", dict(type_names=["A", "B"]), {},
     "moments/chains", "1 1 1 1 1 24 32 1 1 0 0 0", 0x9e5f613f41381be7, 2768128, 13557760),
    ("species3", dict(type_names=["A", "B", "C"]), {},
     "moments/chains", "1 1 1 1 1 24 32 1 1 0 0 0", 0xee864b5e95f7c281, 2789120, 13500416),
    ("species4", dict(type_names=["A", "B", "C", "D"]), {},
     "moments/chains", "0 0 0 0 1 0 0 1 1 0 0 0", 0xb0e648bc6c50efdc, 2752256, 13499392),
    ("spline", SPLINE, {},
     "moments/chains", "0 0 0 0 1 0 0 1 1 0 0 0", 0x80581b338bcf1623, 2757888, 13499392),
    ("spline_species4", dict(SPLINE, type_names=["A", "B", "C", "D"]), {},
     "moments/chains", "0 0 0 0 1 0 0 1 1 0 0 0", 0x11afab5c73718737, 2819840, 13499392),
    ("embed_dim48", dict(radial_chemical_embed_dim=48), {},
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0xf05c597508f6da59, 4537088, 14295040),
    ("embed_dim32", dict(radial_chemical_embed_dim=32), {},
     "moments/chains", "0 0 0 0 1 0 0 1 1 0 0 0", 0x3752f4e0b14d52d3, 2693376, 13040640),
    # every option plan_create reads, on a case where it changes the outcome
    ("tp_generic", {}, dict(tp_generic=1),
     "general/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0xef9114be7f77aa73, 2530560, 25290752),
    ("tp_no_chain", {}, dict(tp_no_chain=1),
     "operator/chains", "0 0 0 0 1 0 0 1 1 1 0 0", 0x97e5c3f3113fa3bb, 3443968, 15047680),
    ("tp_no_chain_no_operator", {}, dict(tp_no_chain=1, tp_no_operator=1),
     "spec/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0x3190a24e8469f69a, 2530560, 25419776),
    ("tp_no_moments", {}, dict(tp_no_moments=1),
     "spec_chain/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0xf0a85129fece44b4, 2530560, 17162240),
    ("tp_force_operator", {}, dict(tp_force_operator=1),
     "operator/chains", "0 0 0 0 1 0 0 1 1 1 0 0", 0x92187a1810b0f739, 3443968, 14588928),
    ("c5_no_operator", C5, dict(tp_no_operator=1),
     "general/single", "0 0 0 0 0 0 0 0 0 0 0 0", 0x2421b960b40970e3, 32199680, 295522304),
    ("gemm_no_chain", {}, dict(gemm_no_chain=1),
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0x76aad1cafe7afe58, 4545792, 14524416),
    ("gemm_fp32_mfma", {}, dict(gemm_fp32_mfma=1),
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0x76aad1cafe7afe58, 4545792, 14524416),
    ("gemm_valu", {}, dict(gemm_valu=1),
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0x76aad1cafe7afe58, 4545792, 14524416),
    ("gemm_no_chain_prefer_moments", {}, dict(gemm_no_chain=1, tp_prefer_moments=1),
     "moments/single", "0 0 0 0 0 0 0 0 1 0 0 0", 0x6008aa54ddddf66d, 2039040, 13492224),
    ("c5_no_slot_form", C5, dict(no_slot_form=1),
     "operator/single", "0 0 0 0 0 0 0 0 1 1 0 0", 0x4b22852e57bc6597, 35345408, 82694144),
    ("c5_op_proj_never", C5, dict(op_proj_gemm=2),
     "operator/slot", "0 0 0 0 0 0 0 0 1 1 1 0", 0x4ac0f772059eecd2, 41899008, 81645568),
    ("embed_no_fuse", {}, dict(embed_no_fuse=1),
     "moments/chains", "1 1 1 1 1 24 32 1 1 0 0 1", 0x1c500ed149be09ee, 2755840, 13500416),
    ("fused_forward_never", {}, dict(fused_forward=3),
     "moments/chains", "0 0 0 0 1 0 0 1 1 0 0 0", 0x1c500ed149be09ee, 2755840, 13556736),
    ("fused_narrow", {}, dict(fused_narrow=1),
     "moments/chains", "1 1 1 1 1 24 32 1 1 0 0 0", 0x1c500ed149be09ee, 2755840, 13557760),
]


def _describe(flags: str) -> dict:
    return {k: (int(v) if k in COUNTS else bool(int(v))) for k, v in zip(KEYS, flags.split())}


def _plan_facts(lib, cfg, options):
    opt = _lib.PlanOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    h = lib.model_plan_create(cfg, opt)
    try:
        buf = C.create_string_buffer(1024)
        lib.check(min(0, lib.lib.aa_model_plan_describe(h, buf, 1024)), "aa_model_plan_describe")
        return (json.loads(buf.value.decode()), lib.lib.aa_model_plan_layout_hash(h), lib.lib.aa_model_weights_bytes(h),
                lib.lib.aa_model_workspace_bytes(h, 64, 1792, 1))
    finally:
        lib.model_plan_destroy(h)


def _check_case(lib, case):
    name, overrides, options, pipeline, flags, layout_hash, weight_bytes, workspace_bytes = case
    cfg, keep = HipAllegroModel(**dict(BASE, **overrides))._build_config()
    d, h, wb, ws = _plan_facts(lib, cfg, options)
    print(f"{name}: {pipeline} {d} hash {h:#018x} weights {wb} workspace {ws}")
    want = _describe(flags)
    assert list(d) == KEYS and d == want, (name, d, want)
    tp, linear = pipeline.split("/")
    assert d["operator_path"] == (tp == "operator") and d["moments"] == (tp in ("moments", "operator")), (name, pipeline, d)
    assert d["chain_gemm"] == (linear == "chains") and d["slot_form"] == (linear == "slot"), (name, pipeline, d)
    assert h != 0 and (h, wb, ws) == (layout_hash, weight_bytes, workspace_bytes), (name, hex(h), wb, ws)
    assert _plan_facts(lib, cfg, options) == (d, h, wb, ws), name  # a second plan from the same inputs
    del keep


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_pipeline_emulation(case):
    from tests.hip_utils import emu_lib

    _check_case(emu_lib(), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_pipeline_gpu(case):
    assert torch.cuda.is_available()
    _check_case(_lib.load(), case)


def test_the_cases_reach_every_pipeline():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    assert {c[3] for c in CASES} == PIPELINES
    described = [_describe(c[4]) for c in CASES]
    for k in KEYS:  # both values of every key (the two step counts: zero and non-zero)
        assert {bool(d[k]) for d in described} == {False, True}, k
    # the three per-edge paths, which the dictionary cannot tell apart, have different layouts on the same model
    by_name = {c[0]: c for c in CASES}
    assert len({by_name[n][5] for n in ("tp_generic", "tp_no_chain_no_operator", "tp_no_moments")}) == 3
    # every option the selector reads changes the outcome of a case it is set on: the same model without it is in the table too
    facts = {(json.dumps(c[1], sort_keys=True), json.dumps(c[2], sort_keys=True)): c[4:] for c in CASES}
    for opt, val in OPTIONS.items():
        moved = False
        for c in CASES:
            if c[2].get(opt) == val:
                rest = {k: v for k, v in c[2].items() if k != opt}
                twin = facts.get((json.dumps(c[1], sort_keys=True), json.dumps(rest, sort_keys=True)))
                moved = moved or (twin is not None and twin != c[4:])
        assert moved, opt
