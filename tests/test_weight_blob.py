"""The packed weight blob, byte by byte.

`layout_blob` (csrc/aa_model.hip) lays the blob out and `pack_blob_host` fills it: padding, the ScalarMLPFunction constants, every
fold product, the fp32 rounding and the bf16x3 split are host arithmetic, so the result is reproducible to the byte.  Each case of
`tests/test_plan_pipeline.py` (the same model overrides and plan options: every pipeline, every fold flag) is planned and packed --
no step, no kernel launch -- and the sha256 of the blob is the recorded one (its first 16 hex digits).
The weights are closed-form, not the seeded initialisation, so that a digest does not depend on torch's generator: element i of the
k-th floating-point entry of the state_dict (key order) is ((A i + C (k + 1)) mod 2^24 / 2^24 - 0.5) * 2, exact in fp32 and fp64.
`bessel_weights` and `edge_norm.rmax_recip` keep the constructor's (deterministic) values: the packer recognises the roots n pi.
(The configuration, which reads the w3j buffers, is built before the overwrite.)
The expected values were recorded from the library of the commit BEFORE the layout was gathered into `BlobLayout` and the packer was
split (that commit's emulation build, the same inputs), not from the code under test: the refactor must not move a byte.  Both
variants assert that one column: the host code of the gfx950 build comes from another compiler (hipcc -O3 instead of clang -O1),
but neither may reassociate fp64 sums or fuse multiply-adds on baseline x86-64, so the bytes agree.  `pytest -s -n0` prints
`name digest` lines, from which the table can be regenerated on that commit.
Two guards against an empty test: one changed element of a late tensor changes the digest, and cases of equal layout and equal
model have equal digests."""
import hashlib
import json

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd.nn import HipAllegroModel
from tests.test_plan_pipeline import BASE, CASES

# name -> first 16 hex digits of sha256(blob)
DIGESTS = {
    "c1": "7a447c75739f8b12",
    "c1_one_layer": "a6d479208e54855b",
    "c1_f64": "ea4beb17263b691b",
    "c2_c3_c4": "5d8ea83bfe7c64ec",
    "c5": "5cd534e8620cd075",
    "f32_u64_S128": "738b8a61acf1cc5c",
    "f32_u64_S128_prefer_moments": "1f5c1d5c3523f38e",
    "f64_u64_S64": "1a9c89add42cd5ad",
    "f64_u64_S64_prefer_moments": "2c0af0cf584631aa",
    "f64_u64_S128": "e175e07b19ef5dcb",
    "f32_S64_latents128": "d5c267caa6a4035c",
    "f32_S64_latents128_force_operator": "4d9f2a2b029fee65",
    "f64_lmax3_u64": "be26647b8085d132",
    "f64_lmax3_u8_three_layers": "1592953fe86a0585",
    "f64_lmax3_u64_no_operator": "87ca955cb4554358",
    "three_layers": "59b4ed92becaec8b",
    "three_layers_no_operator": "472b974165b9e156",
    "three_layers_u128": "0f2016e96068075b",
    "deep_latents": "e6899cf07f796088",
    "u32": "5afdb9d49b7ea0d6",
    "u32_no_padding": "e3f9d0da6bfcb698",
    "u96": "1673cd58b59639df",
    "u96_no_padding": "31ca7380021b3f80",
    "u16_S32": "62de5bed20691f93",
    "readout32": "254139f91df6f4a6",
    "readout32_no_padding": "247af80ac4068ced",
    "readout32_no_padding_no_operator": "b5e88f36802f3746",
    "mish_latents": "7ceffcad9dd3d8f8",
    "mish_latents_no_chain": "7ceffcad9dd3d8f8",
    "species2": "cc9074c4201eb004",
    "species3": "65744a86195b6726",
    "species4": "37c4504967198fc0",
    "spline": "03c314949b8c5f6e",
    "spline_species4": "5c755618bea3b59f",
    "embed_dim48": "bd53c2947347f5c3",
    "embed_dim32": "a9d6bb7a011c2ab3",
    "tp_generic": "30939a28c0084547",
    "tp_no_chain": "4299d74c4f5d5556",
    "tp_no_chain_no_operator": "53f570da508e73ab",
    "tp_no_moments": "53f570da508e73ab",
    "tp_force_operator": "4299d74c4f5d5556",
    "c5_no_operator": "0507cc84cd3fcbe3",
    "gemm_no_chain": "467db3c740422ad5",
    "gemm_fp32_mfma": "467db3c740422ad5",
    "gemm_valu": "467db3c740422ad5",
    "gemm_no_chain_prefer_moments": "4f636cc0c25b80ed",
    "c5_no_slot_form": "46cff363e35e7dfb",
    "c5_op_proj_never": "ddf6b133fb5c8ee4",
    "embed_no_fuse": "5d8ea83bfe7c64ec",
    "fused_forward_never": "5d8ea83bfe7c64ec",
    "fused_narrow": "5d8ea83bfe7c64ec",
}

_MODELS = {}


def _closed_form(n: int, k: int) -> np.ndarray:
    i = np.arange(n, dtype=np.uint64)
    x = (np.uint64(0x9E3779B1) * i + np.uint64(0x632BE5AB) * np.uint64(k + 1)) % np.uint64(1 << 24)
    return (x.astype(np.float64) / float(1 << 24) - 0.5) * 2.0


def _model(overrides):
    """(model with the closed-form weights, its configuration, what the configuration points into): one per distinct overrides"""
    key = json.dumps(overrides, sort_keys=True)
    if key not in _MODELS:
        model = HipAllegroModel(**dict(BASE, **overrides))
        cfg, keep = model._build_config()
        with torch.no_grad():
            k = 0
            for name, v in model.state_dict().items():
                if not v.is_floating_point():
                    continue
                if not name.endswith(("bessel_weights", "edge_norm.rmax_recip")):
                    v.copy_(torch.from_numpy(_closed_form(v.numel(), k)).reshape(v.shape).to(v.dtype))
                k += 1
        _MODELS[key] = (model, cfg, keep)
    return _MODELS[key]


def _digest(lib, device, overrides, options) -> str:
    model, cfg, _ = _model(overrides)
    opt = _lib.PlanOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    model._bind_library(lib)
    h = lib.model_plan_create(cfg, opt)
    try:
        blob = model._pack_blob(h, torch.device(device))
        assert blob.numel() == lib.lib.aa_model_weights_bytes(h)
        return hashlib.sha256(blob.cpu().numpy().tobytes()).hexdigest()[:16]
    finally:
        lib.model_plan_destroy(h)


def _check_case(lib, device, case):
    name, overrides, options = case[:3]
    d = _digest(lib, device, overrides, options)
    print(f"{name} {d}")
    assert d == DIGESTS.get(name), (name, d, DIGESTS.get(name))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_weight_blob_emulation(case):
    from tests.hip_utils import emu_lib

    _check_case(emu_lib(), "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_weight_blob_gpu(case):
    assert torch.cuda.is_available()
    _check_case(_lib.load(), "cuda", case)


def test_one_changed_element_changes_the_digest():
    from tests.hip_utils import emu_lib

    model, _, _ = _model({})
    sd = model.state_dict()
    last = max((k for k in sd if ".edge_readout." in k and k.endswith(".weight")), key=lambda k: int(k.split(".")[-2]))
    w = sd[last].view(-1)
    old = w[-1].item()
    try:
        with torch.no_grad():
            w[-1] = old + 0.25
        changed = _digest(emu_lib(), "cpu", {}, {})
    finally:
        with torch.no_grad():
            w[-1] = old
    assert changed != DIGESTS["c2_c3_c4"]
    assert _digest(emu_lib(), "cpu", {}, {}) == DIGESTS["c2_c3_c4"]


def test_equal_layout_and_model_give_equal_digests():
    assert set(DIGESTS) == {c[0] for c in CASES}
    groups = {}
    for c in CASES:
        groups.setdefault((json.dumps(c[1], sort_keys=True), c[5]), []).append(c[0])
    assert ["gemm_no_chain", "gemm_fp32_mfma", "gemm_valu"] in groups.values()
    assert ["c2_c3_c4", "embed_no_fuse", "fused_forward_never", "fused_narrow"] in groups.values()
    for names in groups.values():
        assert len({DIGESTS[n] for n in names}) == 1, names
