"""The per-step decision, case by case: which launches one step consists of.

`choose_step` (csrc/aa_model.hip) decides once per step, from the plan, the graph, whether forces were asked for, the debug
taps and the CU count, which launches the step runs (`StepPlan`); `Runner` only reads that value.
Each case of the table below is a model (constructor overrides on the C2 shape), plan options, a graph recipe, forces
yes / no, taps yes / no, and its ordered list of launches -- stage name, algorithmic bytes, flops -- as
`aa_model_energy_forces_profiled` reports them.

EXPECTED was recorded with `record()` below from the emulation library of the commit BEFORE the decision was gathered into
`choose_step` (`python -m tests.test_step_plan /path/to/that/liballegro_amd_emu.so`), not from the code under test: the
refactor must not move a launch.  The emulation reports 3 CUs, so the size rules of the fused forward (4 and
kFusedTailAtomsPerCu = 64 atoms per CU) fall at 12 and 192 atoms; the cases whose list depends on the CU count run on the
emulation only (`cus_matter`), every other case also on the GPU.  The last test checks the table itself."""
import ctypes as C
import math
import sys

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd.nn import HipAllegroModel, PreparedGraph
from tests.test_plan_pipeline import BASE, PIPELINES

F64 = dict(model_dtype="float64")
L128 = dict(allegro_mlp_hidden_layers_width=128)
R_MAX = BASE["r_max"]


# ---- graph recipes: positions on a jittered grid, per atom the edges to its nearest neighbours --------------------------
def grid_graph(n, degree=3, spacing=1.5, hub_degree=0, bare=(0, 0), species=1, seed=0):
    """`n` atoms; atom i is the center of `degree` - 1 + i % 3 edges, the atom nearest to the middle of the grid (the hub) of
    `hub_degree` edges when that is set; the first bare[0] and the last bare[1] atoms are centers of no edge (the atom-block hint
    then starts above 0 / ends below n).  Every edge is shorter than r_max."""
    rng = np.random.default_rng(seed)
    side = max(1, math.ceil(n ** (1.0 / 3.0) - 1e-9))
    pts = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(float)
    pos = pts * spacing + rng.uniform(-0.1, 0.1, size=(n, 3)) * spacing
    if n == 0:
        return pos, np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.int64)
    d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    np.fill_diagonal(d, np.inf)
    hub = int(np.argmin(np.linalg.norm(pos - pos.mean(0), axis=1))) if hub_degree else -1
    centers, nbrs = [], []
    for i in range(bare[0], n - bare[1]):
        k = hub_degree if i == hub else min(n - 1, degree - 1 + i % 3)
        j = np.argsort(d[i], kind="stable")[:k]
        assert d[i, j].max() < 0.98 * R_MAX, (i, k, d[i, j].max())
        centers += [i] * k
        nbrs += j.tolist()
    return pos, np.array([centers, nbrs], dtype=np.int64), (np.arange(n) % species).astype(np.int64)


LOW12 = dict(n=12)                                   # <= 4 atoms per emulated CU
MID = dict(n=40)                                     # 13..191
BIG = dict(n=200)                                    # >= 64 atoms per emulated CU
LONG_ATOM = dict(n=60, hub_degree=36)                # one atom above 32 neighbours, the average atom far below: mixed form
DENSE = dict(n=48, degree=40, spacing=1.0)           # every atom 39..41 neighbours, 96 tiles: pure team form
VERY_LONG = dict(n=180, spacing=1.0, hub_degree=130)  # a segment above 128: no fused forward
BLOCK = dict(n=40, bare=(5, 3))                      # atom_begin = 5, atom_end = 37
NO_EDGES = dict(n=9, bare=(9, 0))
LARGE = dict(n=4100, degree=2)                       # above the 4096 atoms of op_proj

# (name, model overrides, plan options, graph recipe, extras): extras: forces (default True), taps, no_tcsr (graph without the
# transposed CSR), max_degree (hint set by hand), cus_matter (the list depends on the CU count)
CASES = [
    # every tensor-product path x linear-layer path, forces and energy only
    ("general_single", {}, dict(tp_generic=1), MID, {}),
    ("general_single_energy", {}, dict(tp_generic=1), MID, dict(forces=False)),
    ("general_single_three_layers", dict(num_layers=3), dict(tp_generic=1), MID, {}),
    ("spec_single", {}, dict(tp_no_chain=1, tp_no_operator=1), MID, {}),
    ("spec_single_energy", {}, dict(tp_no_chain=1, tp_no_operator=1), MID, dict(forces=False)),
    ("spec_single_three_layers", dict(num_layers=3), dict(tp_no_operator=1), MID, {}),
    ("spec_single_u128", dict(num_tensor_features=128), dict(tp_no_operator=1, no_channel_padding=1), MID, {}),
    ("spec_chain_single", {}, dict(tp_no_moments=1), MID, {}),
    ("spec_chain_single_energy", {}, dict(tp_no_moments=1), MID, dict(forces=False)),
    ("moments_single", L128, {}, MID, {}),
    ("moments_single_energy", L128, {}, MID, dict(forces=False)),
    ("moments_single_deep_latents", dict(allegro_mlp_hidden_layers_depth=2), {}, MID, {}),
    ("moments_single_f64", F64, dict(tp_prefer_moments=1), MID, {}),
    ("moments_chains_staged", {}, dict(fused_forward=3), MID, {}),
    ("moments_chains_staged_energy", {}, dict(fused_forward=3), MID, dict(forces=False)),
    ("operator_single", L128, dict(tp_force_operator=1), MID, {}),
    ("operator_single_energy", L128, dict(tp_force_operator=1), MID, dict(forces=False)),
    ("operator_slot", {}, dict(gemm_no_chain=1), MID, {}),
    ("operator_slot_energy", {}, dict(gemm_no_chain=1), MID, dict(forces=False)),
    ("operator_slot_f64", F64, {}, MID, {}),
    ("operator_chains", {}, dict(tp_force_operator=1), MID, {}),
    ("operator_chains_energy", {}, dict(tp_force_operator=1), MID, dict(forces=False)),
    ("operator_chains_three_layers", dict(num_layers=3), {}, MID, {}),
    # taps, graph without the transposed CSR, atom-block hint, empty block
    ("taps_fused_plan", {}, {}, MID, dict(taps=True)),
    ("taps_slot_plan", {}, dict(gemm_no_chain=1), MID, dict(taps=True)),
    ("no_tcsr_fused", {}, {}, MID, dict(no_tcsr=True, cus_matter=True)),
    ("no_tcsr_slot", {}, dict(gemm_no_chain=1), MID, dict(no_tcsr=True)),
    ("no_tcsr_general", {}, dict(tp_generic=1), MID, dict(no_tcsr=True)),
    ("block_fused", {}, {}, BLOCK, dict(cus_matter=True)),
    ("block_fused_deep", {}, dict(fused_narrow=2), BLOCK, {}),
    ("block_operator", {}, dict(gemm_no_chain=1), BLOCK, {}),
    ("no_edges_fused_plan", {}, {}, NO_EDGES, {}),
    ("empty_block_fused_deep", {}, dict(fused_narrow=2), dict(n=0), dict(max_degree=8)),
    ("empty_block_staged", {}, dict(fused_forward=3), dict(n=0), {}),
    # fused plan: the size rules of the one-tile pass (3 emulated CUs: <= 12, 13..191, >= 192 atoms)
    ("fused_low", {}, {}, LOW12, dict(cus_matter=True)),
    ("fused_low_energy", {}, {}, LOW12, dict(forces=False)),
    ("fused_mid", {}, {}, MID, dict(cus_matter=True)),
    ("fused_mid_energy", {}, {}, MID, dict(forces=False)),
    ("fused_big", {}, {}, BIG, dict(cus_matter=True)),
    ("fused_big_energy", {}, {}, BIG, dict(forces=False)),
    ("fused_big_lmax1", dict(l_max=1), {}, BIG, dict(cus_matter=True)),
    ("fused_big_species2", dict(type_names=["A", "B"]), {}, dict(BIG, species=2), dict(cus_matter=True)),
    ("fused_narrow1", {}, dict(fused_narrow=1), BIG, {}),
    ("fused_narrow2", {}, dict(fused_narrow=2), MID, {}),
    ("fused_narrow2_energy", {}, dict(fused_narrow=2), MID, dict(forces=False)),
    ("fused_narrow3", {}, dict(fused_narrow=3), BIG, {}),
    ("fused_narrow4", {}, dict(fused_narrow=4), MID, {}),
    ("fused_forward2", {}, dict(fused_forward=2), LONG_ATOM, {}),
    ("fused_forward3", {}, dict(fused_forward=3), LOW12, {}),
    ("fused_forward4", {}, dict(fused_forward=4), DENSE, {}),
    ("fused_forward4_narrow2", {}, dict(fused_forward=4, fused_narrow=2), DENSE, {}),
    ("one_long_atom", {}, {}, LONG_ATOM, dict(cus_matter=True)),
    ("one_long_atom_narrow2", {}, dict(fused_narrow=2), LONG_ATOM, {}),
    ("small_dense", {}, {}, DENSE, {}),
    ("very_long_atom", {}, {}, VERY_LONG, {}),
    ("very_long_atom_energy", {}, {}, VERY_LONG, dict(forces=False)),
    ("three_species", dict(type_names=["A", "B", "C"]), {}, dict(MID, species=3), dict(cus_matter=True)),
    ("three_species_long_atom", dict(type_names=["A", "B", "C"]), {}, dict(LONG_ATOM, species=3), {}),
    ("unknown_degree", {}, {}, MID, dict(max_degree=0)),
    ("staged_no_fold", {}, dict(fused_forward=3, staged_no_fold=1), MID, {}),
    ("chain_staged_weights", {}, dict(fused_narrow=1, chain_staged_weights=1), MID, {}),
    ("chain_staged_weights_staged", {}, dict(fused_forward=3, chain_staged_weights=1), MID, {}),
    ("embed_no_fuse", {}, dict(embed_no_fuse=1), MID, dict(cus_matter=True)),
    ("embed_no_fuse_staged_no_fold", {}, dict(embed_no_fuse=1, fused_forward=3, staged_no_fold=1), MID, {}),
    ("spline_chains", dict(radial_chemical_embed=dict(_target_="allegro.nn.TwoBodySplineScalarEmbed", num_splines=16, spline_span=12)), {}, MID, {}),
    ("species4_chains", dict(type_names=["A", "B", "C", "D"]), {}, dict(MID, species=4), {}),
    ("readout_two_pass", L128, dict(readout_two_pass=1), MID, {}),
    ("readout_two_pass_slot", {}, dict(gemm_no_chain=1, readout_two_pass=1), MID, {}),
    # operator kernels: env projections as GEMMs, fused form
    ("op_proj_auto_small", {}, dict(gemm_no_chain=1), LOW12, {}),
    ("op_proj_auto_large", {}, dict(gemm_no_chain=1), LARGE, {}),
    ("op_proj_auto_large_energy", {}, dict(gemm_no_chain=1), LARGE, dict(forces=False)),
    ("op_proj_always", {}, dict(gemm_no_chain=1, op_proj_gemm=1), MID, {}),
    ("op_proj_always_energy", {}, dict(gemm_no_chain=1, op_proj_gemm=1), MID, dict(forces=False)),
    ("op_proj_always_single", L128, dict(tp_force_operator=1, op_proj_gemm=1), MID, {}),
    ("op_proj_never_large", {}, dict(gemm_no_chain=1, op_proj_gemm=2), LARGE, {}),
    ("tp_operator_fused", {}, dict(gemm_no_chain=1, tp_operator_fused=1), MID, {}),
    ("tp_operator_fused_proj_always", {}, dict(gemm_no_chain=1, tp_operator_fused=1, op_proj_gemm=1), MID, {}),
]
NAMES = [c[0] for c in CASES]


# ---- one step ---------------------------------------------------------------------------------------------------------
def run_case(lib, case, device="cpu"):
    """(launches [(name, bytes, flops)], atom energies, forces | None, pipeline "tp/linear") of one profiled step"""
    name, overrides, options, recipe, extra = case
    dev = torch.device(device)
    m = HipAllegroModel(**dict(BASE, **overrides)).to(dev)
    m._bind_library(lib)
    m._select_device(dev)
    cfg, keep = m._build_config()
    opt = _lib.PlanOptions()
    opt.poison_workspace = 1
    for k, v in options.items():
        setattr(opt, k, v)
    m._plan_handle, m._plan_keep = lib.model_plan_create(cfg, opt), (cfg, keep)
    d = m.describe_plan()
    pipeline = ("operator" if d["operator_path"] else "moments" if d["moments"] else "per_edge") + "/" + (
        "chains" if d["chain_gemm"] else "slot" if d["slot_form"] else "single")
    if extra.get("taps"):
        m.enable_debug_taps()
    pos, ei, types = grid_graph(**recipe)
    n = len(pos)
    rows = max(n, 1)  # (no atoms: the library still wants non-null arrays)
    g = PreparedGraph(torch.tensor(ei, device=dev), torch.tensor(types if n else [0], device=dev), n, None, transposed=not extra.get("no_tcsr"),
                      lib=lib)
    if "max_degree" in extra:
        g.max_degree = extra["max_degree"]
    p = torch.zeros((rows, 3), dtype=m.dtype, device=dev)
    p[:n] = torch.tensor(pos, dtype=m.dtype)
    m._ensure_weights(dev)
    forces = extra.get("forces", True)
    need = lib.lib.aa_model_workspace_bytes(m._plan_handle, n, g.num_edges, int(forces))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    e = torch.full((rows,), float("nan"), dtype=m.dtype, device=dev)
    f = torch.full((rows, 3), float("nan"), dtype=m.dtype, device=dev) if forces else None
    mx = 128
    ms, by, fl, nst = (C.c_float * mx)(), (C.c_double * mx)(), (C.c_double * mx)(), C.c_int(0)
    names = C.create_string_buffer(32 * mx)
    fn = lib.lib.aa_model_energy_forces_profiled
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    cg = g.c_struct()
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    ctx = torch.cuda.device(dev) if dev.type == "cuda" else torch.no_grad()
    with ctx:
        lib.check(fn(m._plan_handle, m._blob.data_ptr(), C.byref(cg), p.data_ptr(), ws.data_ptr(), ws.numel(), e.data_ptr(),
                     f.data_ptr() if forces else None, stream, mx, ms, names, C.byref(nst), by, fl), "aa_model_energy_forces_profiled")
        m.check(dev)
    assert nst.value < mx
    stages = [(names.raw[32 * i: 32 * i + 32].split(b"\0")[0].decode(), by[i], fl[i]) for i in range(nst.value)]
    return stages, e[:n].cpu(), None if f is None else f[:n].cpu(), pipeline


def encode(stages) -> str:
    return " ".join(f"{n}:{b:.17g}:{f:.17g}" for n, b, f in stages)


def record(lib_path):
    """Prints EXPECTED as recorded from the emulation library at `lib_path` (the commit before `choose_step`)."""
    lib = _lib.AllegroLib(C.CDLL(lib_path), is_emulation=True)
    print("EXPECTED = {")
    for case in CASES:
        stages, _, _, pipeline = run_case(lib, case)
        print(f"    {case[0]!r}: ({pipeline!r},\n        {encode(stages)!r}),")
    print("}")


EXPECTED = {
    'general_single': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x448:243712:6823936 tp_layer_fwd:676028:0 gemm_128x64:91392:1949696 gemm_64x256:152320:3899392 tp_layer_fwd:676028:0 gemm_192x64:121856:2924544 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:4764:0 gemm_64x192:121856:2924544 gemm_64x64:91392:974848 gemm_64x192:182784:2924544 tp_layer_bwd:1137272:0 gemm_256x64:182784:3899392 gemm_64x128:121856:1949696 tp_layer_bwd:1137272:0 gemm_448x64:243712:6823936 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:39508:0 force_gather:5084:0'),
    'general_single_energy': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x448:243712:6823936 tp_layer_fwd:676028:0 gemm_128x64:91392:1949696 gemm_64x256:152320:3899392 tp_layer_fwd:676028:0 gemm_192x64:121856:2924544 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:30624:0'),
    'general_single_three_layers': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x448:243712:6823936 tp_layer_fwd:676028:0 gemm_128x64:91392:1949696 gemm_64x256:152320:3899392 tp_layer_fwd:676028:0 gemm_192x64:121856:2924544 gemm_64x256:152320:3899392 tp_layer_fwd:676028:0 gemm_256x64:152320:3899392 gemm_64x64:60928:974848 gemm_256x64:152320:3899392 readout_reduce:61088:0 memset:4764:0 gemm_64x256:152320:3899392 gemm_64x64:91392:974848 gemm_64x256:243712:3899392 tp_layer_bwd:1137272:0 gemm_256x64:182784:3899392 gemm_64x192:182784:2924544 tp_layer_bwd:1137272:0 gemm_256x64:182784:3899392 gemm_64x128:121856:1949696 tp_layer_bwd:1137272:0 gemm_448x64:243712:6823936 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:39508:0 force_gather:5084:0'),
    'spec_single': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x448:243712:6823936 tp_spec_fwd:401852:0 gemm_128x64:91392:1949696 gemm_64x256:152320:3899392 tp_spec_fwd:401852:0 gemm_192x64:121856:2924544 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x192:121856:2924544 gemm_64x64:91392:974848 gemm_64x192:182784:2924544 tp_spec_bwd:1141556:0 gemm_256x64:182784:3899392 gemm_64x128:121856:1949696 tp_spec_bwd:1141556:0 gemm_448x64:243712:6823936 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'spec_single_energy': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x448:243712:6823936 tp_spec_fwd:401852:0 gemm_128x64:91392:1949696 gemm_64x256:152320:3899392 tp_spec_fwd:401852:0 gemm_192x64:121856:2924544 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:30624:0'),
    'spec_single_three_layers': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x448:243712:6823936 tp_spec_fwd:401852:0 gemm_128x64:91392:1949696 gemm_64x256:152320:3899392 tp_spec_fwd:401852:0 gemm_192x64:121856:2924544 gemm_64x256:152320:3899392 tp_spec_fwd:401852:0 gemm_256x64:152320:3899392 gemm_64x64:60928:974848 gemm_256x64:152320:3899392 readout_reduce:61088:0 memset:480:0 gemm_64x256:152320:3899392 gemm_64x64:91392:974848 gemm_64x256:243712:3899392 tp_spec_bwd:1141556:0 gemm_256x64:182784:3899392 gemm_64x192:182784:2924544 tp_spec_bwd:1141556:0 gemm_256x64:182784:3899392 gemm_64x128:121856:1949696 tp_spec_bwd:1141556:0 gemm_448x64:243712:6823936 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:52360:0 force_gather:5084:0'),
    'spec_single_u128': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x832:426496:12673024 tp_spec_fwd:799420:0 gemm_192x64:121856:2924544 gemm_64x448:243712:6823936 tp_chain_fwd_last:799420:0 gemm_256x64:152320:3899392 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:13332:0 gemm_64x192:121856:2924544 gemm_64x64:91392:974848 gemm_64x256:213248:3899392 tp_chain_bwd_last:986488:0 gemm_448x64:274176:6823936 gemm_64x192:152320:2924544 tp_chain_bwd_first:1234484:0 gemm_832x64:426496:12673024 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'spec_chain_single': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x448:243712:6823936 tp_spec_fwd:401852:0 gemm_128x64:91392:1949696 gemm_64x256:152320:3899392 tp_chain_fwd_last:401852:0 gemm_192x64:121856:2924544 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x192:121856:2924544 gemm_64x64:91392:974848 gemm_64x192:182784:2924544 tp_chain_bwd_last:497528:0 gemm_256x64:182784:3899392 gemm_64x128:121856:1949696 tp_chain_bwd_first:623668:0 gemm_448x64:243712:6823936 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'spec_chain_single_energy': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x448:243712:6823936 tp_spec_fwd:401852:0 gemm_128x64:91392:1949696 gemm_64x256:152320:3899392 tp_chain_fwd_last:401852:0 gemm_192x64:121856:2924544 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:30624:0'),
    'moments_single': ('moments/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_mom_fwd_first:248764:0 gemm_128x128:121856:3899392 gemm_128x64:91392:1949696 tp_mom_fwd_last:371388:0 gemm_192x128:152320:5849088 gemm_128x64:91392:1949696 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x192:121856:2924544 gemm_64x128:152320:1949696 gemm_128x192:213248:5849088 tp_mom_bwd_last:344440:0 gemm_64x128:213248:1949696 gemm_128x128:152320:3899392 tp_mom_bwd_first:501812:0 gemm_256x64:182784:3899392 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'moments_single_energy': ('moments/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_mom_fwd_first:248764:0 gemm_128x128:121856:3899392 gemm_128x64:91392:1949696 tp_mom_fwd_last:371388:0 gemm_192x128:152320:5849088 gemm_128x64:91392:1949696 gemm_192x64:121856:2924544 readout_reduce:30624:0'),
    'moments_single_deep_latents': ('moments/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_mom_fwd_first:248764:0 gemm_128x64:91392:1949696 gemm_64x64:60928:974848 gemm_64x64:60928:974848 tp_mom_fwd_last:340924:0 gemm_192x64:121856:2924544 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x192:121856:2924544 gemm_64x64:91392:974848 gemm_64x64:91392:974848 gemm_64x192:182784:2924544 tp_mom_bwd_last:283512:0 gemm_64x64:121856:974848 gemm_64x64:91392:974848 gemm_64x128:121856:1949696 tp_mom_bwd_first:501812:0 gemm_256x64:182784:3899392 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'moments_single_f64': ('moments/single',
        'edge_prologue:79968:0 gemm_64x64:121856:974848 gemm_64x64:121856:974848 gemm_64x256:304640:3899392 tp_mom_fwd_first:497528:0 gemm_128x64:182784:1949696 gemm_64x64:121856:974848 tp_mom_fwd_last:681848:0 gemm_192x64:243712:2924544 gemm_64x64:121856:974848 gemm_192x64:243712:2924544 readout_reduce:122176:0 memset:960:0 gemm_64x192:243712:2924544 gemm_64x64:182784:974848 gemm_64x192:365568:2924544 tp_mom_bwd_last:567024:0 gemm_64x64:243712:974848 gemm_64x128:243712:1949696 tp_mom_bwd_first:1003624:0 gemm_256x64:365568:3899392 gemm_64x64:182784:974848 gemm_64x64:121856:974848 edge_backward:95200:0 force_gather:9372:0'),
    'moments_chains_staged': ('moments/chains',
        'edge_prologue:40460:0 gc_64x64_64x256:182784:4874240 tp_mom_fwd_first:248764:0 gc_128x64:91392:1949696 tp_mom_fwd_last:340924:0 gc_192x64_192x64:213248:5849088 readout_reduce:636:0 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64:182784:3899392 edge_backward:21420:0 force_gather:5084:0'),
    'moments_chains_staged_energy': ('moments/chains',
        'edge_prologue:40460:0 gc_64x64_64x256:182784:4874240 tp_mom_fwd_first:248764:0 gc_128x64:91392:1949696 tp_mom_fwd_last:340924:0 gc_192x64_192x64:213248:5849088 readout_reduce:636:0'),
    'operator_single': ('operator/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_fwd:248764:0 gemm_128x128:121856:3899392 gemm_128x64:91392:1949696 tp_op_fwd:371388:0 gemm_192x128:152320:5849088 gemm_128x64:91392:1949696 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x192:121856:2924544 gemm_64x128:152320:1949696 gemm_128x192:213248:5849088 tp_op_bwd:436600:0 gemm_64x128:213248:1949696 gemm_128x128:152320:3899392 tp_op_bwd:501812:0 gemm_256x64:182784:3899392 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:52360:0 force_gather:5084:0'),
    'operator_single_energy': ('operator/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_fwd:248764:0 gemm_128x128:121856:3899392 gemm_128x64:91392:1949696 tp_op_fwd:371388:0 gemm_192x128:152320:5849088 gemm_128x64:91392:1949696 gemm_192x64:121856:2924544 readout_reduce:30624:0'),
    'operator_slot': ('operator/slot',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_fwd:248764:0 gemm_128x64:91392:1949696 tp_op_fwd:340924:0 gemm_192x64:121856:2924544 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x64:91392:974848 gemm_64x64:60928:974848 tp_op_bwd:375672:0 gemm_128x64:152320:1949696 gemm_64x64:60928:974848 tp_op_bwd:501812:0 gemm_192x64:121856:2924544 gemm_256x64:213248:3899392 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'operator_slot_energy': ('operator/slot',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_fwd:248764:0 gemm_128x64:91392:1949696 tp_op_fwd:340924:0 gemm_192x64:121856:2924544 gemm_192x64:121856:2924544 readout_reduce:30624:0'),
    'operator_slot_f64': ('operator/slot',
        'edge_prologue:79968:0 gemm_64x64:121856:974848 gemm_64x256:304640:3899392 tp_op_fwd:497528:0 gemm_128x64:182784:1949696 tp_op_fwd:681848:0 gemm_192x64:243712:2924544 gemm_192x64:243712:2924544 readout_reduce:122176:0 memset:960:0 gemm_64x64:182784:974848 gemm_64x64:121856:974848 tp_op_bwd:751344:0 gemm_128x64:304640:1949696 gemm_64x64:121856:974848 tp_op_bwd:1003624:0 gemm_192x64:243712:2924544 gemm_256x64:426496:3899392 gemm_64x64:121856:974848 edge_backward:95200:0 force_gather:9372:0'),
    'operator_chains': ('operator/chains',
        'edge_prologue:40460:0 gc_64x64_64x64_64x256:213248:5849088 tp_op_fwd:248764:0 gc_128x64_64x64:121856:2924544 tp_op_fwd:340924:0 gc_192x64_64x64_192x64:243712:6823936 readout_reduce:636:0 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_op_bwd:375672:0 gc_64x128:182784:1949696 tp_op_bwd:501812:0 gc_256x64_64x64:182784:4874240 edge_backward:21420:0 force_gather:5084:0'),
    'operator_chains_energy': ('operator/chains',
        'edge_prologue:40460:0 gc_64x64_64x64_64x256:213248:5849088 tp_op_fwd:248764:0 gc_128x64_64x64:121856:2924544 tp_op_fwd:340924:0 gc_192x64_64x64_192x64:243712:6823936 readout_reduce:636:0'),
    'operator_chains_three_layers': ('operator/chains',
        'edge_prologue:40460:0 gc_64x64_64x64_64x256:213248:5849088 tp_op_fwd:248764:0 gc_128x64_64x64:121856:2924544 tp_op_fwd:340924:0 gc_192x64_64x64:152320:3899392 tp_op_fwd:433084:0 gc_256x64_64x64_256x64:304640:8773632 readout_reduce:636:0 memset:480:0 gc_64x64_64x64_128x192_64x64:213248:8773632 tp_op_bwd:467832:0 gc_64x64_64x192:243712:3899392 tp_op_bwd:467832:0 gc_64x64_64x128:182784:2924544 tp_op_bwd:624436:0 gc_256x64_64x64:182784:4874240 edge_backward:25704:0 force_gather:5084:0'),
    'taps_fused_plan': ('moments/chains',
        'edge_prologue:40460:0 gc_64x64_64x64_64x256:213248:5849088 tp_mom_fwd_first:248764:0 gc_128x64_64x64:121856:2924544 tp_mom_fwd_last:340924:0 gc_192x64_64x64_192x64:243712:6823936 readout_reduce:636:0 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64_64x64:182784:4874240 edge_backward:21420:0 force_gather:5084:0'),
    'taps_slot_plan': ('operator/slot',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_fwd:248764:0 gemm_128x64:91392:1949696 gemm_64x64:60928:974848 tp_op_fwd:340924:0 gemm_192x64:121856:2924544 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x192:121856:2924544 gemm_64x64:91392:974848 gemm_64x192:182784:2924544 tp_op_bwd:375672:0 gemm_64x64:121856:974848 gemm_64x128:121856:1949696 tp_op_bwd:501812:0 gemm_256x64:182784:3899392 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'no_tcsr_fused': ('moments/chains',
        'fused_fwd:436924:15597568 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64:182784:3899392 edge_backward:22372:0'),
    'no_tcsr_slot': ('operator/slot',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_fwd:248764:0 gemm_128x64:91392:1949696 tp_op_fwd:340924:0 gemm_192x64:121856:2924544 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x64:91392:974848 gemm_64x64:60928:974848 tp_op_bwd:375672:0 gemm_128x64:152320:1949696 gemm_64x64:60928:974848 tp_op_bwd:501812:0 gemm_192x64:121856:2924544 gemm_256x64:213248:3899392 gemm_64x64:60928:974848 edge_backward:49028:0'),
    'no_tcsr_general': ('per_edge/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x448:243712:6823936 tp_layer_fwd:676028:0 gemm_128x64:91392:1949696 gemm_64x256:152320:3899392 tp_layer_fwd:676028:0 gemm_192x64:121856:2924544 gemm_64x64:60928:974848 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:4764:0 gemm_64x192:121856:2924544 gemm_64x64:91392:974848 gemm_64x192:182784:2924544 tp_layer_bwd:1137272:0 gemm_256x64:182784:3899392 gemm_64x128:121856:1949696 tp_layer_bwd:1137272:0 gemm_448x64:243712:6823936 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:40460:0'),
    'block_fused': ('moments/chains',
        'fused_fwd:388256:12582912 memset:480:0 gc_64x64_128x128_64x64:147456:4718592 tp_mom_bwd_last:246528:0 gc_64x128:147456:1572864 tp_mom_bwd_first:440448:0 gc_256x64:147456:3145728 edge_backward:17280:0 force_gather:4256:0'),
    'block_fused_deep': ('moments/chains',
        'fused_fwd:440864:18874368 memset:480:0 tp_mom_bwd_first:440448:0 gc_256x64:147456:3145728 edge_backward:17280:0 force_gather:4256:0'),
    'block_operator': ('operator/slot',
        'edge_prologue:32640:0 gemm_64x64:49152:786432 gemm_64x256:122880:3145728 tp_op_fwd:218496:0 gemm_128x64:73728:1572864 tp_op_fwd:310656:0 gemm_192x64:98304:2359296 gemm_192x64:98304:2359296 readout_reduce:49312:0 memset:480:0 gemm_64x64:73728:786432 gemm_64x64:49152:786432 tp_op_bwd:338688:0 gemm_128x64:122880:1572864 gemm_64x64:49152:786432 tp_op_bwd:440448:0 gemm_192x64:98304:2359296 gemm_256x64:172032:3145728 gemm_64x64:49152:786432 edge_backward:38784:0 force_gather:4256:0'),
    'no_edges_fused_plan': ('moments/chains',
        'edge_prologue:0:0 gc_64x64_64x256:0:0 tp_mom_fwd_first:20736:0 gc_128x64:0:0 tp_mom_fwd_last:41472:0 gc_192x64_192x64:0:0 readout_reduce:36:0 memset:108:0 gc_64x64_128x128_64x64:0:0 tp_mom_bwd_last:20736:0 gc_64x128:0:0 tp_mom_bwd_first:41472:0 gc_256x64:0:0 edge_backward:0:0'),
    'empty_block_fused_deep': ('moments/chains',
        'fused_fwd:0:0 memset:0:0 gc_64x64_128x128_64x64:0:0 tp_mom_bwd_last:0:0 gc_64x128:0:0 tp_mom_bwd_first:0:0 gc_256x64:0:0 edge_backward:0:0'),
    'empty_block_staged': ('moments/chains',
        'edge_prologue:0:0 gc_64x64_64x256:0:0 tp_mom_fwd_first:0:0 gc_128x64:0:0 tp_mom_fwd_last:0:0 gc_192x64_192x64:0:0 readout_reduce:0:0 memset:0:0 gc_64x64_128x128_64x64:0:0 tp_mom_bwd_last:0:0 gc_64x128:0:0 tp_mom_bwd_first:0:0 gc_256x64:0:0 edge_backward:0:0'),
    'fused_low': ('moments/chains',
        'fused_fwd:131712:4718592 memset:144:0 gc_64x64_128x128_64x64:55296:1769472 tp_mom_bwd_last:85536:0 gc_64x128:55296:589824 tp_mom_bwd_first:151344:0 gc_256x64:55296:1179648 edge_backward:6480:0 force_gather:1536:0'),
    'fused_low_energy': ('moments/chains',
        'fused_fwd:131712:4718592'),
    'fused_mid': ('moments/chains',
        'fused_fwd:436924:15597568 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64:182784:3899392 edge_backward:21420:0 force_gather:5084:0'),
    'fused_mid_energy': ('moments/chains',
        'fused_fwd:436924:15597568'),
    'fused_big': ('moments/chains',
        'fused_fwd:2521336:117768192 memset:2400:0 tp_mom_bwd_first:2519732:0 gc_256x64:920064:19628032 edge_backward:107820:0 force_gather:25564:0'),
    'fused_big_energy': ('moments/chains',
        'fused_fwd:2193084:78512128'),
    'fused_big_lmax1': ('moments/chains',
        'fused_fwd:1832032:112861184 memset:2400:0 tp_mom_bwd_first:1665104:0 gc_192x64:766720:14721024 edge_backward:71880:0 force_gather:25564:0'),
    'fused_big_species2': ('moments/chains',
        'fused_fwd:2193084:78512128 memset:2400:0 gc_64x64_128x128_64x64:920064:29442048 tp_mom_bwd_last:1423992:0 gc_64x128:920064:9814016 tp_mom_bwd_first:2519732:0 gc_256x64:920064:19628032 edge_backward:107820:0 force_gather:25564:0'),
    'fused_narrow1': ('moments/chains',
        'fused_fwd:2193084:78512128 memset:2400:0 gc_64x64_128x128_64x64:920064:29442048 tp_mom_bwd_last:1423992:0 gc_64x128:920064:9814016 tp_mom_bwd_first:2519732:0 gc_256x64:920064:19628032 edge_backward:107820:0 force_gather:25564:0'),
    'fused_narrow2': ('moments/chains',
        'fused_fwd:502136:23396352 memset:480:0 tp_mom_bwd_first:501812:0 gc_256x64:182784:3899392 edge_backward:21420:0 force_gather:5084:0'),
    'fused_narrow2_energy': ('moments/chains',
        'fused_fwd:436924:15597568'),
    'fused_narrow3': ('moments/chains',
        'fused_fwd:2193084:78512128 memset:2400:0 gc_64x64_128x128_64x64:920064:29442048 tp_mom_bwd_last:1423992:0 gc_64x128:920064:9814016 tp_mom_bwd_first:2519732:0 gc_256x64:920064:19628032 edge_backward:107820:0 force_gather:25564:0'),
    'fused_narrow4': ('moments/chains',
        'fused_fwd:467388:21446656 memset:480:0 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64:182784:3899392 edge_backward:21420:0 force_gather:5084:0'),
    'fused_forward2': ('moments/chains',
        'fused_fwd:728388:27918336 memset:720:0 gc_64x64_128x128_64x64:327168:10469376 tp_mom_bwd_last:480744:0 gc_64x128:327168:3489792 tp_mom_bwd_first:844764:0 gc_256x64:327168:6979584 edge_backward:38340:0 force_gather:8868:0'),
    'fused_forward3': ('moments/chains',
        'edge_prologue:12240:0 gc_64x64_64x256:55296:1474560 tp_mom_fwd_first:75024:0 gc_128x64:27648:589824 tp_mom_fwd_last:102672:0 gc_192x64_192x64:64512:1769472 readout_reduce:192:0 memset:144:0 gc_64x64_128x128_64x64:55296:1769472 tp_mom_bwd_last:85536:0 gc_64x128:55296:589824 tp_mom_bwd_first:151344:0 gc_256x64:55296:1179648 edge_backward:6480:0 force_gather:1536:0'),
    'fused_forward4': ('moments/chains',
        'fused_fwd:4284864:251658240 memset:576:0 gc_64x64_128x128_64x64:2949120:94371840 tp_mom_bwd_last:3197952:0 gc_64x128:2949120:31457280 tp_mom_bwd_first:5343744:0 gc_256x64:2949120:62914560 edge_backward:345600:0 force_gather:70080:0'),
    'fused_forward4_narrow2': ('moments/chains',
        'fused_fwd:4284864:251658240 memset:576:0 gc_64x64_128x128_64x64:2949120:94371840 tp_mom_bwd_last:3197952:0 gc_64x128:2949120:31457280 tp_mom_bwd_first:5343744:0 gc_256x64:2949120:62914560 edge_backward:345600:0 force_gather:70080:0'),
    'one_long_atom': ('moments/chains',
        'fused_fwd:728388:27918336 memset:720:0 gc_64x64_128x128_64x64:327168:10469376 tp_mom_bwd_last:480744:0 gc_64x128:327168:3489792 tp_mom_bwd_first:844764:0 gc_256x64:327168:6979584 edge_backward:38340:0 force_gather:8868:0'),
    'one_long_atom_narrow2': ('moments/chains',
        'fused_fwd:728388:27918336 memset:720:0 gc_64x64_128x128_64x64:327168:10469376 tp_mom_bwd_last:480744:0 gc_64x128:327168:3489792 tp_mom_bwd_first:844764:0 gc_256x64:327168:6979584 edge_backward:38340:0 force_gather:8868:0'),
    'small_dense': ('moments/chains',
        'fused_fwd:4284864:251658240 memset:576:0 gc_64x64_128x128_64x64:2949120:94371840 tp_mom_bwd_last:3197952:0 gc_64x128:2949120:31457280 tp_mom_bwd_first:5343744:0 gc_256x64:2949120:62914560 edge_backward:345600:0 force_gather:70080:0'),
    'very_long_atom': ('moments/chains',
        'edge_prologue:226440:0 gc_64x64_64x256:1022976:27279360 tp_mom_fwd_first:1291176:0 gc_128x64:511488:10911744 tp_mom_fwd_last:1705896:0 gc_192x64_192x64:1193472:32735232 readout_reduce:3384:0 memset:2160:0 gc_64x64_128x128_64x64:1022976:32735232 tp_mom_bwd_last:1485648:0 gc_64x128:1022976:10911744 tp_mom_bwd_first:2606328:0 gc_256x64:1022976:21823488 edge_backward:119880:0 force_gather:27576:0'),
    'very_long_atom_energy': ('moments/chains',
        'edge_prologue:226440:0 gc_64x64_64x256:1022976:27279360 tp_mom_fwd_first:1291176:0 gc_128x64:511488:10911744 tp_mom_fwd_last:1705896:0 gc_192x64_192x64:1193472:32735232 readout_reduce:3384:0'),
    'three_species': ('moments/chains',
        'fused_fwd:436924:15597568 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64_64x64:213248:4874240 edge_backward:48076:0 force_gather:5084:0'),
    'three_species_long_atom': ('moments/chains',
        'edge_prologue:72420:0 gc_64x64_64x256:327168:8724480 tp_mom_fwd_first:418548:0 gc_128x64:163584:3489792 tp_mom_fwd_last:556788:0 gc_192x64_192x64:381696:10469376 readout_reduce:1092:0 memset:720:0 gc_64x64_128x128_64x64:327168:10469376 tp_mom_bwd_last:480744:0 gc_64x128:327168:3489792 tp_mom_bwd_first:844764:0 gc_256x64_64x64:381696:8724480 edge_backward:86052:0 force_gather:8868:0'),
    'unknown_degree': ('moments/chains',
        'edge_prologue:40460:0 gc_64x64_64x256:182784:4874240 tp_mom_fwd_first:248764:0 gc_128x64:91392:1949696 tp_mom_fwd_last:340924:0 gc_192x64_192x64:213248:5849088 readout_reduce:636:0 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64:182784:3899392 edge_backward:21420:0 force_gather:5084:0'),
    'staged_no_fold': ('moments/chains',
        'edge_prologue:40460:0 gc_64x64_64x64_64x256:213248:5849088 tp_mom_fwd_first:248764:0 gc_128x64_64x64:121856:2924544 tp_mom_fwd_last:340924:0 gc_192x64_64x64_192x64:243712:6823936 readout_reduce:636:0 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64_64x64:182784:4874240 edge_backward:21420:0 force_gather:5084:0'),
    'chain_staged_weights': ('moments/chains',
        'fused_fwd:436924:15597568 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64:182784:3899392 edge_backward:21420:0 force_gather:5084:0'),
    'chain_staged_weights_staged': ('moments/chains',
        'edge_prologue:40460:0 gc_64x64_64x256:182784:4874240 tp_mom_fwd_first:248764:0 gc_128x64:91392:1949696 tp_mom_fwd_last:340924:0 gc_192x64_192x64:213248:5849088 readout_reduce:636:0 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64:182784:3899392 edge_backward:21420:0 force_gather:5084:0'),
    'embed_no_fuse': ('moments/chains',
        'fused_fwd:436924:15597568 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64_64x64:213248:4874240 edge_backward:48076:0 force_gather:5084:0'),
    'embed_no_fuse_staged_no_fold': ('moments/chains',
        'edge_prologue:40460:0 gc_64x64_64x64_64x256:213248:5849088 tp_mom_fwd_first:248764:0 gc_128x64_64x64:121856:2924544 tp_mom_fwd_last:340924:0 gc_192x64_64x64_192x64:243712:6823936 readout_reduce:636:0 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64_64x64_64x64:213248:5849088 edge_backward:48076:0 force_gather:5084:0'),
    'spline_chains': ('moments/chains',
        'edge_prologue:40460:0 gc_64x64_64x256:182784:4874240 tp_mom_fwd_first:248764:0 gc_128x64:91392:1949696 tp_mom_fwd_last:340924:0 gc_192x64_192x64:213248:5849088 readout_reduce:636:0 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64_64x64:213248:4874240 edge_backward:48076:0 force_gather:5084:0'),
    'species4_chains': ('moments/chains',
        'edge_prologue:40460:0 gc_64x64_64x256:182784:4874240 tp_mom_fwd_first:248764:0 gc_128x64:91392:1949696 tp_mom_fwd_last:340924:0 gc_192x64_192x64:213248:5849088 readout_reduce:636:0 memset:480:0 gc_64x64_128x128_64x64:182784:5849088 tp_mom_bwd_last:283512:0 gc_64x128:182784:1949696 tp_mom_bwd_first:501812:0 gc_256x64_64x64:213248:4874240 edge_backward:48076:0 force_gather:5084:0'),
    'readout_two_pass': ('moments/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_mom_fwd_first:248764:0 gemm_128x128:121856:3899392 gemm_128x64:91392:1949696 tp_mom_fwd_last:371388:0 gemm_192x128:152320:5849088 gemm_128x64:91392:1949696 gemm_192x64:121856:2924544 readout_reduce:30624:0 memset:480:0 readout_backward:60928:0 gemm_64x192:121856:2924544 gemm_64x128:152320:1949696 gemm_128x192:213248:5849088 tp_mom_bwd_last:344440:0 gemm_64x128:213248:1949696 gemm_128x128:152320:3899392 tp_mom_bwd_first:501812:0 gemm_256x64:182784:3899392 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'readout_two_pass_slot': ('operator/slot',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_fwd:248764:0 gemm_128x64:91392:1949696 tp_op_fwd:340924:0 gemm_192x64:121856:2924544 gemm_192x64:121856:2924544 readout_reduce:30624:0 memset:480:0 readout_backward:60928:0 gemm_64x64:91392:974848 gemm_64x64:60928:974848 tp_op_bwd:375672:0 gemm_128x64:152320:1949696 gemm_64x64:60928:974848 tp_op_bwd:501812:0 gemm_192x64:121856:2924544 gemm_256x64:213248:3899392 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'op_proj_auto_small': ('operator/slot',
        'edge_prologue:12240:0 gemm_64x64:18432:294912 gemm_64x256:46080:1179648 tp_op_fwd:75024:0 gemm_128x64:27648:589824 tp_op_fwd:102672:0 gemm_192x64:36864:884736 gemm_192x64:36864:884736 readout_reduce:18480:0 memset:144:0 gemm_64x64:27648:294912 gemm_64x64:18432:294912 tp_op_bwd:113184:0 gemm_128x64:46080:589824 gemm_64x64:18432:294912 tp_op_bwd:151344:0 gemm_192x64:36864:884736 gemm_256x64:64512:1179648 gemm_64x64:18432:294912 edge_backward:14544:0 force_gather:1536:0'),
    'op_proj_auto_large': ('operator/slot',
        'edge_prologue:2787660:0 gemm_64x64:4197888:67166208 gemm_64x256:10494720:268664832 tp_op_moments:2394108:0 op_proj_gemm:18892800:302284800 tp_op_fwd:17842176:0 gemm_128x64:6296832:134332416 tp_op_moments:2394108:0 op_proj_gemm:18892800:302284800 tp_op_fwd:27288576:0 gemm_192x64:8395776:201498624 gemm_192x64:8395776:201498624 readout_reduce:4214288:0 memset:49200:0 gemm_64x64:6296832:67166208 gemm_64x64:4197888:67166208 tp_op_bwd:27583740:0 op_proj_gemm:18892800:302284800 tp_op_edge_env:4493052:0 gemm_128x64:10494720:134332416 gemm_64x64:4197888:67166208 tp_op_bwd:36274680:0 op_proj_gemm:18892800:302284800 tp_op_edge_env:4493052:0 gemm_192x64:8395776:201498624 gemm_256x64:14692608:268664832 gemm_64x64:4197888:67166208 edge_backward:3312396:0 force_gather:377164:0'),
    'op_proj_auto_large_energy': ('operator/slot',
        'edge_prologue:2787660:0 gemm_64x64:4197888:67166208 gemm_64x256:10494720:268664832 tp_op_moments:2394108:0 op_proj_gemm:18892800:302284800 tp_op_fwd:17842176:0 gemm_128x64:6296832:134332416 tp_op_moments:2394108:0 op_proj_gemm:18892800:302284800 tp_op_fwd:27288576:0 gemm_192x64:8395776:201498624 gemm_192x64:8395776:201498624 readout_reduce:2115344:0'),
    'op_proj_always': ('operator/slot',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_moments:34748:0 op_proj_gemm:184320:2949120 tp_op_fwd:214016:0 gemm_128x64:91392:1949696 tp_op_moments:34748:0 op_proj_gemm:184320:2949120 tp_op_fwd:306176:0 gemm_192x64:121856:2924544 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x64:91392:974848 gemm_64x64:60928:974848 tp_op_bwd:310460:0 op_proj_gemm:184320:2949120 tp_op_edge_env:65212:0 gemm_128x64:152320:1949696 gemm_64x64:60928:974848 tp_op_bwd:436600:0 op_proj_gemm:184320:2949120 tp_op_edge_env:65212:0 gemm_192x64:121856:2924544 gemm_256x64:213248:3899392 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'op_proj_always_energy': ('operator/slot',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_moments:34748:0 op_proj_gemm:184320:2949120 tp_op_fwd:214016:0 gemm_128x64:91392:1949696 tp_op_moments:34748:0 op_proj_gemm:184320:2949120 tp_op_fwd:306176:0 gemm_192x64:121856:2924544 gemm_192x64:121856:2924544 readout_reduce:30624:0'),
    'op_proj_always_single': ('operator/single',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_moments:34748:0 op_proj_gemm:184320:2949120 tp_op_fwd:214016:0 gemm_128x128:121856:3899392 gemm_128x64:91392:1949696 tp_op_moments:65212:0 op_proj_gemm:276480:5898240 tp_op_fwd:306176:0 gemm_192x128:152320:5849088 gemm_128x64:91392:1949696 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x192:121856:2924544 gemm_64x128:152320:1949696 gemm_128x192:213248:5849088 tp_op_bwd:310460:0 op_proj_gemm:276480:5898240 tp_op_edge_env:126140:0 gemm_64x128:213248:1949696 gemm_128x128:152320:3899392 tp_op_bwd:436600:0 op_proj_gemm:184320:2949120 tp_op_edge_env:65212:0 gemm_256x64:182784:3899392 gemm_64x64:91392:974848 gemm_64x64:60928:974848 edge_backward:52360:0 force_gather:5084:0'),
    'op_proj_never_large': ('operator/slot',
        'edge_prologue:2787660:0 gemm_64x64:4197888:67166208 gemm_64x256:10494720:268664832 tp_op_fwd:20236284:0 gemm_128x64:6296832:134332416 tp_op_fwd:29682684:0 gemm_192x64:8395776:201498624 gemm_192x64:8395776:201498624 readout_reduce:4214288:0 memset:49200:0 gemm_64x64:6296832:67166208 gemm_64x64:4197888:67166208 tp_op_bwd:32076792:0 gemm_128x64:10494720:134332416 gemm_64x64:4197888:67166208 tp_op_bwd:40767732:0 gemm_192x64:8395776:201498624 gemm_256x64:14692608:268664832 gemm_64x64:4197888:67166208 edge_backward:3312396:0 force_gather:377164:0'),
    'tp_operator_fused': ('operator/slot',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_fwd:248764:0 gemm_128x64:91392:1949696 tp_op_fwd:340924:0 gemm_192x64:121856:2924544 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x64:91392:974848 gemm_64x64:60928:974848 tp_op_bwd:375672:0 gemm_128x64:152320:1949696 gemm_64x64:60928:974848 tp_op_bwd:501812:0 gemm_192x64:121856:2924544 gemm_256x64:213248:3899392 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
    'tp_operator_fused_proj_always': ('operator/slot',
        'edge_prologue:40460:0 gemm_64x64:60928:974848 gemm_64x256:152320:3899392 tp_op_fwd:248764:0 gemm_128x64:91392:1949696 tp_op_fwd:340924:0 gemm_192x64:121856:2924544 gemm_192x64:121856:2924544 readout_reduce:61088:0 memset:480:0 gemm_64x64:91392:974848 gemm_64x64:60928:974848 tp_op_bwd:375672:0 gemm_128x64:152320:1949696 gemm_64x64:60928:974848 tp_op_bwd:501812:0 gemm_192x64:121856:2924544 gemm_256x64:213248:3899392 gemm_64x64:60928:974848 edge_backward:48076:0 force_gather:5084:0'),
}


def _check_case(lib, case, device):
    stages, e, f, pipeline = run_case(lib, case, device)
    print(case[0], pipeline)
    for s in stages:
        print("   ", s)
    want_pipeline, want = EXPECTED[case[0]]
    assert pipeline == want_pipeline
    assert encode(stages) == want, (case[0], [s[0] for s in stages], [w.split(":")[0] for w in want.split()])
    assert torch.isfinite(e).all() and (f is None or torch.isfinite(f).all())  # (the workspace was poisoned)


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_step_launches_emulation(case):
    from tests.hip_utils import emu_lib

    _check_case(emu_lib(), case, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if not c[4].get("cus_matter")], ids=[c[0] for c in CASES if not c[4].get("cus_matter")])
def test_step_launches_gpu(case):
    assert torch.cuda.is_available()
    _check_case(_lib.load(), case, "cuda:0")


def _names(case_name):
    return [s.split(":")[0] for s in EXPECTED[case_name][1].split()]


def _bytes(case_name, stage):
    return [float(s.split(":")[1]) for s in EXPECTED[case_name][1].split() if s.split(":")[0] == stage]


def test_the_cases_reach_every_kind_of_step():
    by_name = {c[0]: c for c in CASES}
    assert len(by_name) == len(CASES) and set(EXPECTED) == set(by_name)
    # every tensor-product path x linear-layer path of tests/test_plan_pipeline.py (the three per-edge paths show in their launches),
    # with forces and energy only
    reached = set()
    for name, (pipeline, _) in EXPECTED.items():
        tp, linear = pipeline.split("/")
        if tp == "per_edge":
            ns = _names(name)
            tp = "general" if "tp_layer_fwd" in ns else "spec_chain" if "tp_chain_fwd_last" in ns else "spec"
        reached.add((f"{tp}/{linear}", by_name[name][4].get("forces", True)))
    assert reached >= {(p, f) for p in PIPELINES for f in (True, False)}, reached
    # taps, no transposed CSR (atomics: no force_gather), atom block with atom_begin > 0, empty block
    assert any(c[4].get("taps") for c in CASES)
    assert "fused_fwd" not in _names("taps_fused_plan") and "fused_fwd" in _names("fused_mid")
    for n in ("no_tcsr_fused", "no_tcsr_slot", "no_tcsr_general"):
        assert "force_gather" not in _names(n) and "edge_backward" in _names(n)
    assert "force_gather" in _names("fused_mid")
    assert grid_graph(**BLOCK)[1][0].min() == 5
    assert len(grid_graph(**by_name["empty_block_fused_deep"][3])[0]) == 0
    # fused plan: one-tile forward on both sides of the two size bounds (3 emulated CUs) -- the tails show as absent launches
    sizes = {n: by_name[n][3]["n"] for n in ("fused_low", "fused_mid", "fused_big")}
    assert sizes["fused_low"] <= 12 < sizes["fused_mid"] < 192 <= sizes["fused_big"]
    for n in ("fused_low", "fused_mid"):
        assert {"fused_fwd", "tp_mom_bwd_last", "gc_64x128"} <= set(_names(n)), n
    assert "fused_fwd" in _names("fused_big") and not {"tp_mom_bwd_last", "gc_64x128"} & set(_names("fused_big"))
    assert {by_name[n][2].get("fused_narrow") for n in NAMES} >= {1, 2, 3, 4} and {by_name[n][2].get("fused_forward") for n in NAMES} >= {2, 3, 4}
    # chain-only tail (4) against deep tail (2): the latent-0 chain and the layer-1 moments reverse come back
    assert not {"tp_mom_bwd_last", "gc_64x128"} & set(_names("fused_narrow2")) and {"tp_mom_bwd_last", "gc_64x128"} <= set(_names("fused_narrow4"))
    assert len({_bytes(n, "fused_fwd")[0] / by_name[n][3]["n"] for n in ("fused_narrow2", "fused_narrow4", "fused_narrow3")}) == 3
    # mixed form, pure team form, staged-folded (a segment above 128), three species (LDS bound of the team form)
    assert max(np.bincount(grid_graph(**LONG_ATOM)[1][0])) == 36 and "fused_fwd" in _names("one_long_atom")
    assert min(np.bincount(grid_graph(**DENSE)[1][0])) > 32 and "fused_fwd" in _names("small_dense")
    assert max(np.bincount(grid_graph(**VERY_LONG)[1][0])) > 128 and "fused_fwd" not in _names("very_long_atom")
    assert "fused_fwd" in _names("three_species") and "fused_fwd" not in _names("three_species_long_atom")
    # staged folded against unfolded forward chains; the general chain kernel for the latent-0 reverse; readout in two passes
    assert _names("moments_chains_staged") != _names("staged_no_fold") or EXPECTED["moments_chains_staged"] != EXPECTED["staged_no_fold"]
    assert "gc_64x128" in _names("fused_narrow1") and "gc_64x128" in _names("chain_staged_weights")  # (both kernels report this stage)
    assert "readout_backward" in _names("readout_two_pass") and "readout_backward" not in _names("moments_single")
    assert "readout_backward" in _names("readout_two_pass_slot") and "readout_backward" not in _names("operator_slot")
    # env projections of the operator kernels: automatic below / above 4096 atoms, always, never; fused form
    assert by_name["op_proj_auto_large"][3]["n"] > 4096
    assert "op_proj_gemm" not in _names("op_proj_auto_small") and "op_proj_gemm" in _names("op_proj_auto_large")
    assert "op_proj_gemm" in _names("op_proj_always") and "op_proj_gemm" not in _names("op_proj_never_large")
    assert "tp_op_edge_env" in _names("op_proj_always") and "tp_op_edge_env" not in _names("op_proj_always_energy")
    assert "op_proj_gemm" not in _names("tp_operator_fused") and "op_proj_gemm" not in _names("tp_operator_fused_proj_always")


if __name__ == "__main__":
    record(sys.argv[1])
