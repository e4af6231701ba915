"""Potential part of the Green-Kubo heat flux as one streaming reduction (`aa_model_heat_flux`, `aa_model_blocked_heat_flux`,
`HipAllegroModel.heat_flux_potential`).

Edge e has center i(e) and neighbor j(e), g_e = dE/dr_e (`dvec`), r_e = unit vector * length (`vec`):
    J_pot[b] = -sum_e (r_e)_b (g_e . v_j(e))
References: the fp64 sum of exactly those products from the two taps the step leaves in the workspace (with a DERIVED bound: the
kernel forms the same products in double, adds them in double and rounds once), `-(v0 @ virial)` for one common velocity, the
einsum of the neighbor-attributed per-atom virial, and the oracle's total energy differentiated with respect to a vector t that
displaces every edge vector by v_j(e) (r_e . t).  Tolerances are the project's: 1e-9 (fp64) / 5e-5 (fp32) times max(1, max |expected|).

`emu`: the unmodified kernels under the CPU emulation; `gpu`: the gfx950 library on the device.
"""
import ctypes as C
import os

import pytest
import torch

from allegro_amd import _lib
from allegro_amd import graph as G
from allegro_amd.nn import HipAllegroModel, PreparedGraph
from tests.golden_utils import load_model_fixture
from tests.hip_utils import fixture_data, model_from_fixture
from tests.test_atom_virial import (BACKENDS, DTYPES, TOL, _backend, _stage_names, assert_close, build, cfg_for, frame,
                                    frame_tensors, stepped)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
# aa_model_workspace_bytes(plan, 14, E of the frame, with_forces = 0 / 1) of the model `cfg_for(dtype)`, as returned by the commit
# before this entry point existed (the flux borrows the virial's scratch: the layout must not move)
WORKSPACE_BYTES = {torch.float32: (316416, 609536), torch.float64: (824576, 1631488)}


def velocities(n, dtype, dev, seed=3):
    """[n,3] random, already rounded to the model dtype."""
    return torch.randn(n, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


def tap_flux(m, g, vel):
    """fp64 from the taps of the last step: (want [3], A [3]) with A_b = sum_e |(r_e)_b| sum_a |g_e[a] v_j[a]|."""
    d = m.debug_tap("dvec", g, with_forces=True)[:, :3].double()
    v = m.debug_tap("vec", g, with_forces=True).double()
    r = v[:, :3] * v[:, 3:4]
    p = d * vel.double()[g.nbr.long()]
    want = -(r * p.sum(-1, keepdim=True)).sum(0)
    return want, (r.abs() * p.abs().sum(-1, keepdim=True)).sum(0)


def assert_derived(name, got, want, A, num_edges, dtype):
    """|got_b - want_b| <= 2 eps(dtype) |want_b| + 4 E 2^-53 A_b: one rounding to the model dtype (with room for the reference's own
    last place), and E additions of products of three factors in double on either side."""
    err = (got.double() - want).abs()
    bound = 2 * EPS[dtype] * want.abs() + 4 * num_edges * 2.0 ** -53 * A
    print(f"{name}: |got - expected| = {[f'{x:.3e}' for x in err.tolist()]}, bound {[f'{x:.3e}' for x in bound.tolist()]} "
          f"(expected {[f'{x:.3e}' for x in want.tolist()]})")
    assert bool((err <= bound).all()), name


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the step's own per-edge data
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_matches_the_taps(backend, dtype):
    m, g, pos, _ = stepped(backend, dtype)
    m.energy_forces(pos, g)
    vel = velocities(14, dtype, pos.device)
    got = m.heat_flux_potential(g, vel)
    assert got.shape == (3,) and got.dtype == dtype
    want, A = tap_flux(m, g, vel)
    assert float(want.abs().max()) > 1e-3
    assert_derived("random velocities", got, want, A, g.num_edges, dtype)
    v0 = torch.tensor([0.3, -1.1, 0.7], dtype=torch.float64, device=pos.device)
    got0 = m.heat_flux_potential(g, v0.to(dtype).expand(14, 3))
    assert_close("one common velocity", got0, -(v0.to(dtype).double() @ m.virial(g).double()), dtype)
    assert_close("the einsum of the neighbor tensor", got, -torch.einsum("na,nab->b", vel.double(), m.atom_virial(g, "neighbor").double()),
                 dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def oracle_flux(fx, vel):
    """-dE_total/dt at t = 0 of the oracle's energy with every edge vector displaced by v_j(e) (r_e . t), in fp64."""
    from oracle import restatement as R

    cfg = dict(fx["cfg"], model_dtype="float64")
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in fx["sd"].items()}
    pos, ei = fx["pos"].double(), fx["edge_index"]
    sv = torch.zeros(ei.shape[1], 3, dtype=torch.float64) if fx["shift_vec"] is None else fx["shift_vec"].double()
    r = (pos[ei[1]] - pos[ei[0]] + sv).detach()
    t = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    e = R.allegro_energy(cfg, sd, pos, ei, fx["types"], sv + vel.double()[ei[1]] * (r @ t).unsqueeze(-1)).sum()
    return -torch.autograd.grad(e, t)[0]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name,dtype,tol", [("t_coupled", torch.float64, 1e-9), ("c2", torch.float32, 5e-5)])
def test_matches_the_oracle_derivative(backend, name, dtype, tol):
    lib, dev = _backend(backend)
    fx = load_model_fixture(name, dtype)
    m = model_from_fixture(fx, dtype, lib, dev)
    data, sv = fixture_data(fx, dtype, dev)
    n = data["pos"].shape[0]
    g = m.prepare_graph(data["edge_index"], data["atom_types"], n, sv)
    m.energy_forces(data["pos"], g)
    vel = velocities(n, dtype, "cpu", seed=5)
    got = m.heat_flux_potential(g, vel.to(dev)).cpu()
    want = oracle_flux(fx, vel)
    scale = max(1.0, float(want.abs().max()))
    err = float((got.double() - want).abs().max())
    print(f"{name}: max|J - (-dE/dt)| = {err:.3e}, bound {tol * scale:.3e} (max|expected| {float(want.abs().max()):.3e})")
    assert err <= tol * scale


# ---------------------------------------------------------------------------------------------------------------------
# 3. a graph without a transposed CSR, 4. ghost layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_without_a_transposed_csr(backend, dtype):
    m, g, pos, lib = stepped(backend, dtype)
    _, ei, types, shift = frame_tensors(dtype, pos.device)
    g_at = PreparedGraph(ei, types, 14, shift, transposed=False, lib=lib)
    assert g.t_perm is not None and g_at.t_perm is None
    vel = velocities(14, dtype, pos.device)
    m.energy_forces(pos, g)
    with_t = m.heat_flux_potential(g, vel).clone()
    m.energy_forces(pos, g_at)
    without = m.heat_flux_potential(g_at, vel)
    assert float(with_t.abs().max()) > 1e-3
    assert_close("with and without the transposed CSR", without, with_t.double(), dtype)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_layout(backend, dtype):
    """pair_allegro layout: every periodic image is a ghost atom of its own, whose velocity row is its source atom's.  (The two forms
    see different inputs in fp32: the periodic one rounds pos_j - pos_i, then adds the shift; the ghost one rounds pos_j + shift first,
    at coordinates of up to 60 A, under a ZBL core -- 1.2e-3 of a bound of 2.3e-3 in fp32, 1e-12 in fp64, on the device and emulated.)"""
    import numpy as np

    m, g, pos, lib = stepped(backend, dtype)
    dev = pos.device
    fr = frame()
    vel = velocities(14, dtype, dev)
    m.energy_forces(pos, g)
    periodic = m.heat_flux_potential(g, vel).clone()
    gg = G.to_ghost_layout(G.Graph(pos=fr["pos"], types=fr["types"], edge_index=fr["ei"], cell=fr["cell"], cell_shift=fr["cs"]))
    assert gg.num_atoms > 14
    # one ghost per edge that leaves the cell, in the order of those edges: its source atom is that edge's neighbor (checked: a lattice
    # translate of it, of the same type)
    source = fr["ei"][1][np.abs(fr["cs"]).sum(-1) != 0]
    assert source.size == gg.num_atoms - 14 and (gg.types[14:] == fr["types"][source]).all()
    frac = (gg.pos[14:] - fr["pos"][source]) / 60.0
    assert np.abs(frac - np.round(frac)).max() < 1e-12 and np.abs(np.round(frac)).sum(-1).min() >= 1
    vel_g = torch.cat([vel, vel[torch.tensor(source, device=dev)]])
    gl = m.prepare_graph(torch.tensor(gg.edge_index, device=dev), torch.tensor(gg.types, device=dev), gg.num_atoms, None)
    m.energy_forces(torch.tensor(gg.pos, dtype=dtype, device=dev), gl)
    got = m.heat_flux_potential(gl, vel_g)
    assert_close("ghost layout against the periodic form", got, periodic.double(), dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 5. blocked
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_blocked(backend, dtype):
    m, g, pos, lib = stepped(backend, dtype)
    vel = velocities(14, dtype, pos.device)
    m.energy_forces(pos, g)
    ref = m.heat_flux_potential(g, vel).clone()
    cap = 3 * g.max_degree
    ba, _ = g.blocks(cap)
    assert len(ba) - 1 >= 3
    runs = []
    for _ in range(2):
        m.energy_forces(pos, g, max_block_edges=cap)
        runs.append(m.heat_flux_potential(g, vel).clone())
    assert_close("blocked against unblocked", runs[0], ref.double(), dtype)
    assert torch.equal(runs[0], runs[1])
    # a blocked step without a transposed CSR cannot give forces; its energy-only form leaves nothing to read
    m.energy_forces(pos, g, with_forces=False, max_block_edges=cap)
    with pytest.raises(RuntimeError, match="energy-only"):
        m.heat_flux_potential(g, vel)
    m.energy_forces(pos, g)
    assert torch.equal(m.heat_flux_potential(g, vel), ref)


# ---------------------------------------------------------------------------------------------------------------------
# 6. size edges of the reduction
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_edges_gives_zeros(backend, dtype):
    lib, dev = _backend(backend)
    m = build(cfg_for(dtype, num_scalar_features=16, num_tensor_features=8), lib, dev)
    pos = torch.tensor([[1.0, 2.0, 3.0]], dtype=dtype, device=dev)
    g = PreparedGraph(torch.zeros((2, 0), dtype=torch.long, device=dev), torch.tensor([1], device=dev), 1, None, lib=lib)
    assert g.num_edges == 0
    m.energy_forces(pos, g)
    got = m.heat_flux_potential(g, torch.ones(1, 3, dtype=dtype, device=dev))
    assert got.shape == (3,) and float(got.abs().max()) == 0.0


@pytest.mark.parametrize("backend", BACKENDS)
def test_several_blocks_c2(backend):
    """1 792 edges: seven blocks of 256 lanes (the 14-atom frame of the tests above is one partly filled block)."""
    lib, dev = _backend(backend)
    dtype = torch.float32
    fx = load_model_fixture("c2", dtype)
    m = model_from_fixture(fx, dtype, lib, dev)
    data, sv = fixture_data(fx, dtype, dev)
    n = data["pos"].shape[0]
    g = m.prepare_graph(data["edge_index"], data["atom_types"], n, sv)
    assert g.num_edges == 1792
    m.energy_forces(data["pos"], g)
    vel = velocities(n, dtype, dev, seed=7)
    got = m.heat_flux_potential(g, vel)
    want, A = tap_flux(m, g, vel)
    assert_derived("c2", got, want, A, g.num_edges, dtype)


@pytest.mark.gpu
def test_more_edges_than_lanes_c3():
    """2.98e5 edges > 512 blocks x 256 lanes: every lane takes more than one edge, the grid is at its cap."""
    import bench

    dev = torch.device("cuda:0")
    w, cfg = bench.make_workload("c3")
    m = HipAllegroModel(**cfg).to(dev)
    g = PreparedGraph(torch.tensor(w.edge_index, device=dev), torch.tensor(w.types, device=dev), w.num_atoms,
                      torch.tensor(w.shift_vec(), dtype=torch.float32, device=dev))
    assert g.num_edges > 512 * 256
    m.energy_forces(torch.tensor(w.pos, dtype=torch.float32, device=dev), g)
    vel = velocities(w.num_atoms, torch.float32, dev, seed=9)
    got = m.heat_flux_potential(g, vel)
    want, A = tap_flux(m, g, vel)
    assert_derived("c3", got, want, A, g.num_edges, torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 7. reproducibility
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_bit_reproducible(backend):
    m, g, pos, _ = stepped(backend, torch.float32)
    vel = velocities(14, torch.float32, pos.device)
    runs = []
    for _ in range(2):
        m.energy_forces(pos, g)
        runs.append(m.heat_flux_potential(g, vel).clone())
    assert torch.equal(runs[0], runs[1])


# ---------------------------------------------------------------------------------------------------------------------
# 8. guards
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_guards(backend):
    lib, dev = _backend(backend)
    dtype = torch.float64
    pos, ei, types, shift = frame_tensors(dtype, dev)
    m = build(cfg_for(dtype, num_scalar_features=16, num_tensor_features=8), lib, dev)  # (a small model: the guards do not depend on its size)
    g = PreparedGraph(ei, types, 14, shift, lib=lib)
    vel = velocities(14, dtype, dev)
    with pytest.raises(RuntimeError, match="call energy_forces first"):
        m.heat_flux_potential(g, vel)
    m.energy_forces(pos, g)
    ref = m.heat_flux_potential(g, vel).clone()
    with pytest.raises(ValueError, match="velocities"):
        m.heat_flux_potential(g, vel[:5])
    with pytest.raises(ValueError, match="velocities"):
        m.heat_flux_potential(g, vel.reshape(3, 14))
    out = torch.full((3,), 7.0, dtype=dtype, device=dev)
    gs = g.c_struct()
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    L, ws = lib.lib, m._workspace
    cap = g.num_edges
    for v_ptr, o_ptr in ((None, out.data_ptr()), (vel.data_ptr(), None)):
        assert L.aa_model_heat_flux(m._plan_handle, C.byref(gs), ws.data_ptr(), ws.numel(), v_ptr, o_ptr, stream) == -1  # AA_ERR_INVALID
        assert L.aa_model_blocked_heat_flux(m._plan_handle, C.byref(gs), cap, ws.data_ptr(), ws.numel(), v_ptr, o_ptr, stream) == -1
    # a workspace sized for an energy-only step (what a C host allocates for one) is too small
    need0 = L.aa_model_workspace_bytes(m._plan_handle, g.num_atoms, g.num_edges, 0)
    assert need0 < L.aa_model_workspace_bytes(m._plan_handle, g.num_atoms, g.num_edges, 1)
    assert L.aa_model_heat_flux(m._plan_handle, C.byref(gs), ws.data_ptr(), need0, vel.data_ptr(), out.data_ptr(), stream) == -2  # AA_ERR_WORKSPACE
    assert b"workspace too small" in L.aa_last_error()
    assert L.aa_model_blocked_heat_flux(m._plan_handle, C.byref(gs), cap, ws.data_ptr(), need0, vel.data_ptr(), out.data_ptr(), stream) == -2
    assert b"workspace too small" in L.aa_last_error()
    full = m._workspace
    m._workspace = full[:need0]
    with pytest.raises(_lib.AllegroError, match="workspace too small"):
        m.heat_flux_potential(g, vel)
    m._workspace = full
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0  # (a refused call writes nothing)
    assert torch.equal(m.heat_flux_potential(g, vel), ref)


# ---------------------------------------------------------------------------------------------------------------------
# 9. nothing else moved
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_step_is_unchanged_by_the_call(backend):
    lib, dev = _backend(backend)
    dtype = torch.float32
    pos, ei, types, shift = frame_tensors(dtype, dev)
    m = build(cfg_for(dtype), lib, dev)
    g = PreparedGraph(ei, types, 14, shift, lib=lib)
    e0, f0 = (t.clone() for t in m.energy_forces(pos, g))
    plan0 = dict(m.describe_plan())
    stages0, _, _ = _stage_names(m, lib, pos, g)
    assert "force_gather" in stages0 and not any("heat" in s for s in stages0)
    m.heat_flux_potential(g, velocities(14, dtype, dev))
    assert m.describe_plan() == plan0
    stages1, e1, f1 = _stage_names(m, lib, pos, g)
    assert stages1 == stages0
    assert torch.equal(e1, e0) and torch.equal(f1, f0)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_workspace_size_is_unchanged(backend, dtype):
    m, g, _, lib = stepped(backend, dtype)
    sizes = tuple(lib.lib.aa_model_workspace_bytes(m._plan_handle, 14, g.num_edges, f) for f in (0, 1))
    print(f"aa_model_workspace_bytes(14 atoms, {g.num_edges} edges): {sizes}")
    assert sizes == WORKSPACE_BYTES[dtype]


# ---------------------------------------------------------------------------------------------------------------------
# 10. symbols
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_in_both_header_copies_and_exported():
    from allegro_amd.build import INCLUDE_DIR, build_library

    lib_path = build_library(verbose=False)  # (also generates the package's copy of the header)
    lib = C.CDLL(lib_path)
    for path in (os.path.join(ROOT, "include", "allegro_amd.h"), os.path.join(INCLUDE_DIR, "allegro_amd.h")):
        src = open(path).read()
        for name in ("aa_model_heat_flux", "aa_model_blocked_heat_flux"):
            assert f"int {name}(" in src, (path, name)
    for name in ("aa_model_heat_flux", "aa_model_blocked_heat_flux"):
        assert hasattr(lib, name), name
