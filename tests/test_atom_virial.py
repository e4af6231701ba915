"""Per-atom virial (`aa_model_atom_virial`, `HipAllegroModel.atom_virial` / `heat_flux_potential`).

Edge e has center i(e) and neighbor j(e), g_e = dE/dr_e (`dvec`), r_e = unit vector * length (`vec`), W[a][b] = sum g_a r_b:
    center    Wc_n = sum_{e in seg(n)} g_e (x) r_e   (= dE_n/d(strain): every E_n depends on its own edges only)
    neighbor  Wn_n = sum_{e: j(e) = n} g_e (x) r_e   (the tensor of the heat flux)
    split     (Wc_n + Wn_n) / 2
References: an fp64 `index_add` of the outer products of the two taps the step leaves in the workspace, and, for `center`, the
oracle's per-atom energies differentiated with respect to a strain of positions and shift vectors (one backward pass per atom).
Tolerances are the project's: 1e-9 (fp64) / 5e-5 (fp32) times max(1, max |expected|).

`emu`: the unmodified kernels under the CPU emulation; `gpu`: the gfx950 library on the device.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd import graph as G
from allegro_amd.nn import HipAllegroModel, PreparedGraph
from tests.golden_utils import load_model_fixture
from tests.hip_utils import fixture_data, model_from_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {torch.float64: 1e-9, torch.float32: 5e-5}
DTYPES = [pytest.param(torch.float64, id="f64"), pytest.param(torch.float32, id="f32")]
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
ATTRIBUTIONS = ("center", "neighbor", "split")
R_MAX, R_SIO = 3.4, 2.4  # the model's cutoff, and the shortened one of the Si-O pairs
SPECIES = ["Si", "O", "H"]
ISOLATED, LOPSIDED = 13, 12  # the atom of degree 0; the atom that is listed as a neighbor more often than it lists neighbors


def _backend(name):
    if name == "emu":
        from tests.hip_utils import emu_lib

        return emu_lib(), torch.device("cpu")
    return _lib.load(), torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# the frame
# ---------------------------------------------------------------------------------------------------------------------
_FRAME = None


def frame():
    """14 atoms of three species around a corner of a 60 A box, wrapped into it (most edges cross the periodic boundary), one of
    them far away from the rest.  Three of atom 12's own edges are taken off the list (a directed list need not be symmetric:
    every E_n is a function of the edges of n alone), so that its transposed group is larger than its segment."""
    global _FRAME
    if _FRAME is None:
        rng = np.random.default_rng(2)
        pos = rng.uniform(-2.9, 2.9, size=(14, 3))
        pos[ISOLATED] = [30.0, 30.0, 30.0]
        pos = np.mod(pos, 60.0)
        types = rng.integers(0, 3, size=14)
        cell = np.eye(3) * 60.0
        ei, cs = G.neighbor_list_pbc(pos, cell, R_MAX)
        own = np.flatnonzero(ei[0] == LOPSIDED)
        keep = np.ones(ei.shape[1], dtype=bool)
        keep[own[:3]] = False
        ei, cs = ei[:, keep], cs[keep]
        deg = np.bincount(ei[0], minlength=14)
        indeg = np.bincount(ei[1], minlength=14)
        assert deg[ISOLATED] == 0 and indeg[ISOLATED] == 0              # one atom of degree 0
        assert deg.max() > 8 and indeg.max() > 8                        # a lane takes more than one edge, in either pass
        assert (deg % 2 == 1).any() and (indeg % 2 == 1).any()          # odd degrees
        assert indeg[LOPSIDED] > deg[LOPSIDED] > 0                      # transposed group larger than the segment
        assert (np.abs(cs).sum(-1) != 0).any() and (np.abs(cs).sum(-1) == 0).any()  # periodic and plain edges
        assert len(set(types.tolist())) == 3
        r = np.linalg.norm(pos[ei[1]] - pos[ei[0]] + cs @ cell, axis=1)
        sio = ((types[ei[0]] == 0) & (types[ei[1]] == 1)) | ((types[ei[0]] == 1) & (types[ei[1]] == 0))
        assert (sio & (r >= R_SIO)).any()                               # listed edges beyond their pair's shortened cutoff
        _FRAME = dict(pos=pos, types=types, cell=cell, ei=ei, cs=cs, deg=deg, indeg=indeg)
    return _FRAME


def cfg_for(dtype, pair=True, species=3, **over):
    """`species=1`: the same frame with every atom Si (no shortened pair cutoff left): the shape on which the plan takes the
    two-waves-per-SIMD form of the fused forward, whose two-body table has to leave its LDS to eight waves."""
    fr = frame()
    names = SPECIES[:species]
    cfg = dict(type_names=list(names), r_max=R_MAX, l_max=2, num_layers=2, num_scalar_features=64, num_tensor_features=64,
               radial_chemical_embed={"_target_": "allegro.nn.TwoBodyBesselScalarEmbed", "num_bessels": 8, "polynomial_cutoff_p": 6},
               per_edge_type_cutoff={"Si": {"O": R_SIO}, "O": {"Si": R_SIO}}, avg_num_neighbors=float(fr["deg"].mean()), seed=11,
               model_dtype={torch.float32: "float32", torch.float64: "float64"}[dtype])
    if species < 3:
        del cfg["per_edge_type_cutoff"]
    cfg.update(over)
    if pair:
        cfg["pair_potential"] = {"_target_": "nequip.nn.pair_potential.ZBL", "units": "metal", "chemical_species": list(names)}
    return cfg


def build(cfg, lib, dev):
    m = HipAllegroModel(**cfg).to(dev)
    m._bind_library(lib)
    return m


def frame_tensors(dtype, dev, species=3):
    fr = frame()
    pos = torch.tensor(fr["pos"], dtype=dtype, device=dev)
    shift = torch.tensor(fr["cs"] @ fr["cell"], dtype=dtype, device=dev)
    types = torch.tensor(fr["types"] % species, device=dev)
    return pos, torch.tensor(fr["ei"], device=dev), types, shift


def tap_reference(m, g):
    """fp64, from the taps of the last step: dict of the three [N,3,3] tensors, plus g_e [E,3] and r_e [E,3]."""
    d = m.debug_tap("dvec", g, with_forces=True)[:, :3].double()
    v = m.debug_tap("vec", g, with_forces=True).double()
    r = v[:, :3] * v[:, 3:4]
    outer = d.unsqueeze(2) * r.unsqueeze(1)  # [E,3,3]: (g_e)_a (r_e)_b
    zero = torch.zeros(g.num_atoms, 3, 3, dtype=torch.float64, device=d.device)
    wc = zero.index_add(0, g.center.long(), outer)
    wn = zero.index_add(0, g.nbr.long(), outer)
    return {"center": wc, "neighbor": wn, "split": 0.5 * (wc + wn)}, d, r


def assert_close(name, got, want, dtype):
    scale = max(1.0, float(want.abs().max()))
    err = float((got.double() - want.to(got.device)).abs().max())
    print(f"{name}: max|got - expected| = {err:.3e}, bound {TOL[dtype] * scale:.3e} (max|expected| {float(want.abs().max()):.3e})")
    assert err <= TOL[dtype] * scale, name


_STEPPED = {}


def stepped(backend, dtype):
    """One model with the ZBL term, one step with forces on the frame in the default forward (shared: the tests below only read it
    or repeat the same step)."""
    if (backend, dtype) not in _STEPPED:
        lib, dev = _backend(backend)
        pos, ei, types, shift = frame_tensors(dtype, dev)
        m = build(cfg_for(dtype), lib, dev)
        g = PreparedGraph(ei, types, pos.shape[0], shift, lib=lib)
        m.energy_forces(pos, g)
        _STEPPED[(backend, dtype)] = (m, g, pos, lib)
    return _STEPPED[(backend, dtype)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the taps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("species,dtype", [pytest.param(3, torch.float64, id="3-f64"), pytest.param(3, torch.float32, id="3-f32"),
                                           pytest.param(1, torch.float32, id="1-f32")])
def test_matches_the_taps(backend, species, dtype, forward_mode):
    """Which forward left the buffers is asserted per mode on the plan and on the step's launch list: fp64 runs the staged
    stages in every mode; in fp32 "staged" does and the other two run the fused forward.  The two-waves-per-SIMD form (aa_fused8.hip)
    exists for one species, so the three-species frame takes the one-wave-per-SIMD kernel in "auto" and in "wide" alike, and its
    one-species variant is what puts the call behind the wide form: "auto" as four-wave workgroups with every reverse stage a
    launch of its own, "wide" as eight-wave workgroups whose tail has already run the reverse down to the latent-0 chain."""
    lib, dev = _backend(backend)
    pos, ei, types, shift = frame_tensors(dtype, dev, species)
    assert len(set(types.tolist())) == species
    m = build(cfg_for(dtype, species=species), lib, dev)
    plan = m.describe_plan()
    assert plan["pair"] == "zbl"
    g = PreparedGraph(ei, types, pos.shape[0], shift, lib=lib)
    launches, _, _ = _stage_names(m, lib, pos, g)
    fused = dtype == torch.float32 and forward_mode != "staged"
    assert ("fused_fwd" in launches) == fused and ("edge_prologue" in launches) == (not fused), launches
    assert plan["fused_wide"] == (fused and species == 1), plan
    if dtype == torch.float32:  # (fp64 is the operator pipeline: no moments kernels at all)
        assert ("tp_mom_bwd_last" in launches) == (not (plan["fused_wide"] and forward_mode == "wide")), launches
    assert "force_gather" in launches and "atom_virial" not in launches
    m.energy_forces(pos, g)
    ref, _, _ = tap_reference(m, g)
    assert float(ref["center"].abs().max()) > 1e-3 and float((ref["center"] - ref["neighbor"]).abs().max()) > 1e-3
    for attribution in ATTRIBUTIONS:
        w = m.atom_virial(g, attribution)
        assert w.shape == (14, 3, 3) and w.dtype == dtype
        assert_close(f"{attribution} ({forward_mode})", w, ref[attribution], dtype)
        assert float(w[ISOLATED].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the oracle: Wc_n = dE_n/d(strain)
# ---------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_atom_strain_derivative(name, dtype):
    """[N,3,3] fp64: the gradient of the oracle's E_n with respect to a strain eps applied to positions and shift vectors
    (x -> x + x @ eps^T, the construction of oracle.restatement.allegro_virial), one backward pass per atom."""
    if (name, dtype) not in _ORACLE:
        from oracle import restatement as R

        fx = load_model_fixture(name, dtype)
        cfg = dict(fx["cfg"], model_dtype="float64")
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in fx["sd"].items()}
        pos = fx["pos"].double()
        sv = None if fx["shift_vec"] is None else fx["shift_vec"].double()
        eps = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
        e_atom = R.allegro_energy(cfg, sd, pos + pos @ eps.T, fx["edge_index"], fx["types"],
                                  None if sv is None else sv + sv @ eps.T).reshape(-1)
        rows = [torch.autograd.grad(e_atom[n], eps, retain_graph=True)[0] for n in range(e_atom.shape[0])]
        _ORACLE[(name, dtype)] = torch.stack(rows)
    return _ORACLE[(name, dtype)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name,dtype,tol", [("t_coupled", torch.float64, 1e-9), ("c2", torch.float32, 5e-5)])
def test_center_matches_oracle_strain_derivative(backend, name, dtype, tol):
    lib, dev = _backend(backend)
    fx = load_model_fixture(name, dtype)
    assert "pair_potential" not in fx["cfg"]
    m = model_from_fixture(fx, dtype, lib, dev)
    data, sv = fixture_data(fx, dtype, dev)
    g = m.prepare_graph(data["edge_index"], data["atom_types"], data["pos"].shape[0], sv)
    m.energy_forces(data["pos"], g)
    w = m.atom_virial(g, "center").cpu()
    ref = oracle_atom_strain_derivative(name, dtype)
    scale = max(1.0, float(ref.abs().max()))
    err = float((w.double() - ref).abs().max())
    print(f"{name}: max|Wc - dE_n/d eps| = {err:.3e}, bound {tol * scale:.3e} (max|expected| {float(ref.abs().max()):.3e})")
    assert err <= tol * scale


# ---------------------------------------------------------------------------------------------------------------------
# 3. sum rule, 4. reproducibility
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_to_the_total_virial(backend, dtype):
    m, g, _, _ = stepped(backend, dtype)
    total = m.virial(g).double()
    for attribution in ATTRIBUTIONS:
        assert_close(f"sum over atoms, {attribution}", m.atom_virial(g, attribution).double().sum(0), total, dtype)


@pytest.mark.parametrize("backend", BACKENDS)
def test_bit_reproducible(backend):
    m, g, pos, _ = stepped(backend, torch.float32)
    runs = []
    for _ in range(2):
        m.energy_forces(pos, g)
        runs.append([m.atom_virial(g, a).clone() for a in ATTRIBUTIONS])
    for a, first, second in zip(ATTRIBUTIONS, *runs):
        assert torch.equal(first, second), a


# ---------------------------------------------------------------------------------------------------------------------
# 5. ghost layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_layout(backend, dtype):
    """pair_allegro layout: ghost atoms are nobody's center (zero Wc) and carry the neighbor share of the edges that point at them."""
    lib, dev = _backend(backend)
    fr = frame()
    gg = G.to_ghost_layout(G.Graph(pos=fr["pos"], types=fr["types"], edge_index=fr["ei"], cell=fr["cell"], cell_shift=fr["cs"]))
    assert gg.num_atoms > 14
    pos = torch.tensor(gg.pos, dtype=dtype, device=dev)
    m = build(cfg_for(dtype), lib, dev)
    g = m.prepare_graph(torch.tensor(gg.edge_index, device=dev), torch.tensor(gg.types, device=dev), gg.num_atoms, None)
    m.energy_forces(pos, g)
    ref, _, _ = tap_reference(m, g)
    wc, wn = m.atom_virial(g, "center"), m.atom_virial(g, "neighbor")
    assert float(wc[14:].abs().max()) == 0.0
    # every ghost is the neighbor of exactly one edge; its row is non-zero unless that edge is a Si-O one beyond the pair's shortened
    # cutoff, which the list (built at r_max) holds and which contributes exactly 0 to everything
    ghost_edge = torch.argsort(g.nbr.long())[-(gg.num_atoms - 14):]
    assert torch.equal(g.nbr[ghost_edge].long().cpu(), torch.arange(14, gg.num_atoms))
    ci, nj = g.center[ghost_edge].long(), g.nbr[ghost_edge].long()
    tc, tn = g.types[ci], g.types[nj]
    beyond = (((tc == 0) & (tn == 1)) | ((tc == 1) & (tn == 0))) & ((pos[nj] - pos[ci]).double().norm(dim=-1) >= R_SIO)
    assert int((~beyond).sum()) >= 10
    assert torch.equal(wn[14:].abs().amax(dim=(1, 2)) > 0, ~beyond)
    assert_close("ghost layout, center", wc, ref["center"], dtype)
    assert_close("ghost layout, neighbor", wn, ref["neighbor"], dtype)
    assert_close("ghost layout, neighbor, ghost rows", wn[14:], ref["neighbor"][14:], dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 6. heat flux
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_heat_flux_potential(backend, dtype):
    m, g, pos, _ = stepped(backend, dtype)
    _, d, r = tap_reference(m, g)
    vel = torch.randn(14, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(pos.device)
    want = -(r * (d * vel[g.nbr.long()]).sum(-1, keepdim=True)).sum(0)  # -sum_e r_e (g_e . v_j(e))
    got = m.heat_flux_potential(g, vel.to(dtype))
    assert got.shape == (3,) and got.dtype == dtype
    assert_close("heat flux, random velocities", got, want, dtype)
    v0 = torch.tensor([0.3, -1.1, 0.7], dtype=torch.float64, device=pos.device)
    got0 = m.heat_flux_potential(g, v0.to(dtype).expand(14, 3))
    assert_close("heat flux, one common velocity", got0, -(v0 @ m.virial(g).double()), dtype)
    with pytest.raises(ValueError, match="velocities"):
        m.heat_flux_potential(g, vel[:5].to(dtype))


# ---------------------------------------------------------------------------------------------------------------------
# 7. guards
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_guards(backend):
    lib, dev = _backend(backend)
    dtype = torch.float64
    pos, ei, types, shift = frame_tensors(dtype, dev)
    over = dict(num_scalar_features=16, num_tensor_features=8)  # (a small model: the guards do not depend on its size)
    m = build(cfg_for(dtype, **over), lib, dev)
    g = PreparedGraph(ei, types, 14, shift, lib=lib)
    g_at = PreparedGraph(ei, types, 14, shift, transposed=False, lib=lib)
    assert g.t_perm is not None and g_at.t_perm is None
    # a workspace sized for an energy-only step (what a C host allocates for one) is too small
    m.energy_forces(pos, g, with_forces=False)
    need0 = lib.lib.aa_model_workspace_bytes(m._plan_handle, g.num_atoms, g.num_edges, 0)
    need1 = lib.lib.aa_model_workspace_bytes(m._plan_handle, g.num_atoms, g.num_edges, 1)
    assert need0 < need1
    m._workspace = m._workspace[:need0]
    with pytest.raises(_lib.AllegroError, match="workspace too small"):
        m.atom_virial(g, "center")
    m.energy_forces(pos, g)
    ref, _, _ = tap_reference(m, g)
    assert_close("center after the refused call", m.atom_virial(g, "center"), ref["center"], dtype)
    # an unknown attribution: in Python and on the C ABI
    with pytest.raises(ValueError, match="attribution"):
        m.atom_virial(g, "pairwise")
    with pytest.raises(ValueError, match="attribution"):
        m.atom_virial(g, 1)
    out = torch.full((14, 3, 3), 7.0, dtype=dtype, device=dev)
    gs = g.c_struct()
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    for bad in (-1, 3):
        rc = lib.lib.aa_model_atom_virial(m._plan_handle, C.byref(gs), m._workspace.data_ptr(), m._workspace.numel(), bad, out.data_ptr(), stream)
        assert rc == -1 and b"attribution" in lib.lib.aa_last_error()  # AA_ERR_INVALID
    assert float((out - 7.0).abs().max()) == 0.0  # (a refused call writes nothing)
    assert_close("neighbor after the refused calls", m.atom_virial(g, "neighbor"), ref["neighbor"], dtype)
    # without the transposed CSR: center works, neighbor and split are refused (no atomics fallback)
    m.energy_forces(pos, g_at)
    ref_at, _, _ = tap_reference(m, g_at)
    for attribution in ("neighbor", "split"):
        with pytest.raises(_lib.AllegroError, match="transposed CSR"):
            m.atom_virial(g_at, attribution)
    assert_close("center without the transposed CSR", m.atom_virial(g_at, "center"), ref_at["center"], dtype)
    assert_close("center with and without it", m.atom_virial(g_at, "center"), ref["center"], dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 8. nothing else moved
# ---------------------------------------------------------------------------------------------------------------------
def _stage_names(m, lib, pos, g):
    L = lib.lib
    L.aa_model_energy_forces_profiled.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_lib.Graph), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_char_p, C.POINTER(C.c_int),
                                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]
    m.energy_forces(pos, g)  # (the plan, the blob and a workspace for a step with forces)
    ms, names, n = (C.c_float * 256)(), C.create_string_buffer(256 * 32), C.c_int()
    e = torch.empty(pos.shape[0], dtype=pos.dtype, device=pos.device)
    f = torch.empty((pos.shape[0], 3), dtype=pos.dtype, device=pos.device)
    gs = g.c_struct()
    stream = torch.cuda.current_stream(pos.device).cuda_stream if pos.is_cuda else None
    lib.check(L.aa_model_energy_forces_profiled(m._plan_handle, m._blob.data_ptr(), C.byref(gs), pos.data_ptr(), m._workspace.data_ptr(),
                                                m._workspace.numel(), e.data_ptr(), f.data_ptr(), stream, 256, ms, names, C.byref(n), None, None),
              "aa_model_energy_forces_profiled")
    return [names.raw[32 * i: 32 * i + 32].split(b"\0")[0].decode() for i in range(n.value)], e, f


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
    assert "atom_virial" not in stages0 and "force_gather" in stages0
    for attribution in ATTRIBUTIONS:
        m.atom_virial(g, attribution)
    assert m.describe_plan() == plan0
    stages1, e1, f1 = _stage_names(m, lib, pos, g)
    assert stages1 == stages0
    assert torch.equal(e1, e0) and torch.equal(f1, f0)


def test_symbol_is_declared_in_both_header_copies_and_exported():
    from allegro_amd.build import INCLUDE_DIR, build_library

    lib_path = build_library(verbose=False)  # (also generates the package's copy of the header)
    for path in (os.path.join(ROOT, "include", "allegro_amd.h"), os.path.join(INCLUDE_DIR, "allegro_amd.h")):
        src = open(path).read()
        assert "int aa_model_atom_virial(" in src, path
        for name in ("AA_ATOM_VIRIAL_CENTER", "AA_ATOM_VIRIAL_NEIGHBOR", "AA_ATOM_VIRIAL_SPLIT"):
            assert name in src, (path, name)
    assert hasattr(C.CDLL(lib_path), "aa_model_atom_virial")
