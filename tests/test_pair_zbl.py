"""ZBL pair potential (`pair_potential=` of HipAllegroModel: nequip.nn.pair_potential.ZBL = LAMMPS pair_style zbl) on the
inference and training paths.

Oracle: the closed form below, in fp64 with plain torch -- forces by autograd with respect to the positions, the strain
derivative by autograd with respect to a symmetric strain applied to positions and shift vectors.  Every check runs the same
model (identical weights: the `seed=` constructor argument), library and forward mode twice, with and without the pair
potential, and asserts  (with - without) == closed form  -- which isolates the new term from the model's own rounding.
Tolerances are the project's: 1e-9 (fp64) / 5e-5 (fp32) times max(1, max |expected total|), the total being what the step with
the pair potential returns (the model's own part + the closed form).

`emu`: the unmodified kernels under the CPU emulation; `gpu`: the gfx950 library on the device.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd import graph as G
from allegro_amd.nn import HipAllegroModel

PSI = ((0.02817, 0.20162), (0.28022, 0.40290), (0.50986, 0.94229), (0.18175, 3.19980))
QQR2E = {"metal": 14.399645, "real": 332.06371}
Z_OF = {"H": 1.0, "O": 8.0, "Si": 14.0}
TOL = {torch.float64: 1e-9, torch.float32: 5e-5}
DTYPES = [pytest.param(torch.float64, id="f64"), pytest.param(torch.float32, id="f32")]
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
R_MAX, R_SIO = 3.4, 2.4  # the model's cutoff, and the shortened one of the Si-O pairs


def _backend(name):
    if name == "emu":
        from tests.hip_utils import emu_lib

        return emu_lib(), torch.device("cpu")
    return _lib.load(), torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# closed form
# ---------------------------------------------------------------------------------------------------------------------
def closed_form(pos, ei, shift, types, z, rmax, p, qqr2e):
    """fp64: per-edge energies [E], per-atom energies [N], forces [N,3], dE/d(strain) [3,3] of the ZBL term alone.
    z: [T] atomic numbers, rmax: [T,T] cutoffs (center type, neighbor type), shift: [E,3] cartesian or None."""
    pos = pos.detach().cpu().double().requires_grad_(True)
    eps = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
    sym = 0.5 * (eps + eps.T)
    i, j = ei[0].cpu().long(), ei[1].cpu().long()
    ps = pos + pos @ sym.T
    vec = ps[j] - ps[i]
    if shift is not None:
        sv = shift.detach().cpu().double()
        vec = vec + sv + sv @ sym.T
    r = vec.norm(dim=-1)
    types = types.cpu().long()
    z = torch.as_tensor(z, dtype=torch.float64)
    zi, zj = z[types[i]], z[types[j]]
    x = (zi.pow(0.23) + zj.pow(0.23)) * r / 0.46850
    psi = sum(c * torch.exp(-d * x) for c, d in PSI)
    xc = r / torch.as_tensor(rmax, dtype=torch.float64)[types[i], types[j]]
    f = 1.0 - (p + 1) * (p + 2) / 2 * xc ** p + p * (p + 2) * xc ** (p + 1) - p * (p + 1) / 2 * xc ** (p + 2)
    f = torch.where(xc < 1.0, f, torch.zeros_like(f))
    e_edge = 0.5 * qqr2e * zi * zj / r * psi * f
    e_atom = torch.zeros(pos.shape[0], dtype=torch.float64).index_add(0, i, e_edge)
    g_pos, g_eps = torch.autograd.grad(e_atom.sum(), [pos, eps])
    return e_edge.detach(), e_atom.detach(), -g_pos, g_eps


def test_psi_coefficients_sum_to_one():
    assert abs(sum(c for c, _ in PSI) - 1.0) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# main frame: three species, ragged segments, a 0.6 A pair, periodic edges, one shortened type pair
# ---------------------------------------------------------------------------------------------------------------------
_FRAME = None


def main_frame():
    """14 atoms around a corner of a 60 A box, wrapped into it: part of the edges cross the periodic boundary."""
    global _FRAME
    if _FRAME is None:
        rng = np.random.default_rng(2)
        pos = rng.uniform(-2.9, 2.9, size=(14, 3))
        pos[1] = pos[0] + 0.6 * np.array([0.48, -0.6, 0.64])  # the regime ZBL exists for
        pos[13] = [30.0, 30.0, 30.0]  # isolated: degree 0
        pos = np.mod(pos, 60.0)
        types = rng.integers(0, 3, size=14)
        types[0] = types[1] = 0  # the close pair: Si-Si
        cell = np.eye(3) * 60.0
        ei, cs = G.neighbor_list_pbc(pos, cell, R_MAX)
        deg = np.bincount(ei[0], minlength=14)
        assert (deg % 2 == 1).any() and deg[13] == 0 and deg.max() > 8 and (np.abs(cs).sum(-1) != 0).any(), deg
        r = np.linalg.norm(pos[ei[1]] - pos[ei[0]] + cs @ cell, axis=1)
        assert abs(r.min() - 0.6) < 1e-9
        _FRAME = dict(pos=pos, types=types, cell=cell, ei=ei, cs=cs, deg=deg)
    return _FRAME


MAIN_SPECIES = ["Si", "O", "H"]


def main_cfg(dtype, frame, pair=True, units="metal", **over):
    cfg = dict(type_names=list(MAIN_SPECIES), r_max=R_MAX, l_max=2, num_layers=2, num_scalar_features=64, num_tensor_features=64,
               radial_chemical_embed={"_target_": "allegro.nn.TwoBodyBesselScalarEmbed", "num_bessels": 8, "polynomial_cutoff_p": 6},
               per_edge_type_cutoff={"Si": {"O": R_SIO}, "O": {"Si": R_SIO}}, avg_num_neighbors=float(frame["deg"].mean()), seed=11,
               model_dtype={torch.float32: "float32", torch.float64: "float64"}[dtype])
    cfg.update(over)
    if pair:
        cfg["pair_potential"] = {"_target_": "nequip.nn.pair_potential.ZBL", "units": units, "chemical_species": list(cfg["type_names"])}
    return cfg


def main_rmax():
    rmax = torch.full((3, 3), R_MAX, dtype=torch.float64)
    rmax[0, 1] = rmax[1, 0] = R_SIO
    return rmax


def build(cfg, lib, dev):
    m = HipAllegroModel(**cfg).to(dev)
    m._bind_library(lib)
    return m


def frame_tensors(frame, dtype, dev):
    pos = torch.tensor(frame["pos"], dtype=dtype, device=dev)
    shift = torch.tensor(frame["cs"] @ frame["cell"], dtype=dtype, device=dev)
    return pos, torch.tensor(frame["ei"], device=dev), torch.tensor(frame["types"], device=dev), shift


def step(m, pos, ei, types, shift, transposed=True, virial=True):
    from allegro_amd.nn import PreparedGraph

    g = PreparedGraph(ei, types, pos.shape[0], shift, transposed=transposed, lib=m._bound_lib)
    e, f = m.energy_forces(pos, g)
    w = m.virial(g).clone() if virial else None
    return g, e.clone(), f.clone(), w


def assert_term(name, got_with, got_without, want, dtype):
    """(with - without) == closed form, to the project's tolerance at the scale of the expected total."""
    want = want.to(got_with.device)
    total = got_without.double() + want
    scale = max(1.0, float(total.abs().max()))
    err = float((got_with.double() - got_without.double() - want).abs().max())
    print(f"{name}: max|with - without - closed form| = {err:.3e}, bound {TOL[dtype] * scale:.3e} (scale {scale:.3e}, "
          f"max|closed form| {float(want.abs().max()):.3e})")
    assert err <= TOL[dtype] * scale, name


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_main_frame_energies_forces_virial(backend, dtype, forward_mode):
    lib, dev = _backend(backend)
    fr = main_frame()
    pos, ei, types, shift = frame_tensors(fr, dtype, dev)
    e_edge, e_ref, f_ref, w_ref = closed_form(pos, ei, shift, types, [Z_OF[s] for s in MAIN_SPECIES], main_rmax(), 6.0, QQR2E["metal"])
    # the shortened pair: the list (built at r_max) holds Si-O edges beyond their own cutoff, and they contribute exactly 0
    tc, tn = types[ei[0]].cpu(), types[ei[1]].cpu()
    r = (pos[ei[1]] - pos[ei[0]] + shift).double().norm(dim=-1).cpu()
    beyond = (((tc == 0) & (tn == 1)) | ((tc == 1) & (tn == 0))) & (r >= R_SIO)
    assert beyond.any() and (e_edge[beyond] == 0).all() and (e_edge[~beyond] > 0).all()
    m1, m0 = build(main_cfg(dtype, fr), lib, dev), build(main_cfg(dtype, fr, pair=False), lib, dev)
    assert m1.describe_plan()["pair"] == "zbl" and "pair" not in m0.describe_plan()
    g1, e1, f1, w1 = step(m1, pos, ei, types, shift)
    d1 = m1.debug_tap("dvec", g1, with_forces=True)
    g0, e0, f0, w0 = step(m0, pos, ei, types, shift)
    d0 = m0.debug_tap("dvec", g0, with_forces=True)
    assert_term("atom energies", e1, e0, e_ref, dtype)
    assert_term("forces", f1, f0, f_ref, dtype)
    assert_term("virial", w1, w0, w_ref, dtype)
    # per edge (both graphs keep the list's order: it is center-sorted already): rows beyond the pair's cutoff are untouched, those of the close pair are not
    assert g1.perm is None or torch.equal(g1.perm.cpu(), torch.arange(ei.shape[1]))
    assert torch.equal(d1[beyond.to(dev)], d0[beyond.to(dev)])
    close = (r < 0.61).to(dev)  # (the 0.6 A pair, both directions: far above the rounding of the model's own rows)
    assert int(close.sum()) == 2 and (d1[close] != d0[close]).any(dim=1).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_layout_energy_only_unsorted_edges(backend, dtype):
    """shift_vec NULL (every outside-cell edge has its own ghost atom), no forces, the edge list shuffled before prepare_graph."""
    lib, dev = _backend(backend)
    fr = main_frame()
    gg = G.to_ghost_layout(G.Graph(pos=fr["pos"], types=fr["types"], edge_index=fr["ei"], cell=fr["cell"], cell_shift=fr["cs"]))
    assert gg.num_atoms > 14
    pos = torch.tensor(gg.pos, dtype=dtype, device=dev)
    types = torch.tensor(gg.types, device=dev)
    perm = torch.randperm(gg.num_edges, generator=torch.Generator().manual_seed(0))
    ei = torch.tensor(gg.edge_index)[:, perm].to(dev)
    _, e_ref, _, _ = closed_form(pos, ei, None, types, [Z_OF[s] for s in MAIN_SPECIES], main_rmax(), 6.0, QQR2E["metal"])
    out = []
    for pair in (True, False):
        m = build(main_cfg(dtype, fr, pair=pair), lib, dev)
        g = m.prepare_graph(ei, types, gg.num_atoms, None)
        e, f = m.energy_forces(pos, g, with_forces=False)
        assert f is None
        out.append(e.clone())
    assert float(e_ref[14:].abs().max()) == 0.0  # (ghost atoms are nobody's center)
    assert_term("atom energies, ghost layout", out[0], out[1], e_ref, dtype)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_atomics_mode_forces(backend, dtype):
    """No transposed CSR: the kernel adds to the forces itself, the way edge_backward_kernel does."""
    lib, dev = _backend(backend)
    fr = main_frame()
    pos, ei, types, shift = frame_tensors(fr, dtype, dev)
    _, e_ref, f_ref, w_ref = closed_form(pos, ei, shift, types, [Z_OF[s] for s in MAIN_SPECIES], main_rmax(), 6.0, QQR2E["metal"])
    m1, m0 = build(main_cfg(dtype, fr), lib, dev), build(main_cfg(dtype, fr, pair=False), lib, dev)
    g1, e1, f1, w1 = step(m1, pos, ei, types, shift, transposed=False)
    g0, e0, f0, w0 = step(m0, pos, ei, types, shift, transposed=False)
    assert g1.t_perm is None
    assert_term("atom energies, atomics", e1, e0, e_ref, dtype)
    assert_term("forces, atomics", f1, f0, f_ref, dtype)
    assert_term("virial, atomics", w1, w0, w_ref, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# a second shape class: two species, l_max 3, fp64 on the operator pipeline (the `c5_small` shape); the spline embedding (p = 6)
# ---------------------------------------------------------------------------------------------------------------------
def _small_frame(n=10, seed=5):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 6.5, size=(n, 3))
    pos[n - 1] = [30.0, 30.0, 30.0]
    pos[1] = pos[0] + [0.0, 0.9, 0.0]
    cell = np.eye(3) * 60.0
    ei, cs = G.neighbor_list_pbc(pos, cell, R_MAX)
    deg = np.bincount(ei[0], minlength=n)
    assert deg[n - 1] == 0 and ei.shape[1] >= 10
    return dict(pos=pos, types=rng.integers(0, 2, size=n), cell=cell, ei=ei, cs=cs, deg=deg)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", ["c5_small", "spline"])
def test_second_shape_class(backend, shape):
    lib, dev = _backend(backend)
    fr = _small_frame(n=7 if shape == "c5_small" else 10)
    dtype = torch.float64
    if shape == "c5_small":  # (the hyper-parameters of tests/golden's c5_small fixture: the operator kernels)
        over = dict(type_names=["O", "H"], l_max=3, num_layers=3, num_scalar_features=128, num_tensor_features=128,
                    scalar_embed_mlp_hidden_layers_width=32, allegro_mlp_hidden_layers_width=128, readout_mlp_hidden_layers_width=32,
                    radial_chemical_embed_dim=16, per_edge_type_cutoff=None)
        p = 6.0
    else:  # the spline embedding provides no cutoff: the envelope is the polynomial one with p = 6, whatever the key says
        over = dict(type_names=["O", "H"], num_scalar_features=16, num_tensor_features=8, per_edge_type_cutoff=None,
                    radial_chemical_embed={"_target_": "allegro.nn.TwoBodySplineScalarEmbed", "num_splines": 8, "spline_span": 3,
                                           "polynomial_cutoff_p": 9})
        p = 6.0
    pos, ei, types, shift = frame_tensors(fr, dtype, dev)
    rmax = torch.full((2, 2), R_MAX, dtype=torch.float64)
    _, e_ref, f_ref, w_ref = closed_form(pos, ei, shift, types, [Z_OF["O"], Z_OF["H"]], rmax, p, QQR2E["metal"])
    m1, m0 = build(main_cfg(dtype, fr, **over), lib, dev), build(main_cfg(dtype, fr, pair=False, **over), lib, dev)
    if shape == "c5_small":
        assert m1.describe_plan()["operator_path"]
    _, e1, f1, w1 = step(m1, pos, ei, types, shift)
    _, e0, f0, w0 = step(m0, pos, ei, types, shift)
    assert_term(f"atom energies, {shape}", e1, e0, e_ref, dtype)
    assert_term(f"forces, {shape}", f1, f0, f_ref, dtype)
    assert_term(f"virial, {shape}", w1, w0, w_ref, dtype)


@pytest.mark.parametrize("backend", BACKENDS)
def test_units_real_is_metal_rescaled(backend):
    lib, dev = _backend(backend)
    fr, dtype = _small_frame(), torch.float64
    over = dict(type_names=["O", "H"], num_scalar_features=16, num_tensor_features=8, per_edge_type_cutoff=None)
    pos, ei, types, shift = frame_tensors(fr, dtype, dev)
    res = {}
    for units in ("metal", "real", None):
        m = build(main_cfg(dtype, fr, pair=units is not None, units=units, **over), lib, dev)
        res[units] = step(m, pos, ei, types, shift)[1:]
    ratio = 332.06371 / 14.399645
    for k, name in enumerate(("atom energies", "forces", "virial")):
        metal, real = res["metal"][k] - res[None][k], res["real"][k] - res[None][k]
        assert float(metal.abs().max()) > 1e-2  # (the term is there)
        assert float((real - ratio * metal).abs().max()) <= 1e-9 * max(1.0, float(res["real"][k].abs().max())), name
    assert abs(sum(c for c, _ in PSI) - 1.0) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# hipGraph replay, the C setter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_graph_replay_and_removal():
    lib, dev = _backend("gpu")
    fr, dtype = main_frame(), torch.float32
    pos, ei, types, shift = frame_tensors(fr, dtype, dev)
    m1, m0 = build(main_cfg(dtype, fr), lib, dev), build(main_cfg(dtype, fr, pair=False), lib, dev)
    g1, e1, f1, w1 = step(m1, pos, ei, types, shift)
    g0, e0, f0, _ = step(m0, pos, ei, types, shift, virial=False)
    m1.enable_hip_graph(True)
    try:
        for _ in range(2):
            e, f = m1.energy_forces(pos, g1)
            torch.cuda.synchronize()
            assert torch.equal(e, e1) and torch.equal(f, f1)
            assert torch.equal(m1.virial(g1), w1)
        m1.set_pair_zbl(None)  # drops the captured step
        assert "pair" not in m1.describe_plan()
        e, f = m1.energy_forces(pos, g1)
        torch.cuda.synchronize()
        assert torch.equal(e, e0) and torch.equal(f, f0)
        m1.set_pair_zbl(m1.pair_zbl)
        e, f = m1.energy_forces(pos, g1)
        torch.cuda.synchronize()
        assert torch.equal(e, e1) and torch.equal(f, f1)
    finally:
        m1.enable_hip_graph(False)


@pytest.mark.parametrize("backend", BACKENDS)
def test_setter_on_a_plain_plan_and_its_guards(backend):
    """aa_model_plan_set_pair_zbl straight on the C ABI: adds / removes the term of a model built without one; rejects a wrong
    num_types, a non-positive Z and a non-positive qqr2e; a plan that never saw the setter and one it was removed from report the
    same description and the same profiled stage names."""
    lib, dev = _backend(backend)
    fr, dtype = _small_frame(), torch.float64
    over = dict(type_names=["O", "H"], num_scalar_features=16, num_tensor_features=8, per_edge_type_cutoff=None)
    pos, ei, types, shift = frame_tensors(fr, dtype, dev)
    m0, m1 = build(main_cfg(dtype, fr, pair=False, **over), lib, dev), build(main_cfg(dtype, fr, **over), lib, dev)
    g0, e0, f0, _ = step(m0, pos, ei, types, shift, virial=False)
    _, e1, f1, _ = step(m1, pos, ei, types, shift, virial=False)
    never = dict(m0.describe_plan())
    stages_never = _stage_names(m0, lib, pos, g0)
    assert "pair_zbl" not in stages_never

    def call(num_types, zs, qqr2e, poly_p=6.0):
        arr = (C.c_double * len(zs))(*zs)
        return lib.lib.aa_model_plan_set_pair_zbl(m0._plan_handle, C.byref(_lib.PairZbl(num_types, arr, qqr2e, poly_p)))

    assert call(3, [8.0, 1.0, 1.0], 14.399645) != 0  # num_types of the plan is 2
    assert call(2, [8.0, 0.0], 14.399645) != 0
    assert call(2, [8.0, -1.0], 14.399645) != 0
    assert call(2, [8.0, 1.0], 0.0) != 0
    assert m0.describe_plan() == never  # (a rejected call changes nothing)
    assert call(2, [8.0, 1.0], 14.399645) == 0
    assert m0.describe_plan() == dict(never, pair="zbl")
    stages_with = _stage_names(m0, lib, pos, g0)
    k = stages_with.index("pair_zbl")
    assert stages_with[k - 1] == "edge_backward" and stages_with[k + 1] == "force_gather"
    assert stages_with[:k] + stages_with[k + 1:] == stages_never
    assert _stage_names(m0, lib, pos, g0, with_forces=False)[-1] == "pair_zbl"
    e, f = m0.energy_forces(pos, g0)
    assert torch.equal(e, e1) and torch.equal(f, f1)
    assert lib.lib.aa_model_plan_set_pair_zbl(m0._plan_handle, None) == 0
    assert m0.describe_plan() == never and _stage_names(m0, lib, pos, g0) == stages_never
    e, f = m0.energy_forces(pos, g0)
    assert torch.equal(e, e0) and torch.equal(f, f0)


def _stage_names(m, lib, pos, g, with_forces=True):
    L = lib.lib
    L.aa_model_energy_forces_profiled.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_lib.Graph), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_char_p, C.POINTER(C.c_int),
                                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]
    ms, names, n = (C.c_float * 256)(), C.create_string_buffer(256 * 32), C.c_int()
    e = torch.empty(pos.shape[0], dtype=pos.dtype, device=pos.device)
    f = torch.empty((pos.shape[0], 3), dtype=pos.dtype, device=pos.device)
    gs = g.c_struct()
    stream = torch.cuda.current_stream(pos.device).cuda_stream if pos.is_cuda else None
    lib.check(L.aa_model_energy_forces_profiled(m._plan_handle, m._blob.data_ptr(), C.byref(gs), pos.data_ptr(), m._workspace.data_ptr(),
                                                m._workspace.numel(), e.data_ptr(), f.data_ptr() if with_forces else None, stream, 256, ms,
                                                names, C.byref(n), None, None), "aa_model_energy_forces_profiled")
    return [names.raw[32 * i: 32 * i + 32].split(b"\0")[0].decode() for i in range(n.value)]


# ---------------------------------------------------------------------------------------------------------------------
# public interface: forward(data), batched frames, training mode, guards
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_forward_dict_batched_frames_with_stress(backend):
    """forward(data) on two frames in one batch (per-atom and total energies, forces, stress): the pair term of each frame."""
    lib, dev = _backend(backend)
    fr, dtype = _small_frame(), torch.float64
    over = dict(type_names=["O", "H"], num_scalar_features=16, num_tensor_features=8, per_edge_type_cutoff=None)
    n = fr["pos"].shape[0]
    pos = torch.tensor(np.concatenate([fr["pos"], fr["pos"] * 1.03]), dtype=dtype, device=dev)
    ei = torch.tensor(np.concatenate([fr["ei"], fr["ei"] + n], axis=1), device=dev)
    cells = torch.tensor(np.stack([fr["cell"], fr["cell"] * 1.03]), dtype=dtype, device=dev)
    data = dict(pos=pos, edge_index=ei, atom_types=torch.tensor(np.concatenate([fr["types"]] * 2), device=dev), cell=cells,
                edge_cell_shift=torch.tensor(np.concatenate([fr["cs"]] * 2), dtype=dtype, device=dev),
                batch=torch.arange(2, device=dev).repeat_interleave(n))
    out1 = build(main_cfg(dtype, fr, **over), lib, dev)(data)
    out0 = build(main_cfg(dtype, fr, pair=False, **over), lib, dev)(data)
    rmax = torch.full((2, 2), R_MAX, dtype=torch.float64)
    for k in range(2):
        sl = slice(k * n, (k + 1) * n)
        shift = torch.tensor(fr["cs"], dtype=dtype) @ cells[k].cpu()
        _, e_ref, f_ref, w_ref = closed_form(pos[sl], torch.tensor(fr["ei"]), shift, data["atom_types"][sl], [8.0, 1.0], rmax, 6.0, QQR2E["metal"])
        assert_term(f"frame {k} atomic_energy", out1["atomic_energy"][sl, 0], out0["atomic_energy"][sl, 0], e_ref, dtype)
        assert_term(f"frame {k} total_energy", out1["total_energy"][k], out0["total_energy"][k], e_ref.sum().reshape(1), dtype)
        assert_term(f"frame {k} forces", out1["forces"][sl], out0["forces"][sl], f_ref, dtype)
        vol = float(torch.linalg.det(cells[k]).abs())
        assert_term(f"frame {k} stress * volume", out1["stress"][k] * vol, out0["stress"][k] * vol, w_ref, dtype)


@pytest.mark.parametrize("backend", BACKENDS)
def test_training_mode_matches_eval_and_differentiates(backend):
    lib, dev = _backend(backend)
    fr, dtype = _small_frame(), torch.float64
    over = dict(type_names=["O", "H"], num_scalar_features=16, num_tensor_features=8, per_edge_type_cutoff={"O": {"H": R_SIO}, "H": {"O": R_SIO}})
    m = build(main_cfg(dtype, fr, **over), lib, dev)
    data = dict(pos=torch.tensor(fr["pos"], dtype=dtype, device=dev), edge_index=torch.tensor(fr["ei"], device=dev),
                atom_types=torch.tensor(fr["types"], device=dev), cell=torch.tensor(fr["cell"], dtype=dtype, device=dev),
                edge_cell_shift=torch.tensor(fr["cs"], dtype=dtype, device=dev))
    ev = {k: v.clone() for k, v in m(data).items() if k in ("atomic_energy", "forces", "stress")}
    m.train()
    out = m(data)
    for k, v in ev.items():
        assert float((out[k].detach() - v).abs().max()) <= 1e-9 * max(1.0, float(v.abs().max())), k
    assert out["forces"].requires_grad
    out["forces"].square().sum().backward()
    grads = [p.grad for p in m.parameters() if p.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    # the block-by-block training step evaluates the same function
    for p in m.parameters():
        p.grad = None
    graph = m._graph_for(data)
    loss, f, e = m.chunked_training_step(graph, 12).step(data["pos"], lambda forces, energy: forces.square().sum())
    assert float((f - ev["forces"]).abs().max()) <= 1e-9 * max(1.0, float(ev["forces"].abs().max()))
    for p, g in zip([p for p in m.parameters() if p.requires_grad], grads):
        assert float((p.grad - g).abs().max()) <= 1e-7 * max(1.0, float(g.abs().max()))


def test_constructor_and_export_guards(tmp_path):
    fr = _small_frame()
    over = dict(type_names=["O", "H"], num_scalar_features=16, num_tensor_features=8, per_edge_type_cutoff=None)

    def with_pair(**pp):
        cfg = main_cfg(torch.float64, fr, pair=False, **over)
        cfg["pair_potential"] = {"_target_": "nequip.nn.pair_potential.ZBL", "units": "metal", "chemical_species": ["O", "H"], **pp}
        return HipAllegroModel(**cfg)

    with pytest.raises(NotImplementedError, match="LennardJones"):
        with_pair(_target_="nequip.nn.pair_potential.LennardJones")
    with pytest.raises(ValueError, match="Xx"):
        with_pair(chemical_species=["O", "Xx"])
    with pytest.raises(ValueError, match="units"):
        with_pair(units="si")
    with pytest.raises(ValueError, match="one chemical symbol per entry"):
        with_pair(chemical_species=["O", "H", "H"])
    m, plain = with_pair(), HipAllegroModel(**main_cfg(torch.float64, fr, pair=False, **over))
    assert m.pair_zbl == dict(atomic_numbers=[8.0, 1.0], qqr2e=14.399645, poly_p=6.0)
    # no parameters, no state: the two state_dicts hold the same keys, and each loads the other's strictly
    assert list(m.state_dict()) == list(plain.state_dict())
    m.load_state_dict(plain.state_dict())
    # entries of a pair-potential module in a checkpoint are accepted; its atomic numbers must be the configured ones
    sd = dict(plain.state_dict())
    sd["func.pair_potential.atomic_numbers"] = torch.tensor([8, 1])
    m.load_state_dict(sd)
    sd["func.pair_potential.atomic_numbers"] = torch.tensor([8, 6])
    with pytest.raises(ValueError, match="atomic numbers"):
        m.load_state_dict(sd)
    from allegro_amd import export

    with pytest.raises(NotImplementedError, match="pair_potential"):
        export.write_host_model(m, str(tmp_path / "m.aamodel"))
    with pytest.raises(NotImplementedError, match="pair_potential"):
        export.serialize_config(m, 1)
    with pytest.raises(NotImplementedError, match="pair_potential"):
        export.ExportableAllegro(m, "cpu")
    export.write_host_model(plain, str(tmp_path / "p.aamodel"))


# ---------------------------------------------------------------------------------------------------------------------
# sharded path in one process
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_two_halo_shards_match_the_one_shard_step(backend):
    from allegro_amd.dist import InProcessHaloGroup

    lib, dev = _backend(backend)
    fr, dtype = main_frame(), torch.float64
    pos, ei, types, shift = frame_tensors(fr, dtype, dev)
    over = dict(num_scalar_features=16, num_tensor_features=8)  # (the frame is the main one; the model is a small one)
    m1, m0 = build(main_cfg(dtype, fr, **over), lib, dev), build(main_cfg(dtype, fr, pair=False, **over), lib, dev)
    _, e_one, f_one, _ = step(m1, pos, ei, types, shift, virial=False)
    _, e_ref, f_ref, _ = closed_form(pos, ei, shift, types, [Z_OF[s] for s in MAIN_SPECIES], main_rmax(), 6.0, QQR2E["metal"])
    grp = InProcessHaloGroup.from_positions(pos, types, fr["cell"], R_MAX, 2, lib=lib)
    assert sum(s.n_own for s in grp.shards) == 14 and sum(s.n_ghost for s in grp.shards) > 0
    res = {}
    for name, m in (("with", m1), ("without", m0)):
        e_all, f_all = torch.full_like(e_one, float("nan")), torch.full_like(f_one, float("nan"))
        for s, (e, f) in zip(grp.shards, grp.step(m, [pos[s.owned_ids()] for s in grp.shards])):
            e_all[s.owned_ids()] = e
            f_all[s.owned_ids()] = f
        res[name] = (e_all, f_all)
    for got, want, name in ((res["with"][0], e_one, "atom energies"), (res["with"][1], f_one, "forces")):
        assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), name
    assert_term("atom energies, 2 shards", res["with"][0], res["without"][0], e_ref, dtype)
    assert_term("forces, 2 shards", res["with"][1], res["without"][1], f_ref, dtype)
