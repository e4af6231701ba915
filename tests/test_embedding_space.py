"""The two-body embedding's parameter space through every forward: species count, basis size, cutoff exponent, edges beyond the
cutoff, edge counts at the 256-edge block boundaries, and the limits that depend on them.

The rest of the suite pins parity at one point of this space: at most four species, 8 Bessel functions (8 or 16 splines) and
p = 6 on hardware, lists without an edge at r >= r_max (but for the three-species per-pair-cutoff fixtures), edge counts that are
whatever the fixture gives.  The species count T enters every class index `ti * T + tj`, the per-type tables, the `ti | tj << 16`
packing and the LDS size of `edge_backward_kernel` (opt-in above 64 KB, refused above 160 KB); the basis size selects the bodies
of `edge_prologue_kernel` (`B != 8`, `prologue_ldb`) and the general phase 1 of `edge_backward_kernel`; a neighbour list with skin
holds edges with r >= r_max on every step, handled by `cutoff_and_grad` / `spline_basis_and_grad` in the staged kernels and in both
fused forwards; the edge kernels work in blocks of 256 edges with clamped reads.

Sections (each test exists twice: `_emulated` on the CPU emulation of the unmodified kernels, `_on_gpu` on the gfx950 library):

1. species count (T = 5 .. 89; no fused forward from four species on), 2. basis size and cutoff exponent (one species; the fp32 rows
   under `forward_mode`): atom energies, forces and the strain derivative against `oracle.restatement`, the taps `edge_attrs` and
   `emb0` of a second, tapped model against its intermediates, and `edge_prologue` / `edge_backward` in the launch list of the
   profiled step.  (The two p rows are the 8 x 64 table the fused forward takes: in the automatic and wide modes `fused_fwd` stands
   in for `edge_prologue` there, which the staged mode pins; every other row pins `edge_prologue` in all three modes.);
3. skin edges: a list at 1.3 r_max against the plain list of the same frame -- energies, forces, strain derivative, per-atom
   tensors, heat flux within the reference's whole-model tolerance (`TOL` of tests/test_hip_model.py), and the `dvec` rows of the
   edges beyond the cutoff exactly zero (Bessel: f = df = 0 by branch, every later layer is bias-free with act(0) = 0) or at most
   eps(dtype) x max |dvec| (spline: 1 - cos at a one-ulp error of 2 pi);
4. edge counts 1, 255, 256, 257, 512, with and without the transposed CSR (gather / atomics in `edge_backward_kernel`), on a
   NaN-poisoned workspace of the exact size;
5. the limits: 17 Bessel functions, a prologue above 64 KB of LDS and an edge reverse above 160 KB are refused by
   `aa_model_plan_create` with AA_ERR_INVALID and a message naming the limit -- before any step exists -- and the largest accepted
   neighbours of the two LDS rows step correctly.

Every model-level comparison is one of the project's two rules (`check` of tests/test_step_values.py: fp64 within 1e-9 x max(1,
max |expected|); fp32 not further from the fp64 oracle on the upcast weights than twice the fp32 CPU oracle is, + 1e-5 of the
output scale); `-s` prints `name quantity err_hip err_cpu32 scale` per comparison, DESIGN.md section 5 quotes the worst ratios."""
import ctypes as C

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd import graph as G
from allegro_amd.nn import HipAllegroModel, PreparedGraph, _device_ctx
from tests.test_hip_model import TOL
from tests.test_plan_pipeline import BASE
from tests.test_step_values import Rig, check, exactly_zero

R_MAX = 3.0
N_ATOMS = 40
F32, F64 = "float32", "float64"


def BESSEL(n, p=None):
    return dict(_target_="allegro.nn.TwoBodyBesselScalarEmbed", num_bessels=n, **({} if p is None else {"polynomial_cutoff_p": p}))


def SPLINE(n, span):
    return dict(_target_="allegro.nn.TwoBodySplineScalarEmbed", num_splines=n, spline_span=span)


def _emu():
    from tests.hip_utils import emu_lib

    return emu_lib(), torch.device("cpu")


def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return None, torch.device("cuda:0")


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def _min_image(d, cell):
    box = np.diag(cell)
    return d - np.round(d / box) * box


def _place(pos, cell, i, j, r, rng):
    """Moves atom j to the distance r of atom i, in the one of 64 seeded directions that keeps it farthest from every other atom."""
    u = rng.normal(size=(64, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    others = np.delete(pos, [i, j], axis=0)
    cand = pos[i] + r * u
    clearance = np.linalg.norm(_min_image(cand[:, None] - others[None], cell), axis=-1).min(1)
    pos[j] = cand[int(np.argmax(clearance))]


def _lengths(pos, cell, ei, shift):
    return np.linalg.norm(pos[ei[1]] - pos[ei[0]] + shift @ cell, axis=1)


def _pair_length(pos, cell, ei, shift, i, j):
    sel = (ei[0] == i) & (ei[1] == j)
    assert sel.sum() == 1, (i, j, int(sel.sum()))
    return float(_lengths(pos, cell, ei[:, sel], shift[sel])[0])


_GEOMETRY = {}


def geometry(kind="box", seed=0):
    """40 atoms on a jittered 4 x 4 x 3 lattice (seeded like tests/test_emu_fuzz.py: no unphysically close pairs) and the list at
    r_max = 3.0 from `neighbor_list_pbc`.  "box": a periodic box of 8 A; "dense": the same lattice at a spacing of 1.4 A in a cell
    of 60 A, where a list at 1.3 r_max holds more than 32 neighbours per atom and the plain one does not.  Atom 1 is moved to
    0.25 r_max of atom 0, atom 21 to (1 - 2**-10) r_max of atom 20 and atom 31 to (1 + 2**-7) r_max of atom 30 (an edge of the
    skin list only).  dict(pos, cell, ei, shift, skin_ei, skin_shift) as numpy; the skin list is the one at 1.3 r_max."""
    key = (kind, seed)
    if key in _GEOMETRY:
        return _GEOMETRY[key]
    rng = np.random.default_rng(500 + seed)
    grid = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)[:N_ATOMS]
    if kind == "dense":
        cell = np.eye(3) * 60.0
        pos = (grid + rng.uniform(-0.1, 0.1, (N_ATOMS, 3))) * 1.4 + 20.0
    else:
        box = 8.0
        cell = np.eye(3) * box
        pos = (grid + 0.5 + rng.uniform(-0.25, 0.25, (N_ATOMS, 3))) * (box / np.array([4.0, 4.0, 3.0]))
    _place(pos, cell, 0, 1, 0.25 * R_MAX, rng)
    _place(pos, cell, 20, 21, (1.0 - 2.0 ** -10) * R_MAX, rng)
    _place(pos, cell, 30, 31, (1.0 + 2.0 ** -7) * R_MAX, rng)
    ei, shift = G.neighbor_list_pbc(pos, cell, R_MAX)
    skin_ei, skin_shift = G.neighbor_list_pbc(pos, cell, 1.3 * R_MAX)
    # both special pairs are in the list, at the lengths asked for
    assert abs(_pair_length(pos, cell, ei, shift, 0, 1) / R_MAX - 0.25) < 1e-12
    assert abs(_pair_length(pos, cell, ei, shift, 20, 21) / R_MAX - (1.0 - 2.0 ** -10)) < 1e-12
    assert _lengths(pos, cell, ei, shift).min() >= 0.25 * R_MAX - 1e-12
    geo = dict(pos=pos, cell=cell, ei=ei, shift=shift, skin_ei=skin_ei, skin_shift=skin_shift)
    _GEOMETRY[key] = geo
    return geo


def species(geo, T, seed=0):
    """Types of the 40 atoms: random, with atoms 0 and 1 (the pair at 0.25 r_max) of type T - 1 and another neighbour of atom 0 of
    type 0, so that the list holds edges of the classes (T-1, T-1), (0, T-1) and (T-1, 0)."""
    rng = np.random.default_rng(700 + seed)
    types = rng.integers(0, T, size=N_ATOMS)
    if T > 1:
        ei = geo["ei"]
        j = int(ei[1][(ei[0] == 0) & (ei[1] != 1)][0])
        types[[0, 1]] = T - 1
        types[j] = 0
        classes = set(zip(types[ei[0]].tolist(), types[ei[1]].tolist()))
        assert {(T - 1, T - 1), (0, T - 1), (T - 1, 0)} <= classes
    return types


def config(T, dtype, rce, embed_dim, geo, l_max=2, pair_cutoffs=False, seed=0):
    """The C2 shape (tests/test_plan_pipeline.py: BASE) at r_max = 3.0 with T species, per-type scales and shifts that are all
    distinct and, with `pair_cutoffs`, an asymmetric per-type-pair cutoff table between 0.7 and 1.0 r_max."""
    names = [f"X{t}" for t in range(T)]
    cfg = dict(BASE, type_names=names, r_max=R_MAX, l_max=l_max, radial_chemical_embed=rce, radial_chemical_embed_dim=embed_dim,
               avg_num_neighbors=float(geo["ei"].shape[1]) / N_ATOMS, seed=100 + seed, model_dtype=dtype,
               per_type_energy_scales=[0.5 + 1.5 * (t + 1) / (T + 1) for t in range(T)],
               per_type_energy_shifts=[-1.0 + 2.0 * (t + 0.5) / T for t in range(T)])
    if pair_cutoffs:
        cfg["per_edge_type_cutoff"] = {a: {b: R_MAX * (0.7 + 0.05 * ((3 * i + 5 * j) % 7)) for j, b in enumerate(names)} for i, a in enumerate(names)}
        tab = np.array([[cfg["per_edge_type_cutoff"][a][b] for b in names] for a in names])
        assert tab.max() <= R_MAX and not np.allclose(tab, tab.T)
    return cfg


# ---- model, steps, oracle ---------------------------------------------------------------------------------------------------
def build(cfg, lib, dev, taps=False):
    m = HipAllegroModel(**cfg).to(dev)
    if lib is not None:
        m._bind_library(lib)
    if taps:
        m.enable_debug_taps(True)
    return m


def prepared(m, dev, geo, types, skin=False):
    ei, shift = (geo["skin_ei"], geo["skin_shift"]) if skin else (geo["ei"], geo["shift"])
    sv = torch.tensor(shift @ geo["cell"], dtype=m.dtype, device=dev)
    return m.prepare_graph(torch.tensor(ei, device=dev), torch.tensor(types, device=dev), N_ATOMS, sv)


def profiled_step(m, pos, g):
    """One force step through `aa_model_energy_forces_profiled` in the model's own workspace (so `virial`, `atom_virial`,
    `heat_flux_potential` and the taps read what it left): (atom energies, forces, launch names), as tests/test_step_plan.py::run_case."""
    lib, dev = m._get_lib(), pos.device
    mx = 128
    ms, by, fl, nst = (C.c_float * mx)(), (C.c_double * mx)(), (C.c_double * mx)(), C.c_int(0)
    names = C.create_string_buffer(32 * mx)
    fn = lib.lib.aa_model_energy_forces_profiled
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    with _device_ctx(dev):
        m._select_device(dev)
        m._blocked = None
        m._ensure_plan()
        m._ensure_weights(dev)
        m._ensure_workspace(lib.lib.aa_model_workspace_bytes(m._plan_handle, g.num_atoms, g.num_edges, 1), dev)
        e = torch.full((g.num_atoms,), float("nan"), dtype=m.dtype, device=dev)
        f = torch.full((g.num_atoms, 3), float("nan"), dtype=m.dtype, device=dev)
        cg = g.c_struct()
        stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
        lib.check(fn(m._plan_handle, m._blob.data_ptr(), C.byref(cg), pos.data_ptr(), m._workspace.data_ptr(), m._workspace.numel(),
                     e.data_ptr(), f.data_ptr(), stream, mx, ms, names, C.byref(nst), by, fl), "aa_model_energy_forces_profiled")
        m.check(dev)
    assert nst.value < mx
    return e, f, [names.raw[32 * i: 32 * i + 32].split(b"\0")[0].decode() for i in range(nst.value)]


def weights(m):
    return {k[len("func."):]: v.detach().cpu() for k, v in m.state_dict().items()}


_ORACLE = {}


def oracle(key, cfg, sd, geo_pos, ei, shift_vec, types):
    """Once per row (the models are seeded, so every forward mode and both backends of a row share it): per quantity
    (fp32 oracle | None, fp64 oracle) -- for an fp64 model the fp64 oracle on its own weights, for an fp32 one the fp32 oracle and
    the fp64 oracle on the upcast weights.  e, f, w and the intermediates edge_attrs, emb0."""
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import restatement as R

    ocfg = dict(cfg, polynomial_cutoff_p=cfg["radial_chemical_embed"].get("polynomial_cutoff_p", 6))
    ei_t, tt = torch.tensor(ei), torch.tensor(types)

    def run(sd_, dtype, cfg_):
        p, sv = torch.tensor(geo_pos, dtype=dtype), torch.tensor(shift_vec, dtype=dtype)
        out = R.allegro_energy_forces(cfg_, sd_, p, ei_t, tt, sv)
        w = R.allegro_virial(cfg_, sd_, p, ei_t, tt, sv).detach()
        _, inter = R.allegro_energy(cfg_, sd_, p, ei_t, tt, sv, return_intermediates=True)
        return dict(e=out["atomic_energy"].reshape(-1), f=out["forces"], w=w, edge_attrs=inter["edge_attrs"].detach(), emb0=inter["emb0"].detach())

    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    r64 = run(sd64, torch.float64, dict(ocfg, model_dtype=F64))
    r32 = run(sd, torch.float32, ocfg) if cfg["model_dtype"] == F32 else {q: None for q in r64}
    _ORACLE[key] = {q: (r32[q], r64[q]) for q in r64}
    return _ORACLE[key]


def fusable(cfg):
    """The fused forward is offered to the standard fp32 stack with the two-body table: 8 basis functions, 64 columns, <= 3 species."""
    rce = cfg["radial_chemical_embed"]
    return (cfg["model_dtype"] == F32 and rce.get("num_bessels", rce.get("num_splines")) == 8 and cfg["radial_chemical_embed_dim"] == 64 and
            len(cfg["type_names"]) <= 3 and cfg["l_max"] <= 2)


def model_row(name, cfg, geo, types, lib, dev, mode=None):
    """Sections 1 and 2: one row against the oracle -- E_i, forces, strain derivative behind ONE profiled step; the launch list; the
    taps of a second, tapped model (once per row: a tapped step is the staged one whatever the mode)."""
    m = build(cfg, lib, dev)
    g = prepared(m, dev, geo, types)
    pos = torch.tensor(geo["pos"], dtype=m.dtype, device=dev)
    e, f, launches = profiled_step(m, pos, g)
    w = m.virial(g)
    want = oracle(name, cfg, weights(m), geo["pos"], geo["ei"], geo["shift"] @ geo["cell"], types)
    tag = name if mode is None else f"{name}[{mode}]"
    failures = []
    for what, got in (("E", e), ("F", f), ("W", w)):
        try:
            check(tag, what, got.cpu(), *want[what.lower()])
        except AssertionError as err:
            failures.append(f"{what}: {err}")
    # the row ran the edge kernels: a fused forward (never from four species on, never off the 8 x 64 table) stands in for the prologue only
    print(f"{tag} launches {' '.join(launches)}")
    assert "edge_backward" in launches, launches
    if not fusable(cfg) or mode == "staged":
        assert "edge_prologue" in launches, launches
    else:  # (every segment of this frame fits one tile: the one launch of the fused forward, which evaluates the embedding itself)
        assert "fused_fwd" in launches and "edge_prologue" not in launches, launches
    if mode in (None, "auto"):
        mt = build(cfg, lib, dev, taps=True)
        gt = prepared(mt, dev, geo, types)
        mt.energy_forces(pos, gt, with_forces=False)
        for tap in ("edge_attrs", "emb0"):
            try:
                check(tag, tap, mt.debug_tap(tap, gt).cpu(), *want[tap])
            except AssertionError as err:
                failures.append(f"{tap}: {err}")
    assert not failures, "\n".join(failures)


# ---- 1. species count -------------------------------------------------------------------------------------------------------
# (name, T, dtype, embedding, radial_chemical_embed_dim, extras)
SPECIES = [
    ("T5_f32", 5, F32, BESSEL(8), 64, {}),
    ("T5_f64", 5, F64, BESSEL(8), 64, {}),
    ("T5_f32_pair_cutoffs", 5, F32, BESSEL(8), 64, dict(pair_cutoffs=True)),  # the full list: edges beyond their pair's cutoff stay in
    ("T5_f64_pair_cutoffs", 5, F64, BESSEL(8), 64, dict(pair_cutoffs=True)),
    ("T8_f32", 8, F32, BESSEL(8), 64, {}),
    ("T89_f32", 89, F32, BESSEL(8), 64, {}),
    ("T89_f64_s128", 89, F64, BESSEL(8), 128, {}),  # edge reverse: more than 64 KB of LDS, the opt-in branch
    ("T89_f32_spline", 89, F32, SPLINE(8, 6), 64, {}),  # class table of 89^2 rows
    ("T64_f64_b5_s48", 64, F64, BESSEL(5), 48, {}),  # general phase 1, general prologue
    ("T16_f64_spline12", 16, F64, SPLINE(12, 6), 32, {}),
]


def _species_case(row, lib, dev):
    name, T, dtype, rce, embed_dim, extra = row
    geo = geometry("box")
    model_row(name, config(T, dtype, rce, embed_dim, geo, **extra), geo, species(geo, T), lib, dev)


@pytest.mark.parametrize("row", SPECIES, ids=[r[0] for r in SPECIES])
def test_species_count_emulated(row):
    _species_case(row, *_emu())


@pytest.mark.gpu
@pytest.mark.parametrize("row", SPECIES, ids=[r[0] for r in SPECIES])
def test_species_count_on_gpu(row):
    _species_case(row, *_gpu())


# ---- 2. basis and cutoff, one species ---------------------------------------------------------------------------------------------
# (name, dtype, embedding, radial_chemical_embed_dim, l_max)
BASIS_F32 = [
    ("b1_f32", F32, BESSEL(1), 64, 2),
    ("b7_f32_lmax1", F32, BESSEL(7), 64, 1),
    ("b9_f32", F32, BESSEL(9), 64, 2),
    ("b16_f32_lmax3", F32, BESSEL(16), 64, 3),
    ("s4_span1_f32", F32, SPLINE(4, 1), 64, 2),
    ("s4_span4_f32", F32, SPLINE(4, 4), 64, 2),
    ("s16_span1_f32", F32, SPLINE(16, 1), 64, 2),
    ("s16_span16_f32", F32, SPLINE(16, 16), 64, 2),
]
BASIS_F32_FUSABLE = [
    ("p2_f32", F32, BESSEL(8, 2), 64, 2),
    ("p9_f32", F32, BESSEL(8, 9), 64, 2),
]
BASIS_F64 = [
    ("b16_f64_s128", F64, BESSEL(16), 128, 2),
    ("p2_f64", F64, BESSEL(8, 2), 64, 2),
    ("p9_f64", F64, BESSEL(8, 9), 64, 2),
]
assert not any(fusable(dict(model_dtype=r[1], radial_chemical_embed=r[2], radial_chemical_embed_dim=r[3], type_names=["X0"], l_max=r[4]))
               for r in BASIS_F32 + BASIS_F64)


def _basis_case(row, lib, dev, mode=None):
    name, dtype, rce, embed_dim, l_max = row
    geo = geometry("box")
    model_row(name, config(1, dtype, rce, embed_dim, geo, l_max=l_max), geo, species(geo, 1), lib, dev, mode)


def _ids(rows):
    return [r[0] for r in rows]


BASIS_F32_ALL = BASIS_F32 + BASIS_F32_FUSABLE


@pytest.mark.parametrize("row", BASIS_F32_ALL, ids=_ids(BASIS_F32_ALL))
def test_basis_and_cutoff_every_forward_emulated(row, forward_mode):
    _basis_case(row, *_emu(), mode=forward_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("row", BASIS_F32_ALL, ids=_ids(BASIS_F32_ALL))
def test_basis_and_cutoff_every_forward_on_gpu(row, forward_mode):
    _basis_case(row, *_gpu(), mode=forward_mode)


@pytest.mark.parametrize("row", BASIS_F64, ids=_ids(BASIS_F64))
def test_basis_and_cutoff_emulated(row):
    _basis_case(row, *_emu())


@pytest.mark.gpu
@pytest.mark.parametrize("row", BASIS_F64, ids=_ids(BASIS_F64))
def test_basis_and_cutoff_on_gpu(row):
    _basis_case(row, *_gpu())


# ---- 3. skin edges ----------------------------------------------------------------------------------------------------------
# (name, T, dtype, embedding)
SKIN_ONE = [("bessel_f32", 1, F32, BESSEL(8)), ("spline_f32", 1, F32, SPLINE(8, 6))]
SKIN_F64 = ("bessel_f64", 1, F64, BESSEL(8))
SKIN_THREE = ("bessel_f32_three_species", 3, F32, BESSEL(8))
SKIN_GEOMETRIES = ["box", "dense"]  # (a) max_degree <= 32 with the skin; (b) <= 32 without it, above 32 with it


def _degrees(ei):
    return np.bincount(ei[0], minlength=N_ATOMS)


def test_skin_geometries_are_what_section_3_asks_for():
    a, b = geometry("box"), geometry("dense")
    assert _degrees(a["skin_ei"]).max() <= 32
    assert _degrees(b["ei"]).max() <= 32 < _degrees(b["skin_ei"]).max()
    for geo in (a, b):
        r = _lengths(geo["pos"], geo["cell"], geo["skin_ei"], geo["skin_shift"]) / R_MAX
        assert 4 * int((r >= 1.0).sum()) >= len(r)
        assert abs(_pair_length(geo["pos"], geo["cell"], geo["skin_ei"], geo["skin_shift"], 30, 31) / R_MAX - (1.0 + 2.0 ** -7)) < 1e-12


def _observables(m, dev, geo, types, skin, vel):
    g = prepared(m, dev, geo, types, skin=skin)
    e, f, launches = profiled_step(m, torch.tensor(geo["pos"], dtype=m.dtype, device=dev), g)
    out = dict(E=e, F=f, W=m.virial(g), W_split=m.atom_virial(g, "split"), J=m.heat_flux_potential(g, vel),
               dvec=m.debug_tap("dvec", g, with_forces=True), vec=m.debug_tap("vec", g, with_forces=True))
    return dict({k: v.cpu() for k, v in out.items()}, launches=launches, max_degree=int(g.max_degree))


def _forward_of(launches):
    """"fused" / "staged": which forward a launch list shows (the fused forward is ONE launch, `fused_fwd`, whatever its form)."""
    fused, staged = "fused_fwd" in launches, "edge_prologue" in launches
    assert fused != staged, launches
    return "fused" if fused else "staged"


def _skin_case(row, kind, lib, dev, mode=None):
    name, T, dtype, rce = row
    geo = geometry(kind)
    types = species(geo, T)
    cfg = config(T, dtype, rce, 64, geo)
    tag = f"{name}_{kind}" + ("" if mode is None else f"[{mode}]")
    m = build(cfg, lib, dev)
    vel = torch.tensor(np.random.default_rng(9).normal(size=(N_ATOMS, 3)), dtype=m.dtype, device=dev)
    plain = _observables(m, dev, geo, types, False, vel)
    skin = _observables(m, dev, geo, types, True, vel)
    failures = []
    # which forward each list took.  The dispatcher reads the graph's max_degree hint: up to 32 the one-tile form of the fused forward;
    # above it (the skin list of the dense frame) the team / mixed forms, which exist for one and two species only -- three species
    # fall back to the staged forward (their table and the team exchange area exceed the LDS).  The launch list names the fused
    # forward, not its form: that a fused step on a list above 32 is a team-form step is `choose_forward`'s rule (csrc/aa_model.hip),
    # pinned by name in tests/test_step_plan.py (`one_long_atom`, `small_dense`, `three_species_long_atom`).
    print(f"{tag} max_degree {plain['max_degree']} -> {skin['max_degree']}; plain: {' '.join(plain['launches'])}; skin: {' '.join(skin['launches'])}")
    assert plain["max_degree"] <= 32 and (skin["max_degree"] > 32) == (kind == "dense"), (plain["max_degree"], skin["max_degree"])
    can_fuse = fusable(cfg) and mode != "staged"
    assert _forward_of(plain["launches"]) == ("fused" if can_fuse else "staged"), plain["launches"]
    assert _forward_of(skin["launches"]) == ("fused" if can_fuse and not (kind == "dense" and T > 2) else "staged"), skin["launches"]
    assert "edge_backward" in plain["launches"] and "edge_backward" in skin["launches"]
    # the plain list against the oracle
    want = oracle(f"{name}_{kind}", cfg, weights(m), geo["pos"], geo["ei"], geo["shift"] @ geo["cell"], types)
    for what in ("E", "F", "W"):
        try:
            check(tag, what, plain[what], *want[what.lower()])
        except AssertionError as err:
            failures.append(f"plain {what}: {err}")
    # guard: a quarter of the skin list lies beyond the cutoff in the kernel's own lengths, one edge just beyond it
    x = skin["vec"][:, 3].double() / R_MAX
    outside = x >= 1.0
    assert 4 * int(outside.sum()) >= len(x), (int(outside.sum()), len(x))
    assert bool(((x > 1.0) & (x <= 1.0 + 2.0 ** -6)).any())
    # the skin list against the plain list, within the reference's own whole-model tolerance
    for what in ("E", "F", "W", "W_split", "J"):
        got, ref = skin[what], plain[what]
        scale = max(1.0, float(ref.abs().max()))
        err = float((got - ref).abs().max())
        print(f"{tag} skin-plain {what} err {err:.3e} scale {scale:.3e} rel {err / scale:.3e} bound {TOL[m.dtype]:.1e}")
        if not (torch.isfinite(got).all() and err <= TOL[m.dtype] * scale):
            failures.append(f"skin {what}: {err:.3e} > {TOL[m.dtype] * scale:.3e}")
    # dE/dr of the edges beyond the cutoff
    d_out, d_in = skin["dvec"][outside], skin["dvec"][~outside]
    assert torch.isfinite(skin["dvec"]).all() and torch.isfinite(skin["vec"]).all(), tag
    worst = float(d_out.abs().max())
    print(f"{tag} max |dvec| beyond the cutoff {worst:.3e}, inside {float(d_in.abs().max()):.3e}")
    if "num_bessels" in rce:
        if not exactly_zero(d_out):
            failures.append(f"dvec beyond the cutoff is not exactly zero: {worst:.3e}")
    elif worst > torch.finfo(m.dtype).eps * float(d_in.abs().max()):
        failures.append(f"dvec beyond the cutoff: {worst:.3e} > eps x {float(d_in.abs().max()):.3e}")
    assert not failures, tag + "\n" + "\n".join(failures)


def _pin_forward(monkeypatch, mode):
    """The "auto" / "staged" halves of tests/conftest.py::forward_mode for the rows that have no wide form (three species)."""
    monkeypatch.delenv("AA_FUSED_NARROW", raising=False)
    if mode == "staged":
        monkeypatch.setenv("AA_FUSED", "0")
    else:
        monkeypatch.delenv("AA_FUSED", raising=False)


@pytest.mark.parametrize("kind", SKIN_GEOMETRIES)
@pytest.mark.parametrize("row", SKIN_ONE, ids=_ids(SKIN_ONE))
def test_skin_edges_one_species_emulated(row, kind, forward_mode):
    _skin_case(row, kind, *_emu(), mode=forward_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SKIN_GEOMETRIES)
@pytest.mark.parametrize("row", SKIN_ONE, ids=_ids(SKIN_ONE))
def test_skin_edges_one_species_on_gpu(row, kind, forward_mode):
    _skin_case(row, kind, *_gpu(), mode=forward_mode)


@pytest.mark.parametrize("kind", SKIN_GEOMETRIES)
def test_skin_edges_fp64_emulated(kind):
    _skin_case(SKIN_F64, kind, *_emu())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SKIN_GEOMETRIES)
def test_skin_edges_fp64_on_gpu(kind):
    _skin_case(SKIN_F64, kind, *_gpu())


@pytest.mark.parametrize("kind", SKIN_GEOMETRIES)
@pytest.mark.parametrize("mode", ["auto", "staged"])
def test_skin_edges_three_species_emulated(mode, kind, monkeypatch):
    _pin_forward(monkeypatch, mode)
    _skin_case(SKIN_THREE, kind, *_emu(), mode=mode)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SKIN_GEOMETRIES)
@pytest.mark.parametrize("mode", ["auto", "staged"])
def test_skin_edges_three_species_on_gpu(mode, kind, monkeypatch):
    _pin_forward(monkeypatch, mode)
    _skin_case(SKIN_THREE, kind, *_gpu(), mode=mode)


# ---- 4. edge-count boundaries -----------------------------------------------------------------------------------------------
EDGE_COUNTS = [1, 255, 256, 257, 512]
# (name, dtype, transposed CSR, plan options): gather / atomics in edge_backward_kernel; the fp32 shape takes the fused forward unless
# the plan is the staged one (edge_prologue_kernel), the fp64 one has no fused forward
BOUNDARY_FORMS = [
    ("f32_gather", F32, True, {}),
    ("f32_atomics", F32, False, {}),
    ("f32_atomics_staged", F32, False, dict(fused_forward=3)),
    ("f64_gather", F64, True, {}),
    ("f64_atomics", F64, False, {}),
]


def _boundary_case(form, E, lib, dev):
    name, dtype, tcsr, options = form
    geo = geometry("dense")  # (the one with more than 512 edges)
    assert geo["ei"].shape[1] > max(EDGE_COUNTS) and bool((np.diff(geo["ei"][0]) >= 0).all())
    ei, sv = geo["ei"][:, :E], (geo["shift"] @ geo["cell"])[:E]  # (center-sorted: the trailing atoms lose their edges)
    types = np.zeros(N_ATOMS, dtype=np.int64)
    shift_of_type = 0.375
    overrides = dict(r_max=R_MAX, model_dtype=dtype, avg_num_neighbors=float(geo["ei"].shape[1]) / N_ATOMS, per_type_energy_shifts=[shift_of_type])
    if lib is None:
        lib = _lib.load()
    rig = Rig(lib, dev, overrides, options)
    g = PreparedGraph(torch.tensor(ei, device=dev), torch.tensor(types, device=dev), N_ATOMS, torch.tensor(sv, dtype=rig.dtype, device=dev),
                      transposed=tcsr, lib=lib)
    assert g.num_edges == E and (g.t_perm is not None) == tcsr
    pos = torch.tensor(geo["pos"], dtype=rig.dtype, device=dev)
    ws = rig.workspace(rig.workspace_bytes(g, True))
    e, f = rig.outputs(N_ATOMS)
    rig.step(g, pos, ws, e, f)
    rc, w = rig.virial(g, ws)
    assert rc == 0, rig.last_error()
    e, f = e.cpu(), f.cpu()
    tag = f"{name}_E{E}"
    want = oracle(f"boundary_{dtype}_E{E}", dict(rig.cfg), rig.oracle_weights(), geo["pos"], ei, sv, types)
    failures = []
    for what, got in (("E", e), ("F", f), ("W", w)):
        try:
            check(tag, what, got, *want[what.lower()])
        except AssertionError as err:
            failures.append(f"{what}: {err}")
    # atoms that are the center of no edge carry exactly their type's shift; atoms in no edge at all exactly zero force
    bare = torch.tensor(np.bincount(ei[0], minlength=N_ATOMS) == 0)
    untouched = bare & torch.tensor(np.bincount(ei[1], minlength=N_ATOMS) == 0)
    assert int(bare.sum()) > 0 and (E > 257 or int(untouched.sum()) > 0)
    assert bool((e[bare] == shift_of_type).all()), (tag, e[bare])
    assert exactly_zero(f[untouched]), (tag, f[untouched])
    assert not failures, tag + "\n" + "\n".join(failures)


_BOUNDARY = [(form, E) for form in BOUNDARY_FORMS for E in EDGE_COUNTS]
_BOUNDARY_IDS = [f"{form[0]}-E{E}" for form, E in _BOUNDARY]


@pytest.mark.parametrize("form,E", _BOUNDARY, ids=_BOUNDARY_IDS)
def test_edge_count_boundaries_emulated(form, E):
    _boundary_case(form, E, *_emu())


@pytest.mark.gpu
@pytest.mark.parametrize("form,E", _BOUNDARY, ids=_BOUNDARY_IDS)
def test_edge_count_boundaries_on_gpu(form, E):
    _boundary_case(form, E, *_gpu())


# ---- 5. limits are refused before a step starts -----------------------------------------------------------------------------
def _limit_config(T, dtype, rce, embed_dim):
    names = [f"X{t}" for t in range(T)]
    return dict(BASE, type_names=names, r_max=R_MAX, radial_chemical_embed=rce, radial_chemical_embed_dim=embed_dim, avg_num_neighbors=1.0,
                seed=5, model_dtype=dtype, per_type_energy_scales=[1.0 + 0.001 * t for t in range(T)],
                per_type_energy_shifts=[0.002 * t for t in range(T)])


# (name, T, dtype, embedding, radial_chemical_embed_dim, words of the refusal).  The LDS rows come in pairs with their largest accepted
# neighbour below: 8 (256 (16 + 1) + 16 S0) + 2048 <= 65536 holds up to S0 = 224, 8 (256 (8 + 1) + 16 x 128 + 128 T) + 1024 <= 163840 up to
# T = 125
REFUSED = [
    ("bessel17", 1, F32, BESSEL(17), 64, ("num_bessels", "17", "1..16")),
    ("spline17", 1, F32, SPLINE(17, 6), 64, ("num_splines", "17", "1..16")),
    ("prologue_f64_b16_s256", 1, F64, BESSEL(16), 256, ("edge prologue", "69632", "65536", "radial_chemical_embed_dim = 256")),
    ("prologue_f64_b16_s226", 1, F64, BESSEL(16), 226, ("edge prologue", "65792", "65536")),
    ("edge_reverse_f64_s128_T140", 140, F64, BESSEL(8), 128, ("edge reverse", "179200", "163840", "140 types")),
    ("edge_reverse_f64_s128_T126", 126, F64, BESSEL(8), 128, ("edge reverse", "164864", "163840")),
]
ACCEPTED = [
    ("prologue_f64_b16_s224", 1, F64, BESSEL(16), 224),
    ("edge_reverse_f64_s128_T125", 125, F64, BESSEL(8), 128),
]


def _refused_case(row, lib, dev):
    name, T, dtype, rce, embed_dim, words = row
    m = build(_limit_config(T, dtype, rce, embed_dim), lib, dev)
    m._select_device(dev)
    with pytest.raises(_lib.AllegroError) as err:
        m._ensure_plan()  # aa_model_plan_create_with_options: no plan, so no step whose forward could run before the refusal
    msg = str(err.value)
    print(f"{name}: {msg}")
    assert m._plan_handle is None
    assert "aa_model_plan_create failed (-1)" in msg and all(w in msg for w in words), msg  # AA_ERR_INVALID


def _accepted_case(row, lib, dev):
    """The largest accepted neighbour of an LDS row on a graph of one atom pair (types 0 and T - 1)."""
    name, T, dtype, rce, embed_dim = row
    cfg = _limit_config(T, dtype, rce, embed_dim)
    m = build(cfg, lib, dev)
    pos = np.array([[0.0, 0.0, 0.0], [0.9, -0.7, 1.1]])
    ei, types = np.array([[0, 1], [1, 0]]), np.array([0, T - 1])
    g = m.prepare_graph(torch.tensor(ei, device=dev), torch.tensor(types, device=dev), 2)
    e, f, launches = profiled_step(m, torch.tensor(pos, dtype=m.dtype, device=dev), g)
    assert "edge_prologue" in launches and "edge_backward" in launches, launches
    w = m.virial(g)
    want = oracle(name, cfg, weights(m), pos, ei, np.zeros((2, 3)), types)
    for what, got in (("E", e), ("F", f), ("W", w)):
        check(name, what, got.cpu(), *want[what.lower()])


@pytest.mark.parametrize("row", REFUSED, ids=_ids(REFUSED))
def test_limits_are_refused_at_plan_creation_emulated(row):
    _refused_case(row, *_emu())


@pytest.mark.gpu
@pytest.mark.parametrize("row", REFUSED, ids=_ids(REFUSED))
def test_limits_are_refused_at_plan_creation_on_gpu(row):
    _refused_case(row, *_gpu())


@pytest.mark.parametrize("row", ACCEPTED, ids=_ids(ACCEPTED))
def test_largest_accepted_sizes_step_correctly_emulated(row):
    _accepted_case(row, *_emu())


@pytest.mark.gpu
@pytest.mark.parametrize("row", ACCEPTED, ids=_ids(ACCEPTED))
def test_largest_accepted_sizes_step_correctly_on_gpu(row):
    _accepted_case(row, *_gpu())
