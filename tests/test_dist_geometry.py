"""The sharded step (`allegro_amd/dist.py`) on general cells: every constructor of `HaloShard`, every slab axis, three species,
atoms outside the cell, slabs and ranks without atoms.

Reference of every sharded case: ONE step of the same model on the same backend on the whole frame, on the list
`neighbor_list(pos, cell, True, r_max)` -- `E_i`, forces, `virial`, `heat_flux_potential` and `atom_virial` for the three attributions.
The whole-frame step itself is held against `oracle.restatement.allegro_energy_forces` in fp64 on one frame per dtype, so the
reference does not rest on the code under test alone.  Tolerances are the project's (`TOL` of tests/test_dist_observables.py): 1e-9
(fp64) / 5e-5 (fp32) times max(1, max |expected|).

Model: fixture `t_coupled` (three species, r_max 4 A).  Atom types are drawn over all three species and every shard's ghost set holds
at least two of them, so a mix-up of the ghost types moves a number (`test_permuted_ghost_types_move_the_forces`).

Frames (seeded; fractional coordinates in -0.4 .. 1.5, so atoms lie outside the cell; lattice vectors as rows):
  tri      (9, 0, 0), (2.5, 8, 0), (-1.5, 2, 7), 48 atoms
  sheared  (8.5, 0, 0), (6, 8.5, 0), (3, -4, 9), 48 atoms
  thin     (22, 0, 0), (1, 3.5, 0), (0.5, -0.7, 6), 30 atoms: the 3.5 A axis is shorter than r_max (self-image edges, shifts of +-2)
  vacuum   `thin` with every atom at fractional a in [0.55, 0.8) drawn again until none is left there

Parts:
  1  `InProcessHaloGroup.from_positions`, worlds 1, 2, 3, 5, 7 x axis 0, 1, 2 (`thin` / `vacuum`: axes 0 and 1) in fp64, two rows in fp32
  2  `HaloShard.from_graph` cut from the whole list (shifts kept), connected in process
  3  the real collectives under gloo: `from_positions` and `from_owned` through `energy_forces_halo`, collectives counted, slabs
     without atoms (`vacuum` with unequal bounds); one run of two ranks on one device
  4  fewer atoms than ranks
  5  `DeviceNeighborList.ghost_layout` with three species on `tri` and `thin`

The emulated grid of part 1 leaves out world 7 and the `sheared` frame (a step set takes seconds on the emulation); the device grid
(`gpu`) is complete.  Parts 2, 4 and 5 run the same cases on both backends.
"""
import contextlib
import os
import queue as queue_mod
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_dist_observables import ATTRIBUTIONS, TOL, _free_port, close, frame_velocities

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
R_MAX = 4.0
MARGIN = 1.02  # the constructors' halo margin along the slab axis, in units of r_cut
CELLS = {"tri": [[9.0, 0, 0], [2.5, 8.0, 0], [-1.5, 2.0, 7.0]],
         "sheared": [[8.5, 0, 0], [6.0, 8.5, 0], [3.0, -4.0, 9.0]],
         "thin": [[22.0, 0, 0], [1.0, 3.5, 0], [0.5, -0.7, 6.0]]}
CELLS["vacuum"] = CELLS["thin"]
ATOMS = {"tri": 48, "sheared": 48, "thin": 30, "vacuum": 30}
SEEDS = {"tri": 101, "sheared": 102, "thin": 103, "vacuum": 103}
GAP = (0.55, 0.8)
AXES = {"tri": (0, 1, 2), "sheared": (0, 1, 2), "thin": (0, 1), "vacuum": (0, 1)}
WORLDS = (1, 2, 3, 5, 7)
GRID = [(name, axis, world) for name in CELLS for axis in AXES[name] for world in WORLDS]
GRID_EMU = [(name, axis, world) for name, axis, world in GRID if name != "sheared" and world != 7]
GRID_F32 = [("tri", 1, 3), ("thin", 0, 5)]
BOUNDS_ONE_EMPTY = [0.0, 0.3, 0.55, 0.8, 1.0]   # on `vacuum`, axis 0: the third slab owns no atom
BOUNDS_TWO_EMPTY = [0.0, 0.55, 0.65, 0.8, 1.0]  # the second and the third


def case_id(case):
    return "-".join(f"{k}{v}" if isinstance(v, int) else str(v) for k, v in zip(("", "a", "w"), case))


def wrapped(frac):
    return frac - np.floor(frac)


def make_frame(name):
    """(cell [3,3], pos [n,3], types [n]) in numpy float64 / int64; the same on every call and in every process."""
    rng = np.random.default_rng(SEEDS[name])
    cell = np.array(CELLS[name], dtype=np.float64)
    n = ATOMS[name]
    frac = rng.uniform(-0.4, 1.5, size=(n, 3))
    types = rng.integers(0, 3, size=n)
    if name == "vacuum":
        while True:
            a = wrapped(frac[:, 0])
            bad = (a >= GAP[0]) & (a < GAP[1])
            if not bad.any():
                break
            frac[bad, 0] = rng.uniform(-0.4, 1.5, size=int(bad.sum()))
    assert frac.min() < -0.2 and frac.max() > 1.2 and set(types.tolist()) == {0, 1, 2}
    return cell, frac @ cell, types


def slab_coordinate(name, pos, axis):
    """Wrapped fractional coordinate of every atom along lattice direction `axis`, and the cell's height along it."""
    cell = np.array(CELLS[name], dtype=np.float64)
    fx = wrapped(np.linalg.solve(cell.T, np.asarray(pos, dtype=np.float64).T).T[:, axis])
    height = abs(np.linalg.det(cell)) / np.linalg.norm(np.cross(cell[(axis + 1) % 3], cell[(axis + 2) % 3]))
    return fx, float(height)


def within_margin(fx, lo, hi, margin):
    """Atoms inside [lo, hi] or closer than `margin` to it along the periodic axis (wrapped fractional units)."""
    return ((fx >= lo) & (fx <= hi)) | (np.remainder(lo - fx, 1.0) < margin) | (np.remainder(fx - hi, 1.0) < margin)


_WORST = {}


def check(part, name, got, want, dtype):
    """`close`, and the worst error of every (part, dtype) in units of max(1, max |expected|) on the `-s` log."""
    w = want.double()
    rel = float((got.double().to(w.device) - w).abs().max()) / max(1.0, float(w.abs().max()))
    key = (part, "f64" if dtype == F64 else "f32")
    if rel > _WORST.get(key, -1.0):
        _WORST[key] = rel
        print(f"[worst] part {key[0]} {key[1]} {rel:.3e} of max(1, max|expected|), bound {TOL[dtype]:.0e} ({name})")
    close(name, got, want, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the reference: one step on the whole frame
# ---------------------------------------------------------------------------------------------------------------------
_MODELS, _WHOLE = {}, {}


def backend_of(backend):
    if backend == "emu":
        from tests.hip_utils import emu_lib

        return torch.device("cpu"), emu_lib()
    return torch.device("cuda:0"), None


def model_of(backend, dtype):
    if (backend, dtype) not in _MODELS:
        from tests.golden_utils import load_model_fixture
        from tests.hip_utils import model_from_fixture

        dev, lib = backend_of(backend)
        fx = load_model_fixture("t_coupled", dtype)
        assert float(fx["cfg"]["r_max"]) == R_MAX and len(fx["cfg"]["type_names"]) == 3
        _MODELS[(backend, dtype)] = (fx, model_from_fixture(fx, dtype, lib, dev))
    return _MODELS[(backend, dtype)]


def reference_step(m, pos, g, vel):
    e, f = m.energy_forces(pos, g)
    ref = dict(e=e.clone(), f=f.clone(), virial=m.virial(g).clone(), heat_flux=m.heat_flux_potential(g, vel).clone())
    for a in ATTRIBUTIONS:
        ref[a] = m.atom_virial(g, a).clone()
    return ref


def whole(backend, dtype, name):
    """The frame `name` on `backend` in `dtype` and its reference, computed once and only read afterwards:
    dict(m, pos, types, cell, vel, nl, ref)."""
    key = (backend, dtype, name)
    if key not in _WHOLE:
        from allegro_amd.nn import neighbor_list

        dev, lib = backend_of(backend)
        _, m = model_of(backend, dtype)
        cell, pos, types = make_frame(name)
        pos_t = torch.tensor(pos, dtype=dtype, device=dev)
        types_t = torch.tensor(types, device=dev)
        nl = neighbor_list(pos_t, cell, True, R_MAX, lib=lib)
        vel = frame_velocities(len(pos), dtype).to(dev)
        g = nl.prepare(types_t)
        bump = 0.01 * torch.randn(len(pos), 3, dtype=F64, generator=torch.Generator().manual_seed(29)).to(device=dev, dtype=dtype)
        ref_moved = reference_step(m, pos_t + bump, g, vel)  # (the same list at displaced positions: the step in between)
        ref = reference_step(m, pos_t, g, vel)
        assert float((ref_moved["f"] - ref["f"]).abs().max()) > 10 * TOL[dtype] * max(1.0, float(ref["f"].abs().max()))
        assert float(ref["virial"].abs().max()) > 1e-3 and float(ref["heat_flux"].abs().max()) > 1e-3
        assert float((ref["center"] - ref["neighbor"]).abs().max()) > 1e-3
        if name in ("thin", "vacuum"):  # the 3.5 A axis: every atom sees its own images; atoms outside the cell: shifts of two cells
            assert int((nl.edge_index[0] == nl.edge_index[1]).sum()) >= 2 * len(pos)
            assert int(nl.cell_shift.min()) == -2 and int(nl.cell_shift.max()) == 2
        if name == "vacuum":
            a = slab_coordinate(name, pos, 0)[0]
            assert not ((a >= GAP[0]) & (a < GAP[1])).any()
        _WHOLE[key] = dict(m=m, pos=pos_t, types=types_t, cell=cell, vel=vel, nl=nl, ref=ref, bump=bump, ref_moved=ref_moved)
    return _WHOLE[key]


def oracle_case(backend, dtype, name):
    """The whole-frame step against the fp64 restatement on the same (upcast) weights and positions."""
    from oracle import restatement as R

    fx, _ = model_of(backend, dtype)
    w = whole(backend, dtype, name)
    cfg = dict(fx["cfg"], model_dtype="float64")
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in fx["sd"].items()}
    nl = w["nl"]
    out = R.allegro_energy_forces(cfg, sd, w["pos"].double().cpu(), nl.edge_index.long().cpu(), w["types"].cpu(),
                                  nl.cell_shift.double().cpu() @ torch.tensor(w["cell"]))
    check("ref", f"{name} whole frame vs oracle: E_i", w["ref"]["e"], out["atomic_energy"].reshape(-1), dtype)
    check("ref", f"{name} whole frame vs oracle: F", w["ref"]["f"], out["forces"], dtype)


@pytest.mark.parametrize("dtype,name", [pytest.param(F64, "tri", id="f64-tri"), pytest.param(F32, "thin", id="f32-thin")])
def test_whole_frame_reference_against_the_oracle_emu(dtype, name):
    oracle_case("emu", dtype, name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,name", [pytest.param(F64, "tri", id="f64-tri"), pytest.param(F32, "thin", id="f32-thin")])
def test_whole_frame_reference_against_the_oracle_gpu(dtype, name):
    oracle_case("gpu", dtype, name)


# ---------------------------------------------------------------------------------------------------------------------
# parts 1, 2, 4: all shards of a frame in one process
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def listed_atoms(sizes):
    """Appends the atom count of every `neighbor_list` call the constructors make to `sizes`."""
    import allegro_amd.nn as nn_mod

    orig = nn_mod.neighbor_list

    def counting(pos, *a, **k):
        sizes.append(int(pos.shape[0]))
        return orig(pos, *a, **k)

    nn_mod.neighbor_list = counting
    try:
        yield
    finally:
        nn_mod.neighbor_list = orig


def assemble(own, res, key, like):
    out = torch.full_like(like, float("nan"))
    for i, r in zip(own, res):
        out[i] = r[key] if isinstance(key, int) else r[2][key]
    return out


def check_group(part, what, grp, w, dtype, ghosts_expected=True):
    """The shards of `grp` partition atoms and edges of the frame `w`, carry at least two species among their ghosts, and three steps
    (first positions, displaced, first again) give the whole-frame values -- the third the bits of the first."""
    m, pos, vel, ref = w["m"], w["pos"], w["vel"], w["ref"]
    n = pos.shape[0]
    own = [s.owned_ids() for s in grp.shards]
    assert torch.equal(torch.sort(torch.cat(own))[0].cpu(), torch.arange(n))  # every atom is owned by exactly one shard
    assert sum(s.graph.num_edges for s in grp.shards) == w["nl"].num_edges
    for s in grp.shards:
        assert s.graph.num_atoms == s.n_own + s.n_ghost and s.graph.types.numel() == s.n_own + s.n_ghost
        if ghosts_expected:
            assert s.n_ghost > 0 and torch.unique(s.graph.types[s.n_own:]).numel() >= 2, "a ghost set of one species"

    def step(p, attribution, want, what):
        res = grp.step(m, [p[i] for i in own], virial=True, atom_virial=attribution, velocities_own_list=[vel[i] for i in own])
        for i, (e, f, obs) in zip(own, res):
            assert e.shape == (i.numel(),) and f.shape == (i.numel(), 3) and obs["atom_virial"].shape == (i.numel(), 3, 3)
            assert e.dtype == dtype and f.dtype == dtype and obs["atom_virial"].dtype == dtype
            assert obs["virial"].shape == (3, 3) and obs["heat_flux"].shape == (3,)
            assert torch.equal(obs["virial"], res[0][2]["virial"]) and torch.equal(obs["heat_flux"], res[0][2]["heat_flux"])
        check(part, f"{what} E_i", assemble(own, res, 0, want["e"]), want["e"], dtype)
        check(part, f"{what} F", assemble(own, res, 1, want["f"]), want["f"], dtype)
        check(part, f"{what} virial", res[0][2]["virial"], want["virial"], dtype)
        check(part, f"{what} heat flux", res[0][2]["heat_flux"], want["heat_flux"], dtype)
        check(part, f"{what} atom virial, {attribution}", assemble(own, res, "atom_virial", want[attribution]), want[attribution], dtype)
        return res

    # three steps on the persistent buffers: the first positions, displaced ones (another reference), the first again -- the same bits
    first = step(pos, "neighbor", ref, what)
    step(pos + w["bump"], "center", w["ref_moved"], f"{what}, displaced")
    again = step(pos, "split", ref, f"{what}, again")
    for (e0, f0, o0), (e1, f1, o1) in zip(first, again):
        assert torch.equal(e0, e1) and torch.equal(f0, f1)
        assert torch.equal(o0["virial"], o1["virial"]) and torch.equal(o0["heat_flux"], o1["heat_flux"])
    return first


def positions_case(backend, dtype, name, axis, world):
    from allegro_amd.dist import InProcessHaloGroup

    _, lib = backend_of(backend)
    w = whole(backend, dtype, name)
    sizes = []
    with listed_atoms(sizes):
        grp = InProcessHaloGroup.from_positions(w["pos"], w["types"], w["cell"], R_MAX, world, lib=lib, axis=axis)
    # the list of a shard is built of its slab and a halo: no atom further than the margin from the slab's extent along the axis
    fx, height = slab_coordinate(name, w["pos"].double().cpu().numpy(), axis)
    assert len(sizes) == world
    for s, n_listed in zip(grp.shards, sizes):
        mine = fx[s.owned_ids().cpu().numpy()]
        allowed = int(within_margin(fx, mine.min(), mine.max(), MARGIN * R_MAX / height + 1e-9).sum())
        assert s.n_own + s.n_ghost <= n_listed <= max(allowed, s.n_own), (n_listed, allowed)
    mult = max([int(s._rows.shape[1]) for s in grp.shards if s._rows is not None], default=0)
    print(f"{name} axis {axis} W={world}: height {height:.2f} A, largest multiplicity of an accumulation row {mult}, listed atoms {sizes}")
    if world >= 3 and height / world < R_MAX:  # slabs thinner than the cutoff: an owned atom is a ghost on several ranks
        assert mult > 1
    check_group(1, f"{name} axis {axis} W={world}", grp, w, dtype, ghosts_expected=world > 1)


@pytest.mark.parametrize("name,axis,world", GRID_EMU, ids=[case_id(c) for c in GRID_EMU])
def test_group_from_positions_emu(name, axis, world):
    positions_case("emu", F64, name, axis, world)


@pytest.mark.parametrize("name,axis,world", GRID_F32, ids=[case_id(c) for c in GRID_F32])
def test_group_from_positions_f32_emu(name, axis, world):
    positions_case("emu", F32, name, axis, world)


@pytest.mark.gpu
@pytest.mark.parametrize("name,axis,world", GRID, ids=[case_id(c) for c in GRID])
def test_group_from_positions_gpu(name, axis, world):
    positions_case("gpu", F64, name, axis, world)


@pytest.mark.gpu
@pytest.mark.parametrize("name,axis,world", GRID_F32, ids=[case_id(c) for c in GRID_F32])
def test_group_from_positions_f32_gpu(name, axis, world):
    positions_case("gpu", F32, name, axis, world)


def test_permuted_ghost_types_move_the_forces():
    """The sanity half of the species assertion: ghost types of ONE shard rotated by hand -> forces off by more than the tolerance."""
    from allegro_amd.dist import InProcessHaloGroup

    _, lib = backend_of("emu")
    w = whole("emu", F64, "tri")
    grp = InProcessHaloGroup.from_positions(w["pos"], w["types"], w["cell"], R_MAX, 2, lib=lib, axis=0)
    own = [s.owned_ids() for s in grp.shards]
    s = grp.shards[0]
    ghost_types = s.graph.types[s.n_own:].clone()
    assert torch.unique(ghost_types).numel() >= 2
    shift = next(k for k in range(1, ghost_types.numel()) if not torch.equal(torch.roll(ghost_types, k), ghost_types))
    s.graph.types[s.n_own:] = torch.roll(ghost_types, shift)
    f = assemble(own, grp.step(w["m"], [w["pos"][i] for i in own]), 1, w["ref"]["f"])
    err, scale = float((f - w["ref"]["f"]).abs().max()), max(1.0, float(w["ref"]["f"].abs().max()))
    print(f"ghost types of shard 0 rotated by {shift}: max|dF| = {err:.3e}, tolerance {TOL[F64] * scale:.3e}")
    assert err > 1e3 * TOL[F64] * scale
    s.graph.types[s.n_own:] = ghost_types
    f = assemble(own, grp.step(w["m"], [w["pos"][i] for i in own]), 1, w["ref"]["f"])
    check(1, "ghost types restored: F", f, w["ref"]["f"], F64)


def graph_case(backend, dtype, name, world):
    """Part 2: shards cut from the whole center-sorted list (periodic shifts kept), blocks of equal edge count, connected in process."""
    from allegro_amd.dist import HaloShard, InProcessHaloGroup

    w = whole(backend, dtype, name)
    nl, n = w["nl"], w["pos"].shape[0]
    ei = nl.edge_index.long().cpu().numpy()
    sv = nl.shift_vec.cpu().numpy()
    types = w["types"].cpu().numpy()
    shards = [HaloShard.from_graph(ei, types, n, sv, r, world, w["pos"].device, dtype, connect=False) for r in range(world)]
    assert all(s.order is None and not s.connected for s in shards)
    grp = InProcessHaloGroup(shards)
    check_group(2, f"{name} from_graph W={world}", grp, w, dtype)


GRAPH_CASES = [("tri", 2), ("tri", 5), ("thin", 2), ("thin", 5)]


@pytest.mark.parametrize("name,world", GRAPH_CASES, ids=[f"{n}-w{w}" for n, w in GRAPH_CASES])
def test_group_from_graph_emu(name, world):
    graph_case("emu", F64, name, world)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")])
@pytest.mark.parametrize("name,world", GRAPH_CASES, ids=[f"{n}-w{w}" for n, w in GRAPH_CASES])
def test_group_from_graph_gpu(name, world, dtype):
    graph_case("gpu", dtype, name, world)


# -- part 4: fewer atoms than ranks ---------------------------------------------------------------------------------------
FEW_POS = [[1.0, 1.0, 1.0], [2.5, 1.5, 1.2], [6.0, 6.0, 6.0]]  # two within r_max of each other, one alone (images included)
FEW_CELL = np.eye(3) * 9.0


def few_atoms_case(backend, world):
    from allegro_amd.dist import InProcessHaloGroup
    from allegro_amd.nn import neighbor_list

    dtype = F64
    dev, lib = backend_of(backend)
    _, m = model_of(backend, dtype)
    pos = torch.tensor(FEW_POS, dtype=dtype, device=dev)
    types = torch.tensor([0, 1, 2], device=dev)
    vel = frame_velocities(3, dtype).to(dev)
    nl = neighbor_list(pos, FEW_CELL, True, R_MAX, lib=lib)
    assert nl.num_edges == 2 and sorted(nl.edge_index[0].tolist()) == [0, 1]
    ref = reference_step(m, pos, nl.prepare(types), vel)
    grp = InProcessHaloGroup.from_positions(pos, types, FEW_CELL, R_MAX, world, lib=lib)
    counts = [s.n_own for s in grp.shards]
    assert sum(counts) == 3 and counts.count(0) == world - 3
    own = [s.owned_ids() for s in grp.shards]
    assert torch.equal(torch.sort(torch.cat(own))[0].cpu(), torch.arange(3))
    assert sum(s.graph.num_edges for s in grp.shards) == 2
    for attribution in ATTRIBUTIONS:
        res = grp.step(m, [pos[i] for i in own], virial=True, atom_virial=attribution, velocities_own_list=[vel[i] for i in own])
        for s, (e, f, obs) in zip(grp.shards, res):
            assert e.shape == (s.n_own,) and f.shape == (s.n_own, 3) and obs["atom_virial"].shape == (s.n_own, 3, 3)
            assert e.dtype == dtype and f.dtype == dtype and obs["atom_virial"].dtype == dtype
            assert torch.equal(obs["virial"], res[0][2]["virial"]) and torch.equal(obs["heat_flux"], res[0][2]["heat_flux"])
            if s.n_own == 0:
                assert s.n_ghost == 0 and s.local_gids.numel() == 0 and s.graph.num_edges == 0 and sum(s.send_counts) == 0
        what = f"3 atoms, W={world}"
        check(4, f"{what} E_i", assemble(own, res, 0, ref["e"]), ref["e"], dtype)
        check(4, f"{what} F", assemble(own, res, 1, ref["f"]), ref["f"], dtype)
        check(4, f"{what} virial", res[0][2]["virial"], ref["virial"], dtype)
        check(4, f"{what} heat flux", res[0][2]["heat_flux"], ref["heat_flux"], dtype)
        check(4, f"{what} atom virial, {attribution}", assemble(own, res, "atom_virial", ref[attribution]), ref[attribution], dtype)
    plain = grp.step(m, [pos[i] for i in own])
    assert all(len(r) == 2 and r[0].shape == (s.n_own,) and r[1].shape == (s.n_own, 3) for r, s in zip(plain, grp.shards))
    check(4, f"3 atoms, W={world}, plain step: F", assemble(own, plain, 1, ref["f"]), ref["f"], dtype)


@pytest.mark.parametrize("world", [3, 5])
def test_more_ranks_than_atoms_emu(world):
    few_atoms_case("emu", world)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [3, 5])
def test_more_ranks_than_atoms_gpu(world):
    few_atoms_case("gpu", world)


# ---------------------------------------------------------------------------------------------------------------------
# part 3: the real collectives
# ---------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q, case):
    """One rank of `energy_forces_halo` under gloo (the pattern of `_worker` of tests/test_dist_observables.py) on a frame of this
    module.  `case`: dict(name, axis, ctor "positions" | "owned", bounds | None, dtype "f64" | "f32", device)."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from allegro_amd.dist import HaloShard, energy_forces_halo
    from tests.golden_utils import load_model_fixture
    from tests.hip_utils import emu_lib, model_from_fixture

    dtype = F64 if case["dtype"] == "f64" else F32
    dev = torch.device(case["device"])
    lib = emu_lib() if dev.type == "cpu" else None
    m = model_from_fixture(load_model_fixture("t_coupled", dtype), dtype, lib, dev)
    name, axis = case["name"], case["axis"]
    cell, pos_np, types_np = make_frame(name)
    pos, types = torch.tensor(pos_np, dtype=dtype, device=dev), torch.tensor(types_np, device=dev)
    n = pos.shape[0]
    fx, height = slab_coordinate(name, pos.double().cpu().numpy(), axis)
    sent = []  # rows of every float all_to_all of the set-up: the candidates' positions
    orig_a2a, orig_ar = dist.all_to_all_single, dist.all_reduce

    def recording(out, inp, *a, **k):
        if out.is_floating_point():
            sent.append(int(out.shape[0]))
        return orig_a2a(out, inp, *a, **k)

    dist.all_to_all_single = recording
    try:
        if case["ctor"] == "owned":  # a domain-decomposed host: every rank is handed ONLY the atoms of its slab
            bounds = case["bounds"] if case["bounds"] is not None else [r / world for r in range(world + 1)]
            ids = torch.tensor(np.nonzero((fx >= bounds[rank]) & (fx < bounds[rank + 1]))[0], device=dev)
            sh = HaloShard.from_owned(pos[ids].contiguous(), types[ids], cell, R_MAX, rank, world, axis=axis, bounds=case["bounds"], lib=lib)
            assert sh.order is None and sh.n_own == ids.numel()
            # set-up traffic: the candidates of the slab's surroundings only, not the frame
            others = np.ones(n, dtype=bool)
            others[ids.cpu().numpy()] = False
            allowed = int((within_margin(fx, bounds[rank], bounds[rank + 1], MARGIN * R_MAX / height + 1e-9) & others).sum())
            assert len(sent) == 1 and sent[0] <= allowed, (sent, allowed)
        else:
            sh = HaloShard.from_positions(pos, types, cell, R_MAX, rank, world, axis=axis, lib=lib)
            ids = sh.owned_ids()
            assert sent == []
    finally:
        dist.all_to_all_single = orig_a2a
    assert sh.connected and sh.host_staged == (dev.type == "cuda")
    pos_own = pos[ids].contiguous()
    vel_own = frame_velocities(n, dtype).to(dev)[ids].contiguous()
    calls = {"a2a": 0, "ar": 0}
    dist.all_to_all_single = lambda *a, **k: (calls.__setitem__("a2a", calls["a2a"] + 1), orig_a2a(*a, **k))[1]
    dist.all_reduce = lambda *a, **k: (calls.__setitem__("ar", calls["ar"] + 1), orig_ar(*a, **k))[1]
    try:
        plain = energy_forces_halo(m, pos_own + 0.01, sh)
        assert len(plain) == 2 and (calls["a2a"], calls["ar"]) == (2, 0), calls  # forward + reverse, nothing else
        calls.update(a2a=0, ar=0)
        e, f, obs = energy_forces_halo(m, pos_own, sh, virial=True, atom_virial="neighbor", velocities_own=vel_own)
        # the two of the plain step + velocities forward + 9-wide rows in reverse, and ONE all-reduce of the 9 + 3 numbers
        assert (calls["a2a"], calls["ar"]) == (4, 1), calls
        calls.update(a2a=0, ar=0)
        _, _, obs_c = energy_forces_halo(m, pos_own, sh, atom_virial="center")
        assert (calls["a2a"], calls["ar"]) == (2, 0), calls  # (the center attribution is local)
        calls.update(a2a=0, ar=0)
        _, _, obs_s = energy_forces_halo(m, pos_own, sh, atom_virial="split")
        assert (calls["a2a"], calls["ar"]) == (3, 0), calls
    finally:
        dist.all_to_all_single, dist.all_reduce = orig_a2a, orig_ar
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert e.dtype == dtype and f.dtype == dtype and obs["virial"].dtype == dtype and obs["heat_flux"].dtype == dtype
    parts = [None] * world
    dist.all_gather_object(parts, dict(ids=ids.cpu(), e=e.cpu(), f=f.cpu(), virial=obs["virial"].cpu(), heat_flux=obs["heat_flux"].cpu(),
                                       neighbor=obs["atom_virial"].cpu(), center=obs_c["atom_virial"].cpu(), split=obs_s["atom_virial"].cpu(),
                                       mult=0 if sh._rows is None else int(sh._rows.shape[1]), edges=sh.graph.num_edges,
                                       ghost_species=int(torch.unique(sh.graph.types[sh.n_own:]).numel())))
    if rank == 0:
        got = dict(e=torch.zeros(n, dtype=dtype), f=torch.zeros(n, 3, dtype=dtype), **{a: torch.zeros(n, 3, 3, dtype=dtype) for a in ATTRIBUTIONS})
        for p in parts:
            assert p["e"].shape == (p["ids"].numel(),) and p["f"].shape == (p["ids"].numel(), 3)
            assert all(p[a].shape == (p["ids"].numel(), 3, 3) for a in ATTRIBUTIONS)
            for k in got:
                got[k][p["ids"]] = p[k]
        # (numpy arrays: pickled by value, see `_worker` of tests/test_dist_observables.py)
        q.put(dict({k: v.numpy() for k, v in got.items()}, virial=[p["virial"].numpy() for p in parts],
                   heat_flux=[p["heat_flux"].numpy() for p in parts], mult=max(p["mult"] for p in parts),
                   owned=[int(p["ids"].numel()) for p in parts], edges=sum(p["edges"] for p in parts),
                   ghost_species=[p["ghost_species"] for p in parts],
                   ids=np.sort(np.concatenate([p["ids"].numpy() for p in parts]))))
    dist.barrier()
    dist.destroy_process_group()


def run_ranks(world, case):
    """Spawns the ranks and returns what rank 0 assembled.  Every rank has to return: one that dies ends the wait at once."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, case["port"], q, case)) for r in range(world)]
    for p in procs:
        p.start()
    got = None
    try:
        for _ in range(600):
            try:
                got = q.get(timeout=1)
                break
            except queue_mod.Empty:
                dead = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
                assert not dead, f"ranks died (rank, exit code): {dead}"
        assert got is not None, "no result from rank 0"
        for p in procs:
            p.join(timeout=120)
        assert [p.exitcode for p in procs] == [0] * world
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return got


def gloo_case(name, axis, world, ctor, bounds=None, dtype=F64, backend="emu"):
    w = whole(backend, dtype, name)
    ref = w["ref"]
    case = dict(name=name, axis=axis, ctor=ctor, bounds=bounds, dtype="f64" if dtype == F64 else "f32",
                device="cpu" if backend == "emu" else "cuda:0", port=_free_port())
    got = run_ranks(world, case)
    n = ref["e"].shape[0]
    what = f"gloo {name} axis {axis} W={world} ({ctor}{'' if bounds is None else ', bounds ' + str(bounds)})"
    print(f"{what}: owned atoms {got['owned']}, largest multiplicity {got['mult']}, ghost species {got['ghost_species']}")
    assert np.array_equal(got["ids"], np.arange(n)) and got["edges"] == w["nl"].num_edges
    t = lambda v: torch.from_numpy(v)  # noqa: E731
    check(3, f"{what} E_i", t(got["e"]), ref["e"].cpu(), dtype)
    check(3, f"{what} F", t(got["f"]), ref["f"].cpu(), dtype)
    for a in ATTRIBUTIONS:
        check(3, f"{what} atom virial, {a}", t(got[a]), ref[a].cpu(), dtype)
    check(3, f"{what} virial", t(got["virial"][0]), ref["virial"].cpu(), dtype)
    check(3, f"{what} heat flux", t(got["heat_flux"][0]), ref["heat_flux"].cpu(), dtype)
    assert len(got["virial"]) == world and len(got["heat_flux"]) == world
    for v, j in zip(got["virial"], got["heat_flux"]):  # the same bits on every rank
        assert np.array_equal(v, got["virial"][0]) and np.array_equal(j, got["heat_flux"][0])
    return got


@pytest.mark.parametrize("ctor", ["positions", "owned"])
@pytest.mark.parametrize("name,axis,world", GRID_F32, ids=[case_id(c) for c in GRID_F32])
def test_gloo_ranks_on_general_cells(name, axis, world, ctor):
    got = gloo_case(name, axis, world, ctor)
    assert all(c > 0 for c in got["owned"]) and all(k >= 2 for k in got["ghost_species"])
    fx, height = slab_coordinate(name, make_frame(name)[1], axis)
    if height / world < R_MAX:
        assert got["mult"] > 1


@pytest.mark.parametrize("bounds,empty", [(BOUNDS_ONE_EMPTY, [2]), (BOUNDS_TWO_EMPTY, [1, 2])], ids=["one-empty", "two-adjacent-empty"])
def test_gloo_ranks_with_slabs_over_vacuum(bounds, empty):
    """`from_owned` on `vacuum` with slabs that own no atom: every rank returns (run_ranks), an empty rank returns `E_i` [0] and
    forces [0, 3] (asserted in the worker for every rank: rows = owned atoms) and the frame's virial and heat flux like the others."""
    got = gloo_case("vacuum", 0, 4, "owned", bounds=bounds)
    assert [r for r, c in enumerate(got["owned"]) if c == 0] == empty


@pytest.mark.gpu
def test_two_ranks_on_one_device_on_a_triclinic_cell():
    got = gloo_case("tri", 1, 2, "owned", dtype=F32, backend="gpu")
    assert all(c > 0 for c in got["owned"]) and all(k >= 2 for k in got["ghost_species"])


# ---------------------------------------------------------------------------------------------------------------------
# part 5: the ghost-atom layout of the device list
# ---------------------------------------------------------------------------------------------------------------------
def ghost_layout_case(backend, dtype, name):
    w = whole(backend, dtype, name)
    m, pos, types, nl, ref = w["m"], w["pos"], w["types"], w["nl"], w["ref"]
    n = pos.shape[0]
    pos_x, types_x, ei_x, src = nl.ghost_layout(pos, types)
    ei = nl.edge_index.long()
    outside = (nl.cell_shift != 0).any(dim=1)
    n_ghost = int(outside.sum())
    assert 0 < n_ghost < nl.num_edges
    assert pos_x.shape == (n + n_ghost, 3) and types_x.shape == (n + n_ghost,) and ei_x.shape == (2, nl.num_edges) and src.shape == (n_ghost,)
    assert torch.equal(src, ei[1][outside])
    assert torch.equal(types_x[:n], types) and torch.equal(types_x[n:], types[src]) and torch.unique(types_x[n:]).numel() == 3
    assert torch.equal(pos_x[:n], pos)
    shift = (nl.cell_shift[outside].double().cpu() @ torch.tensor(w["cell"])).to(pos.device)
    check(5, f"{name} ghost positions", pos_x[n:], pos[src].double() + shift, dtype)
    # edges: the same centers in the same order; inside the cell the same neighbour, outside one ghost per edge, in edge order
    assert torch.equal(ei_x[0], ei[0]) and torch.equal(ei_x[1][~outside], ei[1][~outside])
    assert torch.equal(ei_x[1][outside], n + torch.arange(n_ghost, device=pos.device))
    e, f = m.energy_forces(pos_x, m.prepare_graph(ei_x, types_x, n + n_ghost))
    check(5, f"{name} ghost layout: E_i of the real atoms", e[:n], ref["e"], dtype)
    check(5, f"{name} ghost layout: ghost forces folded onto ghost_source", f[:n].clone().index_add_(0, src, f[n:]), ref["f"], dtype)


@pytest.mark.parametrize("dtype", [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")])
@pytest.mark.parametrize("name", ["tri", "thin"])
def test_device_ghost_layout_on_general_cells_emu(name, dtype):
    ghost_layout_case("emu", dtype, name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")])
@pytest.mark.parametrize("name", ["tri", "thin"])
def test_device_ghost_layout_on_general_cells_gpu(name, dtype):
    ghost_layout_case("gpu", dtype, name)
