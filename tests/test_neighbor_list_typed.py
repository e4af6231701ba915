"""Per-type-pair cutoffs in the device neighbour list: the typed build (aa_nl_count_typed / aa_nl_fill_typed), the pruning of
an existing list (aa_graph_prune_*) and the model on the shorter lists.

An edge i -> j is listed iff |r| < min(r_cut, table[type_i, type_j]).  Oracle of the lists: a numpy float64 enumeration of every
image with that predicate, and the untyped list masked by it (which pins the order).  Oracle of the model: the fixtures' recorded
reference outputs, computed on the FULL list -- the edges the typed list drops are exact zeros behind the model's envelope.

Every list case first asserts, in numpy, that no pair distance lies within a relative 1e-5 of its cutoff: the typed build forms a
distance from wrapped double positions, the pruning from `pos` and `shift_vec` in the positions' dtype, numpy from unwrapped
positions, and only away from the cutoff do all three classify a pair alike.  That is a condition on the inputs (the seeds below
satisfy it), not a tolerance on the result.

`emu`: the unmodified kernels under the CPU emulation; `gpu`: the gfx950 library on the device.
"""
import itertools

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd.nn import neighbor_list

# the reference's own whole-model tolerances (tests/test_hip_model.py: TOL), relative to max(1, |want|max)
TOL = {torch.float64: 1e-9, torch.float32: 5e-5}
DTYPES = [pytest.param(torch.float64, id="f64"), pytest.param(torch.float32, id="f32")]
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
GAP = 1e-5


def _backend(name):
    if name == "emu":
        from tests.hip_utils import emu_lib

        return emu_lib(), torch.device("cpu")
    return _lib.load(), torch.device("cuda:0")


# the five geometries of tests/test_neighbor_list.py::CASES, a dense one (~97 neighbours per atom: segments longer than a wave,
# two passes of the pruning kernel; a box barely larger than the cutoff) and one of 300 atoms (two workgroups of the pair kernels)
CASES = {
    "orthorhombic": (lambda r: r.uniform(0, 1, (60, 3)) * [13.0, 11.0, 12.0], np.diag([13.0, 11.0, 12.0]), (1, 1, 1), 3.1),
    "small_box_many_images": (lambda r: r.uniform(0, 1, (5, 3)) * [2.2, 3.0, 7.5], np.diag([2.2, 3.0, 7.5]), (1, 1, 1), 3.4),
    "triclinic": (lambda r: r.uniform(-0.3, 1.4, (40, 3)) @ np.array([[9.0, 0, 0], [2.5, 8.0, 0], [-1.5, 2.0, 7.0]]),
                  np.array([[9.0, 0, 0], [2.5, 8.0, 0], [-1.5, 2.0, 7.0]]), (1, 1, 1), 3.0),
    "slab_with_atoms_outside": (lambda r: r.uniform(-0.4, 1.5, (50, 3)) * [8.0, 9.0, 14.0], np.diag([8.0, 9.0, 14.0]),
                                (1, 1, 0), 3.2),
    "molecule_no_pbc": (lambda r: r.uniform(0, 6.0, (20, 3)), np.diag([6.0, 6.0, 6.0]), (0, 0, 0), 2.5),
    "dense_long_segments": (lambda r: r.uniform(0, 3.6, (40, 3)), np.diag([3.6, 3.6, 3.6]), (1, 1, 1), 3.0),
    "two_workgroups": (lambda r: r.uniform(0, 30.0, (300, 3)), np.diag([30.0, 30.0, 30.0]), (1, 1, 1), 3.0),
}
# per geometry, the first seed for which every table below and both dtypes meet the input condition of the module docstring (no
# pair distance within a relative 1e-5 of its cutoff); brute_force_typed asserts it
SEEDS = {name: 0 for name in CASES}


def make_table(kind, rc):
    """[T, T] cutoffs (row = center type, column = neighbour type) for the cutoff `rc` of the list."""
    if kind == "symmetric":
        return np.array([[1.0, 0.8, 0.6], [0.8, 0.9, 0.7], [0.6, 0.7, 0.5]]) * rc
    if kind == "asymmetric":  # one row at half the others
        return np.array([[1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]]) * rc
    if kind == "empty_pair":  # centers of type 0 see no neighbour of type 2 at all
        t = np.full((3, 3), 1.0) * rc
        t[0, 2] = 1e-3
        return t
    if kind == "all_beyond_r_cut":  # nothing to drop: the untyped list, bit for bit
        return np.array([[1.0, 1.5, 2.0], [1.25, 1.0, 3.0], [2.0, 1.0, 1.75]]) * rc
    if kind == "one_type":  # T = 1, and a table whose largest entry is smaller than r_cut: the grid follows it
        return np.array([[0.8]]) * rc
    raise KeyError(kind)


TABLES = ["symmetric", "asymmetric", "empty_pair", "all_beyond_r_cut", "one_type"]


def make_case(name, kind, dtype):
    """Positions rounded to `dtype` (what the library sees), types, table, and the enumeration they are judged by."""
    gen, cell, pbc, rc = CASES[name]
    rng = np.random.default_rng(SEEDS[name])
    pos = torch.tensor(gen(rng), dtype=dtype)
    table = make_table(kind, rc)
    types = rng.integers(0, table.shape[0], size=pos.shape[0])
    return pos, np.asarray(cell, np.float64), pbc, rc, types, table


_ENUM = {}


def enumerate_images(pos, cell, pbc, r_cut):
    """numpy float64: every (i, j, S, |pos[j] - pos[i] + S @ cell|) with a distance below 1.01 r_cut (i == j only for S != 0)."""
    key = (pos.tobytes(), cell.tobytes(), tuple(pbc), r_cut)
    if key in _ENUM:
        return _ENUM[key]
    inv = np.linalg.inv(cell)
    h = 1.0 / np.linalg.norm(inv, axis=0)
    frac = pos @ inv
    span = np.ceil(frac.max(0) - frac.min(0)).astype(int) if len(pos) else np.zeros(3, int)
    reps = [range(-(int(np.ceil(1.01 * r_cut / h[a])) + span[a]), int(np.ceil(1.01 * r_cut / h[a])) + span[a] + 1) if pbc[a] else [0]
            for a in range(3)]
    out = []
    for S in itertools.product(*reps):
        d = pos[None, :, :] + (np.array(S) @ cell)[None, None, :] - pos[:, None, :]
        r = np.sqrt((d ** 2).sum(-1))
        ii, jj = np.nonzero(r < 1.01 * r_cut)
        for i, j in zip(ii, jj):
            if i != j or any(S):
                out.append((int(i), int(j)) + tuple(int(s) for s in S) + (float(r[i, j]),))
    _ENUM[key] = out
    return out


def brute_force_typed(pos, cell, pbc, r_cut, types, table):
    """The edge set {(i, j, S)} of the per-pair predicate; asserts the gap condition of the module docstring on the way."""
    pos = np.asarray(pos, np.float64)
    out = set()
    for i, j, s0, s1, s2, r in enumerate_images(pos, cell, pbc, r_cut):
        cut = min(r_cut, table[types[i], types[j]])
        assert abs(r - cut) > GAP * cut and abs(r - r_cut) > GAP * r_cut, "input condition: a pair distance within 1e-5 of its cutoff"
        if r < cut:
            out.add((i, j, s0, s1, s2))
    return out


def edges_of(nl):
    ei, cs = nl.edge_index.cpu().numpy(), nl.cell_shift.cpu().numpy()
    return [(int(ei[0, e]), int(ei[1, e])) + tuple(int(s) for s in cs[e]) for e in range(ei.shape[1])]


def predicate_mask(nl, pos, cell, r_cut, types, table):
    """Which edges of the list `nl` pass the per-pair predicate, in numpy float64 from pos and the integer cell shifts."""
    ei, cs = nl.edge_index.cpu().numpy().astype(np.int64), nl.cell_shift.cpu().numpy().astype(np.float64)
    p = pos.double().cpu().numpy()
    r = np.linalg.norm(p[ei[1]] - p[ei[0]] + cs @ cell, axis=1)
    return r < np.minimum(r_cut, table[types[ei[0]], types[ei[1]]])


def assert_lists_equal(a, b, what):
    assert torch.equal(a.rowptr, b.rowptr), f"{what}: rowptr"
    assert torch.equal(a.edge_index, b.edge_index), f"{what}: edge_index"
    assert torch.equal(a.cell_shift, b.cell_shift), f"{what}: cell_shift"
    assert a.shift_vec.dtype == b.shift_vec.dtype and torch.equal(a.shift_vec, b.shift_vec), f"{what}: shift_vec"  # (bitwise)


def build_lists(name, kind, dtype, lib, dev):
    pos, cell, pbc, rc, types, table = make_case(name, kind, dtype)
    want = brute_force_typed(pos.double().numpy(), cell, pbc, rc, types, table)
    p = pos.to(dev)
    t64 = torch.tensor(types, dtype=torch.int64, device=dev)
    typed = neighbor_list(p, cell, pbc, rc, lib=lib, atom_types=t64, cutoffs=table)
    # the list whose order the typed one keeps: untyped at the radius the typed grid is sized by
    base = neighbor_list(p, cell, pbc, min(rc, float(table.max())), lib=lib)
    return dict(pos=p, cell=cell, pbc=pbc, rc=rc, types=types, t64=t64, table=table, want=want, typed=typed, base=base)


# ---------------------------------------------------------------------------------------------------------------------
# 1. typed build vs brute force, vs the masked untyped list
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("name", list(CASES))
def test_typed_list_matches_brute_force_and_masked_untyped_list(name, kind, dtype, backend):
    lib, dev = _backend(backend)
    c = build_lists(name, kind, dtype, lib, dev)
    typed, base, N = c["typed"], c["base"], c["pos"].shape[0]
    got = edges_of(typed)
    assert len(got) == len(set(got)), "duplicate edges"
    assert set(got) == c["want"], (len(got), len(c["want"]))
    ei, rp = typed.edge_index.cpu().long(), typed.rowptr.cpu().long()
    assert rp.numel() == N + 1 and int(rp[0]) == 0 and int(rp[-1]) == typed.num_edges
    assert torch.equal(rp[1:] - rp[:-1], torch.bincount(ei[0], minlength=N))
    assert bool((ei[0, 1:] >= ei[0, :-1]).all()) if ei.shape[1] > 1 else True
    # order: the untyped list with the dropped edges removed, element by element
    keep = torch.tensor(predicate_mask(base, c["pos"], c["cell"], c["rc"], c["types"], c["table"]), device=dev)
    assert torch.equal(typed.edge_index, base.edge_index[:, keep])
    assert torch.equal(typed.cell_shift, base.cell_shift[keep])
    assert typed.shift_vec.dtype == dtype and torch.equal(typed.shift_vec, base.shift_vec[keep])
    if kind == "all_beyond_r_cut":
        assert bool(keep.all())
        assert_lists_equal(typed, base, "a table that reaches r_cut everywhere")
    elif kind == "empty_pair":
        tc, tn = c["types"][ei[0].numpy()], c["types"][ei[1].numpy()]
        assert not ((tc == 0) & (tn == 2)).any()
        if name != "small_box_many_images":  # (5 atoms: the draw has no such pair)
            bi = base.edge_index.cpu().numpy()
            assert ((c["types"][bi[0]] == 0) & (c["types"][bi[1]] == 2)).any(), "vacuous: the untyped list has no such pair either"
    n_full = sum(1 for e in enumerate_images(c["pos"].double().cpu().numpy(), c["cell"], c["pbc"], c["rc"]) if e[-1] < c["rc"])
    if kind != "all_beyond_r_cut" and not (name == "small_box_many_images" and kind in ("asymmetric", "empty_pair")):
        assert typed.num_edges < n_full, "vacuous: nothing was dropped"  # (the 5-atom draw has no center of type 1 and no 0 -> 2 pair)
    # int32 types: the same list
    t32 = neighbor_list(c["pos"], c["cell"], c["pbc"], c["rc"], lib=lib, atom_types=c["t64"].to(torch.int32), cutoffs=c["table"])
    assert_lists_equal(t32, typed, "int32 vs int64 atom types")
    assert typed.kept is None


# ---------------------------------------------------------------------------------------------------------------------
# 2. pruning an existing list == building the typed one
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("name", list(CASES))
def test_prune_equals_typed_build(name, kind, dtype, backend):
    lib, dev = _backend(backend)
    c = build_lists(name, kind, dtype, lib, dev)
    typed, base = c["typed"], c["base"]
    for types in (c["t64"], c["t64"].to(torch.int32)):
        pruned = base.prune(c["pos"], types, c["table"])
        assert_lists_equal(pruned, typed, f"prune ({types.dtype})")
        kept = pruned.kept.long()
        assert pruned.kept.dtype == torch.int32 and kept.numel() == typed.num_edges
        assert bool((kept[1:] > kept[:-1]).all()) if kept.numel() > 1 else True  # (stable: input order)
        assert torch.equal(base.edge_index[:, kept], pruned.edge_index) and torch.equal(base.cell_shift[kept], pruned.cell_shift)
        assert torch.equal(base.shift_vec[kept], pruned.shift_vec)
    assert base.kept is None


@pytest.mark.parametrize("backend", BACKENDS)
def test_prune_empty_list_isolated_atoms_and_emptied_segment(backend):
    lib, dev = _backend(backend)
    table = np.array([[2.0, 0.5], [0.5, 2.0]])
    # no atoms
    nl = neighbor_list(torch.zeros((0, 3), dtype=torch.float64, device=dev), np.eye(3) * 5, True, 2.0, lib=lib)
    pr = nl.prune(torch.zeros((0, 3), dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), table)
    assert pr.num_edges == 0 and pr.rowptr.tolist() == [0] and pr.kept.numel() == 0
    ty = neighbor_list(torch.zeros((0, 3), dtype=torch.float64, device=dev), np.eye(3) * 5, True, 2.0, lib=lib,
                       atom_types=torch.zeros(0, dtype=torch.int64, device=dev), cutoffs=table)
    assert ty.num_edges == 0 and ty.rowptr.tolist() == [0]
    # isolated atoms: an empty list with rows
    pos = torch.tensor([[0.0, 0, 0], [10.0, 10, 10]], dtype=torch.float64, device=dev)
    t = torch.tensor([0, 1], device=dev)
    nl = neighbor_list(pos, np.eye(3) * 40, True, 2.0, lib=lib)
    pr = nl.prune(pos, t, table)
    assert pr.num_edges == 0 and pr.rowptr.tolist() == [0, 0, 0] and tuple(pr.cell_shift.shape) == (0, 3)
    ty = neighbor_list(pos, np.eye(3) * 40, True, 2.0, lib=lib, atom_types=t, cutoffs=table)
    assert ty.num_edges == 0 and ty.rowptr.tolist() == [0, 0, 0]
    # atom 1 (type 1) has only type-0 neighbours, at 0.7 and 1.1 > 0.5: its segment empties; atoms 0 and 2 keep each other (1.8 < 2)
    pos = torch.tensor([[0.0, 0, 0], [0.7, 0, 0], [1.8, 0, 0], [20.0, 20, 20]], dtype=torch.float32, device=dev)
    t = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=dev)
    nl = neighbor_list(pos, np.eye(3) * 40, True, 2.0, lib=lib)
    assert nl.rowptr.tolist() == [0, 2, 4, 6, 6]
    pr = nl.prune(pos, t, table)
    ty = neighbor_list(pos, np.eye(3) * 40, True, 2.0, lib=lib, atom_types=t, cutoffs=table)
    for got in (pr, ty):
        assert got.rowptr.tolist() == [0, 1, 1, 2, 2]
        assert got.edge_index.tolist() == [[0, 2], [2, 0]]
    assert pr.kept.tolist() == [1, 4]
    assert_lists_equal(pr, ty, "emptied segment")


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. the model on the typed list: fixtures that carry per-type cutoffs
# ---------------------------------------------------------------------------------------------------------------------
PEREDGE_FIXTURES = ["t_peredge", "t_spline_peredge", "t_mish"]
# per_edge_type_cutoff = {"H": 2.0, "C": {"H": 4.0, "C": 3.5, "O": 3.7}, "O": 3.9} of these fixtures, written out (H, C, O)
PEREDGE_TABLE = [[2.0, 2.0, 2.0], [4.0, 3.5, 3.7], [3.9, 3.9, 3.9]]


def _close(name, got, want, dtype):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"{name}: max error {err:.3e}, bound {TOL[dtype] * scale:.3e}")
    assert err <= TOL[dtype] * scale, f"{name}: {err:.3e} > {TOL[dtype] * scale:.3e}"


def _fixture_setup(name, dtype, lib, dev):
    from oracle import make_golden as MG
    from tests.golden_utils import load_model_fixture
    from tests.hip_utils import fixture_data, model_from_fixture

    fx = load_model_fixture(name, dtype)
    m = model_from_fixture(fx, dtype, lib, dev)
    data, _ = fixture_data(fx, dtype, dev)
    g = MG.molecule_graph()  # the geometry of these fixtures: 24 atoms, box 9 A, list at 4 A
    assert np.allclose(g.pos, fx["pos"].double().numpy())
    return fx, m, data, g


def _model_parity_case(name, dtype, lib, dev):
    fx, m, data, g = _fixture_setup(name, dtype, lib, dev)
    pos, types = data["pos"], data["atom_types"]
    nl = m.neighbor_list(pos, g.cell, True, types)
    # guards: the list is the per-pair one, and it is shorter where it should be
    tnp = fx["types"].numpy()
    want = brute_force_typed(fx["pos"].double().numpy(), np.asarray(g.cell, np.float64), (1, 1, 1), 4.0, tnp, np.array(PEREDGE_TABLE))
    full_edges = fx["edge_index"].shape[1]
    assert set(edges_of(nl)) == want and nl.num_edges == len(want)
    assert nl.num_edges < full_edges
    deg_full = np.bincount(fx["edge_index"][0].numpy(), minlength=24)
    deg = (nl.rowptr[1:] - nl.rowptr[:-1]).cpu().numpy()
    assert ((deg < deg_full) & (tnp == 0)).any(), "no H-centered segment lost edges"
    e, f = m.energy_forces(pos, nl.prepare(types))
    ref = fx["out"]  # the reference's outputs on the FULL list
    _close(f"{name} E_i", e, ref["atomic_energy"].reshape(-1), dtype)
    _close(f"{name} F", f, ref["forces"], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", PEREDGE_FIXTURES)
def test_model_on_typed_list_matches_reference_outputs_emulated(name, dtype):
    _model_parity_case(name, dtype, *_backend("emu"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", PEREDGE_FIXTURES)
def test_model_on_typed_list_matches_reference_outputs_on_gpu(name, dtype, forward_mode):
    _model_parity_case(name, dtype, *_backend("gpu"))


def _derived_case(name, dtype, lib, dev):
    """virial and the split per-atom virial on the typed graph == the same calls on the full graph."""
    fx, m, data, g = _fixture_setup(name, dtype, lib, dev)
    pos, types = data["pos"], data["atom_types"]
    out = {}
    for tag, nl in (("full", neighbor_list(pos, g.cell, True, 4.0, lib=lib)), ("typed", m.neighbor_list(pos, g.cell, True, types))):
        graph = nl.prepare(types)
        e, f = m.energy_forces(pos, graph)
        out[tag] = dict(E=nl.num_edges, e=e.clone(), f=f.clone(), w=m.virial(graph).clone(), aw=m.atom_virial(graph, "split").clone())
    assert out["typed"]["E"] < out["full"]["E"] == fx["edge_index"].shape[1]
    for k in ("e", "f", "w", "aw"):
        _close(f"{name} {k}", out["typed"][k], out["full"][k], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", PEREDGE_FIXTURES)
def test_virial_and_atom_virial_on_typed_list_emulated(name, dtype):
    _derived_case(name, dtype, *_backend("emu"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", PEREDGE_FIXTURES)
def test_virial_and_atom_virial_on_typed_list_on_gpu(name, dtype, forward_mode):
    _derived_case(name, dtype, *_backend("gpu"))


def _zbl_case(dtype, lib, dev):
    """The ZBL model and frame of tests/test_pair_zbl.py (Si-O shortened to 2.4 A inside r_max = 3.4 A): typed list == full list."""
    from tests.test_pair_zbl import R_MAX, build, main_cfg, main_frame

    fr = main_frame()
    m = build(main_cfg(dtype, fr), lib, dev)
    assert m.describe_plan()["pair"] == "zbl"
    pos = torch.tensor(fr["pos"], dtype=dtype, device=dev)
    types = torch.tensor(fr["types"], device=dev)
    full = neighbor_list(pos, fr["cell"], True, R_MAX, lib=lib)
    typed = m.neighbor_list(pos, fr["cell"], True, types)
    assert typed.num_edges < full.num_edges == fr["ei"].shape[1]
    e0, f0 = (x.clone() for x in m.energy_forces(pos, full.prepare(types)))
    e1, f1 = m.energy_forces(pos, typed.prepare(types))
    _close("zbl E_i", e1, e0, dtype)
    _close("zbl F", f1, f0, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zbl_model_on_typed_list_emulated(dtype):
    _zbl_case(dtype, *_backend("emu"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_zbl_model_on_typed_list_on_gpu(dtype, forward_mode):
    _zbl_case(dtype, *_backend("gpu"))


# ---------------------------------------------------------------------------------------------------------------------
# 5. interface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_interface_errors_name_the_argument(backend):
    from allegro_amd._lib import AllegroError

    lib, dev = _backend(backend)
    pos = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [0, 1.6, 0]], dtype=torch.float64, device=dev)
    cell = np.eye(3) * 9
    types = torch.tensor([0, 1, 1], device=dev)
    table = np.array([[2.0, 1.5], [1.5, 2.0]])
    ok = neighbor_list(pos, cell, True, 2.0, lib=lib, atom_types=types, cutoffs=table)
    assert ok.num_edges == 4  # (0-1 at 1.0 < 1.5 and 1-2 at 1.89 < 2.0 are listed, 0-2 at 1.6 > 1.5 is not)
    base = neighbor_list(pos, cell, True, 2.0, lib=lib)
    with pytest.raises(ValueError, match="cutoffs"):
        neighbor_list(pos, cell, True, 2.0, lib=lib, atom_types=types)
    with pytest.raises(ValueError, match="atom_types"):
        neighbor_list(pos, cell, True, 2.0, lib=lib, cutoffs=table)
    for bad in (np.ones((2, 3)), np.ones(4), np.ones((2, 2, 2))):
        with pytest.raises(ValueError, match="cutoffs"):
            neighbor_list(pos, cell, True, 2.0, lib=lib, atom_types=types, cutoffs=bad)
        with pytest.raises(ValueError, match="cutoffs"):
            base.prune(pos, types, bad)
    with pytest.raises(ValueError, match="atom_types"):
        neighbor_list(pos, cell, True, 2.0, lib=lib, atom_types=types[:2], cutoffs=table)
    with pytest.raises(ValueError, match="atom_types"):
        base.prune(pos, types.double(), table)
    for entry in (-1.0, 0.0, float("nan"), float("inf")):
        t = table.copy()
        t[1, 0] = entry
        with pytest.raises(AllegroError, match="cutoffs"):
            neighbor_list(pos, cell, True, 2.0, lib=lib, atom_types=types, cutoffs=t)
        with pytest.raises(AllegroError, match="cutoffs"):
            base.prune(pos, types, t)
    with pytest.raises(AllegroError, match="num_types"):
        neighbor_list(pos, cell, True, 2.0, lib=lib, atom_types=types, cutoffs=np.ones((65, 65)))
    with pytest.raises(AllegroError, match="num_types"):
        base.prune(pos, types, np.ones((65, 65)))
    big = neighbor_list(pos, cell, True, 2.0, lib=lib, atom_types=types + 62, cutoffs=np.full((64, 64), 1.2))  # T = 64: the cap itself
    assert big.num_edges == 2
    for off in (torch.tensor([0, 2, 1], device=dev), torch.tensor([0, -1, 1], device=dev), torch.tensor([0, 1 << 40, 1], device=dev)):
        for t in ((off,) if int(off.max()) > 2 ** 31 else (off, off.to(torch.int32))):
            with pytest.raises(AllegroError, match="atom_types"):
                neighbor_list(pos, cell, True, 2.0, lib=lib, atom_types=t, cutoffs=table)
            with pytest.raises(AllegroError, match="atom_types"):
                base.prune(pos, t, table)
    again = neighbor_list(pos, cell, True, 2.0, lib=lib, atom_types=types, cutoffs=table)  # (an error leaves nothing behind)
    assert_lists_equal(again, ok, "after the errors")


def test_cpu_tensors_are_refused_by_the_product_library():
    from allegro_amd._lib import AllegroError

    pos = torch.zeros((3, 3), dtype=torch.float64)
    with pytest.raises(AllegroError, match="GPU"):
        neighbor_list(pos, np.eye(3) * 5, True, 2.0, atom_types=torch.zeros(3, dtype=torch.int64), cutoffs=np.ones((1, 1)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cutoff_table_follows_the_state_dict(dtype):
    from tests.golden_utils import load_model_fixture
    from tests.hip_utils import model_from_fixture
    from allegro_amd.nn import HipAllegroModel

    fx = load_model_fixture("t_peredge", dtype)
    assert fx["cfg"]["per_edge_type_cutoff"] == {"H": 2.0, "C": {"H": 4.0, "C": 3.5, "O": 3.7}, "O": 3.9}
    want = torch.tensor(PEREDGE_TABLE, dtype=torch.float64)
    eps = 4 * torch.finfo(dtype).eps  # two roundings in `dtype`: 1 / r when the buffer is made, 1 / that here
    m = model_from_fixture(fx, dtype)
    t = m.cutoff_table()
    assert t.dtype == torch.float64 and t.device.type == "cpu" and tuple(t.shape) == (3, 3)
    assert float(((t - want).abs() / want).max()) <= eps
    # a model built WITHOUT the option, then given the fixture's state_dict: the table is the loaded one, not r_max everywhere
    cfg = {k: v for k, v in fx["cfg"].items() if k != "per_edge_type_cutoff"}
    cfg["model_dtype"] = {torch.float32: "float32", torch.float64: "float64"}[dtype]
    plain = HipAllegroModel(**cfg)
    assert torch.equal(plain.cutoff_table(), torch.full((3, 3), 4.0, dtype=torch.float64))
    plain.load_state_dict({"func." + k: v.to(dtype) if v.is_floating_point() else v for k, v in fx["sd"].items()})
    assert float(((plain.cutoff_table() - want).abs() / want).max()) <= eps
