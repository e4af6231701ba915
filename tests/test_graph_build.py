"""aa_graph_build_* / PreparedGraph.from_edge_index: the graph of ANY edge list (int64 / int32, any order, rows a stride apart),
optionally reduced to per-type-pair cutoffs, in one library operation.

Everything is compared exactly (`torch.equal`, integer equality).  Expected values never come from the code under test: the order is
numpy's `argsort(kind="stable")` of the center row restricted to the kept edges, the other fields follow from it in numpy, and the
existing routes -- `PreparedGraph(...)`, `DeviceNeighborList.prune(...).prepare(...)`, `aa_graph_transpose` behind both -- are
compared field for field.

The stable order is defined by INPUT edge ids.  Where a shuffled list is compared with the pruning of the center-sorted list it was
shuffled from (cases 4 and 6), the shuffle interleaves the center segments but keeps every segment's own order (`interleave`);
fully random orders are judged by numpy (cases 1 to 3).

`emu`: the unmodified kernels under the CPU emulation; `gpu`: the gfx950 library on the device.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd.nn import DeviceNeighborList, PreparedGraph, neighbor_list
from tests.test_neighbor_list_typed import BACKENDS, DTYPES, PEREDGE_TABLE, _backend, _close, _fixture_setup

FIELDS = ("center", "nbr", "rowptr", "types", "t_rowptr", "t_perm")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle(ei, N, keep=None):
    """numpy: the fields of the graph of `ei` [2, E] restricted to the edges `keep` (bool [E])."""
    c, j = np.asarray(ei[0], np.int64), np.asarray(ei[1], np.int64)
    ids = np.arange(c.size) if keep is None else np.nonzero(keep)[0]
    perm = ids[np.argsort(c[ids], kind="stable")]
    center, nbr = c[perm], j[perm]
    csr = lambda x: np.concatenate([[0], np.cumsum(np.bincount(x, minlength=N))])  # noqa: E731
    rowptr = csr(center)
    deg = np.diff(rowptr)
    nz = np.nonzero(deg)[0]
    hints = (int(nz[0]), int(nz[-1]) + 1, int(deg.max())) if nz.size else (0, 0, 0)
    return dict(perm=perm, center=center, nbr=nbr, rowptr=rowptr, t_rowptr=csr(nbr), t_perm=np.argsort(nbr, kind="stable"), hints=hints,
                sorted=bool(np.all(c[1:] >= c[:-1])))


def check(g, want, N, types, sv_in=None, E_in=None):
    """`g` (from_edge_index) against the numpy oracle `want`, field by field."""
    dev = g.rowptr.device
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)  # noqa: E731
    assert g.num_atoms == N and g.num_edges == want["perm"].size
    for f in ("center", "nbr", "rowptr", "t_rowptr", "t_perm"):
        got = getattr(g, f)
        assert got.dtype == torch.int32 and torch.equal(got, i32(want[f])), f
    assert g.types.dtype == torch.int32 and torch.equal(g.types, types.to(torch.int32))
    assert (g.atom_begin, g.atom_end, g.max_degree) == want["hints"]
    assert g.input_is_sorted == want["sorted"]
    unchanged = want["sorted"] and (E_in is None or want["perm"].size == E_in)
    if unchanged:
        assert g.perm is None
    else:
        assert g.perm.dtype == torch.int64 and torch.equal(g.perm, torch.tensor(want["perm"], device=dev))
    if sv_in is None:
        assert g.shift_vec is None
    else:
        assert g.shift_vec.dtype == sv_in.dtype and torch.equal(g.shift_vec, sv_in[torch.tensor(want["perm"], device=dev)])


def same_graph(a, b, what):
    for f in FIELDS + ("shift_vec",):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f"{what}: {f}"
        assert x is None or (x.dtype == y.dtype and torch.equal(x, y)), f"{what}: {f}"
    for f in ("num_atoms", "num_edges", "atom_begin", "atom_end", "max_degree"):
        assert getattr(a, f) == getattr(b, f), f"{what}: {f}"


def random_list(rng, N, max_deg, empty_ends=True):
    deg = rng.integers(0, max_deg + 1, N)
    if empty_ends and N > 4:
        deg[:2] = 0
        deg[-3:] = 0
    c = np.repeat(np.arange(N), deg)
    return np.stack([c, rng.integers(0, N, c.size)]).astype(np.int64)


def interleave(rng, center):
    """sh [E]: the shuffled list is list[:, sh]; center segments are interleaved at random, each keeps its own order."""
    slots = rng.permutation(center.size)
    new_pos = np.empty(center.size, np.int64)
    for a in np.unique(center):
        idx = np.nonzero(center == a)[0]
        new_pos[idx] = np.sort(slots[idx])
    return np.argsort(new_pos)


# ---------------------------------------------------------------------------------------------------------------------
# 0. the feature exists
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_attributes_exist():
    from allegro_amd.nn import HipAllegroModel
    import inspect

    from tests.hip_utils import emu_lib

    L = emu_lib().lib
    for name in ("aa_graph_build_workspace_bytes", "aa_graph_build_count", "aa_graph_build_fill"):
        assert hasattr(L, name), name
    assert hasattr(_lib, "EdgeList") and callable(PreparedGraph.from_edge_index)
    assert {"pos", "prune"} <= set(inspect.signature(HipAllegroModel.prepare_graph).parameters)
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "allegro_amd.h")).read()
    assert "aa_edge_list" in header and "aa_graph_build_fill" in header


# ---------------------------------------------------------------------------------------------------------------------
# 1. order and contents
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_shift", [False, True], ids=["ghost", "shift"])
@pytest.mark.parametrize("idx", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("order", ["sorted", "reversed", "permuted"])
def test_order_and_contents(order, idx, with_shift, dtype, backend):
    lib, dev = _backend(backend)
    rng = np.random.default_rng(7)
    N = 40
    base = random_list(rng, N, 20)
    E = base.shape[1]
    o = {"sorted": np.arange(E), "reversed": np.arange(E)[::-1].copy(), "permuted": rng.permutation(E)}[order]
    ei_np = base[:, o]
    types = torch.tensor(rng.integers(0, 3, N), device=dev)
    sv = torch.tensor(rng.normal(size=(E, 3)), dtype=dtype, device=dev) if with_shift else None
    want = oracle(ei_np, N)
    assert want["sorted"] == (order == "sorted") and want["hints"][0] == 2 and want["hints"][1] == N - 3
    ei = torch.tensor(ei_np, dtype=idx, device=dev)
    g = PreparedGraph.from_edge_index(ei, types, N, sv, lib=lib)
    check(g, want, N, types, sv)
    if order == "sorted":
        assert g.perm is None and g.input_is_sorted is True
    # the existing route (takes int64 indices)
    ref = PreparedGraph(ei.long(), types, N, sv, lib=lib)
    same_graph(g, ref, "PreparedGraph(...)")
    assert (g.perm is None) == (ref.perm is None) and (g.perm is None or torch.equal(g.perm, ref.perm))
    # rows a stride apart: a view of a wider tensor, read in place
    wide = torch.full((2, E + 13), -7, dtype=idx, device=dev)
    wide[:, 5:5 + E] = ei
    view = wide[:, 5:5 + E]
    assert view.stride(0) == E + 13 and not view.is_contiguous()
    same_graph(PreparedGraph.from_edge_index(view, types, N, sv, lib=lib), g, "strided view")
    # a column stride other than one is taken too (copied)
    same_graph(PreparedGraph.from_edge_index(ei.t().contiguous().t(), types, N, sv, lib=lib), g, "column-major")


# ---------------------------------------------------------------------------------------------------------------------
# 2. boundaries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("E", [0, 1, 255, 256, 257])
def test_edge_counts_at_the_launch_block(E, backend):
    lib, dev = _backend(backend)
    rng = np.random.default_rng(E)
    N = 23
    for shuffled in (False, True):
        c = np.sort(rng.integers(2, N - 2, E))
        ei_np = np.stack([c, rng.integers(0, N, E)]).astype(np.int64)
        if shuffled:
            ei_np = ei_np[:, rng.permutation(E)]
        types = torch.zeros(N, dtype=torch.int64, device=dev)
        g = PreparedGraph.from_edge_index(torch.tensor(ei_np, device=dev).reshape(2, E), types, N, lib=lib)
        check(g, oracle(ei_np, N), N, types)
        if E == 0:
            assert g.rowptr.tolist() == [0] * (N + 1) == g.t_rowptr.tolist() and (g.atom_begin, g.atom_end, g.max_degree) == (0, 0, 0)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("N", [1, 4095, 4096, 4097])
def test_atom_counts_at_the_scan_block(N, backend):
    lib, dev = _backend(backend)
    rng = np.random.default_rng(N)
    lo, hi = (0, 1) if N == 1 else (3, N - 5)  # atoms without edges at both ends
    ei_np = np.stack([rng.integers(lo, hi, 100), rng.integers(0, N, 100)]).astype(np.int64)
    types = torch.zeros(N, dtype=torch.int32, device=dev)
    want = oracle(ei_np, N)
    if N > 1:
        assert want["hints"][0] >= 3 and want["hints"][1] <= N - 5
    g = PreparedGraph.from_edge_index(torch.tensor(ei_np, device=dev), types, N, lib=lib)
    check(g, want, N, types)
    same_graph(g, PreparedGraph(torch.tensor(ei_np, device=dev), types, N, lib=lib), "PreparedGraph(...)")


@pytest.mark.parametrize("backend", BACKENDS)
def test_no_atoms(backend):
    lib, dev = _backend(backend)
    g = PreparedGraph.from_edge_index(torch.zeros((2, 0), dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), 0,
                                      lib=lib)
    assert g.rowptr.tolist() == [0] and g.t_rowptr.tolist() == [0] and g.num_edges == 0 and g.perm is None


@pytest.mark.parametrize("backend", BACKENDS)
def test_ghost_fixture(backend):
    """64 local + 822 ghost atoms, edges as the reference's transform emits them: not sorted by center."""
    lib, dev = _backend(backend)
    z = np.load(os.path.join(GOLDEN_DIR, "model_c2_ghost.npz"))
    ei_np, N = z["edge_index"].astype(np.int64), int(z["pos"].shape[0])
    assert N == 64 + 822 and not np.all(np.diff(ei_np[0]) >= 0)
    types = torch.tensor(z["types"], device=dev)
    ei = torch.tensor(ei_np, device=dev)
    g = PreparedGraph.from_edge_index(ei, types, N, lib=lib)
    want = oracle(ei_np, N)
    assert want["hints"][:2] == (0, 64)
    check(g, want, N, types)
    same_graph(g, PreparedGraph(ei, types, N, lib=lib), "PreparedGraph(...)")


# ---------------------------------------------------------------------------------------------------------------------
# 3. long groups
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_star_with_segments_and_groups_beyond_256(backend):
    """atom 0 <-> atoms 1..300 (center segment 0 and neighbour group 0 hold 300 + 100 entries: the serial branch of the ranking);
    atom 1 additionally -> 100 atoms and <- 100 atoms (a segment and a group in 65..256); edges shuffled.  Twice in one process:
    both results equal numpy, whatever order the atomics were served in."""
    lib, dev = _backend(backend)
    rng = np.random.default_rng(3)
    N = 301
    spokes = np.arange(1, N)
    extra = np.arange(2, 102)
    c = np.concatenate([np.zeros(300, np.int64), spokes, np.ones(100, np.int64), extra])
    j = np.concatenate([spokes, np.zeros(300, np.int64), extra, np.ones(100, np.int64)])
    ei_np = np.stack([c, j])[:, rng.permutation(c.size)]
    want = oracle(ei_np, N)
    deg, tdeg = np.diff(want["rowptr"]), np.diff(want["t_rowptr"])
    assert deg[0] > 256 and tdeg[0] > 256 and 64 < deg[1] <= 256 and 64 < tdeg[1] <= 256
    types = torch.zeros(N, dtype=torch.int64, device=dev)
    sv = torch.tensor(rng.normal(size=(c.size, 3)), dtype=torch.float32, device=dev)
    for _ in range(2):
        check(PreparedGraph.from_edge_index(torch.tensor(ei_np, device=dev), types, N, sv, lib=lib), want, N, types, sv)


# ---------------------------------------------------------------------------------------------------------------------
# 4. pruning
# ---------------------------------------------------------------------------------------------------------------------
def _molecule(dtype, lib, dev):
    """The geometry and table of the per-edge-cutoff fixtures: positions, types (3 species), the device list at 4 A."""
    from oracle import make_golden as MG

    g = MG.molecule_graph()
    pos = torch.tensor(g.pos, dtype=dtype, device=dev)
    types = torch.tensor(g.types, device=dev)
    assert len(set(g.types.tolist())) == 3
    return pos, types, neighbor_list(pos, g.cell, True, 4.0, lib=lib)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("idx", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_pruned_build_equals_prune_then_prepare(idx, dtype, backend):
    lib, dev = _backend(backend)
    pos, types, nl = _molecule(dtype, lib, dev)
    table = np.array(PEREDGE_TABLE)
    assert not np.allclose(table, table.T)
    pruned = nl.prune(pos, types, table)
    assert 0 < pruned.num_edges < nl.num_edges
    want = pruned.prepare(types)
    sh = torch.tensor(interleave(np.random.default_rng(5), nl.edge_index[0].cpu().numpy()), device=dev)
    ei_s, sv_s = nl.edge_index[:, sh].to(idx), nl.shift_vec[sh]
    assert not bool((ei_s[0, 1:] >= ei_s[0, :-1]).all())
    for t in (types, types.to(torch.int32)):
        g = PreparedGraph.from_edge_index(ei_s, t, pos.shape[0], sv_s, pos=pos, cutoffs=table, lib=lib)
        same_graph(g, want, "prune().prepare()")
        assert torch.equal(sh[g.perm], pruned.kept.long())  # perm composed with the shuffle = kept
    # the center-sorted list itself: sorted input, edges dropped -> perm is there and is `kept`
    g = PreparedGraph.from_edge_index(nl.edge_index.to(idx), types, pos.shape[0], nl.shift_vec, pos=pos, cutoffs=table, lib=lib)
    same_graph(g, want, "sorted input")
    assert g.input_is_sorted and torch.equal(g.perm, pruned.kept.long())
    # a fully random order: judged by numpy with the keep mask of the existing pruning
    rp = torch.tensor(np.random.default_rng(6).permutation(nl.num_edges), device=dev)
    keep = np.zeros(nl.num_edges, bool)
    keep[pruned.kept.cpu().numpy()] = True
    g = PreparedGraph.from_edge_index(nl.edge_index[:, rp].to(idx), types, pos.shape[0], nl.shift_vec[rp], pos=pos, cutoffs=table, lib=lib)
    ei_r = nl.edge_index[:, rp].cpu().numpy()
    check(g, oracle(ei_r, pos.shape[0], keep[rp.cpu().numpy()]), pos.shape[0], types, nl.shift_vec[rp], E_in=nl.num_edges)


@pytest.mark.parametrize("backend", BACKENDS)
def test_tables_beyond_and_below_every_edge(backend):
    lib, dev = _backend(backend)
    pos, types, nl = _molecule(torch.float64, lib, dev)
    N = pos.shape[0]
    sh = torch.tensor(np.random.default_rng(8).permutation(nl.num_edges), device=dev)
    ei_s, sv_s = nl.edge_index[:, sh].long(), nl.shift_vec[sh]
    plain = PreparedGraph.from_edge_index(ei_s, types, N, sv_s, lib=lib)
    big = PreparedGraph.from_edge_index(ei_s, types, N, sv_s, pos=pos, cutoffs=np.full((3, 3), 50.0), lib=lib)
    same_graph(big, plain, "a table beyond every edge")
    assert torch.equal(big.perm, plain.perm)
    none = PreparedGraph.from_edge_index(ei_s, types, N, sv_s, pos=pos, cutoffs=np.full((3, 3), 1e-3), lib=lib)
    assert none.num_edges == 0 and (none.atom_begin, none.atom_end, none.max_degree) == (0, 0, 0)
    assert none.rowptr.tolist() == [0] * (N + 1) == none.t_rowptr.tolist() and none.perm.numel() == 0
    assert tuple(none.shift_vec.shape) == (0, 3) and none.center.numel() == 0 == none.t_perm.numel()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_pruned_graph_gives_isolated_atom_energies(dtype, backend):
    lib, dev = _backend(backend)
    fx, m, data, g = _fixture_setup("t_peredge", dtype, lib, dev)
    pos, types, N = data["pos"], data["atom_types"], data["pos"].shape[0]
    sv = fx["shift_vec"].to(dtype).to(dev)  # (a periodic fixture)
    spread = pos * 100.0  # (every edge far beyond the model's cutoffs, shifts included)
    graph = m.prepare_graph(data["edge_index"], types, N, sv * 100.0, pos=spread, prune=True)
    assert graph.num_edges == 0
    e, f = (x.clone() for x in m.energy_forces(spread, graph))
    empty = PreparedGraph(torch.zeros((2, 0), dtype=torch.int64, device=dev), types, N, lib=lib)
    e0, f0 = m.energy_forces(spread, empty)
    assert torch.equal(e, e0) and torch.equal(f, f0) and not bool(f.any())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_exactly_at_its_cutoff_is_dropped(dtype, backend):
    """|r|^2 = 2.25 = 1.5^2 exactly (all values are dyadic): strict `<` drops it, with and without a shift; 1.25 stays."""
    lib, dev = _backend(backend)
    pos = torch.tensor([[0.0, 0, 0], [1.5, 0, 0], [0, 1.25, 0], [0.5, 0, 0]], dtype=dtype, device=dev)
    ei = torch.tensor([[0, 1, 0, 2, 0], [1, 0, 2, 0, 3]], device=dev)
    sv = torch.zeros((5, 3), dtype=dtype, device=dev)
    sv[4, 0] = 1.0  # 0 -> 3 through an image: 0.5 + 1.0 = 1.5
    types = torch.zeros(4, dtype=torch.int64, device=dev)
    g = PreparedGraph.from_edge_index(ei, types, 4, sv, pos=pos, cutoffs=[[1.5]], lib=lib)
    assert g.perm.tolist() == [2, 3] and g.center.tolist() == [0, 2] and g.nbr.tolist() == [2, 0]
    g = PreparedGraph.from_edge_index(ei[:, :4], types, 4, pos=pos, cutoffs=[[1.5]], lib=lib)
    assert g.perm.tolist() == [2, 3] and g.shift_vec is None
    g = PreparedGraph.from_edge_index(ei, types, 4, sv, pos=pos, cutoffs=[[1.5000001]], lib=lib)
    assert g.num_edges == 5 and g.perm.tolist() == [0, 2, 4, 1, 3]


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------------------------------------------------
def _raw(lib, dev, ei, N, guard=4, ws_bytes=None):
    """aa_graph_build_count / _fill through ctypes on outputs with `guard` extra elements filled with -99."""
    E = ei.shape[1]
    inp = _lib.EdgeList(N, E, ei.data_ptr(), ei.stride(0), int(ei.dtype == torch.int64), _lib.AA_F32, None, None)
    nbytes = lib.lib.aa_graph_build_workspace_bytes(N, E)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mk = lambda n: torch.full((n + guard,), -99, dtype=torch.int32, device=dev)  # noqa: E731
    out = dict(rowptr=mk(N + 1), center=mk(E), nbr=mk(E), perm=mk(E), t_rowptr=mk(N + 1), t_perm=mk(E))
    n_edges, hints, was_sorted = C.c_int64(-1), (C.c_int32 * 3)(), C.c_int32(-1)
    rc = lib.lib.aa_graph_build_count(C.byref(inp), None, ws.data_ptr(), nbytes if ws_bytes is None else ws_bytes, out["rowptr"].data_ptr(),
                                      C.byref(n_edges), hints, C.byref(was_sorted), 0)
    msg = lib.lib.aa_last_error().decode() if rc else ""
    rc2 = lib.lib.aa_graph_build_fill(C.byref(inp), None, ws.data_ptr(), nbytes if ws_bytes is None else ws_bytes, out["rowptr"].data_ptr(),
                                      out["center"].data_ptr(), out["nbr"].data_ptr(), out["perm"].data_ptr(), None, out["t_rowptr"].data_ptr(),
                                      out["t_perm"].data_ptr(), 0)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return rc, msg, rc2, out, int(n_edges.value), list(hints), int(was_sorted.value)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("idx", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_indices_out_of_range_are_refused_in_bounds(idx, backend):
    lib, dev = _backend(backend)
    N = 6
    good = torch.tensor([[3, 0, 5, 1], [1, 2, 0, 4]], dtype=idx, device=dev)
    rc, msg, rc2, out, E2, hints, was_sorted = _raw(lib, dev, good, N)
    assert (rc, rc2, E2, hints, was_sorted) == (0, 0, 4, [0, 6, 1], 0)
    assert out["center"].tolist() == [0, 1, 3, 5, -99, -99, -99, -99] and out["perm"].tolist()[:4] == [1, 3, 0, 2]
    assert all(t.tolist()[-4:] == [-99] * 4 for t in out.values())
    for row, col, value, word in ((0, 2, N, "centers"), (1, 1, -1, "neighbours"), (0, 0, -3, "centers"), (1, 3, N + 100, "neighbours")):
        bad = good.clone()
        bad[row, col] = value
        rc, msg, rc2, out, _, _, _ = _raw(lib, dev, bad, N)
        assert rc == -1 and f"row {row}" in msg and word in msg and f"edge {col}" in msg, msg
        # a fill issued regardless writes no edge output; nothing beyond any extent
        for k in ("center", "nbr", "perm", "t_perm"):
            assert out[k].tolist() == [-99] * (4 + 4), k
        assert all(t.tolist()[-4:] == [-99] * 4 for t in out.values())
        with pytest.raises(_lib.AllegroError, match=f"row {row}"):
            PreparedGraph.from_edge_index(bad, torch.zeros(N, dtype=torch.int64, device=dev), N, lib=lib)
    after = PreparedGraph.from_edge_index(good, torch.zeros(N, dtype=torch.int64, device=dev), N, lib=lib)  # (an error leaves nothing behind)
    assert after.center.tolist() == [0, 1, 3, 5]


@pytest.mark.parametrize("backend", BACKENDS)
def test_argument_errors(backend):
    lib, dev = _backend(backend)
    N = 6
    ei = torch.tensor([[3, 0, 5, 1], [1, 2, 0, 4]], device=dev)
    types = torch.zeros(N, dtype=torch.int64, device=dev)
    pos = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    rc, msg, rc2, out, *_ = _raw(lib, dev, ei, N, ws_bytes=lib.lib.aa_graph_build_workspace_bytes(N, 4) - 1)
    assert rc == -2 and rc2 == -2 and "workspace" in msg  # AA_ERR_WORKSPACE
    assert all(t.tolist() == [-99] * t.numel() for t in out.values())
    with pytest.raises(ValueError, match="pos"):
        PreparedGraph.from_edge_index(ei, types, N, cutoffs=np.ones((1, 1)), lib=lib)
    # the checks on `types` are those of aa_graph_prune_count
    with pytest.raises(_lib.AllegroError, match="atom_types"):
        PreparedGraph.from_edge_index(ei, types + 1, N, pos=pos, cutoffs=np.ones((1, 1)), lib=lib)
    with pytest.raises(_lib.AllegroError, match="atom_types"):
        PreparedGraph.from_edge_index(ei, (types - 1).to(torch.int32), N, pos=pos, cutoffs=np.ones((2, 2)), lib=lib)
    with pytest.raises(_lib.AllegroError, match="cutoffs"):
        PreparedGraph.from_edge_index(ei, types, N, pos=pos, cutoffs=np.array([[-1.0]]), lib=lib)
    with pytest.raises(_lib.AllegroError, match="num_types"):
        PreparedGraph.from_edge_index(ei, types, N, pos=pos, cutoffs=np.ones((65, 65)), lib=lib)
    with pytest.raises(ValueError, match="cutoffs"):
        PreparedGraph.from_edge_index(ei, types, N, pos=pos, cutoffs=np.ones((2, 3)), lib=lib)
    with pytest.raises(ValueError, match="edge_index"):
        PreparedGraph.from_edge_index(ei.double(), types, N, lib=lib)
    # sizes at or above 2^31 are refused before anything is touched
    inp = _lib.EdgeList(1 << 31, 4, ei.data_ptr(), 4, 1, _lib.AA_F32, None, None)
    one = torch.zeros(64, dtype=torch.int32, device=dev)
    assert lib.lib.aa_graph_build_count(C.byref(inp), None, one.data_ptr(), 256, one.data_ptr(), C.byref(C.c_int64()), None, None, 0) == -1
    inp = _lib.EdgeList(N, 1 << 31, ei.data_ptr(), 1 << 31, 1, _lib.AA_F32, None, None)
    assert lib.lib.aa_graph_build_count(C.byref(inp), None, one.data_ptr(), 256, one.data_ptr(), C.byref(C.c_int64()), None, None, 0) == -1


def test_cpu_tensors_are_refused_by_the_product_library():
    with pytest.raises(_lib.AllegroError, match="GPU"):
        PreparedGraph.from_edge_index(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(3, dtype=torch.int64), 3)


# ---------------------------------------------------------------------------------------------------------------------
# 6. model level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["t_peredge", "t_spline_peredge"])
def test_model_on_pruned_build(name, dtype, backend):
    """prepare_graph(shuffled list, pos=, prune=True): the step meets the fixtures' reference outputs (computed on the FULL list; the
    dropped edges are exact zeros) at the tolerances of the typed list, and is bit-identical to the step on the prune().prepare() graph."""
    lib, dev = _backend(backend)
    fx, m, data, g = _fixture_setup(name, dtype, lib, dev)
    pos, types, N = data["pos"], data["atom_types"], data["pos"].shape[0]
    sv = fx["shift_vec"].to(dtype).to(dev)
    full = PreparedGraph(data["edge_index"], types, N, sv, lib=lib)
    assert full.perm is None
    base = DeviceNeighborList(torch.stack([full.center, full.nbr]), full.rowptr, None, full.shift_vec, lib)
    want_graph = base.prune(pos, types, m.cutoff_table()).prepare(types)
    assert 0 < want_graph.num_edges < full.num_edges
    sh = torch.tensor(interleave(np.random.default_rng(11), full.center.cpu().numpy()), device=dev)
    graph = m.prepare_graph(data["edge_index"][:, sh], types, N, sv[sh], pos=pos, prune=True)
    same_graph(graph, want_graph, "prune().prepare()")
    out = {}
    for tag, gr in (("want", want_graph), ("got", graph)):
        e, f = m.energy_forces(pos, gr)
        out[tag] = dict(e=e.clone(), f=f.clone(), w=m.virial(gr).clone(), aw=m.atom_virial(gr, "split").clone())
    ref = fx["out"]
    _close(f"{name} E_i", out["got"]["e"], ref["atomic_energy"].reshape(-1), dtype)
    _close(f"{name} F", out["got"]["f"], ref["forces"], dtype)
    for k in ("e", "f", "w", "aw"):
        assert torch.equal(out["got"][k], out["want"][k]), k
    # without pruning, pos only selects the route: the graph of PreparedGraph(...)
    same_graph(m.prepare_graph(data["edge_index"], types, N, sv, pos=pos), full, "pos, prune=False")
    with pytest.raises(ValueError, match="pos"):
        m.prepare_graph(data["edge_index"], types, N, sv, prune=True)
