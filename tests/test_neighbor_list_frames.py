"""The neighbour list of a batch of frames in one pair of calls (`aa_nl_frames_count` / `aa_nl_frames_fill`,
`neighbor_list_frames`): every frame in its own cell, global atom ids, `shift_vec` from each edge's own cell.

The batch is the one of tests/test_frames.py (two 64-atom silicon frames, one of them triclinic, an empty frame, a lone atom, two
atoms in a 3.6 A cell that needs k = 2 images).  Reference: the brute-force image enumeration of tests/test_neighbor_list.py, frame
by frame, ids offset.  Documented order inside a centre's segment: image (n0, n1, n2) of the WRAPPED positions ascending, then
neighbour id ascending, where cell_shift = n + wrap[nbr] - wrap[center] and wrap = -floor(fractional coordinate) along periodic
directions.

`emu`: the unmodified kernels under the CPU emulation; `gpu`: the gfx950 library on the device.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd.nn import _TORCH2AA, Frames, neighbor_list, neighbor_list_frames
from tests.golden_utils import load_model_fixture
from tests.hip_utils import model_from_fixture
from tests.test_atom_virial import BACKENDS, DTYPES, _backend, assert_close
from tests.test_frames import NUM_FRAMES, batch
from tests.test_neighbor_list import as_set, brute_force


def build(backend, dtype, pos=None, cells=None, pbc=(1, 1, 1), offsets=None):
    lib, dev = _backend(backend)
    b = batch()
    p = torch.tensor(b["pos"] if pos is None else pos, dtype=dtype, device=dev)
    frames = Frames(torch.tensor(b["offsets"] if offsets is None else offsets), device=dev)
    cells_t = torch.tensor(b["cells"] if cells is None else cells, dtype=torch.float64, device=dev)
    return neighbor_list_frames(p, cells_t, pbc, b["r_max"], frames, lib=lib), p


def expected(pos, cells, pbc, offsets, r_cut):
    """Union of the per-frame brute-force sets with global ids; `pos` as the kernel sees it (rounded to its dtype), in double."""
    want = set()
    for f in range(len(offsets) - 1):
        lo, hi = int(offsets[f]), int(offsets[f + 1])
        want |= {(i + lo, j + lo, s0, s1, s2) for i, j, s0, s1, s2 in brute_force(pos[lo:hi], cells[f], pbc, r_cut)}
    return want


def wraps(pos, cells, pbc, offsets):
    """[N,3] -floor(fractional coordinate) along periodic directions."""
    w = np.zeros((len(pos), 3), dtype=np.int64)
    for f in range(len(offsets) - 1):
        lo, hi = int(offsets[f]), int(offsets[f + 1])
        w[lo:hi] = -np.floor(pos[lo:hi] @ np.linalg.inv(cells[f])).astype(np.int64) * np.array(pbc)
    return w


def check_structure(nl, pos, cells, pbc, offsets, dtype):
    """rowptr consistent, centres sorted, the documented order inside every segment, shift_vec from the edge's own cell."""
    n = len(pos)
    ei, cs = nl.edge_index.cpu().long().numpy(), nl.cell_shift.cpu().long().numpy()
    rp = nl.rowptr.cpu().long().numpy()
    assert rp[0] == 0 and rp[-1] == ei.shape[1] and (np.diff(rp) == np.bincount(ei[0], minlength=n)).all()
    assert (np.diff(ei[0]) >= 0).all()
    w = wraps(pos, cells, pbc, offsets)
    image = cs - w[ei[1]] + w[ei[0]]
    keys = [tuple(image[e]) + (int(ei[1, e]),) for e in range(ei.shape[1])]
    for a in range(n):
        seg = keys[rp[a]: rp[a + 1]]
        assert seg == sorted(seg), f"segment of atom {a}"
    frame_of = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    assert (frame_of[ei[0]] == frame_of[ei[1]]).all()  # every neighbour lies in its centre's frame
    sv = np.einsum("ei,eij->ej", cs.astype(np.float64), cells[frame_of[ei[0]]])
    err = float(np.abs(nl.shift_vec.cpu().double().numpy() - sv).max())
    assert err <= (1e-6 if dtype == torch.float32 else 1e-12) * max(1.0, float(np.abs(sv).max()))


# ---------------------------------------------------------------------------------------------------------------------
# 7. against brute_force
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pbc", [(1, 1, 1), (1, 1, 0)], ids=["periodic", "slab"])
def test_matches_brute_force(backend, dtype, pbc):
    b = batch()
    nl, p = build(backend, dtype, pbc=pbc)
    got = as_set(nl)
    assert len(got) == len(set(got)), "duplicate edges"
    seen = p.double().cpu().numpy()
    want = expected(seen, b["cells"], pbc, b["offsets"], b["r_max"])
    assert set(got) == want, (len(got), len(want))
    if pbc == (1, 1, 1) and dtype == torch.float64:
        assert want == {tuple(int(x) for x in (*b["edge_index"][:, e], *b["cell_shift"][e])) for e in range(b["edge_index"].shape[1])}
        assert np.abs(nl.cell_shift.cpu().numpy()).max() == 2  # (the 3.6 A frame: second images)
    check_structure(nl, seen, b["cells"], pbc, b["offsets"], dtype)
    again, _ = build(backend, dtype, pbc=pbc)
    for x, y in ((nl.edge_index, again.edge_index), (nl.rowptr, again.rowptr), (nl.cell_shift, again.cell_shift), (nl.shift_vec, again.shift_vec)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_frame_equals_the_cell_list(backend, dtype):
    lib, dev = _backend(backend)
    b = batch()
    for f in (1, 4):  # the triclinic frame, and the frame smaller than the cutoff
        pos, cell = b["geo"][f]
        p = torch.tensor(pos, dtype=dtype, device=dev)
        one = neighbor_list_frames(p, torch.tensor(cell).reshape(1, 3, 3), True, b["r_max"], Frames(torch.tensor([0, len(pos)]), device=dev), lib=lib)
        ref = neighbor_list(p, cell, True, b["r_max"], lib=lib)
        assert one.num_edges == ref.num_edges and set(as_set(one)) == set(as_set(ref))
        assert torch.equal(one.rowptr, ref.rowptr)


@pytest.mark.parametrize("backend", BACKENDS)
def test_atoms_outside_their_cell_and_a_translated_frame(backend):
    """Atoms moved by whole lattice vectors, and frame 1 translated by 1 000 A: the same pairs at the same distances, cell_shift
    absorbs the move (fp64 positions: at 1 000 A an fp32 position is a different geometry)."""
    b = batch()
    dtype = torch.float64
    base, _ = build(backend, dtype)
    pos = b["pos"].copy()
    rng = np.random.default_rng(5)
    moved = np.zeros((len(pos), 3), dtype=np.int64)
    for f in (0, 1, 4):
        lo, hi = int(b["offsets"][f]), int(b["offsets"][f + 1])
        moved[lo:hi] = rng.integers(-2, 3, size=(hi - lo, 3))
        pos[lo:hi] += moved[lo:hi] @ b["cells"][f]
    nl, p = build(backend, dtype, pos=pos)
    # r_e = pos[j] - pos[i] + S @ cell is unchanged, so S' = S - moved[j] + moved[i]
    ei = base.edge_index.cpu().long().numpy()
    want = {(int(ei[0, e]), int(ei[1, e])) + tuple(int(x) for x in base.cell_shift.cpu().numpy()[e] - moved[ei[1, e]] + moved[ei[0, e]])
            for e in range(ei.shape[1])}
    assert set(as_set(nl)) == want and nl.num_edges == base.num_edges
    assert set(as_set(nl)) == expected(pos, b["cells"], (1, 1, 1), b["offsets"], b["r_max"])
    check_structure(nl, pos, b["cells"], (1, 1, 1), b["offsets"], dtype)
    far = b["pos"].copy()
    lo, hi = int(b["offsets"][1]), int(b["offsets"][2])
    far[lo:hi] += np.array([1000.0, -1000.0, 1000.0])
    nl2, _ = build(backend, dtype, pos=far)
    assert set(as_set(nl2)) == expected(far, b["cells"], (1, 1, 1), b["offsets"], b["r_max"])
    assert nl2.num_edges == base.num_edges and torch.equal(nl2.rowptr, base.rowptr)
    pairs = lambda x: sorted(zip(*x.edge_index.cpu().tolist()))  # noqa: E731
    assert pairs(nl2) == pairs(base)
    r = lambda x, q: (q[x.edge_index[1].long()] - q[x.edge_index[0].long()] + x.shift_vec).norm(dim=1).sort().values  # noqa: E731
    dev = base.edge_index.device
    assert float((r(nl2, torch.tensor(far, device=dev)) - r(base, torch.tensor(b["pos"], device=dev))).abs().max()) < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    lib, dev = _backend(backend)
    b = batch()
    dtype = torch.float64
    singular = b["cells"].copy()
    singular[1, 2] = singular[1, 0] * 2.0  # frame 1: two parallel lattice vectors
    with pytest.raises(_lib.AllegroError, match=r"\(-1\).*frame 1: singular cell"):
        build(backend, dtype, cells=singular)
    tiny = b["cells"].copy()
    tiny[4] = np.eye(3) * 0.05  # frame 4: 100 images along every direction
    with pytest.raises(_lib.AllegroError, match=r"\(-1\).*frame 4: .*more than 64 images"):
        build(backend, dtype, cells=tiny)
    both = singular.copy()
    both[4] = tiny[4]
    with pytest.raises(_lib.AllegroError, match="frame 1: singular cell"):  # (the first such frame)
        build(backend, dtype, cells=both)
    beyond = b["offsets"].copy()
    beyond[-1] += 3
    with pytest.raises(_lib.AllegroError, match="frame 4: frame_atoms"):
        build(backend, dtype, offsets=beyond)
    # fill after a failed count writes nothing (C ABI, poisoned outputs)
    n = len(b["pos"])
    pos = torch.tensor(b["pos"], dtype=dtype, device=dev)
    cells = torch.tensor(singular, dtype=torch.float64, device=dev)
    frames = Frames(torch.tensor(b["offsets"]), device=dev)
    inp = _lib.NlFramesInput()
    inp.num_atoms, inp.pos, inp.cells, inp.dtype, inp.r_cut = n, pos.data_ptr(), cells.data_ptr(), _TORCH2AA[dtype], b["r_max"]
    for q in range(3):
        inp.pbc[q] = 1
    fs = frames.c_struct()
    L = lib.lib
    nbytes = L.aa_nl_frames_workspace_bytes(n, NUM_FRAMES)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    good, _ = build(backend, dtype)
    rowptr = good.rowptr.clone()  # (row pointers that WOULD send every edge somewhere)
    count_rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    n_edges = C.c_int64(-7)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    assert L.aa_nl_frames_count(C.byref(inp), C.byref(fs), ws.data_ptr(), nbytes, count_rowptr.data_ptr(), C.byref(n_edges), stream) == -1
    assert n_edges.value == -7 and b"frame 1: singular cell" in L.aa_last_error()
    E = good.num_edges
    center, nbr = (torch.full((E,), -5, dtype=torch.int32, device=dev) for _ in range(2))
    cell_shift = torch.full((E, 3), -5, dtype=torch.int32, device=dev)
    shift_vec = torch.full((E, 3), 7.0, dtype=dtype, device=dev)
    assert L.aa_nl_frames_fill(C.byref(inp), C.byref(fs), ws.data_ptr(), nbytes, rowptr.data_ptr(), center.data_ptr(), nbr.data_ptr(),
                               cell_shift.data_ptr(), shift_vec.data_ptr(), stream) == 0
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    assert bool((center == -5).all()) and bool((nbr == -5).all()) and bool((cell_shift == -5).all()) and bool((shift_vec == 7.0).all())
    # no frames, no atoms
    none = neighbor_list_frames(torch.zeros((0, 3), dtype=dtype, device=dev), torch.zeros((0, 3, 3)), True, 2.0, Frames(torch.tensor([0]), device=dev), lib=lib)
    assert none.num_edges == 0 and none.rowptr.tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------------
# 9. end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_list_prepare_step_meets_the_fixture(backend, dtype):
    lib, dev = _backend(backend)
    b = batch()
    fx = load_model_fixture("c2", dtype)
    m = model_from_fixture(fx, dtype, lib, dev)
    nl, pos = build(backend, dtype)
    g = nl.prepare(torch.zeros(len(b["pos"]), dtype=torch.long, device=dev))
    e, f = m.energy_forces(pos, g)
    assert_close("frame 0: atomic energies against the fixture", e[:64].cpu(), fx["out"]["atomic_energy"].reshape(-1).double(), dtype)
    assert_close("frame 0: forces against the fixture", f[:64].cpu(), fx["out"]["forces"].double(), dtype)
    frames = Frames(torch.tensor(b["offsets"]), device=dev)
    assert_close("frame energies", m.frame_energies(e, frames)[0].cpu(), fx["out"]["atomic_energy"].double().sum(), dtype)
    assert float(m.frame_virial(g, frames)[4].abs().max()) > 1e-3


def test_symbols_are_declared_and_exported():
    import os

    from allegro_amd.build import build_library

    lib_path = build_library(verbose=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "allegro_amd.h")).read()
    cdll = C.CDLL(lib_path)
    for name in ("aa_nl_frames_workspace_bytes", "aa_nl_frames_count", "aa_nl_frames_fill"):
        assert f" {name}(" in src and hasattr(cdll, name), name
