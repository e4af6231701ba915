"""Batches of frames: per-frame energy, virial and heat flux of ONE step on the concatenated graph (`aa_frames`,
`aa_model_frame_energies` / `_frame_virial` / `_frame_heat_flux` and the blocked twins; `Frames`, `HipAllegroModel.frame_*`, and
`forward(data)` with a non-decreasing `batch`).

The batch: the `c2` fixture's model (one species, r_max from its config) on five frames, in this order:
  0  the fixture's 64-atom frame: 1 792 edges, so every lane of the frame's workgroup strides seven times
  1  a copy perturbed by 0.02 A and strained into a triclinic cell (as tests/test_forward_dict.py does)
  2  an empty frame
  3  one atom alone in a 30 A box: no edges
  4  two atoms in a cubic cell of 3.6 A: k = 2 images along every direction, edges with |cell_shift| = 2 and self-image edges.
     Degrees found on the CPU: 18 and 18 (6 self images + 12 images of the other atom each), so the largest degree of the batch
     stays the 28 of the silicon frames (<= 32) and the batch keeps the default forward.
Edge lists are the brute-force image enumeration of tests/test_neighbor_list.py, per frame.

References: every frame stepped alone (`e_atom.sum()`, `virial`, `heat_flux_potential`); the fp64 sums of exactly the kernel's
products from the `dvec` / `vec` taps with the derived bound of tests/test_heat_flux.py at the frame's own edge count; the fixture's
recorded outputs.  Tolerances are the project's: 1e-9 (fp64) / 5e-5 (fp32) times max(1, max |expected|).

`emu`: the unmodified kernels under the CPU emulation; `gpu`: the gfx950 library on the device.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd import graph as G
from allegro_amd.nn import Frames, PreparedGraph
from tests.golden_utils import load_model_fixture
from tests.hip_utils import model_from_fixture
from tests.test_atom_virial import BACKENDS, DTYPES, _backend, assert_close
from tests.test_heat_flux import assert_derived, velocities
from tests.test_neighbor_list import brute_force

NUM_FRAMES = 5
SMALL_CELL = 3.6


# ---------------------------------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------------------------------
_BATCH = None


def frame_geometries():
    """[(pos [n,3], cell [3,3])] of the five frames, float64."""
    si = G.make_si_graph(2)  # the geometry of the c2 fixture
    rng = np.random.default_rng(9)
    pos1 = (si.pos + rng.normal(0, 0.02, si.pos.shape)) * 1.015
    cell1 = si.cell * 1.015 + np.array([[0, 0.05, 0], [0, 0, 0], [0.02, 0, 0]])
    return [(si.pos, si.cell), (pos1, cell1), (np.zeros((0, 3)), np.eye(3) * 10.0), (np.array([[15.0, 14.0, 16.0]]), np.eye(3) * 30.0),
            (np.array([[0.3, 0.5, 0.4], [3.0, 0.7, 0.7]]), np.eye(3) * SMALL_CELL)]


def frame_list(pos, cell, r_cut, pbc=(1, 1, 1)):
    """(edge_index [2,E], cell_shift [E,3]) of one frame, sorted by (center, neighbor, shift)."""
    edges = sorted(brute_force(pos, cell, pbc, r_cut))
    a = np.array(edges, dtype=np.int64).reshape(-1, 5)
    return a[:, :2].T.copy(), a[:, 2:].copy()


def batch():
    """The five frames concatenated: pos, cells [5,3,3], offsets [6], batch vector, edge_index (global ids), cell_shift, shift_vec, and
    the per-frame pieces."""
    global _BATCH
    if _BATCH is None:
        fx = load_model_fixture("c2", torch.float64)
        r_max = float(fx["cfg"]["r_max"])
        geo = frame_geometries()
        assert np.allclose(geo[0][0], fx["pos"].numpy())
        offsets = np.concatenate([[0], np.cumsum([len(p) for p, _ in geo])])
        lists = [frame_list(p, c, r_max) for p, c in geo]
        counts = [ei.shape[1] for ei, _ in lists]
        assert counts[0] == fx["edge_index"].shape[1] == 1792 and counts[2] == 0 and counts[3] == 0
        deg4 = np.bincount(lists[4][0][0], minlength=2)
        assert deg4.tolist() == [18, 18], deg4                      # (the degrees the docstring states)
        assert np.abs(lists[4][1]).max() == 2                         # k = 2 images are needed
        assert (lists[4][0][0] == lists[4][0][1]).any()               # self-image edges
        assert max(int(np.bincount(ei[0]).max()) for ei, _ in lists if ei.shape[1]) <= 32
        _BATCH = dict(
            r_max=r_max, geo=geo, offsets=offsets, lists=lists, counts=counts,
            pos=np.concatenate([p for p, _ in geo]), cells=np.stack([c for _, c in geo]),
            batch=np.repeat(np.arange(NUM_FRAMES), np.diff(offsets)),
            edge_index=np.concatenate([ei + offsets[b] for b, (ei, _) in enumerate(lists)], axis=1),
            cell_shift=np.concatenate([cs for _, cs in lists]),
            shift_vec=np.concatenate([cs @ geo[b][1] for b, (_, cs) in enumerate(lists)]))
    return _BATCH


_STEPPED = {}


def stepped(backend, dtype):
    """One model, one force step on the batch and the three per-frame calls (shared: the tests below only read it, or step again on
    the same inputs)."""
    if (backend, dtype) not in _STEPPED:
        lib, dev = _backend(backend)
        b = batch()
        m = model_from_fixture(load_model_fixture("c2", dtype), dtype, lib, dev)
        n = len(b["pos"])
        pos = torch.tensor(b["pos"], dtype=dtype, device=dev)
        types = torch.zeros(n, dtype=torch.long, device=dev)
        vel = velocities(n, dtype, dev)
        g = PreparedGraph(torch.tensor(b["edge_index"], device=dev), types, n, torch.tensor(b["shift_vec"], dtype=dtype, device=dev), lib=lib)
        assert g.perm is None  # (the list is center-sorted already: edge e of the graph is edge e of the batch)
        frames = Frames(torch.tensor(b["offsets"]), device=dev)
        e_atom, forces = m.energy_forces(pos, g)
        rows = (m.frame_energies(e_atom, frames), m.frame_virial(g, frames), m.frame_heat_flux_potential(g, frames, vel))
        _STEPPED[(backend, dtype)] = dict(m=m, g=g, pos=pos, vel=vel, frames=frames, e_atom=e_atom, forces=forces, rows=rows, lib=lib, dev=dev)
    return _STEPPED[(backend, dtype)]


def stepped_alone(s, dtype):
    """Every non-empty frame stepped alone, on a model of its own: [(sum of e_atom, virial, heat flux) | None], fp64 on the host."""
    b, lib, dev = batch(), s["lib"], s["dev"]
    m = model_from_fixture(load_model_fixture("c2", dtype), dtype, lib, dev)
    alone = []
    for f, ((p, c), (ei, cs)) in enumerate(zip(b["geo"], b["lists"])):
        if len(p) == 0:
            alone.append(None)
            continue
        types = torch.zeros(len(p), dtype=torch.long, device=dev)
        gf = PreparedGraph(torch.tensor(ei, device=dev), types, len(p), torch.tensor(cs @ c, dtype=dtype, device=dev), lib=lib)
        e, _ = m.energy_forces(torch.tensor(p, dtype=dtype, device=dev), gf)
        lo = int(b["offsets"][f])
        alone.append((e.double().sum().cpu(), m.virial(gf).double().cpu(), m.heat_flux_potential(gf, s["vel"][lo: lo + len(p)]).double().cpu()))
    return alone


def unblocked(s):
    """`s` with the unblocked batch step in the model's workspace (the blocked test leaves its own there)."""
    if s["m"]._blocked is not None:
        s["m"].energy_forces(s["pos"], s["g"])
    return s


# ---------------------------------------------------------------------------------------------------------------------
# 1. against single frames
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_equal_the_frames_stepped_alone(backend, dtype):
    s = unblocked(stepped(backend, dtype))
    alone = stepped_alone(s, dtype)
    fe, fw, fj = s["rows"]
    assert fe.shape == (NUM_FRAMES,) and fw.shape == (NUM_FRAMES, 3, 3) and fj.shape == (NUM_FRAMES, 3)
    assert fe.dtype == fw.dtype == fj.dtype == dtype
    for f, ref in enumerate(alone):
        if ref is None:
            continue
        e, w, j = ref
        assert_close(f"frame {f}: energy", fe[f].cpu(), e, dtype)
        assert_close(f"frame {f}: virial", fw[f].cpu(), w, dtype)
        assert_close(f"frame {f}: heat flux", fj[f].cpu(), j, dtype)
    assert float(alone[0][1].abs().max()) > 1e-3 and float(alone[4][1].abs().max()) > 1e-3
    assert_close("frame rows summed: virial of the batch", fw.double().sum(0).cpu(), s["m"].virial(s["g"]).double().cpu(), dtype)
    assert_close("frame rows summed: heat flux of the batch", fj.double().sum(0).cpu(),
                 s["m"].heat_flux_potential(s["g"], s["vel"]).double().cpu(), dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the taps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_match_the_taps(backend, dtype):
    """The fp64 sums of exactly the kernel's products -- g_a * (u_b * r), u_b * r * (g . v_j), E_n -- frame by frame, with the
    derived bound at the frame's own element count."""
    s = unblocked(stepped(backend, dtype))
    m, g, b = s["m"], s["g"], batch()
    fe, fw, fj = m.frame_energies(s["e_atom"], s["frames"]), m.frame_virial(g, s["frames"]), m.frame_heat_flux_potential(g, s["frames"], s["vel"])
    d = m.debug_tap("dvec", g, with_forces=True)[:, :3].double().cpu()
    v = m.debug_tap("vec", g, with_forces=True).double().cpu()
    r = v[:, :3] * v[:, 3:4]
    p = d * s["vel"].double().cpu()[g.nbr.long().cpu()]
    e_atom = s["e_atom"].double().cpu()
    edge_off = np.concatenate([[0], np.cumsum(b["counts"])])
    for f in range(NUM_FRAMES):
        lo, hi, a0, a1 = int(edge_off[f]), int(edge_off[f + 1]), int(b["offsets"][f]), int(b["offsets"][f + 1])
        outer = d[lo:hi].unsqueeze(2) * r[lo:hi].unsqueeze(1)
        assert_derived(f"frame {f}: virial", fw[f].reshape(9).cpu(), outer.sum(0).reshape(9), outer.abs().sum(0).reshape(9), hi - lo, dtype)
        want = -(r[lo:hi] * p[lo:hi].sum(-1, keepdim=True)).sum(0)
        assert_derived(f"frame {f}: heat flux", fj[f].cpu(), want, (r[lo:hi].abs() * p[lo:hi].abs().sum(-1, keepdim=True)).sum(0), hi - lo, dtype)
        assert_derived(f"frame {f}: energy", fe[f].reshape(1).cpu(), e_atom[a0:a1].sum().reshape(1), e_atom[a0:a1].abs().sum().reshape(1),
                       a1 - a0, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bits(backend, dtype):
    s = unblocked(stepped(backend, dtype))
    m, g, b = s["m"], s["g"], batch()
    call = lambda fr: (m.frame_energies(s["e_atom"], fr).clone(), m.frame_virial(g, fr).clone(),  # noqa: E731
                       m.frame_heat_flux_potential(g, fr, s["vel"]).clone())
    first, second = call(s["frames"]), call(s["frames"])
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    for f in (1, 4):  # a descriptor that holds this frame only returns the bits of its row of the full call
        one = Frames(torch.tensor(b["offsets"][f: f + 2]), device=s["dev"])
        assert one.num_frames == 1
        for name, x, y in zip(("energy", "virial", "flux"), call(one), first):
            assert x.shape[0] == 1 and torch.equal(x[0], y[f]), (f, name)


# ---------------------------------------------------------------------------------------------------------------------
# 4. edge cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_frame_no_frames_and_offsets_beyond_the_atoms(backend, dtype):
    s = unblocked(stepped(backend, dtype))
    m, g, b, lib, dev = s["m"], s["g"], batch(), s["lib"], s["dev"]
    m.check()
    n = g.num_atoms
    for x in s["rows"]:  # the empty frame: +0
        row = x[2].reshape(-1)
        assert bool((row == 0).all()) and not bool(torch.signbit(row).any())
    assert float(s["rows"][1][3].abs().max()) == 0.0  # (one atom, no edges)
    # B = 0: AA_OK, nothing written (C ABI, poisoned outputs), and empty results in Python
    none = Frames(torch.tensor([0]), device=dev)
    assert none.num_frames == 0
    fs, gs = none.c_struct(), g.c_struct()
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    out = torch.full((4, 9), 7.0, dtype=dtype, device=dev)
    L, ws = lib.lib, m._workspace
    assert L.aa_model_frame_energies(m._plan_handle, C.byref(fs), n, s["e_atom"].data_ptr(), out.data_ptr(), stream) == 0
    assert L.aa_model_frame_virial(m._plan_handle, C.byref(gs), C.byref(fs), ws.data_ptr(), ws.numel(), out.data_ptr(), stream) == 0
    assert L.aa_model_frame_heat_flux(m._plan_handle, C.byref(gs), C.byref(fs), ws.data_ptr(), ws.numel(), s["vel"].data_ptr(), out.data_ptr(),
                                      stream) == 0
    assert float((out - 7.0).abs().max()) == 0.0
    assert m.frame_energies(s["e_atom"], none).shape == (0,) and m.frame_virial(g, none).shape == (0, 3, 3)
    assert m.frame_heat_flux_potential(g, none, s["vel"]).shape == (0, 3)
    m.check()
    # an offset beyond N: NaN in that frame's row only, check() names the frame, the next step is clean
    off = b["offsets"].copy()
    off[-1] = n + 5
    bad = Frames(torch.tensor(off), device=dev)
    for name, call, want in (("energy", lambda: m.frame_energies(s["e_atom"], bad), s["rows"][0]),
                             ("virial", lambda: m.frame_virial(g, bad), s["rows"][1]),
                             ("flux", lambda: m.frame_heat_flux_potential(g, bad, s["vel"]), s["rows"][2])):
        got = call()
        assert bool(torch.isnan(got[4]).all()), name
        assert torch.equal(got[:4], want[:4]), name
        with pytest.raises(_lib.AllegroError, match="frame 4"):
            m.check()
        m.check()  # (reported once)
    e2, f2 = m.energy_forces(s["pos"], g)
    m.check()
    assert torch.equal(e2, s["e_atom"]) and torch.equal(f2, s["forces"])
    assert torch.equal(m.frame_virial(g, s["frames"]), s["rows"][1])
    with pytest.raises(ValueError, match="non-decreasing"):
        Frames.from_batch(torch.tensor([0, 1, 0]))
    assert Frames.from_batch(torch.tensor(b["batch"]), NUM_FRAMES).frame_atoms.tolist() == b["offsets"].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 5. blocked
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_blocked_twins(backend, dtype):
    s = stepped(backend, dtype)
    m, g = s["m"], s["g"]
    cap = 1000  # (cuts inside frame 0, whose 1 792 edges do not fit one block)
    block_atoms, _ = g.blocks(cap)
    assert 0 < int(block_atoms[1]) < 64
    e, f = m.energy_forces(s["pos"], g, max_block_edges=cap)
    assert m._blocked is not None
    assert_close("blocked step: energies", e.cpu(), s["e_atom"].double().cpu(), dtype)
    fw, fj = m.frame_virial(g, s["frames"]), m.frame_heat_flux_potential(g, s["frames"], s["vel"])
    assert_close("blocked twin: virial", fw.cpu(), s["rows"][1].double().cpu(), dtype)
    assert_close("blocked twin: heat flux", fj.cpu(), s["rows"][2].double().cpu(), dtype)
    assert float(fw[2].abs().max()) == 0.0 and float(fw[0].abs().max()) > 1e-3
    # (the blocked step stays in the workspace: `unblocked` steps again for whoever needs the other one)


# ---------------------------------------------------------------------------------------------------------------------
# 6. forward(data)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_dict(backend, dtype):
    s = stepped(backend, dtype)
    b, dev = batch(), s["dev"]
    fx = load_model_fixture("c2", dtype)
    m = model_from_fixture(fx, dtype, s["lib"], dev)
    data = {"pos": s["pos"], "edge_index": torch.tensor(b["edge_index"], device=dev), "atom_types": torch.zeros(len(b["pos"]), dtype=torch.long, device=dev),
            "cell": torch.tensor(b["cells"], dtype=dtype, device=dev), "edge_cell_shift": torch.tensor(b["cell_shift"], dtype=dtype, device=dev),
            "batch": torch.tensor(b["batch"], device=dev)}
    out = m(data)
    assert isinstance(m._frames_cache[2], Frames) and m._frames_cache[2].frame_atoms.tolist() == b["offsets"].tolist()
    fe, fw, _ = s["rows"]
    assert out["total_energy"].shape == (NUM_FRAMES, 1) and out["stress"].shape == out["virial"].shape == (NUM_FRAMES, 3, 3)
    vol = torch.tensor(np.abs(np.linalg.det(b["cells"])), dtype=torch.float64).reshape(-1, 1, 1)
    assert_close("total_energy", out["total_energy"].reshape(-1).cpu(), fe.double().cpu(), dtype)
    assert_close("virial", out["virial"].cpu(), -fw.double().cpu(), dtype)
    assert_close("stress", out["stress"].cpu(), fw.double().cpu() / vol, dtype)
    assert_close("frame 0: atomic energies against the fixture", out["atomic_energy"].reshape(-1)[:64].cpu(), fx["out"]["atomic_energy"].reshape(-1).double(), dtype)
    assert_close("frame 0: forces against the fixture", out["forces"][:64].cpu(), fx["out"]["forces"].double(), dtype)


@pytest.mark.parametrize("backend", BACKENDS)
def test_unsorted_batch_keeps_the_index_add_route(backend):
    """Two frames of the small `t_coupled` molecule (three species, fp64), atoms of the two frames interleaved: `batch` is not
    non-decreasing, no `Frames` is made, and the outputs -- same keys, same shapes -- are those of the sorted batch, atom for atom."""
    from tests.test_forward_dict import _data, _molecule

    lib, dev = _backend(backend)
    dtype = torch.float64
    fx = load_model_fixture("t_coupled", dtype)
    m = model_from_fixture(fx, dtype, lib, dev)
    pos, cell, ei, shift, types = _molecule()
    f0 = _data(pos, cell, ei, shift, types)
    f1 = _data(pos * 1.01, cell * 1.01, ei, shift, types)
    n = pos.shape[0]
    data = {"pos": torch.cat([f0["pos"], f1["pos"]]), "edge_index": torch.cat([f0["edge_index"], f1["edge_index"] + n], 1),
            "atom_types": torch.cat([f0["atom_types"], f1["atom_types"]]), "cell": torch.stack([f0["cell"], f1["cell"]]),
            "edge_cell_shift": torch.cat([f0["edge_cell_shift"], f1["edge_cell_shift"]]),
            "batch": torch.cat([torch.zeros(n, dtype=torch.long), torch.ones(n, dtype=torch.long)])}
    data = {k: v.to(dev) for k, v in data.items()}
    out = m(data)
    assert isinstance(m._frames_cache[2], Frames) and m._frames_cache[2].frame_atoms.tolist() == [0, n, 2 * n]
    perm = torch.arange(2 * n, device=dev).reshape(2, n).T.reshape(-1)  # new atom k is old atom perm[k]: frames interleaved
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(2 * n, device=dev)
    mixed = dict(data, pos=data["pos"][perm], atom_types=data["atom_types"][perm], batch=data["batch"][perm], edge_index=inv[data["edge_index"]])
    out2 = m(mixed)
    assert m._frames_cache[2] is None
    assert set(out2) == set(out)
    for k in ("total_energy", "stress", "virial"):
        assert out2[k].shape == out[k].shape
        assert_close(f"interleaved batch: {k}", out2[k].cpu(), out[k].double().cpu(), dtype)
    assert_close("interleaved batch: forces", out2["forces"].cpu(), out["forces"][perm].double().cpu(), dtype)


def test_symbols_are_declared_and_exported():
    import os

    from allegro_amd.build import build_library

    lib_path = build_library(verbose=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "allegro_amd.h")).read()
    cdll = C.CDLL(lib_path)
    assert "typedef struct aa_frames {" in src
    for name in ("aa_model_frame_energies", "aa_model_frame_virial", "aa_model_frame_heat_flux", "aa_model_blocked_frame_virial",
                 "aa_model_blocked_frame_heat_flux"):
        assert f"int {name}(" in src and hasattr(cdll, name), name
