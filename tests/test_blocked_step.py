"""Block-wise inference step (`aa_model_energy_forces_blocked`, `HipAllegroModel.energy_forces(..., max_block_edges=)`).

One frame is evaluated one block of center atoms after the other in an arena sized for the largest block; per-edge `dvec` / `vec`
rows land in frame-wide arrays, forces are assembled once over the frame, and `virial` / `atom_virial` / `heat_flux_potential`
read the frame arrays.  Allegro is strictly local, so the reference of every case is the unblocked step of the same model (and,
for the golden fixtures, the reference's own outputs).

Tolerances are the project's: TOL = 1e-9 (fp64) / 5e-5 (fp32) times max(1, max |expected|); blocked against unblocked 2 x TOL.
`emu`: the unmodified kernels under the CPU emulation; `gpu`: the gfx950 library on the device.

Which case runs in which forward mode is written into the parametrisation, not decided at run time:
* fp32 on the 14-atom frames A and B: every mode (`forward_mode` fixture), both backends -- this is where the modes differ for the
  blocked path (the fused kernels' `vec` rows and their energy fill, in the one-wave and in the two-waves-per-SIMD form);
* fp64: no `forward_mode` at all, on either backend -- an fp64 plan runs the staged stages whatever the mode says
  (tests/test_atom_virial.py::test_matches_the_taps asserts it), so the three runs would be one run three times;
* the golden fixtures (64 / 81 atoms): every mode on the device; under the emulation, where ONE unblocked step of `c2` takes 20 s and
  of `c2_L3` 40 s, the default mode, one blocked pass per case (`EMU_GOLDENS` says which).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd.nn import PreparedGraph
from tests.golden_utils import load_model_fixture
from tests.hip_utils import fixture_data, model_from_fixture
from tests.test_atom_virial import ATTRIBUTIONS, ISOLATED, _backend, build, cfg_for, frame, frame_tensors

TOL = {torch.float64: 1e-9, torch.float32: 5e-5}
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
GOLDENS = [("c2", torch.float32), ("c2_L3", torch.float32), ("t_peredge", torch.float64), ("c5_small", torch.float64)]


def check(name, got, want, bound):
    """max |got - want| <= bound x max(1, max |want|); prints the figure before it asserts."""
    want = want.double().to(got.device)
    scale = max(1.0, float(want.abs().max()))
    err = float((got.double() - want).abs().max())
    print(f"{name}: max|got - expected| = {err:.3e}, bound {bound * scale:.3e} (max|expected| {float(want.abs().max()):.3e})")
    assert err <= bound * scale, name


def one_atom_blocks(g):
    rp = g.rowptr_host()
    return np.arange(g.num_atoms + 1, dtype=np.int64), rp.copy()


def cut_at(g, *atoms):
    ba = np.asarray([0, *atoms, g.num_atoms], dtype=np.int64)
    return ba, g.rowptr_host()[ba].copy()


def step_outputs(m, g, velocities=None):
    """Everything a step leaves behind, cloned: E_i, F are the caller's; virial, the three per-atom virials, the heat flux."""
    out = {"virial": m.virial(g).clone()}
    for a in ATTRIBUTIONS:
        out[a] = m.atom_virial(g, a).clone()
    if velocities is not None:
        out["heat"] = m.heat_flux_potential(g, velocities).clone()
    return out


def frame_case(backend, dtype, species):
    lib, dev = _backend(backend)
    pos, ei, types, shift = frame_tensors(dtype, dev, species)
    m = build(cfg_for(dtype, species=species), lib, dev)
    g = PreparedGraph(ei, types, pos.shape[0], shift, lib=lib)
    return m, g, pos, lib


def fixture_case(backend, name, dtype):
    lib, dev = _backend(backend)
    fx = load_model_fixture(name, dtype)
    m = model_from_fixture(fx, dtype, lib, dev)
    data, sv = fixture_data(fx, dtype, dev)
    g = m.prepare_graph(data["edge_index"], data["atom_types"], data["pos"].shape[0], sv)
    return m, g, data["pos"], fx


# ---------------------------------------------------------------------------------------------------------------------
# 1. one block is the unblocked step
# ---------------------------------------------------------------------------------------------------------------------
def one_block_case(m, g, pos):
    e0, f0 = m.energy_forces(pos, g)
    ref = step_outputs(m, g)
    e1, f1 = m.energy_forces(pos, g, max_block_edges=g.num_edges)
    ba, be = g.blocks(g.num_edges)
    assert ba.tolist() == [0, g.num_atoms] and be.tolist() == [0, g.num_edges]
    got = step_outputs(m, g)
    assert torch.equal(e1, e0) and torch.equal(f1, f0)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    m.check()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("species", [pytest.param(3, id="A"), pytest.param(1, id="B")])
def test_one_block_is_the_unblocked_step_bit_for_bit_fp32(backend, species, forward_mode):
    one_block_case(*frame_case(backend, torch.float32, species)[:3])


@pytest.mark.parametrize("backend", BACKENDS)
def test_one_block_is_the_unblocked_step_bit_for_bit_fp64(backend):
    one_block_case(*frame_case(backend, torch.float64, 3)[:3])


@pytest.mark.gpu
def test_one_block_is_the_unblocked_step_bit_for_bit_c2_gpu(forward_mode):
    one_block_case(*fixture_case("gpu", "c2", torch.float32)[:3])


def test_one_block_is_the_unblocked_step_bit_for_bit_c2_emu():
    one_block_case(*fixture_case("emu", "c2", torch.float32)[:3])


# ---------------------------------------------------------------------------------------------------------------------
# 2. one atom per block, two blocks
# ---------------------------------------------------------------------------------------------------------------------
FRAMES = [pytest.param(3, id="A"), pytest.param(1, id="B")]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("species", FRAMES)
def test_blocks_reproduce_the_unblocked_step_fp32(backend, species, forward_mode):
    blocks_case(backend, species, torch.float32)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("species", FRAMES)
def test_blocks_reproduce_the_unblocked_step_fp64(backend, species):
    blocks_case(backend, species, torch.float64)


def blocks_case(backend, species, dtype):
    """Frame A: three species, ZBL, a shortened pair cutoff, an isolated atom; frame B: the same atoms as one species."""
    m, g, pos, _ = frame_case(backend, dtype, species)
    n = g.num_atoms
    vel = torch.randn(n, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(pos.device).to(dtype)
    e0, f0 = (t.clone() for t in m.energy_forces(pos, g))
    ref = step_outputs(m, g, vel)
    assert float(ref["center"].abs().max()) > 1e-3
    rp = g.rowptr_host()
    assert rp[ISOLATED + 1] == rp[ISOLATED]  # (the isolated atom is a block without edges)
    for what, (ba, be) in (("one atom per block", one_atom_blocks(g)), ("two blocks cut at atom 7", cut_at(g, 7))):
        assert len(ba) - 1 == (n if what.startswith("one") else 2)
        e, f = m.energy_forces_blocks(pos, g, ba, be)
        got = step_outputs(m, g, vel)
        check(f"{what}: E_i", e, e0, 2 * TOL[dtype])
        check(f"{what}: F", f, f0, 2 * TOL[dtype])
        for k in ("virial",) + ATTRIBUTIONS:
            check(f"{what}: {k}", got[k], ref[k], 2 * TOL[dtype])
        # sum rules of the blocked result itself
        fscale = max(1.0, float(f0.abs().max()))
        print(f"{what}: |sum F| = {float(f.double().sum(0).abs().max()):.3e}")
        assert float(f.double().sum(0).abs().max()) <= TOL[dtype] * fscale
        for a in ATTRIBUTIONS:
            check(f"{what}: sum over atoms, {a}", got[a].double().sum(0), got["virial"], TOL[dtype])
        assert float(got["center"][ISOLATED].abs().max()) == 0.0
        # heat flux: the einsum of the neighbor tensor -- the one the UNBLOCKED step left, so that the blocked frame arrays are checked
        # against something they did not produce
        want = -torch.einsum("na,nab->b", vel.double(), ref["neighbor"].double())
        check(f"{what}: heat flux vs the einsum of the unblocked neighbor tensor", got["heat"], want, 2 * TOL[dtype])
        check(f"{what}: heat flux vs the unblocked step", got["heat"], ref["heat"], 2 * TOL[dtype])
        m.check()
    # the unblocked step afterwards is what it was (the kind of step that ran last decides what virial() reads)
    e2, f2 = m.energy_forces(pos, g)
    assert torch.equal(e2, e0) and torch.equal(f2, f0)
    assert torch.equal(m.virial(g), ref["virial"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. goldens through blocks
# ---------------------------------------------------------------------------------------------------------------------
def assert_golden(name, what, e, f, fx, dtype):
    ref = fx["out"]
    check(f"{name} {what}: E_i vs the reference", e.cpu(), ref["atomic_energy"].reshape(-1), TOL[dtype])
    check(f"{name} {what}: F vs the reference", f.cpu(), ref["forces"], TOL[dtype])
    if dtype == torch.float32:
        err = float((f.cpu() - ref["forces"]).abs().max())
        print(f"{name} {what}: max|F - reference| = {err:.3e} (< 1e-4)")
        assert err < 1e-4


CUTS = [pytest.param("2deg", id="blocks-of-2-max-degree"), pytest.param("atoms", id="one-atom-per-block")]


def golden_case(backend, name, dtype, cut):
    m, g, pos, fx = fixture_case(backend, name, dtype)
    if cut == "2deg":
        cap = 2 * g.max_degree
        ba, be = g.blocks(cap)
        assert len(ba) > 2 and int(np.diff(be).max()) <= cap
        e, f = m.energy_forces(pos, g, max_block_edges=cap)
        assert_golden(name, f"{len(ba) - 1} blocks of <= {cap} edges", e, f, fx, dtype)
    else:
        e, f = m.energy_forces_blocks(pos, g, *one_atom_blocks(g))
        assert_golden(name, "one atom per block", e, f, fx, dtype)
    m.check()


@pytest.mark.gpu
@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("name,dtype", GOLDENS)
def test_goldens_through_blocks_gpu(name, dtype, cut, forward_mode):
    golden_case("gpu", name, dtype, cut)


# Under the emulation a blocked pass costs about 1.5 unblocked steps in blocks of 2 x max_degree and 2.5 with one atom per block
# (c2 30 / 50 s, c2_L3 60 / 100 s, c5_small 50 / 95 s, t_peredge 10 / 20 s).  Both cuts run on the 24-atom t_peredge (fp64) and on c2
# (fp32, fused forward); c2_L3 and c5_small (the operator path) add the blocks of 2 x max_degree.  One atom per block on those two
# is a device case (above): it differs from the cases kept here in the number of blocks only, not in a code path.
EMU_GOLDENS = [(n, d, c) for n, d in GOLDENS for c in ("2deg", "atoms") if c == "2deg" or n in ("c2", "t_peredge")]


@pytest.mark.parametrize("name,dtype,cut", EMU_GOLDENS, ids=[f"{n}-{c}" for n, _, c in EMU_GOLDENS])
def test_goldens_through_blocks_emu(name, dtype, cut):
    golden_case("emu", name, dtype, cut)


def test_c2_unblocked_step_meets_the_golden_bounds_emu():
    """The bounds of the two tests above are the reference's, not the new code's: the unblocked step meets them."""
    m, g, pos, fx = fixture_case("emu", "c2", torch.float32)
    e, f = m.energy_forces(pos, g)
    assert_golden("c2", "unblocked", e, f, fx, torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 4. reproducible
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_bit_reproducible_on_a_refilled_workspace(backend):
    m, g, pos, _ = frame_case(backend, torch.float32, 3)
    ba, be = cut_at(g, 4, 7, 11)
    runs = []
    for _ in range(2):
        e, f = m.energy_forces_blocks(pos, g, ba, be)
        runs.append([e.clone(), f.clone()] + [m.atom_virial(g, a).clone() for a in ATTRIBUTIONS])
        m._workspace.fill_(255)  # 0xFF bytes: NaN in fp32 and fp64
    for what, first, second in zip(("E_i", "F") + ATTRIBUTIONS, *runs):
        assert torch.isfinite(first).all(), what
        assert torch.equal(first, second), what


# ---------------------------------------------------------------------------------------------------------------------
# 5. the cut check and the refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [pytest.param(torch.float64, id="f64"), pytest.param(torch.float32, id="f32")])
def test_a_wrong_cut_gives_nan_and_is_reported(backend, dtype):
    lib, dev = _backend(backend)
    pos, ei, types, shift = frame_tensors(dtype, dev)
    m = build(cfg_for(dtype, num_scalar_features=16, num_tensor_features=8), lib, dev)  # (a small model: the check does not depend on its size)
    g = PreparedGraph(ei, types, pos.shape[0], shift, lib=lib)
    e0, f0 = (t.clone() for t in m.energy_forces(pos, g))
    ba, be = cut_at(g, 4, 7, 11)
    wrong = be.copy()
    wrong[2] += 1  # the cut between blocks 1 and 2: block 1 is the first one that sees it
    e, f = m.energy_forces_blocks(pos, g, ba, wrong)
    assert bool(torch.isnan(e).all()) and bool(torch.isnan(f).all())
    with pytest.raises(_lib.AllegroError, match="wrong cut for block 1"):
        m.check()
    m.check()  # (reported once)
    # ... or by the next call, whichever comes first
    wrong[2] -= 2
    e, f = m.energy_forces_blocks(pos, g, ba, wrong)
    if pos.is_cuda:
        torch.cuda.synchronize()
    assert bool(torch.isnan(e).all()) and bool(torch.isnan(f).all())
    with pytest.raises(_lib.AllegroError, match="wrong cut for block 1"):
        m.energy_forces(pos, g)
    e, f = m.energy_forces_blocks(pos, g, ba, be)
    check("after the refused calls: E_i", e, e0, 2 * TOL[dtype])
    check("after the refused calls: F", f, f0, 2 * TOL[dtype])
    m.check()


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    lib, dev = _backend(backend)
    dtype = torch.float64
    pos, ei, types, shift = frame_tensors(dtype, dev)
    over = dict(num_scalar_features=16, num_tensor_features=8)  # (a small model: the guards do not depend on its size)
    m = build(cfg_for(dtype, **over), lib, dev)
    g = PreparedGraph(ei, types, 14, shift, lib=lib)
    g_at = PreparedGraph(ei, types, 14, shift, transposed=False, lib=lib)
    rp = g.rowptr_host()
    ba, be = cut_at(g, 7)
    for read in (lambda: m.virial(g), lambda: m.atom_virial(g, "center")):  # (before any step: said so, in the same words)
        with pytest.raises(RuntimeError, match="call energy_forces first"):
            read()
    e0, f0 = (t.clone() for t in m.energy_forces_blocks(pos, g, ba, be))
    assert bool(torch.isfinite(e0).all()) and bool(torch.isfinite(f0).all())

    def refused(match, graph, block_atoms, block_edges, with_forces=True):
        with pytest.raises(_lib.AllegroError, match=match) as err:
            m.energy_forces_blocks(pos, graph, block_atoms, block_edges, with_forces)
        assert "(-1)" in str(err.value)  # AA_ERR_INVALID

    bad = np.asarray([0, 9, 7, 14], dtype=np.int64)
    refused("block_atoms must be non-decreasing", g, bad, rp[bad])
    refused("block_edges must be non-decreasing", g, np.asarray([0, 7, 9, 14]), np.asarray([0, rp[9], rp[7], rp[14]]))
    refused("block_atoms must run from 0 to num_atoms", g, np.asarray([0, 7, 13]), np.asarray([0, rp[7], rp[14]]))
    refused("block_atoms must run from 0 to num_atoms", g, np.asarray([1, 7, 14]), np.asarray([0, rp[7], rp[14]]))
    refused("block_edges must run from 0 to num_edges", g, ba, np.asarray([0, rp[7], rp[14] - 1]))
    refused("transposed CSR", g_at, ba, be)
    # (energy only: no force assembly, no transposed CSR needed)
    e, f = m.energy_forces_blocks(pos, g_at, ba, be, with_forces=False)
    assert f is None
    check("energy only, without the transposed CSR", e, e0, 2 * TOL[dtype])
    # (... and nothing for virial / atom_virial to read: said so, not answered from arrays that were never laid out)
    with pytest.raises(RuntimeError, match="energy-only"):
        m.virial(g_at)
    with pytest.raises(RuntimeError, match="energy-only"):
        m.atom_virial(g_at, "center")
    m.enable_debug_taps(True)
    refused("debug taps", g, ba, be)
    m.enable_debug_taps(False)
    if backend == "gpu":  # (the emulation has no stream capture to enable)
        m.enable_hip_graph(True)
        refused("hipGraph", g, ba, be)
        m.enable_hip_graph(False)
    with pytest.raises(ValueError, match=r"\[B\+1\]"):
        m.energy_forces_blocks(pos, g, ba, be[:-1])
    # a workspace sized for the unblocked energy-only step is too small for the frame arrays
    need = lib.lib.aa_model_blocked_workspace_bytes(m._plan_handle, 14, g.num_edges, int(np.diff(be).max()), 1)
    small = torch.empty(need - 256, dtype=torch.uint8, device=dev)
    gs = g.c_struct()
    i64p = C.POINTER(C.c_int64)
    out_e, out_f = torch.full((14,), 7.0, dtype=dtype, device=dev), torch.full((14, 3), 7.0, dtype=dtype, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    rc = lib.lib.aa_model_energy_forces_blocked(m._plan_handle, m._blob.data_ptr(), C.byref(gs), pos.data_ptr(), 2, ba.ctypes.data_as(i64p),
                                                be.ctypes.data_as(i64p), small.data_ptr(), small.numel(), out_e.data_ptr(), out_f.data_ptr(), stream)
    assert rc == -2 and b"workspace too small" in lib.lib.aa_last_error()  # AA_ERR_WORKSPACE
    w9 = torch.empty(9, dtype=dtype, device=dev)
    rc = lib.lib.aa_model_blocked_virial(m._plan_handle, C.byref(gs), int(np.diff(be).max()), small.data_ptr(), small.numel(), w9.data_ptr(), stream)
    assert rc == -2
    rc = lib.lib.aa_model_blocked_atom_virial(m._plan_handle, C.byref(gs), int(np.diff(be).max()), m._workspace.data_ptr(), m._workspace.numel(), 3,
                                              w9.data_ptr(), stream)
    assert rc == -1 and b"attribution" in lib.lib.aa_last_error()
    assert float((out_e - 7.0).abs().max()) == 0.0 and float((out_f - 7.0).abs().max()) == 0.0  # (a refused call writes nothing)
    # and everything still works
    e, f = m.energy_forces_blocks(pos, g, ba, be)
    assert torch.equal(e, e0) and torch.equal(f, f0)
    m.check()


# ---------------------------------------------------------------------------------------------------------------------
# 6. PreparedGraph.blocks (host logic)
# ---------------------------------------------------------------------------------------------------------------------
def test_blocks_host_logic():
    fr = frame()
    ei, types = torch.tensor(fr["ei"]), torch.tensor(fr["types"])
    g = PreparedGraph(ei, types, 14, None, transposed=False)
    rp = np.concatenate([[0], np.cumsum(fr["deg"])]).astype(np.int64)
    dmax = int(fr["deg"].max())
    assert np.array_equal(g.rowptr_host(), rp) and g.rowptr_host() is g.rowptr_host()  # (one host read, kept)
    for cap in (dmax, dmax + 1, 2 * dmax, 3 * dmax + 5, int(rp[-1]) - 1, int(rp[-1]), 10 * int(rp[-1])):
        ba, be = g.blocks(cap)
        assert ba.dtype == np.int64 and be.dtype == np.int64 and len(ba) == len(be) >= 2
        assert ba[0] == 0 and ba[-1] == 14 and (np.diff(ba) > 0).all()
        assert np.array_equal(be, rp[ba])                      # the cuts are the row pointers of their atoms
        assert int(np.diff(be).max()) <= cap                   # every block within the cap
        for b in range(len(ba) - 2):                           # greedy: the next atom would not have fitted
            assert rp[ba[b + 1] + 1] - be[b] > cap
    assert g.blocks(int(rp[-1]))[0].tolist() == [0, 14]
    # atoms without edges ride along: the isolated atom (the last one) never opens a block of its own unless it must
    ba, _ = g.blocks(dmax)
    assert ISOLATED == 13 and ISOLATED not in ba[1:-1].tolist()
    with pytest.raises(ValueError, match=rf"atom {int(fr['deg'].argmax())} has {dmax} edges"):
        g.blocks(dmax - 1)
    # a frame without edges is one block; leading and trailing edge-less atoms join their neighbours
    g0 = PreparedGraph(torch.zeros((2, 0), dtype=torch.long), types, 14, None, transposed=False)
    assert [a.tolist() for a in g0.blocks(0)] == [[0, 14], [0, 0]]
    ei2 = torch.tensor([[3, 3, 4, 6, 6, 6], [4, 6, 3, 3, 4, 1]])
    g2 = PreparedGraph(ei2, types[:9], 9, None, transposed=False)
    for cap in (3, 4, 5):  # atoms 0-2 lead, atom 5 rides along with the block of atoms 3 and 4, atoms 7-8 with atom 6
        assert [a.tolist() for a in g2.blocks(cap)] == [[0, 6, 9], [0, 3, 6]]
    assert [a.tolist() for a in g2.blocks(6)] == [[0, 9], [0, 6]]


# ---------------------------------------------------------------------------------------------------------------------
# 7. the workspace claim (size functions only: no step runs)
# ---------------------------------------------------------------------------------------------------------------------
def roundup256(n):
    return (n + 255) // 256 * 256


def assert_workspace_claim(L, plan, n, e, cap, esize):
    whole = L.aa_model_workspace_bytes(plan, n, e, 1)
    with_f, without = L.aa_model_blocked_workspace_bytes(plan, n, e, cap, 1), L.aa_model_blocked_workspace_bytes(plan, n, e, cap, 0)
    bound_f = L.aa_model_workspace_bytes(plan, n, cap, 1) + 2 * roundup256(4 * e * esize) + 4 * (n + 1) + 65536
    bound_0 = L.aa_model_workspace_bytes(plan, n, cap, 0) + 4 * (n + 1) + 65536
    print(f"N={n} E={e} cap={cap}: whole frame {whole} B, blocked {with_f} B (bound {bound_f}), energy only {without} B (bound {bound_0})")
    assert 0 < with_f <= bound_f and 0 < without <= bound_0 and without < with_f
    return whole, with_f


@pytest.mark.parametrize("name,dtype", GOLDENS)
def test_workspace_claim_on_the_fixture_plans(name, dtype):
    from tests.hip_utils import emu_lib

    lib = emu_lib()
    fx = load_model_fixture(name, dtype)
    m = model_from_fixture(fx, dtype, lib, "cpu")
    m._ensure_plan()
    n, e = fx["pos"].shape[0], fx["edge_index"].shape[1]
    esize = 4 if dtype == torch.float32 else 8
    for cap in (e, max(1, e // 8), 1, 0):
        assert_workspace_claim(lib.lib, m._plan_handle, n, e, cap, esize)
    # a cap beyond the frame is the frame
    assert lib.lib.aa_model_blocked_workspace_bytes(m._plan_handle, n, e, 10 * e, 1) == lib.lib.aa_model_blocked_workspace_bytes(m._plan_handle, n, e, e, 1)


def test_workspace_claim_at_the_headline_shape():
    """C4: 97 336 atoms, 2 725 408 edges, the headline configuration, cut into eight: the per-edge workspace is paid for an eighth
    of the edges, 32 B per edge stay frame-wide."""
    import bench
    from allegro_amd.nn import HipAllegroModel
    from tests.hip_utils import emu_lib

    lib = emu_lib()
    n, e = 97336, 2725408
    m = HipAllegroModel(**bench.si_model_cfg(e / n), model_dtype=bench.WORKLOADS["c4"]["dtype"])
    assert m.dtype == torch.float32
    m._bind_library(lib)
    m._ensure_plan()
    whole, blocked = assert_workspace_claim(lib.lib, m._plan_handle, n, e, e // 8, 4)
    assert whole > 20e9  # the 21.8 GB of the whole frame
    assert blocked < whole / 5


@pytest.mark.parametrize("with_forces", [True, False])
def test_max_block_edges_for_is_the_last_cap_that_fits(with_forces):
    from tests.hip_utils import emu_lib

    lib = emu_lib()
    fx = load_model_fixture("c2", torch.float32)
    m = model_from_fixture(fx, torch.float32, lib, "cpu")
    data, sv = fixture_data(fx, torch.float32, "cpu")
    g = m.prepare_graph(data["edge_index"], data["atom_types"], data["pos"].shape[0], sv)
    n, e = g.num_atoms, g.num_edges
    size = lambda cap: lib.lib.aa_model_blocked_workspace_bytes(m._plan_handle, n, e, cap, int(with_forces))  # noqa: E731
    m._ensure_plan()
    lo, hi = size(g.max_degree), size(e)
    assert lo < hi
    for budget in (lo, lo + 1, (lo + hi) // 2, (lo + 3 * hi) // 4, hi - 1):
        cap = m.max_block_edges_for(g, budget, with_forces)
        assert g.max_degree <= cap < e
        assert size(cap) <= budget < size(cap + 1)
        # atom-granular: the blocks it gives fit, and with one more atom's edges the largest one would not have
        ba, be = g.blocks(cap)
        assert size(int(np.diff(be).max())) <= budget
    assert m.max_block_edges_for(g, hi, with_forces) == e and m.max_block_edges_for(g, 10 * hi, with_forces) == e
    with pytest.raises(ValueError, match="one-atom blocks"):
        m.max_block_edges_for(g, lo - 1, with_forces)
