"""Layer-0 moments reverse with its per-edge half in the epilogue of the last reverse chain (StepPlan::mom0_in_chain).

`tp_mom_bwd_first` stops after the per-atom GM0 and the folded 256 -> 64 chain forms d a_e = Y GM0 and the layer-0 slab of
d Y = silu(h) GM0 on its own rows (csrc/aa_gemm.hip, `mom_epilogue`).  `aa_plan_options.mom0_epilogue` selects the form: 1 = wherever it
applies (the new form on these small graphs, which the automatic rule leaves on the two-pass form), 2 = never.

Graphs: the 64-atom Si cell of the C2 fixture (periodic, 28 edges per atom) on the C2 model at l_max 2 and at l_max 1 -- the two
signature pairs the chain's epilogue is compiled for --, and a hand-built graph of 41 atoms with degrees {0, 1, 2, 27, 28, 32} on which
  * 128-row blocks 1 and 3 span more atoms than the chain stages GM0 blocks for (kChainMomSlots = 8): rows read GM0 from global memory,
    blocks 0 and 2 span five / six atoms: rows read it from LDS;
  * segments straddle 32-row tile boundaries and every 128-row block boundary;
  * E = 511 is no multiple of 32 and the last block is partial (127 rows);
  * an atom without edges lies inside a staged atom range (its GM0 block is never written: the workspace is NaN-poisoned),
once without shift vectors and once with a third of the atoms moved by a cell vector and the shift vectors that undo it.

Per graph: energies, forces and virial of the new form against the fp64 oracle under the project's fp32 rule (tests/fastpath_utils.py,
`check` of tests/test_step_values.py); energies of the two forms bit-identical (the forward is the same launch); the largest force
difference between the forms is printed.  On the hand-built graphs the layer-0 slab of d Y and the chain's `trev` output of the two forms
are compared row by row, separately for the rows of the LDS blocks and of the global-memory blocks, within the floor of the same rule
(1e-5 of the output scale): the forms sum the same fp32 products in another order.

Every test exists on the CPU emulation of the unmodified kernels and on the gfx950 library (`gpu`)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from allegro_amd.nn import PreparedGraph
from tests.golden_utils import load_model_fixture
from tests.test_step_values import Rig, _backend, check

SLOTS = 8  # kChainMomSlots (csrc/aa_gemm.hip)
NEW, OLD = 1, 2  # aa_plan_options.mom0_epilogue
HAND_DEGREES = [28, 27, 32, 28, 27,                         # block 0: five atoms; atom 4 straddles row 128
                1, 2, 0, 1, 2, 0, 2, 1, 2, 1, 0, 2,         # block 1: low-degree atoms, 17 atoms in the block
                32, 28, 27, 28,                             # atom 20 straddles row 256
                32, 0, 27, 28, 28,                          # block 2: six atoms, one without edges; atom 25 straddles row 384
                2, 1, 0, 27, 28, 32, 1, 2, 0, 27, 2, 1, 0, 1, 1]  # block 3: partial, 16 atoms


def hand_graph(with_shift):
    """(pos [n,3] float64, edge_index [2,E] center-sorted, types, shift_vec [E,3] | None)"""
    rng = np.random.default_rng(7)
    n = len(HAND_DEGREES)
    pts = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)[:n].astype(float)
    pos = pts + rng.uniform(-0.1, 0.1, size=(n, 3))
    d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    np.fill_diagonal(d, np.inf)
    centers, nbrs = [], []
    for i, k in enumerate(HAND_DEGREES):
        j = np.argsort(d[i], kind="stable")[:k]
        assert k == 0 or d[i, j].max() < 0.98 * 5.0
        centers += [i] * k
        nbrs += j.tolist()
    ei = np.array([centers, nbrs], dtype=np.int64)
    shift = None
    if with_shift:
        cell_a = np.array([9.0, 0.5, -0.25])
        moved = (np.arange(n) % 3 == 1)
        pos = pos + moved[:, None] * cell_a
        # edge vector = pos[nbr] - pos[center] + shift: undo the move
        shift = (moved[ei[0]].astype(float) - moved[ei[1]].astype(float))[:, None] * cell_a
    return pos, ei, np.zeros(n, dtype=np.int64), shift


def si_cell():
    fx = load_model_fixture("c2", torch.float64)
    ei = fx["edge_index"].numpy()
    order = np.argsort(ei[0], kind="stable")
    return fx["pos"].numpy(), ei[:, order], fx["types"].numpy(), fx["shift_vec"].numpy()[order]


GRAPHS = {
    "si64_lmax2": ({}, si_cell),
    "si64_lmax1": (dict(l_max=1), si_cell),
    "hand": ({}, lambda: hand_graph(False)),
    "hand_shift": ({}, lambda: hand_graph(True)),
}


def block_paths(centers):
    """per row: True where its 128-row block stages GM0 in LDS"""
    lds = np.zeros(len(centers), dtype=bool)
    for b0 in range(0, len(centers), 128):
        b1 = min(b0 + 127, len(centers) - 1)
        lds[b0:b1 + 1] = centers[b1] - centers[b0] < SLOTS
    return lds


def test_hand_graph_shape():
    pos, ei, _, _ = hand_graph(False)
    E, c = ei.shape[1], ei[0]
    assert len(pos) == 41 and set(HAND_DEGREES) == {0, 1, 2, 27, 28, 32}
    assert E % 32 != 0 and E % 128 != 0 and (np.diff(c) >= 0).all()
    lds = block_paths(c)
    assert lds[:128].all() and not lds[128:256].any() and lds[256:384].all() and not lds[384:].any()
    for boundary in (32, 128, 256, 384):  # a segment on both sides
        assert c[boundary - 1] == c[boundary]
    # atoms without edges inside a staged range
    assert any(HAND_DEGREES[a] == 0 for a in range(c[256], c[383] + 1))


def _profiled_step(rig, g, p, ws, e, f):
    mx = 64
    ms, by, fl, nst = (C.c_float * mx)(), (C.c_double * mx)(), (C.c_double * mx)(), C.c_int(0)
    names = C.create_string_buffer(32 * mx)
    fn = rig.lib.lib.aa_model_energy_forces_profiled
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    cg = g.c_struct()
    e.fill_(float("nan"))
    f.fill_(float("nan"))
    with rig.ctx():
        rig.lib.check(fn(rig.m._plan_handle, rig.m._blob.data_ptr(), C.byref(cg), p.data_ptr(), ws.data_ptr(), ws.numel(), e.data_ptr(),
                         f.data_ptr(), rig.stream, mx, ms, names, C.byref(nst), by, fl), "aa_model_energy_forces_profiled")
        rig.m.check(rig.dev)
    return {names.raw[32 * i: 32 * i + 32].split(b"\0")[0].decode(): by[i] for i in range(nst.value)}


def _tap(rig, name, g, ws):
    ptr, ld = C.c_void_p(), C.c_int64()
    fn = rig.lib.lib.aa_model_debug_tap
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    rig.lib.check(min(0, fn(rig.m._plan_handle, (name + "+f").encode(), g.num_atoms, g.num_edges, ws.data_ptr(), C.byref(ptr), C.byref(ld))),
                  "aa_model_debug_tap")
    off = ptr.value - ws.data_ptr()
    return ws[off: off + g.num_edges * ld.value * 4].view(torch.float32).view(g.num_edges, ld.value).cpu().clone()


@functools.lru_cache(maxsize=None)
def measured(backend, name):
    overrides, make = GRAPHS[name]
    pos, ei, types, shift = make()
    lib, dev = _backend(backend)
    out = dict(centers=ei[0])
    for form in (NEW, OLD):
        rig = Rig(lib, dev, overrides, dict(mom0_epilogue=form))
        n = len(pos)
        sv = None if shift is None else torch.tensor(shift, dtype=rig.dtype, device=dev)
        g = PreparedGraph(torch.tensor(ei, device=dev), torch.tensor(types, device=dev), n, sv, lib=lib)
        assert g.perm is None or bool((g.perm.cpu() == torch.arange(ei.shape[1])).all())
        p = torch.tensor(pos, dtype=rig.dtype, device=dev)
        ws = rig.workspace(rig.workspace_bytes(g, True))
        e, f = rig.outputs(n)
        stages = _profiled_step(rig, g, p, ws, e, f)
        rc, w = rig.virial(g, ws)
        assert rc == 0
        out[form] = dict(e=e.cpu().clone(), f=f.cpu().clone(), w=w, stages=stages, gsh=_tap(rig, "gsh_env0", g, ws), trev=_tap(rig, "trev", g, ws))
        if form == NEW:
            from oracle import restatement as R

            sd = rig.oracle_weights()
            ei_t, tt = torch.tensor(ei), torch.tensor(types)

            def run(sd_, dt, cfg_):
                pos_, sv_ = torch.tensor(pos, dtype=dt), None if shift is None else torch.tensor(shift, dtype=dt)
                o = R.allegro_energy_forces(cfg_, sd_, pos_, ei_t, tt, sv_)
                return o["atomic_energy"].reshape(-1), o["forces"], R.allegro_virial(cfg_, sd_, pos_, ei_t, tt, sv_).detach()

            sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
            r64, r32 = run(sd64, torch.float64, dict(rig.cfg, model_dtype="float64")), run(sd, torch.float32, rig.cfg)
            out["oracle"] = {q: (r32[i], r64[i]) for i, q in enumerate(("e", "f", "w"))}
    return out


def _forms_and_oracle(backend, name):
    r = measured(backend, name)
    new, old = r[NEW], r[OLD]
    # the forms ran: the two-pass kernel moves the a_e / d a_e rows and the d Y slab, the other form does not
    assert new["stages"]["tp_mom_bwd_first"] < old["stages"]["tp_mom_bwd_first"], (new["stages"], old["stages"])
    assert set(new["stages"]) == set(old["stages"]), (new["stages"], old["stages"])  # (the same launches under the same names)
    for q, what in (("e", "E"), ("f", "F"), ("w", "W")):
        check(name, what, new[q], *r["oracle"][q])
    assert torch.equal(new["e"], old["e"]), name
    df = (new["f"] - old["f"]).abs().max().item()
    print(f"{name} max |F(new form) - F(two-pass form)| = {df:.3e} (max |F| {old['f'].abs().max().item():.3e})")


def _slabs(backend, name):
    r = measured(backend, name)
    lds = torch.tensor(block_paths(r["centers"]))
    assert lds.any() and (~lds).any()
    for what in ("gsh", "trev"):
        a, b = r[NEW][what], r[OLD][what]
        assert torch.isfinite(a).all() and torch.isfinite(b).all() and a.shape == b.shape, (name, what)
        scale = max(1.0, float(b.abs().max()))
        for path, rows in (("lds", lds), ("global", ~lds)):
            err = (a[rows] - b[rows]).abs().max().item()
            print(f"{name} {what} rows of the {path} blocks: max |new - two-pass| = {err:.3e}, scale {scale:.3e}")
            assert err <= 1e-5 * scale, (name, what, path, err, scale)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_forms_and_oracle_emulation(name):
    _forms_and_oracle("emu", name)


@pytest.mark.parametrize("name", ["hand", "hand_shift"])
def test_slabs_emulation(name):
    _slabs("emu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
def test_forms_and_oracle_gpu(name):
    _forms_and_oracle("gpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hand", "hand_shift"])
def test_slabs_gpu(name):
    _slabs("gpu", name)
