"""`allegro_amd_native::energy_forces_pruned` (ExportableAllegro(..., prune=True)): the exported step on the edges inside the model's
per-type-pair cutoffs, reduced on the device from the caller's list and every call's positions (aa_graph_build_* with types); and
`energy_forces`, whose list now goes through aa_graph_build_* too, against the Python model on `PreparedGraph(...)`.

CPU: schema, Meta kernel, torch.export round trip.  GPU: values.  The op and the Python model are compared exactly (same kernels, same
graph arrays, default plan options on both sides); the reference outputs at the tolerances tests/test_neighbor_list_typed.py uses.
"""
import io
import json
import os

import numpy as np
import pytest
import torch

from tests.golden_utils import load_model_fixture
from tests.hip_utils import emu_lib, fixture_data, model_from_fixture
from tests.test_graph_build import GOLDEN_DIR, interleave
from tests.test_neighbor_list_typed import DTYPES, PEREDGE_TABLE, _close

FIXTURES = ["t_peredge", "t_spline_peredge"]


def _setup(name, dtype, device, lib=None, prune=True):
    from allegro_amd.export import ExportableAllegro

    fx = load_model_fixture(name, dtype)
    m = model_from_fixture(fx, dtype, lib, device=device)
    data, sv = fixture_data(fx, dtype, device)
    return fx, m, data, sv, ExportableAllegro(m, device, prune=prune)


def test_pruned_op_is_registered_and_exportable():
    fx, m, data, sv, ex = _setup("t_peredge", torch.float64, "cpu", emu_lib())
    schema = str(torch.ops.allegro_amd_native.energy_forces_pruned.default._schema)
    assert "Tensor? shift_vec" in schema and "int[] config" in schema and "float[] cutoffs" in schema and "-> (Tensor, Tensor, Tensor)" in schema
    assert ex.cutoffs == m.cutoff_table().flatten().tolist() and len(ex.cutoffs) == 9
    assert np.allclose(np.array(ex.cutoffs).reshape(3, 3), PEREDGE_TABLE, rtol=1e-12)
    args = (data["pos"], data["edge_index"], data["atom_types"], sv)
    ep = torch.export.export(ex, args)
    pruned = lambda prog: [n for n in prog.graph.nodes if n.op == "call_function" and "allegro_amd_native.energy_forces_pruned" in str(n.target)]  # noqa: E731
    plain = lambda prog: [n for n in prog.graph.nodes if n.op == "call_function" and str(n.target).startswith("allegro_amd_native.energy_forces.")]  # noqa: E731
    assert len(pruned(ep)) == 1 and len(plain(ep)) == 0
    N = data["pos"].shape[0]
    outs = [n for n in ep.graph.nodes if n.op == "output"][0].args[0]
    assert [tuple(o.meta["val"].shape) for o in outs] == [(N, 1), (1, 1), (N, 3), (1, 3, 3)]
    buf = io.BytesIO()
    torch.export.save(ep, buf)
    buf.seek(0)
    assert len(pruned(torch.export.load(buf))) == 1
    with pytest.raises((NotImplementedError, RuntimeError)):  # no CPU kernel
        ex(*args)
    # the default module is today's: the unpruned op, no table
    fx, m, data, sv, ex0 = _setup("t_peredge", torch.float64, "cpu", emu_lib(), prune=False)
    ep0 = torch.export.export(ex0, args)
    assert ex0.cutoffs is None and len(pruned(ep0)) == 0 and len(plain(ep0)) == 1


def _python_route(m, pos, ei, types, sv):
    g = m.prepare_graph(ei, types, pos.shape[0], sv, pos=pos, prune=True)
    e, f = m.energy_forces(pos, g)
    return g, e.clone(), f.clone(), m.virial(g).clone()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_pruned_op_matches_reference_and_python_route_on_gpu(name, dtype):
    dev = torch.device("cuda:0")
    fx, m, data, sv, ex = _setup(name, dtype, dev)
    pos, types, N = data["pos"], data["atom_types"], data["pos"].shape[0]
    sh = torch.tensor(interleave(np.random.default_rng(11), data["edge_index"][0].cpu().numpy()), device=dev)
    ei, s = data["edge_index"][:, sh], sv[sh]
    g, e, f, w = _python_route(m, pos, ei, types, s)
    assert 0 < g.num_edges < ei.shape[1]
    e_atom, e_tot, forces, vir = ex(pos, ei, types, s)
    assert tuple(e_atom.shape) == (N, 1) and tuple(forces.shape) == (N, 3) and tuple(vir.shape) == (1, 3, 3)
    ref = fx["out"]
    _close(f"{name} E_i", e_atom.reshape(-1), ref["atomic_energy"].reshape(-1), dtype)
    _close(f"{name} F", forces, ref["forces"], dtype)
    print("max |op - python|:", float((e_atom.reshape(-1) - e).abs().max()), float((forces - f).abs().max()), float((vir[0] + w).abs().max()))
    assert torch.equal(e_atom.reshape(-1), e) and torch.equal(forces, f)
    assert torch.equal(vir[0], -w.reshape(3, 3))  # virial = -dE/d(strain)
    assert torch.equal(e_tot.reshape(()), e_atom.sum())
    # int32 indices and a strided list: the same numbers
    wide = torch.zeros((2, ei.shape[1] + 3), dtype=torch.int32, device=dev)
    wide[:, 3:] = ei
    e2, _, f2, v2 = ex(pos, wide[:, 3:], types.to(torch.int32), s)
    assert torch.equal(e2, e_atom) and torch.equal(f2, forces) and torch.equal(v2, vir)
    # moved positions: the list is reduced again.  Atom i of a kept edge i -> j moves away from j until that edge is beyond its cutoff
    table = m.cutoff_table()
    q = int(g.num_edges // 2)
    i, j = int(g.center[q]), int(g.nbr[q])
    r = pos[j] - pos[i] + g.shift_vec[q]
    d = float(r.norm())
    cut = float(table[int(types[i]), int(types[j])])
    assert d < cut
    pos2 = pos.clone()
    pos2[i] -= r / d * (cut - d + 0.25)
    g2, e_2, f_2, w_2 = _python_route(m, pos2, ei, types, s)
    kept = lambda gr: set(zip(gr.center.tolist(), gr.nbr.tolist(), [tuple(v) for v in gr.shift_vec.tolist()]))  # noqa: E731
    assert (i, j, tuple(g.shift_vec[q].tolist())) in kept(g) - kept(g2)
    e_atom2, _, forces2, vir2 = ex(pos2, ei, types, s)
    assert torch.equal(e_atom2.reshape(-1), e_2) and torch.equal(forces2, f_2) and torch.equal(vir2[0], -w_2.reshape(3, 3))
    assert not torch.equal(e_atom2, e_atom)
    # the exported program, saved and re-loaded
    ep = torch.export.export(ex, (pos, ei, types, s))
    buf = io.BytesIO()
    torch.export.save(ep, buf)
    buf.seek(0)
    e3, _, f3, v3 = torch.export.load(buf).module()(pos, ei, types, s)
    assert torch.equal(e3, e_atom) and torch.equal(f3, forces) and torch.equal(v3, vir)
    # a table of the wrong length
    with pytest.raises(RuntimeError, match="cutoffs"):
        torch.ops.allegro_amd_native.energy_forces_pruned(pos, ei, types, s, ex.config, ex.weights, ex.cutoffs[:-1])


def _ghost(dtype):
    z = np.load(os.path.join(GOLDEN_DIR, "model_c2_ghost.npz"))
    base = load_model_fixture(str(z["weights_of"]), dtype)
    assert json.loads(str(z["cfg_json"])) == base["cfg"]
    return base, torch.tensor(z["pos"]).to(dtype), torch.tensor(z["edge_index"]), torch.tensor(z["types"]), None


def _sorted_fixture(dtype):
    fx = load_model_fixture("c2", dtype)
    return fx, fx["pos"].to(dtype), fx["edge_index"], fx["types"], None if fx["shift_vec"] is None else fx["shift_vec"].to(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", ["ghost", "sorted"])
def test_unpruned_op_equals_python_model_bit_for_bit_on_gpu(frame):
    """energy_forces builds its list through aa_graph_build_* now: same graph arrays as PreparedGraph(...), hence the same numbers."""
    from allegro_amd.export import ExportableAllegro
    from allegro_amd.nn import PreparedGraph

    dev, dtype = torch.device("cuda:0"), torch.float32
    fx, pos, ei, types, sv = (_ghost if frame == "ghost" else _sorted_fixture)(dtype)
    is_sorted = bool((ei[0, 1:] >= ei[0, :-1]).all())
    assert is_sorted == (frame == "sorted")
    m = model_from_fixture(fx, dtype, None, device=dev)
    pos, ei, types = pos.to(dev), ei.to(dev), types.to(dev)
    sv = None if sv is None else sv.to(dev)
    g = PreparedGraph(ei, types, pos.shape[0], sv)
    e, f = (x.clone() for x in m.energy_forces(pos, g))
    w = m.virial(g).clone()
    ex = ExportableAllegro(m, dev)
    for _ in range(2):  # (the second call takes the op's graph cache)
        e_atom, _, forces, vir = ex(pos, ei, types, sv)
        print("max |op - python|:", float((e_atom.reshape(-1) - e).abs().max()), float((forces - f).abs().max()), float((vir[0] + w).abs().max()))
        assert torch.equal(e_atom.reshape(-1), e) and torch.equal(forces, f) and torch.equal(vir[0], -w.reshape(3, 3))
