"""The deep tail of the eight-wave fused forward (aa_fused8.hip, TAIL = 2): the layer-1 moments reverse and the latent-0 reverse
chain run behind the readout-reverse chain in the forward's tail, on the tiles the wave holds, and `tp_mom_bwd_last` / `gc_64x128`
are not launched.  On the CPU emulation build: AA_FUSED_NARROW=2 (deep tail) against =4 (chain-only tail) against the staged
pipeline -- the forward arithmetic does not move (energies bit-equal between 2 and 4), forces agree to the tolerances the golden
fixtures already carry, and nothing reads a row the deep form no longer writes (poisoned workspace)."""
import numpy as np
import pytest
import torch

from allegro_amd import graph as G
from allegro_amd.nn import HipAllegroModel
from tests.golden_utils import load_model_fixture
from tests.hip_utils import emu_lib, fixture_data, model_from_fixture

GOLDEN_TOL = 5e-5  # x max(1, |want|): the fixtures' tolerance (tests/test_fused.py)
FORM_TOL = 2e-5    # x max(1, |want|): form against form, summation orders differ (tests/test_fused.py)
DEEP_ONLY_ABSENT = ("tp_mom_bwd_last", "gc_64x128")


def _launches(m, pos, g):
    import bench

    return [s[0] for s in bench.profile_stages(m, pos, g, reps=1)]


def _close(a, b, tol):
    return (a - b).abs().max().item() <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("name", ["c2", "c2_l1"])  # the l_max 2 and l_max 1 chain pairs
def test_deep_tail_against_chain_only_tail_and_staged_on_the_golden_fixtures_emulated(name, monkeypatch):
    fx = load_model_fixture(name, torch.float32)
    out, names = {}, {}
    for form, env in (("deep", {"AA_FUSED": "1", "AA_FUSED_NARROW": "2"}), ("chain", {"AA_FUSED": "1", "AA_FUSED_NARROW": "4"}),
                      ("staged", {"AA_FUSED": "0"})):
        monkeypatch.delenv("AA_FUSED_NARROW", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("AA_POISON", "1")
        m = model_from_fixture(fx, torch.float32, emu_lib())
        data, sv = fixture_data(fx, torch.float32)
        g = m.prepare_graph(data["edge_index"], data["atom_types"], data["pos"].shape[0], sv)
        assert 0 < g.max_degree <= 32
        e, f = m.energy_forces(data["pos"], g)
        out[form] = (e.clone(), f.clone())
        names[form] = _launches(m, data["pos"], g)
        for got, want in ((e, fx["out"]["atomic_energy"].reshape(-1)), (f, fx["out"]["forces"])):
            assert torch.isfinite(got).all()
            assert _close(got, want, GOLDEN_TOL), (form, (got - want).abs().max().item())
    assert "fused_fwd" in names["deep"] and "fused_fwd" in names["chain"] and "fused_fwd" not in names["staged"]
    assert not any(n in names["deep"] for n in DEEP_ONLY_ABSENT), names["deep"]
    assert all(n in names["chain"] for n in DEEP_ONLY_ABSENT), names["chain"]
    assert "tp_mom_bwd_first" in names["deep"]
    assert torch.equal(out["deep"][0], out["chain"][0])  # the forward arithmetic did not move
    assert _close(out["deep"][1], out["chain"][1], FORM_TOL)
    assert _close(out["deep"][1], out["staged"][1], FORM_TOL)


def _cfg(l_max):
    return dict(type_names=["A"], r_max=3.4, l_max=l_max, num_layers=2, num_scalar_features=64, num_tensor_features=64,
                radial_chemical_embed={"_target_": "allegro.nn.TwoBodyBesselScalarEmbed", "num_bessels": 8},
                radial_chemical_embed_dim=64, scalar_embed_mlp_hidden_layers_width=64, allegro_mlp_hidden_layers_width=64,
                readout_mlp_hidden_layers_width=64, avg_num_neighbors=20.0, seed=7, tp_path_channel_coupling=True,
                model_dtype="float32", per_type_energy_scales=[1.3], per_type_energy_shifts=[-2.0])


def _periodic_box(long_degree=None, seed=3):
    """A small periodic box (edges across the cell faces: ghost atoms exist) of one species whose segments are cut to chosen lengths:
    atom 0 has no edges, one atom has exactly 32, every other one at most 31 -- or, with `long_degree`, one atom has that many (> 32).
    The atom count is not a multiple of 8.  Edges are center-sorted; per center the nearest neighbours are kept."""
    rng = np.random.default_rng(seed)
    a0 = 1.75
    grid = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(float)
    centre = np.array([2.0, 2.0, 2.0])
    far = np.nonzero(np.abs(grid - centre).max(1) >= 2)[0]
    grid = np.delete(grid, far[rng.permutation(len(far))[:5]], axis=0)  # vacancies away from the crowded site
    inter = centre + 0.5 * np.array([[1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1], [-1, -1, 1], [-1, 1, -1]])  # its cube centres
    pos = np.concatenate([grid, inter]) * a0 + rng.uniform(-0.12, 0.12, size=(len(grid) + 6, 3))
    n = len(pos)
    cell = np.eye(3) * (4 * a0)
    ei, shift = G.neighbor_list_pbc(pos, cell, 3.4)
    d = np.linalg.norm(pos[ei[1]] + shift @ cell - pos[ei[0]], axis=1)
    deg = np.bincount(ei[0], minlength=n)
    big = int(np.argmax(deg[1:])) + 1
    want = long_degree if long_degree else 32
    assert deg[big] >= want, deg
    keep = np.zeros(ei.shape[1], dtype=bool)
    for a in range(1, n):
        idx = np.nonzero(ei[0] == a)[0]
        cap = want if a == big else min(31, 10 + 3 * (a % 8))
        keep[idx[np.argsort(d[idx], kind="stable")[:cap]]] = True
    ei, shift = ei[:, keep], shift[keep]
    deg = np.bincount(ei[0], minlength=n)
    assert deg[0] == 0 and deg[big] == want and deg.max() == want and n % 8 != 0 and np.abs(shift).max() > 0
    return pos, cell, ei, shift, np.zeros(n, dtype=np.int64)


def _run(env, cfg, pos, cell, ei, shift, types, monkeypatch, edges=None):
    monkeypatch.delenv("AA_FUSED_NARROW", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("AA_POISON", "1")
    m = HipAllegroModel(**cfg)
    m._bind_library(emu_lib())
    sv = torch.tensor(shift @ cell, dtype=torch.float32)
    sl = slice(None) if edges is None else slice(*edges)
    g = m.prepare_graph(torch.tensor(ei[:, sl]), torch.tensor(types), pos.shape[0], sv[sl])
    p = torch.tensor(pos, dtype=torch.float32)
    e, f = m.energy_forces(p, g)
    return m, g, e.clone(), f.clone(), _launches(m, p, g)


DEEP = {"AA_FUSED": "1", "AA_FUSED_NARROW": "2"}
CHAIN = {"AA_FUSED": "1", "AA_FUSED_NARROW": "4"}
STAGED = {"AA_FUSED": "0"}


@pytest.mark.parametrize("l_max", [2, 1])
def test_deep_tail_on_cut_segments_shards_and_ghost_atoms_emulated(l_max, monkeypatch):
    """An atom without edges, one with exactly 32, an atom count that is not a multiple of 8, a block with atom0 > 0, ghost atoms;
    the workspace poisoned before every step."""
    from oracle import restatement as R

    cfg = _cfg(l_max)
    pos, cell, ei, shift, types = _periodic_box()
    n = len(pos)
    m, g, e2, f2, n2 = _run(DEEP, cfg, pos, cell, ei, shift, types, monkeypatch)
    assert g.max_degree == 32
    _, _, e4, f4, n4 = _run(CHAIN, cfg, pos, cell, ei, shift, types, monkeypatch)
    _, _, es, fs, ns = _run(STAGED, cfg, pos, cell, ei, shift, types, monkeypatch)
    assert "fused_fwd" in n2 and not any(x in n2 for x in DEEP_ONLY_ABSENT), n2
    assert "fused_fwd" in n4 and all(x in n4 for x in DEEP_ONLY_ABSENT), n4
    assert "fused_fwd" not in ns
    assert torch.isfinite(e2).all() and torch.isfinite(f2).all()
    assert torch.equal(e2, e4)
    assert _close(f2, f4, FORM_TOL) and _close(f2, fs, FORM_TOL) and _close(e2, es, FORM_TOL)
    # against the fp64 oracle on the same (upcast) weights: not further away than twice the fp32 CPU oracle + a small floor (the
    # criterion of tests/fastpath_utils.py for fp32 sums)
    sd = {k[len("func."):]: v.detach().cpu() for k, v in m.state_dict().items()}
    sv = torch.tensor(shift @ cell, dtype=torch.float32)
    tt = torch.tensor(types)
    ref32 = R.allegro_energy_forces(cfg, sd, torch.tensor(pos, dtype=torch.float32), torch.tensor(ei), tt, sv)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    ref64 = R.allegro_energy_forces(dict(cfg, model_dtype="float64"), sd64, torch.tensor(pos), torch.tensor(ei), tt, sv.double())
    for got, w32, w64 in ((e2, ref32["atomic_energy"].reshape(-1), ref64["atomic_energy"].reshape(-1)), (f2, ref32["forces"], ref64["forces"])):
        scale = max(1.0, float(w64.abs().max()))
        err_hip = (got.double() - w64).abs().max().item()
        err_cpu32 = (w32.double() - w64).abs().max().item()
        assert err_hip <= 2.0 * err_cpu32 + 1e-5 * scale, (err_hip, err_cpu32, scale)
    # shards: two atom blocks, the second with atom0 > 0; forces add up, every block owns its atoms' energies
    rowptr = G.csr_from_sorted_centers(ei[0], n)
    cut = 27
    fa, ea = torch.zeros_like(f2), torch.zeros_like(e2)
    for a0, a1 in ((0, cut), (cut, n)):
        mb, gb, eb, fb, nb = _run(DEEP, cfg, pos, cell, ei, shift, types, monkeypatch, edges=(int(rowptr[a0]), int(rowptr[a1])))
        assert not any(x in nb for x in DEEP_ONLY_ABSENT) and "fused_fwd" in nb, nb
        if a0 > 0:
            assert gb.atom_begin == a0
        fa += fb
        ea[a0:a1] = eb[a0:a1]
    assert _close(fa, f2, FORM_TOL)
    has_edges = torch.tensor(np.bincount(ei[0], minlength=n) > 0)
    assert (ea - e2)[has_edges].abs().max().item() <= 1e-5 * max(1.0, float(e2.abs().max()))
    # ghost atoms: every edge across a cell face gets its own ghost behind the real atoms, no shifts remain
    outside = np.abs(shift).sum(1) > 0
    ghost_src = ei[1][outside]
    pos_g = np.concatenate([pos, pos[ghost_src] + shift[outside] @ cell])
    nbr = ei[1].copy()
    nbr[outside] = n + np.arange(int(outside.sum()))
    ei_g = np.stack([ei[0], nbr])
    zero = np.zeros_like(shift)
    _, _, eg, fg, ng = _run(DEEP, cfg, pos_g, cell, ei_g, zero, np.zeros(len(pos_g), dtype=np.int64), monkeypatch)
    assert not any(x in ng for x in DEEP_ONLY_ABSENT) and "fused_fwd" in ng, ng
    folded = fg[:n].clone().index_add_(0, torch.tensor(ghost_src), fg[n:])
    assert _close(folded, f2, FORM_TOL) and _close(eg[:n], e2, FORM_TOL)


def test_one_long_atom_keeps_the_separate_launches_emulated(monkeypatch):
    """A box with one atom above 32 neighbours runs the mixed form: no tail (the team pass's atoms would miss it), the moments reverse
    and the latent-0 chain as launches of their own, and the same result as the staged pipeline."""
    cfg = _cfg(2)
    pos, cell, ei, shift, types = _periodic_box(long_degree=36)
    _, g, e2, f2, n2 = _run(DEEP, cfg, pos, cell, ei, shift, types, monkeypatch)
    assert g.max_degree == 36
    _, _, es, fs, ns = _run(STAGED, cfg, pos, cell, ei, shift, types, monkeypatch)
    assert "fused_fwd" in n2 and all(x in n2 for x in DEEP_ONLY_ABSENT), n2
    assert torch.isfinite(f2).all()
    assert _close(f2, fs, FORM_TOL) and _close(e2, es, FORM_TOL)
