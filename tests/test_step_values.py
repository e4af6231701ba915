"""The step table by value: what every case of tests/test_step_plan.py computes, not only which kernels it launches.

tests/test_step_plan.py runs every selectable step on a NaN-poisoned workspace and asserts its launch list; a step can launch
exactly those kernels and still return wrong numbers.  This module runs the same cases (same model, plan options, graph
recipe, forces flag, taps, hints) through `aa_model_energy_forces` and asserts

1. atom energies and forces against `oracle.restatement.allegro_energy_forces` on the model's own weights:
   fp64 plans within 1e-9 x max(1, max |expected|); fp32 plans by the criterion of tests/fastpath_utils.py (not further from the
   fp64 oracle on the upcast weights than twice the fp32 CPU oracle is, + 1e-5 of the output scale).  The cases without
   atoms / without edges are compared exactly (energies = per-type shifts = 0, forces = 0);
2. behind every force step `aa_model_virial` against `oracle.restatement.allegro_virial` under the same two rules, and
   `aa_model_atom_virial`: sum over the atoms = the 3x3 result (1e-12 fp64 / 1e-5 fp32 of max |W|: both sum the same products in
   double), zero rows for atoms without edges, AA_ERR_INVALID for the neighbor attribution without the transposed CSR (and the
   workspace untouched by the refused call); behind every energy-only step `aa_model_virial` is refused with AA_ERR_WORKSPACE;
3. one plan, one workspace and one set of output buffers across a sequence of different graphs: every step equal to the same
   step on a fresh plan, workspace and buffers.  (The same sequence with the captured step graph of `aa_model_plan_enable_graph`
   on a poisoned workspace is NOT here: it ended in an illegal memory access on the device and the cause is not known.)

Every test exists twice: on the CPU emulation of the unmodified kernels, and on the gfx950 library (`gpu`).  On the device all
cases of the table run, the `cus_matter` ones included: their launch list depends on the CU count, the right answer does not.

`-s` prints `name quantity err_hip err_cpu32 scale` per case; DESIGN.md section 5 quotes the worst ratios of those logs."""
import ctypes as C

import numpy as np
import pytest
import torch

from allegro_amd import _lib
from allegro_amd.nn import HipAllegroModel, PreparedGraph
from tests.fastpath_utils import oracle64_errors
from tests.test_fused_deep_tail import FORM_TOL
from tests.test_plan_pipeline import BASE, PIPELINES
from tests.test_step_plan import (BLOCK, CASES, DENSE, EXPECTED, F64, L128, LONG_ATOM, LOW12, MID, NAMES, NO_EDGES, grid_graph)

AA_ERR_INVALID, AA_ERR_WORKSPACE = -1, -2
CENTER, NEIGHBOR = 0, 1  # AA_ATOM_VIRIAL_*


def _backend(name):
    if name == "emu":
        from tests.hip_utils import emu_lib

        return emu_lib(), torch.device("cpu")
    assert torch.cuda.is_available()
    return _lib.load(), torch.device("cuda:0")


# ---- one model + one plan, stepped through the C ABI with caller-owned buffers ---------------------------------------------
class Rig:
    """The model of `overrides` on the C2 shape and one plan with `options` + poison_workspace, as `run_case` builds them."""

    def __init__(self, lib, dev, overrides, options, taps=False):
        self.lib, self.dev = lib, dev
        self.cfg = dict(BASE, **overrides)
        m = HipAllegroModel(**self.cfg).to(dev)
        m._bind_library(lib)
        m._select_device(dev)
        cfg, keep = m._build_config()
        opt = _lib.PlanOptions()
        opt.poison_workspace = 1
        for k, v in options.items():
            setattr(opt, k, v)
        m._plan_handle, m._plan_keep = lib.model_plan_create(cfg, opt), (cfg, keep)
        if taps:
            m.enable_debug_taps()
        m._ensure_weights(dev)
        self.m, self.dtype = m, m.dtype
        self.stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
        self.ctx = (lambda: torch.cuda.device(dev)) if dev.type == "cuda" else torch.no_grad

    def graph(self, recipe, no_tcsr=False, max_degree=None):
        """(PreparedGraph, positions [max(n, 1), 3] in the model dtype, n, (pos, edge_index, types) as numpy)"""
        pos, ei, types = grid_graph(**recipe)
        n = len(pos)
        g = PreparedGraph(torch.tensor(ei, device=self.dev), torch.tensor(types if n else [0], device=self.dev), n, None,
                          transposed=not no_tcsr, lib=self.lib)
        if max_degree is not None:
            g.max_degree = max_degree
        p = torch.zeros((max(n, 1), 3), dtype=self.dtype, device=self.dev)  # (no atoms: the library still wants non-null arrays)
        p[:n] = torch.tensor(pos, dtype=self.dtype)
        return g, p, n, (pos, ei, types)

    def workspace_bytes(self, g, forces):
        return self.lib.lib.aa_model_workspace_bytes(self.m._plan_handle, g.num_atoms, g.num_edges, int(forces))

    def workspace(self, nbytes):
        return torch.empty(nbytes + 256, dtype=torch.uint8, device=self.dev)

    def outputs(self, rows):
        return torch.empty(rows, dtype=self.dtype, device=self.dev), torch.empty((rows, 3), dtype=self.dtype, device=self.dev)

    def step(self, g, p, ws, e, f):
        """One `aa_model_energy_forces` into e (and f, unless None), both NaN before the call; waits for it and for the hint check."""
        e.fill_(float("nan"))
        if f is not None:
            f.fill_(float("nan"))
        cg = g.c_struct()
        with self.ctx():
            self.lib.check(self.lib.lib.aa_model_energy_forces(self.m._plan_handle, self.m._blob.data_ptr(), C.byref(cg), p.data_ptr(), ws.data_ptr(),
                                                               ws.numel(), e.data_ptr(), f.data_ptr() if f is not None else None, self.stream),
                           "aa_model_energy_forces")
            self.m.check(self.dev)

    def virial(self, g, ws):
        """(return code, [3,3] on the host | None)"""
        out = torch.full((9,), float("nan"), dtype=self.dtype, device=self.dev)
        cg = g.c_struct()
        with self.ctx():
            rc = self.lib.lib.aa_model_virial(self.m._plan_handle, C.byref(cg), ws.data_ptr(), ws.numel(), out.data_ptr(), self.stream)
        return rc, (out.cpu().view(3, 3) if rc == 0 else None)

    def atom_virial(self, g, ws, attribution):
        """(return code, [n,3,3] on the host | None)"""
        out = torch.full((max(g.num_atoms, 1), 3, 3), float("nan"), dtype=self.dtype, device=self.dev)
        cg = g.c_struct()
        with self.ctx():
            rc = self.lib.lib.aa_model_atom_virial(self.m._plan_handle, C.byref(cg), ws.data_ptr(), ws.numel(), attribution, out.data_ptr(), self.stream)
        return rc, (out[:g.num_atoms].cpu() if rc == 0 else None)

    def last_error(self):
        return self.lib.lib.aa_last_error().decode()

    def oracle_weights(self):
        return {k[len("func."):]: v.detach().cpu() for k, v in self.m.state_dict().items()}


# ---- the oracle, once per (model, graph) -----------------------------------------------------------------------------------
_ORACLE = {}


def oracle(rig, overrides, recipe, numpy_graph):
    """{"e", "f", "w"}: per quantity (fp32 oracle | None, fp64 oracle) on the weights of `rig`'s model -- for an fp64 model the
    fp64 oracle on its own weights, for an fp32 one the fp32 oracle and the fp64 oracle on the upcast weights (the two runs of
    tests/fastpath_utils.py::_vs_oracle64).  None for a graph without edges: nothing to evaluate, the answer is exactly zero."""
    key = (repr(sorted(overrides.items())), repr(sorted(recipe.items())))
    if key not in _ORACLE:
        from oracle import restatement as R

        pos, ei, types = numpy_graph
        if ei.shape[1] == 0:
            _ORACLE[key] = None
            return None
        sd = rig.oracle_weights()
        ei_t, tt = torch.tensor(ei), torch.tensor(types)

        def run(sd_, pos_, cfg_):
            out = R.allegro_energy_forces(cfg_, sd_, pos_, ei_t, tt)
            return out["atomic_energy"].reshape(-1), out["forces"], R.allegro_virial(cfg_, sd_, pos_, ei_t, tt).detach()

        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        r64 = run(sd64, torch.tensor(pos), dict(rig.cfg, model_dtype="float64"))
        r32 = (None, None, None) if rig.dtype == torch.float64 else run(sd, torch.tensor(pos, dtype=torch.float32), rig.cfg)
        _ORACLE[key] = {q: (r32[i], r64[i]) for i, q in enumerate(("e", "f", "w"))}
    return _ORACLE[key]


# ---- one case of the table: the step and everything read behind it, as host tensors ---------------------------------------------
def measured(backend, case):
    name, overrides, options, recipe, extra = case
    lib, dev = _backend(backend)
    rig = Rig(lib, dev, overrides, options, taps=extra.get("taps", False))
    g, p, n, numpy_graph = rig.graph(recipe, no_tcsr=extra.get("no_tcsr", False), max_degree=extra.get("max_degree"))
    forces = extra.get("forces", True)
    ws = rig.workspace(rig.workspace_bytes(g, forces))
    e, f = rig.outputs(max(n, 1))
    rig.step(g, p, ws, e, f if forces else None)
    out = dict(n=n, dtype=rig.dtype, forces=forces, e=e[:n].cpu(), f=f[:n].cpu() if forces else None, oracle=oracle(rig, overrides, recipe, numpy_graph),
               degree=np.bincount(numpy_graph[1][0], minlength=n), in_degree=np.bincount(numpy_graph[1][1], minlength=n), tcsr=g.t_perm is not None)
    if forces:
        out["w_rc"], out["w"] = rig.virial(g, ws)
        out["wc_rc"], out["wc"] = rig.atom_virial(g, ws, CENTER)
        out["wn_rc"], out["wn"] = rig.atom_virial(g, ws, NEIGHBOR)
        out["wn_error"] = rig.last_error() if out["wn_rc"] else ""
        out["w_again_rc"], out["w_again"] = rig.virial(g, ws)  # (behind the per-atom calls, one of them refused without the transposed CSR)
    else:
        # a workspace sized for an energy-only step has no dvec / vec rows of a reverse pass
        out["sized_for_forces"] = rig.workspace_bytes(g, True)
        out["sized"] = ws.numel()
        out["w_rc"], out["w"] = rig.virial(g, ws)
        out["w_error"] = rig.last_error()
    return out


def check(name, what, got, w32, w64):
    """The project's two rules; prints `name what err_hip err_cpu32 scale` (fp64: err, 0, scale) and returns the printed figures."""
    assert torch.isfinite(got).all(), (name, what)
    if w32 is None:
        scale = max(1.0, float(w64.abs().max()))
        err = (got - w64).abs().max().item()
        print(f"{name} {what} f64 err {err:.3e} scale {scale:.3e} rel {err / scale:.3e}")
        assert err <= 1e-9 * scale, (name, what, err, scale)
        return err, 0.0, scale
    err_hip, err_cpu32, scale = oracle64_errors(got, w32, w64)
    print(f"{name} {what} f32 err_hip {err_hip:.3e} err_cpu32 {err_cpu32:.3e} scale {scale:.3e} ratio {err_hip / max(err_cpu32, 1e-300):.3f}")
    assert err_hip <= 2.0 * err_cpu32 + 1e-5 * scale, (name, what, err_hip, err_cpu32, scale)
    return err_hip, err_cpu32, scale


def exactly_zero(t):
    return bool((t == 0).all())  # (NaN is not zero)


# ---- 1. energies and forces of every case ----------------------------------------------------------------------------------
def _energies_and_forces(name, r):
    assert r["e"].shape == (r["n"],) and (not r["forces"] or r["f"].shape == (r["n"], 3))
    if r["oracle"] is None:  # no atoms / no edges: the per-type shifts (0 for this model) and no force at all
        print(f"{name} exact: {r['n']} atoms, no edges")
        assert exactly_zero(r["e"]) and (not r["forces"] or exactly_zero(r["f"])), (name, r["e"], r["f"])
        return
    check(name, "E", r["e"], *r["oracle"]["e"])
    if r["forces"]:
        check(name, "F", r["f"], *r["oracle"]["f"])


# ---- 2. virial and per-atom virial behind every step -------------------------------------------------------------------------
def _virial_behind_the_step(name, r):
    if not r["forces"]:
        assert r["sized"] < r["sized_for_forces"]
        assert r["w_rc"] == AA_ERR_WORKSPACE and "workspace too small" in r["w_error"], (name, r["w_rc"], r["w_error"])
        return
    n, fp64 = r["n"], r["dtype"] == torch.float64
    assert r["w_rc"] == 0 and r["wc_rc"] == 0, (name, r["w_rc"], r["wc_rc"])
    w = r["w"]
    if r["oracle"] is None:
        assert exactly_zero(w) and exactly_zero(r["wc"]), (name, w)
    else:
        check(name, "W", w, *r["oracle"]["w"])
    # the per-atom tensors: both calls sum the same products in double, so the sum over the atoms is the 3x3 result up to the rounding
    # of the outputs; atoms that are the center (neighbor) of no edge get exact zeros
    sum_tol = (1e-12 if fp64 else 1e-5) * float(w.abs().max())
    per_atom = [("center", r["wc"], r["degree"])]
    if r["tcsr"]:
        assert r["wn_rc"] == 0, (name, r["wn_rc"], r["wn_error"])
        per_atom.append(("neighbor", r["wn"], r["in_degree"]))
    else:
        assert r["wn_rc"] == AA_ERR_INVALID and "transposed CSR" in r["wn_error"], (name, r["wn_rc"], r["wn_error"])
    for which, wa, deg in per_atom:
        assert wa.shape == (n, 3, 3) and torch.isfinite(wa).all(), (name, which)
        err = float((wa.double().sum(0) - w.double()).abs().max()) if n else 0.0
        print(f"{name} sum({which}) - W: {err:.3e}, bound {sum_tol:.3e}")
        assert err <= sum_tol, (name, which, err, sum_tol)
        assert exactly_zero(wa[torch.tensor(deg == 0)]), (name, which)
    # the calls above, the refused one included, left the rows of the step alone
    assert r["w_again_rc"] == 0 and torch.equal(r["w_again"], w), name


def _step_values(backend, case):
    """Sections 1 and 2 behind ONE step of the case (the emulation takes seconds to minutes per step); both are always evaluated."""
    r, failures = measured(backend, case), []
    for section in (_energies_and_forces, _virial_behind_the_step):
        try:
            section(case[0], r)
        except AssertionError as err:
            failures.append(f"{section.__name__}: {err}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_step_values_emulation(case):
    _step_values("emu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_step_values_gpu(case):
    _step_values("gpu", case)


# ---- 3. one plan, one workspace, one set of buffers, changing graphs ---------------------------------------------------------
THREE = dict(type_names=["A", "B", "C"])
# (name, model overrides, plan options): one per way the step is put together
OPTION_SETS = [
    ("default", {}, {}),
    ("fused_narrow2", {}, dict(fused_narrow=2)),
    ("fused_narrow4", {}, dict(fused_narrow=4)),
    ("fused_forward3", {}, dict(fused_forward=3)),
    ("fused_forward4", {}, dict(fused_forward=4)),
    ("slot", {}, dict(gemm_no_chain=1)),
    ("slot_op_proj", {}, dict(gemm_no_chain=1, op_proj_gemm=1)),
    ("operator_chains", {}, dict(tp_force_operator=1)),
    ("general", {}, dict(tp_generic=1)),
    ("l128", L128, {}),
    ("f64", F64, {}),
    ("three_species", THREE, {}),
]
# (graph recipe, forces): the neighbour list changes under the plan; the second MID step is energy only
SEQUENCE = [(MID, True), (LOW12, True), (BLOCK, True), (LONG_ATOM, True), (NO_EDGES, True), (MID, False), (DENSE, True), (MID, True)]
assert max(s[0]["n"] for s in SEQUENCE) <= 200


def _same(name, what, got, fresh_a, fresh_b):
    """Bit-equal to the fresh runs where those are bit-equal to each other (fixed summation order), within FORM_TOL otherwise."""
    assert torch.isfinite(got).all(), (name, what)
    if torch.equal(fresh_a, fresh_b):
        assert torch.equal(got, fresh_a), (name, what, float((got - fresh_a).abs().max()) if got.numel() else 0.0)
    else:
        scale = max(1.0, float(fresh_a.abs().max()))
        err = float((got - fresh_a).abs().max())
        print(f"{name} {what}: fresh runs differ by {float((fresh_a - fresh_b).abs().max()):.3e}; sequence - fresh {err:.3e}, bound {FORM_TOL * scale:.3e}")
        assert err <= FORM_TOL * scale, (name, what, err, scale)


def fresh_step(lib, dev, overrides, options, recipe, forces):
    """(energies, forces | None, virial | None) of one step on a plan, a workspace and buffers of its own."""
    rig = Rig(lib, dev, overrides, options)
    g, p, n, _ = rig.graph(recipe)
    ws = rig.workspace(rig.workspace_bytes(g, forces))
    e, f = rig.outputs(max(n, 1))
    rig.step(g, p, ws, e, f if forces else None)
    w = None
    if forces:
        rc, w = rig.virial(g, ws)
        assert rc == 0, rig.last_error()
    return e[:n].cpu(), f[:n].cpu() if forces else None, w


def run_sequence(backend, option_set):
    name, overrides, options = option_set
    lib, dev = _backend(backend)
    species = len(overrides.get("type_names", BASE["type_names"]))
    recipes = [(dict(recipe, species=species), forces) for recipe, forces in SEQUENCE]
    fresh = {}
    for recipe, forces in recipes:
        key = (repr(sorted(recipe.items())), forces)
        if key not in fresh:
            fresh[key] = (fresh_step(lib, dev, overrides, options, recipe, forces), fresh_step(lib, dev, overrides, options, recipe, forces))
    rig = Rig(lib, dev, overrides, options)
    graphs = [rig.graph(recipe) for recipe, _ in recipes]  # (all alive at once, like the lists of an MD run: no address is reused)
    rows = max(n for _, _, n, _ in graphs)
    ws = rig.workspace(max(rig.workspace_bytes(g, True) for g, _, _, _ in graphs))
    pos = torch.zeros((rows, 3), dtype=rig.dtype, device=dev)
    e, f = rig.outputs(rows)
    for i, ((recipe, forces), (g, p, n, _)) in enumerate(zip(recipes, graphs)):
        (ea, fa, wa), (eb, fb, wb) = fresh[(repr(sorted(recipe.items())), forces)]
        pos[:n] = p[:n]
        step = f"{name} step {i} (n {n}, {g.num_edges} edges, forces {forces})"
        rig.step(g, pos, ws, e, f if forces else None)
        _same(step, "E", e[:n].cpu(), ea, eb)
        if forces:
            _same(step, "F", f[:n].cpu(), fa, fb)
            rc, w = rig.virial(g, ws)
            assert rc == 0, (step, rig.last_error())
            _same(step, "W", w, wa, wb)


SET_NAMES = [s[0] for s in OPTION_SETS]


@pytest.mark.parametrize("option_set", OPTION_SETS, ids=SET_NAMES)
def test_changing_graphs_emulation(option_set):
    run_sequence("emu", option_set)


@pytest.mark.gpu
@pytest.mark.parametrize("option_set", OPTION_SETS, ids=SET_NAMES)
def test_changing_graphs_gpu(option_set):
    run_sequence("gpu", option_set)


# ---- the module itself -------------------------------------------------------------------------------------------------------
def test_no_case_of_the_table_is_left_out(request):
    """The value tests are parametrised over exactly the table: unmarked on the emulation, `gpu` on the device."""
    assert len(NAMES) == len(set(NAMES)) == len(EXPECTED) == len(CASES)
    for test, gpu in ((test_step_values_emulation, False), (test_step_values_gpu, True)):
        marks = {m.name: m for m in test.pytestmark}
        assert ("gpu" in marks) == gpu and set(marks) <= {"gpu", "parametrize"}, test.__name__  # (no skip, no xfail)
        assert list(marks["parametrize"].args[1]) == CASES and list(marks["parametrize"].kwargs["ids"]) == NAMES, test.__name__
        # what was collected, unless a `-k` / node-id selection took part of it (a marker expression takes a whole copy or none)
        ids = [i.name[len(test.__name__) + 1:-1] for i in request.session.items if i.module is request.module and i.name.startswith(test.__name__ + "[")]
        whole = not request.config.option.keyword and not any("::" in a for a in request.config.args)
        assert not (whole and ids) or ids == NAMES, test.__name__
    by_name = {c[0]: c for c in CASES}
    # the virial is refused behind an energy-only step of every pipeline; it is checked behind a force step of every pipeline
    for forces in (False, True):
        reached = set()
        for n, (pipeline, stages) in EXPECTED.items():
            if by_name[n][4].get("forces", True) == forces:
                tp, linear = pipeline.split("/")
                if tp == "per_edge":
                    tp = "general" if "tp_layer_fwd" in stages else "spec_chain" if "tp_chain_fwd_last" in stages else "spec"
                reached.add(f"{tp}/{linear}")
        assert reached >= PIPELINES, (forces, reached)
    assert sum(1 for c in CASES if c[4].get("no_tcsr")) == 3 and sum(1 for c in CASES if c[1] == F64) >= 2
    # the exact cases, and the sequence of section 3
    assert [c[0] for c in CASES if grid_graph(**c[3])[1].shape[1] == 0] == ["no_edges_fused_plan", "empty_block_fused_deep", "empty_block_staged"]
    assert [s[0]["n"] for s in SEQUENCE] == [40, 12, 40, 60, 9, 40, 48, 40] and [s[1] for s in SEQUENCE] == [True] * 5 + [False, True, True]
    assert SEQUENCE[2][0] is BLOCK and SEQUENCE[3][0] is LONG_ATOM and SEQUENCE[4][0] is NO_EDGES and SEQUENCE[6][0] is DENSE
