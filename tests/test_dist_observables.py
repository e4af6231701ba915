"""Observables of the sharded step (`energy_forces_halo(..., virial=, atom_virial=, velocities_own=)`, `InProcessHaloGroup.step`):
the strain derivative and the potential heat flux of the whole frame (one all-reduce of 9 + 3 numbers), the per-atom virial of the
owned atoms (ghost rows [n_ghost,9] sent home by one more reverse communication, added in the fixed order of the forces).

Reference: the one-process step on the whole frame -- `model.virial`, `model.atom_virial` (three attributions),
`model.heat_flux_potential` -- within the project's tolerance, 1e-9 (fp64) / 5e-5 (fp32) times max(1, max |expected|).
The 64-atom Si cell `c2` (1 792 edges): at five slabs a slab is thinner than the cutoff, owned atoms are ghosts on several ranks and
the accumulation table has rows of multiplicity > 1.

Emulated kernels in one process and under gloo (two and five ranks, the real collectives, counted); `gpu`: the device library.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {torch.float64: 1e-9, torch.float32: 5e-5}
DTYPES = [pytest.param(torch.float64, id="f64"), pytest.param(torch.float32, id="f32")]
ATTRIBUTIONS = ("center", "neighbor", "split")
CELL = np.eye(3) * (2 * 5.431)


def close(name, got, want, dtype):
    want = want.double()
    scale = max(1.0, float(want.abs().max()))
    err = float((got.double().to(want.device) - want).abs().max())
    print(f"{name}: max|got - expected| = {err:.3e}, bound {TOL[dtype] * scale:.3e} (max|expected| {float(want.abs().max()):.3e})")
    assert err <= TOL[dtype] * scale, name


def frame_velocities(n, dtype):
    return torch.randn(n, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(17)).to(dtype)


_WHOLE = {}


def whole_frame(backend, dtype):
    """c2 in `dtype`: (fixture, model, velocities [n,3], reference dict) -- ONE step on the whole frame and everything read off it, computed
    once and shared (the tests below only read it)."""
    if (backend, dtype) not in _WHOLE:
        from tests.golden_utils import load_model_fixture
        from tests.hip_utils import emu_lib, fixture_data, model_from_fixture

        dev = torch.device("cpu" if backend == "emu" else "cuda:0")
        fx = load_model_fixture("c2", dtype)
        m = model_from_fixture(fx, dtype, emu_lib() if backend == "emu" else None, dev)
        data, sv = fixture_data(fx, dtype, dev)
        n = data["pos"].shape[0]
        g = m.prepare_graph(data["edge_index"], data["atom_types"], n, sv)
        vel = frame_velocities(n, dtype).to(dev)
        e, f = m.energy_forces(data["pos"], g)
        ref = dict(e=e.clone(), f=f.clone(), virial=m.virial(g).clone(), heat_flux=m.heat_flux_potential(g, vel).clone())
        for a in ATTRIBUTIONS:
            ref[a] = m.atom_virial(g, a).clone()
        assert float(ref["virial"].abs().max()) > 1e-3 and float(ref["heat_flux"].abs().max()) > 1e-3
        assert float((ref["center"] - ref["neighbor"]).abs().max()) > 1e-3
        _WHOLE[(backend, dtype)] = (fx, m, vel, ref)
    return _WHOLE[(backend, dtype)]


def group_case(backend, dtype, world):
    from allegro_amd.dist import InProcessHaloGroup

    fx, m, vel, ref = whole_frame(backend, dtype)
    dev = vel.device
    lib = None
    if backend == "emu":
        from tests.hip_utils import emu_lib

        lib = emu_lib()
    pos = fx["pos"].to(dev)
    n = pos.shape[0]
    grp = InProcessHaloGroup.from_positions(pos, fx["types"].to(dev), CELL, float(fx["cfg"]["r_max"]), world, lib=lib)
    if world == 5:  # slabs thinner than the cutoff: an owned atom is a ghost on several ranks
        assert max(int(s._rows.shape[1]) for s in grp.shards if s._rows is not None) > 1
    own = [s.owned_ids() for s in grp.shards]

    def step(shift, attribution):
        return grp.step(m, [pos[i] + shift for i in own], virial=True, atom_virial=attribution, velocities_own_list=[vel[i] for i in own])

    first = step(0.0, "neighbor")
    assert all(len(r) == 3 and sorted(r[2]) == ["atom_virial", "heat_flux", "virial"] for r in first)
    e_all, f_all = torch.empty(n, dtype=dtype, device=dev), torch.empty(n, 3, dtype=dtype, device=dev)
    w_all = torch.empty(n, 3, 3, dtype=dtype, device=dev)
    for i, (e, f, obs) in zip(own, first):
        e_all[i], f_all[i], w_all[i] = e, f, obs["atom_virial"]
        assert obs["virial"].shape == (3, 3) and obs["heat_flux"].shape == (3,) and obs["atom_virial"].shape == (i.numel(), 3, 3)
        assert obs["virial"].dtype == dtype and obs["heat_flux"].dtype == dtype and obs["atom_virial"].dtype == dtype
        assert torch.equal(obs["virial"], first[0][2]["virial"]) and torch.equal(obs["heat_flux"], first[0][2]["heat_flux"])
    what = f"W={world}"
    close(f"{what} E_i", e_all, ref["e"], dtype)
    close(f"{what} F", f_all, ref["f"], dtype)
    close(f"{what} virial", first[0][2]["virial"], ref["virial"], dtype)
    close(f"{what} heat flux", first[0][2]["heat_flux"], ref["heat_flux"], dtype)
    close(f"{what} atom virial, neighbor", w_all, ref["neighbor"], dtype)
    # other positions and back: the persistent buffers of both widths are reused, nothing of the step in between is left in them
    ptr = [(s.reverse_buffer(9, dtype, dev).data_ptr(), s.reverse_buffer(3, dtype, dev).data_ptr()) for s in grp.shards]
    step(0.01, "split")
    again = step(0.0, "split")
    assert ptr == [(s.reverse_buffer(9, dtype, dev).data_ptr(), s.reverse_buffer(3, dtype, dev).data_ptr()) for s in grp.shards]
    for i, (e0, f0, o0), (e1, f1, o1) in zip(own, first, again):
        assert torch.equal(e0, e1) and torch.equal(f0, f1)
        assert torch.equal(o0["virial"], o1["virial"]) and torch.equal(o0["heat_flux"], o1["heat_flux"])
        w_all[i] = o1["atom_virial"]
    close(f"{what} atom virial, split", w_all, ref["split"], dtype)
    # the center attribution, alone: nothing else is returned, nothing is communicated for it
    res = grp.step(m, [pos[i] for i in own], atom_virial="center")
    assert all(sorted(r[2]) == ["atom_virial"] for r in res)
    for i, (_, _, obs) in zip(own, res):
        w_all[i] = obs["atom_virial"]
    close(f"{what} atom virial, center", w_all, ref["center"], dtype)
    with pytest.raises(ValueError, match="atom_virial"):
        grp.step(m, [pos[i] for i in own], atom_virial="pairwise")


@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_in_process_group_matches_the_whole_frame_emu(dtype, world):
    group_case("emu", dtype, world)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_in_process_group_matches_the_whole_frame_gpu(dtype, world):
    group_case("gpu", dtype, world)


def test_observables_are_accepted_by_one_unconnected_shard():
    """`energy_forces_halo(..., virial=True)` on the one shard of a one-rank job (no process group, no collective): the frame's own values."""
    from allegro_amd.dist import HaloShard, energy_forces_halo
    from tests.hip_utils import emu_lib

    dtype = torch.float32
    fx, m, vel, ref = whole_frame("emu", dtype)
    sh = HaloShard.from_positions(fx["pos"], fx["types"], CELL, float(fx["cfg"]["r_max"]), 0, 1, lib=emu_lib(), connect=False)
    ids = sh.owned_ids()
    assert sh.n_ghost == 0 and not sh.connected
    e, f, obs = energy_forces_halo(m, fx["pos"][ids].contiguous(), sh, virial=True, atom_virial="split", velocities_own=vel[ids])
    close("one shard: virial", obs["virial"], ref["virial"], dtype)
    close("one shard: heat flux", obs["heat_flux"], ref["heat_flux"], dtype)
    w = torch.empty_like(ref["split"])
    w[ids] = obs["atom_virial"]
    close("one shard: atom virial, split", w, ref["split"], dtype)
    assert len(energy_forces_halo(m, fx["pos"][ids].contiguous(), sh)) == 2
    with pytest.raises(ValueError, match="velocities_own"):
        energy_forces_halo(m, fx["pos"][ids].contiguous(), sh, velocities_own=vel[:5])


# ---------------------------------------------------------------------------------------------------------------------
# the real collectives
# ---------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q, mode, device):
    """HaloShard + energy_forces_halo with all three observables under gloo (`_worker_halo` of tests/test_dist_gloo.py);
    `device` "cpu": emulated kernels; "cuda:0": every rank on the one device, rows staged through the host."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from allegro_amd.dist import HaloShard, energy_forces_halo
    from tests.golden_utils import load_model_fixture
    from tests.hip_utils import emu_lib, model_from_fixture

    dtype = torch.float32
    dev = torch.device(device)
    lib = emu_lib() if dev.type == "cpu" else None
    fx = load_model_fixture("c2", dtype)
    m = model_from_fixture(fx, dtype, lib, dev)
    pos, types = fx["pos"].to(dev), fx["types"].to(dev)
    n = pos.shape[0]
    r_max = float(fx["cfg"]["r_max"])
    if mode == "owned":  # a domain-decomposed host: every rank is handed ONLY the atoms of its slab (unequal counts)
        bounds = [0.0] + [min(0.97, (k + 0.37) / world) for k in range(1, world)] + [1.0]
        fxx = torch.remainder(pos[:, 0].double() / (2 * 5.431), 1.0)
        ids = torch.nonzero((fxx >= bounds[rank]) & (fxx < bounds[rank + 1])).reshape(-1)
        sh = HaloShard.from_owned(pos[ids].contiguous(), types[ids], CELL, r_max, rank, world, bounds=bounds, lib=lib)
    else:
        sh = HaloShard.from_positions(pos, types, CELL, r_max, rank, world, lib=lib)
        ids = sh.owned_ids()
    assert sh.connected and sh.host_staged == (dev.type == "cuda")
    pos_own = pos[ids].contiguous()
    vel = frame_velocities(n, dtype).to(dev)
    vel_own = vel[ids].contiguous()
    calls = {"a2a": 0, "ar": 0}
    orig_a2a, orig_ar = dist.all_to_all_single, dist.all_reduce
    dist.all_to_all_single = lambda *a, **k: (calls.__setitem__("a2a", calls["a2a"] + 1), orig_a2a(*a, **k))[1]
    dist.all_reduce = lambda *a, **k: (calls.__setitem__("ar", calls["ar"] + 1), orig_ar(*a, **k))[1]
    try:
        plain = energy_forces_halo(m, pos_own + 0.01, sh)
        assert len(plain) == 2 and (calls["a2a"], calls["ar"]) == (2, 0), calls  # as before: forward + reverse, nothing else
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
    parts = [None] * world
    dist.all_gather_object(parts, dict(ids=ids.cpu(), e=e.cpu(), f=f.cpu(), virial=obs["virial"].cpu(), heat_flux=obs["heat_flux"].cpu(),
                                       neighbor=obs["atom_virial"].cpu(), center=obs_c["atom_virial"].cpu(), split=obs_s["atom_virial"].cpu(),
                                       mult=0 if sh._rows is None else int(sh._rows.shape[1])))
    if rank == 0:
        got = dict(e=torch.zeros(n), f=torch.zeros(n, 3), **{a: torch.zeros(n, 3, 3) for a in ATTRIBUTIONS})
        for p in parts:
            for k in got:
                got[k][p["ids"]] = p[k]
        # (numpy arrays: pickled by value.  A tensor on a multiprocessing queue travels as a handle to shared memory that the
        #  receiver has to fetch from THIS process, which may have left by then)
        q.put(dict({k: v.numpy() for k, v in got.items()}, virial=[p["virial"].numpy() for p in parts],
                   heat_flux=[p["heat_flux"].numpy() for p in parts], mult=max(p["mult"] for p in parts),
                   atoms=sum(int(p["ids"].numel()) for p in parts)))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    """A port nobody listens on right now, from the kernel (the suite runs several rendezvous at a time on xdist workers)."""
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(world, mode, device):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, mode, device)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    as_tensor = lambda v: [torch.from_numpy(x) for x in v] if isinstance(v, list) else torch.from_numpy(v)  # noqa: E731
    return {k: (v if isinstance(v, int) else as_tensor(v)) for k, v in got.items()}


def _compare_ranks(got, ref, dtype, what):
    assert got["atoms"] == ref["e"].shape[0]
    close(f"{what} E_i", got["e"], ref["e"].cpu(), dtype)
    close(f"{what} F", got["f"], ref["f"].cpu(), dtype)
    for a in ATTRIBUTIONS:
        close(f"{what} atom virial, {a}", got[a], ref[a].cpu(), dtype)
    close(f"{what} virial", got["virial"][0], ref["virial"].cpu(), dtype)
    close(f"{what} heat flux", got["heat_flux"][0], ref["heat_flux"].cpu(), dtype)
    for v, j in zip(got["virial"], got["heat_flux"]):  # the same on every rank
        assert torch.equal(v, got["virial"][0]) and torch.equal(j, got["heat_flux"][0])


@pytest.mark.parametrize("world,mode", [(2, "positions"), (5, "positions"), (2, "owned"), (5, "owned")])
def test_gloo_ranks_through_energy_forces_halo(world, mode):
    _, _, _, ref = whole_frame("emu", torch.float32)
    got = _run_ranks(world, mode, "cpu")
    if world == 5:
        assert got["mult"] > 1
    _compare_ranks(got, ref, torch.float32, f"gloo W={world} ({mode})")


@pytest.mark.gpu
def test_two_ranks_on_one_device_through_energy_forces_halo():
    _, _, _, ref = whole_frame("gpu", torch.float32)
    got = _run_ranks(2, "positions", "cuda:0")
    _compare_ranks(got, ref, torch.float32, "2 ranks on cuda:0")
