"""Time of `HipAllegroModel.heat_flux_potential` on a benchmark box, next to the route it took before `aa_model_heat_flux`
existed -- `atom_virial(graph, "neighbor")` (a gather through `t_perm` and an [N,9] write) contracted with the velocities by a
torch einsum.  On a build without the direct kernel the two columns time the same code.  HIP events around batches of calls
after a warm-up, the two routes alternated, the median of several repeats; GB/s of the method on the algorithmic bytes of the
direct form (both [E,4] rows and `nbr` once, the velocities once).

    python tools/heat_flux_bench.py [--workload c4] [--batch 50] [--repeats 7]      ->  one JSON line
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from allegro_amd.nn import HipAllegroModel, PreparedGraph  # noqa: E402


def batch_ms(fn, batch):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(batch):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g, cfg = bench.make_workload(args.workload)
    m = HipAllegroModel(**cfg).to(dev)
    dtype = m.dtype
    es = 4 if dtype == torch.float32 else 8
    pos = torch.tensor(g.pos, dtype=dtype, device=dev)
    sv = g.shift_vec()
    graph = PreparedGraph(torch.tensor(g.edge_index, device=dev), torch.tensor(g.types, device=dev), g.num_atoms,
                          torch.tensor(sv, dtype=dtype, device=dev) if sv is not None else None)
    N, E = graph.num_atoms, graph.num_edges
    m.energy_forces(pos, graph)
    vel = torch.randn(N, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(dtype).to(dev)

    def method():
        return m.heat_flux_potential(graph, vel)

    def gather_route():
        wn = m.atom_virial(graph, "neighbor")
        return -torch.einsum("na,nab->b", vel.to(wn), wn)

    a, b = method(), gather_route()
    scale = max(1.0, float(b.abs().max()))
    res = dict(workload=args.workload, atoms=N, edges=E, dtype=str(dtype).split(".")[-1], batch=args.batch, repeats=args.repeats,
               direct_kernel=hasattr(m._get_lib().lib, "aa_model_heat_flux"),
               max_abs_diff_method_vs_gather_route_over_scale=float((a - b).abs().max()) / scale)
    for fn in (method, gather_route):  # warm-up of both
        for _ in range(args.batch):
            fn()
    torch.cuda.synchronize()
    tm, tg = [], []
    for _ in range(args.repeats):  # alternated, so that both see the same machine state
        tm.append(batch_ms(method, args.batch))
        tg.append(batch_ms(gather_route, args.batch))
    alg = E * (2 * 4 * es + 4) + N * 3 * es
    med_m, med_g = statistics.median(tm), statistics.median(tg)
    res.update(method_us=med_m * 1e3, method_us_min_max=[min(tm) * 1e3, max(tm) * 1e3], gather_route_us=med_g * 1e3,
               gather_route_us_min_max=[min(tg) * 1e3, max(tg) * 1e3], gather_route_over_method=med_g / med_m,
               direct_algorithmic_bytes=alg, method_gbs_on_direct_bytes=alg / (med_m * 1e-3) / 1e9)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
