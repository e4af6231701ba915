"""Time of `aa_model_atom_virial` (center / neighbor / split) on a benchmark box, next to the route a host had to take without
it -- `debug_tap("dvec")`, `debug_tap("vec")`, the [E,3,3] outer products and an `index_add_` per attribution -- and next to
`force_gather` of the profiled step of the same build.  HIP events around batches of calls after a warm-up, the median of several
repeats; GB/s on the algorithmic bytes (every [E,4] row the attribution must read once, `t_perm`, the row pointers, the [N,9] output).

    python tools/atom_virial_bench.py [--workload c4] [--batch 50] [--repeats 7]      ->  one JSON line
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from allegro_amd.nn import HipAllegroModel, PreparedGraph  # noqa: E402

ATTRIBUTIONS = ("center", "neighbor", "split")


def timed(fn, batch, repeats):
    """Median and spread [ms per call] of `repeats` batches of `batch` calls."""
    for _ in range(batch):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(batch):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / batch)
    return statistics.median(out), min(out), max(out)


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
    lib = m._get_lib()
    gs = graph.c_struct()
    out = torch.empty((N, 3, 3), dtype=dtype, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def kernel(code):
        lib.check(lib.lib.aa_model_atom_virial(m._plan_handle, C.byref(gs), m._workspace.data_ptr(), m._workspace.numel(), code,
                                               out.data_ptr(), stream), "aa_model_atom_virial")

    center, nbr = graph.center.long(), graph.nbr.long()

    def tap_route(attribution):
        d = m.debug_tap("dvec", graph, with_forces=True)[:, :3]
        v = m.debug_tap("vec", graph, with_forces=True)
        outer = d.unsqueeze(2) * (v[:, :3] * v[:, 3:4]).unsqueeze(1)
        w = torch.zeros(N, 3, 3, dtype=dtype, device=dev)
        if attribution != "neighbor":
            w.index_add_(0, center, outer)
        if attribution != "center":
            w.index_add_(0, nbr, outer)
        return w * 0.5 if attribution == "split" else w

    row = 4 * es  # one [E,4] row
    alg_bytes = {"center": E * 2 * row + N * (9 * es + 4), "neighbor": E * (2 * row + 4) + N * (9 * es + 4),
                 "split": E * (4 * row + 4) + N * (9 * es + 8)}
    res = dict(workload=args.workload, atoms=N, edges=E, dtype=str(dtype).split(".")[-1], batch=args.batch, repeats=args.repeats,
               plan=m.describe_plan())
    for code, a in enumerate(ATTRIBUTIONS):
        # the two routes agree at this size (fp32 atomics against fixed-order double sums: to rounding)
        kernel(code)
        ref = tap_route(a)
        scale = max(1.0, float(ref.abs().max()))
        res[f"{a}_max_abs_diff_vs_tap_route_over_scale"] = float((out - ref).abs().max()) / scale
        del ref
    # alternate the two routes of each attribution, so that both see the same machine state
    for code, a in enumerate(ATTRIBUTIONS):
        k = timed(lambda: kernel(code), args.batch, args.repeats)
        t = timed(lambda: tap_route(a), max(2, args.batch // 10), args.repeats)
        res[a] = dict(kernel_us=k[0] * 1e3, kernel_us_min_max=[k[1] * 1e3, k[2] * 1e3], algorithmic_bytes=alg_bytes[a],
                      kernel_gbs=alg_bytes[a] / (k[0] * 1e-3) / 1e9, tap_route_us=t[0] * 1e3, tap_route_us_min_max=[t[1] * 1e3, t[2] * 1e3],
                      speedup=t[0] / k[0])
    stages = bench.profile_stages(m, pos, graph, reps=5)
    res["step_stages_us"] = {nm: ms * 1e3 for nm, ms, _, _ in stages if nm in ("force_gather", "edge_backward", "pair_zbl")}
    res["step_total_us"] = sum(ms for _, ms, _, _ in stages) * 1e3
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
