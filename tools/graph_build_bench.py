"""Wall time of preparing the graph of a foreign edge list: `PreparedGraph(edge_index, ...)` (sortedness check + argsort through the
tensor library, then aa_graph_transpose: two host reads) against `PreparedGraph.from_edge_index(...)` (aa_graph_build_count / _fill:
one host read), on Si boxes of 2 / 11 / 23 cells (the C2 / C3 / C4 list sizes), fp32, center-sorted and randomly permuted input.

    python tools/graph_build_bench.py [--cells 2 11 23]  ->  one JSON line; per case the median of 7 batches with [min, max], in ms"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from allegro_amd import graph as G  # noqa: E402
from allegro_amd.nn import PreparedGraph  # noqa: E402


def batches(fn, reps, warmup=5, n_batches=7):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(n_batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e3)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[2, 11, 23])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for cells in args.cells:
        g = G.make_si_graph(cells)
        N = g.num_atoms
        types = torch.tensor(g.types, device=dev)
        ei0 = torch.tensor(g.edge_index, device=dev)
        sv0 = torch.tensor(g.shift_vec(), dtype=torch.float32, device=dev)
        perm = torch.randperm(ei0.shape[1], generator=torch.Generator().manual_seed(0)).to(dev)
        reps = 50 if cells <= 11 else 10
        for order, ei, sv in (("sorted", ei0, sv0), ("permuted", ei0[:, perm].contiguous(), sv0[perm].contiguous())):
            a = PreparedGraph(ei, types, N, sv)
            b = PreparedGraph.from_edge_index(ei, types, N, sv)
            same = all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("center", "nbr", "rowptr", "t_rowptr", "t_perm", "shift_vec"))
            old = batches(lambda: PreparedGraph(ei, types, N, sv), reps)
            new = batches(lambda: PreparedGraph.from_edge_index(ei, types, N, sv), reps)
            rows.append(dict(atoms=N, edges=int(ei.shape[1]), input=order, same_graph=same, prepared_graph=old, from_edge_index=new,
                             ratio=new["median_ms"] / old["median_ms"]))
    print(json.dumps({"graph_build": rows, "note": "fp32 Si boxes; wall time per call, median of 7 batches [min, max]"}))


if __name__ == "__main__":
    main()
