"""Step time of a two-species model on the full device neighbour list and on the typed one (per-type-pair cutoffs applied by the
list, `HipAllegroModel.neighbor_list`), same box, same weights: what the per_edge_type_cutoff knob buys once the list honours it.

Water-like box (types O = 0, H = 1), cutoffs O-O 5.0 / O-H 4.0 / H-H 3.0, u = S = 64, l_max 2, 2 layers, fp32.  HIP events around
batches of steps after a warm-up, the two lists alternated, the median of several repeats; the time of building each list next to it.

    python tools/typed_list_bench.py [--side 14] [--batch 20] [--repeats 7]      ->  one JSON line
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allegro_amd import graph as G  # noqa: E402
from allegro_amd.nn import HipAllegroModel, neighbor_list  # noqa: E402


def timed(fn, batch, repeats):
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=14, help="molecules per box edge (3 side^3 atoms, at the density of bench.py's water box)")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    box = 66.9 / 21.544 * args.side
    pos_h, cell, types_h = G.water_box(args.side, box)
    cfg = dict(type_names=["O", "H"], r_max=5.0, l_max=2, num_layers=2, num_scalar_features=64, num_tensor_features=64,
               per_edge_type_cutoff={"O": {"O": 5.0, "H": 4.0}, "H": {"O": 4.0, "H": 3.0}}, avg_num_neighbors=40.0, seed=1,
               model_dtype="float32")
    m = HipAllegroModel(**cfg).to(dev)
    pos = torch.tensor(pos_h, dtype=torch.float32, device=dev)
    types = torch.tensor(types_h, dtype=torch.int64, device=dev)
    lists = {"full": lambda: neighbor_list(pos, cell, True, 5.0), "typed": lambda: m.neighbor_list(pos, cell, True, types)}
    graphs = {k: f().prepare(types) for k, f in lists.items()}
    out = {k: tuple(x.clone() for x in m.energy_forces(pos, g)) for k, g in graphs.items()}
    scale = max(1.0, float(out["full"][1].abs().max()))
    res = dict(atoms=int(pos.shape[0]), side=args.side, box=box, batch=args.batch, repeats=args.repeats, plan=m.describe_plan(),
               edges={k: g.num_edges for k, g in graphs.items()},
               max_abs_force_diff_over_scale=float((out["typed"][1] - out["full"][1]).abs().max()) / scale)
    res["edge_ratio"] = res["edges"]["typed"] / res["edges"]["full"]
    steps = {k: [] for k in graphs}
    for _ in range(args.repeats):  # alternate, so that both lists see the same machine state
        for k, g in graphs.items():
            steps[k] += timed(lambda: m.energy_forces(pos, g), args.batch, 1)
    res["step_ms"] = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in steps.items()}
    res["step_ratio"] = res["step_ms"]["typed"]["median"] / res["step_ms"]["full"]["median"]
    res["list_ms"] = {k: statistics.median(timed(f, 5, args.repeats)) for k, f in lists.items()}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
