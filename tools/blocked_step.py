"""Block-wise step against the whole-frame step on one bench workload.

    python tools/blocked_step.py [workload] [B ...]      (default: c4, B = 2 4 8 16)

Prints the whole-frame step time and workspace bytes, then per B the blocked step (the frame cut greedily into blocks of at most
ceil(E / B) edges: `PreparedGraph.blocks`) with its time, its workspace bytes and max |dE_i| / max |dF| against the whole-frame
step, and ONE JSON line with all of it.  `--whole-only`: the whole-frame step alone (a baseline build without the blocked entry
points).  `--out FILE`: the JSON line is also written there.
"""
import json
import sys
import time

sys.path.insert(0, ".")
import torch  # noqa: E402

import bench  # noqa: E402
from allegro_amd.nn import HipAllegroModel, PreparedGraph  # noqa: E402


def timeit(fn, n, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path in args:
        args.remove(out_path)
    whole_only = "--whole-only" in sys.argv
    name = args[0] if args and not args[0].isdigit() else "c4"
    Bs = [int(a) for a in args if a.isdigit()] or [2, 4, 8, 16]
    dev = torch.device("cuda:0")
    g, cfg = bench.make_workload(name)
    dtype = {"float32": torch.float32, "float64": torch.float64}[cfg["model_dtype"]]
    N = g.num_atoms
    pos = torch.tensor(g.pos, dtype=dtype, device=dev)
    model = HipAllegroModel(**cfg).to(dev)
    graph = PreparedGraph(torch.tensor(g.edge_index, device=dev), torch.tensor(g.types, device=dev), N,
                          torch.tensor(g.shift_vec(), dtype=dtype, device=dev))
    E = graph.num_edges
    lib = model._get_lib().lib
    reps = 20 if E > 1_000_000 else 50
    e_ref, f_ref = (t.clone() for t in model.energy_forces(pos, graph))
    ws_whole = lib.aa_model_workspace_bytes(model._plan_handle, N, E, 1)
    t_whole = timeit(lambda: model.energy_forces(pos, graph), reps)
    print(f"{name}: N={N} E={E}  whole frame {t_whole:.3f} ms, workspace {ws_whole / 1e9:.3f} GB", flush=True)
    result = dict(tool="blocked_step", workload=name, atoms=N, edges=E, dtype=cfg["model_dtype"], device=torch.cuda.get_device_name(0),
                  whole=dict(ms_per_step=t_whole, workspace_bytes=ws_whole), blocked=[])
    for B in ([] if whole_only else Bs):
        model._workspace = None  # (the arena is re-sized for this cap: the figure below is what a host would allocate)
        torch.cuda.empty_cache()
        cap = max(graph.max_degree, -(-E // B))
        ba, be = graph.blocks(cap)
        largest = int((be[1:] - be[:-1]).max())
        ws = lib.aa_model_blocked_workspace_bytes(model._plan_handle, N, E, largest, 1)
        e, f = model.energy_forces_blocks(pos, graph, ba, be)
        model.check()
        de, df = float((e - e_ref).abs().max()), float((f - f_ref).abs().max())
        t = timeit(lambda: model.energy_forces_blocks(pos, graph, ba, be), reps)
        print(f"  B={B}: {len(ba) - 1} blocks of <= {cap} edges (largest {largest}): {t:.3f} ms ({t / t_whole:.3f} x whole), workspace "
              f"{ws / 1e9:.3f} GB ({ws / ws_whole:.3f} x whole); max|dE_i| {de:.2e} max|dF| {df:.2e}", flush=True)
        result["blocked"].append(dict(B=B, blocks=len(ba) - 1, max_block_edges=largest, ms_per_step=t, ratio_to_whole=t / t_whole,
                                      workspace_bytes=ws, max_abs_dE=de, max_abs_dF=df))
    line = json.dumps(result)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
