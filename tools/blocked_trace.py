"""Launch-by-launch account of the block-wise step: kernel time per kernel name of the whole-frame step against the blocked step.

    rocprofv3 --kernel-trace --stats -d DIR/<workload>_B<B> -o t -- python tools/blocked_trace.py run <workload> <B> > DIR/<workload>_B<B>.log
    python tools/blocked_trace.py summarize DIR [--out FILE]

`run` does 3 warm-up and 10 timed steps of the workload -- whole frame (B = 0) or cut into B blocks like tools/blocked_step.py -- and
prints the wall time per step.  `summarize` reads the traces (the rocpd databases `t_results.db`) of every <workload>_B<B> in DIR:
per kernel name the launches and the kernel time per timed step, what else was dispatched inside the timed span, the device's span per
step and its idle part (span minus kernel time), next to the wall time of the same run; prints a table per workload and one JSON.
"""
import glob
import json
import os
import re
import sys
import time

STEPS, WARM = 13, 3


def run(name, B):
    sys.path.insert(0, ".")
    import torch

    import bench
    from allegro_amd.nn import HipAllegroModel, PreparedGraph

    dev = torch.device("cuda:0")
    g, cfg = bench.make_workload(name)
    dtype = {"float32": torch.float32, "float64": torch.float64}[cfg["model_dtype"]]
    pos = torch.tensor(g.pos, dtype=dtype, device=dev)
    m = HipAllegroModel(**cfg).to(dev)
    graph = PreparedGraph(torch.tensor(g.edge_index, device=dev), torch.tensor(g.types, device=dev), g.num_atoms,
                          torch.tensor(g.shift_vec(), dtype=dtype, device=dev))
    if B:
        ba, be = graph.blocks(max(graph.max_degree, -(-graph.num_edges // B)))
        fn = lambda: m.energy_forces_blocks(pos, graph, ba, be)  # noqa: E731
    else:
        fn = lambda: m.energy_forces(pos, graph)  # noqa: E731
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS - WARM):
        fn()
    torch.cuda.synchronize()
    print(f"TRACE_RUN {name} B={B} steps={STEPS} wall_ms_per_step={(time.perf_counter() - t0) / (STEPS - WARM) * 1e3:.3f}", flush=True)


def short(n):
    n = re.sub(r"\(.*", "", n).replace("void ", "").replace("aa::", "").replace("(anonymous namespace)::", "")
    return re.sub(r"<.*", "", n).strip()


def summarize(root, out_path=None):
    import sqlite3

    out = {}
    for d in sorted(glob.glob(os.path.join(root, "*_B*", ""))):
        tag = os.path.basename(d.rstrip("/"))
        rows = sqlite3.connect(os.path.join(d, "t_results.db")).execute("select name, start, end from kernels order by start").fetchall()
        by = {}
        for n, s, e in rows:
            by.setdefault(short(n), []).append((s, e))
        # the step's own kernels: launched the same number of times in every one of the STEPS steps (setup kernels are not)
        step = {k: v for k, v in by.items() if len(v) % STEPS == 0 and not k.startswith("__amd") and "at::" not in k and "elementwise" not in k}
        per, t0, t1 = {}, None, 0
        for k, v in step.items():
            n = len(v) // STEPS
            timed = v[WARM * n:]
            per[k] = dict(launches=n, us=sum(e - s for s, e in timed) / (STEPS - WARM) / 1e3)
            t0 = timed[0][0] if t0 is None else min(t0, timed[0][0])
            t1 = max(t1, timed[-1][1])
        inside = [(short(n), s, e) for n, s, e in rows if s >= t0 and e <= t1]
        other = {}
        for n, s, e in inside:
            if n not in step:
                o = other.setdefault(n, [0, 0.0])
                o[0] += 1
                o[1] += e - s
        for n, (cnt, ns) in other.items():
            per["(other) " + n] = dict(launches=cnt / (STEPS - WARM), us=ns / (STEPS - WARM) / 1e3)
        busy = sum(e - s for _, s, e in inside) / (STEPS - WARM) / 1e3
        span = (t1 - t0) / (STEPS - WARM) / 1e3
        wall = float(re.search(r"wall_ms_per_step=([\d.]+)", open(os.path.join(root, tag + ".log")).read()).group(1))
        out[tag] = dict(workload=tag.split("_B")[0], blocks_requested=int(tag.split("_B")[1]), wall_ms_per_step=wall,
                        device_span_us_per_step=span, kernel_us_per_step=busy, idle_us_per_step=span - busy,
                        launches_per_step=sum(p["launches"] for p in per.values()), kernels=per)
    for wl in sorted({v["workload"] for v in out.values()}):
        tags = sorted((t for t in out if out[t]["workload"] == wl), key=lambda t: out[t]["blocks_requested"])
        names = sorted({k for t in tags for k in out[t]["kernels"]}, key=lambda k: -max(out[t]["kernels"].get(k, {"us": 0})["us"] for t in tags))
        print("%-30s" % (wl + ": us per step (launches)"), *["%17s" % t for t in tags])
        for k in names:
            print("%-30s" % k[:30], *["%9.1f (%5.1f)" % (out[t]["kernels"].get(k, {"us": 0})["us"], out[t]["kernels"].get(k, {"launches": 0})["launches"])
                                      for t in tags])
        for f in ("kernel_us_per_step", "idle_us_per_step", "device_span_us_per_step", "launches_per_step"):
            print("%-30s" % f, *["%17.1f" % out[t][f] for t in tags])
        print("%-30s" % "wall_ms_per_step", *["%17.3f" % out[t]["wall_ms_per_step"] for t in tags])
    line = json.dumps(dict(tool="blocked_trace", steps=STEPS, warmup=WARM, runs=out))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return out


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run":
        run(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) >= 3 and sys.argv[1] == "summarize":
        summarize(sys.argv[2], sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None)
    else:
        sys.exit(__doc__)
