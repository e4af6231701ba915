"""Batches of small frames: what one batched list + one step + the per-frame kernels cost next to a loop over the frames, what
`forward(data)` with a [B,3,3] cell costs on this tree next to another build of the library's tree (the PARENT commit: the
baseline is never the code under test), and the stream rate of the three `frame_*` calls alone.  Workload: B copies of the C2 box
(64 Si atoms) with seeded jitter, fp32; the lone-workgroup rate is taken at B = 1 on the C3 box.  HIP events around batches of
calls after a warm-up, the two routes alternated, the median of several repeats with min and max.

    python tools/frame_batch_bench.py [--frames 1 16 256] [--repeats 7] [--parent-tree DIR]      ->  one JSON line

(b) runs in child processes (`--forward-child`), one per tree and repeat, alternated; without --parent-tree only this tree is timed.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch_ms(fn, batch):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(batch):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / batch


def stats_us(ms):
    return dict(median_us=statistics.median(ms) * 1e3, min_us=min(ms) * 1e3, max_us=max(ms) * 1e3)


def make_batch(bench, B, dev, dtype):
    """B jittered copies of the C2 box: per-frame positions [B,64,3], the cell, the model configuration."""
    g, cfg = bench.make_workload("c2")
    rng = np.random.default_rng(17)
    pos = np.stack([g.pos + rng.normal(0, 0.01, g.pos.shape) for _ in range(B)])
    return torch.tensor(pos, dtype=dtype, device=dev), np.asarray(g.cell, dtype=np.float64), cfg


def forward_data(nn, pos, cell, r_cut):
    """AtomicDataDict of the batch; the lists come from the per-frame `neighbor_list` (set-up, not timed: exists in either tree)."""
    B, n = pos.shape[0], pos.shape[1]
    ei, cs = [], []
    for b in range(B):
        nl = nn.neighbor_list(pos[b], cell, True, r_cut)
        ei.append(nl.edge_index.long() + b * n)
        cs.append(nl.cell_shift.to(pos.dtype))
    dev = pos.device
    return {"pos": pos.reshape(-1, 3).contiguous(), "edge_index": torch.cat(ei, 1), "atom_types": torch.zeros(B * n, dtype=torch.long, device=dev),
            "cell": torch.tensor(cell, dtype=pos.dtype, device=dev).expand(B, 3, 3).contiguous(), "edge_cell_shift": torch.cat(cs),
            "batch": torch.arange(B, device=dev).repeat_interleave(n)}


def forward_child(args):
    """(b), one tree: median time of `forward(data)` per B, from `--samples` batches each."""
    sys.path.insert(0, args.tree)
    import bench
    from allegro_amd import nn

    assert os.path.realpath(os.path.dirname(os.path.dirname(nn.__file__))) == os.path.realpath(args.tree)
    dev, dtype = torch.device("cuda:0"), torch.float32
    out = {}
    for B in args.frames:
        pos, cell, cfg = make_batch(bench, B, dev, dtype)
        m = nn.HipAllegroModel(**cfg).to(dev)
        data = forward_data(nn, pos, cell, cfg["r_max"])
        calls = max(2, 64 // B)
        for _ in range(calls):
            m(data)
        torch.cuda.synchronize()
        out[str(B)] = [batch_ms(lambda: m(data), calls) for _ in range(args.samples)]
    print("FORWARD_CHILD " + json.dumps(out), flush=True)


def part_b(args):
    trees = {"this": ROOT}
    if args.parent_tree:
        trees["parent"] = os.path.abspath(args.parent_tree)
    ms = {k: {str(B): [] for B in args.frames} for k in trees}
    for _ in range(args.repeats):  # alternated: one child per tree and repeat
        for name, tree in trees.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--forward-child", "--tree", tree, "--samples", "3", "--frames"] + [str(B) for B in args.frames]
            env = dict(os.environ, PYTHONPATH=tree)
            env.pop("ALLEGRO_AMD_LIBRARY", None)
            p = subprocess.run(cmd, check=True, capture_output=True, text=True, env=env, timeout=600)
            line = [l for l in p.stdout.splitlines() if l.startswith("FORWARD_CHILD ")][-1]
            for B, v in json.loads(line[len("FORWARD_CHILD "):]).items():
                ms[name][B].append(statistics.median(v))
    res = {name: {B: stats_us(v) for B, v in per.items()} for name, per in ms.items()}
    if "parent" in res:
        res["parent_over_this"] = {B: res["parent"][B]["median_us"] / res["this"][B]["median_us"] for B in res["this"]}
    return res


def part_a_c(args):
    sys.path.insert(0, ROOT)
    import bench
    from allegro_amd import nn

    dev, dtype, es = torch.device("cuda:0"), torch.float32, 4
    res_a, res_c = {}, {}
    for B in args.frames:
        pos, cell, cfg = make_batch(bench, B, dev, dtype)
        n, r_cut = pos.shape[1], cfg["r_max"]
        m = nn.HipAllegroModel(**cfg).to(dev)
        types = torch.zeros(B * n, dtype=torch.long, device=dev)
        flat = pos.reshape(-1, 3).contiguous()
        cells = torch.tensor(cell, device=dev).expand(B, 3, 3).contiguous()
        frames = nn.Frames(torch.arange(B + 1) * n, device=dev)

        def loop():
            out = []
            for b in range(B):
                g = nn.neighbor_list(pos[b], cell, True, r_cut).prepare(types[:n])
                m.energy_forces(pos[b], g)
                out.append(m.virial(g))
            return torch.stack(out)

        def batched():
            g = nn.neighbor_list_frames(flat, cells, True, r_cut, frames).prepare(types)
            m.energy_forces(flat, g)
            return m.frame_virial(g, frames)

        wl, wb = loop(), batched()
        diff = float((wl - wb).abs().max()) / max(1.0, float(wl.abs().max()))
        calls = max(1, 16 // B)
        for fn in (loop, batched):
            batch_ms(fn, calls)
        tl, tb = [], []
        for _ in range(args.repeats):
            tb.append(batch_ms(batched, calls))
            tl.append(batch_ms(loop, calls))
        res_a[str(B)] = dict(loop=stats_us(tl), batched=stats_us(tb), loop_over_batched=statistics.median(tl) / statistics.median(tb),
                             max_abs_diff_over_scale=diff)
    # (c) the three calls alone: B = 256 copies of C2, and ONE frame holding the C3 box (the lone-workgroup rate)
    for label, B, workload in (("c2_x256", 256, "c2"), ("c3_x1", 1, "c3")):
        if workload == "c2":
            pos, cell, cfg = make_batch(bench, B, dev, dtype)
            n = pos.shape[1]
            flat = pos.reshape(-1, 3).contiguous()
            g = nn.neighbor_list_frames(flat, torch.tensor(cell, device=dev).expand(B, 3, 3).contiguous(), True, cfg["r_max"],
                                        nn.Frames(torch.arange(B + 1) * n, device=dev)).prepare(torch.zeros(B * n, dtype=torch.long, device=dev))
        else:
            gg, cfg = bench.make_workload("c3")
            n = gg.num_atoms
            flat = torch.tensor(gg.pos, dtype=dtype, device=dev)
            g = nn.neighbor_list(flat, gg.cell, True, cfg["r_max"]).prepare(torch.zeros(n, dtype=torch.long, device=dev))
        m = nn.HipAllegroModel(**cfg).to(dev)
        frames = nn.Frames(torch.arange(B + 1) * n, device=dev)
        e_atom, _ = m.energy_forces(flat, g)
        N, E = g.num_atoms, g.num_edges
        vel = torch.randn(N, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(dtype).to(dev)
        fns = dict(frame_energies=(lambda: m.frame_energies(e_atom, frames), N * es + B * es),
                   frame_virial=(lambda: m.frame_virial(g, frames), E * 2 * 4 * es + B * 9 * es),
                   frame_heat_flux=(lambda: m.frame_heat_flux_potential(g, frames, vel), E * (2 * 4 * es + 4) + N * 3 * es + B * 3 * es))
        if B == 1:
            fns["virial_whole_device"] = (lambda: m.virial(g), E * 2 * 4 * es)
        rec = dict(frames=B, atoms=N, edges=E)
        for fn, _ in fns.values():
            batch_ms(fn, 50)
        ts = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, (fn, _) in fns.items():
                ts[k].append(batch_ms(fn, 50))
        for k, (_, nbytes) in fns.items():
            rec[k] = dict(stats_us(ts[k]), algorithmic_bytes=nbytes, gbs=nbytes / (statistics.median(ts[k]) * 1e-3) / 1e9)
        res_c[label] = rec
    return res_a, res_c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit with its library built: the baseline of (b)")
    ap.add_argument("--skip", nargs="*", default=[], choices=["a", "b"])
    ap.add_argument("--forward-child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--samples", type=int, default=3)
    args = ap.parse_args()
    if args.forward_child:
        return forward_child(args)
    res = dict(dtype="float32", repeats=args.repeats, frames=args.frames)
    if "b" not in args.skip:  # (first: its children must not find this process on the device)
        res["b_forward_dict"] = part_b(args)
    if "a" not in args.skip:
        res["a_loop_vs_batched"], res["c_frame_calls_alone"] = part_a_c(args)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
