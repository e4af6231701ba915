#!/usr/bin/env python
"""Benchmark of the Allegro hot path (forward + forces) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c4|c3|c2|c5] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints one JSON line (metric, value, ms_per_step, ...).  `--full` adds
everything else the line can carry, each part measured after the timed steps: the sustained run, the per-launch HIP-event
profile and rooflines, the device neighbour list, the MD loop, the CPU and GPU baselines of the oracle port with the parity
sample, and the secondary C3 / C5 records.  `--dump-outputs DIR` writes what the last timed step computed (atomic_energy.npy,
forces.npy) for output-for-output comparisons of two builds; the inputs are the same from run to run.

A "step" is one pass of the hot path (energies + forces of every atom) over one synthetic periodic
box held resident in HBM; the neighbor list / CSR build is outside the timed region.
Metric (BASELINE.json): edge tensor-products/s = E * L / t_step; ns/day = 0.0864 / t_step[s] at 1 fs.
Default workload: C4, the 10^5-atom bulk-Si box of the metric (97 336 atoms, 2 725 408 directed edges,
l_max=2, 2 layers, 64 features, fp32).  With --gpus N > 1 the SAME box is atom-block decomposed over N
ranks (strong scaling): every rank holds its slab's positions and neighbour list only; per step one forward and one
reverse communication of ghost rows (two RCCL all_to_all_single; allegro_amd/dist.py: energy_forces_halo).
`--dist-mode allreduce` keeps the round-3 form (replicated positions, one all-reduce of the force array).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from allegro_amd import graph as G  # noqa: E402
from allegro_amd.dist import HaloShard, LocalShard, energy_forces_halo, energy_forces_local  # noqa: E402
from allegro_amd.nn import HipAllegroModel, PreparedGraph  # noqa: E402

BESSEL = {"_target_": "allegro.nn.TwoBodyBesselScalarEmbed", "num_bessels": 8, "polynomial_cutoff_p": 6}
PEAK_F32_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32 MFMA = fp32 vector peak
PEAK_F64_TFLOPS = 78.6
PEAK_HBM_GBS = 8000.0
BOOST_CLOCK_GHZ, SUSTAINED_CLOCK_GHZ = 2.4, 2.1  # the guide's peaks assume 2.4 GHz; rocm-smi during the C4 loop: 2.09-2.14 GHz at ~1250 W


def si_model_cfg(avg_nn=28.0):
    return dict(type_names=["Si"], r_max=5.0, l_max=2, parity=True, num_layers=2, num_scalar_features=64,
                num_tensor_features=64, radial_chemical_embed=dict(BESSEL), radial_chemical_embed_dim=64,
                scalar_embed_mlp_hidden_layers_depth=1, scalar_embed_mlp_hidden_layers_width=64,
                allegro_mlp_hidden_layers_depth=1, allegro_mlp_hidden_layers_width=64,
                readout_mlp_hidden_layers_depth=1, readout_mlp_hidden_layers_width=64, avg_num_neighbors=avg_nn,
                tp_path_channel_coupling=True, seed=456)


def water_model_cfg(avg_nn):
    return dict(type_names=["O", "H"], r_max=5.0, l_max=3, parity=True, num_layers=3, num_scalar_features=128,
                num_tensor_features=128, radial_chemical_embed=dict(BESSEL), radial_chemical_embed_dim=128,
                scalar_embed_mlp_hidden_layers_depth=1, scalar_embed_mlp_hidden_layers_width=128,
                allegro_mlp_hidden_layers_depth=1, allegro_mlp_hidden_layers_width=128,
                readout_mlp_hidden_layers_depth=1, readout_mlp_hidden_layers_width=128, avg_num_neighbors=avg_nn,
                tp_path_channel_coupling=True, seed=456)


WORKLOADS = {
    # BASELINE config 0 (configs/tutorial.yaml hyper-parameters on the 64-atom Si cell: l_max=1, 2 layers, 32 tensor features)
    "c1": dict(kind="si", cells=2, dtype="float32", l_max=1, u=32, desc="Si 2^3 cells (64 atoms), l_max=1, L=2, u=32 (tutorial.yaml)"),
    "c2": dict(kind="si", cells=2, dtype="float32", desc="Si 2^3 cells (64 atoms), l_max=2, L=2, u=64"),
    "c3": dict(kind="si", cells=11, dtype="float32", desc="bulk Si 11^3 cells (10 648 atoms), r_cut 5 A, l_max=2, L=2, u=64"),
    "c4": dict(kind="si", cells=23, dtype="float32", desc="bulk Si 23^3 cells (97 336 atoms), r_cut 5 A, l_max=2, L=2, u=64"),
    # 22^3 molecules at the density of BASELINE's "3x10^4-atom" box: 31 944 atoms, ~1.72e6 edges (the exact counts
    # of the generated graph are in config.atoms / config.edges of the line)
    "c5": dict(kind="water", side=22, box=66.9 * 22 / 21.544, dtype="float64",
               desc="water box 22^3 molecules (31 944 atoms, ~1.72e6 edges, 2 species), r_cut 5 A, l_max=3, L=3, u=128, fp64"),
}


def make_workload(name):
    w = WORKLOADS[name]
    if w["kind"] == "si":
        rcut = float(os.environ.get("AA_BENCH_RCUT", "5.0"))  # (experiments only: denser neighbor lists, e.g. 6.5 -> ~60 edges per atom)
        g = G.make_si_graph(int(os.environ.get("AA_BENCH_CELLS", w["cells"])), r_cut=rcut)  # (AA_BENCH_CELLS: size sweeps, experiments only)
        cfg = si_model_cfg(g.num_edges / g.num_atoms)
        cfg["r_max"] = rcut
        cfg["l_max"] = w.get("l_max", cfg["l_max"])
        cfg["num_tensor_features"] = w.get("u", cfg["num_tensor_features"])
        if os.environ.get("AA_BENCH_LMAX"):  # experiments only: the same box and widths at another l_max
            cfg["l_max"] = int(os.environ["AA_BENCH_LMAX"])
        if os.environ.get("AA_BENCH_CFG"):  # experiments only: JSON overrides of the model constructor arguments
            cfg.update(json.loads(os.environ["AA_BENCH_CFG"]))
        if os.environ.get("AA_BENCH_U"):  # experiments only
            cfg["num_tensor_features"] = int(os.environ["AA_BENCH_U"])
        if os.environ.get("AA_BENCH_LAYERS"):  # experiments only
            cfg["num_layers"] = int(os.environ["AA_BENCH_LAYERS"])
    else:
        g = G.make_water_graph(w["side"], w["box"])
        cfg = water_model_cfg(g.num_edges / g.num_atoms)
    cfg["model_dtype"] = os.environ.get("AA_BENCH_DTYPE", w["dtype"])  # (AA_BENCH_DTYPE: experiments only, e.g. C5's shapes in fp32)
    return g, cfg


def step_roofline(cfg, E, t_step, stages, dtype):
    """Whole-step figures of SURVEY.md section 8(d).  (1) fully-fused compute bound: algorithmic forward+force flops
    per edge (GEMM part on the fp32/fp64 MFMA peak, CG/SH/segment-sum part on the vector peak); (2) the HBM time of
    THIS stage-materialised design: sum of the algorithmic bytes of all launches at 8 TB/s."""
    S, u, L, l_max = cfg["num_scalar_features"], cfg["num_tensor_features"], cfg["num_layers"], cfg["l_max"]
    B = cfg["radial_chemical_embed"].get("num_bessels", 8)
    S0 = cfg.get("radial_chemical_embed_dim", S)
    Hs = cfg.get("scalar_embed_mlp_hidden_layers_width", S)
    Ha = cfg.get("allegro_mlp_hidden_layers_width", S)
    Hr = cfg.get("readout_mlp_hidden_layers_width", S)
    R, D = l_max + 1, (l_max + 1) ** 2
    W = R * u
    fg = B * S0 + S0 * Hs + Hs * S + S * W + S * (S + W) + S * (L + 1) * Hr + Hr
    for l in range(L):
        fg += (S * (l + 1) + u) * Ha + Ha * (S + (W if l < L - 1 else 0))
    fg *= 2.0
    from allegro_amd.nn import allegro_layer_irreps, build_w3j
    from allegro_amd import o3
    t = allegro_layer_irreps(l_max, True, L)
    env = o3.Irreps.spherical_harmonics(l_max)
    nnz = [int(np.count_nonzero(build_w3j(t[l], env, t[l + 1])[0])) for l in range(L)]
    tp = sum(3.0 * n * u for n in nnz)
    rest = (L + 1) * u * D + 2 * L * u * D + 5 * D
    f_mfma, f_valu = 2.0 * fg, 3.0 * tp + 2.0 * rest
    pk_m, pk_v = (PEAK_F32_TFLOPS, PEAK_F32_TFLOPS) if dtype == "float32" else (PEAK_F64_TFLOPS, PEAK_F64_TFLOPS)
    t_roof = E * (f_mfma / (pk_m * 1e12) + f_valu / (pk_v * 1e12))
    t_hbm = sum(nb for _, _, nb, _ in stages) / (PEAK_HBM_GBS * 1e9)
    return dict(flop_per_edge=f_mfma + f_valu, t_roof_fused_compute_ms=t_roof * 1e3, frac_of_fused_compute_roof=t_roof / t_step,
                algorithmic_bytes_per_edge=sum(nb for _, _, nb, _ in stages) / E, t_hbm_this_design_ms=t_hbm * 1e3,
                frac_of_hbm_roof_this_design=t_hbm / t_step)


def _tail_in_forward(stages):
    """Round 6: from 64 atoms per CU on the readout-reverse chain (12 MFMA steps, none of them folded away) runs in the tail of the fused
    forward -- the step then has no launch of its own for it and the forward's flops include it."""
    names = [s[0] for s in stages]
    return any(n.startswith("fused_fwd") for n in names) and not any(n.startswith("gc_64x64_128x128") for n in names)


def _fused_executed_ratio(d, stages):
    """MFMA steps the fused forward executes / step-equivalents of the reference's layers it is priced by (plan description; + 12 / + 12
    with the reverse chain in its tail)."""
    extra = 12 if _tail_in_forward(stages) else 0
    return (d["fused_mfma_steps_executed"] + extra) / (d["fused_mfma_steps_reference"] + extra)


def executed_bound(stages, dtype, t_step, model=None):
    """What the step EXECUTES (not SURVEY 8d's per-edge formula, which prices layers the folds and the per-atom operator form
    never run): linear-layer flops and algorithmic bytes of the launches as the library reports them, and the lower bound of a
    stage-materialised design, sum over launches of max(flops / matrix peak, bytes / HBM peak) -- a fraction of it is <= 1 by
    construction."""
    pk = (PEAK_F32_TFLOPS if dtype == "float32" else PEAK_F64_TFLOPS) * 1e12
    d = model.describe_plan() if model is not None else {}
    if d.get("fused_mfma_steps_reference"):  # (the library prices the fused forward by the REFERENCE's layers: scale to what it runs)
        ex = _fused_executed_ratio(d, stages)
        stages = [(n, ms, b, f * ex if n.startswith("fused_fwd") else f) for n, ms, b, f in stages]
    fl = sum(f for _, _, _, f in stages)
    nb = sum(b for _, _, b, _ in stages)
    t_lo = sum(max(f / pk, b / (PEAK_HBM_GBS * 1e9)) for _, _, b, f in stages)
    return dict(linear_layer_flops=fl, algorithmic_bytes=nb, launches=len(stages), t_matrix_at_peak_ms=fl / pk * 1e3,
                t_hbm_at_peak_ms=nb / (PEAK_HBM_GBS * 1e9) * 1e3, t_lower_bound_ms=t_lo * 1e3, frac_of_lower_bound=t_lo / t_step)


def profile_stages(model, pos, graph, reps=5):
    """[(kernel-launch name, ms, algorithmic bytes, flops)] of one forward+force pass, averaged over 5 passes:
    HIP events recorded by the library on the launch stream around every kernel (aa_model_energy_forces_profiled)."""
    lib = model._get_lib()
    model.energy_forces(pos, graph)  # make sure plan/weights/workspace exist
    max_stages = 128
    ms = (C.c_float * max_stages)()
    by = (C.c_double * max_stages)()
    fl = (C.c_double * max_stages)()
    names = C.create_string_buffer(32 * max_stages)
    n = C.c_int(0)
    e_atom = torch.empty(graph.num_atoms, dtype=model.dtype, device=pos.device)
    forces = torch.empty((graph.num_atoms, 3), dtype=model.dtype, device=pos.device)
    g = graph.c_struct()
    fn = lib.lib.aa_model_energy_forces_profiled
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    acc = {}
    stream = torch.cuda.current_stream(pos.device).cuda_stream if pos.is_cuda else 0  # (CPU: the tests' emulation build)
    for _ in range(reps):
        rc = fn(model._plan_handle, model._blob.data_ptr(), C.byref(g), pos.data_ptr(), model._workspace.data_ptr(),
                model._workspace.numel(), e_atom.data_ptr(), forces.data_ptr(),
                stream, max_stages, ms, names, C.byref(n), by, fl)
        lib.check(rc, "aa_model_energy_forces_profiled")
        for i in range(n.value):
            nm = names.raw[32 * i: 32 * i + 32].split(b"\0")[0].decode()
            acc.setdefault(i, [nm, 0.0, by[i], fl[i]])[1] += ms[i] / reps
    return [tuple(v) for _, v in sorted(acc.items())]


# kernel symbol behind each stage-name prefix
_SYMBOLS = (("gc_", "gemm_chain_bf16x3_kernel"), ("gemm_", "gemm_bf16x3_kernel"))
# the fp64 linear layers of one step run on three kernels (launch_gemm<double>: accumulator-resident rows kernel for N <= 128,
# operand-resident rows kernel for plain N > 128 layers, staged kernel for the rest); they are priced as one group
_F64_GEMM_GROUP = "fp64 linear layers (gemm_f64_rows_kernel<false>, gemm_f64_rows_kernel<true>, gemm_mfma_f64_pipe_kernel)"
_F64_GEMM_KEYS = ("gemm_f64_rows_kernel<false>", "gemm_f64_rows_kernel<true>", "gemm_mfma_f64_pipe")
_SYMBOLS_F64 = (("gemm_", _F64_GEMM_GROUP),)


def roofline_from_stages(stages, dtype, workload="c4", attach_traffic=True):
    """Aggregate the per-launch HIP-event times per kernel symbol and report the dominant symbol against its
    roofline.  Algorithmic work per launch comes from the library: every distinct operand
    row read or written once; 2*M*K*N flop per GEMM layer.  All kernels of this path are HBM-bound at their
    algorithmic intensity (the fused GEMM chains run at <= 28 flop/B against a ridge of ~20 fp32 / ~300 bf16
    flop/B; their bf16x3 MFMA time at peak is below the HBM time), so `bound` is "hbm"; the GEMM symbols also
    report their fp32-equivalent TFLOP/s."""
    by_sym = {}
    for name, ms, nbytes, flops in stages:
        sym = next((s for pre, s in (_SYMBOLS if dtype == "float32" else _SYMBOLS_F64) if name.startswith(pre)), name)
        d = by_sym.setdefault(sym, dict(ms=0.0, launches=0, flops=0.0, bytes=0.0))
        d["ms"] += ms
        d["launches"] += 1
        d["flops"] += flops
        d["bytes"] += nbytes
    sym, d = max(by_sym.items(), key=lambda kv: kv[1]["ms"])
    n = max(d["launches"], 1)
    t = d["ms"] * 1e-3 / n
    ach = d["bytes"] / n / t / 1e9
    roof = dict(bound="hbm", achieved=ach, peak=PEAK_HBM_GBS, unit="GB/s", frac=ach / PEAK_HBM_GBS, traffic=None,
                kernel=sym, avg_launch_ms=d["ms"] / n, launches_per_step=d["launches"],
                algorithmic_bytes_per_launch=d["bytes"] / n)
    if dtype == "float32" and sym.startswith("fused_fwd") and d["flops"] > 0:
        # the fused per-atom-tile forward does the work of seven launches with 2.1 KB/edge of traffic: ~80 flop/B against a
        # ridge of ~20 (fp32 matrix peak / HBM peak) -- bound by the matrix pipe.  Priced as SURVEY 8(d) prescribes for the
        # fused design: algorithmic fp32 flops of its linear layers against the fp32 MFMA peak (the arithmetic itself runs
        # as 6 bf16 MFMAs per product: mfma_bf16_TFLOPs below, against the 2.5 PFLOP/s bf16 peak)
        tf = d["flops"] / n / t / 1e12
        roof.update(bound="mfma", achieved=tf, peak=PEAK_F32_TFLOPS, unit="TFLOP/s", frac=tf / PEAK_F32_TFLOPS,
                    algorithmic_flops_per_launch=d["flops"] / n, hbm_GBps=ach)
    if dtype == "float64" and sym == _F64_GEMM_GROUP and d["flops"] > 0:
        # the fp64 linear layers (K, N >= 128) run at >= 64 flop/B: bound by the fp64 matrix pipe, not by HBM
        tf = d["flops"] / n / t / 1e12
        roof.update(bound="mfma", achieved=tf, peak=PEAK_F64_TFLOPS, unit="TFLOP/s", frac=tf / PEAK_F64_TFLOPS,
                    algorithmic_flops_per_launch=d["flops"] / n, hbm_GBps=ach)
    # HBM bytes per launch measured with rocprofv3 PMC passes of this same command (tools/profile_gpu.sh ->
    # tools/pmc_to_json.py, committed under profiles/): rocprofv3 cannot wrap the process from inside, so the last
    # committed measurement of this workload is attached with its provenance
    # (attached only when the measurement was taken on THESE kernel sources: the JSON carries allegro_amd.build.source_hash())
    try:
        if not attach_traffic:  # (a rank's shard of the box: the committed per-launch counters are the whole box's)
            raise KeyError("shard")
        from allegro_amd.build import source_hash

        pj = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", f"pmc_traffic_{workload}.json")))
        key = next((k for k in pj["per_launch"] if k in sym or sym.startswith(k)), None)
        have, want = pj.get("source_hash"), source_hash()
        group = [e for k, e in pj["per_launch"].items() if any(g in k for g in _F64_GEMM_KEYS)] if sym == _F64_GEMM_GROUP else []
        if group and have == want:
            # launch-weighted mean over the kernels of the group
            nl = sum(e["launches"] for e in group)
            roof["traffic"] = sum((e.get("fetch_bytes", 0.0) + e.get("write_bytes", 0.0)) * e["launches"] for e in group) / max(nl, 1)
            roof["traffic_source"] = (f"rocprofv3 --pmc FETCH_SIZE (x2) + WRITE_SIZE, launch-weighted mean over the group's kernels, "
                                      f"{pj['source']} (kernel sources {want})")
        elif key is None and not group:
            roof["traffic_source"] = f"traffic: null -- {pj['source']} has no entry for {sym}"
        elif have != want:
            roof["traffic_source"] = (f"traffic: null -- committed PMC measurement {pj['source']} was taken on kernel sources "
                                      f"{have}, this build is {want}")
        else:
            e = pj["per_launch"][key]
            roof["traffic"] = e.get("fetch_bytes", 0.0) + e.get("write_bytes", 0.0)
            roof["traffic_source"] = (f"rocprofv3 --pmc FETCH_SIZE (x2) + WRITE_SIZE, mean per launch, {pj['source']} "
                                      f"(kernel sources {want})")
    except (OSError, ValueError, KeyError) as ex:
        roof["traffic_source"] = ("traffic: null -- a shard of the box (the committed per-launch counters are the whole box's)" if not attach_traffic else
                                  f"traffic: null -- no committed PMC measurement for this workload ({type(ex).__name__})")
    if d["flops"] > 0:
        roof["fp32_equiv_TFLOPs"] = d["flops"] / n / t / 1e12
        roof["mfma_bf16_TFLOPs"] = (6.0 if dtype == "float32" else 1.0) * d["flops"] / n / t / 1e12
    table = {k: dict(ms=round(v["ms"], 4), launches=v["launches"], GBps=round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1))
             for k, v in sorted(by_sym.items(), key=lambda kv: -kv[1]["ms"])}
    return roof, table


def cpu_baseline(g: G.Graph, cfg, model, target_edges=180000, reps=3, vs_fp64=True):
    """The oracle restatement (a port: kind='port') timed on this host's cores on a bounded sample:
    the first contiguous block of center atoms holding ~target_edges edges, evaluated in chunks of
    <=12k edges (exact by strict locality).  Thread counts: min(cores, 32), 8 and 1 (sweep; the best rate is `value`) -- eager
    PyTorch CPU slows down badly when oversubscribed on these small matrices (measured: 256 threads 70x slower than 8)."""
    from oracle import restatement as R

    dtype = {"float32": torch.float32, "float64": torch.float64}[cfg["model_dtype"]]
    cores = os.cpu_count() or 1
    threads = min(cores, 32)
    torch.set_num_threads(threads)
    sd = {k[len("func."):]: v.detach().cpu() for k, v in model.state_dict().items()}
    rowptr = G.csr_from_sorted_centers(g.edge_index[0], g.num_atoms)
    a1 = int(np.searchsorted(rowptr, target_edges, side="left"))
    a1 = max(1, min(a1, g.num_atoms))
    e1 = int(rowptr[a1])
    pos = torch.tensor(g.pos, dtype=dtype)
    ei = torch.tensor(g.edge_index[:, :e1])
    types = torch.tensor(g.types)
    sv = torch.tensor(g.shift_vec()[:e1], dtype=dtype) if g.cell_shift is not None else None
    ocfg = dict(cfg)
    R.allegro_energy_forces_chunked(ocfg, sd, pos, ei[:, :min(e1, 12000)], types, None if sv is None else sv[:min(e1, 12000)], 12000)
    L = cfg["num_layers"]

    def one_pass(nthreads, edges):
        torch.set_num_threads(nthreads)
        t0 = time.perf_counter()
        o = R.allegro_energy_forces_chunked(ocfg, sd, pos, ei[:, :edges], types, None if sv is None else sv[:edges], 12000)
        return time.perf_counter() - t0, o

    # thread sweep (the port gains 3 % from 8 -> 32 threads): 1 / 8 / min(cores, 32) threads -- the low counts on a
    # contiguous fraction of the sample (the rate per edge is what is compared) -- and the BEST rate is the one quoted
    ts = []
    out = None
    for _ in range(reps):
        t, out = one_pass(threads, e1)
        ts.append(t)
    t = float(np.median(ts))
    sweep = [dict(threads=threads, edges=e1, seconds=t, value=e1 * L / t)]
    if reps > 1:
        for nt, frac in ((8, 1.0), (1, 0.125)):
            if nt >= threads:
                continue
            ee = int(rowptr[max(1, int(np.searchsorted(rowptr, int(e1 * frac), side="left")))]) if frac < 1.0 else e1
            tt, _ = one_pass(nt, ee)
            sweep.append(dict(threads=nt, edges=ee, seconds=tt, value=ee * L / tt))
    torch.set_num_threads(threads)
    best = max(sweep, key=lambda r: r["value"])
    # the reference's own files (verbatim, eager) against this port on the build host, fp32, same chunks:
    # reference / port time = 2.2 / 3.4 / 1.8 / 4.1 at 1 / 2 / 4 / 8 threads (profiles/r04_cpu_reference_vs_port_threads.json) -- the
    # smallest ratio gives the most favourable figure for the reference
    ref_ratio = 1.8
    base = dict(value=best["value"], unit="edge-TP/s", cores=best["threads"], kind="port",
                sample=f"first {a1} center atoms / {e1} edges of the same box in chunks of <=12k edges, "
                       f"oracle/restatement.py eager PyTorch CPU {cfg['model_dtype']}, best of a thread sweep on {cores} cores "
                       f"({', '.join(str(r['threads']) for r in sweep)} threads), median of {reps} at {threads} threads, {t:.2f} s per pass",
                thread_sweep=sweep,
                reference_equivalent=dict(value=best["value"] / ref_ratio, ratio=ref_ratio, ratio_measured_at_threads="1-8 (build host)",
                                          note="port rate / (reference-verbatim time / port time); the reference cannot travel to this box, the "
                                               "ratio is BASELINE.md section 3's smallest (1.8 at 4 threads; 2.2-4.1 at 1, 2, 8)"))
    if threads > 8 and reps > 1:
        r8 = [r for r in sweep if r["threads"] == 8]
        if r8:
            base["at_8_threads"] = dict(value=r8[0]["value"], unit="edge-TP/s", cores=8, seconds=r8[0]["seconds"])
    # parity of the timed HIP path against this oracle pass (same edge subset: the first a1 center atoms' edges)
    dev = next(model.parameters()).device
    gsub = PreparedGraph(ei.to(dev), types.to(dev), g.num_atoms, None if sv is None else sv.to(dev))
    e_h, f_h = model.energy_forces(pos.to(dev), gsub)
    e_o, f_o = out["atomic_energy"].reshape(-1)[:a1], out["forces"]
    d_e = float((e_h[:a1].cpu() - e_o).abs().max())
    d_f = float((f_h.cpu() - f_o).abs().max())
    tol_f = 1e-4 if dtype == torch.float32 else 1e-9 * max(1.0, float(f_o.abs().max()))
    tol_e = (5e-5 if dtype == torch.float32 else 1e-9) * max(1.0, float(e_o.abs().max()))
    parity = dict(atoms=a1, edges=e1, max_dE=d_e, max_dF=d_f, tol_dE=tol_e, tol_dF=tol_f, ok=bool(d_e <= tol_e and d_f <= tol_f),
                  against="oracle/restatement.py (CPU, same dtype) on the same edge subset; tolerances: forces 1e-4 eV/A "
                          "(north star) in fp32, 1e-9 x scale in fp64; energies 5e-5 / 1e-9 x scale "
                          "(tests/model/test_allegro.py:72-74 of the reference)")
    if vs_fp64 and dtype == torch.float32:
        # whose error is it?  The fp32 HIP path and the fp32 CPU oracle each against the fp64 oracle on the same (upcast)
        # weights and the same edge subset: the HIP arithmetic (bf16x3 split products, fp32 accumulation, its own summation
        # orders) is as close to the exact answer as the reference's own fp32 arithmetic is
        cfg64 = dict(ocfg, model_dtype="float64")
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        o64 = R.allegro_energy_forces_chunked(cfg64, sd64, pos.double(), ei, types, None if sv is None else sv.double(), 12000)
        f64, e64 = o64["forces"], o64["atomic_energy"].reshape(-1)[:a1]
        hip_f, cpu_f = float((f_h.cpu().double() - f64).abs().max()), float((f_o.double() - f64).abs().max())
        hip_e, cpu_e = float((e_h[:a1].cpu().double() - e64).abs().max()), float((e_o.double() - e64).abs().max())
        parity["vs_fp64"] = dict(hip=dict(max_dF=hip_f, max_dE=hip_e), oracle_fp32=dict(max_dF=cpu_f, max_dE=cpu_e),
                                 hip_over_oracle_fp32_dF=hip_f / max(cpu_f, 1e-30),
                                 what="max abs deviation from oracle/restatement.py in float64 (weights upcast) on the same edge subset")
    return base, parity


def secondary_workload(name, dev, steps, warmup, cpu_edges):
    """Compact record of another BASELINE workload for the default line (`secondary`): timed exactly like the headline
    (W warm-ups, K steps between synchronisations, inputs resident), dominant kernel against its roofline from a separate
    HIP-event pass, parity of the timed path against the CPU oracle on a bounded edge subset."""
    g, cfg = make_workload(name)
    dtype = {"float32": torch.float32, "float64": torch.float64}[cfg["model_dtype"]]
    model = HipAllegroModel(**cfg).to(dev)
    N, E, L = g.num_atoms, g.num_edges, cfg["num_layers"]
    sv = g.shift_vec()
    pos = torch.tensor(g.pos, dtype=dtype, device=dev)
    graph = PreparedGraph(torch.tensor(g.edge_index, device=dev), torch.tensor(g.types, device=dev), N,
                          torch.tensor(sv, dtype=dtype, device=dev) if sv is not None else None)
    for _ in range(warmup):
        model.energy_forces(pos, graph)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.energy_forces(pos, graph)
    torch.cuda.synchronize()
    t_step = (time.perf_counter() - t0) / steps
    model.check()
    stages = profile_stages(model, pos, graph, reps=3)
    roof, _ = roofline_from_stages(stages, cfg["model_dtype"], name)
    base, parity = cpu_baseline(g, cfg, model, target_edges=cpu_edges, reps=1, vs_fp64=True)
    rec = dict(workload=f"{name}: {WORKLOADS[name]['desc']}", atoms=N, edges=E, dtype="f32" if dtype == torch.float32 else "f64",
               steps=steps, warmup=warmup, ms_per_step=t_step * 1e3, value=E * L / t_step, unit="edge-TP/s",
               roofline={k: roof[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_ms", "launches_per_step")},
               executed=executed_bound(stages, cfg["model_dtype"], t_step, model),
               parity_sample={k: parity[k] for k in ("atoms", "edges", "max_dE", "max_dF", "tol_dE", "tol_dF", "ok") if k in parity},
               cpu_baseline=dict(value=base["value"], unit=base["unit"], cores=base["cores"], kind=base["kind"]))
    if "vs_fp64" in parity:
        rec["parity_sample"]["vs_fp64"] = {k: parity["vs_fp64"][k] for k in ("hip", "oracle_fp32")}
    del model, graph, pos
    torch.cuda.empty_cache()
    return rec


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, out, own_ids, n_atoms, dist, rank):
    """--dump-outputs: (E_i, forces) of the last timed step as out_dir/atomic_energy.npy [N] and out_dir/forces.npy [N,3] in the
    model dtype (float32 / float64), atoms in the order of the generated box.  Sharded runs: every rank's owned rows (`own_ids`: their
    atom ids) are gathered on rank 0.  Above DUMP_MAX_BYTES a fixed, seeded sample of atoms is written instead, their ids (as
    float64) in out_dir/sample_rows.npy."""
    e, f = (t.detach().cpu().numpy() for t in out)
    if own_ids is not None:
        parts = [(np.asarray(own_ids), e, f)]
        if dist is not None:
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, (np.asarray(own_ids), e, f))
        if rank != 0:
            return
        e_all = np.zeros(n_atoms, dtype=e.dtype)
        f_all = np.zeros((n_atoms, 3), dtype=f.dtype)
        seen = np.zeros(n_atoms, dtype=np.int64)
        for ids, ee, ff in parts:
            e_all[ids], f_all[ids] = ee, ff
            seen[ids] += 1
        if not (seen == 1).all():
            raise RuntimeError("--dump-outputs: the shards' owned atoms do not partition the box")
        e, f = e_all, f_all
    elif rank != 0:
        return
    if e.shape != (n_atoms,) or f.shape != (n_atoms, 3):
        raise RuntimeError(f"--dump-outputs: unexpected output shapes {e.shape} / {f.shape} for {n_atoms} atoms")
    arrays = {"atomic_energy": e, "forces": f}
    row_bytes = e.itemsize + 3 * f.itemsize
    if n_atoms * row_bytes > DUMP_MAX_BYTES:
        k = DUMP_MAX_BYTES // (row_bytes + 8)
        rows = np.sort(np.random.default_rng(0).choice(n_atoms, size=k, replace=False))
        arrays = {"atomic_energy": e[rows], "forces": f[rows], "sample_rows": rows.astype(np.float64)}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a))


KB_EV = 8.617333262e-5     # eV / K
ACC_UNIT = 9.64853321e-3   # (eV / A / amu) in A / fs^2


def md_loop(model, pos0, types, cell, r_cut, steps=50, warmup=10, dt=1.0, temperature=300.0, skin=0.0, mass=28.0855, force_scale=0.0,
            cross_check=None, cross_every=0):
    """NVE velocity-Verlet loop with EVERYTHING on the device -- neighbour list (`aa_nl_*`) + graph preparation every step (or a
    Verlet list with `skin`), the hot path, the integrator -- so that "ns/day for the box" is measured as a loop and not derived
    from the step time, and its energy conservation: E_pot + E_kin of the trajectory moves only by the O(dt^2) of the integrator
    when the forces are the gradient of the energies (tools/md_loop.py: 4x smaller per halving of dt at C4).  The model has random
    weights: energies and forces are scaled so that the rms force is 1 eV/A; its potential has no repulsive core, keep runs short
    (~100 fs at 300 K).  Returns a dict; `ns_per_day` is wall-clock, `ns_per_day_at_median` from the median step."""
    from allegro_amd.nn import neighbor_list

    dev = pos0.device
    N = pos0.shape[0]
    pos = pos0.clone()
    gen = torch.Generator(device=dev).manual_seed(7)
    vel = torch.randn(N, 3, device=dev, generator=gen, dtype=pos.dtype) * (KB_EV * temperature / mass * ACC_UNIT) ** 0.5  # A / fs
    vel -= vel.mean(0, keepdim=True)
    state = {"graph": None, "pos_ref": None, "rebuilds": 0, "edges": 0, "max_degree": 0}

    def graph_for(p):
        if state["graph"] is None or skin == 0.0 or float((p - state["pos_ref"]).square().sum(1).max()) > (0.5 * skin) ** 2:
            nl = neighbor_list(p, cell, True, r_cut + skin)
            state["graph"] = nl.prepare(types)
            state["pos_ref"] = p.clone()
            state["rebuilds"] += 1
            state["edges"] = nl.num_edges
            state["max_degree"] = max(state["max_degree"], state["graph"].max_degree)
        return state["graph"]

    e_atom, f = model.energy_forces(pos, graph_for(pos))
    scale = force_scale or 1.0 / float(f.square().sum(1).mean().sqrt())
    f = f * scale

    def kinetic(v):
        return 0.5 * mass / ACC_UNIT * float(v.double().square().sum())

    e0 = float(e_atom.double().sum()) * scale + kinetic(vel)
    trace, cross, step_ms = [], [], []
    half = 0.5 * dt * ACC_UNIT / mass
    t0 = t_prev = 0.0
    for step in range(-warmup, steps):
        if step == 0:
            torch.cuda.synchronize()
            t0 = t_prev = time.perf_counter()
        vel = vel + half * f
        pos = pos + dt * vel
        e_atom, f = model.energy_forces(pos, graph_for(pos))
        f = f * scale
        vel = vel + half * f
        if step >= 0:
            torch.cuda.synchronize()  # (per-step wall times: the median is the robust figure)
            t_now = time.perf_counter()
            step_ms.append((t_now - t_prev) * 1e3)
            t_prev = t_now
            if (step + 1) % max(1, steps // 20) == 0 or step + 1 == steps:
                trace.append((step + 1, float(e_atom.double().sum()) * scale, kinetic(vel), float(f.square().sum(1).max().sqrt())))
                t_prev = time.perf_counter()
            if cross_check is not None and cross_every and (step + 1) % cross_every == 0:
                e2, f2 = cross_check.energy_forces(pos, state["graph"])
                de = e2.double() - e_atom.double()
                cross.append(dict(step=step + 1, max_degree=state["graph"].max_degree, dE_total=float(de.sum()) * scale,
                                  max_dE_atom=float(de.abs().max()) * scale, max_dF=float((f2 * scale - f).abs().max())))
                t_prev = time.perf_counter()
    torch.cuda.synchronize()
    wall = sum(step_ms) * 1e-3
    model.check()
    ke = [t[2] for t in trace]
    drift = max(abs(t[1] + t[2] - e0) for t in trace)
    ke_mean = sum(ke) / len(ke)
    med = sorted(step_ms)[len(step_ms) // 2]
    return dict(atoms=N, edges_last_list=state["edges"], steps=steps, warmup=warmup, dt_fs=dt, temperature_K=temperature, skin_A=skin,
                list_rebuilds=state["rebuilds"], max_degree_seen=state["max_degree"], force_scale=scale,
                ms_per_md_step=wall / steps * 1e3, ns_per_day=dt * 1e-6 * steps / wall * 86400.0, ms_per_md_step_median=med,
                ns_per_day_at_median=dt * 1e-6 / (med * 1e-3) * 86400.0,
                slowest_steps=sorted(((round(t, 2), i + 1) for i, t in enumerate(step_ms)), reverse=True)[:4],
                includes="device neighbour list + graph preparation (every rebuild), hot path, velocity-Verlet update",
                e_total_start_eV=e0, max_abs_drift_eV=drift, mean_kinetic_eV=ke_mean, drift_over_mean_kinetic=drift / max(ke_mean, 1e-30),
                cross_check_vs_staged=cross or None,
                trace=[dict(step=s, e_pot=p, e_kin=k, e_tot=p + k, max_force=mf) for s, p, k, mf in trace])


def gpu_reference_baseline(g: G.Graph, cfg, model, dev, target_edges=60000, reps=3):
    """North-star denominator: the reference-equivalent eager PyTorch-ROCm path (oracle/restatement.py moved
    to the GPU) on a bounded contiguous block of center atoms, in chunks of <=20k edges as BASELINE.md
    prescribes (the reference's eager [E,u,9,9,9] intermediate does not fit otherwise; the restatement
    already avoids that tensor, so this baseline is FASTER than the reference's own eager Contracter)."""
    from oracle import restatement as R

    dtype = {"float32": torch.float32, "float64": torch.float64}[cfg["model_dtype"]]
    sd = {k[len("func."):]: v.detach().to(dev) for k, v in model.state_dict().items()}
    rowptr = G.csr_from_sorted_centers(g.edge_index[0], g.num_atoms)
    a1 = max(1, min(int(np.searchsorted(rowptr, target_edges, side="left")), g.num_atoms))
    e1 = int(rowptr[a1])
    pos = torch.tensor(g.pos, dtype=dtype, device=dev)
    ei = torch.tensor(g.edge_index[:, :e1], device=dev)
    types = torch.tensor(g.types, device=dev)
    sv = torch.tensor(g.shift_vec()[:e1], dtype=dtype, device=dev) if g.cell_shift is not None else None

    def one():
        n_done = 0
        while n_done < e1:
            n = min(20000, e1 - n_done)
            R.allegro_energy_forces(dict(cfg), sd, pos, ei[:, n_done:n_done + n], types,
                                    None if sv is None else sv[n_done:n_done + n])
            n_done += n

    one()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        one()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    return dict(value=e1 * cfg["num_layers"] / t, unit="edge-TP/s", kind="port",
                what="oracle/restatement.py (a port that already avoids the reference's [E,u,9,9,9] intermediate) as eager "
                     "PyTorch-ROCm on this GPU -- the denominator of north_star's '>= 5x the reference PyTorch-ROCm forward'",
                sample=f"first {a1} center atoms / {e1} edges of the same box in chunks of <=20k edges, median of {reps}, "
                       f"{t * 1e3:.1f} ms per pass")


def train_op_bench(args, dev):
    """`--mode train-op`: the training step of the OPERATOR seam (what `nequip-train` runs through a model whose
    Contracters were swapped by `enable_HipContracter`): one `HipContracter.forward` in training mode on the workload's
    neighbor list + a force-matching style loss (a function of the first derivatives w.r.t. x1, differentiated again
    w.r.t. the path weights and both inputs) -- forward + double backward.  Reported for the segmented differentiable
    form (default), the first formulation with every edge its own segment (AA_TRAIN_PER_EDGE=1) and the eager PyTorch-ROCm
    port of the reference's Contracter (oracle, baseline only; on a bounded edge sample: its [E,u,9,9] intermediates)."""
    from allegro_amd.nn import HipContracter

    g, cfg = make_workload(args.workload)
    u, l_max = cfg["num_tensor_features"], cfg["l_max"]
    dtype = {"float32": torch.float32, "float64": torch.float64}[cfg["model_dtype"]]
    irreps = " + ".join(f"{l}{'e' if l % 2 == 0 else 'o'}" for l in range(l_max + 1))
    torch.manual_seed(0)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        c = HipContracter(irreps, irreps, irreps, mul=u, path_channel_coupling=True,
                          scatter_factor=1.0 / float(np.sqrt(cfg["avg_num_neighbors"]))).to(dev)
    finally:
        torch.set_default_dtype(prev)
    c.train()
    c.assume_sorted_idxs = True
    D = (l_max + 1) ** 2
    N = g.num_atoms

    def run(E, fwd, steps, warmup):
        idxs = torch.tensor(g.edge_index[0][:E], device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        x1 = torch.randn(E, u, D, dtype=dtype, device=dev, generator=gen, requires_grad=True)
        x2 = torch.randn(E, u, D, dtype=dtype, device=dev, generator=gen, requires_grad=True)

        def step():
            y = fwd(x1, x2, idxs)
            (g1,) = torch.autograd.grad(y.square().sum(), x1, create_graph=True)  # "forces"
            loss = (g1 ** 2).sum() + y.sum()
            return torch.autograd.grad(loss, [c.weights, x1, x2])

        for _ in range(warmup):
            out = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, [o.detach() for o in out]

    E = g.num_edges
    res = {}
    os.environ.pop("AA_TRAIN_PER_EDGE", None)
    ms_seg, out_seg = run(E, lambda a, b, i: c(a, b, i, N), args.steps, args.warmup)
    res["segmented"] = dict(ms_per_step=ms_seg, edges=E, edges_per_s=E / ms_seg * 1e3)
    os.environ["AA_TRAIN_PER_EDGE"] = "1"
    ms_pe, out_pe = run(E, lambda a, b, i: c(a, b, i, N), max(2, args.steps // 4), 1)
    os.environ.pop("AA_TRAIN_PER_EDGE", None)
    res["per_edge_segments"] = dict(ms_per_step=ms_pe, edges=E, edges_per_s=E / ms_pe * 1e3)
    agree = max(float((a - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(out_seg, out_pe))
    from oracle import restatement as R  # (baseline leg only)

    Es = min(E, 20000)
    ms_eager, _ = run(Es, lambda a, b, i: R.contracter_forward(a, b, i, N, c.weights, c.w3j, True, c.scatter_factor), max(2, args.steps // 4), 1)
    res["eager_port_gpu"] = dict(ms_per_step=ms_eager, edges=Es, edges_per_s=Es / ms_eager * 1e3, kind="port")
    line = dict(metric="Contracter training step (forward + double backward of a force-matching loss), edges/s", mode="train-op",
                value=res["segmented"]["edges_per_s"], unit="edges/s", n_gpus=1, steps=args.steps, warmup=args.warmup,
                ms_per_step=ms_seg, higher_is_better=True, dtype="f32" if dtype == torch.float32 else "f64", data="synthetic",
                config=dict(workload=f"{args.workload}: {N} atoms / {E} edges, {irreps} x {irreps} -> {irreps}, {u} channels, coupled path weights"),
                variants=res, speedup_vs_per_edge_segments=res["segmented"]["edges_per_s"] / res["per_edge_segments"]["edges_per_s"],
                speedup_vs_eager_port=res["segmented"]["edges_per_s"] / res["eager_port_gpu"]["edges_per_s"],
                max_rel_diff_between_hip_variants=agree)
    print(json.dumps(line), flush=True)


def train_step_bench(args, dev):
    """`--mode train-step`: one optimisation step of the WHOLE model in training mode (`HipAllegroModel.train()`,
    allegro_amd/training.py): energies + forces attached to the graph, a force- and energy-matching loss, backward into every
    parameter (the forces are differentiated again), Adam update.  Tensor products on the HIP kernels, linear layers on
    library GEMMs.  Baseline: the same step through the eager PyTorch-ROCm port of the reference model (oracle, baseline
    only) on a bounded block of center atoms (its [E,u,d,d] intermediates)."""
    g, cfg = make_workload(args.workload)
    dtype = {"float32": torch.float32, "float64": torch.float64}[cfg["model_dtype"]]
    torch.manual_seed(0)
    model = HipAllegroModel(**cfg).to(dev).train()
    N, E = g.num_atoms, g.num_edges
    sv = g.shift_vec()
    pos = torch.tensor(g.pos, dtype=dtype, device=dev)
    types = torch.tensor(g.types, device=dev)
    graph = PreparedGraph(torch.tensor(g.edge_index, device=dev), types, N, torch.tensor(sv, dtype=dtype, device=dev) if sv is not None else None)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-4)
    gen = torch.Generator(device=dev).manual_seed(2)
    f_target = 0.1 * torch.randn(N, 3, dtype=dtype, device=dev, generator=gen)
    ev = model._training_evaluator()

    def loss_fn(forces, total_energy):
        return (forces - f_target).square().mean() + 1e-3 * (total_energy / N).square().sum()

    # --train-chunk-edges: the exact gradient accumulated one block of center atoms at a time (ChunkedTrainingStep): boxes whose
    # whole differentiable graph does not fit (C4: ~150 GB of activations in one piece)
    chunked = model.chunked_training_step(graph, args.train_chunk_edges) if args.train_chunk_edges > 0 else None

    def step():
        opt.zero_grad(set_to_none=True)
        if chunked is not None:
            loss, _, _ = chunked.step(pos, loss_fn)
        else:
            out = ev.forward({"pos": pos}, graph)
            loss = loss_fn(out["forces"], out["total_energy"])
            loss.backward()
        opt.step()
        return loss.detach()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    peak0 = torch.cuda.max_memory_allocated(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    peak = max(peak0, torch.cuda.max_memory_allocated(dev))
    # inference step of the same model on the same graph, for scale
    model.eval()
    for _ in range(3):
        model.energy_forces(pos, graph)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        model.energy_forces(pos, graph)
    torch.cuda.synchronize()
    ms_inf = (time.perf_counter() - t0) / 10 * 1e3
    # baseline: eager port of the reference model, same loss, on a bounded block of centers
    from oracle import restatement as R  # (baseline leg only)

    rowptr = G.csr_from_sorted_centers(g.edge_index[0], N)
    a1 = max(1, min(int(np.searchsorted(rowptr, 20000, side="left")), N))
    e1 = int(rowptr[a1])
    sd = {k[len("func."):]: v.detach().clone().to(dev) for k, v in model.state_dict().items()}
    names = [k[len("func."):] for k, p in model.named_parameters() if k not in model._frozen_keys]
    for k in names:
        sd[k].requires_grad_(True)
    opt_r = torch.optim.Adam([sd[k] for k in names], lr=1e-4)
    ei_s = torch.tensor(g.edge_index[:, :e1], device=dev)
    sv_s = torch.tensor(sv[:e1], dtype=dtype, device=dev) if sv is not None else None

    def step_ref():
        opt_r.zero_grad(set_to_none=True)
        p = pos.detach().clone().requires_grad_(True)
        e_atom = R.allegro_energy(dict(cfg), sd, p, ei_s, types, sv_s)
        (gp,) = torch.autograd.grad(e_atom.sum(), p, create_graph=True)
        loss = (-gp - f_target).square().mean() + 1e-3 * (e_atom.sum() / N).square()
        loss.backward()
        opt_r.step()

    if args.no_gpu_reference:  # (profiling runs: only the product's kernels in the trace)
        ms_ref = None
    else:
        step_ref()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            step_ref()
        torch.cuda.synchronize()
        ms_ref = (time.perf_counter() - t0) / 3 * 1e3
    L = cfg["num_layers"]
    line = dict(metric="whole-model training step (forward, force+energy loss, backward into every parameter, Adam), edge tensor-products/s",
                mode="train-step", value=E * L / ms * 1e3, unit="edge-TP/s", n_gpus=1, steps=args.steps, warmup=args.warmup, ms_per_step=ms,
                higher_is_better=True, dtype="f32" if dtype == torch.float32 else "f64", data="synthetic",
                config=dict(workload=f"{args.workload}: {N} atoms / {E} edges, l_max {cfg['l_max']}, {L} layers, {cfg['num_tensor_features']} tensor features",
                            parameters=int(sum(p.numel() for p in params)), optimizer="Adam",
                            kernels="eager / library GEMMs (AA_TRAIN_EAGER=1)" if os.environ.get("AA_TRAIN_EAGER", "0")[:1] == "1" else
                                    "aa_linear_forward / _wgrad + aa_weighted_channels[_pair/_sum] + aa_silu_derivative + aa_scalar_column + tensor-product kernels",
                            chunks=None if chunked is None else dict(max_edges=args.train_chunk_edges, count=len(chunked.chunks))),
                final_loss=float(loss), peak_memory_GB=peak / 1e9, inference_ms_per_step=ms_inf, train_over_inference=ms / ms_inf,
                eager_port_gpu=None if ms_ref is None else dict(ms_per_step=ms_ref, edges=e1, value=e1 * L / ms_ref * 1e3, unit="edge-TP/s", kind="port",
                                    sample=f"first {a1} center atoms / {e1} edges of the same box"),
                speedup_vs_eager_port=None if ms_ref is None else (E / ms) / (e1 / ms_ref))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="c4", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need (sustained run, profile / rooflines, neighbour list, MD loop, "
                         "CPU / GPU baselines with the parity sample, secondary workloads); the --no-* switches below thin this out")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the per-atom energies and forces of the last timed step to DIR/<name>.npy (at most 64 MB: a fixed, "
                         "seeded sample of rows beyond that, with their atom ids in DIR/sample_rows.npy)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-gpu-reference", action="store_true", help="skip the eager PyTorch-ROCm oracle path on the GPU")
    ap.add_argument("--gpu-reference", action="store_true", help="(default now; kept for old command lines)")
    ap.add_argument("--sustain", type=float, default=8.0,
                    help="seconds of additional back-to-back steps AFTER the timed region (reported as config.sustained): "
                         "long enough for an external sampler (rocm-smi every few seconds) to witness the GPU busy; 0 = off")
    ap.add_argument("--stages", action="store_true",
                    help="also print every launch of one step with its HIP-event time (runs the profile pass, also without --full)")
    ap.add_argument("--no-md", action="store_true", help="skip the short NVE loop (config.md_loop: measured ns/day incl. neighbour lists)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="default C4 line only: skip the compact C3 / C5 records (`secondary`: ms/step, roofline fraction, parity sample)")
    ap.add_argument("--emulate-shard", default=None, metavar="R/W",
                    help="analysis only: run rank R's atom block of a W-way partition on this one GPU (no collective)")
    ap.add_argument("--shard-sweep", type=int, default=0, metavar="W",
                    help="analysis only: time every rank's compact shard of a W-way partition on this one GPU, one after "
                         "the other (load balance: max / mean shard time; no collective), print one JSON line and exit")
    ap.add_argument("--dist-mode", default="halo", choices=["halo", "allreduce"],
                    help="N > 1: halo = sharded positions, forward / reverse communication of ghost rows (two all_to_all_single per step; every "
                         "rank builds only its slab's neighbour list); allreduce = replicated positions, one all-reduce of F[N,3] (the round-3 path)")
    ap.add_argument("--train-chunk-edges", type=int, default=0,
                    help="--mode train-step: accumulate the gradient one block of center atoms (<= this many edges) at a time "
                         "(exact; peak memory ~ the block).  0 = the whole frame in one graph")
    ap.add_argument("--mode", default="step", choices=["step", "train-op", "train-step"],
                    help="step: the whole hot path (default, the driver's contract); train-op: training step of the operator seam; "
                         "train-step: optimisation step of the whole model in training mode")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and (args.mode != "step" or args.shard_sweep or args.emulate_shard):
        raise SystemExit("bench.py: --dump-outputs writes the outputs of the whole box: --mode step without --shard-sweep / --emulate-shard")
    if args.mode == "train-op":
        assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
        dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(dev)
        return train_op_bench(args, dev)
    if args.mode == "train-step":
        assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
        dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(dev)
        return train_step_bench(args, dev)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` launches itself: one process per GPU under torch.distributed.run on this node (rendezvous on
        # 127.0.0.1, a free port), same arguments; the ranks below read RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment.
        import socket

        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (RCCL between processes needs dmabuf IPC on this stack)
        os.environ.setdefault("OMP_NUM_THREADS", "4")
        sys.stdout.flush()
        os.execv(sys.executable, cmd)
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    # TEST-ONLY (tests/test_bench_launch.py): AA_BENCH_EMULATED=1 runs the N > 1 launch line on a box without a GPU -- CPU tensors through
    # the CPU emulation build of the same kernel sources (tests/emu), gloo, no profile.  The line says so in `data`; never a measurement.
    emulated = os.environ.get("AA_BENCH_EMULATED") == "1"
    if emulated:
        if not (world > 1 and WORKLOADS[args.workload]["kind"] == "si" and args.dist_mode == "halo"):
            raise SystemExit("AA_BENCH_EMULATED=1 is the launch-line test of the sharded branch only (--gpus N > 1, a Si workload)")
        from tests.hip_utils import emu_lib

        os.environ["AA_BENCH_BACKEND"] = "gloo"
        args.no_profile, args.sustain = True, 0.0
        torch.cuda.synchronize = lambda *a, **k: None
    assert emulated or torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    # (AA_BENCH_BACKEND=gloo AA_BENCH_DEVICE=0: the N > 1 code path with all ranks on ONE device and host-staged rows -- how the
    #  launch line of the driver's scaling run is exercised end to end on a one-GPU box; RCCL refuses two ranks on one GPU)
    backend = os.environ.get("AA_BENCH_BACKEND", "nccl")
    if world > 1 and backend == "nccl" and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py --gpus {world}: {torch.cuda.device_count()} GPU(s) visible and RCCL takes one rank per device "
                         "(AA_BENCH_BACKEND=gloo AA_BENCH_DEVICE=0 runs the same code path with all ranks on one device, rows staged "
                         "through the host: a launch-line check, not a scaling measurement)")
    dev = torch.device("cpu") if emulated else torch.device("cuda", int(os.environ.get("AA_BENCH_DEVICE", local_rank)))
    if not emulated:
        torch.cuda.set_device(dev)
    bench_lib = emu_lib() if emulated else None
    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    halo = (world > 1 or args.emulate_shard or args.shard_sweep) and args.dist_mode == "halo" and WORKLOADS[args.workload]["kind"] == "si"
    shard = None
    owned_mode, pos_local = False, None
    if halo:
        # no rank ever holds the full edge list: positions of the box (the one O(N) array, 1.2 MB at C4) -> slab order -> this
        # rank's slab + halo -> device cell list of that subset only (allegro_amd/dist.py: HaloShard.from_positions)
        w = WORKLOADS[args.workload]
        rcut = float(os.environ.get("AA_BENCH_RCUT", "5.0"))
        pos_np, cell_np = G.diamond_si(int(os.environ.get("AA_BENCH_CELLS", w["cells"])))
        N = pos_np.shape[0]
        cfg = si_model_cfg(28.0)  # (avg_num_neighbors: set from the measured edge count below, as make_workload does)
        cfg["r_max"], cfg["l_max"] = rcut, w.get("l_max", cfg["l_max"])
        cfg["num_tensor_features"] = w.get("u", cfg["num_tensor_features"])
        cfg["model_dtype"] = w["dtype"]
        dtype = {"float32": torch.float32, "float64": torch.float64}[cfg["model_dtype"]]
        owned_mode = world > 1 and not args.emulate_shard and not args.shard_sweep and os.environ.get("AA_BENCH_SHARDS", "owned") == "owned"
        pos = None if owned_mode else torch.tensor(pos_np, dtype=dtype, device=dev)  # (owned mode: the frame never reaches a device)
        types = None if owned_mode else torch.zeros(N, dtype=torch.int64, device=dev)
        L = cfg["num_layers"]

        def make_shard(r, wsize, connect):
            return HaloShard.from_positions(pos, types, cell_np, rcut, r, wsize, connect=connect, lib=bench_lib)

        if args.shard_sweep:
            # every rank's shard through the functions a W-rank job runs (pack_forward, the hot path, accumulate_reverse), with the
            # plan tables of the real partition (InProcessHaloGroup) -- per shard: GPU time eager and replayed from a hipGraph, the
            # HOST time to issue one step (perf_counter around K un-synchronised steps: the Python side with the GPU running
            # behind), and the same with both communications issued as RCCL calls of the plan's row counts on a one-rank
            # communicator (self-exchange: the host and launch cost of the collectives, not xGMI time)
            from allegro_amd.dist import InProcessHaloGroup

            W = args.shard_sweep
            grp = InProcessHaloGroup([make_shard(r, W, False) for r in range(W)])
            E = sum(sh.graph.num_edges for sh in grp.shards)
            cfg["avg_num_neighbors"] = 28.0 if rcut == 5.0 else E / N
            model = HipAllegroModel(**cfg).to(dev)
            loop_err = None
            try:
                import torch.distributed as tdist

                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(29400 + os.getpid() % 2000))
                tdist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
            except Exception as ex:  # noqa: BLE001  (analysis only: the sweep still reports the other columns)
                tdist, loop_err = None, repr(ex)[:200]

            def timed(fn):
                """(GPU-inclusive ms per step, host-issue ms per step): median of 3 batches of K steps."""
                for _ in range(args.warmup):
                    fn()
                reps = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        fn()
                    t_host = time.perf_counter() - t0
                    torch.cuda.synchronize()
                    reps.append(((time.perf_counter() - t0) / args.steps * 1e3, t_host / args.steps * 1e3))
                return sorted(reps)[1], reps

            rows = []
            for sh in grp.shards:
                pl = sh.fill_local_positions(pos)
                pos_own = pl[: sh.n_own].clone()
                ns, ng = int(sh.send_idx.numel()), sh.n_ghost
                scratch = torch.empty((max(ns, ng, 1), 3), dtype=dtype, device=dev)

                def step_local():  # the rank's own work of `energy_forces_halo`, no communication
                    pos_loc, _, recv_r = sh.pack_forward(pos_own)
                    e_loc, f_loc = model.energy_forces(pos_loc, sh.graph)
                    return sh.accumulate_reverse(f_loc[: sh.n_own], recv_r)

                def step_loop():  # + both communications as RCCL self-exchanges of the plan's row counts
                    pos_loc, send_f, recv_r = sh.pack_forward(pos_own)
                    tdist.all_to_all_single(scratch[:ns], send_f)
                    e_loc, f_loc = model.energy_forces(pos_loc, sh.graph)
                    tdist.all_to_all_single(scratch[:ng], f_loc[sh.n_own:].contiguous())
                    return sh.accumulate_reverse(f_loc[: sh.n_own], recv_r)

                (ms, host), reps = timed(step_local)
                row = dict(rank=sh.rank, owned=sh.n_own, ghosts=ng, sent=ns, edges=sh.graph.num_edges, ms=ms, host_issue_ms=host,
                           ms_all=[r[0] for r in reps])
                model.enable_hip_graph(True)
                (row["ms_graph"], row["host_issue_ms_graph"]), _ = timed(step_local)
                if tdist is not None:
                    (row["ms_graph_loopback_comm"], row["host_issue_ms_graph_loopback_comm"]), _ = timed(step_loop)
                model.enable_hip_graph(False)
                if tdist is not None:
                    (row["ms_loopback_comm"], row["host_issue_ms_loopback_comm"]), _ = timed(step_loop)
                rows.append(row)
            if tdist is not None:
                tdist.destroy_process_group()
            ms = [x["ms"] for x in rows]
            hi = max(x.get("host_issue_ms_loopback_comm", x["host_issue_ms"]) / x.get("ms_loopback_comm", x["ms"]) for x in rows)
            print(json.dumps({"shard_sweep": W, "workload": args.workload, "atoms": N, "edges": E, "shards": rows,
                              "max_ms": max(ms), "mean_ms": sum(ms) / W, "imbalance_max_over_mean": max(ms) / (sum(ms) / W),
                              "host_issue_over_gpu_max": hi, "loopback_comm_error": loop_err,
                              "note": "one GPU, shards (slab + halo, each built from positions alone) run one after the other; `ms` has no "
                                      "communication, `*_loopback_comm` issues both all_to_all_single of the step as RCCL self-exchanges on a "
                                      "one-rank communicator (host + launch cost, no xGMI): an upper bound of the per-rank compute time and "
                                      "the host's issue time of a W-GPU run, NOT a multi-GPU measurement"}),
                  flush=True)
            return
        er, ew = (int(x) for x in args.emulate_shard.split("/")) if args.emulate_shard else (rank, world)
        if owned_mode:
            # a domain-decomposed host: the rank hands over ONLY the atoms of its slab (the synthetic generator stands in for the MD
            # code that owns them); halo candidates are exchanged between the ranks, no rank holds the frame on its device
            # (HaloShard.from_owned; AA_BENCH_SHARDS=positions keeps the replicated-frame constructor for A/B)
            fx = pos_np @ np.linalg.inv(cell_np)
            fx = fx[:, 0] - np.floor(fx[:, 0])
            mine = (fx >= rank / world) & (fx < (rank + 1) / world)
            pos_own = torch.tensor(pos_np[mine], dtype=dtype, device=dev)
            shard = HaloShard.from_owned(pos_own, torch.zeros(int(mine.sum()), dtype=torch.int64, device=dev), cell_np, rcut, rank, world,
                                         lib=bench_lib)
        else:
            shard = make_shard(er, ew, not args.emulate_shard)
        e_loc = torch.tensor([shard.graph.num_edges], dtype=torch.int64, device=dev)
        if dist is not None:
            dist.all_reduce(e_loc)
        E = int(e_loc.item()) if dist is not None else shard.graph.num_edges * ew  # (emulated shard: analysis only)
        cfg["avg_num_neighbors"] = E / N
        model = HipAllegroModel(**cfg).to(dev)
        if bench_lib is not None:
            model._bind_library(bench_lib)
        graph = shard.graph
        if not owned_mode:
            pos_local = shard.fill_local_positions(pos)
            pos_own = pos_local[: shard.n_own].clone()
        a0, a1 = shard.a0, shard.a1
        e0, e1 = 0, shard.graph.num_edges
        g = None
        del pos
    else:
        g, cfg = make_workload(args.workload)
        dtype = {"float32": torch.float32, "float64": torch.float64}[cfg["model_dtype"]]
        model = HipAllegroModel(**cfg).to(dev)
        N, E, L = g.num_atoms, g.num_edges, cfg["num_layers"]
        rowptr = G.csr_from_sorted_centers(g.edge_index[0], N)
        sv = g.shift_vec()
        pos = torch.tensor(g.pos, dtype=dtype, device=dev)
        types = torch.tensor(g.types, device=dev)
        if args.shard_sweep:
            # every rank's compact shard (owned block + ghost atoms, allegro_amd/dist.py) timed on this GPU, one at a time
            W = args.shard_sweep
            rows = []
            for r in range(W):
                sh = LocalShard(g.edge_index, g.types, N, sv, r, W, dev, dtype, rowptr)
                for _ in range(args.warmup):
                    sh.step(model, pos)
                reps = []
                for _ in range(3):  # median of 3 timed batches: one-off hiccups (allocator, clocks) are not load imbalance
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        sh.step(model, pos)
                    torch.cuda.synchronize()
                    reps.append((time.perf_counter() - t0) / args.steps * 1e3)
                rows.append(dict(rank=r, owned=sh.n_own, ghosts=sh.n_ghost, edges=sh.graph.num_edges, ms=sorted(reps)[1]))
                del sh
            ms = [x["ms"] for x in rows]
            print(json.dumps({"shard_sweep": W, "workload": args.workload, "atoms": N, "edges": E, "shards": rows,
                              "max_ms": max(ms), "mean_ms": sum(ms) / W, "imbalance_max_over_mean": max(ms) / (sum(ms) / W),
                              "note": "one GPU, shards run one after the other, no collective: an upper bound of the per-rank "
                                      "compute time of a W-GPU run, NOT a multi-GPU measurement"}), flush=True)
            return
        a0, a1 = 0, N
        if world > 1 or args.emulate_shard:
            er, ew = (int(x) for x in args.emulate_shard.split("/")) if args.emulate_shard else (rank, world)
            # this rank's compact share: owned atom block + ghost atoms in local numbering (O(local) graph / workspace)
            shard = LocalShard(g.edge_index, g.types, N, sv, er, ew, dev, dtype, rowptr)
            a0, a1 = shard.a0, shard.a1
            graph = shard.graph
        else:
            graph = PreparedGraph(torch.tensor(g.edge_index, device=dev), types, N,
                                  torch.tensor(sv, dtype=dtype, device=dev) if sv is not None else None)
        e0, e1 = int(rowptr[a0]), int(rowptr[a1])

    def step():
        if shard is None:
            return model.energy_forces(pos, graph)
        if halo:
            # sharded positions: forward communication of ghost positions, the hot path on the compact shard, reverse
            # communication of ghost forces (two all_to_all_single of ghost rows; allegro_amd/dist.py) -- what the gloo tests drive
            return energy_forces_halo(model, pos_own, shard)
        # compact shard + THE collective of the step (one RCCL all-reduce over xGMI carrying ghost-atom force
        # contributions and owned-atom energies; allegro_amd/dist.py) -- the function the gloo tests drive
        return energy_forces_local(model, pos, shard)

    for _ in range(args.warmup):
        step()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    dt_rank = time.perf_counter() - t0  # this rank's own K steps (its waits inside the collectives included), before the closing barrier
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    rank_ms = None
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        tr = torch.zeros(world, dtype=torch.float64, device=dev)
        tr[rank] = dt_rank / args.steps * 1e3
        dist.all_reduce(tr)
        ne = torch.zeros(world, dtype=torch.int64, device=dev)
        ne[rank] = e1 - e0
        dist.all_reduce(ne)
        rank_ms = {"max": float(tr.max()), "mean": float(tr.mean()), "min": float(tr.min()), "per_rank": [round(float(x), 4) for x in tr],
                   "edges_per_rank": [int(x) for x in ne]}
    ms_per_step = dt / args.steps * 1e3
    if args.dump_outputs:
        # (outside the clock, before anything else runs a step: the results may be views of buffers the next step overwrites)
        own_ids = None
        if halo:
            own_ids = np.nonzero(mine)[0] if owned_mode else shard.owned_ids().cpu().numpy()
        dump_outputs(args.dump_outputs, out, own_ids, N, dist, rank)
    # sustained run (outside the timed region, same step): the K-step region of the contract is ~0.2 s at C4, too short
    # for an independent utilisation sampler; all ranks take part so the collective pattern is the same
    sustained = None
    if args.full and args.sustain > 0 and not args.emulate_shard:
        n_sus = max(args.steps, int(args.sustain / max(dt / args.steps, 1e-6)))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n_sus):
            step()
        torch.cuda.synchronize()
        ds = time.perf_counter() - t1
        sustained = {"steps": n_sus, "seconds": ds, "ms_per_step": ds / n_sus * 1e3}

    if rank == 0:
        t_step = ms_per_step * 1e-3
        line = {
            "metric": "edge tensor-products/sec (forward+force)",
            "value": E * L / t_step,
            "unit": "edge-TP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32" if dtype == torch.float32 else "f64",
            "data": "synthetic" if not emulated else "synthetic; EMULATED kernels on CPU (launch-line test, not a measurement)",
            "config": {"workload": f"{args.workload}: {WORKLOADS[args.workload]['desc']}", "atoms": N, "edges": E,
                       "edges_per_s": E / t_step, "ns_per_day_at_1fs": 0.0864 / t_step,
                       "parallelism": ((f"atom-block x{dist.get_world_size()} over {dist.get_backend()}"
                                        f"{' (RCCL)' if dist.get_backend() == 'nccl' else ''}: slab shards "
                                        + ("from each rank's OWN atoms (HaloShard.from_owned: halo candidates exchanged, no replicated frame)"
                                           if owned_mode else "built from positions alone (owned block + ghost atoms)")
                                        + ", sharded positions, forward + reverse communication of ghost rows (2 all_to_all_single per step)")
                                       if world > 1 and halo else
                                       (f"atom-block x{world}: compact shards (owned block + ghost atoms), one all-reduce of F[N,3]"
                                        if world > 1 else "single GPU")),
                       "weights": "random init (reference initialisers), seed 456"},
        }
        ws = getattr(model, "_workspace", None)
        if ws is not None:
            # the caller-owned arena of the stage-materialised design: its size for this frame, incl. the host's 6 % headroom
            line["config"]["workspace_bytes"] = int(ws.numel())
            line["config"]["workspace_bytes_per_edge"] = float(ws.numel()) / max(1, (e1 - e0))
        if sustained is not None:
            line["config"]["sustained"] = sustained
        if rank_ms is not None:
            line["config"]["rank_ms_per_step"] = rank_ms
        if (args.full or args.stages) and not args.no_profile:
            if halo and shard is not None and pos_local is None:
                pos_local = shard._buffers(dtype, dev)[0]  # (owned + ghost rows as the last timed step left them)
            stages = profile_stages(model, pos if shard is None else (pos_local if halo else pos.index_select(0, shard.local_ids)), graph)
            roof, table = roofline_from_stages(stages, cfg["model_dtype"], args.workload, attach_traffic=shard is None)
            if roof.get("kernel", "").startswith("fused_fwd"):
                # `achieved` prices the REFERENCE's linear-layer flops; the kernel executes fewer since the round-4 folds
                # (DESIGN.md section 3.2): both are stated so that `frac` is not read as matrix-pipe utilisation
                d = model.describe_plan()
                roof["plan"] = d
                if d.get("fused_mfma_steps_reference"):
                    ex = _fused_executed_ratio(d, stages)
                    roof["tail_chain_in_forward"] = _tail_in_forward(stages)
                    roof["executed_fp32_equiv_TFLOPs"] = roof["achieved"] * ex
                    roof["executed_frac"] = roof["frac"] * ex
            roof["peak_at_sustained_clock"] = roof["peak"] * SUSTAINED_CLOCK_GHZ / BOOST_CLOCK_GHZ if roof["bound"] == "mfma" else roof["peak"]
            roof["frac_at_sustained_clock"] = roof["achieved"] / roof["peak_at_sustained_clock"]
            roof["peak_note"] = ("peaks are the guide's, at the 2.4 GHz boost clock; rocm-smi samples during a 6000-step C4 loop show the shader "
                                 "clock at 2.09-2.14 GHz at ~1250 W (profiles/r04_v29_power_clock_samples_c4.txt, tools/power_sample.sh)")
            line["roofline"] = roof
            line["step_roofline"] = step_roofline(cfg, e1 - e0, t_step, stages, cfg["model_dtype"])
            line["step_roofline"]["executed"] = executed_bound(stages, cfg["model_dtype"], t_step, model)
            line["stage_ms"] = table
            line["stage_ms_note"] = ("per-launch HIP-event times of a SEPARATE instrumented pass (aa_model_energy_forces_profiled, mean of 5): "
                                     "the event pairs serialise the launches, so their sum runs ~2 % above ms_per_step of the timed loop")
            if args.stages:
                for nm, ms, nb, fl in stages:
                    print(f"[stage] {nm:24s} {ms * 1e3:9.1f} us {nb / max(ms, 1e-9) / 1e6:8.0f} GB/s (algorithmic)"
                          f"{fl / max(ms, 1e-9) / 1e9:8.1f} TFLOP/s", file=sys.stderr)
        if args.full and world == 1 and g is not None and g.cell is not None:
            # reported separately, never part of `value`: the on-device cell-list build of the same graph
            from allegro_amd.nn import neighbor_list

            ts = []
            for _ in range(4):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                nl = neighbor_list(pos, g.cell, True, cfg["r_max"])
                nl_graph = nl.prepare(types)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t1)
            # (positions here are in the model dtype: a pair within rounding of r_cut may be classified differently
            # from the float64 host list the step was timed on, hence a tolerance instead of equality)
            assert abs(nl.num_edges - E) <= 8, (nl.num_edges, E)
            line["config"]["neighbor_list_device_ms"] = {"edges": nl.num_edges, "list": None,
                                                         "list_plus_graph_prep": sorted(ts[1:])[1] * 1e3}
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            neighbor_list(pos, g.cell, True, cfg["r_max"])
            torch.cuda.synchronize()
            line["config"]["neighbor_list_device_ms"]["list"] = (time.perf_counter() - t1) * 1e3
            del nl_graph
        if (args.full and world == 1 and g is not None and g.cell is not None and WORKLOADS[args.workload]["kind"] == "si" and not args.no_md
                and not args.emulate_shard):
            # the metric's "ns/day for the box" as a measured LOOP (never `value`): list + preparation + hot path + integrator, 40 steps
            md = md_loop(model, pos, types, torch.tensor(g.cell, dtype=torch.float64), float(cfg["r_max"]), steps=40, warmup=5)
            line["config"]["md_loop"] = {k: md[k] for k in ("steps", "dt_fs", "temperature_K", "list_rebuilds", "max_degree_seen", "ms_per_md_step",
                                                            "ms_per_md_step_median", "ns_per_day", "includes", "max_abs_drift_eV",
                                                            "mean_kinetic_eV", "drift_over_mean_kinetic")}
        parity_failed = False
        if args.full and world == 1 and not args.no_cpu_baseline and g is not None:
            # ~20 s of CPU work for the headline model; the l_max=3 fp64 stack is ~10x heavier per edge
            line["cpu_baseline"], line["parity_sample"] = cpu_baseline(g, cfg, model,
                                                                       target_edges=180000 if cfg["l_max"] <= 2 else 24000)
            parity_failed = not line["parity_sample"]["ok"]
        if args.full and world == 1 and not args.no_gpu_reference and not args.emulate_shard and g is not None:
            line["gpu_reference_baseline"] = gpu_reference_baseline(g, cfg, model, dev,
                                                                    target_edges=60000 if cfg["l_max"] <= 2 else 12000)
            line["speedup_vs_gpu_reference"] = line["value"] / line["gpu_reference_baseline"]["value"]
        if (args.full and world == 1 and args.workload == "c4" and not args.no_secondary and not args.no_cpu_baseline and not args.emulate_shard
                and not os.environ.get("AA_BENCH_CELLS")):
            # the other BASELINE workloads in front of the driver: same model family at 10^4 atoms (C3), and the
            # fp64 / l_max 3 / 3-layer / 128-feature / 2-species water box (C5) with its own kernel family
            del graph
            torch.cuda.empty_cache()
            line["secondary"] = {"c3": secondary_workload("c3", dev, steps=50, warmup=5, cpu_edges=60000),
                                 "c5": secondary_workload("c5", dev, steps=5, warmup=2, cpu_edges=56000)}  # (>= 1000 center atoms of the water box)
            parity_failed = parity_failed or not all(v["parity_sample"]["ok"] for v in line["secondary"].values())
        print(json.dumps(line), flush=True)
        if parity_failed:
            print("bench.py: parity_sample outside the north-star tolerance -- the measured number is INVALID", file=sys.stderr)
            if dist is None:
                sys.exit(3)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
