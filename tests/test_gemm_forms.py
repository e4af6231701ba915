"""Every kernel form of the scalar-MLP linear layer against a high-precision host product.

aa_gemm.hip decides in one place (gemm_form) which kernel and launch shape runs a layer, from the shape, the segment
widths, the pointer alignment and the plan options; launch_gemm carries the decision out.  The test hook aa_debug_gemm
(include/allegro_amd.h) takes the full argument surface -- up to 3 A and C segments with their own row strides, silu
(mish, gelu) on all of A or on a 32-granular column range, z (times act'(z)), add, per-segment accumulation, batches
with per-problem weight selection, the plan options -- and reports the form that ran.  Each case of the table below
names the form it must reach; per case:
  * every output element is within its bound of a float64 (fp64 cases: long double) host product -- fp64:
    (K + 3) 2^-53 scale with scale = (sum_k |act(a_k) w_k| + |add|) |act'(z)| + |C_old|, the magnitudes of act and act'
    taken as the sum of the magnitudes of their terms (what bounds their own rounding near a zero); fp32: the bf16x3
    bound of test_gemm_accuracy.py, (4 + sqrt(K) / 2) 2^-23 scale, plus one 2^-23 per epilogue operation (three for act');
  * C padding columns and the rows past M still hold a sentinel, bit for bit;
  * A, z and add padding is NaN, so a padding value that reaches an output fails the case;
  * the inputs are unchanged and a second call gives bit-identical output;
  * the reported form is the named one.
CPU: the same kernels in the test-only emulation build at small M.  GPU: the real kernels at larger M too (rows
sampled for the reference), plus a C5-like 128 -> 640 layer and a layer large enough for the automatic column loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from allegro_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SILU, MISH, GELU, NONE = 0, 1, 2, 3
SENTINEL = -987654.25  # (exact in fp32 and fp64)
FORMS = _lib.GEMM_FORMS


def case(form, dtype, M, a, c, **kw):
    """a / c: A / C segment widths.  pad: extra columns per row of every segment (ld = n + pad).  accum: C segments
    accumulated into.  act: None, "all" or (lo, hi).  null: C segments passed as NULL (computed, not stored).
    misalign: the A segments start one element past a 16-B boundary."""
    d = dict(form=form, dtype=dtype, M=M, a=list(a), c=list(c), pad=4, accum=(), z=False, add=False, act=None, act_kind=SILU,
             batch=0, nw=1, bsel=None, force=0, v1=0, lds=0, rows=0, loop=0, misalign=False, null=())
    d.update(kw)
    return d


F64, F32 = torch.float64, torch.float32
EPI = dict(z=True, add=True, accum=(0,))  # every epilogue operand at once

# the table: small M, run on the emulation build and on the GPU
CASES = [
    # fp64 row-resident, output in accumulators (N <= 128)
    case("F64_ROWS_ACC", F64, 129, [16, 0, 32], [64, 64], act="all", **EPI),  # (an empty A segment)
    case("F64_ROWS_ACC", F64, 33, [320, 320], [16], act=(32, 96)),
    case("F64_ROWS_ACC", F64, 1, [128], [48, 80], accum=(1,)),
    case("F64_ROWS_ACC", F64, 31, [144], [128], z=True, rows=1),
    case("F64_ROWS_ACC", F64, 16, [16, 256], [16, 16, 16], add=True, accum=(2,), pad=0),
    # fp64 row-resident, operand rows in registers (K <= 128)
    case("F64_ROWS_OPND", F64, 127, [64, 64], [16, 192], act="all"),
    case("F64_ROWS_OPND", F64, 31, [16], [48, 96], rows=1, **EPI),
    case("F64_ROWS_OPND", F64, 15, [48], [640], pad=12),
    # fp64 pipelined kernel: 2-D grid and column loop
    case("F64_PIPE_GRID", F64, 129, [16, 256], [144], act=(0, 64), **EPI),
    case("F64_PIPE_GRID", F64, 16, [48], [48], rows=2),
    case("F64_PIPE_GRID", F64, 33, [128], [208], accum=(0,)),  # (K <= 128 but the epilogue reads C: the staged kernel)
    case("F64_PIPE_LOOP", F64, 15, [16, 256], [144], loop=2, **EPI),
    case("F64_PIPE_LOOP", F64, 65, [32, 16], [64, 80], loop=2, act="all"),
    # fp64 plain MFMA kernel: misaligned A, C widths not multiples of 16
    case("F64_MFMA", F64, 33, [32], [8, 24], misalign=True, act="all", **EPI),
    case("F64_MFMA", F64, 64, [32], [6, 26]),
    case("F64_MFMA", F64, 1, [16, 32], [2, 5, 25], accum=(1,), z=True),
    # fp64 VALU kernel: the other activations
    case("F64_VALU", F64, 33, [48], [48], act="all", act_kind=MISH, z=True),
    case("F64_VALU", F64, 31, [16, 32], [16, 6], act="all", act_kind=GELU, add=True, accum=(1,)),
    case("F64_VALU", F64, 16, [64], [32], act=(32, 64), force=3, **EPI),
    # fp64 batches
    case("F64_ROWS_ACC_BATCHED", F64, 17, [32], [16, 32], batch=16, nw=4, accum=(1,), act="all"),
    case("F64_ROWS_ACC_BATCHED", F64, 33, [16, 48], [128], batch=2, nw=2, bsel=[1, 1]),
    case("F64_ROWS_OPND_BATCHED", F64, 20, [64], [144], batch=2, nw=2),
    case("F64_ROWS_OPND_BATCHED", F64, 15, [16], [16, 128], batch=16, nw=3, rows=1, accum=(0,)),
    case("F64_VALU_EACH", F64, 17, [32], [32], batch=2, nw=2, act="all", act_kind=NONE),
    case("F64_MFMA_EACH", F64, 16, [32], [8, 24], batch=2, nw=2, misalign=True),
    case("F64_PIPE_GRID_EACH", F64, 31, [144], [144], batch=2, nw=2, accum=(0,)),
    case("F64_PIPE_LOOP_EACH", F64, 16, [32], [48], batch=16, nw=5, loop=2),
    # fp32 split-precision (bf16x3), direct epilogue; C split 6 | 26 and 8 | 24 (the scalar epilogue path)
    case("F32_BF16X3_K2", F32, 64, [32], [6, 26]),
    case("F32_BF16X3_K2", F32, 64, [32], [8, 24], **EPI),
    case("F32_BF16X3_K2", F32, 33, [32, 32], [1, 2, 29], act=(32, 64), accum=(1,)),
    case("F32_BF16X3_K4", F32, 129, [64, 64], [16, 32], act="all", **EPI),
    case("F32_BF16X3_KS", F32, 33, [320, 0, 320], [48], act=(64, 320)),
    case("F32_BF16X3_KS", F32, 16, [160], [6, 58], z=True, accum=(0, 1)),
    # fp32 bf16x3, epilogue through LDS
    case("F32_BF16X3_LDS_K2", F32, 31, [64], [32, 32], lds=1, **EPI),
    case("F32_BF16X3_LDS_K4", F32, 127, [96], [48], lds=1, act="all"),
    case("F32_BF16X3_LDS_KS", F32, 15, [32, 128], [64, 16], lds=1, accum=(1,)),
    case("F32_BF16X3_K2", F32, 16, [64], [30, 2], lds=1, add=True),  # (LDS epilogue asked for, C not 4-granular)
    # fp32-input MFMA, operands straight from memory (A segments 16- but not 32-granular, or forced)
    case("F32_V3_K2", F32, 64, [32], [6, 26], force=1),
    case("F32_V3_K2", F32, 33, [16, 32], [8, 24], **EPI),
    case("F32_V3_K4", F32, 129, [48, 80], [32], act="all", z=True),
    case("F32_V3_KS", F32, 16, [144, 128], [96, 48], act=(0, 32), accum=(0,)),
    # fp32-input MFMA, LDS-staged operands
    case("F32_MFMA_V1", F32, 33, [32], [6, 26], v1=1, **EPI),
    case("F32_MFMA_V1", F32, 31, [16, 32], [48], misalign=True, act="all"),
    # fp32 VALU
    case("F32_VALU", F32, 33, [48], [48], act="all", act_kind=MISH, z=True),
    case("F32_VALU", F32, 16, [32, 16], [16, 6], act="all", act_kind=GELU, add=True, accum=(1,)),
    case("F32_VALU", F32, 1, [64], [32], force=3, **EPI),
    # fp32 batches
    case("F32_BF16X3_BATCHED_K2", F32, 33, [32], [16, 16], batch=16, nw=4, accum=(0,)),
    case("F32_BF16X3_BATCHED_K4", F32, 17, [64, 32], [64], batch=2, nw=2, bsel=[1, 1], act="all"),
    case("F32_BF16X3_BATCHED_KS", F32, 16, [160], [6, 26], batch=2, nw=2),
    case("F32_BF16X3_LDS_EACH", F32, 16, [64], [32], batch=2, nw=2, lds=1),
    case("F32_V3_EACH", F32, 17, [16, 16], [32], batch=2, nw=2, accum=(0,)),
    case("F32_MFMA_V1_EACH", F32, 16, [32], [32], batch=16, nw=3, v1=1),
    case("F32_VALU_EACH", F32, 16, [32], [6, 26], batch=2, nw=2, act="all", act_kind=GELU),
    # nothing to do
    case("NONE", F64, 0, [32], [32]),
    case("NONE", F32, 0, [32], [32]),
]

# a C segment passed as NULL is computed but not stored (emulation only: a wrong store would go through a null pointer)
NULL_CASES = [
    case("F32_BF16X3_K2", F32, 33, [32], [6, 26], null=(0,)),
    case("F32_BF16X3_K2", F32, 33, [32], [32, 32], null=(1,), z=True),
    case("F32_BF16X3_LDS_K2", F32, 33, [32], [32, 32], null=(0,), lds=1),
    case("F32_V3_K2", F32, 16, [16], [8, 24], null=(1,)),
    case("F32_MFMA_V1", F32, 16, [32], [8, 24], null=(0,), v1=1),
    case("F32_VALU", F32, 16, [32], [8, 24], null=(0,), force=3),
    case("F64_ROWS_ACC", F64, 16, [32], [16, 32], null=(0,)),
    case("F64_ROWS_OPND", F64, 16, [32], [16, 144], null=(1,)),
    case("F64_PIPE_GRID", F64, 16, [32], [16, 48], null=(0,), rows=2),
    case("F64_MFMA", F64, 16, [32], [6, 26], null=(0,)),
]

# GPU only: the table's layouts at a few thousand rows, a C5-like 128 -> 640 layer and the automatic column loop
GPU_M = 4099
GPU_CASES = [
    case("F64_ROWS_OPND", F64, 20011, [128], [640], act="all"),
    case("F32_BF16X3_K4", F32, 20011, [128], [640], act="all"),
    case("F64_ROWS_ACC", F64, 20011, [640], [128], act="all", **EPI),
    case("F64_PIPE_LOOP", F64, 262144, [16, 256], [192], act="all", pad=0),
]


def _ids(cases):
    return [f"{c['form']}-{i}" for i, c in enumerate(cases)]


def _np(dtype):
    return np.float64 if dtype == F64 else np.float32


def _bits(x):
    return x.view(np.int64 if x.dtype == np.float64 else np.int32)


def _act(kind, x):
    t = torch.from_numpy(x)
    if kind == SILU:
        r, m = t * torch.sigmoid(t), (t * torch.sigmoid(t)).abs()
    elif kind == MISH:
        r = t * torch.tanh(torch.where(t > 30, t, torch.log1p(torch.exp(t))))
        m = r.abs()
    elif kind == GELU:
        e = torch.special.erf(t * 0.70710678118654752440)
        r, m = 0.5 * t * (1 + e), 0.5 * t.abs() * (1 + e.abs())
    else:
        r, m = t, t.abs()
    return r.numpy(), m.numpy()


def _grad(kind, z):
    """act'(z) and the sum of the magnitudes of its terms."""
    t = torch.from_numpy(z)
    if kind == SILU:
        s = torch.sigmoid(t)
        r, m = s * (1 + t * (1 - s)), s * (1 + t.abs() * (1 - s))
    elif kind == MISH:
        th = torch.tanh(torch.where(t > 30, t, torch.log1p(torch.exp(t))))
        sg = torch.sigmoid(t)
        r, m = th + t * (1 - th * th) * sg, th.abs() + t.abs() * (1 - th * th) * sg
    elif kind == GELU:
        cdf = 0.5 * (1 + torch.special.erf(t * 0.70710678118654752440))
        pdf = 0.39894228040143267794 * torch.exp(-0.5 * t * t)
        r, m = cdf + t * pdf, cdf + t.abs() * pdf
    else:
        r = m = torch.ones_like(t)
    return r.numpy(), m.numpy()


class _Segs:
    """One segment list: a host buffer per segment holding `problems` problems of M rows (+ one spare row) at a common
    element stride `bs`; everything outside the [M, n] views is padding."""

    def __init__(self, widths, pad, M, problems, np_dtype, fill, offset=0):
        self.n = list(widths)
        self.ld = [n + pad if n + pad > 0 else 4 for n in self.n]
        self.M, self.P, self.off = M, problems, offset
        self.bs = (M + 1) * max(self.ld)
        self.bs += (-self.bs) % 4  # (keeps every problem's rows 16-B aligned)
        self.bufs = [np.full(offset + (problems - 1) * self.bs + (M + 1) * ld, fill, dtype=np_dtype) for ld in self.ld]

    def view(self, s, b):
        o = self.off + b * self.bs
        return self.bufs[s][o:o + self.M * self.ld[s]].reshape(self.M, self.ld[s])[:, :self.n[s]]

    def valid(self, s):
        m = np.zeros(self.bufs[s].shape, dtype=bool)
        for b in range(self.P):
            o = self.off + b * self.bs
            m[o:o + self.M * self.ld[s]].reshape(self.M, self.ld[s])[:, :self.n[s]] = True
        return m

    def cat(self, b, rows):
        return np.concatenate([self.view(s, b)[rows] for s in range(len(self.n))], axis=1)


def _run_case(lib, dev, cs, M=None, seed=0):
    M = cs["M"] if M is None else M
    npd = _np(cs["dtype"])
    rng = np.random.default_rng(seed)
    K, N = sum(cs["a"]), sum(cs["c"])
    P = max(cs["batch"], 1)
    nw = cs["nw"]
    bsel = cs["bsel"] if cs["bsel"] is not None else [int(rng.integers(0, nw)) for _ in range(P)] if P > 1 else [0]
    w = (rng.standard_normal((nw, K, N)) / np.sqrt(K)).astype(npd)

    A = _Segs(cs["a"], cs["pad"], M, P, npd, np.nan, offset=1 if cs["misalign"] else 0)
    Cs = _Segs(cs["c"], cs["pad"], M, P, npd, SENTINEL)
    Z = _Segs(cs["c"], cs["pad"] + 4, M, P, npd, np.nan) if cs["z"] else None
    AD = _Segs(cs["c"], cs["pad"] + 8, M, P, npd, np.nan) if cs["add"] else None
    for b in range(P):
        for s in range(len(cs["a"])):
            A.view(s, b)[:] = rng.standard_normal((M, cs["a"][s]))
        for s in range(len(cs["c"])):
            # not accumulated into: NaN, so an element that is never written fails its bound
            Cs.view(s, b)[:] = rng.standard_normal((M, cs["c"][s])) if s in cs["accum"] else np.nan
            if Z is not None:
                Z.view(s, b)[:] = 1.5 * rng.standard_normal((M, cs["c"][s]))
            if AD is not None:
                AD.view(s, b)[:] = rng.standard_normal((M, cs["c"][s]))

    def upload(segs):
        return [torch.from_numpy(x.copy()).to(dev) for x in segs.bufs] if segs is not None else None

    dA, dC, dZ, dAD = upload(A), upload(Cs), upload(Z), upload(AD)
    isz = np.dtype(npd).itemsize

    def segarr(segs, dbufs, null=()):
        arr = (_lib.GemmSeg * 3)()
        for s in range(len(segs.n)):
            p = None if s in null else dbufs[s].data_ptr() + segs.off * isz
            arr[s] = _lib.GemmSeg(p, segs.ld[s], segs.n[s])
        return arr

    d = _lib.GemmDesc()
    d.dtype = _lib.AA_F64 if npd == np.float64 else _lib.AA_F32
    d.M, d.K, d.N = M, K, N
    d.a_count, d.c_count = len(cs["a"]), len(cs["c"])
    d.a = segarr(A, dA)
    d.c = segarr(Cs, dC, cs["null"])
    for s in cs["accum"]:
        d.c_accum[s] = 1
    d.has_z, d.has_add = int(cs["z"]), int(cs["add"])
    if Z is not None:
        d.z = segarr(Z, dZ)
    if AD is not None:
        d.add = segarr(AD, dAD)
    act = cs["act"]
    d.act_a = int(act is not None)
    d.act_lo, d.act_hi = (0, 0) if act in (None, "all") else act
    d.act_kind = cs["act_kind"]
    d.batch = cs["batch"]
    d.a_bs, d.c_bs = (A.bs, Cs.bs) if P > 1 else (0, 0)
    d.bsel4 = sum(sel << (4 * b) for b, sel in enumerate(bsel)) if P > 1 else 0
    d.num_weights = nw
    d.weights = w.ctypes.data
    d.force_kernel, d.v1, d.lds_epilogue, d.f64_rows, d.f64_column_loop = cs["force"], cs["v1"], cs["lds"], cs["rows"], cs["loop"]
    form = C.c_int32(-1)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0

    def call():
        lib.check(lib.lib.aa_debug_gemm(C.byref(d), C.byref(form), stream), "aa_debug_gemm")
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        return [x.cpu().numpy() for x in dC]

    out = call()
    name = f"{cs['form']} M={M}"
    assert form.value == FORMS[cs["form"]], f"{name}: ran form {form.value}, expected {FORMS[cs['form']]}"

    # the inputs are unchanged
    for host, devb, what in ((A, dA, "A"), (Z, dZ, "z"), (AD, dAD, "add")):
        if host is not None:
            for s, x in enumerate(devb):
                assert np.array_equal(_bits(x.cpu().numpy()), _bits(host.bufs[s])), f"{name}: {what} segment {s} modified"
    # C padding, rows past M and the null segments' buffers: the sentinel, bit for bit
    for s in range(len(cs["c"])):
        pad = ~Cs.valid(s) if s not in cs["null"] else np.ones(Cs.bufs[s].shape, dtype=bool)
        bad = np.nonzero(_bits(out[s])[pad] != _bits(Cs.bufs[s])[pad])[0]
        assert bad.size == 0, f"{name}: C segment {s}: {bad.size} padding / unstored elements written, e.g. buffer offsets {np.nonzero(pad)[0][bad[:8]]}"

    # values against the host product (fp64: long double), rows sampled when M is large
    rows = np.arange(M) if M <= 2048 else np.unique(np.concatenate([np.arange(40), np.arange(M - 40, M), rng.integers(0, M, 400)]))
    hp = np.longdouble if npd == np.float64 else np.float64
    amask = np.zeros(K, dtype=bool)
    if act == "all":
        amask[:] = True
    elif act is not None:
        amask[act[0]:act[1]] = True
    cols = np.concatenate([np.full(n, s) for s, n in enumerate(cs["c"])]).astype(int) if N else np.zeros(0, int)
    acc_cols = np.isin(cols, list(cs["accum"]))
    stored = ~np.isin(cols, list(cs["null"]))
    ops = (1 if cs["add"] else 0) + (3 if cs["z"] else 0) + (1 if cs["accum"] else 0)
    for b in range(P):
        if M == 0:
            break
        a = A.cat(b, rows).astype(np.float64)
        am = np.abs(a)
        if act is not None:
            r, m = _act(cs["act_kind"], np.ascontiguousarray(a[:, amask]))
            a[:, amask], am[:, amask] = r, m
        wb = w[bsel[b]].astype(np.float64)
        ref = a.astype(hp) @ wb.astype(hp)
        scale = am @ np.abs(wb)
        if AD is not None:
            ad = AD.cat(b, rows).astype(np.float64)
            ref = ref + ad
            scale = scale + np.abs(ad)
        if Z is not None:
            g, gm = _grad(cs["act_kind"], Z.cat(b, rows).astype(np.float64))
            ref = ref * g
            scale = scale * gm
        cold = np.concatenate([Cs.view(s, b)[rows] for s in range(len(cs["c"]))], axis=1).astype(np.float64)
        cold = np.where(acc_cols[None, :], cold, 0.0)
        ref = ref + cold
        scale = scale + np.abs(cold)
        if npd == np.float64:
            bound = (K + 3) * 2.0 ** -53 * scale
        else:
            bound = (4.0 + 0.5 * np.sqrt(K) + ops) * 2.0 ** -23 * scale
        got = np.concatenate([np.asarray(out[s][Cs.off + b * Cs.bs:][:M * Cs.ld[s]].reshape(M, Cs.ld[s])[rows, :n]) for s, n in enumerate(cs["c"])], axis=1).astype(np.float64)
        err = np.abs(got - ref.astype(np.float64))
        bad = ~(err <= bound) & stored[None, :]
        if bad.any():
            r_, c_ = np.nonzero(bad)
            where = [(b, int(rows[i]), int(j), float(got[i, j])) for i, j in zip(r_[:8], c_[:8])]
            raise AssertionError(f"{name}: {bad.sum()} outputs off their bound or unwritten (NaN), (problem, row, column, value): {where}")

    # a second call (C reset) is bit-identical
    for s, x in enumerate(dC):
        x.copy_(torch.from_numpy(Cs.bufs[s]).to(dev))
    again = call()
    for s in range(len(cs["c"])):
        assert np.array_equal(_bits(again[s]), _bits(out[s])), f"{name}: C segment {s} differs between two calls"
    return form.value


def test_form_enum_matches_header():
    src = open(os.path.join(ROOT, "include", "allegro_amd.h")).read()
    hdr = {("NONE" if k == "FORM_NONE" else k): int(v) for k, v in re.findall(r"\bAA_GEMM_(\w+)\s*=\s*(\d+)", src)}
    assert hdr == FORMS


def test_cases_reach_every_form():
    """A new form cannot land untested: the table's cases together name every aa_gemm_form."""
    named = {c["form"] for c in CASES + GPU_CASES}
    assert named == set(FORMS), sorted(set(FORMS) - named)


@pytest.mark.parametrize("cs", CASES + NULL_CASES, ids=_ids(CASES + NULL_CASES))
def test_form_emulated(cs):
    from tests.hip_utils import emu_lib

    _run_case(emu_lib(), torch.device("cpu"), cs)


@pytest.mark.gpu
@pytest.mark.parametrize("cs", CASES + GPU_CASES, ids=_ids(CASES + GPU_CASES))
def test_form_on_gpu(cs):
    lib, dev = _lib.load(), torch.device("cuda:0")
    _run_case(lib, dev, cs)
    if cs in CASES and cs["M"] > 0:
        _run_case(lib, dev, cs, M=GPU_M, seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("c,epi", [([6, 26], {}), ([32, 96], EPI), ([8, 24], dict(z=True))])
def test_fp32_forms_against_each_other_on_gpu(c, epi):
    """As in test_gemm_accuracy.py: the split-precision forms may not be further from the fp64 product than the native
    fp32-input MFMA kernel is (2x + one ulp of the row scale) -- here with segmented C and the epilogue operands."""
    lib, dev = _lib.load(), torch.device("cuda:0")
    errs = {}
    for form, kw in (("F32_MFMA_V1", dict(v1=1)), ("F32_BF16X3_K4", {}), ("F32_V3_K4", dict(force=1)),
                     ("F32_BF16X3_LDS_K4", dict(lds=1))):
        if form == "F32_BF16X3_LDS_K4" and any(n % 4 for n in c):
            continue  # (the LDS epilogue needs 4-granular C segments)
        cs = case(form, F32, GPU_M, [128], c, act="all", **kw, **epi)
        errs[form] = _fp32_err(lib, dev, cs)
    for form, e in errs.items():
        assert e <= 2.0 * errs["F32_MFMA_V1"] + 2.0 ** -23, (form, errs)


def _fp32_err(lib, dev, cs):
    """max |got - ref| / scale of one fp32 layer, contiguous operands (the same for every form: the seed is fixed)."""
    rng = np.random.default_rng(3)
    M, K, N = cs["M"], sum(cs["a"]), sum(cs["c"])
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    z = (1.5 * rng.standard_normal((M, N))).astype(np.float32)
    ad = rng.standard_normal((M, N)).astype(np.float32)
    c0 = rng.standard_normal((M, N)).astype(np.float32)
    ta = torch.from_numpy(a).to(dev)
    tz, tad = torch.from_numpy(z).to(dev), torch.from_numpy(ad).to(dev)
    tc = torch.from_numpy(c0).to(dev)

    def segs(t, widths):
        arr, o = (_lib.GemmSeg * 3)(), 0
        for s, n in enumerate(widths):
            arr[s] = _lib.GemmSeg(t.data_ptr() + 4 * o, N, n)
            o += n
        return arr

    d = _lib.GemmDesc()
    d.dtype, d.M, d.K, d.N = _lib.AA_F32, M, K, N
    d.a_count, d.c_count = 1, len(cs["c"])
    d.a[0] = _lib.GemmSeg(ta.data_ptr(), K, K)
    d.c = segs(tc, cs["c"])
    for s in cs["accum"]:
        d.c_accum[s] = 1
    d.has_z, d.has_add = int(cs["z"]), int(cs["add"])
    if cs["z"]:
        d.z = segs(tz, cs["c"])
    if cs["add"]:
        d.add = segs(tad, cs["c"])
    d.act_a, d.act_kind = 1, SILU
    d.num_weights, d.weights = 1, w.ctypes.data
    d.force_kernel, d.v1, d.lds_epilogue = cs["force"], cs["v1"], cs["lds"]
    form = C.c_int32(-1)
    lib.check(lib.lib.aa_debug_gemm(C.byref(d), C.byref(form), torch.cuda.current_stream(dev).cuda_stream), "aa_debug_gemm")
    assert form.value == FORMS[cs["form"]], (cs["form"], form.value)
    got = tc.cpu().numpy().astype(np.float64)
    x, xm = _act(SILU, a.astype(np.float64))
    ref, scale = x @ w.astype(np.float64), xm @ np.abs(w.astype(np.float64))
    accm = np.zeros(N, dtype=bool)
    o = 0
    for s, n in enumerate(cs["c"]):
        accm[o:o + n] = s in cs["accum"]
        o += n
    if cs["add"]:
        ref, scale = ref + ad, scale + np.abs(ad)
    if cs["z"]:
        g, gm = _grad(SILU, z.astype(np.float64))
        ref, scale = ref * g, scale * gm
    cold = np.where(accm[None, :], c0.astype(np.float64), 0.0)
    ref, scale = ref + cold, scale + np.abs(cold)
    return float(np.max(np.abs(got - ref) / scale))
