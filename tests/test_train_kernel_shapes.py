"""The training kernels of csrc/aa_train.hip (and `aa_linear_forward`) by value at the shapes where their paths change.

`tests/test_train_kernels.py` reaches these kernels through the torch ops at a handful of shapes (and keeps the second-order and
autograd-closure checks).  This module calls the C ABI directly, through `allegro_amd._lib` and ctypes, on buffers it owns:

* weighted channels (`aa_weighted_channels` which 0 / 1 / 2, `_sum`, `_pair`): fp32 and fp64, l_max 0..3, shared and per-irrep
  weights, u in 1, 3, 63, 64, 65, 128, 129, 257 (channels on lanes, 64 per pass), E in 0, 1, 4, 5, 15, 16, 17, 33 (4 edges per
  workgroup of `wc_grad_sh`, 4 per wave and 16 per workgroup of the pair kernel, G <= 16 of the slot forward, 8 of the general one),
  the weight operand contiguous and as a column block at offset 3 of a wider matrix; every slot count of the slot forward
  (ceil(u D / 256) = 1..8) and the first row past it, with one and two terms; a group of one edge by the 32-KB rule and by the
  clamp alone (the emulated grid leaves out u 3, 129 and E 5, 15 for its time: 154 s on six workers with them, 116 s without);
* `aa_linear_wgrad`: E at the stage (16 / 32 rows) and slab (64 rows) boundaries, exactly two slabs and one row either side, 64- and
  128-wide blocks with ragged edges, vector staging and each of its six conditions broken alone;
* the activation family (`aa_silu_derivative(_pair)`, `aa_act_derivative(_pair)`): silu / mish / gelu, orders 0..3, n around the
  vector width and the workgroup size, and arguments where exp overflows and underflows in fp32;
* `aa_scalar_column`: the three templated row lengths and the run-time division, rows D mod 4 = 0..3, across a workgroup;
* `aa_concat_columns`: 1, 2 and 8 inputs, each condition of the 16-byte path broken alone, a row stride longer than the row;
* `aa_linear_forward`: rows around its 128-row tile, K on both sides of the held / streamed operand limits (64, 128), a transposed
  weight view, row-strided operand and output, and the shapes `ops.linear` keeps on the library GEMM.

Every output and workspace is NaN before the call and has a guard of 64 NaN elements behind it: afterwards the payload holds no NaN
and the guard (and the padding columns of a strided output) is untouched; a refused call and a call without rows write nothing.
Workspaces have exactly the size the entry point's own size function returns.  On the emulation backend every INPUT ends at (where
an alignment is asked for: less than 16 bytes before) a page without access, so a read behind an operand is a fault there -- several
of these kernels guard their stores but not their loads by construction, and a load behind the end changes no value.

Reference: the plain fp64 torch expression on the CPU (broadcasting and autograd for the weighted channels, `x^T g`, autograd through
`torch.nn.functional.silu / mish / gelu` -- at the fixed large arguments mpmath's derivatives of the same functions, which that
autograd has to match wherever it is finite -- slicing and `torch.cat`).  Tolerances are the project's: fp64 weighted channels
1e-12 x max(1, max |expected|); fp32 `err_hip <= 2 err_cpu32 + 1e-5 scale` (tests/fastpath_utils.py) with the same expression in
fp32 on the CPU; `aa_linear_wgrad` tol x scale x sqrt(max(1, E)), tol 2e-6 / 1e-13; activations 1e-12 (silu) / 1e-11 (fp64),
2e-5 (fp32) of max(1, max |expected|); `aa_linear_forward` 3e-6 sqrt(K) max |expected| (tests/test_train_kernels.py); copies exact.
What sums in a fixed order is bit-equal across two identical calls.

`-s` prints `case quantity err_hip err_cpu32 scale` (the worst of a case over its row counts and operand layouts); DESIGN.md
section 5 quotes the worst ratios."""
import ctypes
import mmap

import pytest
import torch

from allegro_amd import _lib
from tests.fastpath_utils import oracle64_errors

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
DTYPES = {"f32": torch.float32, "f64": torch.float64}
GUARD = 64
NAN = float("nan")
AA_ERR_INVALID = -1


def _backend(name):
    if name == "emu":
        from tests.hip_utils import emu_lib

        return emu_lib(), torch.device("cpu")
    assert torch.cuda.is_available()
    return _lib.load(), torch.device("cuda:0")


# ---- caller-owned buffers ------------------------------------------------------------------------------------------------------
_LIBC = ctypes.CDLL(None, use_errno=True)
_LIBC.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]


def _fenced(src, mod16):
    """A host copy of the flat tensor `src` whose last element ends at a page without access (address % 16 == mod16: up to 15 bytes
    of slack before that page)."""
    nbytes, page = src.numel() * src.element_size(), mmap.PAGESIZE
    pages = (nbytes + 16 + page - 1) // page
    mm = mmap.mmap(-1, (pages + 1) * page)
    hold = ctypes.c_char.from_buffer(mm)
    base = ctypes.addressof(hold)
    assert base % page == 0
    if _LIBC.mprotect(base + pages * page, page, 0) != 0:
        raise OSError(ctypes.get_errno(), "mprotect")
    del hold
    start = pages * page - nbytes
    start -= (start - mod16) % 16
    t = torch.frombuffer(mm, dtype=src.dtype, count=src.numel(), offset=start)  # (keeps the mapping alive)
    t.copy_(src)
    assert t.data_ptr() % 16 == mod16 and t.data_ptr() + nbytes + 16 > base + pages * page
    return t


class Ctx:
    """One backend and dtype: inputs, poisoned outputs, calls."""

    def __init__(self, backend, dtype):
        self.lib, self.dev = _backend(backend)
        self.L = self.lib.lib
        self.dtype = dtype
        self.code = _lib.AA_F32 if dtype == torch.float32 else _lib.AA_F64
        self.esize = 4 if dtype == torch.float32 else 8
        self.gpu = self.dev.type == "cuda"
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream if self.gpu else None

    def inp(self, src, mod16=None):
        """The elements of `src`, flat, where the kernels read them; None for no elements (what `data_ptr()` of an empty tensor is).
        mod16: the address modulo 16 where the entry point cares; None: wherever the last element ends at the page without access."""
        src = src.reshape(-1)
        mod16 = (-src.numel() * self.esize) % 16 if mod16 is None else mod16
        assert src.dtype == self.dtype and mod16 % self.esize == 0
        if src.numel() == 0:
            return None
        if not self.gpu:
            return _fenced(src, mod16)
        k = mod16 // self.esize
        t = torch.empty(src.numel() + 4, dtype=self.dtype, device=self.dev)[k:k + src.numel()]
        t.copy_(src)
        assert t.data_ptr() % 16 == mod16
        return t

    def poisoned(self, n, skip=0):
        """(n + GUARD NaNs, n); skip: elements the buffer starts behind a 16-byte boundary."""
        buf = torch.full((n + GUARD + skip,), NAN, dtype=self.dtype, device=self.dev)[skip:]
        assert buf.data_ptr() % 16 == (skip * self.esize) % 16
        return buf, n

    def call(self, fn, *args):
        return fn(*args, self.stream)

    def taken(self, what, buf, n, written=True):
        """The payload of a buffer behind a call, on the host: the guard untouched, and no NaN left in the payload (written) or
        nothing but NaN (not written)."""
        host = buf.cpu()
        assert torch.isnan(host[n:]).all(), f"{what}: wrote behind its {n} elements"
        if written:
            assert not torch.isnan(host[:n]).any(), f"{what}: {int(torch.isnan(host[:n]).sum())} of {n} elements never written"
        else:
            assert torch.isnan(host[:n]).all(), f"{what}: written"
        return host[:n]


def ptr(t, elems=0):
    return None if t is None else t.data_ptr() + elems * t.element_size()


# ---- the rules, and the log ----------------------------------------------------------------------------------------------------
class Log:
    """The worst comparison (nearest to its bound) of every quantity of a case; printed once per case."""

    def __init__(self, case):
        self.case, self.worst = case, {}

    def add(self, what, err_hip, err_cpu32, scale, bound):
        frac = err_hip / bound if bound > 0 else 0.0
        if what not in self.worst or frac > self.worst[what][3]:
            self.worst[what] = (err_hip, err_cpu32, scale, frac)

    def flush(self):
        for what, (err_hip, err_cpu32, scale, frac) in self.worst.items():
            print(f"{self.case} {what} err_hip {err_hip:.3e} err_cpu32 {err_cpu32:.3e} scale {scale:.3e} of_bound {frac:.3f}")


def check(log, where, what, got, w32, w64, tol64):
    """fp64 (w32 None): within tol64 x max(1, max |w64|); fp32: not further from w64 than twice w32 is, + 1e-5 of the scale."""
    assert got.shape == w64.shape and torch.isfinite(got).all(), (log.case, where, what)
    if w32 is None:
        scale = max(1.0, float(w64.abs().max())) if w64.numel() else 1.0
        err = (got - w64).abs().max().item() if w64.numel() else 0.0
        log.add(what, err, 0.0, scale, tol64 * scale)
        assert err <= tol64 * scale, (log.case, where, what, err, scale)
        return
    err_hip, err_cpu32, scale = oracle64_errors(got, w32, w64)
    log.add(what, err_hip, err_cpu32, scale, 2.0 * err_cpu32 + 1e-5 * scale)
    assert err_hip <= 2.0 * err_cpu32 + 1e-5 * scale, (log.case, where, what, err_hip, err_cpu32, scale)


def check_abs(log, where, what, got, w64, bound, err_cpu32=0.0):
    """A bound the caller states in absolute terms (tol x scale [x sqrt E])."""
    assert got.shape == w64.shape and torch.isfinite(got).all(), (log.case, where, what)
    err = (got.double() - w64).abs().max().item() if w64.numel() else 0.0
    log.add(what, err, err_cpu32, max(1.0, float(w64.abs().max())) if w64.numel() else 1.0, bound)
    assert err <= bound, (log.case, where, what, err, bound)


# =================================================================================================================================
# 1. weighted channels
# =================================================================================================================================
WC_U = (1, 3, 63, 64, 65, 128, 129, 257)
WC_E = (0, 1, 4, 5, 15, 16, 17, 33)
WC_U_THIN, WC_E_THIN = (3, 129), (5, 15)  # left out of the emulated grid (its time)
WC_PAD = (3, 5)  # columns in front of and behind the weight block of the wider matrix
K_WC_SLOTS, K_WC_MAX_GROUP, K_WC_LDS_BYTES = 8, 16, 32768  # (aa_train.hip)


def wc_expand(w, u, l_max, shared):
    """[E, u R] -> [E, u, D]: the weight of every component (tests/test_train_kernels.py)."""
    E = w.shape[0]
    if shared:
        return w.reshape(E, u, 1).expand(-1, -1, (l_max + 1) ** 2)
    wr = w.reshape(E, u, l_max + 1)
    return torch.cat([wr[:, :, l:l + 1].expand(-1, -1, 2 * l + 1) for l in range(l_max + 1)], dim=-1)


_WC = {}


def wc_data(u, l_max, shared, dtype, E):
    """Inputs of E edges and the reference {quantity: (fp32 | None, fp64)}, once per shape; every row is independent of the others, so
    the case of fewer edges is the leading rows."""
    key = (u, l_max, shared, dtype, E)
    if key in _WC:
        return _WC[key]
    D, R = (l_max + 1) ** 2, 1 if shared else l_max + 1
    g = torch.Generator().manual_seed(77 + 1000 * u + 10 * l_max + int(shared))
    d = dict(sh=torch.randn(E, D, dtype=dtype, generator=g), w=torch.randn(E, u * R, dtype=dtype, generator=g),
             t=torch.randn(E, u, D, dtype=dtype, generator=g), sh2=torch.randn(E, D, dtype=dtype, generator=g),
             w2=torch.randn(E, u * R, dtype=dtype, generator=g), pad=torch.randn(E, sum(WC_PAD), dtype=dtype, generator=g) + 100.0)

    def evaluate(dt):
        sh, w = d["sh"].to(dt).requires_grad_(True), d["w"].to(dt).requires_grad_(True)
        out = sh.unsqueeze(1) * wc_expand(w, u, l_max, shared)
        gsh, gw = torch.autograd.grad(out, [sh, w], d["t"].to(dt))
        both = out.detach() + d["sh2"].to(dt).unsqueeze(1) * wc_expand(d["w2"].to(dt), u, l_max, shared)
        return dict(fwd=out.detach(), gw=gw, gsh=gsh, sum=both)

    r64 = evaluate(torch.float64)
    r32 = evaluate(torch.float32) if dtype == torch.float32 else {k: None for k in r64}
    d["ref"] = {k: (r32[k], r64[k]) for k in r64}
    _WC[key] = d
    return d


def wc_ref(d, q, E):
    w32, w64 = d["ref"][q]
    return (None if w32 is None else w32[:E]), w64[:E]


class WcCase:
    """The operands of E edges of one shape on the backend; `wide`: the weights as columns 3.. of a wider matrix."""

    def __init__(self, ctx, d, E, u, l_max, shared, wide):
        self.ctx, self.E, self.u, self.l_max, self.shared = ctx, E, u, l_max, int(shared)
        self.D, self.R = (l_max + 1) ** 2, 1 if shared else l_max + 1
        self.sh, self.sh2, self.t = (ctx.inp(d[k][:E]) for k in ("sh", "sh2", "t"))
        wrow = u * self.R
        self.ldw, self.off = (wrow + sum(WC_PAD), WC_PAD[0]) if wide else (wrow, 0)
        self.w, self.w2 = (self._weights(d[k][:E], d["pad"][:E], wide) for k in ("w", "w2"))
        assert E == 0 or not wide or ptr(self.w, self.off) % 16 != 0

    def _weights(self, w, pad, wide):
        if not wide or self.E == 0:
            return self.ctx.inp(w)
        m = torch.cat([pad[:, :WC_PAD[0]], w, pad[:, WC_PAD[0]:]], dim=1)
        return self.ctx.inp(m.reshape(-1)[:m.numel() - WC_PAD[1]], 0)  # (a 16-byte-aligned matrix; ends with the last row's weights)

    def single(self, which, what, written=True, expect=0):
        """`aa_weighted_channels`: the payload (or, refused / no rows: nothing written)."""
        c = self.ctx
        a, b = (self.sh, self.w) if which == 0 else ((self.t, self.sh) if which == 1 else (self.t, self.w))
        n = self.E * (self.u * self.D if which == 0 else (self.u * self.R if which == 1 else self.D))
        out, n = c.poisoned(n)
        # (which 1 has no weight operand: its ldw is ignored)
        rc = c.call(c.L.aa_weighted_channels, c.code, which, self.E, self.u, self.l_max, self.shared, ptr(a), ptr(b, 0 if which == 1 else self.off),
                    0 if which == 1 else self.ldw, ptr(out))
        assert rc == expect, (what, rc, c.L.aa_last_error())
        return c.taken(what, out, n, written=written and self.E > 0)

    def both(self, what, written=True, expect=0):
        c = self.ctx
        out, n = c.poisoned(self.E * self.u * self.D)
        rc = c.call(c.L.aa_weighted_channels_sum, c.code, self.E, self.u, self.l_max, self.shared, ptr(self.sh), ptr(self.w, self.off), self.ldw,
                    ptr(self.sh2), ptr(self.w2, self.off), self.ldw, ptr(out))
        assert rc == expect, (what, rc, c.L.aa_last_error())
        return c.taken(what, out, n, written=written and self.E > 0)

    def pair(self, what, written=True, expect=0):
        c = self.ctx
        osh, nsh = c.poisoned(self.E * self.D)
        ow, nw = c.poisoned(self.E * self.u * self.R)
        rc = c.call(c.L.aa_weighted_channels_pair, c.code, self.E, self.u, self.l_max, self.shared, ptr(self.t), ptr(self.sh), ptr(self.w, self.off),
                    self.ldw, ptr(osh), ptr(ow))
        assert rc == expect, (what, rc, c.L.aa_last_error())
        return c.taken(what + " gsh", osh, nsh, written=written and self.E > 0), c.taken(what + " gw", ow, nw, written=written and self.E > 0)


def close(log, where, what, a, b, ref):
    """Two forms of one quantity that need not sum in the same order: as far apart as two results within the rule of `check` may be."""
    w32, w64 = ref
    scale = max(1.0, float(w64.abs().max()))
    bound = 1e-12 * scale if w32 is None else 2.0 * (w32.double() - w64).abs().max().item() + 1e-5 * scale
    err = float((a - b).abs().max())
    assert err <= bound, (log.case, where, what, err, bound)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shared", [0, 1], ids=["per_irrep", "shared"])
@pytest.mark.parametrize("l_max", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_weighted_channels_grid(dtype, l_max, shared, backend):
    """Every entry point at every (u, E, weight layout); the pair form against the single forms: `out_w` bit for bit, `out_sh` bit for
    bit where a lane holds one channel (u <= 64) and to rounding beyond (tests/test_train_kernels.py asserts the same)."""
    ctx = Ctx(backend, DTYPES[dtype])
    D, R = (l_max + 1) ** 2, 1 if shared else l_max + 1
    # the emulated module took 154 s on six workers with the whole grid: thinned there by u 3, 129 and E 5, 15 -- no dtype, l_max or
    # form; the device runs all of it
    thin = backend == "emu"
    for u in [u for u in WC_U if not (thin and u in WC_U_THIN)]:
        d = wc_data(u, l_max, shared, DTYPES[dtype], max(WC_E))
        log = Log(f"wc_{dtype}_l{l_max}_{'shared' if shared else 'irreps'}_u{u}")
        for E in [E for E in WC_E if not (thin and E in WC_E_THIN)]:
            for wide in (False, True):
                where = f"E{E}_{'wide' if wide else 'dense'}"
                c = WcCase(ctx, d, E, u, l_max, shared, wide)
                got = dict(fwd=c.single(0, where + " fwd").reshape(E, u, D), gw=c.single(1, where + " gw").reshape(E, u * R),
                           gsh=c.single(2, where + " gsh").reshape(E, D), sum=c.both(where + " sum").reshape(E, u, D))
                psh, pw = c.pair(where + " pair")
                got["pair_gsh"], got["pair_gw"] = psh.reshape(E, D), pw.reshape(E, u * R)
                if E == 0:  # AA_OK, nothing written (asserted by `taken`)
                    continue
                for q, v in got.items():
                    check(log, where, q, v, *wc_ref(d, q.replace("pair_", ""), E), 1e-12)
                assert torch.equal(got["pair_gw"], got["gw"]), (log.case, where, "pair out_w against which 1")
                if u <= 64:
                    assert torch.equal(got["pair_gsh"], got["gsh"]), (log.case, where, "pair out_sh against which 2")
                else:
                    close(log, where, "pair out_sh against which 2", got["pair_gsh"], got["gsh"], wc_ref(d, "gsh", E))
                if E == max(WC_E):  # fixed summation orders: the same bits every call
                    again = dict(fwd=c.single(0, where), gw=c.single(1, where), gsh=c.single(2, where), sum=c.both(where))
                    again["pair_gsh"], again["pair_gw"] = c.pair(where)
                    for q, v in again.items():
                        assert torch.equal(v, got[q].reshape(-1)), (log.case, where, q, "not bit-equal across two calls")
        log.flush()


def wc_slots(u, D):
    return (u * D + 255) // 256


def wc_group(u, D, R, esize, terms):
    """Edges per workgroup of the slot forward (`wc_launch_slots`)."""
    per_edge = esize * (u * R + D) * terms
    return max(1, min(K_WC_MAX_GROUP, K_WC_LDS_BYTES // per_edge))


# (l_max, u): every slot count 1..8 of the slot forward and the first row length behind 256 kWcSlots (the general kernel)
WC_SLOT_SHAPES = ([(3, u) for u in (16, 17, 48, 64, 80, 96, 128, 129)] + [(2, u) for u in (28, 29, 57, 86, 114, 143, 171, 227, 228)] +
                  [(1, u) for u in (64, 65, 448, 512, 513)] + [(0, u) for u in (256, 257, 1793, 2048, 2049)])
assert [wc_slots(u, 16) for u in (16, 17, 48, 64, 80, 96, 128, 129)] == [1, 2, 3, 4, 5, 6, 8, 9]
assert [wc_slots(u, 9) for u in (28, 29, 57, 86, 114, 143, 171, 227, 228)] == [1, 2, 3, 4, 5, 6, 7, 8, 9]
assert [wc_slots(u, 4) for u in (64, 65, 448, 512, 513)] == [1, 2, 7, 8, 9] and [wc_slots(u, 1) for u in (256, 257, 1793, 2048, 2049)] == [1, 2, 8, 8, 9]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shared", [0, 1], ids=["per_irrep", "shared"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_weighted_channels_forward_slot_counts(dtype, shared, backend):
    """The slot forward with 1..8 slots per thread, one and two terms, on one edge, 17 and 33 (groups are 16 edges at the most, fewer
    by LDS: 3 in fp64 with two terms at u = 128, l_max = 3); the first row length it does not hold on the general forward."""
    ctx = Ctx(backend, DTYPES[dtype])
    seen = set()
    for l_max, u in WC_SLOT_SHAPES:
        D = (l_max + 1) ** 2
        seen.add(min(wc_slots(u, D), K_WC_SLOTS + 1))
        d = wc_data(u, l_max, shared, DTYPES[dtype], 33)
        log = Log(f"wc_slots_{dtype}_l{l_max}_{'shared' if shared else 'irreps'}_u{u}_ns{wc_slots(u, D)}")
        for E, wide in ((1, False), (17, False), (17, True), (33, False)):
            c = WcCase(ctx, d, E, u, l_max, shared, wide)
            where = f"E{E}_{'wide' if wide else 'dense'}"
            check(log, where, "fwd", c.single(0, where + " fwd").reshape(E, u, D), *wc_ref(d, "fwd", E), 1e-12)
            check(log, where, "sum", c.both(where + " sum").reshape(E, u, D), *wc_ref(d, "sum", E), 1e-12)
        log.flush()
    assert seen == set(range(1, K_WC_SLOTS + 2))


# (l_max, u, shared, terms): fp64 rows whose operands leave room for ONE edge in 32 KB of LDS -- the second one only by the clamp (its
# edge alone asks for 32 784 bytes); and the shape the issue names for it, which takes the general forward (17 slots)
WC_ONE_EDGE_GROUPS = [(1, 512, 0, 2), (0, 2048, 0, 2), (0, 2048, 1, 2), (1, 512, 0, 1)]
assert [wc_group(u, (l + 1) ** 2, 1 if s else l + 1, 8, t) for l, u, s, t in WC_ONE_EDGE_GROUPS] == [1, 1, 1, 3]
assert K_WC_LDS_BYTES // (8 * (2048 + 1) * 2) == 0 and wc_slots(2048, 1) == K_WC_SLOTS and wc_slots(257, 16) > K_WC_SLOTS


@pytest.mark.parametrize("backend", BACKENDS)
def test_weighted_channels_forward_groups_of_one_edge(backend):
    ctx = Ctx(backend, torch.float64)
    for l_max, u, shared, _ in WC_ONE_EDGE_GROUPS[:3] + [(3, 257, 0, 2)]:
        D = (l_max + 1) ** 2
        d = wc_data(u, l_max, shared, torch.float64, 5)
        log = Log(f"wc_one_edge_group_f64_l{l_max}_{'shared' if shared else 'irreps'}_u{u}")
        for E in (1, 5):
            c = WcCase(ctx, d, E, u, l_max, shared, False)
            check(log, f"E{E}", "sum", c.both(f"E{E} sum").reshape(E, u, D), *wc_ref(d, "sum", E), 1e-12)
            check(log, f"E{E}", "fwd", c.single(0, f"E{E} fwd").reshape(E, u, D), *wc_ref(d, "fwd", E), 1e-12)
        log.flush()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_weighted_channels_refusals_write_nothing(dtype, backend):
    ctx = Ctx(backend, DTYPES[dtype])
    u, l_max, E = 6, 2, 5
    d = wc_data(u, l_max, 0, DTYPES[dtype], E)
    for name, change in (("l_max 4", dict(l_max=4)), ("l_max -1", dict(l_max=-1)), ("u 0", dict(u=0)), ("ldw < u R", dict(ldw=u * 3 - 1))):
        c = WcCase(ctx, d, E, u, l_max, 0, False)  # (operands and outputs of the accepted shape behind every refused call)
        for k, v in change.items():
            setattr(c, k, v)
        for which in (0, 1, 2):
            if which == 1 and "ldw" in name:
                continue  # (no weight operand: ldw is ignored)
            c.single(which, f"{name} which {which}", written=False, expect=AA_ERR_INVALID)
        c.both(f"{name} sum", written=False, expect=AA_ERR_INVALID)
        c.pair(f"{name} pair", written=False, expect=AA_ERR_INVALID)
    ok = WcCase(ctx, d, E, u, l_max, 0, False)
    # which = 3 is the two-term form's number inside the library, not a form of aa_weighted_channels
    out, n = ctx.poisoned(E * u * 9)
    for what, which, sh in (("which 3", 3, ok.sh), ("which -1", -1, ok.sh), ("null operand", 0, None)):
        rc = ctx.call(ctx.L.aa_weighted_channels, ctx.code, which, E, u, l_max, 0, ptr(sh), ptr(ok.w), ok.ldw, ptr(out))
        assert rc == AA_ERR_INVALID, what
        ctx.taken(what, out, n, written=False)
    ok.single(0, "accepted")


# =================================================================================================================================
# 2. aa_linear_wgrad
# =================================================================================================================================
def wgrad_rows_per_slab(esize, E, K, N):
    """`wgrad_rows_per_slab` of aa_train.hip: one launch fills the chip once (256 CUs x the workgroups a CU holds by LDS and waves),
    at least 64 rows per slab, at most 4096 slabs, rounded up to 32."""
    kb, nb = (128 if K > 64 else 64), (128 if N > 64 else 64)
    per_slab = ((K + kb - 1) // kb) * ((N + nb - 1) // nb)
    lds = esize * (16 if esize == 8 else 32) * (kb + 4 + nb + 4)
    per_cu = min(8, max(1, (160 * 1024) // lds))
    slabs = max(1, min(4096, 256 * per_cu // per_slab))
    rows = max((E + slabs - 1) // slabs, 64)
    return (rows + 31) // 32 * 32


def wgrad_parts(esize, E, K, N):
    rows = wgrad_rows_per_slab(esize, E, K, N)
    return max(1, (E + rows - 1) // rows)


def wgrad_vec(esize, K, N, ldx, ldg, offx, offg):
    """The condition of the 16-byte staging (offx / offg: elements the base lies behind a 16-byte boundary)."""
    vw = 16 // esize
    return K % vw == 0 and N % vw == 0 and ldx % vw == 0 and ldg % vw == 0 and (offx * esize) % 16 == 0 and (offg * esize) % 16 == 0


def wgrad_call(ctx, E, K, N, x, ldx, g, ldg, nbytes, what, expect=0, short=0, ldx_arg=None):
    """One call on a poisoned workspace of `nbytes` (passed as nbytes - short) and a poisoned output: (workspace payload, out)."""
    assert nbytes % ctx.esize == 0
    ws, nws = ctx.poisoned(nbytes // ctx.esize)
    out, nout = ctx.poisoned(K * N)
    rc = ctx.call(ctx.L.aa_linear_wgrad, ctx.code, E, K, N, ptr(x), ldx if ldx_arg is None else ldx_arg, ptr(g), ldg, ptr(ws), nbytes - short, ptr(out))
    assert rc == expect, (what, rc, ctx.L.aa_last_error())
    written = expect == 0
    return ctx.taken(what + " workspace", ws, nws, written=written and E > 0), ctx.taken(what + " out", out, nout, written=written)


def wgrad_case(ctx, log, E, K, N, ldx, ldg, offx=0, offg=0):
    esize = ctx.esize
    where = f"E{E}_K{K}_N{N}_ldx{ldx}_ldg{ldg}_off{offx}{offg}"
    gen = torch.Generator().manual_seed(4 + E + 1000 * K + N)
    xm = torch.randn(E, ldx, dtype=ctx.dtype, generator=gen)
    gm = torch.randn(E, ldg, dtype=ctx.dtype, generator=gen)
    # the operands end with the last row's K / N elements (rows strided by ldx / ldg)
    x = ctx.inp(xm.reshape(-1)[:max(0, xm.numel() - (ldx - K))], offx * esize)
    g = ctx.inp(gm.reshape(-1)[:max(0, gm.numel() - (ldg - N))], offg * esize)
    nbytes = ctx.L.aa_linear_wgrad_workspace_bytes(ctx.code, E, K, N)
    assert nbytes == wgrad_parts(esize, E, K, N) * K * N * esize, (where, nbytes)
    _, got = wgrad_call(ctx, E, K, N, x, ldx, g, ldg, nbytes, where)
    got = got.reshape(K, N)
    want = xm[:, :K].double().t() @ gm[:, :N].double()
    if E == 0:
        assert bool((got == 0).all()), where
        return
    tol = 2e-6 if esize == 4 else 1e-13
    scale = max(1.0, float(want.abs().max()))
    err_cpu32 = ((xm[:, :K].t() @ gm[:, :N]).double() - want).abs().max().item() if esize == 4 else 0.0
    check_abs(log, where, "wgrad", got, want, tol * scale * max(1, E) ** 0.5, err_cpu32)
    _, again = wgrad_call(ctx, E, K, N, x, ldx, g, ldg, nbytes, where + " again")
    assert torch.equal(again.reshape(K, N), got), (where, "not bit-equal across two calls")


WGRAD_KN = ((64, 64), (65, 64), (64, 65), (128, 129), (1, 1), (128, 192))  # (last: vector staging on 128-wide blocks, a ragged N block)
# exactly two slabs: twice the rows of a slab, as the code computes them
WGRAD_TWO_SLABS = 2 * wgrad_rows_per_slab(4, 128, 64, 64)
WGRAD_E = (0, 1, 31, 32, 33, 63, 64, 65, 129, WGRAD_TWO_SLABS - 1, WGRAD_TWO_SLABS, WGRAD_TWO_SLABS + 1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("KN", WGRAD_KN, ids=[f"K{k}_N{n}" for k, n in WGRAD_KN])
def test_linear_wgrad_rows_at_stage_and_slab_boundaries(KN, dtype, backend):
    ctx = Ctx(backend, DTYPES[dtype])
    K, N = KN
    log = Log(f"wgrad_{dtype}_K{K}_N{N}")
    for es in (4, 8):
        assert wgrad_parts(es, WGRAD_TWO_SLABS, K, N) == 2 and wgrad_parts(es, WGRAD_TWO_SLABS - 1, K, N) == 2 and wgrad_parts(es, WGRAD_TWO_SLABS + 1, K, N) == 3
        assert wgrad_parts(es, 64, K, N) == 1 and wgrad_parts(es, 65, K, N) == 2
    for E in WGRAD_E:
        wgrad_case(ctx, log, E, K, N, K, N)  # dense rows
        wgrad_case(ctx, log, E, K, N, (K + 7) // 4 * 4, (N + 11) // 4 * 4)  # row-strided views (strides that keep 16-byte rows)
    log.flush()


# (name, K, N, ldx, ldg, offx, offg): the 16-byte staging and each of its six conditions broken alone
WGRAD_STAGING = [("vector", 64, 64, 68, 72, 0, 0), ("K", 65, 64, 68, 72, 0, 0), ("N", 64, 65, 68, 72, 0, 0), ("ldx", 64, 64, 69, 72, 0, 0),
                 ("ldg", 64, 64, 68, 73, 0, 0), ("x_base", 64, 64, 68, 72, 1, 0), ("g_base", 64, 64, 68, 72, 0, 1)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_linear_wgrad_vector_staging_and_each_condition_alone(dtype, backend):
    ctx = Ctx(backend, DTYPES[dtype])
    base = WGRAD_STAGING[0][1:]
    assert wgrad_vec(ctx.esize, *base)
    for name, K, N, ldx, ldg, offx, offg in WGRAD_STAGING:
        if name != "vector":  # one value differs from the vector case, and the staging is scalar for it
            assert sum(v != b for v, b in zip((K, N, ldx, ldg, offx, offg), base)) == 1 and not wgrad_vec(ctx.esize, K, N, ldx, ldg, offx, offg), name
        log = Log(f"wgrad_staging_{dtype}_{name}")
        for E in (33, 129):
            wgrad_case(ctx, log, E, K, N, ldx, ldg, offx, offg)
        log.flush()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_linear_wgrad_refusals_write_nothing(dtype, backend):
    ctx = Ctx(backend, DTYPES[dtype])
    E, K, N = 129, 64, 64
    gen = torch.Generator().manual_seed(8)
    x, g = ctx.inp(torch.randn(E, K, dtype=ctx.dtype, generator=gen)), ctx.inp(torch.randn(E, N, dtype=ctx.dtype, generator=gen))
    nbytes = ctx.L.aa_linear_wgrad_workspace_bytes(ctx.code, E, K, N)
    assert nbytes == 3 * K * N * ctx.esize
    wgrad_call(ctx, E, K, N, x, K, g, N, nbytes, "one byte short", expect=AA_ERR_INVALID, short=1)
    assert b"workspace too small" in ctx.L.aa_last_error()
    wgrad_call(ctx, E, K, N, x, K, g, N, nbytes, "ldx < K", expect=AA_ERR_INVALID, ldx_arg=K - 1)
    wgrad_call(ctx, E, K, N, None, K, g, N, nbytes, "null x", expect=AA_ERR_INVALID)
    wgrad_call(ctx, E, K, N, x, K, g, N, nbytes, "accepted")


# =================================================================================================================================
# 3. the activation family
# =================================================================================================================================
ACT_N = (0, 1, 3, 4, 5, 1023, 1024, 1025, 2049)
ACT_FIXED = [0.0] + [s * v for v in (1e-8, 1.0, 20.0, 30.0, 40.0, 90.0, 1e4) for s in (1.0, -1.0)]
# (entry point family, act code | None: the SiLU-only entry points, torch function)
ACT_FAMILIES = {"silu": (None, "silu"), "act_silu": (0, "silu"), "act_mish": (1, "mish"), "act_gelu": (2, "gelu")}


def act_orders(kind, x):
    """The function and its first three derivatives at the fp64 arguments, by autograd through torch's own function."""
    v = x.clone().requires_grad_(True)
    y = getattr(torch.nn.functional, kind)(v)
    outs = [y.detach()]
    for k in range(3):
        (y,) = torch.autograd.grad(y.sum(), v, create_graph=k < 2)
        outs.append(y.detach())
    return outs


def act_call(ctx, act, order, n, x, g, h, what, expect=0, pair=None):
    """`aa_silu_derivative[_pair]` (act None) / `aa_act_derivative[_pair]`: the payloads (out0, out1 | None)."""
    L = ctx.L
    o0, _ = ctx.poisoned(n)
    head = (ctx.code,) if act is None else (ctx.code, act)
    if not (h is not None if pair is None else pair):
        fn = L.aa_silu_derivative if act is None else L.aa_act_derivative
        rc = ctx.call(fn, *head, order, n, ptr(x), ptr(g), ptr(o0))
        assert rc == expect, (what, rc, L.aa_last_error())
        return ctx.taken(what, o0, n, written=expect == 0 and n > 0), None
    o1, _ = ctx.poisoned(n)
    fn = L.aa_silu_derivative_pair if act is None else L.aa_act_derivative_pair
    rc = ctx.call(fn, *head, order, n, ptr(x), ptr(g), ptr(h), ptr(o0), ptr(o1))
    assert rc == expect, (what, rc, L.aa_last_error())
    return ctx.taken(what + " out_x", o0, n, written=expect == 0 and n > 0), ctx.taken(what + " out_g", o1, n, written=expect == 0 and n > 0)


_ACT_FIXED = {}


def act_orders_fixed(kind, x64):
    """`act_orders` at the arguments ACT_FIXED (as the dtype under test holds them).  Autograd through torch's mish returns NaN for the second and third derivative at 1e4 (an inf x 0 in
    its double backward) and nothing else non-finite; so the derivatives of the same three functions are taken here by mpmath's
    numerical differentiation at 120 digits, and torch's autograd has to agree with them wherever it is finite."""
    key = (kind, tuple(x64.tolist()))
    if key not in _ACT_FIXED:
        import mpmath as mp

        fn = {"silu": lambda x: x / (1 + mp.exp(-x)), "mish": lambda x: x * mp.tanh(mp.log(1 + mp.exp(x))),
              "gelu": lambda x: x * (1 + mp.erf(x / mp.sqrt(2))) / 2}[kind]
        with mp.workdps(120):
            outs = [torch.tensor([float(mp.diff(fn, mp.mpf(v), k)) for v in x64.tolist()], dtype=torch.float64) for k in range(4)]
        auto = act_orders(kind, x64)
        for k, (a, o) in enumerate(zip(auto, outs)):
            ok = torch.isfinite(a)
            assert int((~ok).sum()) == (1 if (kind == "mish" and k >= 2) else 0), (kind, k, a)
            assert bool(((a - o).abs()[ok] <= 1e-13 * o.abs().clamp(min=1.0)[ok]).all()), (kind, k, a, o)
        _ACT_FIXED[key] = outs
    return _ACT_FIXED[key]


def act_family_case(ctx, log, act, kind, xh, gh, hh, where, tol, f=None):
    """Every member on one argument vector: orders 0..3 with and without g, the pair form at orders 0..2."""
    n = xh.numel()
    f = f if f is not None else (act_orders(kind, xh.double()) if n else [torch.zeros(0, dtype=torch.float64)] * 4)
    x, g, h = ctx.inp(xh, 0), ctx.inp(gh, 0), ctx.inp(hh, 0)
    fp32 = ctx.dtype == torch.float32

    def verdict(what, got, want):
        # (the fp32 reference is the fp64 result rounded)
        err32 = (want.float().double() - want).abs().max().item() if (fp32 and n) else 0.0
        check_abs(log, where, what, got, want, tol * (max(1.0, float(want.abs().max())) if n else 1.0), err32)

    for order in range(4):
        verdict(f"f{order}", act_call(ctx, act, order, n, x, None, None, f"{where} f{order}")[0], f[order])
        verdict(f"g_f{order}", act_call(ctx, act, order, n, x, g, None, f"{where} g f{order}")[0], gh.double() * f[order])
        if order < 3:
            ox, og = act_call(ctx, act, order, n, x, g, h, f"{where} pair {order}", pair=True)
            verdict(f"pair{order}_x", ox, gh.double() * hh.double() * f[order + 1])
            verdict(f"pair{order}_g", og, hh.double() * f[order])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("family", list(ACT_FAMILIES))
def test_activation_family_sizes(family, dtype, backend):
    """n around the 16-byte vector (4 / 2 elements) and the workgroup (1024 / 512 elements): the vector body, the scalar tail, the last
    thread of a workgroup and the first of the next."""
    ctx = Ctx(backend, DTYPES[dtype])
    act, kind = ACT_FAMILIES[family]
    tol = 2e-5 if dtype == "f32" else (1e-12 if kind == "silu" else 1e-11)
    gen = torch.Generator().manual_seed(11)
    xs, gs, hs = (3.0 * torch.randn(max(ACT_N), dtype=ctx.dtype, generator=gen), torch.randn(max(ACT_N), dtype=ctx.dtype, generator=gen),
                  torch.randn(max(ACT_N), dtype=ctx.dtype, generator=gen))
    log = Log(f"act_{family}_{dtype}")
    for n in ACT_N:
        act_family_case(ctx, log, act, kind, xs[:n].clone(), gs[:n].clone(), hs[:n].clone(), f"n{n}", tol)
    log.flush()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("family", list(ACT_FAMILIES))
def test_activation_family_at_large_and_tiny_arguments(family, dtype, backend):
    """0, +-1e-8, +-1, +-20, +-30, +-40, +-90, +-1e4: exp(|x|) leaves fp32 above 88.7 and fp64 above 709.8, softplus switches form at
    30, the Gaussian of gelu underflows.  Every output finite (asserted by the rule) and within the tolerance of the fp64 reference."""
    ctx = Ctx(backend, DTYPES[dtype])
    act, kind = ACT_FAMILIES[family]
    tol = 2e-5 if dtype == "f32" else (1e-12 if kind == "silu" else 1e-11)
    xh = torch.tensor(ACT_FIXED, dtype=ctx.dtype)
    gen = torch.Generator().manual_seed(12)
    gh, hh = torch.randn(xh.numel(), dtype=ctx.dtype, generator=gen), torch.randn(xh.numel(), dtype=ctx.dtype, generator=gen)
    f = act_orders_fixed(kind, xh.double())
    log = Log(f"act_fixed_{family}_{dtype}")
    act_family_case(ctx, log, act, kind, xh, gh, hh, "fixed", tol, f)
    # one argument at a time: the tolerance scales with the largest expected value of a call, which +-1e4 would set for all of them
    for i, v in enumerate(ACT_FIXED):
        act_family_case(ctx, log, act, kind, xh[i:i + 1].clone(), gh[i:i + 1].clone(), hh[i:i + 1].clone(), f"x{v:g}", tol, [o[i:i + 1] for o in f])
    log.flush()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("family", list(ACT_FAMILIES))
def test_activation_family_refusals_write_nothing(family, dtype, backend):
    ctx = Ctx(backend, DTYPES[dtype])
    act, _ = ACT_FAMILIES[family]
    n = 9
    gen = torch.Generator().manual_seed(13)
    v = [torch.randn(n + 1, dtype=ctx.dtype, generator=gen) for _ in range(3)]
    x, g, h = (ctx.inp(t[:n].clone(), 0) for t in v)
    x1, g1, h1 = (ctx.inp(t[:n].clone(), ctx.esize) for t in v)  # one element behind a 16-byte boundary
    for what, args in (("x", (x1, g, None)), ("g", (x, g1, None)), ("x pair", (x1, g, h)), ("g pair", (x, g1, h)), ("h pair", (x, g, h1))):
        act_call(ctx, act, 0, n, *args, f"misaligned {what}", expect=AA_ERR_INVALID)
        assert b"16-byte aligned" in ctx.L.aa_last_error()
    # a misaligned output
    head = (ctx.code,) if act is None else (ctx.code, act)
    out, _ = ctx.poisoned(n, skip=1)
    rc = ctx.call(ctx.L.aa_silu_derivative if act is None else ctx.L.aa_act_derivative, *head, 0, n, ptr(x), None, ptr(out))
    assert rc == AA_ERR_INVALID
    ctx.taken("misaligned out", out, n, written=False)
    act_call(ctx, act, 3, n, x, g, h, "order 3 pair", expect=AA_ERR_INVALID)
    act_call(ctx, act, 4, n, x, g, None, "order 4", expect=AA_ERR_INVALID)
    act_call(ctx, act, -1, n, x, g, None, "order -1", expect=AA_ERR_INVALID)
    if act is not None:
        act_call(ctx, 3, 0, n, x, g, None, "activation 3", expect=AA_ERR_INVALID)
    act_call(ctx, act, 2, n, x, g, h, "accepted")


# =================================================================================================================================
# 4. aa_scalar_column
# =================================================================================================================================
SC_D = (1, 2, 4, 9, 13, 16, 4096)


def sc_rows(D):
    """1..5 rows (rows D mod 4 takes every value an odd D allows) and the rows on both sides of a workgroup's 1024 elements."""
    around = [1024 // D + k for k in (-1, 0, 1, 2, 3)] if D <= 1024 else []
    return sorted({r for r in [1, 2, 3, 4, 5] + around if r >= 1 and (r * D <= 1100 or D > 1024 and r <= 3)})


assert all({(r * D) % 4 for r in sc_rows(D)} == {0, 1, 2, 3} for D in SC_D if D % 2) and all(any(r * D > 1024 for r in sc_rows(D)) for D in SC_D)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", SC_D)
def test_scalar_column(D, dtype, backend):
    """out = a (NULL: zeros) with s added to component 0 of every row: one addition per element, so equal to torch's bit for bit."""
    ctx = Ctx(backend, DTYPES[dtype])
    gen = torch.Generator().manual_seed(31 + D)
    for rows in [0] + sc_rows(D):
        ah = torch.randn(rows, D, dtype=ctx.dtype, generator=gen)
        sh = torch.randn(rows, dtype=ctx.dtype, generator=gen)
        a, s = ctx.inp(ah, 0), ctx.inp(sh)
        for with_a in (False, True):
            what = f"D{D}_rows{rows}_{'a' if with_a else 'null'}"
            out, n = ctx.poisoned(rows * D)
            rc = ctx.call(ctx.L.aa_scalar_column, ctx.code, rows, D, ptr(a) if with_a else None, ptr(s), ptr(out))
            assert rc == 0, (what, ctx.L.aa_last_error())
            got = ctx.taken(what, out, n, written=rows > 0).reshape(rows, D)
            want = ah.clone() if with_a else torch.zeros_like(ah)
            want[:, 0] += sh
            assert torch.equal(got, want), (what, float((got - want).abs().max()) if rows else 0.0)
    print(f"scalar_column_{dtype}_D{D} out err_hip 0 err_cpu32 0 scale 1 (bit-equal, rows {sc_rows(D)})")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_scalar_column_refusals_write_nothing(dtype, backend):
    ctx = Ctx(backend, DTYPES[dtype])
    gen = torch.Generator().manual_seed(32)
    rows = 3
    a, s = ctx.inp(torch.randn(rows * 4097, dtype=ctx.dtype, generator=gen), 0), ctx.inp(torch.randn(rows, dtype=ctx.dtype, generator=gen))
    a1 = ctx.inp(torch.randn(rows * 9, dtype=ctx.dtype, generator=gen), ctx.esize)
    for what, D, ap, skip in (("D 4097", 4097, a, 0), ("D 0", 0, a, 0), ("misaligned a", 9, a1, 0), ("misaligned out", 9, a, 1), ("null s", 9, a, 0)):
        out, n = ctx.poisoned(rows * max(D, 1), skip=skip)
        rc = ctx.call(ctx.L.aa_scalar_column, ctx.code, rows, D, ptr(ap), None if what == "null s" else ptr(s), ptr(out))
        assert rc == AA_ERR_INVALID, what
        ctx.taken(what, out, n, written=False)


# =================================================================================================================================
# 5. aa_concat_columns
# =================================================================================================================================
def concat_vec(esize, widths, lds, offs, ldo, out_off):
    vec = 16 // esize
    return (ldo % vec == 0 and (out_off * esize) % 16 == 0 and
            all(w % vec == 0 and ld % vec == 0 and (o * esize) % 16 == 0 for w, ld, o in zip(widths, lds, offs)))


def concat_case(ctx, E, widths, lds, offs, ldo, out_off, what, expect=0):
    """Inputs j of widths[j] columns, row stride lds[j], offs[j] elements behind a 16-byte boundary; out with row stride ldo."""
    n, total = len(widths), sum(widths)
    gen = torch.Generator().manual_seed(41 + E + total)
    hosts = [torch.randn(E, ld, dtype=ctx.dtype, generator=gen) for ld in lds]
    ins = [ctx.inp(h.reshape(-1)[:max(0, h.numel() - (ld - w))], o * ctx.esize) for h, ld, w, o in zip(hosts, lds, widths, offs)]
    xs = (ctypes.c_void_p * n)(*[ptr(t) for t in ins])
    ld_arr, w_arr = (ctypes.c_int64 * n)(*lds), (ctypes.c_int * n)(*widths)
    extent = (E - 1) * ldo + total if E > 0 else 0  # (the output ends with the last row's columns)
    out, _ = ctx.poisoned(extent, skip=out_off)
    rc = ctx.call(ctx.L.aa_concat_columns, ctx.code, E, n, xs, ld_arr, w_arr, ptr(out), ldo)
    assert rc == expect, (what, rc, ctx.L.aa_last_error())
    host = out.cpu()
    assert torch.isnan(host[extent:]).all(), f"{what}: wrote behind its {extent} elements"
    if expect != 0 or E == 0:
        assert torch.isnan(host).all(), f"{what}: written"
        return
    rows = torch.full((E * ldo,), NAN, dtype=ctx.dtype)
    rows[:extent] = host[:extent]
    rows = rows.reshape(E, ldo)
    assert torch.isnan(rows[:, total:]).all(), f"{what}: wrote into the padding columns"
    assert torch.equal(rows[:, :total], torch.cat([h[:, :w] for h, w in zip(hosts, widths)], dim=1)), what


# (name, widths, lds, offs, ldo - total, out_off): all conditions of the 16-byte path met, then each broken alone
CONCAT_BASE = ((4, 8), (8, 12), (0, 0), 0, 0)
CONCAT_TOGGLES = [("vector", *CONCAT_BASE), ("vector_padded", (4, 8), (8, 12), (0, 0), 4, 0), ("width", (5, 8), (8, 12), (0, 0), 3, 0),
                  ("ldx", (4, 8), (9, 12), (0, 0), 0, 0), ("x_base", (4, 8), (8, 12), (0, 1), 0, 0), ("ldo", (4, 8), (8, 12), (0, 0), 5, 0),
                  ("out_base", (4, 8), (8, 12), (0, 0), 0, 1), ("scalar_padded", (5, 6, 1), (7, 6, 3), (0, 1, 0), 5, 1)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_concat_columns_each_vector_condition_alone(dtype, backend):
    ctx = Ctx(backend, DTYPES[dtype])
    for name, widths, lds, offs, pad, out_off in CONCAT_TOGGLES:
        ldo = sum(widths) + pad
        vec = concat_vec(ctx.esize, widths, lds, offs, ldo, out_off)
        assert vec == name.startswith("vector"), name
        for E in (0, 1, 257):
            concat_case(ctx, E, widths, lds, offs, ldo, out_off, f"{name}_E{E}")
    print(f"concat_columns_{dtype} out err_hip 0 err_cpu32 0 scale 1 (bit-equal, {len(CONCAT_TOGGLES)} layouts)")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_concat_columns_input_counts(dtype, backend):
    """1, 2 and 8 inputs on both paths, `ldo` = total and total + 5; 9 inputs, no inputs and a row stride below the row are refused."""
    ctx = Ctx(backend, DTYPES[dtype])
    eight_v, eight_s = (4, 8, 4, 12, 4, 4, 8, 4), (1, 2, 3, 1, 5, 1, 1, 2)
    for widths in ((8,), (3,), (4, 8), (5, 6), eight_v, eight_s):
        lds = tuple(w + 4 for w in widths)
        for pad in (0, 5, 8):
            for E in (0, 1, 257):
                concat_case(ctx, E, widths, lds, (0,) * len(widths), sum(widths) + pad, 0, f"w{widths}_pad{pad}_E{E}")
    nine = eight_v + (4,)
    concat_case(ctx, 5, nine, nine, (0,) * 9, sum(nine), 0, "nine inputs", expect=AA_ERR_INVALID)
    concat_case(ctx, 5, (4, 8), (8, 12), (0, 0), 11, 0, "ldo < total", expect=AA_ERR_INVALID)
    concat_case(ctx, 5, (4, 8), (3, 12), (0, 0), 12, 0, "ldx < width", expect=AA_ERR_INVALID)
    out, n = ctx.poisoned(12)
    assert ctx.call(ctx.L.aa_concat_columns, ctx.code, 1, 0, None, None, None, ptr(out), 12) == AA_ERR_INVALID
    ctx.taken("no inputs", out, n, written=False)


# =================================================================================================================================
# 6. aa_linear_forward
# =================================================================================================================================
# `aa_linear_forward` takes fp32 only, K and N multiples of 32 (>= 32), row strides multiples of 4, 16-byte-aligned x / out / workspace;
# it packs W on the device and runs the split-bf16 kernel: 128-row tiles, the operand fragments held for K <= 64 and K <= 128 and
# streamed beyond.  `ops.linear` keeps the library GEMM for everything else (`ops._linear_forward_ok`).
LF_E = (1, 127, 128, 129, 257)
LF_KN = ((32, 32), (64, 64), (96, 32), (128, 64), (160, 96), (64, 192))


def lf_call(ctx, E, K, N, x, ldx, W, ldk, ldn, ldo, what, expect=0, short=0, out_skip=0):
    nbytes = ctx.L.aa_linear_forward_workspace_bytes(K, N)
    assert nbytes % 4 == 0 and nbytes > 0
    ws, nws = ctx.poisoned(nbytes // 4)
    extent = (E - 1) * ldo + N if E > 0 else 0
    out, _ = ctx.poisoned(extent, skip=out_skip)
    rc = ctx.call(ctx.L.aa_linear_forward, E, K, N, ptr(x), ldx, ptr(W), ldk, ldn, ptr(ws), nbytes - short, ptr(out), ldo)
    assert rc == expect, (what, rc, ctx.L.aa_last_error())
    host = out.cpu()
    assert torch.isnan(host[extent:]).all(), f"{what}: wrote behind its {extent} elements"
    if expect != 0 or E == 0:
        assert torch.isnan(host).all() and torch.isnan(ws.cpu()).all(), f"{what}: written"
        return None
    # the packed weights are bit patterns (three bf16 levels in a word), not floats: the guard behind them is what is checked
    assert torch.isnan(ws.cpu()[nws:]).all(), f"{what}: wrote behind the workspace"
    rows = torch.full((E * ldo,), NAN, dtype=ctx.dtype)
    rows[:extent] = host[:extent]
    rows = rows.reshape(E, ldo)
    assert torch.isnan(rows[:, N:]).all(), f"{what}: wrote into the padding columns"
    assert not torch.isnan(rows[:, :N]).any(), f"{what}: elements never written"
    return rows[:, :N]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("KN", LF_KN, ids=[f"K{k}_N{n}" for k, n in LF_KN])
def test_linear_forward_rows_around_the_tile(KN, backend):
    ctx = Ctx(backend, torch.float32)
    K, N = KN
    gen = torch.Generator().manual_seed(5 + K + N)
    log = Log(f"linear_forward_f32_K{K}_N{N}")
    for E in LF_E:
        for transposed, xpad, opad in ((False, 0, 0), (True, 64, 4), (False, 4, 8)):
            where = f"E{E}_{'Wt' if transposed else 'W'}_ldx{K + xpad}_ldo{N + opad}"
            xm = torch.randn(E, K + xpad, generator=gen)
            Wm = torch.randn(K, N, generator=gen)
            x = ctx.inp(xm.reshape(-1)[:xm.numel() - xpad], 0)
            W = ctx.inp(Wm.t().contiguous() if transposed else Wm)
            got = lf_call(ctx, E, K, N, x, K + xpad, W, 1 if transposed else N, K if transposed else 1, N + opad, where)
            want = xm[:, :K].double() @ Wm.double()
            err32 = ((xm[:, :K] @ Wm).double() - want).abs().max().item()
            check_abs(log, where, "out", got, want, 3e-6 * K ** 0.5 * float(want.abs().max()), err32)
    log.flush()


@pytest.mark.parametrize("backend", BACKENDS)
def test_linear_forward_refusals_and_the_library_gemm_of_ops_linear(backend):
    """One shape on the other side of every rule: refused by the entry point with nothing written, kept on the library GEMM by
    `ops.linear` (and equal to it there); the accepted neighbour of each through the op."""
    from allegro_amd import ops

    ctx = Ctx(backend, torch.float32)
    lid = ops.register_library(ctx.lib) if backend == "emu" else 0
    gen = torch.Generator().manual_seed(6)
    E = 5
    xm, Wm = torch.randn(E, 200, generator=gen), torch.randn(200, 200, generator=gen)
    x, W, x1 = ctx.inp(xm, 0), ctx.inp(Wm), ctx.inp(xm, 4)
    for what, K, N, kw in (("K 48", 48, 32, {}), ("N 48", 32, 48, {}), ("K 16", 16, 32, {}), ("N 16", 32, 16, {}), ("ldx % 4", 32, 32, dict(ldx=34)),
                           ("ldx < K", 64, 32, dict(ldx=32)), ("ldo < N", 32, 64, dict(ldo=32)), ("ldo % 4", 32, 32, dict(ldo=34)),
                           ("x base", 32, 32, dict(x=x1)), ("out base", 32, 32, dict(out_skip=1)), ("workspace short", 32, 32, dict(short=1)),
                           ("null W", 32, 32, dict(W=None))):
        lf_call(ctx, E, K, N, kw.get("x", x), kw.get("ldx", 200), kw.get("W", W), 200, 1, kw.get("ldo", max(N, 32)), what, expect=AA_ERR_INVALID,
                short=kw.get("short", 0), out_skip=kw.get("out_skip", 0))
    lf_call(ctx, 0, 32, 32, None, 32, W, 200, 1, 32, "no rows")
    assert lf_call(ctx, E, 32, 32, x, 200, W, 200, 1, 32, "accepted") is not None
    # the op side of the same rules
    xd, Wd = xm.to(ctx.dev), Wm.to(ctx.dev)
    log = Log("linear_forward_ops_f32")
    for K, N, hand in ((32, 32, True), (48, 32, False), (32, 48, False), (16, 32, False), (32, 16, False), (64, 96, True)):
        a, b = xd[:, :K], Wd[:K, :N]
        assert ops._linear_forward_ok(a, b) == hand, (K, N)
        got = ops._matmul(a, b, lid)
        want = xm[:, :K].double() @ Wm[:K, :N].double()
        if not hand:
            assert torch.equal(got, a @ b), (K, N)
        check_abs(log, f"K{K}_N{N}", "out", got.cpu(), want, 3e-6 * K ** 0.5 * float(want.abs().max()), ((xm[:, :K] @ Wm[:K, :N]).double() - want).abs().max().item())
    assert not ops._linear_forward_ok(xd[:0, :32], Wd[:32, :32]) and not ops._linear_forward_ok(xd[:, :32].double(), Wd[:32, :32].double())
    log.flush()
