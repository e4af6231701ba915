"""The operator seam by value at the shapes where its kernels change behaviour.

`aa_tp_forward`, `aa_tp_backward` (with either output NULL), `aa_tp_backward_weights` and `aa_tp_segment_sum` are what
`HipContracter` and the whole training path (allegro_amd/ops.py) call.  The older seam modules run them at N <= 11 atoms with
`randint` scatter indices; this module calls the library directly, with caller-owned buffers, on

* deterministic segment layouts (LAYOUTS): one edge, one long segment, empty segments in every position, no edges at all, no atoms,
  more than 64 path-weight slabs (both column-sum launches), more atoms than slabs on the general (1024) and -- on the device --
  on the dense (8192) path-weight kernels; every layout sorted (`eids` NULL) and with a seeded permutation of the same edges;
* channel counts 1, 3, 96, 256, 300 (and 320 for the path-weight gradient) on the table-driven kernels of aa_tp.hip -- below a
  wave, between two waves, one edge per chunk of 256, an edge's channels straddling chunks, a ragged last 128-channel pass -- and
  64 / 128 / 256 on the specialised kernels of aa_tp_dense.hip, each of those plans a second time on the general kernels.

Every output (`out`, `x2s`, `gx1`, `gx2`, `gw`, the path-weight workspace) is NaN before the call and has a guard of 64 NaN elements
behind it: afterwards the payload holds no NaN and the guard is untouched, so a row a kernel never writes and a store past the end
are both seen.  The workspace is `aa_tp_weights_workspace_bytes` exactly.

Reference: `oracle.restatement.contracter_forward` in float64 on the CPU on the plan's own `w3j` and weights, gradients from autograd
through it, `x2s` from a plain `index_add_`.  fp64 results within 1e-10 x max(1, max |expected|) (tests/test_dense_contracter.py);
fp32 results by `tests.fastpath_utils.assert_vs_oracle64` against the same function evaluated a second time in float32 (not further
from the fp64 reference than twice the fp32 CPU evaluation, + 1e-5 of the scale: the long segments sum 70 to 300 terms).  What the
header promises as deterministic (`aa_tp_segment_sum`, `aa_tp_backward_weights`, the dense forward and backward) is bit-equal across
two identical calls and between the sorted and the permuted run; the general backward sums `gx2` with LDS atomics and is compared
to rounding.

`-s` prints `case quantity err_hip err_cpu32 scale`; DESIGN.md section 5 quotes the worst ratios."""
import pytest
import torch

from allegro_amd import _lib, o3
from allegro_amd.nn import HipContracter, allegro_layer_irreps
from tests.fastpath_utils import oracle64_errors

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
DTYPES = {"f64": torch.float64, "f32": torch.float32}
GUARD = 64
SF = 0.37
NAN = float("nan")

LAYOUTS = {
    "one": [1],                                   # smallest launch
    "long": [70],                                 # 18 chunks of 256 at u = 64, ragged last; one dense wave slot beside 3 invalid ones
    "holes": [0, 0, 5, 0, 1, 33, 0, 2, 0],        # leading, trailing, consecutive empty segments; N % 4 = 1
    "no_edges": [0, 0, 0],                        # E = 0 with N > 0
    "nothing": [],                                # N = 0
    "many": [i % 3 + 1 for i in range(70)],       # > 64 wgrad slabs: both column-sum launches, ragged last chunk
    "blocks": [i % 2 + 1 for i in range(1030)],   # general wgrad above 1024 atoms: two atoms per block, trailing blocks own none
    "slots": [0 if i % 7 == 0 else 1 for i in range(8200)],  # dense wgrad above 8192 slots (device only)
}
assert sum(LAYOUTS["holes"]) == 41 and len(LAYOUTS["many"]) > 64 and len(LAYOUTS["blocks"]) > 1024 and len(LAYOUTS["slots"]) > 8192

# the golden non-standard signature (tests/golden: the reference's kernel test), and a small one for the many-atom layouts
GOLDEN = ("2o + 1e + 0e", "0e + 0o + 1e + 1o", "1o + 2e")
SMALL = ("0e + 1o", "0e + 1o", "0e + 1o")


def _backend(name):
    if name == "emu":
        from tests.hip_utils import emu_lib

        return emu_lib(), torch.device("cpu")
    assert torch.cuda.is_available()
    return _lib.load(), torch.device("cuda:0")


# ---- plans -----------------------------------------------------------------------------------------------------------------
_CONTRACTERS = {}


def contracter(backend, irreps, mul, coupling, dtype):
    """A `HipContracter` of the signature (built as the module builds it: w3j, descriptor, weights) bound to the backend's library."""
    key = (backend, irreps, mul, coupling, dtype)
    if key not in _CONTRACTERS:
        lib, dev = _backend(backend)
        prev = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            torch.manual_seed(5)
            c = HipContracter(*irreps, mul=mul, path_channel_coupling=coupling, scatter_factor=SF)
        finally:
            torch.set_default_dtype(prev)
        c = c.to(dev)
        c._bind_library(lib)
        assert c.num_paths > 1
        _CONTRACTERS[key] = c
    return _CONTRACTERS[key]


def standard_layer(l_max, L, layer):
    irreps = allegro_layer_irreps(l_max, True, L)
    return (str(irreps[layer]), str(o3.Irreps.spherical_harmonics(l_max, p=-1)), str(irreps[layer + 1]))


# ---- inputs and the reference, once per (signature, layout, dtype) ------------------------------------------------------------
_DATA = {}


def case_data(c, irreps, coupling, layout, dtype):
    """Inputs in CSR (sorted) order on the host and the reference: {quantity: (fp32 reference | None, fp64 reference)}."""
    key = (irreps, c.mul, coupling, layout, dtype)
    if key in _DATA:
        return _DATA[key]
    from oracle import restatement as R

    deg = LAYOUTS[layout]
    N, E = len(deg), sum(deg)
    u, d1, d2, dout = c.mul, c.base_dim1, c.base_dim2, c.base_dim_out
    g = torch.Generator().manual_seed(1000 + 7 * N + E)
    x1 = torch.randn(E, u, d1, dtype=dtype, generator=g)
    x2 = torch.randn(E, u, d2, dtype=dtype, generator=g)
    go = torch.randn(E, u, dout, dtype=dtype, generator=g)
    idxs = torch.repeat_interleave(torch.arange(N), torch.tensor(deg, dtype=torch.int64))
    rowptr = torch.zeros(N + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(torch.tensor(deg, dtype=torch.int64), 0).to(torch.int32)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(11 + E))  # sorted position -> edge id of the permuted run

    def evaluate(dt):
        a, b = x1.to(dt).requires_grad_(True), x2.to(dt).requires_grad_(True)
        w = c.weights.detach().cpu().to(dt).requires_grad_(True)
        y = R.contracter_forward(a, b, idxs, N, w, c.w3j.detach().cpu().to(dt), coupling, SF)
        g1, g2, gw = torch.autograd.grad(y, [a, b, w], go.to(dt))
        x2s = torch.zeros(N, u, d2, dtype=dt).index_add_(0, idxs, b.detach()) * SF
        return dict(out=y.detach(), x2s=x2s, gx1=g1, gx2=g2, gw=gw)

    ref = None
    if E:
        r64 = evaluate(torch.float64)
        r32 = evaluate(torch.float32) if dtype == torch.float32 else {k: None for k in r64}
        ref = {k: (r32[k], r64[k]) for k in r64}
    _DATA[key] = dict(N=N, E=E, deg=torch.tensor(deg, dtype=torch.int64), x1=x1, x2=x2, go=go, rowptr=rowptr, perm=perm, ref=ref)
    return _DATA[key]


# ---- one pass over the seam with caller-owned, poisoned, guarded buffers ---------------------------------------------------------
class Seam:
    def __init__(self, backend, c, dtype):
        self.lib, self.dev = _backend(backend)
        self.c, self.dtype = c, dtype
        self.plan = c._plan(dtype, self.dev)
        self.code = _lib.AA_F32 if dtype == torch.float32 else _lib.AA_F64
        self.elem = 4 if dtype == torch.float32 else 8
        self.w = c.weights.detach().contiguous()
        self.gpu = self.dev.type == "cuda"
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream if self.gpu else None

    def use_general(self, on):
        self.lib.check(self.lib.lib.aa_tp_plan_use_general_kernels(self.plan, int(on)), "aa_tp_plan_use_general_kernels")
        return self.lib.lib.aa_tp_plan_is_specialised(self.plan)

    def poisoned(self, *shape):
        """(buffer of numel + GUARD NaNs, numel)"""
        n = 1
        for s in shape:
            n *= s
        return torch.full((n + GUARD,), NAN, dtype=self.dtype, device=self.dev), n

    def call(self, fn, *args):
        if self.gpu:
            with torch.cuda.device(self.dev):
                rc = fn(*args, self.stream)
                torch.cuda.synchronize(self.dev)
        else:
            rc = fn(*args, None)
        return rc

    def taken(self, what, buf, n, shape, must_be_written=True):
        """The payload of a buffer behind a call, on the host: no NaN in it, the guard untouched."""
        host = buf.cpu()
        assert torch.isnan(host[n:]).all(), f"{what}: wrote behind its {n} elements"
        if must_be_written:
            assert not torch.isnan(host[:n]).any(), f"{what}: {int(torch.isnan(host[:n]).sum())} of {n} elements never written"
        return host[:n].reshape(shape)

    def workspace_bytes(self, N):
        return self.lib.lib.aa_tp_weights_workspace_bytes(self.plan, N)

    def backward_weights(self, what, d, dev_in, x2s, eids, nbytes=None):
        """(return code, gw | None): `aa_tp_backward_weights` on a workspace of `nbytes` (default: what the plan asks for) exactly."""
        N, E = d["N"], d["E"]
        nbytes = self.workspace_bytes(N) if nbytes is None else nbytes
        assert nbytes % self.elem == 0
        ws, nws = self.poisoned(nbytes // self.elem)
        gw, ngw = self.poisoned(self.w.numel())
        p = lambda t: t.data_ptr() if E else None  # noqa: E731  (edge tensors without rows: NULL)
        rc = self.call(self.lib.lib.aa_tp_backward_weights, self.plan, E, N, p(dev_in["x1"]), x2s.data_ptr() if E else None, dev_in["rowptr"].data_ptr(),
                       eids, p(dev_in["go"]), ws.data_ptr(), nbytes, gw.data_ptr())
        self.taken(f"{what} workspace", ws, nws, (-1,), must_be_written=False)
        if rc != 0:
            assert torch.isnan(gw.cpu()).all() and torch.isnan(ws.cpu()).all(), f"{what}: a refused call wrote"
            return rc, None
        return rc, self.taken(f"{what} gw", gw, ngw, tuple(self.w.shape))

    def run(self, what, d, permuted, only_gw=False):
        """Every call of the seam once; results on the host with the rows of the edge tensors in CSR order."""
        lib, dev = self.lib, self.dev
        N, E = d["N"], d["E"]
        u, d1, d2, dout = self.c.mul, self.c.base_dim1, self.c.base_dim2, self.c.base_dim_out
        perm = d["perm"]

        def carried(t):  # the same per-edge data at the permuted rows
            if not permuted:
                return t.to(dev)
            moved = torch.empty_like(t)
            moved[perm] = t
            return moved.to(dev)

        back = (lambda t: t[perm]) if permuted else (lambda t: t)
        dev_in = dict(x1=carried(d["x1"]), x2=carried(d["x2"]), go=carried(d["go"]), rowptr=d["rowptr"].to(dev))
        eids_t = perm.to(torch.int32).to(dev) if permuted else None
        eids = eids_t.data_ptr() if (permuted and E) else None
        p = lambda t: t.data_ptr() if E else None  # noqa: E731
        x1, x2, go, rowptr, w = p(dev_in["x1"]), p(dev_in["x2"]), p(dev_in["go"]), dev_in["rowptr"].data_ptr(), self.w.data_ptr()
        res = {}

        seg, nseg = self.poisoned(N, u, d2)
        lib.check(self.call(lib.lib.aa_tp_segment_sum, self.code, E, N, u * d2, x2, rowptr, eids, SF, seg.data_ptr()), f"{what} aa_tp_segment_sum")
        res["seg"] = self.taken(f"{what} segment_sum", seg, nseg, (N, u, d2))
        x2s = seg
        if not only_gw:
            x2s, nx2s = self.poisoned(N, u, d2)
            out, nout = self.poisoned(E, u, dout)
            lib.check(self.call(lib.lib.aa_tp_forward, self.plan, E, N, x1, x2, w, rowptr, eids, SF, x2s.data_ptr(), out.data_ptr()), f"{what} aa_tp_forward")
            res["x2s"] = self.taken(f"{what} x2s", x2s, nx2s, (N, u, d2))
            res["out"] = back(self.taken(f"{what} out", out, nout, (E, u, dout)))
            for name, want1, want2 in (("", True, True), ("_only", True, False), ("_only", False, True)):
                gx1, n1 = self.poisoned(E, u, d1)
                gx2, n2 = self.poisoned(E, u, d2)
                # (a gradient not asked for: its output and the operand only it reads are NULL)
                lib.check(self.call(lib.lib.aa_tp_backward, self.plan, E, N, x1 if want2 else None, x2s.data_ptr() if want1 else None, w, rowptr, eids, SF,
                                    go, gx1.data_ptr() if want1 else None, gx2.data_ptr() if want2 else None), f"{what} aa_tp_backward{name}")
                g1 = self.taken(f"{what} gx1{name}", gx1, n1, (E, u, d1), must_be_written=want1)
                g2 = self.taken(f"{what} gx2{name}", gx2, n2, (E, u, d2), must_be_written=want2)
                assert (want1 or torch.isnan(g1).all()) and (want2 or torch.isnan(g2).all()), f"{what}: a gradient not asked for was written"
                if want1:
                    res["gx1" + name] = back(g1)
                if want2:
                    res["gx2" + name] = back(g2)
        rc, gw = self.backward_weights(what, d, dev_in, x2s, eids)
        lib.check(rc, f"{what} aa_tp_backward_weights")
        res["gw"] = gw
        return res


# ---- the two rules ---------------------------------------------------------------------------------------------------------
WORST = {}


def check(case, what, got, w32, w64):
    assert got.shape == w64.shape and torch.isfinite(got).all(), (case, what)
    if w32 is None:
        scale = max(1.0, float(w64.abs().max()))
        err = (got - w64).abs().max().item()
        print(f"{case} {what} f64 err_hip {err:.3e} err_cpu32 0 scale {scale:.3e} rel {err / scale:.3e}")
        assert err <= 1e-10 * scale, (case, what, err, scale)
        return
    err_hip, err_cpu32, scale = oracle64_errors(got, w32, w64)
    print(f"{case} {what} f32 err_hip {err_hip:.3e} err_cpu32 {err_cpu32:.3e} scale {scale:.3e} of_bound {err_hip / (2.0 * err_cpu32 + 1e-5 * scale):.3f}")
    assert err_hip <= 2.0 * err_cpu32 + 1e-5 * scale, (case, what, err_hip, err_cpu32, scale)


def same(case, what, a, b, bitwise, ref):
    """Two runs of the same case: bit-equal where the header promises a fixed summation order, to rounding otherwise (fp64: the
    tolerance of `check`; fp32: the bound of `check`, both runs being within it of the same reference)."""
    if bitwise:
        assert torch.equal(a, b), (case, what, "not bit-equal", float((a - b).abs().max()) if a.numel() else 0.0)
        return
    w32, w64 = ref
    scale = max(1.0, float(w64.abs().max()))
    bound = 1e-10 * scale if w32 is None else 2.0 * (w32.double() - w64).abs().max().item() + 1e-5 * scale
    err = float((a - b).abs().max())
    assert err <= bound, (case, what, err, bound)


QUANTITIES = ("out", "x2s", "gx1", "gx2", "gx1_only", "gx2_only", "gw")


def seam_case(backend, c, irreps, coupling, dtype, layout, general, case, only_gw=False, expect_specialised=None, runs=("sorted", "again", "permuted")):
    """One plan on one layout: sorted, sorted again, permuted.  Returns the results of the first run."""
    d = case_data(c, irreps, coupling, layout, dtype)
    seam = Seam(backend, c, dtype)
    dense = bool(seam.use_general(general))
    if expect_specialised is not None:
        assert dense == expect_specialised, (case, "aa_tp_plan_is_specialised", dense)
    N, E, ref = d["N"], d["E"], d["ref"]
    res = {r: seam.run(f"{case} {r}", d, permuted=(r == "permuted"), only_gw=only_gw) for r in runs}
    first = res[runs[0]]
    u, d2 = c.mul, c.base_dim2
    for r, got in res.items():
        name = f"{case} {r}"
        assert got["seg"].shape == (N, u, d2) and got["gw"].shape == c.weights.shape
        # atoms without edges: exact zeros, not merely small
        assert bool((got["seg"][d["deg"] == 0] == 0).all()), (name, "segment_sum rows of empty segments")
        if not only_gw:
            assert bool((got["x2s"][d["deg"] == 0] == 0).all()), (name, "x2s rows of empty segments")
            if dense:
                assert torch.equal(got["seg"], got["x2s"]), (name, "aa_tp_segment_sum and the x2s of aa_tp_forward sum in CSR order")
        if E == 0:  # nothing to contract: x2s and gw exactly zero, edge tensors without rows
            assert bool((got["seg"] == 0).all()) and bool((got["gw"] == 0).all()), name
            assert only_gw or (bool((got["x2s"] == 0).all()) and all(got[q].shape[0] == 0 for q in ("out", "gx1", "gx2", "gx1_only", "gx2_only"))), name
            continue
        if r == "again":
            continue
        check(name, "seg", got["seg"], *ref["x2s"])
        for q in QUANTITIES:
            if q in got:
                check(name, q, got[q], *ref[q.replace("_only", "")])
    if E:
        for r in runs[1:]:
            for q, t in res[r].items():
                bitwise = q in ("seg", "gw") or dense
                same(f"{case} {r} vs {runs[0]}", q, t, first[q], bitwise, ref[{"seg": "x2s"}.get(q, q.replace("_only", ""))])
    return first


# ---- general kernels -------------------------------------------------------------------------------------------------------
GENERAL_LAYOUTS = ("one", "long", "holes", "no_edges", "nothing")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("coupling", [True, False], ids=["coupled", "uncoupled"])
@pytest.mark.parametrize("mul", [1, 3, 96, 256, 300])
def test_general_kernels_on_the_golden_signature(mul, coupling, dtype, backend):
    c = contracter(backend, GOLDEN, mul, coupling, DTYPES[dtype])
    assert (c.base_dim1, c.base_dim2, c.base_dim_out) == (9, 8, 8)
    for layout in GENERAL_LAYOUTS:
        seam_case(backend, c, GOLDEN, coupling, DTYPES[dtype], layout, False, f"golden_u{mul}_{'c' if coupling else 'p'}_{dtype}_{layout}",
                  expect_specialised=False)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("coupling", [True, False], ids=["coupled", "uncoupled"])
def test_general_path_weight_gradient_with_a_ragged_last_channel_pass(coupling, dtype, backend):
    """u = 320 = 128 + 128 + 64: three passes of `tp_layer_wgrad_kernel`, the last one with half of its lanes beyond the channels."""
    c = contracter(backend, GOLDEN, 320, coupling, DTYPES[dtype])
    seam_case(backend, c, GOLDEN, coupling, DTYPES[dtype], "holes", False, f"golden_u320_{'c' if coupling else 'p'}_{dtype}_holes", only_gw=True,
              expect_specialised=False)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("coupling", [True, False], ids=["coupled", "uncoupled"])
@pytest.mark.parametrize("layout", ["many", "blocks"])
def test_general_kernels_on_many_atoms(layout, coupling, dtype, backend):
    """More than 64 slabs (both launches of the column sum) and more than 1024 atoms (several atoms per workgroup of the path-weight
    kernel, trailing workgroups without an atom)."""
    c = contracter(backend, SMALL, 2, coupling, DTYPES[dtype])
    seam_case(backend, c, SMALL, coupling, DTYPES[dtype], layout, False, f"small_u2_{'c' if coupling else 'p'}_{dtype}_{layout}", expect_specialised=False)


# ---- dense kernels ---------------------------------------------------------------------------------------------------------
# (l_max, L, layer, mul, coupling); (2, 2, 1, *) is the last layer of a two-layer stack: its output keeps the scalars only
DENSE = [(1, 2, 0, 64, True), (2, 2, 0, 64, True), (2, 2, 1, 128, False), (2, 3, 1, 256, True), (3, 2, 0, 64, False), (2, 2, 1, 64, True)]
DENSE_LAYOUTS = ("one", "long", "holes", "no_edges", "many")
DENSE_CASES = [(s, dt) for s in DENSE for dt in ("f32", "f64")]


def _dense_name(sig, dtype):
    return "l{}_L{}_layer{}_u{}_{}_{}".format(*sig[:4], "c" if sig[4] else "p", dtype)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("sig,dtype", DENSE_CASES, ids=[_dense_name(s, dt) for s, dt in DENSE_CASES])
def test_dense_kernels_on_standard_layers(sig, dtype, backend):
    """The specialised kernels on every layout, and the same plan switched to the general kernels (also 64 / 128 / 256 channels there).
    fp64 at l_max 3 has no specialised kernels: the plan says so and runs the general ones."""
    l_max, L, layer, mul, coupling = sig
    irreps = standard_layer(l_max, L, layer)
    c = contracter(backend, irreps, mul, coupling, DTYPES[dtype])
    if layer == L - 1:
        assert c.base_dim_out == 1
    specialised = not (dtype == "f64" and l_max >= 3)
    for layout in DENSE_LAYOUTS:
        name = f"{_dense_name(sig, dtype)}_{layout}"
        a = seam_case(backend, c, irreps, coupling, DTYPES[dtype], layout, False, name, expect_specialised=specialised)
        if specialised:
            b = seam_case(backend, c, irreps, coupling, DTYPES[dtype], layout, True, name + "_general", expect_specialised=False, runs=("sorted", "permuted"))
            assert a.keys() == b.keys()
    Seam(backend, c, DTYPES[dtype]).use_general(False)


@pytest.mark.gpu
def test_dense_path_weight_gradient_above_its_slot_count():
    """8200 atoms on 8192 slots: two atoms per slot, the trailing slots own none (the largest case: 8200 x 64 x 9 floats per tensor)."""
    sig = (2, 2, 0, 64, True)
    irreps = standard_layer(*sig[:3])
    c = contracter("gpu", irreps, 64, True, torch.float32)
    seam_case("gpu", c, irreps, True, torch.float32, "slots", False, _dense_name(sig, "f32") + "_slots", expect_specialised=True, runs=("sorted", "permuted"))


@pytest.mark.parametrize("backend", BACKENDS)
def test_workspace_size_follows_the_kernel_selection(backend):
    """The dense path-weight kernel takes min(N, 8192) + 1 slabs, the general one min(N, 1024) + 1: a workspace sized after the switch
    to the general kernels is accepted there (and gives the right gradient), and refused -- nothing written -- where the plan asks
    for more than it holds."""
    sig = (1, 2, 0, 64, True)
    irreps = standard_layer(*sig[:3])
    c = contracter(backend, irreps, 64, True, torch.float32)
    d = case_data(c, irreps, True, "blocks", torch.float32)
    seam = Seam(backend, c, torch.float32)
    N, slab = d["N"], 64 * c.num_paths * 4
    assert seam.use_general(False) == 1
    dense_bytes = seam.workspace_bytes(N)
    assert seam.use_general(True) == 0
    general_bytes = seam.workspace_bytes(N)
    assert dense_bytes == (min(N, 8192) + 1) * slab and general_bytes == (min(N, 1024) + 1) * slab and general_bytes < dense_bytes
    dev_in = dict(x1=d["x1"].to(seam.dev), go=d["go"].to(seam.dev), rowptr=d["rowptr"].to(seam.dev))
    x2s = d["ref"]["x2s"][0].to(seam.dev)
    try:
        rc, gw = seam.backward_weights("general kernels, sized after the switch", d, dev_in, x2s, None, general_bytes)
        assert rc == 0, seam.lib.lib.aa_last_error()
        check("workspace_general", "gw", gw, *d["ref"]["gw"])
        rc, _ = seam.backward_weights("general kernels, one slab short", d, dev_in, x2s, None, general_bytes - slab)
        assert rc != 0 and b"workspace too small" in seam.lib.lib.aa_last_error()
        assert seam.use_general(False) == 1
        rc, _ = seam.backward_weights("dense kernels, sized for the general ones", d, dev_in, x2s, None, general_bytes)
        assert rc != 0 and b"workspace too small" in seam.lib.lib.aa_last_error()
        rc, gw = seam.backward_weights("dense kernels", d, dev_in, x2s, None, dense_bytes)
        assert rc == 0, seam.lib.lib.aa_last_error()
        check("workspace_dense", "gw", gw, *d["ref"]["gw"])
    finally:
        seam.use_general(False)


# ---- no edges: the library and the ops that wrap it -----------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("which", ["general", "dense"])
def test_no_edges_with_null_edge_tensors(which, backend):
    """A frame or shard without edges: every call returns AA_OK with NULL for every tensor that has no rows -- what `data_ptr()` of an
    empty tensor is -- and `x2s` is zeroed; the op wrappers of allegro_amd/ops.py return empty edge tensors and a zero `x2s`."""
    from allegro_amd import ops  # noqa: F401  (registers the ops)

    irreps, mul = (GOLDEN, 3) if which == "general" else (standard_layer(2, 2, 0), 64)
    dtype = torch.float64 if which == "general" else torch.float32
    c = contracter(backend, irreps, mul, True, dtype)
    seam = Seam(backend, c, dtype)
    assert seam.use_general(False) == (which == "dense")
    lib, N = seam.lib, 3
    u, d1, d2, dout = c.mul, c.base_dim1, c.base_dim2, c.base_dim_out
    rowptr = torch.zeros(N + 1, dtype=torch.int32, device=seam.dev)
    x2s, n = seam.poisoned(N, u, d2)
    lib.check(seam.call(lib.lib.aa_tp_forward, seam.plan, 0, N, None, None, seam.w.data_ptr(), rowptr.data_ptr(), None, SF, x2s.data_ptr(), None), "aa_tp_forward")
    assert bool((seam.taken("x2s", x2s, n, (N, u, d2)) == 0).all())
    for gx in (None, x2s.data_ptr()):  # (no gradient has a row: no output is needed either)
        lib.check(seam.call(lib.lib.aa_tp_backward, seam.plan, 0, N, None, None, seam.w.data_ptr(), rowptr.data_ptr(), None, SF, None, gx, gx), "aa_tp_backward")
    assert bool((seam.taken("x2s", x2s, n, (N, u, d2)) == 0).all())
    # no atoms either: no x2s
    lib.check(seam.call(lib.lib.aa_tp_forward, seam.plan, 0, 0, None, None, seam.w.data_ptr(), rowptr.data_ptr(), None, SF, None, None), "aa_tp_forward")
    # edges but no tensors is still refused
    assert seam.call(lib.lib.aa_tp_forward, seam.plan, 1, N, None, None, seam.w.data_ptr(), rowptr.data_ptr(), None, SF, x2s.data_ptr(), None) != 0
    assert seam.call(lib.lib.aa_tp_backward, seam.plan, 1, N, None, None, seam.w.data_ptr(), rowptr.data_ptr(), None, SF, None, None, None) != 0

    e1, e2, eo = (torch.empty(0, u, k, dtype=dtype, device=seam.dev) for k in (d1, d2, dout))
    out, s = torch.ops.allegro_amd.tp_forward(e1, e2, seam.w, rowptr, None, N, SF, seam.plan, c._lib_id, d2, dout)
    assert out.shape == (0, u, dout) and s.shape == (N, u, d2) and bool((s == 0).all())
    g1, g2 = torch.ops.allegro_amd.tp_backward(eo, e1, s, seam.w, rowptr, None, N, SF, seam.plan, c._lib_id)
    assert g1.shape == (0, u, d1) and g2.shape == (0, u, d2)
    assert torch.ops.allegro_amd.tp_backward_x1(eo, s, seam.w, rowptr, None, N, SF, seam.plan, c._lib_id, d1).shape == (0, u, d1)
    assert torch.ops.allegro_amd.tp_backward_x2(eo, e1, seam.w, rowptr, None, N, SF, seam.plan, c._lib_id, d2).shape == (0, u, d2)
    gw = torch.ops.allegro_amd.tp_backward_weights(eo, e1, s, seam.w, rowptr, None, N, seam.plan, c._lib_id)
    assert gw.shape == seam.w.shape and bool((gw == 0).all())
    seg = torch.ops.allegro_amd.segment_sum(e2, rowptr, None, N, SF, c._lib_id)
    assert seg.shape == (N, u, d2) and bool((seg == 0).all())


# ---- through the modules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("which", ["general", "dense"])
def test_contracter_module_with_atoms_left_out_and_without_edges(which, backend):
    """`HipContracter.forward` and autograd through it, in eval mode (the inference op) and in training mode (the differentiable
    segmented contraction), with scatter indices that leave atoms out and with none at all, against the eager contraction."""
    from oracle import restatement as R

    irreps, mul = (GOLDEN, 3) if which == "general" else (standard_layer(2, 2, 0), 64)
    dtype = torch.float64 if which == "general" else torch.float32
    lib, dev = _backend(backend)
    c = contracter(backend, irreps, mul, True, dtype)
    Seam(backend, c, dtype).use_general(False)
    N = 9
    g = torch.Generator().manual_seed(3)
    for name, idxs in (("atoms_left_out", torch.tensor([7, 2, 2, 5, 7, 2, 4, 7, 7, 2, 5])), ("no_edges", torch.zeros(0, dtype=torch.int64))):
        E = idxs.numel()
        x1h = torch.randn(E, mul, c.base_dim1, dtype=dtype, generator=g)
        x2h = torch.randn(E, mul, c.base_dim2, dtype=dtype, generator=g)
        goh = torch.randn(E, mul, c.base_dim_out, dtype=dtype, generator=g)
        want = {}
        if E:
            for dt in (torch.float64,) + ((torch.float32,) if dtype == torch.float32 else ()):
                a, b = x1h.to(dt).requires_grad_(True), x2h.to(dt).requires_grad_(True)
                w = c.weights.detach().cpu().to(dt).requires_grad_(True)
                y = R.contracter_forward(a, b, idxs, N, w, c.w3j.detach().cpu().to(dt), True, SF)
                want[dt] = (y.detach(),) + torch.autograd.grad(y, [a, b, w], goh.to(dt))
        for mode in ("eval", "train"):
            c.train(mode == "train")
            x1, x2 = x1h.to(dev).requires_grad_(True), x2h.to(dev).requires_grad_(True)
            y = c(x1, x2, idxs.to(dev), N)
            assert y.shape == (E, mul, c.base_dim_out)
            g1, g2, gw = torch.autograd.grad(y, [x1, x2, c.weights], goh.to(dev))
            got = (y.detach().cpu(), g1.cpu(), g2.cpu(), gw.cpu())
            assert got[1].shape == x1h.shape and got[2].shape == x2h.shape and got[3].shape == c.weights.shape
            if not E:
                assert bool((got[3] == 0).all()), (name, mode)
                continue
            for q, t, w64, w32 in zip(("out", "gx1", "gx2", "gw"), got, want[torch.float64], want.get(torch.float32, (None,) * 4)):
                check(f"module_{which}_{name}_{mode}", q, t, w32, w64)
    c.eval()
