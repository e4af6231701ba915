"""Host-side mirror of the reference's operator / module interface for the hot path.

* `HipContracter`  -- same constructor, parameters (`weights`), persistent buffer (`w3j`) and
  `forward(x1, x2, idxs, scatter_dim_size)` contract as `allegro.nn._strided.Contracter`
  (allegro/nn/_strided/_contract.py:33-211), backed by the HIP tensor-product operator.
* `HipAllegroModel` -- same hyper-parameters and the same `state_dict` keys as
  `allegro.model.AllegroModel` (allegro/model/allegro_models.py:101-103,112-300), so
  `hip_model.load_state_dict(reference_model.state_dict())` is the drop-in step
  (the reference's own modifier swap relies on exactly that, _contract.py:277).  `forward(data)`
  returns `atomic_energy`, `total_energy`, `forces` computed by one C-ABI call
  (`aa_model_energy_forces`): forward and the hand-written reverse pass, all in HIP.

PyTorch is used for device memory, streams and parameter bookkeeping only.  There is no CPU
fallback: on a tensor that is not on a GPU these modules raise.
"""
import ctypes as C
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops, o3

_TORCH2AA = {torch.float32: _lib.AA_F32, torch.float64: _lib.AA_F64}


ACT_KINDS = {"silu": 0, "mish": 1, "gelu": 2, None: 3}


def second_moment_const(nonlinearity: Optional[str] = "silu") -> float:
    """normalize2mom constant of an activation, 1/sqrt(E_{z~N(0,1)}[act(z)^2]), by quadrature (the constant nequip's
    ScalarMLPFunction folds into the layer after an activation); 1 for `None`."""
    if nonlinearity is None:
        return 1.0
    z = np.linspace(-12.0, 12.0, 240001)
    w = np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    if nonlinearity == "silu":
        a = z / (1.0 + np.exp(-z))
    elif nonlinearity == "mish":
        a = z * np.tanh(np.logaddexp(0.0, z))
    elif nonlinearity == "gelu":
        from math import erf

        a = 0.5 * z * (1.0 + np.vectorize(erf)(z / math.sqrt(2.0)))
    else:
        raise NotImplementedError(f"nonlinearity {nonlinearity!r}: the reference offers silu, mish, gelu, None")
    f = a * a * w
    return 1.0 / math.sqrt(float(np.sum((f[1:] + f[:-1]) * 0.5 * (z[1] - z[0]))))


def silu_second_moment_const() -> float:
    return second_moment_const("silu")


def _stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0


def _device_ctx(device):
    """Make `device` the current HIP device for plan creation / packing / launches (plans and packed weights are
    device-specific; kernels are enqueued on that device's current stream)."""
    device = torch.device(device)
    if device.type == "cuda":
        return torch.cuda.device(device)
    import contextlib

    return contextlib.nullcontext()


def _require_gpu(lib: _lib.AllegroLib, t: torch.Tensor, what: str):
    if not t.is_cuda and not lib.is_emulation:
        raise _lib.AllegroError(f"{what}: tensors must live on the GPU (got {t.device}); there is no CPU fallback")


# ------------------------------------------------------------------------------------------------
# irreps logic of the Allegro layer stack
# ------------------------------------------------------------------------------------------------
def allegro_layer_irreps(l_max: int, parity: bool, num_layers: int) -> List[o3.Irreps]:
    """Per-layer tensor-track irreps: forward reachability then backward pruning.
    Mirrors allegro/nn/_allegro.py:101-160 (and the allowed set of allegro_models.py:76-86).
    Returns tps_irreps[0..L]: input irreps of layer l = [l], output = [l+1]."""
    env = o3.Irreps.spherical_harmonics(l_max, p=-1)
    if parity:
        allowed = o3.Irreps([(1, (l, p)) for l in range(l_max + 1) for p in (1, -1)])
    else:
        allowed = env
    arg = env
    tps = [arg]
    for layer in range(num_layers):
        ir_out = o3.Irreps([(1, (0, 1))]) if layer == num_layers - 1 else allowed
        ir_out = o3.Irreps([(m, ir) for m, ir in ir_out if o3.tp_path_exists(arg, env, ir)])
        arg = ir_out
        tps.append(ir_out)
    out = tps[-1]
    new = [out]
    for arg in reversed(tps[:-1]):
        keep = []
        for m, arg_ir in arg:
            if any(any(i in out for i in arg_ir * env_ir) for _, env_ir in env):
                keep.append((m, arg_ir))
        out = o3.Irreps(keep)
        new.append(out)
    tps = list(reversed(new))
    assert tps[-1].lmax == 0
    return tps


def build_w3j(irreps_in1: o3.Irreps, irreps_in2: o3.Irreps, irreps_out: o3.Irreps,
              instructions: Optional[Sequence[Tuple[int, int, int]]] = None, irrep_normalization="component"):
    """The dense `w3j` buffer exactly as Contracter.__init__ lays it out (_contract.py:48-168):
    instructions enumerated in (i_out, i_1, i_2) loop order, values x sqrt(2 l_out + 1), [p,i,k] when
    ij-diagonal else [p,i,j,k], path dim squeezed when there is a single path."""
    if instructions is None:
        instructions = []
        for i_out, (_, ir_out) in enumerate(irreps_out):
            for i_1, (_, ir_1) in enumerate(irreps_in1):
                for i_2, (_, ir_2) in enumerate(irreps_in2):
                    if ir_out in (ir_1 * ir_2):
                        instructions.append((i_1, i_2, i_out))
    assert len(instructions) > 0, "No TP paths available"
    o1, o2, oo = irreps_in1.offsets(), irreps_in2.offsets(), irreps_out.offsets()
    d1, d2, dout = irreps_in1.dim, irreps_in2.dim, irreps_out.dim
    blocks = []
    for (i_1, i_2, i_out) in instructions:
        ir1, ir2, iro = irreps_in1[i_1][1], irreps_in2[i_2][1], irreps_out[i_out][1]
        assert ir1.p * ir2.p == iro.p and abs(ir1.l - ir2.l) <= iro.l <= ir1.l + ir2.l
        w = o3.wigner_3j(ir1.l, ir2.l, iro.l)
        if irrep_normalization == "component":
            w = w * math.sqrt(2 * iro.l + 1)
        elif irrep_normalization is not None:
            raise NotImplementedError(irrep_normalization)
        blocks.append((o1[i_1], o2[i_2], oo[i_out], w))
    diag = d1 == d2 and all(
        all(o_a + i == o_b + j for i, j, _ in zip(*np.nonzero(w))) for o_a, o_b, _, w in blocks)
    P = len(instructions)
    if diag:
        w3j = np.zeros((P, d1, dout))
        for p, (a, b, c, w) in enumerate(blocks):
            for i, j, k in zip(*np.nonzero(w)):
                w3j[p, a + i, c + k] = w[i, j, k]
    else:
        w3j = np.zeros((P, d1, d2, dout))
        for p, (a, b, c, w) in enumerate(blocks):
            w3j[p, a:a + w.shape[0], b:b + w.shape[1], c:c + w.shape[2]] = w
    if P == 1:
        w3j = w3j[0]
    return w3j, list(instructions), bool(diag), (d1, d2, dout)


def w3j_to_desc(w3j: torch.Tensor, mul: int, dims: Tuple[int, int, int], num_paths: int, diag: bool, coupling: bool):
    """Sparse non-zeros of a (possibly squeezed) w3j buffer -> C descriptor."""
    d1, d2, dout = dims
    w = w3j.detach().to("cpu", torch.float64).numpy()
    if num_paths == 1:
        w = w[None]
    if diag:
        p, i, k = np.nonzero(w)
        j = i
        val = w[p, i, k]
    else:
        p, i, j, k = np.nonzero(w)
        val = w[p, i, j, k]
    return _lib.make_tp_desc(mul, d1, d2, dout, num_paths, coupling, i, j, k, p, val)


# ------------------------------------------------------------------------------------------------
# segment bookkeeping
# ------------------------------------------------------------------------------------------------
def segments_from_index(idxs: torch.Tensor, num_segments: int, assume_sorted: bool = False):
    """rowptr[int32, N+1] and (if idxs is not sorted) the stable sort permutation eids[int32, E].
    `assume_sorted=True` skips the sortedness check, i.e. the only device->host synchronisation of this function
    (the caller vouches that `idxs` is non-decreasing, as the center index of a model's edge list is)."""
    idxs = idxs.reshape(-1)
    is_sorted = True
    if not assume_sorted and idxs.numel() > 1:
        is_sorted = bool((idxs[1:] >= idxs[:-1]).all())
    eids = None
    if not is_sorted:
        eids = torch.argsort(idxs, stable=True).to(torch.int32)
    counts = torch.bincount(idxs, minlength=num_segments)
    rowptr = torch.zeros(num_segments + 1, dtype=torch.int32, device=idxs.device)
    rowptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return rowptr, eids


class _SegmentCache:
    """rowptr / eids of the most recent index tensors, keyed on (storage address, in-place version, length, segment
    count).  The keyed tensor is kept alive by the entry, so its address cannot be recycled for another tensor
    while the entry exists.  All Contracters of a model receive the SAME `idxs` tensor in every layer
    (allegro/nn/_allegro.py:238,268), so one entry serves the whole forward; a handful covers train/val alternation."""

    def __init__(self, capacity: int = 4):
        self.capacity = capacity
        self.entries = []  # [(key, idxs_ref, rowptr, eids)]

    def get(self, idxs: torch.Tensor, num_segments: int, assume_sorted: bool):
        key = (idxs.data_ptr(), int(idxs._version), int(idxs.numel()), int(num_segments), str(idxs.device), bool(assume_sorted))
        for i, (k, _ref, rowptr, eids) in enumerate(self.entries):
            if k == key:
                if i:
                    self.entries.insert(0, self.entries.pop(i))
                return rowptr, eids
        rowptr, eids = segments_from_index(idxs, num_segments, assume_sorted)
        self.entries.insert(0, (key, idxs, rowptr, eids))
        del self.entries[self.capacity:]
        return rowptr, eids


_SEGMENTS = _SegmentCache()


def _is_tracing() -> bool:
    """True under torch.compile / torch.export tracing (FakeTensors: no addresses, no values)."""
    c = torch.compiler
    return bool(c.is_compiling() or (hasattr(c, "is_exporting") and c.is_exporting()))


# ------------------------------------------------------------------------------------------------
# Contracter (seam B1/B2)
# ------------------------------------------------------------------------------------------------
class HipContracter(torch.nn.Module):
    """Drop-in for `Contracter` (allegro/nn/_strided/_contract.py:11-251) on the HIP operator."""

    def __init__(self, irreps_in1, irreps_in2, irreps_out, mul: int, instructions=None,
                 path_channel_coupling: bool = True, scatter_factor: Optional[float] = None,
                 irrep_normalization: str = "component"):
        super().__init__()
        self.irreps_in1, self.irreps_in2, self.irreps_out = o3.Irreps(irreps_in1), o3.Irreps(irreps_in2), o3.Irreps(irreps_out)
        for irr in (self.irreps_in1, self.irreps_in2, self.irreps_out):
            assert all(m == 1 for m, _ in irr)
        assert mul > 0
        self.mul = mul
        self.scatter_factor = scatter_factor
        self.irrep_normalization = irrep_normalization
        self.path_channel_coupling = path_channel_coupling
        w3j, instr, diag, (d1, d2, dout) = build_w3j(self.irreps_in1, self.irreps_in2, self.irreps_out, instructions,
                                                      irrep_normalization)
        self.instructions = instructions
        self.num_paths = len(instr)
        self.w3j_is_ij_diagonal = diag
        self.base_dim1, self.base_dim2, self.base_dim_out = d1, d2, dout
        self.register_buffer("w3j", torch.tensor(w3j, dtype=torch.get_default_dtype()))
        shape = (mul,) if path_channel_coupling else tuple()
        if self.num_paths > 1:
            shape = shape + (self.num_paths,)
        self.weights = torch.nn.Parameter(torch.empty(shape).uniform_(-math.sqrt(3), math.sqrt(3)))
        self._plans: Dict[tuple, int] = {}  # (dtype, device index) -> aa_tp_plan*
        self._keep = []
        self._bound_lib: Optional[_lib.AllegroLib] = None
        self._lib_id = 0
        # set True when the caller guarantees center-sorted `idxs` (skips the sortedness check and its host sync)
        self.assume_sorted_idxs = False

    def _get_lib(self) -> _lib.AllegroLib:
        return self._bound_lib if self._bound_lib is not None else _lib.load()

    def _bind_library(self, lib: _lib.AllegroLib):
        """(tests) bind an explicitly loaded library instead of the default gfx950 one."""
        self._bound_lib = lib
        self._lib_id = ops.register_library(lib)
        self._plans.clear()

    def _plan(self, dtype, device=None) -> int:
        """The plan owns device-resident Clebsch-Gordan tables: one per (dtype, device), created with that device current."""
        dev = torch.device("cpu") if device is None else torch.device(device)
        key = (dtype, dev.index if dev.type == "cuda" else -1)
        if key not in self._plans:
            desc, keep = w3j_to_desc(self.w3j, self.mul, (self.base_dim1, self.base_dim2, self.base_dim_out),
                                     self.num_paths, self.w3j_is_ij_diagonal, self.path_channel_coupling)
            self._keep.append(keep)
            with _device_ctx(dev):
                self._plans[key] = self._get_lib().tp_plan_create(desc, _TORCH2AA[dtype])
        return self._plans[key]

    def forward(self, x1, x2, idxs, scatter_dim_size):
        if isinstance(scatter_dim_size, torch.Tensor):
            scatter_dim_size = int(scatter_dim_size.reshape(-1)[0])
        x1 = x1.reshape(-1, self.mul, self.base_dim1)
        x2 = x2.reshape(-1, self.mul, self.base_dim2)
        sf = 1.0 if self.scatter_factor is None else float(self.scatter_factor)
        if self.training and torch.is_grad_enabled():
            # training: the arbitrarily differentiable form of the WHOLE forward (scale + scatter + gather + contraction) on
            # the segmented kernels (ops.contract_segments_differentiable) -- a force-matching loss differentiates the
            # forces again.  (The reference's Triton contracter falls back to the eager formulation when training,
            # _flashallegro.py:725-755; its cuEquivariance contracter keeps the fused gather, _cueq_contracter.py:84-131.)
            if os.environ.get("AA_TRAIN_PER_EDGE", "0")[:1] == "1":  # (A/B: the first formulation, every edge its own segment)
                x2s = torch.zeros((int(scatter_dim_size),) + tuple(x2.shape[1:]), dtype=x2.dtype, device=x2.device)
                x2s = x2s.index_add(0, idxs.reshape(-1), sf * x2)
                return self._contract(x1, x2s.index_select(0, idxs.reshape(-1)))
            rowptr, eids = _SEGMENTS.get(idxs, scatter_dim_size, self.assume_sorted_idxs)
            _require_gpu(self._get_lib(), x1, "HipContracter")
            with _device_ctx(x1.device):
                return ops.contract_segments_differentiable(x1, x2, self.weights, rowptr, eids, idxs, int(scatter_dim_size), sf,
                                                            self._plan(x1.dtype, x1.device), self._lib_id, self.base_dim1,
                                                            self.base_dim2, self.base_dim_out)
        if _is_tracing():
            # torch.export / torch.compile: no data pointers, no data-dependent Python -- the bookkeeping is one opaque
            # op with a fake kernel (ops.segments); plan handles are process-local, so a traced program is valid in
            # THIS process (a Python-free host loads the whole-step op of allegro_amd/export.py instead)
            rowptr, eids = torch.ops.allegro_amd.segments(idxs, scatter_dim_size, self.assume_sorted_idxs)
            return self._op(x1, x2, rowptr, None if self.assume_sorted_idxs else eids, scatter_dim_size, sf)
        # per-call host sync / bincount / cumsum only on the first layer of the first forward with this index tensor
        rowptr, eids = _SEGMENTS.get(idxs, scatter_dim_size, self.assume_sorted_idxs)
        return self._op(x1, x2, rowptr, eids, int(scatter_dim_size), sf)

    def _op(self, x1, x2, rowptr, eids, num_atoms: int, scatter_factor: float):
        """The registered library op (allegro_amd/ops.py).  Autograd gives the x1 / x2 gradients and -- when the path
        weights require grad (training, like the reference's eager and cuEquivariance contracters,
        _contract.py:172-177) -- the weight gradient from `aa_tp_backward_weights`."""
        _require_gpu(self._get_lib(), x1, "HipContracter")
        with _device_ctx(x1.device):
            out, _x2s = torch.ops.allegro_amd.tp_forward(x1, x2, self.weights, rowptr, eids, num_atoms,
                                                         scatter_factor, self._plan(x1.dtype, x1.device), self._lib_id,
                                                         self.base_dim2, self.base_dim_out)
        return out

    def _contract(self, x1, x2):
        """Contraction only (seam B1, _contract.py:213): every edge is its own segment.  Differentiable to any order
        (x1, x2 and the path weights)."""
        _require_gpu(self._get_lib(), x1, "HipContracter")
        with _device_ctx(x1.device):
            return ops.contract_differentiable(x1, x2, self.weights, self._plan(x1.dtype, x1.device), self._lib_id,
                                               self.base_dim1, self.base_dim2, self.base_dim_out)

    @classmethod
    def from_contracter(cls, old: torch.nn.Module) -> "HipContracter":
        """Build from a reference `Contracter` instance (same constructor attributes and state_dict keys,
        _contract.py:72-76,165-177) -- the `factory` of the reference's `enable_*Contracter` modifiers (:262-279)."""
        prev = torch.get_default_dtype()
        torch.set_default_dtype(old.w3j.dtype)
        try:
            new = cls(irreps_in1=str(old.irreps_in1), irreps_in2=str(old.irreps_in2), irreps_out=str(old.irreps_out),
                      mul=old.mul, instructions=old.instructions, path_channel_coupling=old.path_channel_coupling,
                      scatter_factor=old.scatter_factor, irrep_normalization=old.irrep_normalization)
        finally:
            torch.set_default_dtype(prev)
        new.load_state_dict(old.state_dict())
        return new.to(old.weights.device)

    def extra_repr(self):
        return f"{self.irreps_in1} x {self.irreps_in2} -> {self.irreps_out} | {self.mul} channels | {self.num_paths} paths"

    def __del__(self):
        try:
            for h in self._plans.values():
                self._get_lib().tp_plan_destroy(h)
        except Exception:
            pass


def replace_submodules(model: torch.nn.Module, target_cls, factory) -> torch.nn.Module:
    """Recursively replace every instance of `target_cls` by `factory(old)` (nequip.nn.replace_submodules, EXT)."""
    if isinstance(model, target_cls):
        return factory(model)
    for name, child in list(model.named_children()):
        setattr(model, name, replace_submodules(child, target_cls, factory))
    return model


class _DuckContracterMeta(type):
    """isinstance(obj, AnyContracter) <=> obj carries a reference Contracter's attributes and is not already a
    HipContracter (so the modifier works on the reference's class without importing it)."""
    _ATTRS = ("irreps_in1", "irreps_in2", "irreps_out", "mul", "w3j", "weights", "path_channel_coupling")

    def __instancecheck__(cls, obj):
        return (not isinstance(obj, HipContracter)) and all(hasattr(obj, a) for a in cls._ATTRS)


class AnyContracter(metaclass=_DuckContracterMeta):
    pass


def enable_HipContracter(model: torch.nn.Module, contracter_cls=None) -> torch.nn.Module:
    """Model modifier: swap every `Contracter` of `model` for the HIP operator -- the analogue of
    `Contracter.enable_TritonContracter` (_contract.py:253-282).  `contracter_cls` defaults to any module that
    carries a Contracter's attributes.  Unlike the Triton kernel there is no build-time guard: ij-diagonal,
    single-path and uncoupled modes are all covered, and so is training mode (weight gradients).

    Discovery through nequip (`nequip.model.modify` in a config, `nequip-compile --modifiers enable_HipContracter`):
    `allegro_amd._nequip_ext.register()` -- run by the `nequip.extension` entry point of this package's
    pyproject.toml, like the reference's own `init_always = "allegro"` (pyproject.toml:50-51) -- attaches this
    function to the reference's `Contracter` as a `@model_modifier(persistent=False) @classmethod`, the exact form of
    `_contract.py:253-255,284-286`."""
    return replace_submodules(model, AnyContracter if contracter_cls is None else contracter_cls,
                              HipContracter.from_contracter)


def _enable_HipContracter_classmethod(cls, model):
    """Body of the classmethod attached to the reference's Contracter (and to HipContracter below): replaces
    instances of `cls` -- the signature nequip's modifier machinery calls, `_contract.py:255,282`."""
    target = AnyContracter if cls is HipContracter else cls
    return replace_submodules(model, target, HipContracter.from_contracter)


HipContracter.enable_HipContracter = classmethod(_enable_HipContracter_classmethod)


# ------------------------------------------------------------------------------------------------
# whole model
# ------------------------------------------------------------------------------------------------
class _Node(torch.nn.Module):
    """Plain container used to reproduce the reference's state_dict key hierarchy."""


def _ensure_path(root: torch.nn.Module, dotted: str) -> Tuple[torch.nn.Module, str]:
    parts = dotted.split(".")
    node = root
    for name in parts[:-1]:
        if not hasattr(node, name):
            node.add_module(name, _Node())
        node = getattr(node, name)
    return node, parts[-1]


_BESSEL_CONVENTIONS = {"auto": 0, "npi": 1, "sinc": 2}


class PreparedGraph:
    """Device-resident center-sorted CSR view of an edge list (the `aa_graph` struct)."""

    def __init__(self, edge_index: torch.Tensor, atom_types: torch.Tensor, num_atoms: int,
                 shift_vec: Optional[torch.Tensor] = None, transposed: bool = True,
                 rowptr: Optional[torch.Tensor] = None, lib: Optional[_lib.AllegroLib] = None):
        center = edge_index[0]
        self.perm = None
        # (a list that comes with its row pointers -- the device neighbour list -- is center-sorted by construction: no check, no sync)
        if rowptr is None and center.numel() > 1 and not bool((center[1:] >= center[:-1]).all()):
            self.perm = torch.argsort(center, stable=True)
            edge_index = edge_index[:, self.perm]
            if shift_vec is not None:
                shift_vec = shift_vec[self.perm]
        self.num_atoms, self.num_edges = int(num_atoms), int(edge_index.shape[1])
        self.center = edge_index[0].to(torch.int32).contiguous()
        self.nbr = edge_index[1].to(torch.int32).contiguous()
        if rowptr is not None:  # already known (device neighbor list)
            self.rowptr = rowptr.to(torch.int32).contiguous()
        else:
            counts = torch.bincount(edge_index[0], minlength=num_atoms)
            self.rowptr = torch.zeros(num_atoms + 1, dtype=torch.int32, device=edge_index.device)
            self.rowptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
        self.types = atom_types.reshape(-1).to(torch.int32).contiguous()
        self.shift_vec = None if shift_vec is None else shift_vec.contiguous()
        # block of center atoms that have edges (the owned block of an atom-block partition, allegro_amd/dist.py):
        # the per-atom kernels only visit it.  One host read at graph-preparation time, none per step.
        self.atom_begin = self.atom_end = self.max_degree = 0
        # transposed CSR (edges grouped by neighbor): lets the library gather forces per atom in a fixed order
        # (bit-reproducible); without it neighbor contributions are accumulated with floating-point atomics
        self.t_perm = self.t_rowptr = None
        if lib is None and edge_index.is_cuda:
            lib = _lib.load()
        if transposed and lib is not None and (edge_index.is_cuda or lib.is_emulation):
            # one library call per neighbour list (`aa_graph_transpose`: counting sort + per-atom group sort + the three hints) and
            # ONE host read, instead of argsort / bincount / cumsum / max through a dozen tensor operations: an MD loop prepares a
            # graph per list (0.28 -> ~0.1 ms; profiles/r05_*_md_loop_c3.json)
            dev = edge_index.device
            self.t_rowptr = torch.empty(num_atoms + 1, dtype=torch.int32, device=dev)
            self.t_perm = torch.empty(self.num_edges, dtype=torch.int32, device=dev)
            hints = torch.empty(3, dtype=torch.int32, device=dev)
            nbytes = lib.lib.aa_graph_transpose_workspace_bytes(num_atoms)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            with _device_ctx(dev):
                lib.check(lib.lib.aa_graph_transpose(num_atoms, self.num_edges, self.rowptr.data_ptr(), self.nbr.data_ptr(), self.t_rowptr.data_ptr(),
                                                     self.t_perm.data_ptr() if self.num_edges else None, hints.data_ptr(), ws.data_ptr(), nbytes,
                                                     _stream_ptr(edge_index)), "aa_graph_transpose")
            self.atom_begin, self.atom_end, self.max_degree = (int(v) for v in hints.tolist())
            return
        if self.num_edges > 0:
            # largest edge segment: <= 32 selects the fused per-atom-tile kernels (one wave = one atom's MFMA tile); ONE host read
            # for the three hints
            deg_max = (self.rowptr[1:] - self.rowptr[:-1]).max().to(torch.int32)
            first, last, dmax = torch.stack([self.center[0], self.center[-1], deg_max]).tolist()
            self.atom_begin, self.atom_end, self.max_degree = int(first), int(last) + 1, int(dmax)
        if transposed:
            self.t_perm = torch.argsort(edge_index[1], stable=True).to(torch.int32).contiguous()
            self.t_rowptr = torch.zeros(num_atoms + 1, dtype=torch.int32, device=edge_index.device)
            self.t_rowptr[1:] = torch.cumsum(torch.bincount(edge_index[1], minlength=num_atoms), 0).to(torch.int32)

    @classmethod
    def from_edge_index(cls, edge_index: torch.Tensor, atom_types: torch.Tensor, num_atoms: int,
                        shift_vec: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None, cutoffs=None,
                        lib: Optional[_lib.AllegroLib] = None) -> "PreparedGraph":
        """The graph of ANY edge list -- int64 or int32 `edge_index` [2, E], edges in any order, rows a stride apart -- built by the
        library in one operation (`aa_graph_build_count` / `aa_graph_build_fill`): center-sorted in stable order, transposed CSR
        and hints included, with ONE host read (the new edge count, the hints, the sortedness of the input).  With `cutoffs`
        ([T, T], e.g. `model.cutoff_table()`; needs `pos`) only the edges with |r_e| < cutoffs[type_center, type_neighbour] are
        kept, the predicate of `DeviceNeighborList.prune`.  The fields mean what they mean after `PreparedGraph(...)`; `perm`
        (int64, the input id of every output edge) is None exactly when the output is the input list unchanged, and
        `input_is_sorted` tells whether the input's center row was non-decreasing.  An index outside [0, num_atoms) is an
        AllegroError naming the row and an edge."""
        if cutoffs is not None and pos is None:
            raise ValueError("from_edge_index: cutoffs need pos (the per-type-pair predicate is evaluated on the edge vectors)")
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"from_edge_index: edge_index must be an int32 / int64 [2, E] tensor, not {list(edge_index.shape)} {edge_index.dtype}")
        if lib is None:
            lib = _lib.load()
        _require_gpu(lib, edge_index, "PreparedGraph.from_edge_index")
        N, E, dev = int(num_atoms), int(edge_index.shape[1]), edge_index.device
        if E > 0 and (edge_index.stride(1) != 1 or edge_index.stride(0) < E):  # (rows a stride apart are read in place)
            edge_index = edge_index.contiguous()
        dtype = pos.dtype if pos is not None else (shift_vec.dtype if shift_vec is not None else torch.float32)
        if dtype not in _TORCH2AA:
            raise ValueError(f"from_edge_index: pos / shift_vec must be float32 or float64, not {dtype}")
        if shift_vec is not None and (tuple(shift_vec.shape) != (E, 3) or shift_vec.dtype != dtype or shift_vec.device != dev):
            raise ValueError(f"from_edge_index: shift_vec must be [{E}, 3] {dtype} on {dev}, not {list(shift_vec.shape)} "
                             f"{shift_vec.dtype} on {shift_vec.device}")
        if pos is not None and (tuple(pos.shape) != (N, 3) or pos.device != dev):
            raise ValueError(f"from_edge_index: pos must be [{N}, 3] on {dev}, not {list(pos.shape)} on {pos.device}")
        sv = None if shift_vec is None else shift_vec.detach().contiguous()
        p = None if pos is None else pos.detach().contiguous()
        types, keep = (None, None) if cutoffs is None else _nl_types(atom_types, cutoffs, N, dev, "from_edge_index")
        tref = None if types is None else C.byref(types)
        inp = _lib.EdgeList(N, E, edge_index.data_ptr() if E else None, edge_index.stride(0) if E else 0,
                            int(edge_index.dtype == torch.int64), _TORCH2AA[dtype], p.data_ptr() if p is not None and N else None,
                            sv.data_ptr() if sv is not None and E else None)
        g = cls.__new__(cls)
        nbytes = lib.lib.aa_graph_build_workspace_bytes(N, E)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        g.rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
        n_edges, hints, was_sorted = C.c_int64(), (C.c_int32 * 3)(), C.c_int32()
        stream = _stream_ptr(edge_index)
        with _device_ctx(dev):
            lib.check(lib.lib.aa_graph_build_count(C.byref(inp), tref, ws.data_ptr(), nbytes, g.rowptr.data_ptr(), C.byref(n_edges), hints,
                                                   C.byref(was_sorted), stream), "aa_graph_build_count")
            E2 = int(n_edges.value)
            out = torch.empty((2, E2), dtype=torch.int32, device=dev)
            perm = torch.empty(E2, dtype=torch.int32, device=dev)
            g.shift_vec = None if sv is None else torch.empty((E2, 3), dtype=dtype, device=dev)
            g.t_perm = torch.empty(E2, dtype=torch.int32, device=dev)
            if E2 > 0:
                g.t_rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
                lib.check(lib.lib.aa_graph_build_fill(C.byref(inp), tref, ws.data_ptr(), nbytes, g.rowptr.data_ptr(), out[0].data_ptr(),
                                                      out[1].data_ptr(), perm.data_ptr(),
                                                      g.shift_vec.data_ptr() if g.shift_vec is not None else None,
                                                      g.t_rowptr.data_ptr(), g.t_perm.data_ptr(), stream), "aa_graph_build_fill")
            else:
                g.t_rowptr = torch.zeros(N + 1, dtype=torch.int32, device=dev)
        del keep
        g.num_atoms, g.num_edges = N, E2
        g.center, g.nbr = out[0], out[1]
        g.types = atom_types.reshape(-1).to(torch.int32).contiguous()
        g.input_is_sorted = bool(was_sorted.value)
        g.perm = None if g.input_is_sorted and E2 == E else perm.long()
        g.atom_begin, g.atom_end, g.max_degree = (int(v) for v in hints)
        return g

    def rowptr_host(self):
        """The row pointers as a host int64 array: ONE device read per graph, kept."""
        rp = getattr(self, "_rowptr_host", None)
        if rp is None:
            import numpy as np

            rp = self._rowptr_host = self.rowptr.cpu().numpy().astype(np.int64)
        return rp

    def blocks(self, max_edges: int):
        """Cuts the frame into contiguous blocks of center atoms for the block-wise step (`aa_model_energy_forces_blocked`,
        `HipAllegroModel.energy_forces(..., max_block_edges=)`): greedy, every block takes as many atoms as fit `max_edges` edges
        (atoms without edges ride along with the block in front of them).  Returns (block_atoms, block_edges), host int64 arrays
        [B+1] with block_edges[b] = rowptr[block_atoms[b]].  One atom with more than `max_edges` edges cannot be cut: ValueError."""
        import numpy as np

        rp, n = self.rowptr_host(), self.num_atoms
        max_edges = int(max_edges)
        deg = np.diff(rp)
        if n and int(deg.max()) > max_edges:
            a = int(deg.argmax())
            raise ValueError(f"atom {a} has {int(deg[a])} edges, more than max_edges = {max_edges}: a block holds whole atoms")
        if max_edges < 0:
            raise ValueError(f"max_edges must not be negative, got {max_edges}")
        cuts = [0]
        while cuts[-1] < n:
            # the last atom boundary whose row pointer is within max_edges of the block's first edge (>= one atom: its degree fits)
            cuts.append(min(n, int(np.searchsorted(rp, rp[cuts[-1]] + max_edges, side="right")) - 1))
        if len(cuts) == 1:
            cuts.append(n)  # (no atoms: one empty block)
        block_atoms = np.asarray(cuts, dtype=np.int64)
        return block_atoms, rp[block_atoms].copy()

    def c_struct(self) -> _lib.Graph:
        return _lib.Graph(self.num_atoms, self.num_edges, self.center.data_ptr(), self.nbr.data_ptr(),
                          self.rowptr.data_ptr(), self.types.data_ptr(),
                          self.shift_vec.data_ptr() if self.shift_vec is not None else None,
                          self.t_rowptr.data_ptr() if self.t_rowptr is not None else None,
                          self.t_perm.data_ptr() if self.t_perm is not None else None,
                          self.atom_begin, self.atom_end, self.max_degree)


def _max_degree(graph: PreparedGraph) -> int:
    """Largest edge segment of `graph`: its hint where the graph carries one, else from the host copy of the row pointers."""
    if graph.max_degree > 0 or graph.num_edges == 0:
        return int(graph.max_degree)
    import numpy as np

    return int(np.diff(graph.rowptr_host()).max())


def _nl_types(atom_types: torch.Tensor, cutoffs, num_atoms: int, device, what: str):
    """`aa_nl_types` of (atom_types, cutoffs) + what keeps its pointers alive.  The shapes are checked here; the values (table
    entries positive and finite, at most 64 types, atom types inside the table) are checked by the library."""
    table = torch.as_tensor(cutoffs).detach().to(device="cpu", dtype=torch.float64)
    if table.dim() != 2 or table.shape[0] != table.shape[1]:
        raise ValueError(f"{what}: cutoffs must be a square [T, T] table (row = center type, column = neighbour type), "
                         f"not {list(table.shape)}")
    if atom_types.dtype not in (torch.int32, torch.int64) or atom_types.numel() != num_atoms:
        raise ValueError(f"{what}: atom_types must be {num_atoms} int32 or int64 values, not {list(atom_types.shape)} "
                         f"{atom_types.dtype}")
    if atom_types.device != device:
        raise ValueError(f"{what}: atom_types live on {atom_types.device}, the positions on {device}")
    table = np.ascontiguousarray(table.numpy())
    types = atom_types.detach().reshape(-1).contiguous()
    st = _lib.NlTypes(int(table.shape[0]), int(types.dtype == torch.int64), table.ctypes.data_as(_lib._dp), types.data_ptr())
    return st, (table, types)


class DeviceNeighborList:
    """Result of `neighbor_list`: center-sorted edges on the device (`aa_nl_count` / `aa_nl_fill`).  `kept` (lists made by
    `prune` only): for every edge its index in the list it was pruned from."""

    def __init__(self, edge_index, rowptr, cell_shift, shift_vec, lib=None, kept=None):
        self.edge_index, self.rowptr, self.cell_shift, self.shift_vec, self._lib = edge_index, rowptr, cell_shift, shift_vec, lib
        self.kept = kept

    @property
    def num_edges(self) -> int:
        return int(self.edge_index.shape[1])

    def prepare(self, atom_types: torch.Tensor, transposed: bool = True) -> PreparedGraph:
        return PreparedGraph(self.edge_index, atom_types, self.rowptr.numel() - 1, self.shift_vec, transposed=transposed,
                             rowptr=self.rowptr, lib=self._lib)

    def prune(self, pos: torch.Tensor, atom_types: torch.Tensor, cutoffs) -> "DeviceNeighborList":
        """The sub-list of the edges with |r_e| < cutoffs[type_center, type_neighbour] (`aa_graph_prune_*`; `cutoffs`: [T, T],
        e.g. `model.cutoff_table()`), in the same order: what `neighbor_list(..., atom_types=, cutoffs=)` builds directly, for a
        list that exists already.  `cell_shift` follows through `kept` [E'], the surviving edges' indices in this list.  Only
        the new edge count crosses to the host."""
        lib = self._lib if self._lib is not None else _lib.load()
        _require_gpu(lib, pos, "DeviceNeighborList.prune")
        N, E, dev = self.rowptr.numel() - 1, self.num_edges, self.edge_index.device
        if pos.dtype not in _TORCH2AA or tuple(pos.shape) != (N, 3) or pos.device != dev:
            raise ValueError(f"prune: pos must be [{N}, 3] float32 / float64 on {dev}, not {list(pos.shape)} {pos.dtype} on {pos.device}")
        if self.shift_vec is not None and self.shift_vec.dtype != pos.dtype:
            raise ValueError(f"prune: pos is {pos.dtype}, the list's shift_vec {self.shift_vec.dtype}")
        pos = pos.detach().contiguous()
        types, keep = _nl_types(atom_types, cutoffs, N, dev, "prune")
        nbr = self.edge_index[1].contiguous()
        rowptr_in = self.rowptr.contiguous()
        sv = None if self.shift_vec is None else self.shift_vec.contiguous()
        inp = _lib.PruneInput(N, E, pos.data_ptr(), _TORCH2AA[pos.dtype], rowptr_in.data_ptr(), nbr.data_ptr() if E else None,
                              sv.data_ptr() if sv is not None and E else None)
        nbytes = lib.lib.aa_graph_prune_workspace_bytes(N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
        n_edges = C.c_int64()
        stream = _stream_ptr(pos)
        with _device_ctx(dev):
            lib.check(lib.lib.aa_graph_prune_count(C.byref(inp), C.byref(types), ws.data_ptr(), nbytes, rowptr.data_ptr(),
                                                   C.byref(n_edges), stream), "aa_graph_prune_count")
            E2 = int(n_edges.value)
            edge_index = torch.empty((2, E2), dtype=torch.int32, device=dev)
            shift_vec = None if sv is None else torch.empty((E2, 3), dtype=pos.dtype, device=dev)
            kept = torch.empty(E2, dtype=torch.int32, device=dev)
            if E2 > 0:
                lib.check(lib.lib.aa_graph_prune_fill(C.byref(inp), C.byref(types), ws.data_ptr(), nbytes, rowptr.data_ptr(),
                                                      edge_index[0].data_ptr(), edge_index[1].data_ptr(),
                                                      shift_vec.data_ptr() if shift_vec is not None else None, kept.data_ptr(), stream),
                          "aa_graph_prune_fill")
        del keep
        cell_shift = None if self.cell_shift is None else self.cell_shift.index_select(0, kept.long())
        return DeviceNeighborList(edge_index, rowptr, cell_shift, shift_vec, lib, kept=kept)

    def ghost_layout(self, pos: torch.Tensor, atom_types: torch.Tensor):
        """The same list in the ghost-atom layout of the reference's `pair_allegro` contract (allegro/_compile.py:28-63),
        built on the device: every outside-cell edge gets its own ghost atom (not deduplicated) at `pos[nbr] + shift`,
        ghosts are appended after the real atoms, no cell / shifts remain; edges keep their center-sorted order.
        Returns (pos [N + G, 3], atom_types [N + G], edge_index int64 [2, E], ghost_source int64 [G]) -- forces on ghost
        row g belong to atom ghost_source[g] (what LAMMPS reverse-communicates).  One host read: the ghost count."""
        n = pos.shape[0]
        ei = self.edge_index.long()
        outside = (self.cell_shift != 0).any(dim=1)
        slot = torch.cumsum(outside.to(torch.int64), 0) - 1  # running ghost index of each outside-cell edge
        ghost_src = ei[1][outside]
        nbr = torch.where(outside, n + slot, ei[1])
        pos_ext = torch.cat((pos, pos.index_select(0, ghost_src) + self.shift_vec[outside].to(pos.dtype)), dim=0)
        types_ext = torch.cat((atom_types, atom_types.index_select(0, ghost_src)), dim=0)
        return pos_ext, types_ext, torch.stack((ei[0], nbr)), ghost_src


def neighbor_list(pos: torch.Tensor, cell, pbc, r_cut: float, lib: Optional[_lib.AllegroLib] = None, *,
                  atom_types: Optional[torch.Tensor] = None, cutoffs=None) -> DeviceNeighborList:
    """Cell-list neighbor list on the device the positions live on: every pair/image with |r| < r_cut, edges sorted by
    center (`r_e = pos[nbr] - pos[center] + cell_shift @ cell`, the `with_edge_vectors_` convention).  Only the edge
    count crosses to the host (the outputs must be allocated).  `cell`: 3x3, lattice vectors as rows; `pbc`: 3 bools.
    With `atom_types` [N] (int32 / int64, on the device) and `cutoffs` [T, T] (row = center type, column = neighbour type;
    `model.cutoff_table()`) an edge is listed only if |r| < min(r_cut, cutoffs[type_center, type_neighbour]): the model's
    envelope zeroes the others anyway (`aa_nl_count_typed` / `aa_nl_fill_typed`)."""
    if (atom_types is None) != (cutoffs is None):
        raise ValueError("neighbor_list: atom_types and cutoffs go together (a typed list needs both; got only "
                         f"{'atom_types' if cutoffs is None else 'cutoffs'})")
    lib = lib if lib is not None else _lib.load()
    _require_gpu(lib, pos, "neighbor_list")
    assert pos.dtype in _TORCH2AA and pos.dim() == 2 and pos.shape[1] == 3
    pos = pos.detach().contiguous()
    N, dev = pos.shape[0], pos.device
    inp = _lib.NlInput()
    inp.num_atoms, inp.pos, inp.dtype, inp.r_cut = N, pos.data_ptr(), _TORCH2AA[pos.dtype], float(r_cut)
    cell_h = torch.as_tensor(cell, dtype=torch.float64).reshape(9).tolist()
    for q in range(9):
        inp.cell[q] = cell_h[q]
    if isinstance(pbc, bool):
        pbc = (pbc,) * 3
    for q in range(3):
        inp.pbc[q] = int(bool(pbc[q]))
    typed = atom_types is not None
    if typed:
        types, keep = _nl_types(atom_types, cutoffs, N, dev, "neighbor_list")
    nbytes = lib.lib.aa_nl_typed_workspace_bytes(N) if typed else lib.lib.aa_nl_workspace_bytes(N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
    n_edges = C.c_int64()
    stream = _stream_ptr(pos)
    if typed:
        lib.check(lib.lib.aa_nl_count_typed(C.byref(inp), C.byref(types), ws.data_ptr(), nbytes, rowptr.data_ptr(), C.byref(n_edges),
                                            stream), "aa_nl_count_typed")
    else:
        lib.check(lib.lib.aa_nl_count(C.byref(inp), ws.data_ptr(), nbytes, rowptr.data_ptr(), C.byref(n_edges), stream),
                  "aa_nl_count")
    E = int(n_edges.value)
    edge_index = torch.empty((2, E), dtype=torch.int32, device=dev)
    cell_shift = torch.empty((E, 3), dtype=torch.int32, device=dev)
    shift_vec = torch.empty((E, 3), dtype=pos.dtype, device=dev)
    if E > 0 and typed:
        lib.check(lib.lib.aa_nl_fill_typed(C.byref(inp), C.byref(types), ws.data_ptr(), nbytes, rowptr.data_ptr(),
                                           edge_index[0].data_ptr(), edge_index[1].data_ptr(), cell_shift.data_ptr(),
                                           shift_vec.data_ptr(), stream), "aa_nl_fill_typed")
    elif E > 0:
        lib.check(lib.lib.aa_nl_fill(C.byref(inp), ws.data_ptr(), nbytes, rowptr.data_ptr(), edge_index[0].data_ptr(),
                                     edge_index[1].data_ptr(), cell_shift.data_ptr(), shift_vec.data_ptr(), stream),
                  "aa_nl_fill")
    return DeviceNeighborList(edge_index, rowptr, cell_shift, shift_vec, lib)


class Frames:
    """`aa_frames`: a batch of frames concatenated in atom order.  `frame_atoms` [B+1]: frame b owns the atoms
    [frame_atoms[b], frame_atoms[b+1]); non-decreasing, within [0, N].  Holds the int32 offsets on their device and `num_frames`;
    a tensor that is already int32 is kept as it is and never read by the host (the kernels clamp what they are given)."""

    def __init__(self, frame_atoms, device=None):
        t = torch.as_tensor(frame_atoms)
        if t.dim() != 1 or t.numel() < 1 or t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"Frames: frame_atoms must be B + 1 int32 / int64 offsets, not {list(t.shape)} {t.dtype}")
        self.frame_atoms = t.detach().to(device=device if device is not None else t.device, dtype=torch.int32).contiguous()
        self.num_frames = int(t.numel()) - 1

    @classmethod
    def from_batch(cls, batch: torch.Tensor, num_frames: Optional[int] = None) -> "Frames":
        """From nequip's `batch` vector (the frame of every atom).  Checks once, on the host, that it is non-decreasing (frames
        contiguous in atom order) and raises ValueError otherwise; frames without atoms are legal."""
        b = batch.detach().reshape(-1).long()
        if b.numel() > 1 and bool((b[1:] < b[:-1]).any()):
            raise ValueError("Frames.from_batch: batch must be non-decreasing (frames contiguous in atom order)")
        have = int(b[-1]) + 1 if b.numel() else 0
        if b.numel() and int(b[0]) < 0:
            raise ValueError("Frames.from_batch: negative frame index")
        nf = have if num_frames is None else int(num_frames)
        if nf < have:
            raise ValueError(f"Frames.from_batch: batch names frame {have - 1}, num_frames is {nf}")
        counts = torch.bincount(b, minlength=nf)
        offsets = torch.zeros(nf + 1, dtype=torch.int64, device=b.device)
        offsets[1:] = torch.cumsum(counts, 0)
        return cls(offsets)

    def c_struct(self) -> _lib.Frames:
        return _lib.Frames(self.num_frames, self.frame_atoms.data_ptr())


def neighbor_list_frames(pos: torch.Tensor, cells: torch.Tensor, pbc, r_cut: float, frames: Frames,
                         lib: Optional[_lib.AllegroLib] = None) -> DeviceNeighborList:
    """The neighbour list of a batch of small frames in one pair of calls (`aa_nl_frames_count` / `aa_nl_frames_fill`): `pos` [N,3]
    holds the frames one after the other, `cells` [B,3,3] one cell per frame (lattice vectors as rows), `pbc` one setting for all.
    Same conventions and the same result type as `neighbor_list` -- global atom ids, `shift_vec` from each edge's own cell -- so
    `.prepare`, `.prune` and `.ghost_layout` apply.  Inside a centre's segment: image ascending, then neighbour id.  Only the edge
    count and the error flags cross to the host.  All pairs of a frame are tested: for frames of up to a few thousand atoms."""
    lib = lib if lib is not None else _lib.load()
    _require_gpu(lib, pos, "neighbor_list_frames")
    if pos.dtype not in _TORCH2AA or pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"neighbor_list_frames: pos must be [N, 3] float32 / float64, not {list(pos.shape)} {pos.dtype}")
    pos = pos.detach().contiguous()
    N, dev, B = pos.shape[0], pos.device, frames.num_frames
    cells_d = torch.as_tensor(cells).detach().to(device=dev, dtype=torch.float64).reshape(-1, 9).contiguous()
    if cells_d.shape[0] != B:
        raise ValueError(f"neighbor_list_frames: {B} frames, {cells_d.shape[0]} cells")
    if frames.frame_atoms.device != dev:
        raise ValueError(f"neighbor_list_frames: the frame offsets live on {frames.frame_atoms.device}, the positions on {dev}")
    inp = _lib.NlFramesInput()
    inp.num_atoms, inp.pos, inp.cells, inp.dtype, inp.r_cut = N, pos.data_ptr(), cells_d.data_ptr(), _TORCH2AA[pos.dtype], float(r_cut)
    if isinstance(pbc, bool):
        pbc = (pbc,) * 3
    for q in range(3):
        inp.pbc[q] = int(bool(pbc[q]))
    fs = frames.c_struct()
    nbytes = lib.lib.aa_nl_frames_workspace_bytes(N, B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
    n_edges = C.c_int64()
    stream = _stream_ptr(pos)
    with _device_ctx(dev):
        lib.check(lib.lib.aa_nl_frames_count(C.byref(inp), C.byref(fs), ws.data_ptr(), nbytes, rowptr.data_ptr(), C.byref(n_edges), stream),
                  "aa_nl_frames_count")
        E = int(n_edges.value)
        edge_index = torch.empty((2, E), dtype=torch.int32, device=dev)
        cell_shift = torch.empty((E, 3), dtype=torch.int32, device=dev)
        shift_vec = torch.empty((E, 3), dtype=pos.dtype, device=dev)
        if E > 0:
            lib.check(lib.lib.aa_nl_frames_fill(C.byref(inp), C.byref(fs), ws.data_ptr(), nbytes, rowptr.data_ptr(), edge_index[0].data_ptr(),
                                                edge_index[1].data_ptr(), cell_shift.data_ptr(), shift_vec.data_ptr(), stream),
                      "aa_nl_frames_fill")
    return DeviceNeighborList(edge_index, rowptr, cell_shift, shift_vec, lib)


ZBL_QQR2E = {"metal": 14.399645, "real": 332.06371}  # LAMMPS' qqr2e: eV Angstrom / kcal/mol Angstrom per squared elementary charge


def parse_pair_potential(pair_potential: dict, type_names: Sequence[str], poly_p: float) -> dict:
    """The `pair_potential` constructor argument (allegro_models.py:270-288) -> what `aa_model_plan_set_pair_zbl` takes:
    {"atomic_numbers": [Z per type], "qqr2e", "poly_p"}.  Only nequip's ZBL module (EXT) exists here."""
    from ._periodic import ATOMIC_NUMBERS

    cfg = dict(pair_potential)
    tgt = cfg.pop("_target_", None)
    if tgt != "nequip.nn.pair_potential.ZBL":
        raise NotImplementedError(f"pair_potential {tgt!r}: only nequip.nn.pair_potential.ZBL is implemented")
    units = cfg.pop("units", None)
    if units not in ZBL_QQR2E:
        raise ValueError(f"pair_potential units {units!r}: one of {sorted(ZBL_QQR2E)}")
    species = cfg.pop("chemical_species", None)
    if species is None or isinstance(species, str) or len(species) != len(type_names):
        raise ValueError(f"pair_potential chemical_species {species!r}: one chemical symbol per entry of type_names "
                         f"({len(type_names)}: {list(type_names)})")
    unknown = [s for s in species if s not in ATOMIC_NUMBERS]
    if unknown:
        raise ValueError(f"pair_potential chemical_species: {unknown} are not chemical symbols")
    cfg.pop("type_names", None)  # (nequip passes the model's own list along)
    if cfg:
        raise ValueError(f"pair_potential: unknown arguments {sorted(cfg)}")
    return dict(atomic_numbers=[float(ATOMIC_NUMBERS[s]) for s in species], qqr2e=ZBL_QQR2E[units], poly_p=float(poly_p))


class HipAllegroModel(torch.nn.Module):
    """Energy + forces of an Allegro model through the HIP hot path.

    Constructor arguments follow `allegro.model.AllegroModel` (allegro_models.py:112-147): both two-body embeddings
    (`allegro.nn.TwoBodyBesselScalarEmbed`, `allegro.nn.TwoBodySplineScalarEmbed`), the reference's nonlinearities (silu, mish,
    gelu, None) and, as `pair_potential`, nequip's ZBL core repulsion (`nequip.nn.pair_potential.ZBL`).
    """

    def __init__(self, *, type_names: Sequence[str], r_max: float, l_max: int, num_layers: int = 2,
                 num_scalar_features: int = 64, num_tensor_features: int = 16, parity: bool = True,
                 radial_chemical_embed: Optional[dict] = None, radial_chemical_embed_dim: Optional[int] = None,
                 per_edge_type_cutoff: Optional[dict] = None,
                 scalar_embed_mlp_hidden_layers_depth: int = 1, scalar_embed_mlp_hidden_layers_width: int = 64,
                 scalar_embed_mlp_nonlinearity: Optional[str] = "silu",
                 allegro_mlp_hidden_layers_depth: int = 1, allegro_mlp_hidden_layers_width: int = 64,
                 allegro_mlp_nonlinearity: Optional[str] = "silu", tp_path_channel_coupling: bool = True,
                 readout_mlp_hidden_layers_depth: int = 1, readout_mlp_hidden_layers_width: int = 32,
                 readout_mlp_nonlinearity: Optional[str] = "silu", avg_num_neighbors: Optional[float] = None,
                 weight_individual_irreps: bool = True, per_type_energy_scales=None, per_type_energy_shifts=None,
                 per_type_energy_scales_trainable: bool = False, per_type_energy_shifts_trainable: bool = False,
                 pair_potential=None, forward_normalize: bool = True, seed: Optional[int] = None,
                 model_dtype: str = "float32", compile_mode: Optional[str] = None,
                 bessel_convention: str = "auto"):
        super().__init__()
        assert avg_num_neighbors is not None, "`avg_num_neighbors` must be set for Allegro models"
        # which published form of nequip's BesselEdgeLengthEncoding (EXT) the state_dict follows: "npi" (roots n*pi,
        # sin(w x)/x), "sinc" (roots n, sinc(x w) w), or "auto" = told apart by the stored values -- which is only
        # possible for untrained roots (aa_model_config.bessel_convention)
        if bessel_convention not in _BESSEL_CONVENTIONS:
            raise ValueError(f"bessel_convention {bessel_convention!r}: one of {sorted(_BESSEL_CONVENTIONS)}")
        self.bessel_convention = bessel_convention
        self.nonlinearities = (scalar_embed_mlp_nonlinearity, allegro_mlp_nonlinearity, readout_mlp_nonlinearity)
        for nl in self.nonlinearities:
            if nl not in ACT_KINDS:
                raise NotImplementedError(f"nonlinearity {nl!r}: the reference offers silu, mish, gelu, None")
        self.weight_individual_irreps = bool(weight_individual_irreps)
        rce = dict(radial_chemical_embed or {})
        tgt = rce.pop("_target_", "allegro.nn.TwoBodyBesselScalarEmbed")
        self.embed_kind = {"TwoBodyBesselScalarEmbed": 0, "TwoBodySplineScalarEmbed": 1}.get(tgt.rsplit(".", 1)[-1])
        if self.embed_kind is None:
            raise NotImplementedError(f"radial_chemical_embed {tgt}: only allegro.nn.TwoBodyBesselScalarEmbed and "
                                      "allegro.nn.TwoBodySplineScalarEmbed exist in the reference (scalarembed.py)")
        if rce.get("bessel_trainable", False) and bessel_convention == "auto":
            raise NotImplementedError("trained Bessel roots cannot be told apart by their values: pass bessel_convention='sinc' "
                                      "or 'npi'")
        self.dtype = {"float32": torch.float32, "float64": torch.float64}[model_dtype]
        self.type_names = list(type_names)
        T = len(self.type_names)
        S, u, L = num_scalar_features, num_tensor_features, num_layers
        S0 = S if radial_chemical_embed_dim is None else radial_chemical_embed_dim
        # number of radial basis functions: Bessel roots (scalarembed.py:22) or splines (:108)
        B = int(rce.get("num_splines", 16)) if self.embed_kind == 1 else int(rce.get("num_bessels", 8))
        span = int(rce.get("spline_span", 12))
        assert self.embed_kind == 0 or 0 <= span <= B, "spline.py:32"
        self.hparams = dict(r_max=float(r_max), l_max=l_max, num_layers=L, num_scalar_features=S, num_tensor_features=u,
                            embed_dim=S0, num_bessels=B, poly_p=float(rce.get("polynomial_cutoff_p", 6)),
                            spline_span=span,
                            embed_depth=scalar_embed_mlp_hidden_layers_depth, embed_width=scalar_embed_mlp_hidden_layers_width,
                            latent_depth=allegro_mlp_hidden_layers_depth, latent_width=allegro_mlp_hidden_layers_width,
                            readout_depth=readout_mlp_hidden_layers_depth, readout_width=readout_mlp_hidden_layers_width,
                            coupling=bool(tp_path_channel_coupling), avg_num_neighbors=float(avg_num_neighbors),
                            forward_normalize=bool(forward_normalize), parity=bool(parity))
        # pair potential (allegro_models.py:270-288): added to the per-atom energies after the per-type scale / shift; its envelope is
        # the embedding's polynomial cutoff, p = 6 with the spline embedding, which has none (:272-280).  No parameters, no buffers.
        self.pair_zbl = None if pair_potential is None else parse_pair_potential(
            pair_potential, self.type_names, self.hparams["poly_p"] if self.embed_kind == 0 else 6.0)
        if seed is not None:
            torch.manual_seed(seed)
        dt = self.dtype
        self.func = _Node()
        rng_u = lambda *shape: torch.empty(*shape, dtype=dt).uniform_(-math.sqrt(3), math.sqrt(3))  # noqa: E731

        def add(key, tensor, kind):
            node, leaf = _ensure_path(self.func, key)
            if kind == "param":
                node.register_parameter(leaf, torch.nn.Parameter(tensor))
            else:
                node.register_buffer(leaf, tensor)

        # edge_norm (nequip EdgeLengthNormalizer): per-type-pair cutoffs
        rmax = torch.full((T, T), float(r_max), dtype=dt)
        if per_edge_type_cutoff is not None:
            for ci, cn in enumerate(self.type_names):
                if cn not in per_edge_type_cutoff:
                    continue
                v = per_edge_type_cutoff[cn]
                for ni, nn_ in enumerate(self.type_names):
                    if isinstance(v, dict):
                        if nn_ in v:
                            rmax[ci, ni] = float(v[nn_])
                    else:
                        rmax[ci, ni] = float(v)
        add("edge_norm.rmax_recip", 1.0 / rmax, "buffer")
        if self.embed_kind == 1:
            # PerClassSpline (spline.py:43-62) + the init of TwoBodySplineScalarEmbed (scalarembed.py:136-145)
            lower = torch.arange(-span, B - span, dtype=dt) / B
            add("radial_chemical_embed.spline.lower", lower, "buffer")
            add("radial_chemical_embed.spline.upper", lower + (span + 1) / B, "buffer")
            bound = math.sqrt(3 / span) if forward_normalize else math.sqrt(3 / S0)
            add("radial_chemical_embed.spline.class_embed.weight",
                torch.empty(T * T, S0 * B, dtype=dt).uniform_(-bound, bound), "param")
        else:
            # nequip's BesselEdgeLengthEncoding (EXT) holds its roots as a Parameter when `trainable`, as a buffer otherwise
            add("radial_chemical_embed.bessel_encode.bessel_weights",
                (torch.linspace(1.0, B, B, dtype=dt) * math.pi).unsqueeze(0), "param" if rce.get("bessel_trainable", False) else "buffer")
            add("radial_chemical_embed.type_embed.center_embed.weight", torch.randn(T, S0 // 2, dtype=dt), "param")
            add("radial_chemical_embed.type_embed.neighbor_embed.weight", torch.randn(T, S0 // 2, dtype=dt), "param")
            add("radial_chemical_embed.type_embed.basis_linear.mlp.0.weight", rng_u(B, S0), "param")

        def add_mlp(prefix, dims):
            for i, (a, b) in enumerate(zip(dims, dims[1:])):
                add(f"{prefix}.{i}.weight", rng_u(a, b), "param")

        R = l_max + 1
        W = R * u
        We = W if weight_individual_irreps else u  # env-weight columns of the Allegro layers (_channels.py:29-35)
        self._embed_dims = [S0] + [scalar_embed_mlp_hidden_layers_width] * scalar_embed_mlp_hidden_layers_depth + [S]
        add_mlp("scalar_embed_mlp.mlp.mlp", self._embed_dims)
        add_mlp("tensor_embed.env_embed_linear.mlp", [S, W])
        if not weight_individual_irreps:
            # the reference registers an empty, persistent `_rtoi` in this mode (_channels.py:29-31): keep the key
            add("allegro._env_weighter._rtoi", torch.empty(0, dtype=dt), "buffer")
        add_mlp("allegro.first_layer_env_embed_projection.mlp", [S, S + We])
        self.tps_irreps = allegro_layer_irreps(l_max, parity, L)
        env = o3.Irreps.spherical_harmonics(l_max, p=-1)
        self._tp_meta = []
        for l in range(L):
            lat_dims = [S * (l + 1) + u] + [allegro_mlp_hidden_layers_width] * allegro_mlp_hidden_layers_depth + \
                       [S + (We if l < L - 1 else 0)]
            add_mlp(f"allegro.latents.{l}.mlp", lat_dims)
        for l in range(L):
            w3j, instr, diag, dims = build_w3j(self.tps_irreps[l], env, self.tps_irreps[l + 1])
            P = len(instr)
            shape = ((u,) if tp_path_channel_coupling else tuple()) + ((P,) if P > 1 else tuple())
            add(f"allegro.tps.{l}.weights", rng_u(*shape) if len(shape) else rng_u(1).reshape(()), "param")
            add(f"allegro.tps.{l}.w3j", torch.tensor(w3j, dtype=dt), "buffer")
            self._tp_meta.append(dict(num_paths=P, diag=diag, dims=dims))
        ro_dims = [S * (L + 1)] + [readout_mlp_hidden_layers_width] * readout_mlp_hidden_layers_depth + [1]
        add_mlp("edge_readout.mlp.mlp", ro_dims)

        def per_type(v):
            if v is None:
                return None
            if isinstance(v, dict):
                v = [v[t] for t in self.type_names]
            t = torch.as_tensor(v, dtype=dt).reshape(-1)
            return t.expand(T).clone() if t.numel() == 1 else t

        sc, sh = per_type(per_type_energy_scales), per_type(per_type_energy_shifts)
        self.has_scales, self.has_shifts = sc is not None, sh is not None
        if sc is not None:
            add("per_type_energy_scale_shift.scales", sc, "param")
        if sh is not None:
            add("per_type_energy_scale_shift.shifts", sh, "param")
        # eval mode (the default state of a freshly built model here): the hand-written inference / force pipeline, no weight
        # gradients (like _flashallegro.py:660).  `.train()` switches every trainable parameter on and `forward` to the
        # differentiable evaluation of allegro_amd/training.py.
        self._frozen_keys = set()
        if self.has_scales and not per_type_energy_scales_trainable:
            self._frozen_keys.add("func.per_type_energy_scale_shift.scales")
        if self.has_shifts and not per_type_energy_shifts_trainable:
            self._frozen_keys.add("func.per_type_energy_scale_shift.shifts")
        self._trainer = None
        self.training = False
        for p in self.parameters():
            p.requires_grad_(False)
        self._bound_lib: Optional[_lib.AllegroLib] = None
        # plans own device-resident tables and the packed weights / workspace are device buffers: one set per device,
        # `_plan_handle` / `_blob` / `_workspace` always refer to the device of the current call (`_select_device`)
        self._per_device: Dict[int, dict] = {}
        self._plan_handle = None
        self._blocked = None  # (max_block_edges, with_forces) when the last step on the current device was a blocked one
        self._plan_keep = None
        self._blob: Optional[torch.Tensor] = None
        self._blob_key = None
        self._workspace: Optional[torch.Tensor] = None
        self._cur_dev = None
        self._graph_cache = None  # (key, keyed tensors kept alive, PreparedGraph structure) of forward()

    # -- training ---------------------------------------------------------------------------------
    def train(self, mode: bool = True):
        """Training mode: every parameter the reference trains requires grad (MLPs, type embeddings, tensor-product path
        weights; per-type scales / shifts only with `per_type_energy_*_trainable`, allegro_models.py:251-260) and `forward`
        returns energies, forces and stress attached to the autograd graph (allegro_amd/training.py).  `.eval()` returns to
        the inference pipeline; the packed device weights follow in-place optimizer updates (`_ensure_weights`)."""
        mode = bool(mode)
        was = self.training
        super().train(mode)
        if mode == was:
            return self  # (a repeated .train() / .eval(), as training loops issue every epoch, leaves the user's freezes alone)
        if mode:
            # the parameters that were trainable when training mode was last left (so a user's requires_grad_(False) on a
            # sub-module survives an eval() / train() round trip); the first time: everything the reference trains
            on = getattr(self, "_trainable_keys", None)
            for k, p in self.named_parameters():
                p.requires_grad_(k not in self._frozen_keys if on is None else k in on)
        else:
            self._trainable_keys = {k for k, p in self.named_parameters() if p.requires_grad}
            for p in self.parameters():
                p.requires_grad_(False)
        return self

    def _training_evaluator(self):
        if self._trainer is None:
            from .training import TrainingEvaluator

            self._trainer = TrainingEvaluator(self)
        return self._trainer

    def chunked_training_step(self, graph: "PreparedGraph", max_edges_per_chunk: int):
        """Training on boxes whose whole differentiable graph does not fit: `step(pos, loss_fn)` of the returned object
        accumulates the exact gradient of `loss_fn(forces, total_energy)` block of center atoms by block
        (allegro_amd/training.py: ChunkedTrainingStep; peak memory ~ the block, not the frame)."""
        from .training import ChunkedTrainingStep

        return ChunkedTrainingStep(self._training_evaluator(), graph, max_edges_per_chunk)

    # -- library / plan -------------------------------------------------------------------------
    def _get_lib(self) -> _lib.AllegroLib:
        return self._bound_lib if self._bound_lib is not None else _lib.load()

    def _bind_library(self, lib: _lib.AllegroLib):
        """(tests) bind an explicitly loaded library instead of the default gfx950 one."""
        self._drop_device_state()
        self._bound_lib = lib
        self._trainer = None

    def _drop_device_state(self):
        self._stash_device_state()
        for st in self._per_device.values():
            if st.get("plan") is not None:
                try:
                    self._get_lib().model_plan_destroy(st["plan"])
                except Exception:
                    pass
        self._per_device = {}
        self._plan_handle = self._plan_keep = self._blob = self._blob_key = self._workspace = self._cur_dev = self._blocked = None

    def _stash_device_state(self):
        if self._cur_dev is not None:
            self._per_device[self._cur_dev] = dict(plan=self._plan_handle, keep=self._plan_keep, blob=self._blob,
                                                   blob_key=self._blob_key, ws=self._workspace,
                                                   hip_graph=getattr(self, "_hip_graph", False), out=getattr(self, "_out", None),
                                                   blocked=self._blocked)

    def _select_device(self, device) -> None:
        """Switch the per-device state (plan, packed weights, workspace) to `device`."""
        device = torch.device(device)
        idx = device.index if device.type == "cuda" and device.index is not None else (
            torch.cuda.current_device() if device.type == "cuda" else -1)
        if idx == self._cur_dev:
            return
        self._stash_device_state()
        st = self._per_device.get(idx, {})
        self._plan_handle, self._plan_keep = st.get("plan"), st.get("keep")
        self._blob, self._blob_key, self._workspace = st.get("blob"), st.get("blob_key"), st.get("ws")
        self._hip_graph, self._out = st.get("hip_graph", False), st.get("out")
        self._blocked = st.get("blocked")  # (what the workspace of THIS device holds)
        self._cur_dev = idx

    def _sd(self) -> Dict[str, torch.Tensor]:
        return {k[len("func."):]: v for k, v in self.state_dict().items()}

    def _ensure_plan(self):
        if self._cur_dev is None:  # first use without tensors (export, enable_hip_graph): the current device
            self._select_device(torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available()
                                else torch.device("cpu"))
        if self._plan_handle is not None:
            return
        cfg, keep = self._build_config()
        self._plan_handle = self._get_lib().model_plan_create(cfg)
        self._plan_keep = (cfg, keep)
        if self.pair_zbl is not None:
            self.set_pair_zbl(self.pair_zbl)

    def set_pair_zbl(self, zbl: Optional[dict]) -> None:
        """`aa_model_plan_set_pair_zbl` on the plan of the current device: `zbl` as `parse_pair_potential` returns it, or None to
        remove the term from that plan (A/B, tests; the model's own setting is applied whenever a plan is created)."""
        lib = self._get_lib()
        self._ensure_plan()
        arg = None
        if zbl is not None:
            z = (C.c_double * len(zbl["atomic_numbers"]))(*zbl["atomic_numbers"])
            arg = C.byref(_lib.PairZbl(len(zbl["atomic_numbers"]), z, zbl["qqr2e"], zbl["poly_p"]))
        lib.check(lib.lib.aa_model_plan_set_pair_zbl(self._plan_handle, arg), "aa_model_plan_set_pair_zbl")

    def _build_config(self):
        """(`aa_model_config`, keep-alive list) of this model: hyper-parameters + the Clebsch-Gordan non-zeros of every layer.
        Pure host work (no library call)."""
        hp = self.hparams
        cfg = _lib.ModelConfig()
        cfg.dtype = _TORCH2AA[self.dtype]
        cfg.num_types = len(self.type_names)
        cfg.num_bessels, cfg.poly_p = hp["num_bessels"], hp["poly_p"]
        cfg.l_max, cfg.num_layers = hp["l_max"], hp["num_layers"]
        cfg.num_scalar, cfg.num_tensor, cfg.embed_dim = hp["num_scalar_features"], hp["num_tensor_features"], hp["embed_dim"]
        cfg.embed_mlp_depth, cfg.embed_mlp_width = hp["embed_depth"], hp["embed_width"]
        cfg.latent_mlp_depth, cfg.latent_mlp_width = hp["latent_depth"], hp["latent_width"]
        cfg.readout_mlp_depth, cfg.readout_mlp_width = hp["readout_depth"], hp["readout_width"]
        cfg.forward_weight_init = int(hp["forward_normalize"])
        cfg.avg_num_neighbors = hp["avg_num_neighbors"]
        cfg.act_const = silu_second_moment_const()
        cfg.env_shared_weights = int(not self.weight_individual_irreps)
        for i, nl in enumerate(self.nonlinearities):
            cfg.act_kind[i] = ACT_KINDS[nl]
            cfg.act_consts[i] = second_moment_const(nl)
        cfg.has_scales, cfg.has_shifts = int(self.has_scales), int(self.has_shifts)
        cfg.embed_kind, cfg.spline_span = self.embed_kind, hp["spline_span"]
        cfg.bessel_convention = _BESSEL_CONVENTIONS[self.bessel_convention]
        keep = []
        sd = self._sd()
        for l in range(hp["num_layers"]):
            m = self._tp_meta[l]
            desc, k = w3j_to_desc(sd[f"allegro.tps.{l}.w3j"], hp["num_tensor_features"], m["dims"], m["num_paths"],
                                  m["diag"], hp["coupling"])
            cfg.tps[l] = desc
            keep.append(k)
        return cfg, keep

    def _ensure_weights(self, device):
        key = (str(device), tuple(int(p._version) for p in self.parameters()), tuple(p.data_ptr() for p in self.parameters()))
        if self._blob is not None and self._blob_key == key:
            return
        self._blob, self._blob_key = self._pack_blob(self._plan_handle, device), key

    def _raw_tensors(self, sd=None):
        """[(slot, float64 tensor)]: the parameters aa_model_pack_weights consumes, in the reference's own state_dict layout; slot =
        position of the pointer in `aa_model_raw_weights` (include/allegro_amd.h) -- also the tensor ids of a host model file
        (allegro_amd.export.write_host_model, csrc/aa_hostfile.hip)."""
        hp = self.hparams
        if sd is None:
            sd = {k: v.detach().to("cpu", torch.float64).contiguous() for k, v in self._sd().items()}
        ML, LL = _lib.AA_MAX_MLP_LAYERS, _lib.AA_MAX_LAYERS
        T = len(self.type_names)
        rr = sd["edge_norm.rmax_recip"]
        out = [(0, rr.expand(T, T).contiguous() if rr.numel() == 1 else rr)]
        if self.embed_kind == 1:
            out.append((7 + 2 * ML + LL * ML + LL + 2, sd["radial_chemical_embed.spline.class_embed.weight"]))
        else:
            out += [(1, sd["radial_chemical_embed.bessel_encode.bessel_weights"]),
                    (2, sd["radial_chemical_embed.type_embed.center_embed.weight"]),
                    (3, sd["radial_chemical_embed.type_embed.neighbor_embed.weight"]),
                    (4, sd["radial_chemical_embed.type_embed.basis_linear.mlp.0.weight"])]
        out += [(5 + i, sd[f"scalar_embed_mlp.mlp.mlp.{i}.weight"]) for i in range(hp["embed_depth"] + 1)]
        out += [(5 + ML, sd["tensor_embed.env_embed_linear.mlp.0.weight"]),
                (6 + ML, sd["allegro.first_layer_env_embed_projection.mlp.0.weight"])]
        for l in range(hp["num_layers"]):
            out += [(7 + ML + l * ML + i, sd[f"allegro.latents.{l}.mlp.{i}.weight"]) for i in range(hp["latent_depth"] + 1)]
            out.append((7 + ML + LL * ML + l, sd[f"allegro.tps.{l}.weights"]))
        out += [(7 + ML + LL * ML + LL + i, sd[f"edge_readout.mlp.mlp.{i}.weight"]) for i in range(hp["readout_depth"] + 1)]
        if self.has_scales:
            out.append((7 + 2 * ML + LL * ML + LL, sd["per_type_energy_scale_shift.scales"]))
        if self.has_shifts:
            out.append((7 + 2 * ML + LL * ML + LL + 1, sd["per_type_energy_scale_shift.shifts"]))
        return sorted(out, key=lambda kv: kv[0])

    def _pack_blob(self, plan_handle, device) -> torch.Tensor:
        """The model's state_dict packed for `plan_handle` (aa_model_pack_weights): the blob's layout belongs to that plan
        (aa_model_plan_layout_hash)."""
        lib = self._get_lib()
        hp = self.hparams
        sd = {k: v.detach().to("cpu", torch.float64).contiguous() for k, v in self._sd().items()}
        keep = []

        def ptr(t):
            a = np.ascontiguousarray(t.numpy().reshape(-1))
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_double))

        raw = _lib.RawWeights()
        ML, LL = _lib.AA_MAX_MLP_LAYERS, _lib.AA_MAX_LAYERS
        for slot, t in self._raw_tensors(sd):
            p = ptr(t)
            if slot < 5:
                setattr(raw, ("rmax_recip", "bessel_weights", "center_embed", "neighbor_embed", "basis_linear")[slot], p)
            elif slot < 5 + ML:
                raw.embed_mlp[slot - 5] = p
            elif slot < 7 + ML:
                setattr(raw, ("env_embed_linear", "first_proj")[slot - 5 - ML], p)
            elif slot < 7 + ML + LL * ML:
                raw.latent[(slot - 7 - ML) // ML][(slot - 7 - ML) % ML] = p
            elif slot < 7 + ML + LL * ML + LL:
                raw.tp_weights[slot - 7 - ML - LL * ML] = p
            elif slot < 7 + 2 * ML + LL * ML + LL:
                raw.readout[slot - 7 - ML - LL * ML - LL] = p
            else:
                setattr(raw, ("scales", "shifts", "spline_weights")[slot - 7 - 2 * ML - LL * ML - LL], p)
        nbytes = lib.lib.aa_model_weights_bytes(plan_handle)
        blob = torch.empty(nbytes, dtype=torch.uint8, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
        lib.check(lib.lib.aa_model_pack_weights(plan_handle, C.byref(raw), blob.data_ptr(), nbytes, stream),
                  "aa_model_pack_weights")
        return blob

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        # the pair potential holds no state here; a checkpoint that carries entries of such a module is accepted, and its atomic
        # numbers, where present, must be the configured species
        pair = {k: v for k, v in state_dict.items() if k.startswith(("pair_potential.", "func.pair_potential."))}
        if pair:
            state_dict = {k: v for k, v in state_dict.items() if k not in pair}
            for k, v in pair.items():
                if k.endswith("pair_potential.atomic_numbers"):
                    have = None if self.pair_zbl is None else [int(z) for z in self.pair_zbl["atomic_numbers"]]
                    if have != [int(z) for z in torch.as_tensor(v).reshape(-1).tolist()]:
                        raise ValueError(f"{k} = {torch.as_tensor(v).reshape(-1).tolist()} in the state_dict, but the model's "
                                         f"pair_potential is configured for atomic numbers {have}")
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        # w3j buffers may have changed: rebuild device tables lazily
        self._drop_device_state()
        self._trainer = None
        return out

    # -- evaluation -----------------------------------------------------------------------------
    def cutoff_table(self) -> torch.Tensor:
        """The per-type-pair cutoffs the model applies, [T, T] float64 on the host (row = center type, column = neighbour type):
        1 / `edge_norm.rmax_recip`, so it follows a loaded state_dict.  What `neighbor_list(..., cutoffs=)` and
        `DeviceNeighborList.prune` take."""
        return 1.0 / self.func.edge_norm.rmax_recip.detach().to(device="cpu", dtype=torch.float64)

    def neighbor_list(self, pos: torch.Tensor, cell, pbc, atom_types: torch.Tensor) -> DeviceNeighborList:
        """The device neighbour list of this model: `neighbor_list` at `r_max` with the model's own `cutoff_table()`, i.e. without
        the edges the envelope turns into exact zeros."""
        return neighbor_list(pos, cell, pbc, self.hparams["r_max"], lib=self._bound_lib, atom_types=atom_types,
                             cutoffs=self.cutoff_table())

    def prepare_graph(self, edge_index, atom_types, num_atoms, shift_vec=None, pos=None, prune=False) -> PreparedGraph:
        """`PreparedGraph(...)` of a foreign list.  With `pos` (or `prune`, which needs it) the list goes through
        `PreparedGraph.from_edge_index` instead -- one library operation, one host read -- and with `prune` it is reduced to the
        model's own `cutoff_table()` on the way: the edges the envelope turns into exact zeros are never evaluated."""
        if pos is None and not prune:
            return PreparedGraph(edge_index, atom_types, num_atoms, shift_vec, lib=self._bound_lib)
        if pos is None:
            raise ValueError("prepare_graph: prune=True needs pos")
        return PreparedGraph.from_edge_index(edge_index, atom_types, num_atoms, shift_vec, pos=pos,
                                             cutoffs=self.cutoff_table() if prune else None, lib=self._bound_lib)

    def energy_forces(self, pos: torch.Tensor, graph: PreparedGraph, with_forces: bool = True, max_block_edges: Optional[int] = None):
        """One pass of the hot path: returns (atom_energy [N], forces [N,3] | None).
        `max_block_edges`: evaluate the frame block by block (`graph.blocks(max_block_edges)`, `energy_forces_blocks`) in a workspace
        sized for the largest block instead of the frame -- same results, for frames whose per-edge workspace does not fit the device."""
        if max_block_edges is not None:
            block_atoms, block_edges = graph.blocks(max_block_edges)
            return self.energy_forces_blocks(pos, graph, block_atoms, block_edges, with_forces)
        lib = self._get_lib()
        _require_gpu(lib, pos, "HipAllegroModel")
        assert pos.dtype == self.dtype, f"positions must be {self.dtype}"
        with _device_ctx(pos.device):
            return self._energy_forces_on_device(lib, pos, graph, with_forces)

    def energy_forces_blocks(self, pos: torch.Tensor, graph: PreparedGraph, block_atoms, block_edges, with_forces: bool = True):
        """The block-wise step on explicit cuts (`aa_model_energy_forces_blocked`): block b owns the center atoms
        [block_atoms[b], block_atoms[b+1]) and the edges [block_edges[b], block_edges[b+1]) of `graph`, the whole frame.  Forces are
        assembled once over the frame through the graph's transposed CSR (bit-reproducible).  `virial`, `atom_virial` and
        `heat_flux_potential` then read what this call left behind.  Not available with `enable_hip_graph` / `enable_debug_taps`."""
        import numpy as np

        lib = self._get_lib()
        _require_gpu(lib, pos, "HipAllegroModel")
        assert pos.dtype == self.dtype, f"positions must be {self.dtype}"
        block_atoms = np.ascontiguousarray(block_atoms, dtype=np.int64)
        block_edges = np.ascontiguousarray(block_edges, dtype=np.int64)
        if block_atoms.ndim != 1 or block_atoms.shape != block_edges.shape or block_atoms.shape[0] < 2:
            raise ValueError("block_atoms and block_edges must be two [B+1] arrays, B >= 1")
        cap = int(max(0, min(graph.num_edges, np.diff(block_edges).max())))
        i64p = C.POINTER(C.c_int64)
        with _device_ctx(pos.device):
            self._select_device(pos.device)
            self._ensure_plan()
            self._ensure_weights(pos.device)
            N, E = graph.num_atoms, graph.num_edges
            self._ensure_workspace(lib.lib.aa_model_blocked_workspace_bytes(self._plan_handle, N, E, cap, int(with_forces)), pos.device)
            pos = pos.detach().contiguous()
            e_atom = torch.empty(N, dtype=self.dtype, device=pos.device)
            forces = torch.empty((N, 3), dtype=self.dtype, device=pos.device) if with_forces else None
            g = graph.c_struct()
            self._blocked = None
            lib.check(lib.lib.aa_model_energy_forces_blocked(self._plan_handle, self._blob.data_ptr(), C.byref(g), pos.data_ptr(),
                                                             block_atoms.shape[0] - 1, block_atoms.ctypes.data_as(i64p),
                                                             block_edges.ctypes.data_as(i64p), self._workspace.data_ptr(),
                                                             self._workspace.numel(), e_atom.data_ptr(),
                                                             forces.data_ptr() if with_forces else None, _stream_ptr(pos)),
                      "aa_model_energy_forces_blocked")
            self._blocked = (cap, bool(with_forces))  # (virial / atom_virial follow the kind of step that ran last)
        return e_atom, forces

    def max_block_edges_for(self, graph: PreparedGraph, budget_bytes: int, with_forces: bool = True) -> int:
        """The largest `max_block_edges` whose blocked workspace (`aa_model_blocked_workspace_bytes`) fits `budget_bytes` for `graph`;
        raises when even blocks of one atom (a cap of the graph's largest degree) do not."""
        lib = self._get_lib()
        self._ensure_plan()
        N, E = graph.num_atoms, graph.num_edges
        size = lambda cap: lib.lib.aa_model_blocked_workspace_bytes(self._plan_handle, N, E, cap, int(with_forces))  # noqa: E731
        lo = min(E, int(_max_degree(graph)))
        if size(lo) > budget_bytes:
            raise ValueError(f"a blocked workspace for one-atom blocks ({lo} edges) takes {size(lo)} bytes, more than the budget of {int(budget_bytes)}")
        hi = E
        while lo < hi:  # (the size function is monotone in the cap: bisection for the last cap that fits)
            mid = (lo + hi + 1) // 2
            if size(mid) <= budget_bytes:
                lo = mid
            else:
                hi = mid - 1
        return lo

    def _ensure_workspace(self, need: int, device) -> None:
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
            # The arena is the caller's (C ABI): this host grows it with 6 % of headroom and drops the old one FIRST.  In an MD loop
            # the edge count creeps up and down with every neighbour list; an arena sized exactly for the largest list so far is
            # re-allocated at every new maximum, and a fresh 30-GB device allocation costs ~0.5 s on this stack (two such steps in
            # the first 25 fs of the C4 run of tools/md_loop.py: profiles/r05_v22_md_loop_c4.json) while old + new briefly coexist.
            self._workspace = None
            self._workspace = torch.empty(need + need // 16 + (1 << 20), dtype=torch.uint8, device=device)

    def _energy_forces_on_device(self, lib, pos, graph, with_forces):
        self._select_device(pos.device)
        self._blocked = None  # (virial / atom_virial follow the kind of step that ran last)
        self._ensure_plan()
        self._ensure_weights(pos.device)
        N, E = graph.num_atoms, graph.num_edges
        self._ensure_workspace(lib.lib.aa_model_workspace_bytes(self._plan_handle, N, E, int(with_forces)), pos.device)
        pos = pos.detach().contiguous()
        if getattr(self, "_hip_graph", False):
            # replay mode: outputs live in persistent buffers so that every argument of the step keeps its address
            # (the caller updates `pos` in place and reads the results before the next call)
            if getattr(self, "_out", None) is None or self._out[0].shape[0] != N or self._out[0].device != pos.device:
                self._out = (torch.empty(N, dtype=self.dtype, device=pos.device),
                             torch.empty((N, 3), dtype=self.dtype, device=pos.device))
            e_atom, forces = self._out[0], (self._out[1] if with_forces else None)
        else:
            e_atom = torch.empty(N, dtype=self.dtype, device=pos.device)
            forces = torch.empty((N, 3), dtype=self.dtype, device=pos.device) if with_forces else None
        g = graph.c_struct()
        lib.check(lib.lib.aa_model_energy_forces(self._plan_handle, self._blob.data_ptr(), C.byref(g), pos.data_ptr(),
                                                 self._workspace.data_ptr(), self._workspace.numel(), e_atom.data_ptr(),
                                                 forces.data_ptr() if with_forces else None, _stream_ptr(pos)),
                  "aa_model_energy_forces")
        return e_atom, forces

    def describe_plan(self) -> dict:
        """`aa_model_plan_describe`: which forward / folds the plan of the current device runs (benchmark lines, bug reports)."""
        import json

        lib = self._get_lib()
        self._ensure_plan()
        buf = C.create_string_buffer(1024)
        lib.check(min(0, lib.lib.aa_model_plan_describe(self._plan_handle, buf, 1024)), "aa_model_plan_describe")
        return json.loads(buf.value.decode())

    def check(self, device=None) -> None:
        """`aa_model_check`: waits for the steps enqueued so far and raises if one of them contradicted the hints of its graph
        (a `max_degree` smaller than a real segment, edges outside the atom block).  `PreparedGraph` derives both hints from
        the row pointers, so this can only fire for hand-made graphs -- the raw C ABI has the same guard."""
        lib = self._get_lib()
        if getattr(self, "_plan_handle", None) is None:
            return
        dev = device if device is not None else (self._workspace.device if self._workspace is not None else None)
        stream = torch.cuda.current_stream(dev).cuda_stream if dev is not None and dev.type == "cuda" else None
        lib.check(lib.lib.aa_model_check(self._plan_handle, stream), "aa_model_check")

    def _after_step(self, what: str):
        """(lib, cap) for an observable that reads what the last force step left in the workspace of the current device;
        cap: `max_block_edges` of that step when it was a blocked one, None after an unblocked step."""
        lib = self._get_lib()
        if getattr(self, "_plan_handle", None) is None or self._workspace is None:
            raise RuntimeError(f"{what} reads what a step with forces left behind: call energy_forces first")
        if self._blocked is None:
            return lib, None
        cap, with_forces = self._blocked
        if not with_forces:
            raise RuntimeError(f"{what} reads what a step with forces left behind, and the last step was a blocked energy-only one "
                               "(it keeps no frame-wide edge arrays): call energy_forces with forces first")
        return lib, cap

    def _observable(self, step, name: str, graph: PreparedGraph, out: torch.Tensor, *args, frames: Optional[Frames] = None) -> torch.Tensor:
        """`aa_model_<name>` into `out`, or `aa_model_blocked_<name>` (the cap behind the graph) when the last step was a blocked one;
        `step`: what `_after_step` returned.  `frames`: the descriptor of a per-frame sum, which goes in front of the workspace."""
        lib, cap = step
        fn = f"aa_model_{name}" if cap is None else f"aa_model_blocked_{name}"
        g = graph.c_struct()
        head = () if cap is None else (cap,)
        if frames is not None:
            fs = frames.c_struct()
            head += (C.byref(fs),)
        with _device_ctx(out.device):
            lib.check(getattr(lib.lib, fn)(self._plan_handle, C.byref(g), *head, self._workspace.data_ptr(),
                                           self._workspace.numel(), *args, out.data_ptr(), _stream_ptr(out)), fn)
        return out

    def _frames_on(self, frames: Frames, device, what: str) -> Frames:
        if not isinstance(frames, Frames):
            raise ValueError(f"{what}: frames must be a Frames (Frames(frame_atoms) or Frames.from_batch(batch))")
        if frames.frame_atoms.device != device:
            raise ValueError(f"{what}: the frame offsets live on {frames.frame_atoms.device}, the step ran on {device}")
        return frames

    def frame_energies(self, e_atom: torch.Tensor, frames: Frames) -> torch.Tensor:
        """Per-frame energies [B] of a batch: the sum of `e_atom` [N] over each frame's atoms (`aa_model_frame_energies`), in double in
        a fixed order, rounded once.  A frame's bits depend on its own atoms only; an empty frame gives +0."""
        lib, _ = self._after_step("frame_energies")
        e = e_atom.detach().reshape(-1)
        if e.dtype != self.dtype:
            raise ValueError(f"frame_energies: e_atom must be {self.dtype}, not {e.dtype}")
        e = e.contiguous()
        frames = self._frames_on(frames, e.device, "frame_energies")
        out = torch.empty(frames.num_frames, dtype=self.dtype, device=e.device)
        fs = frames.c_struct()
        with _device_ctx(e.device):
            lib.check(lib.lib.aa_model_frame_energies(self._plan_handle, C.byref(fs), e.numel(), e.data_ptr(), out.data_ptr(), _stream_ptr(e)),
                      "aa_model_frame_energies")
        return out

    def frame_virial(self, graph: PreparedGraph, frames: Frames) -> torch.Tensor:
        """`virial` frame by frame [B,3,3] for a batch stepped as one graph (`aa_model_frame_virial`): dE/d(strain) restricted to each
        frame's edges, same convention; the rows sum to `virial(graph)`.  One workgroup per frame, no atomics: bit-reproducible, and
        a frame's bits do not depend on the other frames.  A lone large frame belongs on `virial`."""
        step = self._after_step("frame_virial")
        frames = self._frames_on(frames, self._workspace.device, "frame_virial")
        out = torch.empty((frames.num_frames, 3, 3), dtype=self.dtype, device=self._workspace.device)
        return self._observable(step, "frame_virial", graph, out, frames=frames)

    def frame_heat_flux_potential(self, graph: PreparedGraph, frames: Frames, velocities: torch.Tensor) -> torch.Tensor:
        """`heat_flux_potential` frame by frame [B,3] (`aa_model_frame_heat_flux`); `velocities` [N,3] of the whole batch."""
        if tuple(velocities.shape) != (graph.num_atoms, 3):
            raise ValueError(f"velocities must be [{graph.num_atoms}, 3], not {list(velocities.shape)}")
        step = self._after_step("frame_heat_flux_potential")
        frames = self._frames_on(frames, self._workspace.device, "frame_heat_flux_potential")
        vel = velocities.detach().to(device=self._workspace.device, dtype=self.dtype).contiguous()
        out = torch.empty((frames.num_frames, 3), dtype=self.dtype, device=self._workspace.device)
        return self._observable(step, "frame_heat_flux", graph, out, vel.data_ptr(), frames=frames)

    def virial(self, graph: PreparedGraph) -> torch.Tensor:
        """dE/d(strain) [3,3] of the LAST `energy_forces(..., with_forces=True)` call on `graph` (stress = virial / volume,
        nequip ForceStressOutput; LAMMPS' virial is its negative)."""
        step = self._after_step("virial")
        out = torch.empty(9, dtype=self.dtype, device=self._workspace.device)
        return self._observable(step, "virial", graph, out).view(3, 3)

    _ATOM_VIRIAL = {"center": 0, "neighbor": 1, "split": 2}  # AA_ATOM_VIRIAL_*

    def atom_virial(self, graph: PreparedGraph, attribution: str = "center") -> torch.Tensor:
        """Per-atom dE/d(strain) [N,3,3] of the LAST `energy_forces(..., with_forces=True)` call on `graph`
        (`aa_model_atom_virial`), W_n[a][b] = sum_e (dE/dr_e)_a (r_e)_b over the edges attributed to atom n:
        "center": the edges of its own segment (= dE_n/d(strain)); "neighbor": the edges that point at it (the tensor of the
        heat flux, `heat_flux_potential`); "split": the mean of the two (a pair style's tally).  Not symmetric atom by atom; each
        sums over the atoms to `virial(graph)`.  Ghost rows carry their own neighbor share.  Bit-reproducible; "neighbor" and
        "split" need the graph's transposed CSR."""
        if attribution not in self._ATOM_VIRIAL:
            raise ValueError(f"attribution must be one of {sorted(self._ATOM_VIRIAL)}, not {attribution!r}")
        step = self._after_step("atom_virial")
        out = torch.empty((graph.num_atoms, 3, 3), dtype=self.dtype, device=self._workspace.device)
        return self._observable(step, "atom_virial", graph, out, self._ATOM_VIRIAL[attribution])

    def heat_flux_potential(self, graph: PreparedGraph, velocities: torch.Tensor) -> torch.Tensor:
        """Potential part of the Green-Kubo heat flux [3] of the last step with forces on `graph`:
        J_pot[b] = -sum_e (r_e)_b (dE/dr_e . v_j(e)) = -sum_n sum_a v_n[a] Wn_n[a][b], Wn = atom_virial(graph, "neighbor").
        `velocities`: [N,3] (ghost rows carry the velocity of their source atom).  The convective part sum_n E_n v_n is the caller's.
        One streaming reduction over the edges (`aa_model_heat_flux`): bit-reproducible, and the graph needs no transposed CSR."""
        if tuple(velocities.shape) != (graph.num_atoms, 3):
            raise ValueError(f"velocities must be [{graph.num_atoms}, 3], not {list(velocities.shape)}")
        step = self._after_step("heat_flux_potential")
        vel = velocities.detach().to(device=self._workspace.device, dtype=self.dtype).contiguous()
        out = torch.empty(3, dtype=self.dtype, device=self._workspace.device)
        return self._observable(step, "heat_flux", graph, out, vel.data_ptr())

    def enable_hip_graph(self, on: bool = True) -> None:
        """Capture the step's launch sequence into a hipGraph and replay it (aa_model_plan_enable_graph): for
        launch-bound small systems in MD loops.  `pos` must then be updated in place between calls."""
        lib = self._get_lib()
        self._ensure_plan()
        lib.check(lib.lib.aa_model_plan_enable_graph(self._plan_handle, int(on)), "aa_model_plan_enable_graph")
        self._hip_graph = bool(on)
        self._out = None

    def enable_debug_taps(self, on: bool = True) -> None:
        """Make the following steps materialise the per-edge intermediates `debug_tap` reads (staged pipeline instead
        of the fused kernels, which keep them on chip).  Parity tests only."""
        lib = self._get_lib()
        self._ensure_plan()
        lib.check(lib.lib.aa_model_plan_enable_taps(self._plan_handle, int(on)), "aa_model_plan_enable_taps")

    def debug_tap(self, name: str, graph: PreparedGraph, with_forces: bool = False) -> torch.Tensor:
        """Copy of a per-edge intermediate of the LAST step out of the workspace ("dvec" / "vec" need the layout of a
        step that computed forces: `with_forces=True`)."""
        lib = self._get_lib()
        ptr, ld = C.c_void_p(), C.c_int64()
        rc = lib.lib.aa_model_debug_tap(self._plan_handle, (name + ("+f" if with_forces else "")).encode(), graph.num_atoms,
                                        graph.num_edges, self._workspace.data_ptr(), C.byref(ptr), C.byref(ld))
        if rc < 0:
            lib.check(rc, "aa_model_debug_tap")
        off = (ptr.value - self._workspace.data_ptr()) // self._workspace.element_size()
        esz = 4 if self.dtype == torch.float32 else 8
        flat = self._workspace[off: off + graph.num_edges * ld.value * esz].view(self.dtype)
        return flat.view(graph.num_edges, ld.value).clone()

    def _graph_for(self, data: Dict[str, torch.Tensor]) -> PreparedGraph:
        """Center-sorted CSR view of `data`'s edge list.  The STRUCTURE (sort permutation, rowptr, transposed CSR,
        types) is cached, keyed on the identity + in-place version of `edge_index` and `atom_types`; the keyed
        tensors are kept alive by the cache entry so their addresses cannot be recycled.  Everything that depends
        on values that change while the edge list stays put -- the periodic shift vectors `edge_cell_shift @ cell`
        -- is recomputed on every call (NPT / strain scans change `cell` with a fixed edge list)."""
        pos, ei, at = data["pos"], data["edge_index"], data["atom_types"]
        key = (ei.data_ptr(), tuple(ei.shape), int(ei._version), at.data_ptr(), int(at._version), int(pos.shape[0]),
               str(ei.device))
        if self._graph_cache is None or self._graph_cache[0] != key:
            self._graph_cache = (key, (ei, at), PreparedGraph(ei, at, pos.shape[0], None))
        graph = self._graph_cache[2]
        shift_vec = None
        if "edge_cell_shift" in data and "cell" in data:
            ecs = data["edge_cell_shift"].to(self.dtype)
            cell = data["cell"].to(self.dtype).reshape(-1, 3, 3)
            if cell.shape[0] == 1:
                shift_vec = ecs @ cell[0]
            else:  # batched frames: the cell of each edge's frame (nequip with_edge_vectors_: cell[batch[center]])
                if "batch" not in data:
                    raise ValueError("a [B,3,3] cell needs the `batch` vector")
                shift_vec = torch.einsum("ei,eij->ej", ecs, cell[data["batch"][ei[0]]])
            if graph.perm is not None:
                shift_vec = shift_vec[graph.perm]
            shift_vec = shift_vec.contiguous()
        graph.shift_vec = shift_vec
        return graph

    def _frames_for(self, batch: torch.Tensor, num_frames: int) -> Optional[Frames]:
        """The `Frames` of a `batch` vector, cached like the graph (identity + in-place version of `batch`, kept alive by the entry);
        None for a batch that is not non-decreasing, which keeps the `index_add_` route."""
        key = (batch.data_ptr(), int(batch._version), int(batch.numel()), int(num_frames), str(batch.device))
        cached = getattr(self, "_frames_cache", None)
        if cached is None or cached[0] != key:
            try:
                frames = Frames.from_batch(batch, num_frames)
            except ValueError:
                frames = None
            self._frames_cache = cached = (key, batch, frames)
        return cached[2]

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """AtomicDataDict in, AtomicDataDict out (keys: pos, edge_index, atom_types [, cell, edge_cell_shift, batch])."""
        pos = data["pos"]
        graph = self._graph_for(data)
        if self.training and torch.is_grad_enabled():
            return self._training_evaluator().forward(data, graph)
        e_atom, forces = self.energy_forces(pos.to(self.dtype), graph, with_forces=True)
        out = dict(data)
        out["atomic_energy"] = e_atom.unsqueeze(-1)
        nf = 1
        frames = None
        if "batch" in data:
            nf = int(data["cell"].reshape(-1, 3, 3).shape[0]) if "cell" in data else int(data["batch"].max()) + 1
            frames = self._frames_for(data["batch"], nf)
        if frames is not None:  # frames contiguous in atom order: one fixed-order kernel per observable
            out["total_energy"] = self.frame_energies(e_atom, frames).unsqueeze(-1)
        elif "batch" in data:
            out["total_energy"] = torch.zeros(nf, 1, dtype=self.dtype, device=pos.device).index_add_(0, data["batch"], e_atom.unsqueeze(-1))
        else:
            out["total_energy"] = e_atom.sum().reshape(1, 1)
        out["forces"] = forces
        if "cell" in data:
            # nequip ForceStressOutput (EXT) conventions: stress = dE/d(strain) / volume, virial = -dE/d(strain)
            cell = data["cell"].to(self.dtype).reshape(-1, 3, 3)
            if nf == 1:
                w = self.virial(graph).unsqueeze(0)
            elif frames is not None:
                w = self.frame_virial(graph, frames)
            else:
                # per-frame strain derivative from the per-edge dE/dr_e and r_e the step left in the workspace
                d = self.debug_tap("dvec", graph, with_forces=True)[:, :3]
                v = self.debug_tap("vec", graph, with_forces=True)
                r = v[:, :3] * v[:, 3:4]
                frame = data["batch"][graph.center.long()]
                w = torch.zeros(nf, 3, 3, dtype=self.dtype, device=pos.device).index_add_(
                    0, frame, d.unsqueeze(2) * r.unsqueeze(1))
            vol = torch.linalg.det(cell).abs().reshape(-1, 1, 1)
            out["stress"] = w / vol
            out["virial"] = -w
        return out

    def __del__(self):
        try:
            self._drop_device_state()
        except Exception:
            pass
