"""Device-side engine: packed embedding sets in HBM and the scoring / ranking calls.

PyTorch-ROCm provides device memory and streams only; every computation is a
libcmve.so (hand-written HIP, gfx950) call.  There is no CPU fallback: without a
GPU every entry point raises.
"""
from __future__ import annotations

import atexit
import contextlib
import ctypes as C
import functools
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, Rows

_HANDLES: Dict[Tuple[int, int], int] = {}

# Set by an atexit hook: objects still alive when the interpreter exits (a batch table, a captured graph held by a
# module or a test's traceback) skip their HIP destroy calls in __del__ -- the HIP runtime may already be torn down
# then, and the process releases the device memory anyway.
_EXITING = False


def _mark_exiting():
    global _EXITING
    _EXITING = True


atexit.register(_mark_exiting)


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("cmve needs a ROCm GPU (MI355X / gfx950); no CPU fallback exists")


def default_device() -> torch.device:
    require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def handle(device: Optional[torch.device] = None) -> int:
    """cmve handle bound to the CURRENT torch stream of `device`."""
    device = device or default_device()
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return _handle_for(idx, torch.cuda.current_stream(idx).cuda_stream)


def stream_handle(device: torch.device, stream: "torch.cuda.Stream") -> int:
    """cmve handle bound to an explicit torch stream (no current-stream switch per call)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return _handle_for(idx, stream.cuda_stream)


def _handle_for(idx: int, stream: int) -> int:
    key = (idx, stream)
    h = _HANDLES.get(key)
    if h is None:
        out = C.c_void_p()
        check(lib.cmve_create(idx, C.c_void_p(stream), C.byref(out)), "cmve_create")
        h = out.value
        _HANDLES[key] = h
    return h


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return _lib.CMVE_F32
    if t.dtype == torch.float64:
        return _lib.CMVE_F64
    raise TypeError(f"cmve: unsupported dtype {t.dtype} (float32 / float64 only)")


def pack_size(n: int, d: int) -> Tuple[int, int]:
    n_pad, d_pad = C.c_int64(), C.c_int64()
    check(lib.cmve_pack_size(n, d, C.byref(n_pad), C.byref(d_pad)), "cmve_pack_size")
    return n_pad.value, d_pad.value


def to_device(x, device: Optional[torch.device] = None, dtype=None) -> torch.Tensor:
    """numpy / torch -> contiguous float32|float64 device tensor (dtype preserved unless given)."""
    device = device or default_device()
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    elif t.dtype in (torch.float16, torch.bfloat16):
        t = t.to(torch.float32)
    elif t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.to(device, non_blocking=True).contiguous()


class RowSet:
    """A packed, L2-normalised embedding set resident in HBM (``cmve_rows_t``).

    ``eps=0`` reproduces LINAS ``l2norm`` (no epsilon, ``LINAS-engine/evaluation.py:10-14``);
    ``eps=1e-12`` reproduces ``F.normalize`` (``MultiFusion/src/combiner.py:134``).
    The raw rows are kept: the exact fp64 fix-up reads them.
    """

    def __init__(self, x, eps: float = 0.0, with_lo: bool = True, device: Optional[torch.device] = None,
                 with_f16: bool = True, raw_rows: bool = False):
        device = device or default_device()
        raw = to_device(x, device)
        if raw.dim() != 2:
            raise ValueError(f"RowSet expects a 2-D [n, d] matrix, got shape {tuple(raw.shape)}")
        n, d = raw.shape
        if d == 0:
            raise ValueError("RowSet: zero-dimensional embeddings")
        n_pad, d_pad = pack_size(n, d)
        self.device = device
        self.raw = raw
        self.n, self.d, self.n_pad, self.d_pad = n, d, n_pad, d_pad
        self.raw_ld = _pw_ld(raw)  # not stride(0): a one-row tensor may carry any, 0 for a [None, :] view
        self.eps = float(eps)
        self.hi = torch.empty((n_pad, d_pad), dtype=torch.int16, device=device)
        self.lo = torch.empty((n_pad, d_pad), dtype=torch.int16, device=device) if with_lo else None
        self.inv_norm = torch.empty(n_pad, dtype=torch.float64, device=device)
        self.err_hi = torch.empty(n_pad, dtype=torch.float32, device=device)
        self.err_hilo = torch.empty(n_pad, dtype=torch.float32, device=device)
        self.h16 = torch.empty((n_pad, d_pad), dtype=torch.int16, device=device) if with_f16 else None
        self.err_h16 = torch.empty(n_pad, dtype=torch.float32, device=device) if with_f16 else None
        self.err_max = torch.empty(3, dtype=torch.float32, device=device)
        self.desc = Rows(n=n, d=d, n_pad=n_pad, d_pad=d_pad, hi=self.hi.data_ptr(),
                         lo=self.lo.data_ptr() if self.lo is not None else None,
                         raw=raw.data_ptr() if n else None, raw_dtype=_dtype_code(raw), flags=_lib.PACK_RAW if raw_rows else 0,
                         raw_ld=self.raw_ld, inv_norm=self.inv_norm.data_ptr(),
                         err_hi=self.err_hi.data_ptr(), err_hilo=self.err_hilo.data_ptr(),
                         err_max=self.err_max.data_ptr(), eps=self.eps,
                         h16=self.h16.data_ptr() if with_f16 else None,
                         err_h16=self.err_h16.data_ptr() if with_f16 else None)
        check(lib.cmve_pack_rows(handle(device), C.byref(self.desc)), "cmve_pack_rows")

    def repack(self, x):
        """Copy new rows of the SAME shape into the resident raw buffer and re-pack them in place
        (query batches re-scored against a resident gallery: no allocation per call)."""
        src = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        if tuple(src.shape) != tuple(self.raw.shape):
            raise ValueError(f"RowSet.repack: expected {tuple(self.raw.shape)}, got {tuple(src.shape)}")
        self.raw.copy_(src, non_blocking=True)
        check(lib.cmve_pack_rows(handle(self.device), C.byref(self.desc)), "cmve_pack_rows")
        return self

    @property
    def has_lo(self):
        return self.lo is not None

    @property
    def has_f16(self):
        return self.h16 is not None

    def normalized(self, dtype=torch.float64) -> torch.Tensor:
        """x / max(||x||, eps) on device (K1')."""
        out = torch.empty((self.n, self.d), dtype=dtype, device=self.device)
        if self.n:
            check(lib.cmve_l2norm_rows(handle(self.device), _ptr(self.raw), _dtype_code(self.raw), self.raw_ld,
                                       _ptr(out), _dtype_code(out), out.stride(0), self.n, self.d, self.eps),
                  "cmve_l2norm_rows")
        return out


class PackedOperand:
    """Split-bf16 planes of a raw GEMM operand [n, d] written by a fused kernel (cmve_pack_tblocks,
    cmve_layernorm_pack) instead of cmve_pack_rows: usable wherever cmve_linear takes a RowSet
    packed with raw_rows=True (no fp32 rows behind it, no score bound)."""

    def __init__(self, n: int, d: int, device: Optional[torch.device] = None, row_multiple: int = 1):
        device = device or default_device()
        n_pad, d_pad = pack_size(n, d)
        n_pad = -(-n_pad // row_multiple) * row_multiple
        self.device, self.n, self.d, self.n_pad, self.d_pad = device, n, d, n_pad, d_pad
        self.hi = torch.empty((n_pad, d_pad), dtype=torch.int16, device=device)
        self.lo = torch.empty((n_pad, d_pad), dtype=torch.int16, device=device)
        self.err_max = torch.empty(3, dtype=torch.float32, device=device)
        self.desc = Rows(n=n, d=d, n_pad=n_pad, d_pad=d_pad, hi=self.hi.data_ptr(), lo=self.lo.data_ptr(), raw=None,
                         raw_dtype=_lib.CMVE_F32, flags=_lib.PACK_RAW, raw_ld=d, err_max=self.err_max.data_ptr())

    has_lo = True
    has_f16 = False

    @classmethod
    def from_blocks_transposed(cls, x: torch.Tensor, block_rows: int, block_cols: int):
        """Operand rows (b, c) = column c of block b of x viewed as [nb][block_rows][block_cols]
        (fp32): each row has block_rows elements (cmve_pack_tblocks)."""
        x = x.detach().float().contiguous()
        nb = x.numel() // (block_rows * block_cols)
        op = cls(nb * block_cols, block_rows, x.device, row_multiple=block_cols)
        check(lib.cmve_pack_tblocks(handle(x.device), _ptr(x), nb, block_rows, block_cols, C.byref(op.desc)),
              "cmve_pack_tblocks")
        return op

    @classmethod
    def layernorm(cls, x: torch.Tensor, weight, bias, eps: float):
        """LayerNorm(x) rows (fp64 statistics, cmve_layernorm's arithmetic) as a packed operand."""
        x = x.detach().float().contiguous()
        n, d = x.shape
        op = cls(n, d, x.device)
        w = weight.detach().float().contiguous() if weight is not None else None
        b = bias.detach().float().contiguous() if bias is not None else None
        check(lib.cmve_layernorm_pack(handle(x.device), _ptr(x), x.stride(0), n, d, _ptr(w), _ptr(b), float(eps),
                                      C.byref(op.desc)), "cmve_layernorm_pack")
        return op


def transpose_blocks_kv(x: torch.Tensor, block_rows: int, block_cols: int, d: int, T: int, gs: int,
                        B: int) -> torch.Tensor:
    """transpose_blocks whose output rows of d floats (g, t, bb) of .reshape(B // gs, T, gs, d) are
    stored at row t*B + g*gs + bb (cmve_transpose_blocks_kv): [T * B, d]."""
    x = x.detach().float().contiguous()
    nb = x.numel() // (block_rows * block_cols)
    y = torch.empty((T * B, d), dtype=torch.float32, device=x.device)
    check(lib.cmve_transpose_blocks_kv(handle(x.device), _ptr(x), nb, block_rows, block_cols, d, T, gs, B, _ptr(y)),
          "cmve_transpose_blocks_kv")
    return y


def transpose_blocks(x: torch.Tensor, block_rows: int, block_cols: int) -> torch.Tensor:
    """y[(b, c), :] = column c of block b of x viewed as [nb][block_rows][block_cols] (fp32)."""
    x = x.detach().float().contiguous()
    nb = x.numel() // (block_rows * block_cols)
    y = torch.empty((nb * block_cols, block_rows), dtype=torch.float32, device=x.device)
    check(lib.cmve_transpose_blocks(handle(x.device), _ptr(x), nb, block_rows, block_cols, _ptr(y)),
          "cmve_transpose_blocks")
    return y


def _mode_for(q: RowSet, g: RowSet, mode: Optional[int]) -> int:
    if mode is None:
        mode = _lib.SIM_BF16X3 if (q.has_lo and g.has_lo) else _lib.SIM_BF16
    if mode == _lib.SIM_BF16X3 and not (q.has_lo and g.has_lo):
        raise ValueError("BF16X3 mode needs both sets packed with lo planes")
    return mode


def sim_store(q: RowSet, g: RowSet, alpha: float = 1.0, beta: float = 0.0, mode: Optional[int] = None,
              out_dtype=torch.float32) -> torch.Tensor:
    """out[i, j] = alpha * cos(q_i, g_j) + beta on device."""
    mode = _mode_for(q, g, mode)
    out = torch.empty((q.n, g.n), dtype=out_dtype, device=q.device)
    if q.n and g.n:
        check(lib.cmve_sim_store(handle(q.device), C.byref(q.desc), C.byref(g.desc), mode, alpha, beta, _ptr(out),
                                 _dtype_code(out), out.stride(0)), "cmve_sim_store")
    return out


def pairwise(a: torch.Tensor, b: torch.Tensor, metric: int, alpha: float = 1.0, beta: float = 0.0,
             out_dtype=torch.float64) -> torch.Tensor:
    """out[i, j] = alpha * f(a_i, b_j) + beta for a non-cosine metric (K10, fp64 accumulation)."""
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"pairwise: shapes {tuple(a.shape)} and {tuple(b.shape)} do not match")
    # row-strided views go in as they are (lda >= D); anything else is made contiguous
    a = a if a.stride(1) == 1 and a.stride(0) >= a.shape[1] else a.contiguous()
    b = b if b.stride(1) == 1 and b.stride(0) >= b.shape[1] else b.contiguous()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=out_dtype, device=a.device)
    if a.shape[0] and b.shape[0]:
        check(lib.cmve_pairwise(handle(a.device), _ptr(a), _dtype_code(a), a.stride(0), a.shape[0], _ptr(b),
                                _dtype_code(b), b.stride(0), b.shape[0], a.shape[1], metric, float(alpha),
                                float(beta), _ptr(out), _dtype_code(out), out.stride(0)), "cmve_pairwise")
    return out


def pairwise_bwd_workspace(na: int, nb: int, metric: int) -> int:
    """Bytes of workspace ``cmve_pairwise_bwd`` needs (host only: no launch, no GPU)."""
    n = C.c_int64()
    check(lib.cmve_pairwise_bwd_workspace(na, nb, metric, C.byref(n)), "cmve_pairwise_bwd_workspace")
    return n.value


def pairwise_bwd(a: torch.Tensor, b: torch.Tensor, metric: int, alpha: float, ds: torch.Tensor,
                 need_a: bool = True, need_b: bool = True):
    """(dA, dB) of ``sum(ds * pairwise(a, b, metric, alpha, beta))`` for fp32 rows (K17); a side that is not
    needed is None and is not computed."""
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or ds.shape != (a.shape[0], b.shape[0]):
        raise ValueError(f"pairwise_bwd: shapes {tuple(a.shape)}, {tuple(b.shape)}, {tuple(ds.shape)} do not match")
    if a.dtype != torch.float32 or b.dtype != torch.float32 or ds.dtype != torch.float32:
        raise TypeError("pairwise_bwd: float32 only")
    if not (a.is_cuda and b.is_cuda and ds.is_cuda):
        raise ValueError("pairwise_bwd: device tensors only")
    a = a if a.stride(1) == 1 and a.stride(0) >= a.shape[1] else a.contiguous()
    b = b if b.stride(1) == 1 and b.stride(0) >= b.shape[1] else b.contiguous()
    ds = ds if ds.stride(1) == 1 and ds.stride(0) >= ds.shape[1] else ds.contiguous()
    na, nb, d = a.shape[0], b.shape[0], a.shape[1]
    nbytes = pairwise_bwd_workspace(na, nb, metric)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=a.device)
    da = torch.empty((na, d), dtype=torch.float32, device=a.device) if need_a else None
    db = torch.empty((nb, d), dtype=torch.float32, device=a.device) if need_b else None
    check(lib.cmve_pairwise_bwd(handle(a.device), _ptr(a), a.stride(0), na, _ptr(b), b.stride(0), nb, d, metric,
                                float(alpha), _ptr(ds), max(ds.stride(0), nb), _ptr(da), d, _ptr(db), d, _ptr(ws),
                                nbytes), "cmve_pairwise_bwd")
    return da, db


def pairwise_positions_workspace(na: int, nb: int, row_items: int, col_items: int, metric: int) -> int:
    """Bytes of workspace ``cmve_pairwise_positions`` needs: the item scores (host only: no launch, no GPU)."""
    n = C.c_int64()
    check(lib.cmve_pairwise_positions_workspace(na, nb, row_items, col_items, metric, C.byref(n)),
          "cmve_pairwise_positions_workspace")
    return n.value


def pairwise_topk_workspace(n_q: int, n_g: int, k: int, metric: int) -> Tuple[int, int]:
    """(minimum, recommended) bytes of workspace for ``cmve_pairwise_topk`` (host only: no launch, no GPU)."""
    lo, rec = C.c_int64(), C.c_int64()
    check(lib.cmve_pairwise_topk_workspace(n_q, n_g, int(k), metric, C.byref(lo), C.byref(rec)),
          "cmve_pairwise_topk_workspace")
    return lo.value, rec.value


def _pw_rows(x, name: str) -> torch.Tensor:
    """A pairwise operand: f32 / f64 device rows, row-strided views as they are."""
    t = x if isinstance(x, torch.Tensor) else to_device(x)
    if t.dim() != 2:
        raise ValueError(f"{name}: a 2-d operand is needed, got shape {tuple(t.shape)}")
    if not t.is_cuda:
        t = to_device(t)
    _dtype_code(t)
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def _pw_ld(t: torch.Tensor) -> int:
    """Leading dimension of a [n, d] operand with contiguous rows (torch leaves the stride of a one-row tensor's row
    dimension arbitrary): RowSet's raw rows, RankSession's bound rows and the pairwise operands."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _pw_pair(a, b, name: str):
    a, b = _pw_rows(a, name), _pw_rows(b, name)
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"{name}: shapes {tuple(a.shape)} and {tuple(b.shape)} do not match")
    return a, b


def _pw_code(score_dtype) -> int:
    return _lib.CMVE_F64 if score_dtype == torch.float64 else _lib.CMVE_F32


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


# ---- the Euclidean filter (K19 / K20 / K21): the rules every entry composes, each in ONE place ----
def _l2_applies(metric: int, score_dtype) -> bool:
    """The filter speaks for ``PW_L2`` with float64 score words and for nothing else."""
    return metric == _lib.PW_L2 and score_dtype == torch.float64


def _l2_scaling_ok(alpha: float, beta: float) -> bool:
    """What the filter's C entries ask of the scaling: alpha finite and non-zero, beta finite."""
    return alpha != 0 and bool(np.isfinite(alpha)) and bool(np.isfinite(beta))


def _l2_set_ok(s) -> bool:
    """Plain rows (None: packed inside the call), or a ``RowSet`` the filter's C entries take."""
    return s is None or (s.eps == 0.0 and s.has_f16 and not s.desc.flags & _lib.PACK_RAW)


def _stats4(names, host) -> dict:
    """The int64 [4] counters of a filter entry, on the host, under their names."""
    return dict(zip(names, (int(v) for v in host)))


def _l2_count_stats(host) -> dict:
    """{decided, band, rescored, overflow} of ``cmve_l2_count`` / ``cmve_l2_count_resolved`` / ``cmve_l1_count``."""
    return _stats4(("decided", "band", "rescored", "overflow"), host)


def _count_tail(row, col, ws, ws_bytes: int, stats):
    """The last thirteen arguments of every filtered count entry.  row / col: (offsets, item scores, items, n,
    positions) of the direction; ws: the band list's tensor, ws_bytes of it handed over; stats: the int64 [4] words."""
    (roff, rsc, ritems, rn, rpos), (coff, csc, citems, cn, cpos) = row, col
    return (_ptr(roff), _ptr(rsc) if ritems else None, ritems, rn, _ptr(rpos),
            _ptr(coff), _ptr(csc) if citems else None, citems, cn, _ptr(cpos),
            _ptr(ws) if ws_bytes else None, ws_bytes, _ptr(stats))


def _l2_count_call(entry: str, h, a_set: "RowSet", b_set: "RowSet", alpha, beta, row, col, ws, ws_bytes: int, stats):
    """``cmve_l2_count`` or ``cmve_l2_count_resolved`` (``entry``: one argument list; the rest as ``_count_tail``)."""
    check(getattr(lib, entry)(h, C.byref(a_set.desc), C.byref(b_set.desc), float(alpha), float(beta),
                              *_count_tail(row, col, ws, ws_bytes, stats)), entry)


def _item_scores_into(out, a, b, metric, alpha, beta, score_dtype, off, idx, n_items, col_dir, idx_base):
    """``cmve_pairwise_item_scores`` of one CSR side into the caller's fp64 slice ``out``."""
    check(lib.cmve_pairwise_item_scores(handle(a.device), _ptr(a), _dtype_code(a), _pw_ld(a), a.shape[0], _ptr(b),
                                        _dtype_code(b), _pw_ld(b), b.shape[0], a.shape[1], metric, float(alpha),
                                        float(beta), _pw_code(score_dtype), _ptr(off), _ptr(idx), off.numel() - 1,
                                        int(n_items), 1 if col_dir else 0, int(idx_base), _ptr(out)),
          "cmve_pairwise_item_scores")


def l2_count_workspace(a: "RowSet", b: "RowSet", band_cap: int) -> int:
    """Bytes of workspace ``cmve_l2_count`` needs for a band list of ``band_cap`` pairs (host only: no launch)."""
    n = C.c_int64()
    check(lib.cmve_l2_count_workspace(C.byref(a.desc), C.byref(b.desc), int(band_cap), C.byref(n)),
          "cmve_l2_count_workspace")
    return n.value


# Auto dispatch of the K19 filter (``filter=None``): the smallest na * nb at which it beats the fp64 route by more
# than the spread of the repeats.  tools/l2_filter_bench.py measures both routes at na = nb in {256 .. 4096},
# D = 1024 (profiles/l2_filter.json, "crossover"): up to 2048 x 2048 a call is its host code and launch gaps either
# way (2.34 ms against 2.37 ms there, 0.17 ms of spread; below it the packs cost the filter 0.05-0.2 ms), at
# 4096 x 4096 the filter takes 3.53 ms against 4.64 ms with 0.04 ms of spread.
L2_FILTER_MIN_PAIRS = 4096 * 4096


# ---- the SAD filter of the L1 measures (K22): the rules every entry composes, each in ONE place ----
L1_D_MAX = 65536  # cmve_l1_count's limit on d: the u32 SAD of uint16 codes is exact up to there
# Auto dispatch of the K22 filter (``filter=None``): the smallest na * nb at which it beats the fp64 route by more
# than the two routes' combined spread (None would mean: never taken automatically, ``filter="l1"`` alone runs it).
# tools/l1_filter_bench.py measures both routes at na = nb in {256 .. 16384}, D = 1024 (profiles/l1_filter.json,
# "crossover"): up to 4096 x 4096 the filter's extra launches (grid, two packs, the gated pair) cost it 0.1-0.9 ms
# (4.86 ms against 4.75 ms at 4096 x 4096, inside the spread), at 8192 x 8192 it takes 8.18 ms against 11.72 ms with
# 0.70 ms of combined spread, at 16384 x 16384 17.1 ms against 33.8 ms.
L1_FILTER_MIN_PAIRS = 8192 * 8192


# ---- the SAD filter under jaccard (K24): the same codes, float32 words ----
# Auto dispatch of the K24 filter (``filter=None``): the smallest na * nb at which it beats the K18 route by more than
# the two routes' combined spread; None: never taken automatically, ``filter="jaccard"`` alone runs it.
# tools/jaccard_filter_bench.py measures both routes at na = nb in {256 .. 16384}, D = 1024, non-negative float32 rows
# (profiles/jaccard_filter.json, "crossover"; K18 / filter, one call each): up to 2048 x 2048 the filter's extra
# launches cost it 0.4-0.8 ms (2.67 ms against 3.44 ms at 2048 x 2048); at 4096 x 4096 it takes 4.86 ms against
# 6.15 ms, inside the K18 route's 1.86 ms of spread; at 8192 x 8192 8.25 ms against 17.36 ms with 0.86 ms of combined
# spread, at 16384 x 16384 17.0 ms against 55.2 ms.  (At 16,384 x 131,072: 48.7 ms against 389.1 ms.)
JACCARD_FILTER_MIN_PAIRS = 8192 * 8192


# ---- the cosine filter (K26): every listed item's position, both directions, from one MFMA pass ----
# Auto dispatch of the K26 route (``filter=None`` of cmve.linas: taken only where today's route would run a second or
# third rank pass, i.e. some list holds more than one item): the smallest n_c * n_v at which it beats today's passes
# by more than the two routes' combined spread; None: never taken automatically, ``filter="cosine"`` alone runs it.
# tools/cos_positions_bench.py measures cal_perf_embeddings on both routes at D = 1024 with 20 captions per video, host
# embeddings in, tuples out, 10 alternating repeats (profiles/cos_positions.json; today's passes / one pass, medians):
# 49.0 ms against 11.2 ms at 20,000 x 1,000 -- 4.4x on the medians, but single repeats of either route stray by
# 30-36 ms on the host (combined spread 69.8 ms), so it does not count as a win by the rule; 153.1 ms against 72.1 ms at
# 59,800 x 2,990 with 61.2 ms of combined spread; 1.113 s against 0.397 s at 327,680 x 16,384 with 0.296 s.  The count
# itself (MFMA pass and band re-score) takes 0.48 / 2.13 / 54.7 ms there, the item words 0.08 / 0.26 / 1.39 ms.
COS_FILTER_MIN_PAIRS = 59800 * 2990


def _filter_route(name: str, filter, metric: int, alpha: float, beta: float, score_dtype, l2_scaling: bool,
                  size=None) -> Optional[str]:
    """THE route of a count: None (the canonical chain), ``"l2"`` (the MFMA filter), ``"l1"`` (the SAD filter) or
    ``"jaccard"`` (the SAD filter under jaccard, float32 words), at two moments.
    size None -- before any operand is touched: a forced value (True, ``"l1"``, ``"jaccard"``) gives its route, or ValueError where
    that filter cannot speak for the call; ``filter=True`` judges alpha / beta here only with ``l2_scaling`` (else a
    bad scaling is the C entry's to refuse).  size = (na * nb, d, the sets are ones the Euclidean entries take) --
    the auto rule of ``filter=None``, which never hands an entry what it refuses."""
    scaling = _l2_scaling_ok(alpha, beta)
    if size is None:
        if isinstance(filter, str) and filter in _SAD_FILTERS:
            f = _SAD_FILTERS[filter]
            if not (f.applies(metric, score_dtype) and scaling):
                raise ValueError(f'{name}: filter="{filter}" needs {f.metric} with {f.words} score words, alpha finite '
                                 "and non-zero, beta finite")
            return filter
        if filter:
            if not (_l2_applies(metric, score_dtype) and (scaling or not l2_scaling)):
                raise ValueError(f"{name}: filter=True needs PW_L2 with float64 score words"
                                 + (", alpha finite and non-zero, beta finite" if l2_scaling else ""))
            return "l2"
        return None
    pairs, d, sets_ok = size
    if filter is not None or not scaling:
        return None
    for route, f in _SAD_FILTERS.items():
        if f.applies(metric, score_dtype):
            min_pairs = globals()[f.min_pairs]  # (read at call time; None: never automatically)
            return route if min_pairs is not None and pairs >= min_pairs and d <= L1_D_MAX else None
    return "l2" if _l2_applies(metric, score_dtype) and pairs >= L2_FILTER_MIN_PAIRS and sets_ok else None


def l1_pack_size(n: int, d: int) -> Tuple[int, int]:
    """(n_pad, d_pad) of a set's uint16 codes (``cmve_l1_pack_size``; host only: no launch)."""
    n_pad, d_pad = C.c_int64(), C.c_int64()
    check(lib.cmve_l1_pack_size(int(n), int(d), C.byref(n_pad), C.byref(d_pad)), "cmve_l1_pack_size")
    return n_pad.value, d_pad.value


def _sad_count_workspace(route: str, band_cap: int) -> int:
    """Bytes of workspace the route's count entry needs for a band list of ``band_cap`` pairs (host only: no launch)."""
    entry = _SAD_FILTERS[route].entry + "_workspace"
    n = C.c_int64()
    check(getattr(lib, entry)(int(band_cap), C.byref(n)), entry)
    return n.value


def l1_count_workspace(band_cap: int) -> int:
    """Bytes of workspace ``cmve_l1_count`` needs for a band list of ``band_cap`` pairs (host only: no launch)."""
    return _sad_count_workspace("l1", band_cap)


def jaccard_count_workspace(band_cap: int) -> int:
    """Bytes of workspace ``cmve_jaccard_count`` needs for a band list of ``band_cap`` pairs (host only: no launch)."""
    return _sad_count_workspace("jaccard", band_cap)


def l1_grid(x: torch.Tensor, grid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The device float64 [2] grid words {lo, hi} of the rows ``x`` (``cmve_l1_grid``); with ``grid`` the words
    already there are extended in place, so that two sets share one grid.  No host copy, no synchronisation."""
    accumulate = grid is not None
    if grid is None:
        grid = torch.empty(2, dtype=torch.float64, device=x.device)
    check(lib.cmve_l1_grid(handle(x.device), _ptr(x), _dtype_code(x), _pw_ld(x), x.shape[0], x.shape[1], _ptr(grid),
                           1 if accumulate else 0), "cmve_l1_grid")
    return grid


class L1Set:
    """Rows packed for the SAD filter of the L1 measures (K22): the raw rows (``.raw``, the fp64 route's operand and
    the source of every canonical score), their uint16 codes in ``cmve_l1_pack``'s tiled order, the rows' errors, the
    grid tensor and the pads.  A resident side is packed once: ``L1Set(gallery)`` derives the grid from its own
    rows, ``L1Set(x, grid=other.grid)`` packs a second set on an existing grid (elements outside it clamp: only the
    band grows)."""

    def __init__(self, x, grid: Optional[torch.Tensor] = None, device: Optional[torch.device] = None):
        raw = _pw_rows(x if isinstance(x, torch.Tensor) else to_device(x, device), "L1Set")
        n, d = raw.shape
        if d == 0 or d > L1_D_MAX:
            raise ValueError(f"L1Set: d must be in [1, {L1_D_MAX}], got {d}")
        if grid is not None and (grid.dtype != torch.float64 or grid.numel() != 2 or grid.device != raw.device):
            raise TypeError("L1Set: grid is a float64 [2] tensor on the rows' device")
        self.device, self.raw = raw.device, raw
        self.n, self.d = n, d
        self.n_pad, self.d_pad = l1_pack_size(n, d)
        self.grid = l1_grid(raw) if grid is None else grid
        self.codes = torch.empty(max(self.n_pad * self.d_pad, 8), dtype=torch.int16, device=raw.device)
        self.err = torch.empty(max(n, 1), dtype=torch.float64, device=raw.device)
        check(lib.cmve_l1_pack(handle(raw.device), _ptr(raw), _dtype_code(raw), _pw_ld(raw), n, d, _ptr(self.grid),
                               _ptr(self.codes), self.n_pad, self.d_pad, _ptr(self.err)), "cmve_l1_pack")


class JaccardSet(L1Set):
    """Rows packed for the SAD filter under jaccard (K24): an ``L1Set`` -- the same codes, errors and grid, from the
    same ``cmve_l1_pack`` -- plus the two per-row arrays of ``cmve_jaccard_rowsums``: ``qsum`` (int64, the exact sum of
    the row's codes) and ``asum`` (float64, >= sum |x|; +inf where ``err`` is).  ``JaccardSet(x, grid=other.grid)``
    works as ``L1Set`` does; a resident gallery is packed once.  It serves ``filter="l1"`` as well."""

    def __init__(self, x, grid: Optional[torch.Tensor] = None, device: Optional[torch.device] = None):
        super().__init__(x, grid=grid, device=device)
        raw = self.raw
        self.qsum = torch.empty(max(self.n, 1), dtype=torch.int64, device=raw.device)
        self.asum = torch.empty(max(self.n, 1), dtype=torch.float64, device=raw.device)
        check(lib.cmve_jaccard_rowsums(handle(raw.device), _ptr(raw), _dtype_code(raw), _pw_ld(raw), self.n, self.d,
                                       _ptr(self.grid), self.n_pad, self.d_pad, _ptr(self.qsum), _ptr(self.asum)),
              "cmve_jaccard_rowsums")


def _l1_sets(a, b, a_set: Optional["L1Set"], b_set: Optional["L1Set"], cls=None):
    """Both sides as ``L1Set`` (``cls``: as ``JaccardSet``) on ONE grid: a resident side's when there is one, else
    both sets' elements."""
    if cls is None or cls is L1Set:
        cls = L1Set
    else:
        for given in (a_set, b_set):
            if given is not None and not isinstance(given, cls):
                raise TypeError(f'an L1Set holds no row sums: filter="jaccard" takes a {cls.__name__}')
    if a_set is not None and b_set is not None:
        if a_set.grid.data_ptr() != b_set.grid.data_ptr():
            raise ValueError("the two L1Set sides were packed on different grids: pack one with grid=other.grid")
        return a_set, b_set
    if a_set is not None:
        return a_set, cls(b, grid=a_set.grid)
    if b_set is not None:
        return cls(a, grid=b_set.grid), b_set
    grid = l1_grid(b, l1_grid(a))
    return cls(a, grid=grid), cls(b, grid=grid)


class _SadFilter(NamedTuple):
    """A SAD filter as every entry sees it: what it speaks for, what it packs and what it calls."""
    metric: str  # the ``_lib`` name of the one metric it speaks for ...
    score_dtype: torch.dtype  # ... with these score words, and with nothing else
    set_cls: type  # a packed side
    min_pairs: str  # the module-level auto threshold, by name: read at call time (the tests patch it)
    entry: str  # the C count entry; its workspace entry is ``entry + "_workspace"``
    extras: Tuple[str, ...]  # the per-set arrays both entries take after the codes and the errors
    # the top-k half (K23, K25).  Module-level names again, read at call time: the tests and the tools patch them
    set_words: str  # a packed side as the refusals name it
    topk: str  # the public call; ``topk + "_workspace"`` / ``"_auto"`` are its workspace size and its auto rule,
    #            ``"cmve_" + topk`` the C entry
    topk_min: Tuple[str, str, str, str]  # the auto rule's MIN_GALLERY, MIN_PAIRS (packed), MIN_Q, MIN_PLAIN_PAIRS

    words = property(lambda self: str(self.score_dtype).split(".")[-1])  # as the refusals name the score words

    def applies(self, metric: int, score_dtype) -> bool:
        return metric == getattr(_lib, self.metric) and score_dtype == self.score_dtype

    def set_now(self) -> type:
        """``set_cls`` under the name the module gives it when called (the tests patch ``L1Set``)."""
        return globals()[self.set_cls.__name__]


def _topk_min(prefix: str) -> Tuple[str, str, str, str]:
    return tuple(f"{prefix}_TOPK_FILTER_MIN_{x}" for x in ("GALLERY", "PAIRS", "Q", "PLAIN_PAIRS"))


# the routes of ``_filter_route`` that are SAD filters (K22 / K23, K24 / K25), in the order the auto rules ask them
_SAD_FILTERS = {
    "l1": _SadFilter("PW_L1", torch.float64, L1Set, "L1_FILTER_MIN_PAIRS", "cmve_l1_count", (),
                     "an L1Set", "l1_topk", _topk_min("L1")),
    "jaccard": _SadFilter("PW_JACCARD", torch.float32, JaccardSet, "JACCARD_FILTER_MIN_PAIRS",
                          "cmve_jaccard_count", ("qsum", "asum"), "a JaccardSet", "jaccard_topk", _topk_min("JACCARD")),
}


def _sad_side(f: _SadFilter, s: "L1Set") -> tuple:
    """One packed side as both of the filter's entries take it."""
    return (_ptr(s.raw), _dtype_code(s.raw), _pw_ld(s.raw), s.n, _ptr(s.codes), _ptr(s.err),
            *(_ptr(getattr(s, x)) for x in f.extras))


def _sad_count_call(route: str, h, a_set: "L1Set", b_set: "L1Set", alpha, beta, row, col, ws, ws_bytes: int, stats):
    """The route's count entry (row / col / ws / stats as ``_count_tail``; jaccard's item words are float32 values)."""
    f = _SAD_FILTERS[route]
    check(getattr(lib, f.entry)(h, *_sad_side(f, a_set), *_sad_side(f, b_set), a_set.d, _ptr(a_set.grid), float(alpha),
                                float(beta), *_count_tail(row, col, ws, ws_bytes, stats)), f.entry)


_l1_count_call = functools.partial(_sad_count_call, "l1")            # (the names the bench tools call)
_jaccard_count_call = functools.partial(_sad_count_call, "jaccard")


class _PairwisePositions:
    """One ``cmve_pairwise_positions`` call: per direction the 0-based positions, the item scores and the offsets.

    ``filter``: False -- the fp64 route (K18); True -- the K19 route for ``PW_L2`` with fp64 score words: both sides
    packed, the item scores from ``cmve_pairwise_item_scores``, the count from ``cmve_l2_count`` (fp16 MFMA filter +
    canonical re-score of the band: the same words); None -- the filter when it applies and na * nb reaches
    ``L2_FILTER_MIN_PAIRS``.  The filter is an accelerator: a band list that overflows is redone once with the
    reported need, and a band above 1/8 of the pairs runs the fp64 route.  ``filter_stats``: the four counters of
    the last ``cmve_l2_count`` plus ``redone`` / ``fallback``, or None when the filter was not tried.

    ``filter="l1"`` -- the K22 route for ``PW_L1`` with fp64 score words: both sides packed to uint16 codes on one
    grid, the item scores from ``cmve_pairwise_item_scores``, the count from ONE ``cmve_l1_count`` (integer SAD filter
    + canonical re-score of the band, an overflowing list resolved on the device: the same words, no redo);
    None takes it too when it applies and na * nb reaches ``L1_FILTER_MIN_PAIRS``.  ``filter_stats`` then carries
    the four counters, ``redone=False`` and ``fallback`` (the overflow word: the canonical count ran).

    ``filter="jaccard"`` -- the K24 route for ``PW_JACCARD`` with float32 score words: K22's codes plus the rows' code
    sums, the item words (float32) from ``cmve_pairwise_item_scores``, the count from ONE ``cmve_jaccard_count`` (no
    redo); None takes it too when it applies and na * nb reaches ``JACCARD_FILTER_MIN_PAIRS`` (never while that is
    None).  ``filter_stats`` as for ``"l1"``."""

    def __init__(self, a, b, metric, alpha, beta, score_dtype, row_lists=None, col_lists=None, filter=None):
        self.filter_stats = None
        route = _filter_route("pairwise_gt_positions", filter, metric, alpha, beta, score_dtype, False)
        a, b = _pw_pair(a, b, "pairwise_gt_positions")
        na, nb, dev = a.shape[0], b.shape[0], a.device
        if row_lists is not None and len(row_lists) != na:
            raise ValueError(f"pairwise_gt_positions: {len(row_lists)} row lists for {na} rows")
        if col_lists is not None and len(col_lists) != nb:
            raise ValueError(f"pairwise_gt_positions: {len(col_lists)} column lists for {nb} rows")
        self.n = (nb, na)  # the length of a row / of a column
        self.lists = (row_lists, col_lists)
        sides = []
        for lists in self.lists:
            if lists is None:
                sides.append((None, None, 0, None))
                continue
            off, idx = csr(lists, dev)
            items = sum(len(l) for l in lists)
            sides.append((off, idx, items, torch.empty(max(items, 1), dtype=torch.int32, device=dev)))
        (roff, ridx, ritems, rpos), (coff, cidx, citems, cpos) = sides
        route = route or _filter_route("pairwise_gt_positions", filter, metric, alpha, beta, score_dtype, False,
                                       (na * nb, a.shape[1], True))
        sc = None
        if route and na and nb and ritems + citems:
            sc = (self._filtered(a, b, alpha, beta, sides) if route == "l2"
                  else self._filtered_sad(route, a, b, alpha, beta, sides))
        if sc is None:
            nbytes = pairwise_positions_workspace(na, nb, ritems, citems, metric)
            ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
            check(lib.cmve_pairwise_positions(handle(dev), _ptr(a), _dtype_code(a), _pw_ld(a), na, _ptr(b),
                                              _dtype_code(b), _pw_ld(b), nb, a.shape[1], metric, float(alpha),
                                              float(beta), _pw_code(score_dtype), _ptr(roff), _ptr(ridx), ritems,
                                              _ptr(rpos), _ptr(coff), _ptr(cidx), citems, _ptr(cpos), _ptr(ws), nbytes),
                  "cmve_pairwise_positions")
            sc = ws.cpu().numpy()
        self._collect(sides, sc)

    def _filter_pass(self, a, b, metric, alpha, beta, sides, score_dtype=torch.float64):
        """What the filtered routes share.  The items' scores are computed into ONE device buffer with room for the
        counters; the run(call, nbytes) returned makes a workspace of nbytes, has call(row, col, ws, nbytes, stats)
        count into the sides' position buffers, and brings scores and counters to the host in one copy: (scores,
        {decided, band, rescored, overflow})."""
        (roff, _, ritems, rpos), (coff, _, citems, cpos) = sides
        na, nb, items = a.shape[0], b.shape[0], sides[0][2] + sides[1][2]
        buf = self._item_scores(a, b, metric, alpha, beta, sides, score_dtype)
        row, col = (roff, buf[:ritems], ritems, nb, rpos), (coff, buf[ritems:items], citems, na, cpos)

        def run(call, nbytes):
            ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=a.device)
            call(row, col, ws, nbytes, buf[items:])
            host = buf.cpu().numpy()
            return host[:items], _l2_count_stats(host[items:].view(np.int64))
        return run

    def _filtered(self, a, b, alpha, beta, sides):
        """The K19 route into the sides' position buffers; the items' scores (host), or None when the band is too
        large for the filter to pay (the caller then runs the fp64 route)."""
        dev, h, pairs = a.device, handle(a.device), a.shape[0] * b.shape[0]
        ra, rb = RowSet(a, with_lo=False, device=dev), RowSet(b, with_lo=False, device=dev)
        run = self._filter_pass(ra.raw, rb.raw, _lib.PW_L2, alpha, beta, sides)
        cap = l2_band_cap(pairs)
        for attempt in range(2):
            sc, st = run(lambda *tail: _l2_count_call("cmve_l2_count", h, ra, rb, alpha, beta, *tail),
                         l2_count_workspace(ra, rb, cap))
            self.filter_stats = dict(st, redone=attempt > 0, fallback=False)
            if not st["overflow"]:
                return sc
            cap = l2_band_plan(pairs, st["band"], st["overflow"], cap)  # (the call zeroes the positions again)
            if attempt or cap is None:
                break
        self.filter_stats["fallback"] = True
        return None

    @staticmethod
    def _item_scores(a, b, metric, alpha, beta, sides, score_dtype=torch.float64):
        """The items' scores (fp64 slots; rounded to ``score_dtype``), then room for a filter's four counters, in ONE
        device buffer: one copy to the host brings both."""
        (roff, ridx, ritems, _), (coff, cidx, citems, _) = sides
        na, nb = a.shape[0], b.shape[0]
        buf = torch.empty(ritems + citems + 4, dtype=torch.float64, device=a.device)
        start = 0
        for off, idx, items, col_dir, n_other in ((roff, ridx, ritems, 0, nb), (coff, cidx, citems, 1, na)):
            if items:
                out = buf[start:start + items]
                _item_scores_into(out, a, b, metric, alpha, beta, score_dtype, off, idx, items, col_dir, 0)
                # an index outside the other side scores NaN here (the sharded entry gives it the all-zero word)
                out.masked_fill_((idx[:items] < 0) | (idx[:items] >= n_other), float("nan"))
            start += items
        return buf

    def _filtered_sad(self, route, a, b, alpha, beta, sides):
        """The K22 / K24 route into the sides' position buffers; the items' scores (host).  ONE count call: a band
        list that overflows is resolved on the device (``fallback``: the canonical count ran), never redone."""
        f, h = _SAD_FILTERS[route], handle(a.device)
        sa, sb = _l1_sets(a, b, None, None, f.set_cls)
        run = self._filter_pass(a, b, getattr(_lib, f.metric), alpha, beta, sides, f.score_dtype)
        sc, st = run(lambda *tail: _sad_count_call(route, h, sa, sb, alpha, beta, *tail),
                     _sad_count_workspace(route, l2_band_cap(a.shape[0] * b.shape[0])))
        self.filter_stats = dict(st, redone=False, fallback=bool(st["overflow"]))
        return sc

    def _collect(self, sides, sc):
        self.pos, self.nan = [], []
        start = 0
        for (_, _, items, pos) in sides:
            self.pos.append(None if pos is None else pos[:items].cpu().numpy().astype(np.int64))
            self.nan.append(np.isnan(sc[start:start + items]))
            start += items

    def positions(self, side: int):
        """1-based positions as a list of int64 arrays aligned with the lists (None: direction not asked for)."""
        lists = self.lists[side]
        if lists is None:
            return None
        p = self.pos[side] + 1
        offs = np.zeros(len(lists) + 1, np.int64)
        np.cumsum([len(l) for l in lists], out=offs[1:])
        return [p[offs[i]:offs[i + 1]] for i in range(len(lists))]

    def ranks(self, side: int):
        """1-based best-GT ranks with rank_from_matrix's rules: 1 + the least position over the non-NaN items;
        an empty list ranks n + 1, a list whose items all score NaN ranks n."""
        lists = self.lists[side]
        if lists is None:
            return None
        n_m = self.n[side]
        lens = np.fromiter((len(l) for l in lists), np.int64, count=len(lists))
        big = np.iinfo(np.int64).max
        best = np.full(len(lists), big, np.int64)
        np.minimum.at(best, np.repeat(np.arange(len(lists)), lens), np.where(self.nan[side], big, self.pos[side]))
        ranks = np.where(best == big, n_m - 1, best) + 1
        ranks[lens == 0] = n_m + 1
        return ranks


def pairwise_gt_positions(a, b, metric: int, alpha: float, beta: float, score_dtype, row_lists=None, col_lists=None,
                          filter=None):
    """(row_positions, col_positions): 1-based positions of every listed item under a non-cosine measure, as
    ``metrics.gt_positions`` gives them on ``pairwise(a, b, ...)`` and on its transpose -- without the matrix (K18).
    row_lists[i]: rows of b listed for row i of a; col_lists[j]: rows of a listed for row j of b."""
    r = _PairwisePositions(a, b, metric, alpha, beta, score_dtype, row_lists, col_lists, filter)
    return r.positions(0), r.positions(1)


def pairwise_gt_ranks(a, b, metric: int, alpha: float, beta: float, score_dtype, row_lists=None, col_lists=None,
                      filter=None):
    """(row_ranks, col_ranks) == ``rank_from_matrix`` on ``pairwise(a, b, ...)`` in both orientations (K18)."""
    r = _PairwisePositions(a, b, metric, alpha, beta, score_dtype, row_lists, col_lists, filter)
    return r.ranks(0), r.ranks(1)


def pairwise_gt_eval(a, b, metric: int, alpha: float, beta: float, score_dtype, row_lists=None, col_lists=None,
                     filter=None):
    """((row_positions, row_ranks), (col_positions, col_ranks)) from ONE ``cmve_pairwise_positions`` call: what
    cal_perf needs (both directions' ranks and every mAP position)."""
    r = _PairwisePositions(a, b, metric, alpha, beta, score_dtype, row_lists, col_lists, filter)
    return (r.positions(0), r.ranks(0)), (r.positions(1), r.ranks(1))


def pairwise_item_scores(a, b, metric: int, alpha: float, beta: float, score_dtype, off: torch.Tensor,
                         idx: torch.Tensor, n_items: int, col_dir: bool = False, idx_base: int = 0) -> torch.Tensor:
    """fp64 [n_items] on the device: the score of every listed item this call owns (``cmve_pairwise_item_scores``,
    K18's launch 1 for a gallery sharded by rows).  (off, idx): one CSR side on the device (``csr``) -- the lists of
    a's rows naming GLOBAL rows of b (col_dir: of b's rows naming global rows of a), of which the operand given here
    is [idx_base, idx_base + n).  An item outside that range gets the all-zero word: the int64 SUM over the shards of
    ``out.view(torch.int64)`` is every item's score, bit for bit.  No host copy, no synchronisation."""
    a, b = _pw_pair(a, b, "pairwise_item_scores")
    if idx.numel() < int(n_items) or idx.dtype != torch.int32 or off.dtype != torch.int64:
        raise ValueError(f"pairwise_item_scores: {n_items} items need int64 offsets and as many int32 indices")
    out = torch.empty(max(int(n_items), 1), dtype=torch.float64, device=a.device)
    _item_scores_into(out, a, b, metric, alpha, beta, score_dtype, off, idx, n_items, col_dir, idx_base)
    return out[:int(n_items)]


def l2_band_cap(pairs: int) -> int:
    """The band list a first filtered count over ``pairs`` pairs is given: 1/128 of the pairs, at least 65,536
    slots, never more than the 1/8 above which the filter stops paying."""
    return max(1, min(pairs // 8, max(1 << 16, pairs // 128)))


def l2_band_plan(pairs: int, band: int, overflow, cap: int) -> Optional[int]:
    """The band capacity for the NEXT filtered count over ``pairs`` pairs, from the counters of the last one (pure
    host arithmetic): ``cap`` when its list held the band, the reported ``band`` when it overflowed and
    ``band * 8 <= pairs`` (one list of that size suffices), None above that -- stop asking the filter: the fp64
    route is the cheaper one for these rows."""
    if not overflow:
        return int(cap)
    return int(band) if int(band) * 8 <= int(pairs) else None


def pairwise_count(a, b, metric: int, alpha: float, beta: float, score_dtype, row=None, col=None,
                   filter: Optional[bool] = None, band: Optional[torch.Tensor] = None, return_stats: bool = False):
    """(row_pos, col_pos): int32 device tensors of 0-based positions counted over THIS call's pairs against the
    caller's item scores (``cmve_pairwise_count``, K18's launch 2).  row = (off [na + 1], scores fp64 [items], n):
    a non-NaN item's word is #{ j : e(i, j) < score }; a NaN item's is n - (NaN items of its list) + (its place
    among them) when n > 0 and 0 when n == 0 (one shard passes the global n).  col: the mirror; a direction left
    None gives None.  No host copy, no synchronisation.

    a / b: plain rows, or a ``RowSet`` packed with eps = 0, ``with_lo=False`` and its fp16 plane (a resident side is
    packed once; its ``.raw`` rows are the fp64 route's operand).  ``filter``: False -- ``cmve_pairwise_count``; True
    -- ``cmve_l2_count_resolved`` (K21: the fp16 MFMA filter with the band re-scored on the canonical chain, and a
    band list that overflows resolved ON THE DEVICE by the canonical count: the same words either way, nothing read
    on the host), ValueError unless the metric is ``PW_L2`` with float64 score words, alpha finite and non-zero and
    beta finite; None -- the filter when it applies and na * nb reaches ``L2_FILTER_MIN_PAIRS``.  Plain rows are
    packed inside the call when the filter runs.  ``band``: a caller-owned int64 device tensor that holds the band
    list, one slot per element (None: a fresh one of ``l2_band_cap(na * nb)`` slots).  ``return_stats``: also return
    the int64 [4] DEVICE tensor {decided, band found, band re-scored, overflow} (``l2_band_plan`` reads it once the
    caller has it on the host), or None when the filter did not run.

    ``filter="l1"`` -- ``cmve_l1_count`` (K22: the integer SAD filter of ``PW_L1``, the band re-scored on the canonical
    chain and an overflowing list resolved on the device: the same words), ValueError unless the metric is ``PW_L1``
    with float64 score words, alpha finite and non-zero and beta finite; None also takes it when it applies and
    na * nb reaches ``L1_FILTER_MIN_PAIRS`` (never while that is None).  a / b may then be an ``L1Set`` (a resident
    side packed once; the other side is packed on its grid inside the call) -- plain rows on both sides share a
    grid made from both.  ``band`` / ``return_stats`` as above.

    ``filter="jaccard"`` -- ``cmve_jaccard_count`` (K24: the same SAD filter under ``PW_JACCARD`` with float32 score
    words -- the item scores are float32 values in float64 slots --, the band re-scored on the canonical
    two-accumulator chain, an overflowing list resolved on the device: the same words), ValueError unless the metric
    is ``PW_JACCARD`` with float32 score words, alpha finite and non-zero and beta finite; None also takes it when it
    applies and na * nb reaches ``JACCARD_FILTER_MIN_PAIRS`` (never while that is None).  a / b may then be a
    ``JaccardSet`` (an ``L1Set`` plus the rows' code sums; a resident side packed once)."""
    route = _filter_route("pairwise_count", filter, metric, alpha, beta, score_dtype, True)
    a_l1, b_l1 = (a if isinstance(a, L1Set) else None), (b if isinstance(b, L1Set) else None)
    a_set = a if isinstance(a, RowSet) else None
    b_set = b if isinstance(b, RowSet) else None
    a, b = _pw_pair(a.raw if isinstance(a, (RowSet, L1Set)) else a, b.raw if isinstance(b, (RowSet, L1Set)) else b,
                    "pairwise_count")
    na, nb, dev = a.shape[0], b.shape[0], a.device
    sides = []
    for side, n_lists in ((row, na), (col, nb)):
        if side is None:
            sides.append((None, None, 0, 0, None))
            continue
        off, sc, n = side
        if off.numel() != n_lists + 1:
            raise ValueError(f"pairwise_count: {off.numel() - 1} lists for {n_lists} rows")
        if sc.dtype != torch.float64 or not sc.is_contiguous():
            raise TypeError("pairwise_count: item scores are contiguous float64")
        sides.append((off, sc, sc.numel(), int(n), torch.empty(max(sc.numel(), 1), dtype=torch.int32, device=dev)))
    (roff, rsc, ritems, rn, rpos), (coff, csc, citems, cn, cpos) = sides
    # (auto never hands the entry what it refuses; filter=True does, and the entry says so)
    route = route or _filter_route("pairwise_count", filter, metric, alpha, beta, score_dtype, True,
                                   (na * nb, a.shape[1], _l2_set_ok(a_set) and _l2_set_ok(b_set)))
    if filter is None and route == "jaccard" and any(s is not None and not isinstance(s, JaccardSet)
                                                     for s in (a_l1, b_l1)):
        route = None  # (a plain L1Set holds no row sums: the K18 route on its raw rows)
    stats = None
    if route:
        if band is None:
            band = torch.empty(l2_band_cap(na * nb), dtype=torch.int64, device=dev)
        elif band.dtype != torch.int64 or not band.is_contiguous() or band.device != dev:
            raise TypeError("pairwise_count: band is a contiguous int64 tensor on the rows' device")
        stats = torch.empty(4, dtype=torch.int64, device=dev)
    if route in _SAD_FILTERS:
        a_l1, b_l1 = _l1_sets(a, b, a_l1, b_l1, _SAD_FILTERS[route].set_cls)
        _sad_count_call(route, handle(dev), a_l1, b_l1, alpha, beta, sides[0], sides[1], band, _nbytes(band), stats)
    elif route == "l2":
        if a_l1 is not None or b_l1 is not None:
            raise TypeError("pairwise_count: an L1Set is packed for filter=\"l1\"; the Euclidean filter takes a RowSet")
        if a_set is None:
            a_set = RowSet(a, with_lo=False, device=dev)
        if b_set is None:
            b_set = RowSet(b, with_lo=False, device=dev)
        _l2_count_call("cmve_l2_count_resolved", handle(dev), a_set, b_set, alpha, beta, sides[0], sides[1], band,
                       _nbytes(band), stats)
    else:
        check(lib.cmve_pairwise_count(handle(dev), _ptr(a), _dtype_code(a), _pw_ld(a), na, _ptr(b), _dtype_code(b),
                                      _pw_ld(b), nb, a.shape[1], metric, float(alpha), float(beta),
                                      _pw_code(score_dtype), _ptr(roff), _ptr(rsc), ritems, rn, _ptr(rpos), _ptr(coff),
                                      _ptr(csc), citems, cn, _ptr(cpos)), "cmve_pairwise_count")
    out = (None if rpos is None else rpos[:ritems]), (None if cpos is None else cpos[:citems])
    return out + (stats,) if return_stats else out


def pairwise_list_ranks(off: torch.Tensor, scores: torch.Tensor, pos: torch.Tensor, n_m: int) -> torch.Tensor:
    """int64 [n_lists] on the device: the 1-based best-GT rank of every list from its items' scores (fp64) and
    0-based positions (int32) -- ``_PairwisePositions.ranks`` without the host (``cmve_pairwise_list_ranks``)."""
    n_lists = off.numel() - 1
    if scores.dtype != torch.float64 or pos.dtype != torch.int32 or scores.numel() != pos.numel():
        raise TypeError("pairwise_list_ranks: float64 scores and int32 positions of one length")
    out = torch.empty(max(n_lists, 1), dtype=torch.int64, device=off.device)
    if scores.numel() == 0:  # every list is empty: the kernel reads neither, but the entry takes no NULL
        scores, pos = scores.new_zeros(1), pos.new_zeros(1)
    check(lib.cmve_pairwise_list_ranks(handle(off.device), _ptr(off), _ptr(scores.contiguous()),
                                       _ptr(pos.contiguous()), n_lists, int(n_m), _ptr(out)),
          "cmve_pairwise_list_ranks")
    return out[:n_lists]


L2_TOPK_CAND_MAX = 2048  # cmve_l2_topk's limit on cand_cap, and so on k: what its last launch sorts in LDS
# the share of unresolved queries above which engine.pairwise_topk answers the whole call on the fp64 route: past it
# the filter's launches are mostly wasted (rows clustered far from the origin leave EVERY query unresolved)
L2_TOPK_MAX_UNRESOLVED = 0.25
# Auto dispatch of the K20 filter (``filter=None``), from tools/l2_topk_bench.py -> profiles/l2_topk.json (top-10,
# D = 1024, medians of 5 alternating repeats; "wins" = by more than the two spreads together).  Against a gallery that
# is already packed (a RowSet: GalleryScorer, ShardedGallery) the filter won at every n_q from 1 to 16,384 over 131,072
# and 1,048,576 rows (0.80 against 0.87 ms at n_q = 1 over 131,072; 7.2 against 148 ms at 1000 over 1,048,576), and over
# 16,384 rows from 256 queries (0.89 against 1.11 ms) but not at 64 (0.87 against 0.78 ms; below that both routes are
# launch gaps, 0.59-0.66 ms): a packed gallery takes it from MIN_GALLERY rows or MIN_PAIRS pairs.  A gallery given as
# plain rows is packed inside the call (0.16 / 0.50 / 3.9 ms at 16,384 / 131,072 / 1,048,576 rows), which the filter
# earned back from 64 queries over 131,072 rows and 256 over 16,384, not at 16 over 131,072: plain rows take it from
# MIN_Q queries AND MIN_PAIRS pairs.  Between the measured gallery sizes the pair rule is an interpolation.
L2_TOPK_FILTER_MIN_Q = 64
L2_TOPK_FILTER_MIN_PAIRS = 1 << 22
L2_TOPK_FILTER_MIN_GALLERY = 131072


def l2_topk_auto(n_q: int, n_g: int, packed: bool = False) -> bool:
    """Whether ``pairwise_topk(filter=None)`` takes the K20 filter at this size (given PW_L2 with fp64 words);
    ``packed``: the gallery is a RowSet already."""
    if n_q < 1 or n_g < 1:
        return False
    if packed:
        return n_g >= L2_TOPK_FILTER_MIN_GALLERY or n_q * n_g >= L2_TOPK_FILTER_MIN_PAIRS
    return n_q >= L2_TOPK_FILTER_MIN_Q and n_q * n_g >= L2_TOPK_FILTER_MIN_PAIRS


def l2_topk_workspace(q: "RowSet", g: "RowSet", k: int, cand_cap: Optional[int] = None,
                      sample_rows: Optional[int] = None) -> int:
    """Bytes of workspace ``cmve_l2_topk`` needs (host only: no launch)."""
    n = C.c_int64()
    check(lib.cmve_l2_topk_workspace(C.byref(q.desc), C.byref(g.desc), int(k),
                                     L2_TOPK_CAND_MAX if cand_cap is None else int(cand_cap),
                                     int(sample_rows or 0), C.byref(n)), "cmve_l2_topk_workspace")
    return n.value


def _filtered_topk_call(fn, name: str, head: tuple, n_q: int, k: int, nbytes: int, ws, dev):
    """What ``l2_topk`` and ``l1_topk`` share: ``fn(handle, *head, ws, nbytes, idx, err, stats)`` with ws the caller's
    when it holds ``nbytes`` at an 8-byte aligned address (a fresh one otherwise), fresh outputs, the stats record."""
    if ws is None or _nbytes(ws) < nbytes or ws.data_ptr() % 8:
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
    idx = torch.empty((n_q, int(k)), dtype=torch.int64, device=dev)
    err = torch.empty((n_q, int(k)), dtype=torch.float64, device=dev)
    st = torch.empty(4, dtype=torch.int64, device=dev)
    check(fn(handle(dev), *head, _ptr(ws), nbytes, _ptr(idx), _ptr(err), _ptr(st)), name)
    return idx, err, _stats4(("excluded", "candidates", "rescored", "unresolved"), st.cpu().numpy())


def l2_topk(q: "RowSet", g: "RowSet", alpha: float, beta: float, k: int, cand_cap: Optional[int] = None,
            sample_rows: Optional[int] = None, ws: Optional[torch.Tensor] = None):
    """``cmve_l2_topk`` (K20): (idx int64 [n_q, k], err fp64 [n_q, k]) on the device and the stats dict
    {excluded, candidates, rescored, unresolved} (one small copy to the host).  An unresolved query has
    idx[i, 0] == -2 and the rest of its row unwritten.  k must not exceed the gallery.  ws: a caller-held device
    workspace, used when it holds ``l2_topk_workspace`` bytes (a fresh one otherwise)."""
    cap = L2_TOPK_CAND_MAX if cand_cap is None else int(cand_cap)
    head = (C.byref(q.desc), C.byref(g.desc), float(alpha), float(beta), int(k), cap, int(sample_rows or 0))
    return _filtered_topk_call(lib.cmve_l2_topk, "cmve_l2_topk", head, q.n, k,
                               l2_topk_workspace(q, g, k, cap, sample_rows), ws, g.device)


# ---- the SAD-filtered top-ks (K23, K25): ONE implementation over the ``_SAD_FILTERS`` record; the public names below it
# are one-line wrappers, and generic code reaches a family's functions and constants by name when called ----
def _n_rows(s) -> int:
    return int(s.n) if hasattr(s, "n") else int(s)


def _sad_topk_auto(route: str, n_q: int, n_g: int, packed: bool = False) -> bool:
    """The route's auto rule from ITS four constants alone: a packed gallery takes the filter from MIN_GALLERY rows or
    MIN_PAIRS pairs, plain rows from MIN_Q queries AND MIN_PLAIN_PAIRS pairs; None switches a clause off."""
    if n_q < 1 or n_g < 1:
        return False
    min_gallery, min_pairs, min_q, min_plain = (globals()[name] for name in _SAD_FILTERS[route].topk_min)
    if packed:
        return ((min_gallery is not None and n_g >= min_gallery)
                or (min_pairs is not None and n_q * n_g >= min_pairs))
    return min_q is not None and min_plain is not None and n_q >= min_q and n_q * n_g >= min_plain


def _sad_topk_workspace(route: str, q, g, k: int, cand_cap: Optional[int] = None,
                        sample_rows: Optional[int] = None) -> int:
    """Bytes of workspace the route's top-k entry needs (host only: no launch).  q / g: a packed set or a row count."""
    entry = f"cmve_{_SAD_FILTERS[route].topk}_workspace"
    n = C.c_int64()
    check(getattr(lib, entry)(_n_rows(q), _n_rows(g), int(k), L2_TOPK_CAND_MAX if cand_cap is None else int(cand_cap),
                              int(sample_rows or 0), C.byref(n)), entry)
    return n.value


def _sad_topk(route: str, q: "L1Set", g: "L1Set", alpha: float, beta: float, k: int, cand_cap: Optional[int] = None,
              sample_rows: Optional[int] = None, ws: Optional[torch.Tensor] = None):
    """The route's top-k entry over two sets packed on ONE grid: (idx, err, stats) as ``l2_topk``.  (The three
    ``*_TOPK_CAND_MAX`` are one number: the same last launch, the same LDS.)"""
    f = _SAD_FILTERS[route]
    q, g = _l1_sets(None, None, q, g, f.set_now())
    if q.d != g.d:
        raise ValueError(f"{f.topk}: dimensions differ ({q.d}, {g.d})")
    cap = L2_TOPK_CAND_MAX if cand_cap is None else int(cand_cap)
    head = (*_sad_side(f, q), *_sad_side(f, g), g.d, _ptr(g.grid), float(alpha), float(beta), int(k), cap,
            int(sample_rows or 0))
    return _filtered_topk_call(getattr(lib, "cmve_" + f.topk), "cmve_" + f.topk, head, q.n, k,
                               _sad_topk_workspace(route, q, g, k, cap, sample_rows), ws, g.device)


# the public face of a SAD route: what a caller that holds a resident gallery (cmve.linas.inference, cmve.dist) needs,
# without naming the families.  The per-family names are resolved when called, so a patched ``l1_topk_auto`` is asked.
def sad_route_of(metric: int, score_dtype) -> Optional[str]:
    """The SAD filter family that speaks for ``metric`` with these score words: ``"l1"``, ``"jaccard"`` or None.  The
    word is the ``filter=`` value that forces it."""
    return next((route for route, f in _SAD_FILTERS.items() if f.applies(metric, score_dtype)), None)


def sad_set(route: str, rows, grid: Optional[torch.Tensor] = None) -> "L1Set":
    """``rows`` packed for the route (an ``L1Set`` / a ``JaccardSet``), on their own grid or on ``grid``."""
    return _SAD_FILTERS[route].set_now()(rows, grid=grid)


def sad_min_pairs(route: str) -> Optional[int]:
    """The pairs from which ``filter=None`` takes the route's COUNT filter (None: never)."""
    return globals()[_SAD_FILTERS[route].min_pairs]


def sad_topk_auto(route: str, n_q: int, n_g: int, packed: bool = False) -> bool:
    """Whether ``pairwise_topk(filter=None)`` takes the route's top-k filter at this size (``l1_topk_auto`` /
    ``jaccard_topk_auto``)."""
    return globals()[_SAD_FILTERS[route].topk + "_auto"](n_q, n_g, packed=packed)


def sad_topk_workspace(route: str, n_q, n_g, k: int) -> int:
    """Bytes of workspace the route's top-k needs (``l1_topk_workspace`` / ``jaccard_topk_workspace``)."""
    return globals()[_SAD_FILTERS[route].topk + "_workspace"](n_q, n_g, k)


L1_TOPK_CAND_MAX = L2_TOPK_CAND_MAX  # cmve_l1_topk's limit on cand_cap: the same last launch, the same LDS
# Auto dispatch of the K23 filter (``filter=None``), a rule of its own beside K20's (None in a constant switches its
# clause off: "never taken automatically", as K22 allowed for ``L1_FILTER_MIN_PAIRS``).  From tools/l1_topk_bench.py ->
# profiles/l1_topk.json (top-10, D = 1024, fp64 rows, l1, medians of 5 alternating repeats, fp64 route / filter in ms;
# "wins" = by more than the two spreads together; the constants were None while it ran).  Against a gallery that is
# already packed (an L1Set: GalleryScorer, the sharded gallery) the filter won at 64 x 131,072 (1.91 / 1.19), 1000 x
# 131,072 (18.0 / 4.17), 16,384 x 131,072 (327.1 / 64.7) and over 1,048,576 rows at every n_q: 1 (3.27 / 3.02,
# spreads 0.08 + 0.05), 64 (11.85 / 3.85), 1000 (141.7 / 19.4); it lost at 1 x 131,072 (0.88 / 1.09: both are launch
# gaps).  A packed gallery takes it from MIN_GALLERY rows or MIN_PAIRS pairs, the smallest sizes measured to win.  A
# gallery given as plain rows pays the grid and both packs inside the call (0.78 ms at 131,072 rows, 4.8 ms at
# 1,048,576): it won at 64 x 1,048,576 (11.72 / 8.63), 1000 x 131,072 (17.9 / 5.07), 1000 x 1,048,576 (141.5 / 24.5) and
# 16,384 x 131,072 (326.0 / 65.6), tied at 64 x 131,072 (1.93 / 1.99) and lost at one query (3.26 / 7.76 over
# 1,048,576): plain rows take it from MIN_Q queries AND MIN_PLAIN_PAIRS pairs.  Between the measured sizes the pair
# rules are an interpolation.
L1_TOPK_FILTER_MIN_GALLERY = 1 << 20      # packed: 1 x 1,048,576
L1_TOPK_FILTER_MIN_PAIRS = 1 << 23        # packed: 64 x 131,072
L1_TOPK_FILTER_MIN_Q = 64                 # plain rows
L1_TOPK_FILTER_MIN_PLAIN_PAIRS = 1 << 26  # plain rows: 64 x 1,048,576


def l1_topk_auto(n_q: int, n_g: int, packed: bool = False) -> bool:
    """Whether ``pairwise_topk(filter=None)`` takes the K23 filter at this size (given PW_L1 with fp64 words);
    ``packed``: the gallery is an L1Set already.  A constant left None switches its clause off."""
    return _sad_topk_auto("l1", n_q, n_g, packed)


def l1_topk_workspace(q, g, k: int, cand_cap: Optional[int] = None, sample_rows: Optional[int] = None) -> int:
    """Bytes of workspace ``cmve_l1_topk`` needs (host only: no launch).  q / g: an ``L1Set`` or a row count."""
    return _sad_topk_workspace("l1", q, g, k, cand_cap, sample_rows)


def l1_topk(q: "L1Set", g: "L1Set", alpha: float, beta: float, k: int, cand_cap: Optional[int] = None,
            sample_rows: Optional[int] = None, ws: Optional[torch.Tensor] = None):
    """``cmve_l1_topk`` (K23): (idx int64 [n_q, k], err fp64 [n_q, k]) on the device and the stats dict
    {excluded, candidates, rescored, unresolved} (one small copy to the host), as ``l2_topk``.  Both sets are packed
    on ONE grid (ValueError otherwise).  An unresolved query has idx[i, 0] == -2 and the rest of its row unwritten.
    k must not exceed the gallery.  ws: a caller-held device workspace, used when it holds ``l1_topk_workspace``
    bytes (a fresh one otherwise)."""
    return _sad_topk("l1", q, g, alpha, beta, k, cand_cap, sample_rows, ws)


JACCARD_TOPK_CAND_MAX = L2_TOPK_CAND_MAX  # cmve_jaccard_topk's limit on cand_cap: the same last launch, the same LDS
# Auto dispatch of the K25 filter (``filter=None`` under PW_JACCARD with float32 words): a rule of its own with
# ``l1_topk_auto``'s clauses (None in a constant switches its clause off: "never taken automatically",
# ``filter="jaccard"`` alone runs it).  From tools/jaccard_topk_bench.py -> profiles/jaccard_topk.json (top-10, D = 1024,
# non-negative float32 rows, alpha = -1, medians of 5 alternating repeats, K18 route / filter in ms; "wins" = by more
# than the two spreads together; the constants were None while it ran).  Against a gallery that is already packed (a
# JaccardSet: GalleryScorer, the sharded gallery) the filter won at 64 x 131,072 (2.45 / 1.62, spreads 0.07 + 0.01),
# 1000 x 131,072 (28.9 / 4.52), 16,384 x 131,072 (502.6 / 70.2) and over 1,048,576 rows at every n_q: 1 (3.32 / 3.05,
# spreads 0.01 + 0.05), 64 (17.1 / 3.76), 1000 (232.0 / 20.8); it lost at 1 x 131,072 (0.83 / 1.11: both are launch
# gaps).  A packed gallery takes it from MIN_GALLERY rows or MIN_PAIRS pairs, the smallest sizes measured to win.  A
# gallery given as plain rows pays the grid, both packs and the row sums inside the call (0.92 ms at 131,072 rows,
# 5.7 ms at 1,048,576): it won at 64 x 1,048,576 (17.3 / 9.51), 1000 x 131,072 (29.0 / 5.53), 1000 x 1,048,576
# (232.0 / 26.4) and 16,384 x 131,072 (502.8 / 71.4), lost at 64 x 131,072 (2.45 / 2.56) and at one query (0.83 / 1.97
# and 3.30 / 8.67): plain rows take it from MIN_Q queries AND MIN_PLAIN_PAIRS pairs.  Between the measured sizes the
# pair rules are an interpolation.
JACCARD_TOPK_FILTER_MIN_GALLERY = 1 << 20      # packed: 1 x 1,048,576
JACCARD_TOPK_FILTER_MIN_PAIRS = 1 << 23        # packed: 64 x 131,072
JACCARD_TOPK_FILTER_MIN_Q = 64                 # plain rows
JACCARD_TOPK_FILTER_MIN_PLAIN_PAIRS = 1 << 26  # plain rows: 64 x 1,048,576


def jaccard_topk_auto(n_q: int, n_g: int, packed: bool = False) -> bool:
    """Whether ``pairwise_topk(filter=None)`` takes the K25 filter at this size (given PW_JACCARD with float32 words);
    ``packed``: the gallery is a JaccardSet already.  A constant left None switches its clause off."""
    return _sad_topk_auto("jaccard", n_q, n_g, packed)


def jaccard_topk_workspace(q, g, k: int, cand_cap: Optional[int] = None, sample_rows: Optional[int] = None) -> int:
    """Bytes of workspace ``cmve_jaccard_topk`` needs (host only: no launch).  q / g: a ``JaccardSet`` or a row
    count."""
    return _sad_topk_workspace("jaccard", q, g, k, cand_cap, sample_rows)


def jaccard_topk(q: "JaccardSet", g: "JaccardSet", alpha: float, beta: float, k: int, cand_cap: Optional[int] = None,
                 sample_rows: Optional[int] = None, ws: Optional[torch.Tensor] = None):
    """``cmve_jaccard_topk`` (K25): (idx int64 [n_q, k], err fp64 [n_q, k] holding float32 words) on the device and the
    stats dict {excluded, candidates, rescored, unresolved} (one small copy to the host), as ``l1_topk``.  Both sets
    are ``JaccardSet`` packed on ONE grid (TypeError / ValueError otherwise).  An unresolved query has
    idx[i, 0] == -2 and the rest of its row unwritten.  k must not exceed the gallery.  ws: a caller-held device
    workspace, used when it holds ``jaccard_topk_workspace`` bytes (a fresh one otherwise)."""
    return _sad_topk("jaccard", q, g, alpha, beta, k, cand_cap, sample_rows, ws)


def _topk_filtered(metric: int, filtered, q, g, alpha, beta, k, score_dtype=torch.float64):
    """A filtered route of ``pairwise_topk`` (K20: ``metric`` PW_L2, K23: PW_L1, K25: PW_JACCARD with float32 words):
    ``filtered()`` is the filter's call and returns (idx, err, stats) as ``l2_topk`` / ``l1_topk`` do; q / g are the
    raw rows, ``score_dtype`` the call's own (unresolved rows are re-run with it).  Returns (idx, err) on the device
    with the same words as the K18 route, and the ``topk_stats`` record; idx is None when the whole call has to take
    the K18 route."""
    idx, err, stats = filtered()
    n_q = q.shape[0]
    stats.update(fallback_rows=0, fallback=False)
    if stats["unresolved"]:
        if stats["unresolved"] > L2_TOPK_MAX_UNRESOLVED * n_q:
            stats.update(fallback_rows=n_q, fallback=True)
            return None, None, stats
        rows = (idx[:, 0] == -2).nonzero().flatten()
        sub_i, sub_e = pairwise_topk(q[rows], g, metric, alpha, beta, score_dtype, k, to_host=False, filter=False)
        idx[rows], err[rows] = sub_i, sub_e
        stats["fallback_rows"] = int(rows.numel())
    return idx, err, stats


def pairwise_topk(q, g, metric: int, alpha: float, beta: float, score_dtype, k: int, to_host: bool = True,
                  ws: Optional[torch.Tensor] = None, ws_bytes: Optional[int] = None, geometry: int = 0,
                  filter: Optional[bool] = None, cand_cap: Optional[int] = None, sample_rows: Optional[int] = None,
                  return_stats: bool = False):
    """The k rows of g with the smallest error per row of q under a non-cosine measure, by (error asc, index asc),
    NaN last -- a stable argsort of ``pairwise(q, g, ...)`` cut at k, without the matrix (K18).  Returns
    (idx int64 [n_q, k], errors fp64 [n_q, k]); k is clamped to the gallery.  ws: a caller-held uint8 device
    workspace (at least the minimum of ``pairwise_topk_workspace``; default: the recommended size); ws_bytes
    sizes a fresh one.  The K20 route uses ws too when it holds ``l2_topk_workspace`` bytes; a call that then falls
    back to the fp64 route with a ws below that route's minimum allocates its own.

    ``filter``: False -- the fp64 route (K18); True -- the K20 route for ``PW_L2`` with float64 score words
    (``cmve_l2_topk``: fp16 MFMA filter, canonical re-score of the candidates: the same words), ValueError for any
    other measure; None -- the filter when it applies and ``l2_topk_auto`` says it pays (a packed gallery: from
    ``L2_TOPK_FILTER_MIN_GALLERY`` rows or ``L2_TOPK_FILTER_MIN_PAIRS`` pairs; plain rows: from
    ``L2_TOPK_FILTER_MIN_Q`` queries and that many pairs).  g (and q) may be a ``RowSet`` packed with eps = 0: a
    resident gallery is packed once and its ``.raw`` rows are the fp64 route's operand; plain rows are packed per call.  The filter is an
    accelerator: queries it leaves unresolved are re-run on the fp64 route and scattered back, more than
    ``L2_TOPK_MAX_UNRESOLVED`` of them (and k > ``L2_TOPK_CAND_MAX``) send the whole call there.  ``cand_cap`` /
    ``sample_rows``: ``cmve_l2_topk``'s.  ``return_stats``: also return ``topk_stats`` -- {excluded, candidates,
    rescored, unresolved, fallback_rows, fallback}, or None when the filter was not tried.

    ``filter="l1"`` -- the K23 route for ``PW_L1`` with float64 score words (``cmve_l1_topk``: the integer SAD filter of
    K22, canonical re-score of the candidates: the same words), ValueError unless the metric is ``PW_L1`` with
    float64 score words, alpha finite and non-zero and beta finite; None also takes it when it applies and
    ``l1_topk_auto`` says it pays (never while its ``L1_TOPK_FILTER_MIN_*`` are None).  g (and q) may then be an
    ``L1Set``: a resident gallery is packed once on its own grid and the queries are packed on ``g.grid`` inside the
    call; plain rows on both sides share a grid made from both; two ``L1Set`` on different grids are a ValueError.
    Unresolved queries, the whole-call fallback, ``cand_cap`` / ``sample_rows`` and ``topk_stats``: as above.

    ``filter="jaccard"`` -- the K25 route for ``PW_JACCARD`` with float32 score words (``cmve_jaccard_topk``: the same
    SAD filter under K24's interval of the two sums, canonical re-score of the candidates with the one rounding to
    float32: the same words), ValueError unless the metric is ``PW_JACCARD`` with float32 score words, alpha finite
    and non-zero and beta finite; None also takes it when it applies and ``jaccard_topk_auto`` says it pays (never
    while its ``JACCARD_TOPK_FILTER_MIN_*`` are None; the L1 and L2 constants are not consulted).  g (and q) may then
    be a ``JaccardSet``, as an ``L1Set`` above; a ``RowSet`` or a bare ``L1Set`` is a TypeError.  Unresolved queries
    are re-run with float32 words; the rest as above."""
    route = _filter_route("pairwise_topk", filter, metric, alpha, beta, score_dtype, False)
    g_set = g if isinstance(g, RowSet) else None
    q_set = q if isinstance(q, RowSet) else None
    g_l1 = g if isinstance(g, L1Set) else None
    q_l1 = q if isinstance(q, L1Set) else None
    q, g = _pw_pair(q.raw if isinstance(q, (RowSet, L1Set)) else q, g.raw if isinstance(g, (RowSet, L1Set)) else g,
                    "pairwise_topk")
    n_q, n_g = q.shape[0], g.shape[0]

    def result(idx, err, stats):
        out = (idx.cpu().numpy(), err.cpu().numpy()) if to_host and torch.is_tensor(idx) else (idx, err)
        return out + (stats,) if return_stats else out

    k = int(min(k, n_g))
    if k < 1:
        return result(np.zeros((n_q, 0), np.int64), np.zeros((n_q, 0)), None)
    if k > _lib.TOPK_MAX:
        raise ValueError(f"pairwise_topk: k <= {_lib.TOPK_MAX}")
    if filter is None and _l2_scaling_ok(alpha, beta):
        # auto never hands an entry what it refuses; a forced route does, and the entry says so
        if _l2_applies(metric, score_dtype):
            if l2_topk_auto(n_q, n_g, g_set is not None) and _l2_set_ok(q_set) and _l2_set_ok(g_set):
                route = "l2"
        else:
            for name, f in _SAD_FILTERS.items():  # (the one family that speaks for the call, and its own rule alone)
                if f.applies(metric, score_dtype):
                    if sad_topk_auto(name, n_q, n_g, isinstance(g_l1, f.set_now())) and q.shape[1] <= L1_D_MAX:
                        route = name
                    break
    topk_stats = None
    if route and n_q > 0 and k <= L2_TOPK_CAND_MAX:
        if route in _SAD_FILTERS:
            f = _SAD_FILTERS[route]
            if q_set is not None or g_set is not None:
                raise TypeError(f'pairwise_topk: a RowSet is packed for the Euclidean filter; filter="{route}" takes '
                                f"{f.set_words}")
            q_l1, g_l1 = _l1_sets(q, g, q_l1, g_l1, f.set_now())
            filtered = lambda: globals()[f.topk](q_l1, g_l1, alpha, beta, k, cand_cap, sample_rows, ws)  # noqa: E731
        elif route == "l2":
            if q_l1 is not None or g_l1 is not None:
                raise TypeError('pairwise_topk: an L1Set is packed for filter="l1"; the Euclidean filter takes a RowSet')
            if g_set is None:
                g_set = RowSet(g, with_lo=False, device=g.device)
            if q_set is None:
                q_set = RowSet(q, with_lo=False, device=g.device)
            filtered = lambda: l2_topk(q_set, g_set, alpha, beta, k, cand_cap, sample_rows, ws)  # noqa: E731
        else:
            raise AssertionError(f"pairwise_topk: no top-k behind the route {route!r}")
        idx, err, topk_stats = _topk_filtered(metric, filtered, q, g, alpha, beta, k, score_dtype)
        if idx is not None:
            return result(idx, err, topk_stats)
    lo, rec = pairwise_topk_workspace(n_q, n_g, k, metric)
    if ws is None or (topk_stats is not None and _nbytes(ws) < lo):
        ws = torch.empty(max(rec if ws_bytes is None else int(ws_bytes), 8), dtype=torch.uint8, device=q.device)
    if _nbytes(ws) < lo:
        raise ValueError(f"pairwise_topk: workspace of {_nbytes(ws)} bytes < minimum {lo}")
    idx = torch.empty((n_q, k), dtype=torch.int64, device=q.device)
    err = torch.empty((n_q, k), dtype=torch.float64, device=q.device)
    check(lib.cmve_pairwise_topk(handle(q.device), _ptr(q), _dtype_code(q), _pw_ld(q), n_q, _ptr(g), _dtype_code(g),
                                 _pw_ld(g), n_g, q.shape[1], metric, float(alpha), float(beta),
                                 _pw_code(score_dtype), k, int(geometry), _ptr(ws), _nbytes(ws), _ptr(idx), _ptr(err)),
          "cmve_pairwise_topk")
    return result(idx, err, topk_stats)


def csr(lists: Sequence[Sequence[int]], device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Python GT lists -> (offsets int64 [n+1], indices int32) device tensors."""
    lens = np.fromiter((len(l) for l in lists), dtype=np.int64, count=len(lists))
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    idx = np.fromiter((int(v) for l in lists for v in l), dtype=np.int32, count=int(off[-1]))
    if idx.size == 0:
        idx = np.zeros(1, np.int32)
    return (torch.from_numpy(off).to(device), torch.from_numpy(idx).to(device))


def gt_thresholds(a: RowSet, b: RowSet, off: torch.Tensor, idx: torch.Tensor, mode: int):
    sgt = torch.empty(a.n_pad, dtype=torch.float64, device=a.device)
    hi = torch.empty(a.n_pad, dtype=torch.float32, device=a.device)
    lo = torch.empty(a.n_pad, dtype=torch.float32, device=a.device)
    check(lib.cmve_gt_thresholds(handle(a.device), C.byref(a.desc), C.byref(b.desc), mode, _ptr(off), _ptr(idx),
                                 _ptr(sgt), _ptr(hi), _ptr(lo)), "cmve_gt_thresholds")
    return sgt, hi, lo


class RankWorkspace:
    """Reusable device buffers for rank_count: the undecided-pair list (grown on overflow) and
    one int64 pair counter per gallery chunk (cmve_rank_count_overlap)."""

    def __init__(self, device, cap: int = 1 << 20):
        self.device = device
        self.cand = torch.empty(max(cap, 1), dtype=torch.int64, device=device)
        self.count = torch.zeros(_lib.MAX_CHUNKS, dtype=torch.int64, device=device)
        self.chunks = 1

    @property
    def cap(self):
        return self.cand.numel()

    def ncand(self) -> int:
        """Undecided pairs of the last launch (synchronises)."""
        return int(self.count[:self.chunks].sum().item())

    def overflowed(self) -> bool:
        """True if a chunk's list outgrew its share of the buffer (counts incomplete)."""
        return bool((self.count[:self.chunks] > self.cap // self.chunks).any().item())

    def grow(self, need: int = 0):
        need = max(need, self.ncand())
        self.cand = torch.empty(int(need * 1.25) * self.chunks + 1024 * self.chunks, dtype=torch.int64,
                                device=self.device)


def rank_thresholds(a: RowSet, b: RowSet, sgt: torch.Tensor, mode: int):
    """fp32 bracketing thresholds for given exact GT scores sgt[a.n_pad] (NaN = no GT)."""
    hi = torch.empty(a.n_pad, dtype=torch.float32, device=a.device)
    lo = torch.empty(a.n_pad, dtype=torch.float32, device=a.device)
    check(lib.cmve_rank_thresholds(handle(a.device), C.byref(a.desc), C.byref(b.desc), mode, _ptr(sgt), _ptr(hi),
                                   _ptr(lo)), "cmve_rank_thresholds")
    return hi, lo


def rank_count_launch(q: RowSet, g: RowSet, mode: int, row=None, col=None, ws: Optional[RankWorkspace] = None,
                      row_cnt=None, col_cnt=None, events=None, chunks: int = 1):
    """Enqueue the fused rank count (no sync).  row/col = (sgt, thr_hi, thr_lo) or None.
    chunks > 1: cmve_rank_count_overlap -- the gallery in `chunks` pieces, each piece's fp64
    fix-up on the handle's auxiliary stream behind the next piece's MFMA pass.
    events = (start, mid, end) torch.cuda.Event triple recorded around the MFMA pass and the
    fix-up (with chunks > 1 the two overlap: mid is recorded with end)."""
    dirs = (_lib.DIR_ROW if row is not None else 0) | (_lib.DIR_COL if col is not None else 0)
    if row is not None and row_cnt is None:
        row_cnt = torch.empty(q.n_pad, dtype=torch.int32, device=q.device)
    if col is not None and col_cnt is None:
        col_cnt = torch.empty(g.n_pad, dtype=torch.int32, device=q.device)
    r = row if row is not None else (None, None, None)
    c = col if col is not None else (None, None, None)
    h = handle(q.device)
    chunks = max(1, min(int(chunks), _lib.MAX_CHUNKS))
    ws.chunks = chunks
    if events is not None:
        events[0].record()
    if chunks > 1:
        check(lib.cmve_rank_count_overlap(h, C.byref(q.desc), C.byref(g.desc), mode, dirs, _ptr(r[0]), _ptr(r[1]),
                                          _ptr(r[2]), _ptr(c[0]), _ptr(c[1]), _ptr(c[2]), _ptr(row_cnt),
                                          _ptr(col_cnt), _ptr(ws.cand), ws.cap, _ptr(ws.count), chunks),
              "cmve_rank_count_overlap")
        if events is not None:
            events[1].record()
            events[2].record()
        return row_cnt, col_cnt
    check(lib.cmve_rank_mfma(h, C.byref(q.desc), C.byref(g.desc), mode, dirs, _ptr(r[1]), _ptr(r[2]), _ptr(c[1]),
                             _ptr(c[2]), _ptr(row_cnt), _ptr(col_cnt), _ptr(ws.cand), ws.cap, _ptr(ws.count)),
          "cmve_rank_mfma")
    if events is not None:
        events[1].record()
    check(lib.cmve_rank_fixup(h, C.byref(q.desc), C.byref(g.desc), dirs, _ptr(r[0]), _ptr(c[0]), _ptr(row_cnt),
                              _ptr(col_cnt), _ptr(ws.cand), ws.cap, _ptr(ws.count)), "cmve_rank_fixup")
    if events is not None:
        events[2].record()
    return row_cnt, col_cnt


def gt_rank_counts(q: RowSet, g: RowSet, row_gts=None, col_gts=None, mode: int = _lib.SIM_F16,
                   ws: Optional[RankWorkspace] = None, chunks: int = 1):
    """Exact GT ranks in both directions from ONE fused GEMM pass.

    row_gts[i]: GT indices into g for query row i (t2v); col_gts[j]: GT indices into q
    for gallery row j (v2t).  Returns (row_ranks, col_ranks, n_candidates) as numpy int64,
    1-based; empty GT lists give n_other + 1 (``LINAS-engine/util/metrics.py:140``).
    """
    if row_gts is None and col_gts is None:
        raise ValueError("gt_rank_counts: need row_gts and/or col_gts")
    if mode == _lib.SIM_BF16X3 and not (q.has_lo and g.has_lo):
        raise ValueError("BF16X3 needs lo planes")
    if mode == _lib.SIM_F16 and not (q.has_f16 and g.has_f16):
        mode = _lib.SIM_BF16
    ws = ws or RankWorkspace(q.device, cap=max(1 << 16, 64 * (q.n + g.n)))
    row = col = None
    if row_gts is not None:
        roff, ridx = csr(row_gts, q.device)
        row = gt_thresholds(q, g, roff, ridx, mode)
    if col_gts is not None:
        coff, cidx = csr(col_gts, q.device)
        col = gt_thresholds(g, q, coff, cidx, mode)
    for _attempt in range(4):
        rc, cc = rank_count_launch(q, g, mode, row, col, ws, chunks=chunks)
        ncand = ws.ncand()  # synchronises
        if not ws.overflowed():
            break
        ws.grow(ncand)
    else:
        raise _lib.CmveError("rank_count: candidate list kept overflowing")
    out_r = gt_ranks(rc, row[0], q.n, g.n).cpu().numpy() if row_gts is not None else None
    out_c = gt_ranks(cc, col[0], g.n, q.n).cpu().numpy() if col_gts is not None else None
    return out_r, out_c, ncand


def gt_ranks(cnt: torch.Tensor, sgt: torch.Tensor, n: int, n_m: int, out: Optional[torch.Tensor] = None,
             recall: Optional[torch.Tensor] = None) -> torch.Tensor:
    """1-based ranks int64 [n] on the device from better-than-GT counts and GT scores (cmve_gt_ranks):
    empty GT list (sgt NaN) -> n_m + 1, every GT NaN (sgt +inf) -> n_m, else count + 1
    (``LINAS-engine/util/metrics.py:137-147``).  recall: optional int64 [4] device output
    (#rank<=1, #rank<=5, #rank<=10, sum of ranks)."""
    if out is None:
        out = torch.empty(max(n, 1), dtype=torch.int64, device=cnt.device)
    check(lib.cmve_gt_ranks(handle(cnt.device), _ptr(cnt), _ptr(sgt), n, n_m, _ptr(out), _ptr(recall)),
          "cmve_gt_ranks")
    return out[:n]


class RankSession:
    """Resident exact GT-rank evaluation of a fixed problem (the reference re-runs
    ``encode_* -> cal_error -> cal_perf`` on new embeddings of the same sets every validation,
    ``LINAS-engine/validate.py:61-74``): the packed planes of both sets, the GT lists, thresholds,
    counts and the undecided-pair list are allocated once, and one evaluation is FOUR launches on
    the session's stream (``cmve_eval_ranks``, K14): pack both sets + exact GT scores, the fused rank
    GEMM (thresholds derived in-kernel), the fp64 fix-up, ranks + R@K sums.
    ``run(captions, videos)`` returns (t2v ranks, v2t ranks) exactly as ``gt_rank_counts`` does.
    Device tensors of the session's dtype are read in place (no copy); anything else is copied into
    the session's own buffers first.  An undecided-pair overflow grows the list and redoes the run.
    ``enqueue`` + ``stats`` is the non-blocking form (R@K sums / overflow on the device)."""

    def __init__(self, n_q: int, n_g: int, d: int, row_gts=None, col_gts=None, dtype=torch.float32,
                 mode: int = _lib.SIM_F16, eps: float = 0.0, device: Optional[torch.device] = None,
                 cand_cap: Optional[int] = None, stream: Optional["torch.cuda.Stream"] = None):
        if row_gts is None and col_gts is None:
            raise ValueError("RankSession: need row_gts and/or col_gts")
        if n_q < 1 or n_g < 1:
            raise ValueError("RankSession: both sets need rows")
        self.device = device or default_device()
        dev = self.device
        self.mode, self.dtype = mode, dtype
        self.q = RowSet(torch.zeros((n_q, d), dtype=dtype, device=dev), eps=eps, with_lo=(mode == _lib.SIM_BF16X3),
                        with_f16=(mode == _lib.SIM_F16), device=dev)
        self.g = RowSet(torch.zeros((n_g, d), dtype=dtype, device=dev), eps=eps, with_lo=(mode == _lib.SIM_BF16X3),
                        with_f16=(mode == _lib.SIM_F16), device=dev)
        self.row = csr(row_gts, dev) if row_gts is not None else None
        self.col = csr(col_gts, dev) if col_gts is not None else None
        # a one-to-one GT pairing (MSR-VTT-1kA: caption i <-> video p(i)) lets the evaluation's prep pack and
        # score each (caption, video) pair in one wave (CMVE_EVAL_PAIRED)
        self.paired = self._is_pairing(row_gts, col_gts, n_q, n_g)
        self._alloc(int(cand_cap) if cand_cap else max(1 << 16, 64 * (n_q + n_g)))
        self.out = torch.zeros(_lib.EVAL_OUT_HEAD + n_q + n_g, dtype=torch.int64, device=dev)
        self.host = torch.zeros(_lib.EVAL_OUT_HEAD + n_q + n_g, dtype=torch.int64).pin_memory()
        self._bound = (None, None)
        # stream: the session's own HIP stream (every launch and copy of the session goes there, with no
        # current-stream switch per evaluation: ~6 us of host time each); None = the caller's current stream
        self.stream = stream
        self._h = stream_handle(dev, stream) if stream is not None else None

    @staticmethod
    def _is_pairing(row_gts, col_gts, n_q, n_g) -> bool:
        if row_gts is None or col_gts is None or n_q != n_g:
            return False
        rows = [row_gts[i] for i in range(n_q)]
        cols = [col_gts[j] for j in range(n_g)]
        if any(len(l) != 1 for l in rows) or any(len(l) != 1 for l in cols):
            return False
        return all(0 <= int(rows[i][0]) < n_g and int(cols[int(rows[i][0])][0]) == i for i in range(n_q))

    def _ctx(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _alloc(self, cap: int):
        nbytes = C.c_int64()
        check(lib.cmve_eval_workspace(C.byref(self.q.desc), C.byref(self.g.desc), int(cap), C.byref(nbytes)),
              "cmve_eval_workspace")
        self.ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=self.device)  # zeroed once (ABI contract)
        self.cap = int(cap)
        self._args = None
        # captured graphs bake the workspace address in: a new workspace makes them stale (EvalGraph.launch
        # refuses them), and each graph keeps the workspace it was captured with alive
        self._ws_gen = getattr(self, "_ws_gen", -1) + 1

    @property
    def ncand(self) -> int:
        """Undecided pairs of the last evaluation written into ``self.out`` (synchronises)."""
        return int(self.out[8].item())

    def _bind(self, rs: RowSet, x):
        """Point the packed set's raw rows at x (a device tensor of the session dtype, rows contiguous),
        or copy x into the set's own buffer."""
        if (torch.is_tensor(x) and x.device == self.device and x.dtype == self.dtype and x.dim() == 2
                and tuple(x.shape) == tuple(rs.raw.shape) and x.stride(1) == 1 and x.stride(0) >= x.shape[1]):
            src = x
        else:
            src_t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            if tuple(src_t.shape) != tuple(rs.raw.shape):
                raise ValueError(f"RankSession: expected {tuple(rs.raw.shape)}, got {tuple(src_t.shape)}")
            rs.raw.copy_(src_t, non_blocking=True)
            src = rs.raw
        rs.desc.raw = src.data_ptr()
        rs.desc.raw_ld = _pw_ld(src)
        return src

    def enqueue(self, captions, videos, timing_slot: int = -1, out: Optional[torch.Tensor] = None,
                _bind_only: bool = False, wait_current: bool = True):
        """Enqueue one evaluation (no host synchronisation) on the session's stream, or on the current
        stream without one.  The inputs must stay unmodified until it completes.  With a session stream the
        evaluation first waits for the work already enqueued on the caller's current stream (the producer of
        the embeddings, e.g. an encoder), and inputs read in place are recorded on the session stream for
        the caching allocator; ``wait_current=False`` skips the wait for callers whose inputs are known to
        be complete (a resident buffer the caller synchronised once).  out: optional int64 device tensor of
        ``EVAL_OUT_HEAD + n_q + n_g`` words receiving this evaluation's head + ranks instead of
        ``self.out`` (a ring of them lets pipelined evaluations be read back in batches)."""
        if out is None:
            out = self.out
        elif (out.dtype != torch.int64 or out.device != self.out.device or not out.is_contiguous()
              or out.numel() < self.out.numel()):
            raise ValueError(f"RankSession.enqueue: out must be a contiguous int64 {self.out.device} tensor of "
                             f">= {self.out.numel()} words")
        if not (self._bound[0] is captions and self._bound[1] is videos and self._args is not None
                and captions.data_ptr() == self.q.desc.raw and videos.data_ptr() == self.g.desc.raw):
            # (re)bind: the same input tensors again (a resident buffer refilled between evaluations)
            # reuse the bound descriptors and the prepared argument tuple -- the host side of an
            # evaluation is then one ctypes call
            if self.stream is not None and wait_current:
                self._order_after_current()
                wait_current = False
            with self._ctx():  # a copying bind goes on the session's stream
                self._bound = (self._bind(self.q, captions), self._bind(self.g, videos))
            if self.stream is not None:  # read in place on another stream: keep the allocator from reusing them early
                for x, b in zip((captions, videos), self._bound):
                    if torch.is_tensor(x) and b is x:
                        x.record_stream(self.stream)
            if self._bound[0] is not captions or self._bound[1] is not videos:
                self._bound = (None, None)  # copied into the session's own buffers: rebind next time
            r = self.row if self.row is not None else (None, None)
            c = self.col if self.col is not None else (None, None)
            mode = self.mode | (_lib.EVAL_PAIRED if self.paired else 0)
            self._args = (C.byref(self.q.desc), C.byref(self.g.desc), mode, _ptr(r[0]), _ptr(r[1]), _ptr(c[0]),
                          _ptr(c[1]), _ptr(self.ws), self.ws.numel(), self.cap)
        if _bind_only:
            return
        if self.stream is not None and wait_current:
            self._order_after_current()
        h = self._h if self._h is not None else handle(self.device)
        check(lib.cmve_eval_ranks(h, *self._args, _ptr(out), int(timing_slot)), "cmve_eval_ranks")

    def _order_after_current(self):
        """The session stream waits for the work enqueued so far on the caller's current stream."""
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.stream.cuda_stream:
            self.stream.wait_stream(cur)

    def graph(self, captions, videos, out: Optional[torch.Tensor] = None) -> "EvalGraph":
        """One evaluation of these inputs into `out` (default self.out) captured into a HIP graph on the
        session's stream (cmve_eval_graph_create): ``launch()`` replays it with one host call, same results
        bit for bit.  Every address is baked in: the inputs must be device tensors of the session dtype read
        in place (refill them between launches), and `out` stays where it is."""
        for x in (captions, videos):
            if not (torch.is_tensor(x) and x.device == self.device and x.dtype == self.dtype):
                raise ValueError("RankSession.graph: inputs must be device tensors of the session dtype")
        self.enqueue(captions, videos, out=out, _bind_only=True)
        if self._bound[0] is not captions or self._bound[1] is not videos:
            raise ValueError("RankSession.graph: inputs must be readable in place (rows contiguous)")
        out = self.out if out is None else out
        h = self._h if self._h is not None else handle(self.device)
        gh = C.c_void_p()
        check(lib.cmve_eval_graph_create(h, *self._args, _ptr(out), C.byref(gh)), "cmve_eval_graph_create")
        return EvalGraph(gh.value, h, (captions, videos, out, self, self.ws), self, self._ws_gen)

    def timing(self, slot: int):
        """(pack+thresholds, rank GEMM, fix-up+ranks) milliseconds of the evaluation that used `slot`."""
        ms = (C.c_float * 3)()
        h = self._h if self._h is not None else handle(self.device)
        check(lib.cmve_eval_timing(h, int(slot), ms), "cmve_eval_timing")
        return list(ms)

    def kernel_timing(self, slot: int):
        """(prep, rank GEMM, fix-up, finish) kernel durations in ms of the evaluation that used `slot`, each
        from its launch's own start / stop (the durations rocprofv3 reports)."""
        ms = (C.c_float * 4)()
        h = self._h if self._h is not None else handle(self.device)
        check(lib.cmve_eval_kernel_timing(h, int(slot), ms), "cmve_eval_kernel_timing")
        return list(ms)

    def run(self, captions, videos):
        """Exact 1-based (t2v ranks, v2t ranks) of new caption / video embeddings (numpy or torch)."""
        for _attempt in range(4):
            self.enqueue(captions, videos)
            with self._ctx():
                self.host.copy_(self.out, non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
            need = int(self.host[9])
            if int(self.host[11]):  # (the paired prep's per-caption check of CMVE_EVAL_PAIRED)
                raise _lib.CmveError("RankSession: the GT lists are not a one-to-one pairing")
            if need == 0:
                break
            self._alloc(max(need, 2 * self.cap))  # a bucket overflowed: the counts are incomplete
        else:
            raise _lib.CmveError("RankSession: undecided-pair list kept overflowing")
        h = self.host.numpy()
        nq, ng, o = self.q.n, self.g.n, _lib.EVAL_OUT_HEAD
        t2v = h[o:o + nq].copy() if self.row is not None else None
        v2t = h[o + nq:o + nq + ng].copy() if self.col is not None else None
        return t2v, v2t


class RankBatch:
    """A batch of same-shaped RankSession evaluations (cmve_eval_batch_*: one prep, one rank GEMM and one
    finish launch over all of them).  ``sessions`` share sizes, dtype, mode and GT lists (each keeps its own
    packed sets, workspace and output); ``inputs`` holds one (captions, videos) pair of device tensors of the
    session dtype per session, read in place (refill them between runs: every address is baked in, as for
    RankSession.graph); ``outs`` optionally one int64 output per session (default each session's ``out``).
    ``run()`` enqueues the batch on ``stream`` (default the current stream); the results equal each session's
    own ``enqueue`` bit for bit.  Sizes must take the G64 rank geometry (e.g. MSR-VTT-1kA's 1,000 x 1,000)."""

    def __init__(self, sessions, inputs, outs=None, stream: Optional["torch.cuda.Stream"] = None):
        sessions = list(sessions)
        if not sessions or len(inputs) != len(sessions):
            raise ValueError("RankBatch: one (captions, videos) input pair per session")
        s0 = sessions[0]
        for s in sessions[1:]:
            same_lists = all((a is None) == (b is None) and (a is None or all(torch.equal(x, y) for x, y in zip(a, b)))
                             for a, b in ((s0.row, s.row), (s0.col, s.col)))
            if (s.q.n, s.g.n, s.q.d, s.dtype, s.mode, s.paired) != (s0.q.n, s0.g.n, s0.q.d, s0.dtype, s0.mode,
                                                                   s0.paired) or not same_lists:
                raise ValueError("RankBatch: sessions must share sizes, dtype, mode and GT lists")
        # one undecided-pair capacity for the whole batch (the C table holds one cand_cap and workspace size): a
        # session whose list was grown sets it, the others are grown to it here, before any input is bound
        cap = max(s.cap for s in sessions)
        for s in sessions:
            if s.cap != cap:
                s._alloc(cap)
        outs = [s.out for s in sessions] if outs is None else list(outs)
        for s, o in zip(sessions, outs):
            if o.dtype != torch.int64 or not o.is_contiguous() or o.numel() < s.out.numel():
                raise ValueError("RankBatch: outs must be contiguous int64 tensors of EVAL_OUT_HEAD + n_q + n_g words")
        for s, (c, v) in zip(sessions, inputs):
            for x in (c, v):
                if not (torch.is_tensor(x) and x.device == s.device and x.dtype == s.dtype):
                    raise ValueError("RankBatch: inputs must be device tensors of the session dtype")
            s.enqueue(c, v, _bind_only=True)
            if s._bound[0] is not c or s._bound[1] is not v:
                raise ValueError("RankBatch: inputs must be readable in place (rows contiguous)")
        n = len(sessions)
        self._q = (C.POINTER(Rows) * n)(*[C.pointer(s.q.desc) for s in sessions])
        self._g = (C.POINTER(Rows) * n)(*[C.pointer(s.g.desc) for s in sessions])
        self._ws = (C.c_void_p * n)(*[s.ws.data_ptr() for s in sessions])
        self._out = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        ws_bytes = sessions[0].ws.numel()
        if any(s.cap != cap or s.ws.numel() != ws_bytes for s in sessions):
            raise ValueError("RankBatch: sessions must share one undecided-pair capacity and workspace size")
        r = s0.row if s0.row is not None else (None, None)
        c = s0.col if s0.col is not None else (None, None)
        mode = s0.mode | (_lib.EVAL_PAIRED if s0.paired else 0)
        bh = C.c_void_p()
        check(lib.cmve_eval_batch_create(n, self._q, self._g, mode, _ptr(r[0]), _ptr(r[1]), _ptr(c[0]), _ptr(c[1]),
                                         self._ws, ws_bytes, cap, self._out, C.byref(bh)), "cmve_eval_batch_create")
        self._b = bh.value
        self._keep = (sessions, [tuple(x) for x in inputs], outs)  # everything the table points at stays alive
        self._ws_gens = [s._ws_gen for s in sessions]
        self.sessions, self.outs, self.stream = sessions, outs, stream
        self._h = stream_handle(s0.device, stream) if stream is not None else None

    def run(self, timing_slot: int = -1, wait_current: bool = True):
        """Enqueue the batch; ``timing_slot`` >= 0 records its launches' durations in that slot of the stream
        handle's timing ring (``kernel_timing``).  With a batch stream the run first waits for the work already
        enqueued on the caller's current stream (the producer that refilled the inputs, as RankSession.enqueue
        does); ``wait_current=False`` skips that for inputs known to be complete."""
        if not self._b:
            raise RuntimeError("RankBatch.run: the batch was closed")
        if any(s._ws_gen != g for s, g in zip(self.sessions, self._ws_gens)):
            raise RuntimeError("RankBatch.run: a session's workspace was regrown after the batch was built")
        if self.stream is not None and wait_current:
            cur = torch.cuda.current_stream(self.sessions[0].device)
            if cur.cuda_stream != self.stream.cuda_stream:
                self.stream.wait_stream(cur)
        h = self._h if self._h is not None else handle(self.sessions[0].device)
        check(lib.cmve_eval_batch_run(h, self._b, int(timing_slot)), "cmve_eval_batch_run")

    def run_chained(self, prev: Optional["RankBatch"] = None, timing_slot: int = -1, wait_current: bool = True):
        """Enqueue the batch with its finish (the words of its outputs: ranks, R@K) deferred to the next chained run on
        the same stream, whose first launch holds it beside that run's prep (``cmve_eval_batch_run_chained``); ``prev``
        is the batch chained before this one on the stream (its outputs are complete once this run's first launch
        has run), None for the first.  After a stream's last chained run call ``finish()``.  ``prev`` must share no
        session with this batch."""
        if not self._b or (prev is not None and not prev._b):
            raise RuntimeError("RankBatch.run_chained: a batch was closed")
        if any(s._ws_gen != g for s, g in zip(self.sessions, self._ws_gens)):
            raise RuntimeError("RankBatch.run_chained: a session's workspace was regrown after the batch was built")
        if self.stream is not None and wait_current:
            cur = torch.cuda.current_stream(self.sessions[0].device)
            if cur.cuda_stream != self.stream.cuda_stream:
                self.stream.wait_stream(cur)
        h = self._h if self._h is not None else handle(self.sessions[0].device)
        check(lib.cmve_eval_batch_run_chained(h, self._b, prev._b if prev is not None else None, int(timing_slot)),
              "cmve_eval_batch_run_chained")

    def finish(self):
        """The deferred finish of this batch's last chained run, alone (``cmve_eval_batch_finish``)."""
        if not self._b:
            raise RuntimeError("RankBatch.finish: the batch was closed")
        h = self._h if self._h is not None else handle(self.sessions[0].device)
        check(lib.cmve_eval_batch_finish(h, self._b), "cmve_eval_batch_finish")

    def kernel_timing(self, slot: int):
        """(prep, rank GEMM, 0, finish) durations in ms of the batch run that used `slot` (each launch's own
        start / stop: the whole batch's launches; a chained run: the prep launch holds the previous batch's finish,
        and finish is 0)."""
        ms = (C.c_float * 4)()
        h = self._h if self._h is not None else handle(self.sessions[0].device)
        check(lib.cmve_eval_kernel_timing(h, int(slot), ms), "cmve_eval_kernel_timing")
        return list(ms)

    def close(self):
        if self._b:
            if not _EXITING:  # (past interpreter exit the HIP runtime may be gone: the process releases the table)
                lib.cmve_eval_batch_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter teardown)
            pass


class EvalGraph:
    """A captured RankSession evaluation (cmve_eval_graph_*): ``launch()`` enqueues it on the session's
    stream with one host call.  Keeps its inputs, output and session alive."""

    def __init__(self, gh: int, h: int, keep, session: Optional["RankSession"] = None, ws_gen: int = 0):
        self._g, self._h, self._keep = gh, h, keep  # keep: inputs, output, session and the captured workspace
        self._session, self._ws_gen = session, ws_gen

    @property
    def stale(self) -> bool:
        """True once the session replaced its workspace (an overflow in run()): the graph's baked-in
        undecided-pair list is no longer the session's, and its capacity is the one that overflowed."""
        return self._session is not None and self._session._ws_gen != self._ws_gen

    def launch(self):
        if not self._g:
            raise RuntimeError("EvalGraph.launch: the graph was closed")
        if self.stale:
            raise RuntimeError("EvalGraph.launch: the session's workspace was regrown after this graph was "
                               "captured; capture a new graph (RankSession.graph)")
        check(lib.cmve_eval_graph_launch(self._h, self._g), "cmve_eval_graph_launch")

    def close(self):
        if self._g:
            if not _EXITING:
                lib.cmve_eval_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


def rank_from_matrix(errors, gts, transposed: bool = False, device=None) -> np.ndarray:
    """1-based GT ranks from a materialised error matrix (lower = better), on device."""
    device = device or default_device()
    e = to_device(errors, device)
    n_rows, n_cols = e.shape
    n_q = n_cols if transposed else n_rows
    lists = [gts[i] if (not isinstance(gts, dict) or i in gts) else [] for i in range(n_q)]
    off, idx = csr(lists, device)
    cnt = torch.zeros(n_q, dtype=torch.int32, device=device)
    check(lib.cmve_rank_from_matrix(handle(device), _ptr(e), _dtype_code(e), n_rows, n_cols, e.stride(0),
                                    1 if transposed else 0, _ptr(off), _ptr(idx), _ptr(cnt)),
          "cmve_rank_from_matrix")
    ranks = cnt.to(torch.int64).cpu().numpy() + 1
    n_m = n_rows if transposed else n_cols
    empty = np.fromiter((len(l) == 0 for l in lists), bool, count=n_q)
    ranks[empty] = n_m + 1
    return ranks


def topk_workspace_floats(q: RowSet, g: RowSet, k: int) -> int:
    """Floats of device workspace cmve_topk needs for this query set / gallery / k."""
    n = C.c_int64()
    check(lib.cmve_topk_workspace(C.byref(q.desc), C.byref(g.desc), int(k), C.byref(n)), "cmve_topk_workspace")
    return n.value


TOPK_BATCH_MIN_Q = 512   # below this the dense score block is small: cmve_topk
TOPK_BATCH_MAX_K = 32     # cmve_topk_batch's limit (its sample is ~k/128 of the gallery)


def topk_batch_plan(q: RowSet, g: RowSet, k: int):
    """(use_batch, sample_rows, workspace_floats) of cmve_topk_batch for this problem: the fused
    path pays off when the sample it scores densely is at most a quarter of the gallery."""
    if q.n < TOPK_BATCH_MIN_Q or not 1 <= k <= TOPK_BATCH_MAX_K or g.n >= (1 << 24):
        return False, 0, 0
    ns, nf = C.c_int64(), C.c_int64()
    check(lib.cmve_topk_batch_workspace(C.byref(q.desc), C.byref(g.desc), int(k), C.byref(ns), C.byref(nf)),
          "cmve_topk_batch_workspace")
    return 4 * ns.value <= g.n, ns.value, nf.value


def topk_batch(q: RowSet, g: RowSet, k: int, mode: int = _lib.SIM_F16, ws: Optional[torch.Tensor] = None):
    """cmve_topk_batch on device: (idx int32 [n, k], fp64 scores [n, k], unresolved int32 [1]).
    Rows left unresolved hold idx -2 (topk() finishes them through cmve_topk)."""
    ok, _, need = topk_batch_plan(q, g, k)
    if not ok:
        raise ValueError("topk_batch: problem outside the batch path (see topk_batch_plan)")
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=q.device)
    idx = torch.empty((q.n, k), dtype=torch.int32, device=q.device)
    sc = torch.empty((q.n, k), dtype=torch.float64, device=q.device)
    unres = torch.zeros(1, dtype=torch.int32, device=q.device)
    check(lib.cmve_topk_batch(handle(q.device), C.byref(q.desc), C.byref(g.desc), int(mode), int(k), _ptr(ws),
                              ws.numel(), _ptr(idx), _ptr(sc), _ptr(unres)), "cmve_topk_batch")
    return idx, sc, unres


def topk(q: RowSet, g: RowSet, k: int, mode: int = _lib.SIM_F16, scores_ws: Optional[torch.Tensor] = None,
         to_host: bool = True, batch: Optional[bool] = None, out=None):
    """Exact top-k gallery indices per query (score desc, index asc) + their fp64 cosines.
    to_host=False returns the device tensors (int32 idx, fp64 scores) instead of numpy arrays.
    Large query batches go through cmve_topk_batch (no score matrix; batch=False forces the
    dense path); rows it leaves unresolved are finished by cmve_topk."""
    k = int(min(k, g.n))
    if k < 1:
        return np.zeros((q.n, 0), np.int64), np.zeros((q.n, 0))
    if k > _lib.TOPK_MAX:
        raise ValueError(f"topk: k <= {_lib.TOPK_MAX}")
    if mode == _lib.SIM_F16 and not (q.has_f16 and g.has_f16):
        mode = _lib.SIM_BF16
    use_batch = topk_batch_plan(q, g, k)[0] if batch is None else bool(batch)
    if use_batch:
        idx, sc, unres = topk_batch(q, g, k, mode, ws=scores_ws)
        if int(unres.item()):
            rows = torch.nonzero(idx[:, 0] == -2).flatten()
            sub = RowSet(q.raw.index_select(0, rows), eps=q.eps, with_lo=q.has_lo, device=q.device,
                         with_f16=q.has_f16)
            i2, s2 = topk(sub, g, k, mode, to_host=False, batch=False)
            idx[rows] = i2
            sc[rows] = s2
        if not to_host:
            return idx, sc
        return idx.to(torch.int64).cpu().numpy(), sc.cpu().numpy()
    need = topk_workspace_floats(q, g, k)
    if scores_ws is None or scores_ws.numel() < need:
        scores_ws = torch.empty(need, dtype=torch.float32, device=q.device)
    if out is not None:  # caller-held (idx int32, scores fp64 [max(n, 1), k], overflow int32 [1]) buffers
        idx, sc, ovf = out
    else:
        idx = torch.empty((max(q.n, 1), k), dtype=torch.int32, device=q.device)
        sc = torch.empty((max(q.n, 1), k), dtype=torch.float64, device=q.device)
        ovf = torch.zeros(1, dtype=torch.int32, device=q.device)
    if mode == _lib.SIM_F16 and not (q.has_f16 and g.has_f16):
        mode = _lib.SIM_BF16
    for m in ((mode, _lib.SIM_BF16X3) if (mode != _lib.SIM_BF16X3 and q.has_lo and g.has_lo) else (mode,)):
        check(lib.cmve_topk(handle(q.device), C.byref(q.desc), C.byref(g.desc), m, k, _ptr(scores_ws),
                            scores_ws.numel(), _ptr(idx), _ptr(sc), _ptr(ovf)), "cmve_topk")
        if int(ovf.item()) == 0:
            break
    else:  # a query's error band held > TOPK_CAP columns (near-duplicate gallery rows at the k-th score)
        idx, sc = _topk_dense_exact(q, g, k)
        if not to_host:
            return idx, sc
        return idx.to(torch.int64).cpu().numpy(), sc.cpu().numpy()
    if not to_host:
        return idx[:q.n], sc[:q.n]
    return idx[:q.n].to(torch.int64).cpu().numpy(), sc[:q.n].cpu().numpy()


def _topk_dense_exact(q: RowSet, g: RowSet, k: int, gallery_chunk: int = 1 << 16):
    """Exact top-k by dense fp64 scoring (the fallback of topk when an error band overflows): the
    normalised rows in fp64, gallery chunks scored by the K10 DOT kernel (a k-ordered fp64 fma chain
    per pair, so exact duplicates score identically -- a library dgemm rounds by tile position), each
    chunk merged with the running top-k by K12f (cmve_topk_dense_merge: radix select + bitonic sort on the
    device, score desc, index asc, NaN last as np.argsort of the errors)."""
    qn = q.normalized(torch.float64)
    gn_all = g.normalized(torch.float64)
    bufs = [(torch.empty((q.n, k), dtype=torch.float64, device=q.device),
             torch.empty((q.n, k), dtype=torch.int64, device=q.device)) for _ in range(2)]
    kb, cur = 0, 0
    for j0 in range(0, g.n, gallery_chunk):
        s = pairwise(qn, gn_all[j0:j0 + gallery_chunk].contiguous(), _lib.PW_DOT, 1.0, 0.0, torch.float64)
        (bs, bi), (os_, oi) = bufs[cur], bufs[1 - cur]
        check(lib.cmve_topk_dense_merge(handle(q.device), _ptr(bs), _ptr(bi), kb, _ptr(s), s.stride(0), q.n,
                                        s.shape[1], j0, k, _ptr(os_), _ptr(oi)), "cmve_topk_dense_merge")
        kb, cur = k, 1 - cur
    best_s, best_i = bufs[cur]
    return best_i.to(torch.int32), best_s


def gt_positions_fused(a: RowSet, b: RowSet, lists, mode: int = _lib.SIM_F16):
    """Exact 1-based position of EVERY GT item: for row i of `a` and k in lists[i],
    1 + #{j : cos64(a_i, b_j) > cos64(a_i, b_k)}.  Implemented as a fused rank count
    over an expanded query set (row i repeated once per GT item, GT list [k])."""
    owners = np.fromiter((i for i, l in enumerate(lists) for _ in l), dtype=np.int64)
    items = [[int(k)] for l in lists for k in l]
    out = [np.zeros(0, np.int64) for _ in lists]
    if owners.size == 0:
        return out
    sel = torch.from_numpy(owners).to(a.device)
    expanded = RowSet(a.raw.index_select(0, sel), eps=a.eps, with_lo=a.has_lo, device=a.device, with_f16=a.has_f16)
    r, _, _ = gt_rank_counts(expanded, b, row_gts=items, mode=mode)
    n_m = b.n
    p = 0
    for i, l in enumerate(lists):
        pi = r[p:p + len(l)].copy()
        # Items ranked individually: an all-NaN GT item gets n_m.  Several items at n_m are all NaN (a
        # finite item can only be last in a row without NaN), and NaN items share the row's last
        # positions n_m - n_nan + 1 .. n_m (AP depends only on the set of positions).
        last = np.flatnonzero(pi == n_m)
        if last.size > 1:
            pi[last] = n_m - last.size + 1 + np.arange(last.size)
        out[i] = pi
        p += len(l)
    return out



# ---- K26: exact positions of every listed item under cosine from ONE MFMA pass (csrc/cos_filter.hip) ----
def _cos_sets(a, b, name: str):
    if not (isinstance(a, RowSet) and isinstance(b, RowSet)):
        raise TypeError(f"{name}: both sides are RowSets (eps = 0, with their fp16 plane)")
    if a.d != b.d:
        raise ValueError(f"{name}: dimensions {a.d} and {b.d} do not match")
    if a.device != b.device:
        raise ValueError(f"{name}: the two sets live on different devices")


def cos_item_scores(a: RowSet, b: RowSet, off: torch.Tensor, idx: torch.Tensor, n_items: int, col_dir: bool = False,
                    out: Optional[torch.Tensor] = None, idx_base: Optional[int] = None) -> torch.Tensor:
    """fp64 [n_items] on the device: cos64 of every listed item of one CSR side (``cmve_cos_item_scores``) -- the word
    ``gt_thresholds`` and the rank fix-up compute.  (off, idx): ``csr`` of the lists of a's rows naming b's rows
    (col_dir: of b's rows naming a's rows).  An index outside the other set scores NaN.  No host copy, no
    synchronisation.  ``idx_base`` (an int, K27: ``cmve_cos_item_scores_sharded``, for a gallery sharded by rows): idx
    holds GLOBAL rows of the other side, of which the operand given here is [idx_base, idx_base + n); an item outside
    that range gets the all-zero word, not NaN: the int64 SUM over the shards of ``out.view(torch.int64)`` is every
    item's word, bit for bit."""
    _cos_sets(a, b, "cos_item_scores")
    n_items = int(n_items)
    if idx.numel() < n_items or idx.dtype != torch.int32 or off.dtype != torch.int64:
        raise ValueError(f"cos_item_scores: {n_items} items need int64 offsets and as many int32 indices")
    if out is None:
        out = torch.empty(max(n_items, 1), dtype=torch.float64, device=a.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() < n_items:
        raise TypeError("cos_item_scores: out is a contiguous float64 tensor of at least n_items words")
    head = (handle(a.device), C.byref(a.desc), C.byref(b.desc), _ptr(off), _ptr(idx), off.numel() - 1, n_items,
            1 if col_dir else 0)
    if idx_base is None:
        check(lib.cmve_cos_item_scores(*head, _ptr(out)), "cmve_cos_item_scores")
    else:
        check(lib.cmve_cos_item_scores_sharded(*head, int(idx_base), _ptr(out)), "cmve_cos_item_scores_sharded")
    return out[:n_items]


def cos_count_workspace(a: RowSet, b: RowSet, band_cap: int) -> int:
    """Bytes of workspace ``cmve_cos_count`` needs for a band list of ``band_cap`` pairs (host only: no launch)."""
    n = C.c_int64()
    check(lib.cmve_cos_count_workspace(C.byref(a.desc), C.byref(b.desc), int(band_cap), C.byref(n)),
          "cmve_cos_count_workspace")
    return n.value


def cos_count(a: RowSet, b: RowSet, row=None, col=None, band: Optional[torch.Tensor] = None,
              stats: Optional[torch.Tensor] = None, row_pos: Optional[torch.Tensor] = None,
              col_pos: Optional[torch.Tensor] = None, resolved: bool = False):
    """(row_pos, col_pos, stats): ``cmve_cos_count`` on device tensors, no host copy, no synchronisation.
    row = (off [na + 1], item words fp64 [items], n): a non-NaN item's word is #{ j : cos64(i, j) > word }, a NaN item's
    n - (NaN items of its list) + (its place among them); col: the mirror; a direction left None gives None.
    ``band``: a caller-owned contiguous int64 device tensor, one slot per element (None: ``l2_band_cap(na * nb)``
    slots).  ``stats``: int64 [4] on the device, {decided, band found, band re-scored, overflow}: when the overflow
    word is 1 the positions are NOT valid and ``stats[1]`` is the capacity a redo needs (``cos_gt_eval`` does that).
    ``resolved`` (K27: ``cmve_cos_count_resolved``): an overflow is resolved on the device -- the positions are those
    of a list large enough whatever the list did; the overflow word and ``stats[1]`` still say what a later call's
    list should hold."""
    _cos_sets(a, b, "cos_count")
    dev = a.device
    sides = []
    for side, n_lists, pos in ((row, a.n, row_pos), (col, b.n, col_pos)):
        if side is None:
            sides.append((None, None, 0, 0, None))
            continue
        off, sc, n = side
        if off.numel() != n_lists + 1:
            raise ValueError(f"cos_count: {off.numel() - 1} lists for {n_lists} rows")
        if sc.dtype != torch.float64 or not sc.is_contiguous():
            raise TypeError("cos_count: item words are contiguous float64")
        if pos is None:
            pos = torch.empty(max(sc.numel(), 1), dtype=torch.int32, device=dev)
        elif pos.dtype != torch.int32 or not pos.is_contiguous() or pos.numel() < sc.numel():
            raise TypeError("cos_count: positions are contiguous int32, one per item")
        sides.append((off, sc, sc.numel(), int(n), pos))
    if band is None:
        band = torch.empty(l2_band_cap(a.n * b.n), dtype=torch.int64, device=dev)
    elif band.dtype != torch.int64 or not band.is_contiguous() or band.device != dev:
        raise TypeError("cos_count: band is a contiguous int64 tensor on the sets' device")
    if stats is None:
        stats = torch.empty(4, dtype=torch.int64, device=dev)
    entry = "cmve_cos_count_resolved" if resolved else "cmve_cos_count"
    check(getattr(lib, entry)(handle(dev), C.byref(a.desc), C.byref(b.desc),
                              *_count_tail(sides[0], sides[1], band, _nbytes(band), stats)), entry)
    (_, _, ritems, _, rpos), (_, _, citems, _, cpos) = sides
    return (None if rpos is None else rpos[:ritems]), (None if cpos is None else cpos[:citems]), stats


def cos_gt_eval_flat(caps: RowSet, vids: RowSet, row_lists=None, col_lists=None, band_cap: Optional[int] = None):
    """``cos_gt_eval`` without the per-list arrays: per direction (offsets int64 [n + 1], 1-based positions int64
    [items] in list order, ranks int64 [n]) on the host, or None for a direction without lists."""
    _cos_sets(caps, vids, "cos_gt_eval")
    na, nb, dev = caps.n, vids.n, caps.device
    if row_lists is not None and len(row_lists) != na:
        raise ValueError(f"cos_gt_eval: {len(row_lists)} row lists for {na} rows")
    if col_lists is not None and len(col_lists) != nb:
        raise ValueError(f"cos_gt_eval: {len(col_lists)} column lists for {nb} rows")
    sides, total = [], 0
    for lists in (row_lists, col_lists):
        if lists is None:
            sides.append(None)
            continue
        off, idx = csr(lists, dev)
        items = sum(len(l) for l in lists)
        sides.append((off, idx, items, total))
        total += items
    buf = torch.empty(total + 4, dtype=torch.float64, device=dev)  # the items' words, then the four counters
    stats = buf[total:].view(torch.int64)
    args = []
    for side, col_dir, n_m in ((sides[0], False, nb), (sides[1], True, na)):
        if side is None:
            args.append(None)
            continue
        off, idx, items, start = side
        sc = buf[start:start + items]
        if items:
            cos_item_scores(caps, vids, off, idx, items, col_dir, out=sc)
        args.append((off, sc, n_m))
    cap = max(1, int(band_cap) if band_cap is not None else l2_band_cap(na * nb))
    for attempt in range(2):
        band = torch.empty(cap, dtype=torch.int64, device=dev)
        rpos, cpos, _ = cos_count(caps, vids, args[0], args[1], band, stats)
        st = _l2_count_stats(stats.cpu().numpy())
        cos_gt_eval.stats = dict(st, redone=attempt > 0)
        if not st["overflow"]:
            break
        cap = st["band"]
    else:
        raise _lib.CmveError("cos_gt_eval: the band list overflowed at the capacity the count itself reported")
    out = []
    for side, arg, pos in ((sides[0], args[0], rpos), (sides[1], args[1], cpos)):
        if side is None:
            out.append(None)
            continue
        ranks = pairwise_list_ranks(side[0], arg[1], pos, arg[2]).cpu().numpy()
        out.append((side[0].cpu().numpy(), pos.cpu().numpy().astype(np.int64) + 1, ranks))
    return out[0], out[1]


def cos_gt_eval(caps: RowSet, vids: RowSet, row_lists=None, col_lists=None, band_cap: Optional[int] = None):
    """((t2v positions, t2v ranks), (v2t positions, v2t ranks)) under cosine from ONE pass over the caps x vids pairs
    (K26), in ``pairwise_gt_eval``'s shapes: per direction the 1-based position of every listed item (a list of int64
    arrays aligned with the lists) and the 1-based best-GT rank of every list (``cmve_pairwise_list_ranks``); a
    direction without lists gives (None, None).  The words are ``gt_positions_fused``'s and ``gt_rank_counts``'s.
    row_lists[i]: rows of vids listed for caption i; col_lists[j]: rows of caps listed for video j.  A band list that
    overflows (``band_cap`` slots; None: ``l2_band_cap``) is redone once with the reported need.  The counters of the
    last count are left in ``cos_gt_eval.stats`` ({decided, band, rescored, overflow, redone})."""
    out = []
    for side in cos_gt_eval_flat(caps, vids, row_lists, col_lists, band_cap):
        if side is None:
            out.append((None, None))
            continue
        offs, p, ranks = side
        out.append(([p[offs[i]:offs[i + 1]] for i in range(offs.size - 1)], ranks))
    return out[0], out[1]


cos_gt_eval.stats = None
