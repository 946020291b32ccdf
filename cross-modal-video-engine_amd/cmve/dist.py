"""Gallery sharded across GPUs: one shard per rank, RCCL over xGMI.

Each rank keeps a contiguous shard of the video gallery resident in HBM (packed once).  One
exact two-direction evaluation of a caption batch (the reference's ``cal_perf`` over
``cal_error``, ``LINAS-engine/validate.py:15-54``, ``util/metrics.py:124-157``) is:
  1. all-gather of the caption embeddings (each rank contributes its slice);
  2. t2v GT scores: every rank scores the GTs that live in its shard (fp64), an all-reduce(MAX)
     gives each caption its best-GT score;
     v2t GT scores: a video's GT captions are all present after the gather, so they are local;
  3. ONE fused rank GEMM over (all captions) x (this shard): row counts (t2v, partial: this
     shard's videos) and column counts (v2t, complete: every caption) -- fp16 MFMA + fp64 fix-up;
  4. one all-reduce(SUM) carrying the t2v counts, this shard's v2t R@K sums and the
     undecided-pair overflow flag -> global t2v ranks on every rank, global v2t R@K sums.
     The v2t ranks themselves are rank-local (medr / mAP gather them once at the end).
The top-k path all-gathers each shard's exact local top-k (score, global id) and merges them
(score desc, global id asc) on the device (cmve_merge_topk).  The reference never shards
(SURVEY.md section 0.2).

``ShardedGallery(..., measure=)`` under euclidean / l1 / l2 / l1_norm / l2_norm / jaccard (evaluation.py:17-36): the
shard keeps its rows unnormalised in the measure's input dtype and K18's launches (csrc/pairwise_rank.hip) do the
arithmetic.  A position counts with a strict < and no index tie-break, so it is the plain sum over the shards of
their counts against the same item score:
  1. all-gather of the captions, as above;
  2. every rank builds the same CSR of all captions' GT videos (global ids) and scores the items whose video it
     holds (cmve_pairwise_item_scores, the all-zero word elsewhere); ONE all-reduce(SUM) of the scores' int64 words
     gives every rank every item's score bit for bit -- errors are unbounded, so no sentinel is safe inside a MAX;
     the v2t items are local;
  3. ONE cmve_pairwise_count pass over (all captions) x (this shard) counts both directions; rank 0 alone passes
     n_global for the NaN items' positions;
  4. ONE all-reduce(SUM) carrying the t2v positions and this shard's v2t R@K sums (cmve_pairwise_list_ranks).
Top-k merges the shards' local lists on score = -error.  The words are those of the unsharded K18.

Collectives go through a communicator object: ``TorchComm`` is the torch.distributed process
group (backend "nccl" = RCCL on the GPU, gloo in the CPU tests); ``LocalGroup`` runs N shards in
ONE process, one thread and HIP stream per shard (a host driving several shards -- on one GPU or
several -- with the same coordination code).

``ShardedGallery(...)`` is the one constructor and the base class: the layout, the collectives and the endings of
cal_perf / evaluate / topk that both families share.  It builds a ``CosineShardedGallery`` (``shard``: a RowSet, ``ws``,
``eps``; the first protocol above) or a ``MeasureShardedGallery`` (``shard``: a Tensor, the filters' pack, band list,
latch and counters; the second), each with its own bodies of the eight public methods.  A family's shard-local
arithmetic is a handful of methods over the HIP kernels (``_pack``, ``_row_gt``, ``_col_gt``, ``_count``, ``_ranks``,
``_positions``; ``_pw_rows``, ``_pw_items``, ``_pw_count``, ``_pw_ranks``, ``_pw_topk``): the seam a test's oracle
subclass replaces.  The coordination above them is the same for every communicator.
"""
from __future__ import annotations

import functools
import threading
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import engine
from . import _lib


def _world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def shard_bounds(n_global: int, world: int, rank: int):
    """Contiguous shards of ceil(n/world) rows: [lo, hi)."""
    per = (n_global + world - 1) // world
    lo = min(n_global, rank * per)
    return lo, min(n_global, lo + per)


# ---------------------------------------------------------------------------------------------
# communicators
# ---------------------------------------------------------------------------------------------

class _Done:
    """A completed collective (the Work of a synchronous exchange)."""

    def wait(self):
        return True


class TorchComm:
    """torch.distributed's default process group (RCCL on the GPU path, gloo in CPU tests); a
    single-process job (no process group) is world 1 and every collective is a no-op / copy."""

    def __init__(self):
        self.rank, self.world = _world()

    def all_reduce(self, t: torch.Tensor, op: str) -> torch.Tensor:
        """In place; op 'sum' or 'max'."""
        if self.world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM if op == "sum" else dist.ReduceOp.MAX)
        return t

    def all_gather_into(self, out: torch.Tensor, x: torch.Tensor, async_op: bool = False):
        """out = cat over ranks of x (equal shapes); async_op returns a Work to .wait() on."""
        if self.world == 1:
            out.copy_(x)
            return _Done() if async_op else None
        w = dist.all_gather_into_tensor(out, x.contiguous(), async_op=async_op)
        return w

    def barrier(self):
        if self.world > 1:
            dist.barrier()


class CAbiComm:
    """The torch.distributed ranks over the C ABI's own RCCL communicator (``cmve_dist_*``, csrc/dist.hip): the
    collectives a host without torch would call, driven through the same ShardedGallery coordination.  The
    128-byte unique id is made on rank 0 and broadcast over the process group (``uid`` given: used as is,
    e.g. by a host with its own bootstrap); every collective is enqueued on the caller's current stream.
    At world 1 the collectives still run (identity gathers / reductions), so the path is exercised on one GPU."""

    always = True  # run the collectives at world 1 too (see _solo)
    _TYPES = {torch.float32: _lib.CMVE_F32, torch.float64: _lib.CMVE_F64, torch.int32: _lib.CMVE_I32,
              torch.int64: _lib.CMVE_I64}

    def __init__(self, device: Optional[torch.device] = None, rank: Optional[int] = None,
                 world: Optional[int] = None, uid: Optional[bytes] = None):
        import ctypes as C
        r0, w0 = _world()
        self.rank = r0 if rank is None else int(rank)
        self.world = w0 if world is None else int(world)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        self.device = torch.device(dev.type, idx)  # indexed: tensors report 'cuda:N', never bare 'cuda'
        if uid is None:
            buf = C.create_string_buffer(_lib.DIST_UNIQUE_ID_BYTES)
            if self.rank == 0:
                _lib.check(_lib.lib.cmve_dist_unique_id(buf), "cmve_dist_unique_id")
            if self.world > 1:
                obj = [bytes(buf.raw) if self.rank == 0 else None]
                dist.broadcast_object_list(obj, src=0)
                buf = C.create_string_buffer(obj[0], _lib.DIST_UNIQUE_ID_BYTES)
        else:
            buf = C.create_string_buffer(bytes(uid), _lib.DIST_UNIQUE_ID_BYTES)
        h = C.c_void_p()
        _lib.check(_lib.lib.cmve_create(idx, C.c_void_p(torch.cuda.current_stream(idx).cuda_stream), C.byref(h)),
                   "cmve_create")
        self._h = h.value
        _lib.check(_lib.lib.cmve_dist_init(self._h, self.world, self.rank, buf), "cmve_dist_init")
        n, rk = C.c_int32(), C.c_int32()
        _lib.check(_lib.lib.cmve_dist_size(self._h, C.byref(n), C.byref(rk)), "cmve_dist_size")
        if (n.value, rk.value) != (self.world, self.rank):
            raise RuntimeError(f"CAbiComm: communicator is rank {rk.value} of {n.value}, expected "
                               f"{self.rank} of {self.world}")

    def _code(self, t: torch.Tensor) -> int:
        if t.dtype not in self._TYPES or not t.is_contiguous() or t.device != self.device:
            raise ValueError(f"CAbiComm: contiguous {list(self._TYPES)} tensors on {self.device} only, got "
                             f"{t.dtype} on {t.device}")
        return self._TYPES[t.dtype]

    def _on_current(self):
        import ctypes as C
        _lib.check(_lib.lib.cmve_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                   "cmve_set_stream")

    def all_reduce(self, t: torch.Tensor, op: str) -> torch.Tensor:
        """In place; op 'sum' or 'max'."""
        code = self._code(t)
        self._on_current()
        _lib.check(_lib.lib.cmve_dist_allreduce(self._h, engine._ptr(t), t.numel(), code,
                                                _lib.DIST_SUM if op == "sum" else _lib.DIST_MAX),
                   "cmve_dist_allreduce")
        return t

    def all_gather_into(self, out: torch.Tensor, x: torch.Tensor, async_op: bool = False):
        """out = cat over ranks of x (equal shapes), enqueued on the current stream (async_op: a completed
        Work -- the stream order already holds every later reader)."""
        x = x.contiguous()
        code = self._code(x)
        if (out.dtype != x.dtype or out.numel() != self.world * x.numel() or not out.is_contiguous()
                or out.device != self.device):
            raise ValueError(f"CAbiComm.all_gather_into: out must be world x the input, same dtype, contiguous, on "
                             f"{self.device}")
        self._on_current()
        _lib.check(_lib.lib.cmve_dist_allgather(self._h, engine._ptr(x), x.numel(), code, engine._ptr(out)),
                   "cmve_dist_allgather")
        return _Done() if async_op else None

    def barrier(self):
        t = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.all_reduce(t, "sum")
        torch.cuda.current_stream(self.device).synchronize()

    def close(self):
        if self._h:
            _lib.lib.cmve_dist_destroy(self._h)
            _lib.lib.cmve_destroy(self._h)
            self._h = None


class ThreadComm:
    """One shard's view of a ``LocalGroup``: the collectives of TorchComm between threads of one
    process.  Every exchange completes its inputs on the caller's stream first and its outputs
    before returning, so the shards may run on different HIP streams (or devices)."""

    def __init__(self, group: "LocalGroup", rank: int):
        self.group, self.rank, self.world = group, rank, group.n

    def _exchange(self, x: torch.Tensor) -> List[torch.Tensor]:
        if x.is_cuda:
            torch.cuda.current_stream(x.device).synchronize()
        g = self.group
        g.slots[self.rank] = x
        g.barrier.wait()
        vals = list(g.slots)
        return vals

    def _release(self, out: torch.Tensor):
        if out.is_cuda:
            torch.cuda.current_stream(out.device).synchronize()
        self.group.barrier.wait()  # every shard has read the deposited inputs

    def all_reduce(self, t: torch.Tensor, op: str) -> torch.Tensor:
        vals = [v.to(t.device) for v in self._exchange(t)]
        st = torch.stack(vals)
        r = st.sum(0) if op == "sum" else st.max(0).values
        self._release(r)
        t.copy_(r)
        if t.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()
        return t

    def all_gather_into(self, out: torch.Tensor, x: torch.Tensor, async_op: bool = False):
        vals = [v.to(out.device) for v in self._exchange(x.contiguous())]
        r = torch.cat(vals)
        self._release(r)
        out.copy_(r.reshape(out.shape))
        if out.is_cuda:
            torch.cuda.current_stream(out.device).synchronize()
        return _Done() if async_op else None

    def barrier(self):
        self.group.barrier.wait()


class LocalGroup:
    """N shards in ONE process: ``run(fn)`` calls fn(rank, comm) on N threads, each on its own HIP
    stream (devices[rank] if given, else the current device), and returns the N results.  The
    coordination code is the same as across processes; a shard that raises aborts the group."""

    def __init__(self, n: int, devices: Optional[Sequence[torch.device]] = None, timeout: float = 600.0):
        self.n = int(n)
        self.devices = list(devices) if devices is not None else None
        self.barrier = threading.Barrier(self.n, timeout=timeout)
        self.slots: List[Optional[torch.Tensor]] = [None] * self.n

    def comm(self, rank: int) -> ThreadComm:
        return ThreadComm(self, rank)

    def run(self, fn: Callable[[int, ThreadComm], object]) -> list:
        results: list = [None] * self.n
        errors: list = [None] * self.n

        def body(r):
            try:
                dev = self.devices[r] if self.devices is not None else None
                if torch.cuda.is_available():
                    dev = dev or torch.device("cuda", torch.cuda.current_device())
                    torch.cuda.set_device(dev)
                    with torch.cuda.stream(torch.cuda.Stream(dev)):
                        results[r] = fn(r, self.comm(r))
                        torch.cuda.current_stream(dev).synchronize()
                else:
                    results[r] = fn(r, self.comm(r))
            except BaseException as e:  # noqa: BLE001 -- re-raised below; free the others
                errors[r] = e
                self.barrier.abort()

        threads = [threading.Thread(target=body, args=(r,)) for r in range(self.n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        first = next((e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)), None)
        if first is None:
            first = next((e for e in errors if e is not None), None)
        if first is not None:
            raise first
        return results


def _solo(comm) -> bool:
    """A world-1 communicator whose collectives may be skipped (CAbiComm runs them even then: `always`)."""
    return comm.world == 1 and not getattr(comm, "always", False)


def _comm(comm):
    """A communicator from None (TorchComm), an int world size (legacy: TorchComm, which must agree),
    or a communicator object."""
    if comm is None or isinstance(comm, int):
        c = TorchComm()
        if isinstance(comm, int) and comm != c.world:
            raise ValueError(f"world {comm} given, but the process group has {c.world} ranks")
        return c
    return comm


# ---------------------------------------------------------------------------------------------
# collective steps (device-agnostic: RCCL / gloo / threads)
# ---------------------------------------------------------------------------------------------

def local_gt_lists(gts_global: Sequence[Sequence[int]], lo: int, hi: int):
    """GT lists restricted to the shard [lo, hi), re-indexed locally."""
    return [[g - lo for g in l if lo <= g < hi] for l in gts_global]


_NAN_GT = -1e300  # below every cosine: "this shard's GTs all score NaN" inside the MAX all-reduce


def encode_gt_scores(sgt: torch.Tensor) -> torch.Tensor:
    """Per-shard GT scores (cmve_gt_thresholds: NaN = no GT in this shard, +inf = GTs here but every
    one scores NaN, else the best finite score) -> keys whose MAX over the shards is the global
    answer: a finite score wins over NaN GTs, which win over no GT (NaN -> -inf, +inf -> -1e300)."""
    return torch.nan_to_num(sgt, nan=-np.inf, posinf=_NAN_GT)


def decode_gt_scores(key: torch.Tensor) -> torch.Tensor:
    """Inverse of encode_gt_scores after the MAX: -inf -> NaN (no GT anywhere), -1e300 -> +inf."""
    s = torch.where(key == _NAN_GT, torch.full_like(key, float("inf")), key)
    return torch.where(torch.isinf(s) & (s < 0), torch.full_like(s, float("nan")), s)


def merge_gt_scores(sgt_partial: torch.Tensor, comm=None) -> torch.Tensor:
    """all-reduce(MAX) of per-shard best-GT scores (encode / MAX / decode)."""
    comm = _comm(comm)
    if _solo(comm):
        return sgt_partial
    s = encode_gt_scores(sgt_partial)
    comm.all_reduce(s, "max")
    return decode_gt_scores(s)


def reduce_counts(cnt: torch.Tensor, comm=None) -> torch.Tensor:
    """all-reduce(SUM) of per-shard better-than-GT counts."""
    return _comm(comm).all_reduce(cnt, "sum")


def gather_rows_async(x_local: torch.Tensor, out: torch.Tensor, comm=None):
    """all_gather_into_tensor(out, x_local) as an async collective (RCCL runs it on its own stream):
    returns the Work to .wait() on before reading `out`, or None at world 1 (plain copy)."""
    comm = _comm(comm)
    if _solo(comm):
        out.copy_(x_local)
        return None
    return comm.all_gather_into(out, x_local.contiguous(), async_op=True)


def all_gather_rows(x_local: torch.Tensor, comm=None) -> torch.Tensor:
    """Rows of every rank in rank order (equal row counts on every rank)."""
    comm = _comm(comm)
    if _solo(comm):
        return x_local
    out = torch.empty((comm.world * x_local.shape[0],) + tuple(x_local.shape[1:]), dtype=x_local.dtype,
                      device=x_local.device)
    comm.all_gather_into(out, x_local.contiguous())
    return out


def all_gather_var(x_local: torch.Tensor, comm=None) -> torch.Tensor:
    """Rows of every rank in rank order when ranks hold different row counts: the counts are
    gathered first, every rank pads to the largest, and the padding is dropped after the gather."""
    comm = _comm(comm)
    if _solo(comm):
        return x_local
    n = torch.tensor([x_local.shape[0]], dtype=torch.int64, device=x_local.device)
    ns = all_gather_rows(n, comm).tolist()
    m = max(ns)
    if min(ns) == m:
        return all_gather_rows(x_local, comm)
    pad = torch.zeros((m,) + tuple(x_local.shape[1:]), dtype=x_local.dtype, device=x_local.device)
    pad[:x_local.shape[0]] = x_local
    g = all_gather_rows(pad, comm)
    return torch.cat([g[r * m:r * m + ns[r]] for r in range(comm.world)])


def any_flag(flag: torch.Tensor, comm=None) -> torch.Tensor:
    """OR of a per-rank boolean over the ranks (all-reduce MAX), so that all ranks take the same branch."""
    comm = _comm(comm)
    if _solo(comm):
        return flag
    o = flag.to(torch.int32).reshape(1)
    comm.all_reduce(o, "max")
    return o[0] > 0


def ranks_from(cnt: torch.Tensor, sgt: torch.Tensor, n_q: int, n_global: int) -> torch.Tensor:
    """Global 1-based ranks on the device (cmve_gt_ranks): no GT (NaN) -> n_global + 1, every GT NaN
    (+inf) -> n_global, else count + 1."""
    return engine.gt_ranks(cnt, sgt, n_q, n_global)


def pad_topk(idx: torch.Tensor, scores: torch.Tensor, k: int):
    """Pad a local [n_q, kk] top-k to k columns with empty slots (id -1, score NaN)."""
    n_q, kk = idx.shape
    if kk >= k:
        return idx, scores
    pi = torch.full((n_q, k - kk), -1, dtype=idx.dtype, device=idx.device)
    ps = torch.full((n_q, k - kk), float("nan"), dtype=scores.dtype, device=scores.device)
    return torch.cat([idx, pi], 1), torch.cat([scores, ps], 1)


def gather_topk(idx_global: torch.Tensor, scores: torch.Tensor, comm=None):
    """all-gather of every shard's local top-k: [n_q, world * k] ids (int64) / fp64 scores, shard r's
    run at columns [r*k, (r+1)*k) of each query (the layout cmve_merge_topk reads)."""
    comm = _comm(comm)
    world = comm.world
    ids = idx_global.to(torch.int64).contiguous()
    sc = scores.to(torch.float64).contiguous()
    if _solo(comm):
        return ids, sc
    n_q, kk = ids.shape
    gi = all_gather_rows(ids, comm)
    gs = all_gather_rows(sc, comm)
    return (gi.reshape(world, n_q, kk).permute(1, 0, 2).reshape(n_q, -1).contiguous(),
            gs.reshape(world, n_q, kk).permute(1, 0, 2).reshape(n_q, -1).contiguous())


def merge_sorted_topk(ids: torch.Tensor, scores: torch.Tensor, lists: int, k: int):
    """cmve_merge_topk on the device: `lists` sorted runs per query -> the best k (score desc, global
    id asc; empty slots -1 / NaN)."""
    n_q, width = ids.shape
    k_in = width // lists
    out_i = torch.empty((n_q, k), dtype=torch.int64, device=ids.device)
    out_s = torch.empty((n_q, k), dtype=torch.float64, device=ids.device)
    _lib.check(_lib.lib.cmve_merge_topk(engine.handle(ids.device), engine._ptr(ids.contiguous()),
                                        engine._ptr(scores.contiguous()), n_q, lists, k_in, k,
                                        engine._ptr(out_i), engine._ptr(out_s)), "cmve_merge_topk")
    return out_i, out_s


def merge_topk(idx_global: torch.Tensor, scores: torch.Tensor, k: int, comm=None, to_host: bool = True):
    """Gather every shard's local top-k (global ids, fp64 scores; id -1 = empty slot) and keep the best
    k per query, ordered (score desc, global id asc), by the HIP k-way merge.  Returns (ids int64
    [n_q, k'], scores fp64 [n_q, k']), k' = min(k, world * k_local); slots past the available entries
    hold -1 / NaN."""
    comm = _comm(comm)
    ids, sc = gather_topk(idx_global, scores, comm)
    kout = min(k, ids.shape[1])
    out_i, out_s = merge_sorted_topk(ids, sc, comm.world, kout)
    if not to_host:
        return out_i, out_s
    return out_i.cpu().numpy(), out_s.cpu().numpy()


def recall_counts_device(ranks: torch.Tensor) -> torch.Tensor:
    """#(rank <= 1), #(rank <= 5), #(rank <= 10), sum of ranks: int64 [4] on the device (R@K counts
    without a host round trip; metrics.py:149-157 divides by n_q)."""
    return torch.stack([(ranks <= 1).sum(), (ranks <= 5).sum(), (ranks <= 10).sum(), ranks.sum()])


def metrics_from_ranks(ranks: np.ndarray) -> List[float]:
    """(R@1, R@5, R@10, medr, meanr) -- LINAS-engine/util/metrics.py:149-157."""
    n = ranks.shape[0]
    return [100.0 * np.count_nonzero(ranks <= 1) / n, 100.0 * np.count_nonzero(ranks <= 5) / n,
            100.0 * np.count_nonzero(ranks <= 10) / n, float(np.median(ranks)), float(ranks.mean())]


def metrics_from_recall(rec: Sequence[int], n: int) -> List[float]:
    """(R@1, R@5, R@10, meanr) from recall_counts_device sums over n queries."""
    return [100.0 * rec[0] / n, 100.0 * rec[1] / n, 100.0 * rec[2] / n, rec[3] / n]


def ap_from_positions(positions) -> float:
    """APScorer (LINAS-engine/basic/metric.py:31-46) from the positions of a list's relevant items."""
    p = np.sort(np.asarray(positions, np.float64))
    if p.size == 0:
        return 0.0
    return float(np.sum(np.arange(1, p.size + 1) / p) / p.size)


# ---------------------------------------------------------------------------------------------
# the shard
# ---------------------------------------------------------------------------------------------

_L2_MEASURES = ('euclidean', 'l2', 'l2_norm')  # CMVE_PW_L2 with fp64 score words: what K19 - K21 filter
_L1_MEASURES = ('l1', 'l1_norm')  # CMVE_PW_L1 with fp64 score words: what K22 / K23 filter (filter="l1")
_JACCARD_MEASURES = ('jaccard',)  # CMVE_PW_JACCARD with float32 score words: what K24 / K25 filter (filter="jaccard")


class ShardedGallery:
    """This rank's gallery shard [offset, offset + n) of an n_global-video gallery, resident in HBM: the constructor
    of both families and what they share -- the layout, the collectives and the endings of cal_perf, evaluate and
    topk.  ``ShardedGallery(...)`` builds a ``CosineShardedGallery`` under measure='cosine' (the default) and a
    ``MeasureShardedGallery`` under one of evaluation.py's non-cosine measures (ValueError on an unknown one); each
    family's docstring names the arguments it reads, and it ignores the others.  A family built directly takes its own
    measures only, and code that overrides the shard-local arithmetic subclasses a family, not this base: ValueError.

    ``comm``: a communicator (default: TorchComm over torch.distributed's process group).
    ``filter=True`` needs a Euclidean measure: ValueError under any other, cosine included; ``filter="l1"`` needs
    l1 / l1_norm, ``filter="jaccard"`` needs jaccard, ``filter="cosine"`` needs cosine: ValueError under any other.
    Under cosine ``filter="cosine"`` builds a ``CosineFilterShardedGallery``, the cosine family with the one-pass route
    (K27) that the measure family takes: ``_OnePassRoute`` holds that route's coordination once, for both."""

    def __new__(cls, *args, **kw):
        if cls is ShardedGallery:  # measure, filter: __init__'s 10th and 11th arguments
            cls = _family(kw.get('measure', args[9] if len(args) > 9 else 'cosine'),
                          kw.get('filter', args[10] if len(args) > 10 else None))
        return object.__new__(cls)

    def __init__(self, local_embs, offset: int, n_global: int, with_lo: bool = False, eps: float = 0.0,
                 device: Optional[torch.device] = None, with_f16: bool = True, comm=None, cap: int = 1 << 22,
                 measure: str = 'cosine', filter: Optional[bool] = None, band_cap: Optional[int] = None):
        if isinstance(filter, str) and filter == "l1":
            if measure not in _L1_MEASURES:
                raise ValueError(f'ShardedGallery: filter="l1" needs an L1 measure {_L1_MEASURES}, not {measure!r}')
        elif isinstance(filter, str) and filter == "jaccard":
            if measure not in _JACCARD_MEASURES:
                raise ValueError(f'ShardedGallery: filter="jaccard" needs the jaccard measure, not {measure!r}')
        elif isinstance(filter, str) and filter == "cosine":
            if measure != 'cosine':
                raise ValueError(f'ShardedGallery: filter="cosine" needs the cosine measure, not {measure!r}')
        elif filter and measure not in _L2_MEASURES:
            raise ValueError(f"ShardedGallery: filter=True needs a Euclidean measure {_L2_MEASURES}, not {measure!r}")
        family = _family(measure, filter)
        if not isinstance(self, family):  # a family built directly, or a subclass of this base alone
            raise ValueError(f"ShardedGallery: measure {measure!r} needs a {family.__name__}, "
                             f"not a {type(self).__name__}")
        self.comm = _comm(comm)
        self.rank, self.world = self.comm.rank, self.comm.world
        self.offset = int(offset)
        self.n_global = int(n_global)
        self.measure = measure
        # the family's own state: shard, device, n and what its route needs
        self._init_shard(local_embs, device, with_lo=with_lo, eps=eps, with_f16=with_f16, cap=cap, filter=filter,
                         band_cap=band_cap)

    @property
    def filter_stats(self):
        """The counters of the last pass's filtered count over this shard, or None: that pass ran no filter."""
        return None

    def local_v2t_lists(self, v2t_gts_global):
        return [list(v2t_gts_global[self.offset + j]) for j in range(self.n)]

    # ---- collectives ----
    def all_gather_rows(self, x_local: torch.Tensor) -> torch.Tensor:
        return all_gather_rows(x_local, self.comm)

    def gather_rows_async(self, x_local: torch.Tensor, out: torch.Tensor):
        """gather_rows_async for this shard's communicator.  Issue it BEFORE enqueueing the compute that
        should overlap it -- the collective first waits for the work already on the current stream --
        and call .wait() on the returned Work before reading `out`."""
        return gather_rows_async(x_local, out, self.comm)

    def _check_layout(self):
        """Gathers in rank order must reproduce the global video order: shard r = [offset_r, offset_r + n_r),
        contiguous and increasing with r."""
        if self.world == 1:
            if self.offset != 0 or self.n != self.n_global:
                raise ValueError("ShardedGallery: a world-1 shard must hold the whole gallery")
            return
        t = torch.tensor([[self.offset, self.n]], dtype=torch.int64, device=self.device)
        lay = all_gather_rows(t, self.comm).cpu().numpy()
        ends = lay[:, 0] + lay[:, 1]
        if lay[0, 0] != 0 or ends[-1] != self.n_global or not np.array_equal(lay[1:, 0], ends[:-1]):
            raise ValueError(f"ShardedGallery: shards are not contiguous in rank order: {lay.tolist()}")

    # ---- the endings both families share ----
    def _ranks_to_host(self, t2v, v2t, *more):
        """The evaluation's ending on the host: this shard's v2t ranks become those of ALL videos (the layout is
        checked, then one gather in rank order), and every device result an int64 host array (None stays None)."""
        if v2t is not None:
            self._check_layout()
            v2t = all_gather_var(v2t, self.comm)
        return tuple(None if x is None else x.cpu().numpy().astype(np.int64) for x in (t2v, v2t) + more)

    def _perf_lists(self, n_q: int, v2t_gt, t2v_gt):
        """cal_perf's (v2t, t2v) GT lists in global video / caption order."""
        t2v_lists = [t2v_gt[i] for i in range(n_q)]  # KeyError on a caption without GT, like metrics.py:142
        return [v2t_gt[j] for j in range(self.n_global)], t2v_lists

    def _perf(self, t2v, v2t, t2v_map: float, aps):
        """cal_perf's two 6-tuples from the global ranks, the t2v mAP and this shard's videos' v2t APs."""
        s = torch.tensor([float(np.sum(aps))], dtype=torch.float64, device=self.device)
        v2t_map = float(reduce_counts(s, self.comm).item()) / self.n_global
        return (tuple(metrics_from_ranks(v2t)) + (v2t_map,), tuple(metrics_from_ranks(t2v)) + (t2v_map,))

    def _merge_local_topk(self, local, n_q: int, k: int, to_host: bool):
        """merge_topk of every shard's contribution of k columns.  local: this shard's (local ids int64, scores)
        [n_q, <= k] on the device, best first, or None when it has nothing to offer: k empty slots."""
        if local is None:
            idx = torch.full((n_q, k), -1, dtype=torch.int64, device=self.device)
            sc = torch.full((n_q, k), float("nan"), dtype=torch.float64, device=self.device)
        else:
            idx, sc = local
            idx = torch.where(idx >= 0, idx + self.offset, idx)
            idx, sc = pad_topk(idx, sc, k)  # (shards may hold fewer than k rows)
        return merge_topk(idx, sc, k, self.comm, to_host=to_host)


class _OnePassRoute:
    """The coordination of the one-pass route, once, for the families that take it (mixed in ahead of
    ``ShardedGallery``): global-id lists, the item words scored where they live and merged by an int64 SUM, ONE count
    over (all gathered captions) x (this shard), ONE all-reduce(SUM) of the t2v positions and the v2t R@K sums, and
    cal_perf's ending on those positions; the shard's band list, its counters and the plan after a pass that ended on
    the host.  A family supplies the shard-local arithmetic: ``_pw_rows`` (the captions as the count takes them),
    ``_pw_items``, ``_pw_count`` and ``_pw_ranks``."""

    def _pw_init(self, filter, band_cap):
        self._pw_filter = filter
        self._pw_band_cap = band_cap
        self._pw_stats = None  # the device counters of the last pass's filtered count
        self._pw_filter_off = False  # latched by a top-k the filter handed back whole, or a count whose band
        #                              exceeds 1/8 of the pairs: this shard stays on its unfiltered route
        self._pw_band = None  # the shard's band list, persistent; _pw_plan grows it
        self._pw_pairs = 0  # the pairs of the last filtered count

    @property
    def filter_stats(self):
        """The counters of the last pass's filtered count over this shard -- {decided, band, rescored, overflow,
        fallback}, fallback = the band list overflowed and the canonical count gave the words -- or None when that
        pass did not try the filter.  Read from the device: this synchronises."""
        if self._pw_stats is None:
            return None
        st = engine._l2_count_stats(self._pw_stats.cpu().numpy())
        return dict(st, fallback=st["overflow"] == 1)

    def _pw_plan(self):
        """After a pass that ended on the host anyway: grow this shard's band list to the reported need, or latch
        the unfiltered route when the band exceeds 1/8 of the pairs (``engine.l2_band_plan``).  Shard-local: it may
        change what a later ``_pw_count`` launches, never its words and never a collective, so the ranks need not
        agree on it."""
        st = self.filter_stats
        if st is None:
            return
        cap = engine.l2_band_plan(self._pw_pairs, st["band"], st["overflow"], self._pw_band.numel())
        if cap is None:
            self._pw_filter_off = True
        elif cap > self._pw_band.numel():
            self._pw_band = torch.empty(cap, dtype=torch.int64, device=self.device)

    def _pw_csr(self, lists, n_other: Optional[int], what: str):
        """(off, idx, items, end) of GT lists with GLOBAL ids, end = the largest id + 1 (a host int: _pw_pass checks
        it where the other side's size is known).  An id outside [0, n_other) has no owner: ValueError."""
        off = np.zeros(len(lists) + 1, np.int64)
        np.cumsum(np.fromiter((len(l) for l in lists), np.int64, count=len(lists)), out=off[1:])
        items = int(off[-1])
        ids = np.fromiter((g for l in lists for g in l), np.int64, count=items)  # int64: no wrap before the check
        end = int(ids.max()) + 1 if items else 0
        if items and (ids.min() < 0 or end > (1 << 31 if n_other is None else n_other)):
            raise ValueError(f"ShardedGallery: a {what} id outside [0, {'2^31' if n_other is None else n_other})")
        idx = ids.astype(np.int32) if items else np.zeros(1, np.int32)
        return torch.from_numpy(off).to(self.device), torch.from_numpy(idx).to(self.device), items, end

    def _pw_pass(self, q, n_q: int, row, col):
        """One evaluation of the gathered captions q against every shard, no host
        synchronisation.  row: _pw_csr of every caption's GT videos (global ids, the same on every rank) or
        None; col: _pw_csr of this shard's videos' GT captions (gathered order) or None.  Returns
        (t2v ranks | None, t2v 0-based positions int32 [items] | None -- both global, equal on every rank; v2t ranks
        | None, v2t positions | None -- this shard's videos; v2t recall sums int64 [4] of all shards | None; the merged
        t2v item words fp64 [items] | None -- equal on every rank)."""
        # an item outside the other side would get the zero word, a legitimate score: refuse it (host ints, no sync)
        if row is not None and row[3] > self.n_global:
            raise ValueError(f"ShardedGallery: a GT video id outside [0, {self.n_global})")
        if col is not None and col[3] > n_q:
            raise ValueError(f"ShardedGallery: a GT caption id outside [0, {n_q})")
        solo = _solo(self.comm)
        row_side = col_side = None
        if row is not None:
            off, idx, items = row[:3]
            # each item is scored where its video lives; the other shards hold the zero word, so the SUM of the
            # scores' integer words is the owner's word on every rank (NaN, +-inf and -0.0 as they are)
            row_sc = self._pw_items(q, (off, idx), items, False, self.offset)
            if not solo and items:
                self.comm.all_reduce(row_sc.view(torch.int64), "sum")
            # the NaN items' n_global - ... comes from ONE rank (the count entry applies it on an empty shard too)
            row_side = (off, row_sc, self.n_global if self.rank == 0 else 0)
        if col is not None:
            coff, cidx, citems = col[:3]
            # a shard video's GT captions are all here after the gather: scores and positions are rank-local
            col_side = (coff, self._pw_items(q, (coff, cidx), citems, True, 0), n_q)
        rpos, cpos = self._pw_count(q, row_side, col_side)
        v2t = self._pw_ranks(col_side[0], col_side[1], cpos, n_q) if col is not None else None
        rec = recall_counts_device(v2t) if col is not None else torch.zeros(4, dtype=torch.int64, device=self.device)
        parts = ([rpos.to(torch.int64)] if row is not None else []) + [rec.to(torch.int64)]
        # ONE all-reduce(SUM): the t2v positions and the v2t R@K sums
        both = reduce_counts(torch.cat(parts), self.comm)
        t2v = t2v_pos = None
        if row is not None:
            t2v_pos = both[:-4].to(torch.int32)
            t2v = self._pw_ranks(row_side[0], row_side[1], t2v_pos, self.n_global)
        return (t2v, t2v_pos, v2t, cpos, (both[-4:] if col is not None else None),
                row_side[1] if row is not None else None)

    def _pw_evaluate_gathered(self, q, n_q: int, t2v_gts, v2t_gts, words: bool = False):
        """(t2v ranks, t2v positions, v2t ranks of ALL videos, this shard's v2t positions) on the host from one
        _pw_pass; ``words``: also the merged t2v item words, as the pass left them on the device."""
        row = self._pw_csr(t2v_gts, self.n_global, "GT video") if t2v_gts is not None else None
        col = self._pw_csr(self.local_v2t_lists(v2t_gts), n_q, "GT caption") if v2t_gts is not None else None
        t2v, t2v_pos, v2t, v2t_pos, _, row_words = self._pw_pass(q, n_q, row, col)
        t2v, v2t, t2v_pos, v2t_pos = self._ranks_to_host(t2v, v2t, t2v_pos, v2t_pos)
        self._pw_plan()  # (after the result copies: the stream has drained)
        return (t2v, t2v_pos, v2t, v2t_pos) + ((row_words,) if words else ())

    def _pw_first_positions(self, t2v_pos, firsts, row_words):
        """The 1-based position of each caption's FIRST GT from the positions of every item (firsts: the first
        item of every non-empty list; row_words: the items' merged words on the device)."""
        return t2v_pos[firsts] + 1

    def _pw_cal_perf(self, q, n_q: int, v2t_gt, t2v_gt):
        """cal_perf's two 6-tuples from ONE _pw_pass over the captions' rows q: ranks and both mAPs (t2v: each
        caption's FIRST GT; v2t: every GT caption of a video) come from its positions, multi-GT lists included."""
        v2t_lists, t2v_lists = self._perf_lists(n_q, v2t_gt, t2v_gt)
        t2v, t2v_pos, v2t, v2t_pos, row_words = self._pw_evaluate_gathered(q, n_q, t2v_lists, v2t_lists, words=True)
        # the first GT's position is among every item's
        lens = np.fromiter((len(l) for l in t2v_lists), np.int64, count=n_q)
        has = lens > 0
        ap = np.zeros(n_q, np.float64)
        ap[has] = 1.0 / self._pw_first_positions(t2v_pos, (np.cumsum(lens) - lens)[has], row_words)
        t2v_map = float(np.mean(ap))
        offs = np.cumsum([0] + [len(l) for l in self.local_v2t_lists(v2t_lists)])
        aps = [ap_from_positions(v2t_pos[offs[j]:offs[j + 1]] + 1) for j in range(self.n)]
        return self._perf(t2v, v2t, t2v_map, aps)


class CosineShardedGallery(ShardedGallery):
    """The shard under measure='cosine': rows packed once (``shard``: a RowSet), ranked by the fp16 MFMA rank GEMM
    with its fp64 fix-up.  ``with_lo`` / ``with_f16`` / ``eps``: the pack's; ``cap``: the slots of the undecided-pair
    list (``ws``), grown by the methods that end on the host when a pass overflows it.  ``mode``: a SIM_* scoring
    mode.  Top-k returns cosines (descending)."""

    def _init_shard(self, local_embs, device, with_lo, eps, with_f16, cap, **_):
        self._setup(local_embs, with_lo, eps, device, with_f16, cap)

    def _setup(self, local_embs, with_lo, eps, device, with_f16, cap):
        self.shard = engine.RowSet(local_embs, eps=eps, with_lo=with_lo, device=device, with_f16=with_f16)
        self.device = self.shard.device
        self.n = self.shard.n
        self.eps = eps
        self.ws = engine.RankWorkspace(self.device, cap=cap)

    # ---- shard-local arithmetic (HIP kernels) ----
    def _pack(self, q_all: torch.Tensor, mode: int):
        return engine.RowSet(q_all, eps=self.eps, with_lo=(mode == _lib.SIM_BF16X3), with_f16=(mode == _lib.SIM_F16),
                             device=self.device)

    def _csr(self, lists):
        return engine.csr(lists, self.device)

    def _row_gt(self, q, csr, mode: int) -> torch.Tensor:
        """Best fp64 GT score of every caption over the GTs in this shard (NaN none, +inf all NaN)."""
        off, idx = csr
        return engine.gt_thresholds(q, self.shard, off, idx, mode)[0]

    def _col_gt(self, q, csr, mode: int):
        """(best GT score, thresholds) of every shard video over its GT captions (all gathered)."""
        off, idx = csr
        return engine.gt_thresholds(self.shard, q, off, idx, mode)

    def _count(self, q, mode: int, sgt_row: Optional[torch.Tensor], col, events=None, chunks: int = 1):
        """One fused rank GEMM: (row counts [q.n_pad] | None, col counts [n_pad] | None, overflow bool [])."""
        if sgt_row is None and col is None:
            return None, None, torch.zeros((), dtype=torch.bool, device=self.device)
        row = None
        if sgt_row is not None:
            hi, lo = engine.rank_thresholds(q, self.shard, sgt_row, mode)
            row = (sgt_row, hi, lo)
        rc, cc = engine.rank_count_launch(q, self.shard, mode, row=row, col=col, ws=self.ws, events=events,
                                          chunks=chunks)
        ch = self.ws.chunks
        ovf = (self.ws.count[:ch] > self.ws.cap // ch).any()
        return rc, cc, ovf

    def _ranks(self, cnt, sgt, n: int, n_m: int) -> torch.Tensor:
        return ranks_from(cnt, sgt, n, n_m)

    def _grow(self):
        self.ws.grow()

    def _positions(self, q, lists, mode: int):
        """1-based positions of every GT caption of every shard video among all captions (v2t mAP)."""
        return engine.gt_positions_fused(self.shard, q, lists, mode=mode)

    # ---- GT lists restricted to this shard ----
    def local_gt_csr(self, gts_global: Sequence[Sequence[int]]):
        """t2v: every caption's GT videos inside this shard, re-indexed locally."""
        return self._csr(local_gt_lists(gts_global, self.offset, self.offset + self.n))

    def local_v2t_csr(self, v2t_gts_global: Sequence[Sequence[int]]):
        """v2t: the GT captions (gathered order) of this shard's videos."""
        return self._csr(self.local_v2t_lists(v2t_gts_global))

    # ---- t2v only (the gallery_shard bench leg) ----
    def rank_queries(self, q_local: torch.Tensor, gt_csr, n_q: int, mode: int = _lib.SIM_F16, events=None,
                     return_host: bool = True, chunks: int = 1):
        """Global 1-based GT ranks of all gathered queries (t2v direction).

        q_local: this rank's [n_local, D] query embeddings (equal n_local on every rank);
        gt_csr: (off, idx) from ``local_gt_csr`` for the GATHERED query order.  The overflow flag of
        the undecided-pair list rides the counts' all-reduce, so every rank sees the same flag: all of
        them grow their lists and redo the batch together (a rank that trusted its own flag alone would
        return incomplete counts while another waited in the next all-gather)."""
        q_all = self.all_gather_rows(q_local)
        for _attempt in range(4):
            ranks, ovf = self.rank_queries_device(q_all, gt_csr, n_q, mode, events, chunks)
            if not bool(ovf.item()):
                break
            self._grow()  # every rank: the flag is the all-reduced one
        else:
            raise _lib.CmveError("ShardedGallery.rank_queries: undecided-pair list kept overflowing")
        if not return_host:
            return ranks
        return ranks.cpu().numpy().astype(np.int64)

    def rank_queries_device(self, q_all: torch.Tensor, gt_csr, n_q: int, mode: int = _lib.SIM_F16, events=None,
                            chunks: int = 1):
        """rank_queries on already-gathered queries with no host synchronisation: returns
        (ranks int64 [n_q] on the device, overflow flag bool [] on the device).  A set flag means the
        undecided-pair list overflowed and the counts are incomplete: grow the workspace and redo."""
        q = self._pack(q_all, mode)
        sgt = merge_gt_scores(self._row_gt(q, gt_csr, mode), self.comm)
        cnt, _, ovf = self._count(q, mode, sgt, None, events=events, chunks=chunks)
        if self.world > 1:  # the overflow flag rides the counts' all-reduce(SUM): one collective, all ranks agree
            both = reduce_counts(torch.cat([cnt, ovf.to(cnt.dtype).reshape(1)]), self.comm)
            cnt, ovf = both[:-1], both[-1] > 0
        return self._ranks(cnt, sgt, n_q, self.n_global), ovf

    # ---- both directions (cal_perf) ----
    def evaluate_device(self, q_all: torch.Tensor, row_csr, col_csr, n_q: int, mode: int = _lib.SIM_F16,
                        events=None, q=None):
        """One exact two-direction evaluation of the gathered captions against every shard, no host
        synchronisation.  row_csr: t2v GT lists restricted to this shard (``local_gt_csr``) or None;
        col_csr: this shard's v2t GT lists into the gathered captions (``local_v2t_csr``) or None.
        Returns (t2v ranks int64 [n_q] | None -- global, equal on every rank; v2t ranks int64 [n] | None
        -- this shard's videos; v2t recall sums int64 [4] | None -- all shards; overflow bool []).  q: the
        captions already packed (``_pack(q_all, mode)``), reused across passes over the same captions."""
        if q is None:
            q = self._pack(q_all, mode)
        sgt_r = merge_gt_scores(self._row_gt(q, row_csr, mode), self.comm) if row_csr is not None else None
        col = self._col_gt(q, col_csr, mode) if (col_csr is not None and self.n > 0) else None
        rc, cc, ovf = self._count(q, mode, sgt_r, col, events=events)
        v2t = self._ranks(cc, col[0], self.n, n_q) if col is not None else None
        if col_csr is not None and self.n == 0:  # an empty shard (shard_bounds' last rank): no videos to rank
            v2t = torch.zeros(0, dtype=torch.int64, device=ovf.device)
        parts = []
        if rc is not None:
            parts.append(rc[:n_q].to(torch.int64))
        v2t_rec = recall_counts_device(v2t) if v2t is not None else torch.zeros(4, dtype=torch.int64,
                                                                                   device=ovf.device)
        parts += [v2t_rec, ovf.to(torch.int64).reshape(1)]
        # ONE all-reduce(SUM): the t2v counts, the v2t R@K sums and the overflow flag
        both = reduce_counts(torch.cat(parts), self.comm)
        ovf = both[-1] > 0
        rec = both[-5:-1] if col_csr is not None else None
        t2v = self._ranks(both[:n_q].to(torch.int32), sgt_r, n_q, self.n_global) if row_csr is not None else None
        return t2v, v2t, rec, ovf

    def evaluate(self, q_local: torch.Tensor, t2v_gts=None, v2t_gts=None, mode: int = _lib.SIM_F16):
        """Exact global ranks of both directions, on every rank (host int64 arrays): captions = the
        rank-ordered gather of every rank's q_local (row counts may differ); t2v_gts[i] = GT video ids
        (global) of gathered caption i; v2t_gts[v] = GT caption ids (gathered order) of global video v.
        Returns (t2v ranks [n_q] | None, v2t ranks [n_global] | None)."""
        q_all = all_gather_var(q_local, self.comm)
        return self._evaluate_gathered(q_all, self._pack(q_all, mode), t2v_gts, v2t_gts, mode)

    def _evaluate_gathered(self, q_all, q, t2v_gts, v2t_gts, mode: int):
        """evaluate() on captions already gathered (q_all) and packed (q)."""
        n_q = q_all.shape[0]
        row_csr = self.local_gt_csr(t2v_gts) if t2v_gts is not None else None
        col_csr = self.local_v2t_csr(v2t_gts) if v2t_gts is not None else None
        for _attempt in range(4):
            t2v, v2t, _, ovf = self.evaluate_device(q_all, row_csr, col_csr, n_q, mode, q=q)
            if not bool(ovf.item()):
                break
            self._grow()
        else:
            raise _lib.CmveError("ShardedGallery.evaluate: undecided-pair list kept overflowing")
        return self._ranks_to_host(t2v, v2t)

    def cal_perf(self, q_local: torch.Tensor, v2t_gt, t2v_gt, mode: int = _lib.SIM_F16):
        """``LINAS-engine/validate.py:15-54`` cal_perf over the sharded gallery: the reference's two
        6-tuples (v2t (r1, r5, r10, medr, meanr, mAP), t2v (...)) on every rank.  v2t_gt: list over the
        n_global videos of GT caption ids (gathered order); t2v_gt: dict or list over the captions of GT
        video ids (metrics.get_gt's outputs).  t2v mAP is the AP of each caption's FIRST GT
        (metrics.py:61-79); v2t mAP is over every GT caption of a video (metrics.py:83-102)."""
        # the captions are gathered and packed ONCE; every pass below (both directions, the first-GT t2v pass, the
        # v2t GT positions) reuses them
        q_all = all_gather_var(q_local, self.comm)
        q = self._pack(q_all, mode)
        v2t_lists, t2v_lists = self._perf_lists(q_all.shape[0], v2t_gt, t2v_gt)
        t2v, v2t = self._evaluate_gathered(q_all, q, t2v_lists, v2t_lists, mode)
        if all(len(l) == 1 for l in t2v_lists):
            t2v_first = t2v
        else:
            t2v_first, _ = self._evaluate_gathered(q_all, q, [[l[0]] for l in t2v_lists], None, mode)
        local = self.local_v2t_lists(v2t_lists)
        if all(len(l) <= 1 for l in v2t_lists):
            aps = [1.0 / v2t[self.offset + j] if local[j] else 0.0 for j in range(self.n)]
        else:
            aps = [ap_from_positions(p) for p in self._positions(q, local, mode)]
        return self._perf(t2v, v2t, float(np.mean(1.0 / t2v_first)), aps)

    def topk(self, q_local: torch.Tensor, k: int, mode: int = _lib.SIM_F16):
        """Global exact top-k (global ids int64, fp64 cosines; host arrays) of all gathered queries (equal row
        counts on every rank), ordered (cosine desc, global id asc)."""
        q_all = self.all_gather_rows(q_local)
        q = engine.RowSet(q_all, with_lo=self.shard.has_lo, with_f16=self.shard.has_f16, device=self.device)
        kk = min(k, self.n)
        local = None  # an empty shard (shard_bounds' last rank)
        if kk >= 1:
            idx, sc = engine.topk(q, self.shard, kk, mode=mode, to_host=False)
            local = idx.to(torch.int64), sc
        return self._merge_local_topk(local, q.n, k, to_host=True)


class MeasureShardedGallery(_OnePassRoute, ShardedGallery):
    """The shard under euclidean / l1 / l2 / l1_norm / l2_norm / jaccard: the rows stay resident unnormalised in the
    measure's input dtype (``shard``: a Tensor) and K18's launches (csrc/pairwise_rank.hip) do the arithmetic.  The
    methods have the cosine family's signatures and return types; their ``mode`` / ``events`` / ``chunks`` are unused,
    no pass can overflow (the flags they return are never set) and top-k returns errors (ascending).
    ``filter`` (euclidean / l2 / l2_norm): the route of the evaluation's count pass over this shard -- False: the
    fp64 chain (K18); True: the fp16 MFMA filter (K21, ``engine.pairwise_count(filter=True)``: the same words, an
    overflowing band list resolved on the device, so nothing synchronises and no flag rides a collective); None: the
    filter from ``engine.L2_FILTER_MIN_PAIRS`` (captions x this shard's videos).  ``band_cap``: the slots of the
    shard's first band list (default ``engine.l2_band_cap`` of the first filtered pass); the methods that end on the
    host grow it, or switch this shard's later passes to the fp64 route, from the counters (``filter_stats``).
    ``filter`` (l1 / l1_norm): False -- fp64; ``"l1"`` -- the integer SAD filter: K22's count
    (``engine.pairwise_count(filter="l1")``: the same words, an overflow resolved on the device) and K23's top-k
    (``engine.pairwise_topk(filter="l1")``) over this shard, packed once as an ``engine.L1Set`` on its own grid by the
    first call that needs it; None -- the count from ``engine.L1_FILTER_MIN_PAIRS`` (d <= ``engine.L1_D_MAX``), the
    top-k from ``engine.l1_topk_auto``.  ``band_cap`` / ``filter_stats`` as above.
    ``filter`` (jaccard): the same with ``"jaccard"`` -- K24's count (``engine.pairwise_count(filter="jaccard")``) and
    K25's top-k (``engine.pairwise_topk(filter="jaccard")``) over this shard, packed once as an ``engine.JaccardSet``
    on its own grid; None -- the count from ``engine.JACCARD_FILTER_MIN_PAIRS`` (d <= ``engine.L1_D_MAX``), the top-k
    from ``engine.jaccard_topk_auto``."""

    # ---- shard-local arithmetic (HIP kernels) ----
    def _init_shard(self, local_embs, device, filter, band_cap, **_):
        from .linas.evaluation import measure_spec
        measure_spec(self.measure, 1)  # ValueError on an unknown measure
        self._pw_init(filter, band_cap)
        self._pw_device = device
        self.shard = self._pw_rows(local_embs)  # resident, unnormalised, in the measure's input dtype
        self.device = self.shard.device
        self.n = int(self.shard.shape[0])
        # the filter family that speaks for the measure: "l2" (K19 - K21, a RowSet), "l1" (K22 / K23, an L1Set),
        # "jaccard" (K24 / K25, a JaccardSet) or None; the last two are the SAD families: ``filter`` names them
        metric, _, _, sc_dt = self._pw_spec()
        self._pw_family = "l2" if self.measure in _L2_MEASURES else engine.sad_route_of(metric, sc_dt)
        self._pw_packed = None  # the shard's pack for its family's filters, made by the first call that needs it

    def _pw_spec(self):
        from .linas.evaluation import measure_spec
        metric, alpha, beta, _, sc_dt = measure_spec(self.measure, int(self.shard.shape[1]))
        return metric, alpha, beta, sc_dt

    def _pw_rows(self, x) -> torch.Tensor:
        """Rows on the device in the measure's input dtype (fp64; fp32 for jaccard)."""
        from .linas.evaluation import measure_rows
        return measure_rows(x, self.measure, self._pw_device)

    def _pw_items(self, q, csr, n_items: int, col_dir: bool, idx_base: int) -> torch.Tensor:
        """fp64 [n_items]: the scores of the listed items this shard owns, the all-zero word elsewhere."""
        off, idx = csr
        return engine.pairwise_item_scores(q, self.shard, *self._pw_spec(), off, idx, n_items, col_dir, idx_base)

    def _pw_pack(self):
        """The shard's pack for the filters, made ONCE and shared by the top-k and the count; it keeps the rows it
        is given, so there is no second copy of the shard."""
        if self._pw_packed is None:
            self._pw_packed = (engine.sad_set(self._pw_family, self.shard) if self._pw_sad()  # (on the shard's own grid)
                               else engine.RowSet(self.shard, eps=0.0, with_lo=False, device=self.device))
        return self._pw_packed

    def _pw_sad(self) -> bool:
        """The measure's filters are the SAD ones (K22 - K25): ``filter`` names the family, the pack is on a grid."""
        return self._pw_family not in (None, "l2")

    def _pw_forced(self) -> bool:
        """The constructor's filter names this family's filter (True: Euclidean, "l1": L1, "jaccard": jaccard)."""
        f = self._pw_filter
        return (isinstance(f, str) and f == self._pw_family) if self._pw_sad() else bool(f)

    def _pw_count_auto(self, pairs: int) -> bool:
        """filter=None: the family's count filter pays from its measured number of pairs (None there: never)."""
        if self._pw_sad():
            lo = engine.sad_min_pairs(self._pw_family) if self.shard.shape[1] <= engine.L1_D_MAX else None
        else:
            lo = engine.L2_FILTER_MIN_PAIRS
        return lo is not None and pairs >= lo

    def _pw_count(self, q, row, col):
        """ONE pass over (all captions) x (this shard): (row positions | None, column positions | None), int32.
        With the family's filter due the count is ``cmve_l2_count_resolved``'s (K21, Euclidean), ``cmve_l1_count``'s
        (K22, l1 / l1_norm) or ``cmve_jaccard_count``'s (K24): the same words whatever the band list does -- an
        overflow is resolved on the device --
        its counters kept on the device as this pass's ``filter_stats``."""
        self._pw_stats = None
        pairs = int(q.shape[0]) * self.n
        due = (self._pw_family is not None and self._pw_filter is not False and not self._pw_filter_off
               and (self._pw_forced() or (self._pw_filter is None and self._pw_count_auto(pairs))))
        if not due:  # (filter=False: the shard decides the route, not the engine's own auto rule on plain rows)
            return engine.pairwise_count(q, self.shard, *self._pw_spec(), row=row, col=col, filter=False)
        if self._pw_band is None:
            cap = engine.l2_band_cap(pairs) if self._pw_band_cap is None else int(self._pw_band_cap)
            self._pw_band = torch.empty(cap, dtype=torch.int64, device=self.device)
        rpos, cpos, self._pw_stats = engine.pairwise_count(q, self._pw_pack(), *self._pw_spec(), row=row, col=col,
                                                           filter=self._pw_family if self._pw_sad() else True,
                                                           band=self._pw_band, return_stats=True)
        self._pw_pairs = pairs
        return rpos, cpos

    def _pw_ranks(self, off, sc, pos, n_m: int) -> torch.Tensor:
        return engine.pairwise_list_ranks(off, sc, pos, n_m)

    def _pw_topk(self, q, k: int):
        """This shard's (local ids int64, errors fp64) [n_q, k] on the device, (error asc, id asc), NaN last.
        Under a Euclidean measure engine.pairwise_topk may take the K20 filter (auto), under l1 / l1_norm the K23
        filter and under jaccard the K25 filter (auto, or forced by ``filter="l1"`` / ``filter="jaccard"``; never under
        ``filter=False``); what it leaves unresolved is finished on the K18 route here, on this shard alone: the words
        are the same and no flag rides a collective."""
        sad = self._pw_sad()
        if self._pw_filter_off or (sad and self._pw_filter is False):
            return engine.pairwise_topk(q, self.shard, *self._pw_spec(), k, to_host=False, filter=False)
        forced = sad and self._pw_forced()
        auto = functools.partial(engine.sad_topk_auto, self._pw_family) if sad else engine.l2_topk_auto
        fits = not sad or self.shard.shape[1] <= engine.L1_D_MAX  # (beyond it auto stays on K18; forced: ValueError)
        if (self._pw_packed is None and self._pw_family is not None
                and (forced or (fits and auto(q.shape[0], self.n, packed=True)))):
            self._pw_pack()  # ONCE, by the first call large enough for a filter
        g = self.shard if self._pw_packed is None else self._pw_packed
        idx, err, st = engine.pairwise_topk(q, g, *self._pw_spec(), k, to_host=False, return_stats=True,
                                            filter=self._pw_family if forced else None)
        self._pw_filter_off = st is not None and st["fallback"]
        return idx, err

    # ---- GT lists: global ids ----
    def local_gt_csr(self, gts_global: Sequence[Sequence[int]]):
        """t2v: (off, idx, items, end) of every caption's GT videos with GLOBAL ids -- the same on every rank (the
        items are scored where they live)."""
        return self._pw_csr(gts_global, self.n_global, "GT video")

    def local_v2t_csr(self, v2t_gts_global: Sequence[Sequence[int]]):
        """v2t: (off, idx, items, end) of the GT captions (gathered order) of this shard's videos; the caption ids
        are checked against n_q where it is known, in the evaluation."""
        return self._pw_csr(self.local_v2t_lists(v2t_gts_global), None, "GT caption")

    # ---- t2v only ----
    def rank_queries(self, q_local: torch.Tensor, gt_csr, n_q: int, mode: int = _lib.SIM_F16, events=None,
                     return_host: bool = True, chunks: int = 1):
        """Global 1-based GT ranks of all gathered queries (t2v direction).  q_local: this rank's [n_local, D]
        query embeddings (equal n_local on every rank); gt_csr: ``local_gt_csr``'s tuple for the GATHERED order."""
        ranks, _ = self.rank_queries_device(self.all_gather_rows(q_local), gt_csr, n_q)
        if not return_host:
            return ranks
        ranks = ranks.cpu().numpy().astype(np.int64)
        self._pw_plan()
        return ranks

    def rank_queries_device(self, q_all: torch.Tensor, gt_csr, n_q: int, mode: int = _lib.SIM_F16, events=None,
                            chunks: int = 1):
        """rank_queries on already-gathered queries with no host synchronisation: (ranks int64 [n_q] on the
        device, an overflow flag bool [] that is never set)."""
        t2v = self._pw_pass(self._pw_rows(q_all), n_q, gt_csr, None)[0]
        return t2v, torch.zeros((), dtype=torch.bool, device=self.device)

    # ---- both directions (cal_perf) ----
    def evaluate_device(self, q_all: torch.Tensor, row_csr, col_csr, n_q: int, mode: int = _lib.SIM_F16,
                        events=None, q=None):
        """One exact two-direction evaluation of the gathered captions against every shard, no host
        synchronisation.  row_csr / col_csr: ``local_gt_csr``'s / ``local_v2t_csr``'s tuples or None (a GT video id
        outside the gallery or a GT caption id outside [0, n_q) raises ValueError); q: the captions' rows
        (``_pw_rows(q_all)``) when the caller holds them.  Returns (t2v ranks int64 [n_q] | None -- global, equal on
        every rank; v2t ranks int64 [n] | None -- this shard's videos; v2t recall sums int64 [4] | None -- all
        shards; an overflow flag bool [] that is never set)."""
        t2v, _, v2t, _, rec, _ = self._pw_pass(self._pw_rows(q_all) if q is None else q, n_q, row_csr, col_csr)
        return t2v, v2t, rec, torch.zeros((), dtype=torch.bool, device=self.device)

    def evaluate(self, q_local: torch.Tensor, t2v_gts=None, v2t_gts=None, mode: int = _lib.SIM_F16):
        """Exact global ranks of both directions, on every rank (host int64 arrays): captions = the
        rank-ordered gather of every rank's q_local (row counts may differ); t2v_gts[i] = GT video ids
        (global) of gathered caption i; v2t_gts[v] = GT caption ids (gathered order) of global video v.
        Returns (t2v ranks [n_q] | None, v2t ranks [n_global] | None)."""
        q_all = all_gather_var(q_local, self.comm)
        t2v, _, v2t, _ = self._pw_evaluate_gathered(self._pw_rows(q_all), q_all.shape[0], t2v_gts, v2t_gts)
        return t2v, v2t

    def cal_perf(self, q_local: torch.Tensor, v2t_gt, t2v_gt, mode: int = _lib.SIM_F16):
        """``LINAS-engine/validate.py:15-54`` cal_perf over the sharded gallery: the reference's two 6-tuples
        (v2t (r1, r5, r10, medr, meanr, mAP), t2v (...)) on every rank, v2t_gt / t2v_gt as metrics.get_gt returns
        them (gathered caption order).  Ranks and both mAPs (t2v: each caption's FIRST GT; v2t: every GT caption
        of a video) come from the positions of ONE pass, multi-GT lists included."""
        q_all = all_gather_var(q_local, self.comm)
        return self._pw_cal_perf(self._pw_rows(q_all), q_all.shape[0], v2t_gt, t2v_gt)

    def topk(self, q_local: torch.Tensor, k: int, mode: int = _lib.SIM_F16):
        """Global exact top-k of all gathered queries (row counts may differ: a single caption may sit on one
        rank alone): host (ids int64, ERRORS fp64) ordered (error asc, global id asc), NaN last, k clamped to the
        gallery -- the order of cmve_pairwise_topk on the whole gallery (inference.py:78-80)."""
        q = self._pw_rows(all_gather_var(q_local, self.comm))
        k = int(min(k, self.n_global))  # as cmve_pairwise_topk clamps k to the gallery
        if k < 1:
            return np.zeros((q.shape[0], 0), np.int64), np.zeros((q.shape[0], 0))
        if k > _lib.TOPK_MAX:
            raise ValueError(f"ShardedGallery.topk: k <= {_lib.TOPK_MAX}")
        local = None  # an empty shard
        if self.n >= 1:
            idx, err = self._pw_topk(q, min(k, self.n))
            local = idx, -err  # the merge orders by score descending: score = -error
        ids, sc = self._merge_local_topk(local, q.shape[0], k, to_host=False)
        return ids.cpu().numpy(), (-sc).cpu().numpy()


class CosineFilterShardedGallery(_OnePassRoute, CosineShardedGallery):
    """The cosine family under ``filter="cosine"`` (K27): cal_perf, evaluate, evaluate_device, rank_queries and
    rank_queries_device take ONE pass per shard, the measure family's plan (``_pw_pass``) on K26's count -- the item
    words scored where the video lives and merged by an int64 SUM, one ``engine.cos_count(resolved=True)`` over (all
    captions) x (this shard): the same words whatever the band list does, an overflow resolved on the device, so
    nothing synchronises, no flag rides a collective and the flags the ``*_device`` methods return are never set --,
    one all-reduce(SUM) of the t2v positions and the v2t R@K sums.  It needs eps = 0 and the fp16 plane (ValueError),
    and ``mode=SIM_F16`` on those methods (ValueError); ``local_gt_csr`` / ``local_v2t_csr`` return global-id lists.
    ``band_cap``: the slots of the shard's first band list (default ``engine.l2_band_cap`` of the first pass); the
    methods that end on the host grow it to the need the counters report (``filter_stats``).  There is no latch back to
    the cosine family's route: that route issues other collectives (an encoded MAX, other lengths, redo loops), and a
    shard that left the one pass on its own counters would leave the other ranks waiting in theirs -- a shard whose
    band is large keeps the pass, with a list that holds the band.  topk is the cosine family's.  Built with ``filter``
    None / False it is the cosine family."""

    def _init_shard(self, local_embs, device, with_lo, eps, with_f16, cap, filter=None, band_cap=None, **_):
        self._pw_init(filter, band_cap)
        if self._pw_forced():  # the pass is fp16 on what cmve_cos_count accepts
            if eps != 0:
                raise ValueError(f'ShardedGallery: filter="cosine" needs eps = 0, not {eps!r}')
            if not with_f16:
                raise ValueError('ShardedGallery: filter="cosine" needs the fp16 plane (with_f16=True)')
        super()._init_shard(local_embs, device, with_lo=with_lo, eps=eps, with_f16=with_f16, cap=cap)

    # ---- shard-local arithmetic (HIP kernels) ----
    def _pw_rows(self, x):
        """The gathered captions packed as ``cmve_cos_count`` takes them."""
        return self._pack(x, _lib.SIM_F16)

    def _pw_items(self, q, csr, n_items: int, col_dir: bool, idx_base: int) -> torch.Tensor:
        """fp64 [n_items]: cos64 of the listed items this shard owns, the all-zero word elsewhere."""
        off, idx = csr
        return engine.cos_item_scores(q, self.shard, off, idx, n_items, col_dir, idx_base=idx_base)

    def _pw_count(self, q, row, col):
        """ONE ``cmve_cos_count_resolved`` over (all captions) x (this shard): (row positions | None, column
        positions | None), int32; its counters stay on the device as this pass's ``filter_stats``."""
        pairs = int(q.n) * self.n
        if self._pw_band is None:
            cap = engine.l2_band_cap(pairs) if self._pw_band_cap is None else int(self._pw_band_cap)
            self._pw_band = torch.empty(cap, dtype=torch.int64, device=self.device)
        rpos, cpos, self._pw_stats = engine.cos_count(q, self.shard, row, col, band=self._pw_band, resolved=True)
        self._pw_pairs = pairs
        return rpos, cpos

    def _pw_ranks(self, off, sc, pos, n_m: int) -> torch.Tensor:
        return engine.pairwise_list_ranks(off, sc, pos, n_m)

    def _pw_first_positions(self, t2v_pos, firsts, row_words):
        """As the cosine family ranks a caption's first GT ALONE: a first item whose word is NaN takes the last
        place, n_global, wherever the list's other NaN items put it among them."""
        first = t2v_pos[firsts] + 1
        nan = torch.isnan(row_words[torch.from_numpy(firsts).to(row_words.device)])
        first[nan.cpu().numpy()] = self.n_global
        return first

    def _pw_plan(self):
        """After a pass that ended on the host anyway: grow this shard's band list to the reported need.  Shard-local,
        and it never changes the route (class docstring): the collectives of every later pass are the same on every
        rank."""
        st = self.filter_stats
        if st is not None and st["overflow"] and st["band"] > self._pw_band.numel():
            self._pw_band = torch.empty(st["band"], dtype=torch.int64, device=self.device)

    # ---- the route of a call ----
    def _pw_forced(self) -> bool:
        return isinstance(self._pw_filter, str) and self._pw_filter == "cosine"

    def _pw_due(self, mode: int) -> bool:
        """This call takes the one pass: the constructor forced it -- on every rank alike, so the ranks agree.  A call
        on the cosine family's own route leaves no counters."""
        if not self._pw_forced():
            self._pw_stats = None
            return False
        if mode != _lib.SIM_F16:
            raise ValueError('ShardedGallery: filter="cosine" is an fp16 pass: mode must be SIM_F16')
        return True

    # ---- GT lists ----
    def local_gt_csr(self, gts_global: Sequence[Sequence[int]]):
        """t2v: (off, idx, items, end) of every caption's GT videos with GLOBAL ids -- the same on every rank (the
        items are scored where they live)."""
        if not self._pw_forced():
            return super().local_gt_csr(gts_global)
        return self._pw_csr(gts_global, self.n_global, "GT video")

    def local_v2t_csr(self, v2t_gts_global: Sequence[Sequence[int]]):
        """v2t: (off, idx, items, end) of the GT captions (gathered order) of this shard's videos."""
        if not self._pw_forced():
            return super().local_v2t_csr(v2t_gts_global)
        return self._pw_csr(self.local_v2t_lists(v2t_gts_global), None, "GT caption")

    # ---- the methods: one pass under the filter, the cosine family's otherwise ----
    def rank_queries(self, q_local: torch.Tensor, gt_csr, n_q: int, mode: int = _lib.SIM_F16, events=None,
                     return_host: bool = True, chunks: int = 1):
        if not self._pw_due(mode):  # (a refusal comes before any collective)
            return super().rank_queries(q_local, gt_csr, n_q, mode, events, return_host, chunks)
        ranks, _ = self.rank_queries_device(self.all_gather_rows(q_local), gt_csr, n_q, mode)
        if not return_host:
            return ranks
        ranks = ranks.cpu().numpy().astype(np.int64)
        self._pw_plan()
        return ranks

    def rank_queries_device(self, q_all: torch.Tensor, gt_csr, n_q: int, mode: int = _lib.SIM_F16, events=None,
                            chunks: int = 1):
        if not self._pw_due(mode):
            return super().rank_queries_device(q_all, gt_csr, n_q, mode, events, chunks)
        t2v = self._pw_pass(self._pw_rows(q_all), n_q, gt_csr, None)[0]
        return t2v, torch.zeros((), dtype=torch.bool, device=self.device)

    def evaluate_device(self, q_all: torch.Tensor, row_csr, col_csr, n_q: int, mode: int = _lib.SIM_F16,
                        events=None, q=None):
        if not self._pw_due(mode):
            return super().evaluate_device(q_all, row_csr, col_csr, n_q, mode, events, q)
        t2v, _, v2t, _, rec, _ = self._pw_pass(self._pw_rows(q_all) if q is None else q, n_q, row_csr, col_csr)
        return t2v, v2t, rec, torch.zeros((), dtype=torch.bool, device=self.device)

    def evaluate(self, q_local: torch.Tensor, t2v_gts=None, v2t_gts=None, mode: int = _lib.SIM_F16):
        if not self._pw_due(mode):
            return super().evaluate(q_local, t2v_gts, v2t_gts, mode)
        q_all = all_gather_var(q_local, self.comm)
        t2v, _, v2t, _ = self._pw_evaluate_gathered(self._pw_rows(q_all), q_all.shape[0], t2v_gts, v2t_gts)
        return t2v, v2t

    def cal_perf(self, q_local: torch.Tensor, v2t_gt, t2v_gt, mode: int = _lib.SIM_F16):
        if not self._pw_due(mode):
            return super().cal_perf(q_local, v2t_gt, t2v_gt, mode)
        q_all = all_gather_var(q_local, self.comm)
        return self._pw_cal_perf(self._pw_rows(q_all), q_all.shape[0], v2t_gt, t2v_gt)


def _family(measure, filter=None) -> type:
    """The ONE dispatch on the measure (and, under cosine, on ``filter="cosine"``): the class that
    ``ShardedGallery(..., measure=, filter=)`` builds."""
    if measure != 'cosine':
        return MeasureShardedGallery
    return CosineFilterShardedGallery if isinstance(filter, str) and filter == "cosine" else CosineShardedGallery
