"""world_size-2 gloo rehearsal of ShardedGallery(..., measure=) on CPU: the sharded evaluation under the six
non-cosine measures of LINAS-engine/evaluation.py:17-36.

Every rank runs the PRODUCT coordination code of cmve.dist.ShardedGallery -- evaluate / cal_perf under a measure:
the caption all-gather (uneven slices), the same global-id CSR on every rank, the int64-word all-reduce(SUM) of the
item scores (each scored where its video lives), ONE counting pass, ONE all-reduce(SUM) carrying the t2v positions
and the v2t R@K sums, the v2t rank gather and the mAP reduction.  Only the shard-local arithmetic (``_pw_rows`` /
``_pw_items`` / ``_pw_count`` / ``_pw_ranks``: HIP kernels in the product, covered by the -m gpu tests) is
replaced by ``oracle.measures.cal_error`` arithmetic, so the test runs without a GPU.  Inputs and expectations are
the reference-recorded tests/golden/measures_retrieval.npz (141 videos, 150 captions, D = 67, tie-free, nine
videos with two captions); shards are cut at 100, caption slices at 83."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

MEASURES = ["euclidean", "l1", "l2", "l1_norm", "l2_norm", "jaccard"]
CUT, Q_CUT = 100, 83
NEG_ZERO = np.array([-0.0]).view(np.int64)[0]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_shard_class():
    from cmve import dist as D
    from oracle import measures as OM

    class OracleShard(D.MeasureShardedGallery):
        """ShardedGallery(measure=) whose shard-local arithmetic is the oracle (test infrastructure)."""
        count_calls = 0
        craft = None     # {item: value}: row items whose score is replaced where this shard owns them
        seen_row = None  # the merged row item scores the counting pass received

        def _pw_rows(self, x):
            x = x.numpy() if torch.is_tensor(x) else np.asarray(x)
            return torch.from_numpy(np.ascontiguousarray(x, np.float32 if self.measure == "jaccard" else np.float64))

        def _err(self, q):
            if self.n == 0:
                return np.zeros((q.shape[0], 0))
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.asarray(OM.cal_error(self.shard.numpy(), q.numpy(), self.measure), np.float64)

        def _pw_items(self, q, csr, n_items, col_dir, idx_base):
            off, idx = (t.numpy() for t in csr)
            e = self._err(q)
            out = np.zeros(n_items)
            for l in range(len(off) - 1):
                for p in range(off[l], off[l + 1]):
                    o = int(idx[p]) - idx_base
                    i, j = (o, l) if col_dir else (l, o)
                    if 0 <= i < e.shape[0] and 0 <= j < e.shape[1]:
                        out[p] = e[i, j]
                        if self.craft and not col_dir and p in self.craft:
                            out[p] = self.craft[p]
            return torch.from_numpy(out)

        def _pw_count(self, q, row, col):
            self.count_calls += 1
            e = self._err(q)
            if row is not None:
                self.seen_row = row[1].clone()

            def side(s, mat):
                if s is None:
                    return None
                off, sc, n = s[0].numpy(), s[1].numpy(), s[2]
                pos = np.zeros(sc.size, np.int32)
                for l in range(len(off) - 1):
                    nan = [p for p in range(off[l], off[l + 1]) if np.isnan(sc[p])]
                    for p in range(off[l], off[l + 1]):
                        if not np.isnan(sc[p]):
                            pos[p] = np.count_nonzero(mat[l] < sc[p])
                    for t, p in enumerate(nan):
                        pos[p] = n - len(nan) + t if n > 0 else 0
                return torch.from_numpy(pos)

            return side(row, e), side(col, e.T)

        def _pw_ranks(self, off, sc, pos, n_m):
            off, sc, pos = off.numpy(), sc.numpy(), pos.numpy().astype(np.int64)
            out = np.empty(len(off) - 1, np.int64)
            for l in range(len(off) - 1):
                p = [pos[t] for t in range(off[l], off[l + 1]) if not np.isnan(sc[t])]
                out[l] = n_m + 1 if off[l] == off[l + 1] else (min(p) + 1 if p else n_m)
            return torch.from_numpy(out)

    return OracleShard


def _worker(rank, world, port, result_q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "cross-modal-video-engine_amd"))
    sys.path.insert(0, os.path.dirname(here))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cmve import dist as D
        from oracle import measures as OM, retrieval as R
        fx = np.load(os.path.join(here, "golden", "measures_retrieval.npz"), allow_pickle=False)
        v2t, t2v = R.get_gt(list(fx["video_ids"]), list(fx["caption_ids"]))
        n_g, n_q = len(fx["video_ids"]), len(fx["caption_ids"])
        t2v_lists = [t2v[i] for i in range(n_q)]
        lo, hi = (0, CUT) if rank == 0 else (CUT, n_g)
        qlo, qhi = (0, Q_CUT) if rank == 0 else (Q_CUT, n_q)
        comm = D.TorchComm()
        Shard = _oracle_shard_class()
        ok = {}
        for m in MEASURES:
            vid, cap = (fx["vid_p"], fx["cap_p"]) if m == "jaccard" else (fx["vid"], fx["cap"])
            sh = Shard(vid[lo:hi], offset=lo, n_global=n_g, comm=comm, measure=m)
            q_local = torch.from_numpy(cap[qlo:qhi].copy())
            r_t, r_v = sh.evaluate(q_local, t2v_lists, v2t)
            ok[m + ":t2v_ranks"] = bool(np.array_equal(r_t, fx["t2v_ranks_" + m]))
            ok[m + ":v2t_ranks"] = bool(np.array_equal(r_v, fx["v2t_ranks_" + m]))
            before = sh.count_calls
            perf = sh.cal_perf(q_local, v2t, t2v)
            ok[m + ":one_count_pass"] = sh.count_calls - before == 1
            ref = fx["cal_perf_" + m]
            ok[m + ":cal_perf"] = bool(np.allclose(np.array(perf[0], float), ref[0], rtol=0, atol=1e-12)
                                       and np.allclose(np.array(perf[1], float), ref[1], rtol=0, atol=1e-12))
            # the device step: the v2t R@K sums of all shards ride the t2v positions' all-reduce
            q_all = D.all_gather_var(q_local, comm)
            t_d, v_loc, rec, ovf = sh.evaluate_device(q_all, sh.local_gt_csr(t2v_lists), sh.local_v2t_csr(v2t), n_q)
            rv = fx["v2t_ranks_" + m].astype(np.int64)
            ok[m + ":device"] = (bool(np.array_equal(t_d.numpy(), fx["t2v_ranks_" + m])) and not bool(ovf)
                                 and bool(np.array_equal(v_loc.numpy(), rv[lo:hi]))
                                 and rec.tolist() == [int((rv <= 1).sum()), int((rv <= 5).sum()),
                                                      int((rv <= 10).sum()), int(rv.sum())])
        # multi-GT t2v lists: still ONE counting pass per cal_perf, and the unsharded oracle's tuples
        vid, cap = fx["vid"], fx["cap"]
        t2v_m = {i: list(t2v[i]) + ([(7 * i + 3) % n_g] if i < 10 else []) for i in range(n_q)}
        v2t_m = [list(l) for l in v2t]
        for i in range(10):
            v2t_m[(7 * i + 3) % n_g].append(i)
        sh = Shard(vid[lo:hi], offset=lo, n_global=n_g, comm=comm, measure="l1")
        q_local = torch.from_numpy(cap[qlo:qhi].copy())
        perf = sh.cal_perf(q_local, v2t_m, t2v_m)
        exp = R.cal_perf(OM.cal_error(vid, cap, "l1"), v2t_m, t2v_m)
        ok["multi_gt:one_count_pass"] = sh.count_calls == 1
        ok["multi_gt:cal_perf"] = all(np.allclose(np.array(g, float), np.array(e, float), rtol=0, atol=1e-12)
                                      for g, e in zip(perf, exp))
        # the item-score merge: a NaN word and a -0.0 word owned by rank 0, an item owned by rank 1 only
        own0 = [i for i in range(n_q) if t2v_lists[i][0] < CUT][:2]
        own1 = next(i for i in range(n_q) if t2v_lists[i][0] >= CUT)
        assert all(len(l) == 1 for l in t2v_lists)  # item p is caption p's only GT
        sh = Shard(vid[lo:hi], offset=lo, n_global=n_g, comm=comm, measure="l1")
        sh.craft = {own0[0]: float("nan"), own0[1]: -0.0}
        r_t, _ = sh.evaluate(q_local, t2v_lists, None)
        words = sh.seen_row.numpy().view(np.int64)
        e_full = OM.cal_error(vid, cap, "l1")
        ok["merge:nan"] = bool(np.isnan(sh.seen_row[own0[0]])) and r_t[own0[0]] == n_g
        ok["merge:neg_zero"] = bool(words[own0[1]] == NEG_ZERO) and r_t[own0[1]] == 1
        ok["merge:rank1_only"] = bool(sh.seen_row[own1] == e_full[own1, t2v_lists[own1][0]] != 0.0)
        others = [i for i in range(n_q) if i not in own0]
        ok["merge:rest"] = bool(np.array_equal(r_t[others], fx["t2v_ranks_l1"][others]))
        # a GT id no shard owns
        bad = [list(l) for l in t2v_lists]
        bad[5] = [n_g]
        try:
            sh.evaluate(q_local, bad, None)
            ok["bad_gt"] = False
        except ValueError:
            ok["bad_gt"] = True
        result_q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def world2():
    world = 2
    ctx = mp.get_context("spawn")
    result_q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, result_q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0
    got = dict(result_q.get() for _ in range(world))
    assert sorted(got) == [0, 1]
    return got


@pytest.mark.parametrize("m", MEASURES)
def test_ranks_and_cal_perf_equal_the_reference_on_both_ranks(world2, m):
    for rank in (0, 1):
        ok = {k: v for k, v in world2[rank].items() if k.startswith(m + ":")}
        assert len(ok) == 5 and all(ok.values()), (rank, ok)


def test_one_counting_pass_with_multi_gt_lists(world2):
    for rank in (0, 1):
        assert world2[rank]["multi_gt:one_count_pass"] and world2[rank]["multi_gt:cal_perf"], world2[rank]


def test_item_score_merge_preserves_the_words(world2):
    for rank in (0, 1):
        ok = {k: v for k, v in world2[rank].items() if k.startswith("merge:")}
        assert len(ok) == 4 and all(ok.values()), (rank, ok)


def test_gt_id_outside_the_gallery_raises(world2):
    assert world2[0]["bad_gt"] and world2[1]["bad_gt"]
