"""Edge shapes and strided operands of the head, loss and training kernels, through the C ABI.

pool.hip (K2), loss.hip (K6 triplet, K7 InfoNCE, the fp32 MFMA GEMM K6g) and train.hip (K11) are
otherwise reached only through the Python modules: contiguous tensors at the golden files' shapes.
Here every leading dimension, base offset and NULL-able argument is the test's own, each operand is
a window of a NaN-filled buffer (an operand read past its row poisons the result; an output written
past it breaks the canary, which is checked after every call that writes), and every reference is
a few lines of numpy / torch in fp64 (fp32 where the kernel's own fp32 steps are exact to restate).
Each docstring names the path its shapes take: staging mode, split count, lane strides, vector or
scalar.
"""
import numpy as np
import pytest
import torch

from _windows import Pad, _within

pytestmark = pytest.mark.gpu

U24, U23, U53 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -53


def _api():
    from cmve import engine
    from cmve._lib import lib, check
    return engine, lib, check


# ------------------------------------------------------------------ 1. fp32 GEMM (K6g)
GT, GK = 64, 32  # loss.hip's block tile and K step


def _gemm_plan(ta, tb, M, N, K, lda, ldb, a_al, b_al):
    """gemm_f32_launch's rule restated: (float4 staging?, K slices, kslice, slices the loop chose)."""
    blocks = -(-M // GT) * -(-N // GT)
    loop = 1
    while blocks * loop * 2 <= 512 and K // (loop * 2) >= 2 * GK:
        loop *= 2
    kslice = -(-K // (loop * GK)) * GK
    splits = max(1, -(-K // kslice))
    vec = (a_al and lda % 4 == 0 and b_al and ldb % 4 == 0 and (M if ta else K) % 4 == 0
           and (K if tb else N) % 4 == 0)
    return vec, splits, kslice, loop


# name: (M, N, K, extra leading dimension, A's base offset in floats,
#        {(ta, tb): float4 staging}, K slices, kslice, slices the loop chose)
ALL4 = {(0, 0): True, (0, 1): True, (1, 0): True, (1, 1): True}
NONE4 = {k: False for k in ALL4}
GEMM_CASES = {
    "vec_partial_tiles": (68, 72, 36, 0, 0, ALL4, 1, 64, 1),
    "vec_splitk_1000": (64, 64, 1000, 0, 0, ALL4, 8, 128, 8),
    "vec_splitk_520": (64, 64, 520, 0, 0, ALL4, 6, 96, 8),
    "scalar_splitk_1001": (60, 68, 1001, 0, 0, {(0, 0): False, (0, 1): False, (1, 0): True, (1, 1): False}, 8, 128, 8),
    "scalar_splitk_1001_all": (61, 67, 1001, 0, 0, NONE4, 8, 128, 8),
    "one_float4": (4, 4, 4, 0, 0, ALL4, 1, 32, 1),
    "ld_plus_4": (128, 64, 256, 4, 0, ALL4, 4, 64, 4),
    "ld_plus_1": (128, 64, 256, 1, 0, NONE4, 4, 64, 4),
    "a_base_plus_1": (128, 64, 256, 0, 1, NONE4, 4, 64, 4),
}


def _gemm_call(ta, tb, M, N, K, A, Bm, C, bias, beta, relu):
    engine, lib, check = _api()
    check(lib.cmve_gemm_f32_ex(engine.handle(), ta, tb, M, N, K, 0.75, A.ptr, A.ld, Bm.ptr, Bm.ld, beta, C.ptr, C.ld,
                               bias.ptr if bias is not None else None, relu), "cmve_gemm_f32_ex")


@pytest.mark.parametrize("ta,tb", sorted(ALL4))
@pytest.mark.parametrize("name", sorted(GEMM_CASES))
def test_gemm_f32_staging_splitk_and_strides(name, ta, tb):
    """cmve_gemm_f32_ex against fp64 within the parent test's bound, 0.75 (|A| |B|) K 2^-24 +
    1e-6 (1 + |want|), for op(A) [M, K] . op(B) [K, N], plain epilogue (no bias, beta = 0 on a NaN C: C
    must not be read) and bias + relu + beta = 0.5.  Paths by gemm_f32_launch's rule (float4 staging
    iff both bases are 16-byte aligned, lda and ldb are multiples of 4 and so is each operand's
    contiguous extent: K or M for A, N or K for B; K slices = ceil(K / kslice), kslice = ceil(K /
    (32 loop)) 32, loop doubling while blocks loop 2 <= 512 and K / (2 loop) >= 64):
      (68, 72, 36)    4 blocks, 1 slice; float4; partial tiles in M (4), N (8) and K (4 of 32).
      (64, 64, 1000)  1 block, 8 slices of 128, the last 104; float4.
      (64, 64, 520)   1 block, the loop chooses 8, kslice 96 gives 6 slices, the last 40; float4.
      (60, 68, 1001)  2 blocks, 8 slices of 128, the last 105; scalar, as K % 4 != 0 is a contiguous
                      extent, except (transA, transB) = (1, 0) where K is contiguous in neither: float4.
      (61, 67, 1001)  the same split, scalar under all four transposes.
      (4, 4, 4)       1 block, 1 slice, a single float4 per operand row.
      (128, 64, 256)  2 blocks, 4 slices of 64: ld + 4 float4; ld + 1 scalar; A's base + 1 float scalar,
                      and bit for bit the aligned call's values (the same k-ordered chain per slice).
    """
    M, N, K, dld, aoff, vecs, splits, kslice, loop = GEMM_CASES[name]
    a_shape, b_shape = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    lda, ldb, ldc = a_shape[1] + dld, b_shape[1] + dld, N + dld
    rng = np.random.default_rng(sum(map(ord, name)) * 4 + ta * 2 + tb)
    a, b = rng.standard_normal(a_shape).astype(np.float32), rng.standard_normal(b_shape).astype(np.float32)
    bias, c0 = rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
    A, Bm = Pad(*a_shape, ld=lda, off=aoff, data=a), Pad(*b_shape, ld=ldb, data=b)
    assert A.aligned16 == (aoff == 0) and Bm.aligned16
    assert _gemm_plan(ta, tb, M, N, K, lda, ldb, A.aligned16, Bm.aligned16) == (vecs[(ta, tb)], splits, kslice, loop)
    bias_d = Pad(1, N, data=bias[None])
    ad, bd = (a.T if ta else a).astype(np.float64), (b.T if tb else b).astype(np.float64)
    for relu, beta, bp in ((0, 0.0, None), (1, 0.5, bias_d)):
        C = Pad(M, N, ld=ldc, data=c0 if beta else None)
        _gemm_call(ta, tb, M, N, K, A, Bm, C, bp, beta, relu)
        got = C.numpy()
        C.assert_canary(f"C {name}")
        want = 0.75 * (ad @ bd) + beta * c0 + (bias if bp is not None else 0.0)
        if relu:
            want = np.maximum(want, 0)
        bound = 0.75 * (np.abs(ad) @ np.abs(bd)) * K * U24 + 1e-6 * (1 + np.abs(want))
        _within(got, want, bound, f"{name} relu={relu} beta={beta}")
        if aoff:  # the aligned twin: float4 staging of the same values
            A2, C2 = Pad(*a_shape, ld=lda, data=a), Pad(M, N, ld=ldc, data=c0 if beta else None)
            assert _gemm_plan(ta, tb, M, N, K, lda, ldb, A2.aligned16, True)[0]
            _gemm_call(ta, tb, M, N, K, A2, Bm, C2, bp, beta, relu)
            assert np.array_equal(got, C2.numpy()), f"{name}: scalar and float4 staging differ"


@pytest.mark.parametrize("M,N", [(0, 5), (5, 0)])
def test_gemm_f32_empty_leaves_c(M, N):
    """M = 0 or N = 0 (K = 3): CMVE_OK before any launch, C is left as it was."""
    for ta, tb in sorted(ALL4):
        A, Bm, C = Pad(4, 8), Pad(4, 8), Pad(5, 5)
        _gemm_call(ta, tb, M, N, 3, A, Bm, C, None, 0.5, 1)
        C.assert_untouched("C of an empty product")


# ------------------------------------------------------------------ 2. temporal pool and collate (K2)
POOL_MODES = {0: "mean_valid", 1: "mean_all", 2: "max_masked_zero", 3: "max_all"}


def _pool_ref(x, lens, mode):
    """fp64 numpy over the same elements -> (want, bound); bound None = exact.  The mean bound: an
    fp32 sum of T terms in any order is within T 2^-24 sum|x| of the exact one; dividing by the count
    and rounding the quotient adds 2^-24 |want|."""
    B, T, F = x.shape
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == 0:
            want, bound = np.empty((B, F)), np.empty((B, F))
            for b in range(B):
                e = min(int(lens[b]), T)  # len > T: every step is valid
                # len = 0: np.mean of an empty slice, 0 / 0 = NaN (LINAS model.py:152-156 divides by the length)
                want[b] = x64[b, :e].sum(0) / e if e else np.nan
                bound[b] = T * U24 * np.abs(x64[b, :e]).sum(0) / max(e, 1)
            return want, bound + U24 * np.abs(want)
        if mode == 1:
            want = x64.mean(1)
            return want, T * U24 * np.abs(x64).sum(1) / T + U24 * np.abs(want)
        if mode == 2:
            mask = (np.arange(T)[None, :] < np.asarray(lens)[:, None]).astype(np.float32)
            # len = 0 over finite values: every step is x * 0 = 0, the max is 0; a masked NaN / inf is NaN * 0 = NaN
            return np.max(x * mask[:, :, None], axis=1), None
        return np.max(x, axis=1), None


def _pool_check(xt, x, lens, mode, what, ldo_extra=3):
    engine, lib, check = _api()
    B, T, F = x.shape
    out = Pad(B, F, ld=F + ldo_extra)
    lens_d = torch.from_numpy(np.asarray(lens, np.int32)).cuda() if mode in (0, 2) else None
    check(lib.cmve_temporal_pool(engine.handle(), engine._ptr(xt), xt.stride(0), xt.stride(1), B, T, F,
                                 engine._ptr(lens_d), mode, out.ptr, out.ld), "cmve_temporal_pool")
    got = out.numpy()
    out.assert_canary(f"pool out {what}")
    want, bound = _pool_ref(x, lens, mode)
    if bound is None:
        assert np.array_equal(got, want.astype(np.float32), equal_nan=True), f"{what} {POOL_MODES[mode]}"
    else:
        _within(got, want, bound, f"{what} {POOL_MODES[mode]}")
    return got


def _lens(B, T, shift):
    return np.array([0, 1, T, T + 3])[(np.arange(B) + shift) % 4]


@pytest.mark.parametrize("mode", sorted(POOL_MODES))
@pytest.mark.parametrize("B,T,F", [(3, 1, 5), (3, 2, 3), (2, 3, 1), (5, 5, 260)])
def test_pool_small_shapes_and_lengths(B, T, F, mode):
    """cmve_temporal_pool on a contiguous x, lengths cycling through 0, 1, T and T + 3, ldo = F + 3.
    Wave w takes steps w, w + 4, ...: T = 1, 2, 3 leave 3, 2, 1 waves with no step (their partial is 0
    for the means, -inf for the maxima), T = 5 gives wave 0 a second step.  F = 5, 3, 1: one lane or two,
    scalar loads with a partly filled group of 4; F = 260: float4 loads (strides and F multiples of 4,
    base aligned) and a second block in x holding one float4."""
    rng = np.random.default_rng(B * 1000 + T * 100 + F)
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    for shift in range(4 if B < 4 else 1):
        _pool_check(torch.from_numpy(x).cuda(), x, _lens(B, T, shift), mode, f"({B},{T},{F}) shift {shift}")


@pytest.mark.parametrize("mode", sorted(POOL_MODES))
def test_pool_nan_and_infinities(mode):
    """NaN, +inf and -inf at valid and at masked steps of (5, 5, 260) and, with empty waves, (4, 2, 7):
    the maxima propagate NaN from any wave (torch.max), a masked special value is x * 0 = NaN under
    MAX_MASKED_ZERO, MEAN_VALID never reads a masked step, and the means follow IEEE (inf - inf = NaN)."""
    for B, T, F in ((5, 5, 260), (4, 2, 7)):
        rng = np.random.default_rng(17 + T)
        x = rng.standard_normal((B, T, F)).astype(np.float32)
        lens = np.array([2, 1, T, T + 3, 0])[:B]
        vals = [np.nan, np.inf, -np.inf]
        for b in range(B):
            for t in range(T):  # one column per (video, step, value); step t of video b is masked iff t >= lens[b]
                for k, v in enumerate(vals):
                    x[b, t, (3 * (b * T + t) + k) % F] = v
        x[0, :, F - 1] = -np.inf          # a column that is -inf at every step
        x[1, 0, F - 2], x[1, 1, F - 2] = np.inf, -np.inf  # both infinities in one column
        _pool_check(torch.from_numpy(x).cuda(), x, lens, mode, f"specials ({B},{T},{F})")


def test_pool_no_videos():
    """B = 0: CMVE_OK without a launch (a grid of 0 blocks is a launch error), out untouched."""
    engine, lib, check = _api()
    x, out = Pad(4, 8), Pad(1, 8)
    for mode in sorted(POOL_MODES):
        lens = torch.zeros(1, dtype=torch.int32, device="cuda")
        check(lib.cmve_temporal_pool(engine.handle(), x.ptr, 8, 4, 0, 2, 4, engine._ptr(lens), mode, out.ptr, 8),
              "cmve_temporal_pool")
    torch.cuda.synchronize()
    out.assert_untouched("pool out with B = 0")


@pytest.mark.parametrize("mode", sorted(POOL_MODES))
def test_pool_float4_needs_an_aligned_base(mode):
    """x = big[:, :, 1:641] of a [4, 9, 700] tensor: both strides and F are multiples of 4 but the base
    is 4 bytes past a 16-byte boundary, so the loads must be scalar; big[:, :, 4:644] holds the same
    values on an aligned base (float4).  Both equal the reference and each other bit for bit (same
    order of additions either way)."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 9, 640)).astype(np.float32)
    lens = np.array([3, 9, 12, 0])
    res = []
    for c0 in (1, 4):
        big = torch.full((4, 9, 700), float("nan"), device="cuda")
        view = big[:, :, c0:c0 + 640]
        view.copy_(torch.from_numpy(x))
        assert big.data_ptr() % 16 == 0 and (view.data_ptr() % 16 == 0) == (c0 == 4)
        res.append(_pool_check(view, x, lens, mode, f"column {c0} view"))
    assert np.array_equal(res[0], res[1], equal_nan=True)


COLLATE_T = (1, 0, 63, 130, 64, 65)


def _collate_check(F, ldf, t_max, off=0):
    engine, lib, check = _api()
    B, total = len(COLLATE_T), sum(COLLATE_T)
    rng = np.random.default_rng(F + ldf)
    x = (rng.standard_normal((total, F)) + 0.5).astype(np.float32)
    frames = Pad(total, F, ld=ldf, off=off, data=x)
    assert frames.aligned16 == (off == 0)
    offs = np.concatenate([[0], np.cumsum(COLLATE_T)]).astype(np.int64)
    videos, origin, mask = Pad(B * t_max, F), Pad(B, F), Pad(B, t_max)
    check(lib.cmve_collate_frames(engine.handle(), frames.ptr, frames.ld, engine._ptr(torch.from_numpy(offs).cuda()),
                                  B, F, 64, t_max, videos.ptr, origin.ptr, mask.ptr), "cmve_collate_frames")
    got_v, got_o, got_m = videos.numpy().reshape(B, t_max, F), origin.numpy(), mask.numpy()
    for p, n in ((videos, "videos"), (origin, "origin"), (mask, "mask")):
        p.assert_canary(f"collate {n} F={F} ldf={ldf} t_max={t_max}")
    want_v, want_m = np.zeros((B, t_max, F), np.float32), np.zeros((B, t_max), np.float32)
    want_o, bound_o = np.empty((B, F)), np.zeros((B, F))
    for b, T in enumerate(COLLATE_T):
        f = x[offs[b]:offs[b + 1]]
        keep = min(T, 64)
        want_v[b, :keep], want_m[b, :keep] = f[:keep], 1.0
        # no frames: the mean of nothing, 0 / 0 = NaN (tag_data_provider.py:104 is np.mean over the frames)
        want_o[b] = f.astype(np.float64).sum(0) / T if T else np.nan
        # fp32 sum over ALL T frames in any order, then one rounded division
        bound_o[b] = T * U24 * np.abs(f.astype(np.float64)).sum(0) / max(T, 1)
    assert np.array_equal(got_v, want_v) and np.array_equal(got_m, want_m)
    _within(got_o, want_o, bound_o + U24 * np.abs(want_o), f"origin F={F} ldf={ldf}")
    return got_v, got_o


@pytest.mark.parametrize("t_max", [64, 70])
@pytest.mark.parametrize("dld", [2, 4])
@pytest.mark.parametrize("F", [1030, 4096])
def test_collate_wide_rows_padded_frames(F, dld, t_max):
    """cmve_collate_frames, max_len 64, videos of 1, 0, 63, 130, 64 and 65 frames (T_b above and below 64
    in one call; the longest kept length is 64, so t_max = 64 is tight and 70 pads every video), rows
    of ldf = F + 2 / F + 4 floats.  F = 4096 (LINAS): 4 blocks in x, float4 loads with ldf = F + 4, scalar
    with F + 2.  F = 1030: 2 blocks in x, the second holding 6 features in two lanes, scalar loads
    (F % 4 != 0) with the last group of 4 half filled.  origin averages ALL T_b frames; NaN for the empty
    video, whose videos / mask rows are zero."""
    _collate_check(F, F + dld, t_max)


def test_collate_float4_needs_an_aligned_base():
    """F = 4096, ldf = F + 4, frames' base one float past a 16-byte boundary: scalar loads; the values
    equal the aligned call's bit for bit (the same sum over t per feature)."""
    v1, o1 = _collate_check(4096, 4100, 64, off=1)
    v0, o0 = _collate_check(4096, 4100, 64, off=0)
    assert np.array_equal(v1, v0) and np.array_equal(o1, o0, equal_nan=True)


# ------------------------------------------------------------------ 3. InfoNCE (K7)
def _unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.mark.parametrize("B", [1, 3, 65, 130])
def test_infonce_edges_directly_on_ds(B):
    """cmve_infonce_fwd / _bwd on S = P . T^T of unit rows in 4 dimensions (scale 100: logits over about
    +-100), ld = B + 5, ldd = B + 3, g = 0.7, dir 1 / 2 / 3, scale 100 and 1.  One wave per row, 4 rows per
    block: B = 1, 3, 65, 130 all leave `r >= B` waves in the last block; B = 65 and 130 give lanes 0 and
    0..1 a second and a third stride of the lane loop (k = lane + 64, + 128).  Reference in fp64 from the
    fp32 product t * S_ij as the kernel forms it; lse = max + log(sum(exp(x - max))).  Bounds: lse 1e-12;
    loss 2^-23 |want|; dS 2^-23 |want| + 1e-14 |g t / B| (one rounding of an fp64 chain, the absolute
    term for the cancellation at the diagonal)."""
    engine, lib, check = _api()
    rng = np.random.default_rng(B)
    S = (_unit_rows(rng, B, 4) @ _unit_rows(rng, B, 4).T).astype(np.float32)
    Sd = Pad(B, B, ld=B + 5, data=S)
    g32 = np.float32(0.7)
    g = torch.full((1,), 0.7, dtype=torch.float32, device="cuda")
    eye = np.eye(B)
    for scale in (100.0, 1.0):
        t32 = np.float32(scale)
        X = (t32 * S).astype(np.float64)  # the fp32 product, then fp64
        assert scale != 100.0 or B < 65 or (X.max() > 90 and X.min() < -90)

        def lse(axis):
            m = X.max(axis, keepdims=True)
            return (m + np.log(np.exp(X - m).sum(axis, keepdims=True))).squeeze(axis)
        want_lse = {1: lse(1), 2: lse(0)}
        want_mean = {d: float(np.mean(want_lse[d] - np.diag(X))) for d in (1, 2)}
        for dr in (1, 2, 3):
            loss3 = Pad(1, 3)
            lses = {1: Pad(1, B, dtype=torch.float64), 2: Pad(1, B, dtype=torch.float64)}
            per = {1: Pad(1, B), 2: Pad(1, B)}
            check(lib.cmve_infonce_fwd(engine.handle(), Sd.ptr, Sd.ld, B, scale, dr, loss3.ptr, lses[1].ptr,
                                       lses[2].ptr, per[1].ptr, per[2].ptr), "cmve_infonce_fwd")
            got3 = loss3.numpy()[0].astype(np.float64)
            for p in (loss3, lses[1], lses[2], per[1], per[2]):
                p.assert_canary(f"infonce_fwd B={B} dir={dr}")
            tag = f"B={B} scale={scale} dir={dr}"
            for d in (1, 2):
                if dr & d:
                    _within(lses[d].numpy()[0], want_lse[d], 1e-12, f"lse[{d}] {tag}")
                    _within(got3[d - 1], want_mean[d], U23 * abs(want_mean[d]), f"loss3[{d - 1}] {tag}")
                else:  # the unused direction is neither written nor read
                    lses[d].assert_untouched(f"lse[{d}] {tag}")
                    per[d].assert_untouched(f"per-row loss[{d}] {tag}")
            want = {1: want_mean[1], 2: want_mean[2], 3: 0.5 * (want_mean[1] + want_mean[2])}[dr]
            _within(got3[2], want, U23 * abs(want), f"loss3[2] {tag}")

            dS = Pad(B, B, ld=B + 3)
            check(lib.cmve_infonce_bwd(engine.handle(), Sd.ptr, Sd.ld, B, scale, dr, engine._ptr(g),
                                       lses[1].ptr if dr & 1 else None, lses[2].ptr if dr & 2 else None, dS.ptr,
                                       dS.ld), "cmve_infonce_bwd")
            got = dS.numpy()
            dS.assert_canary(f"infonce dS {tag}")
            w = 0.5 if dr == 3 else 1.0
            v = np.zeros((B, B))
            if dr & 1:
                v += w * (np.exp(X - want_lse[1][:, None]) - eye)
            if dr & 2:
                v += w * (np.exp(X - want_lse[2][None, :]) - eye)
            gt = float(g32) * float(t32)
            want_ds = gt * v / B
            _within(got, want_ds, U23 * np.abs(want_ds) + 1e-14 * abs(gt / B), f"dS {tag}")


# ------------------------------------------------------------------ 4. triplet (K6)
MARGIN = np.float32(0.2)


def _triplet_scores(B):
    """S on the grid of multiples of 2^-6 in [-1, 1] (ties are frequent and margin + S_ij - S_dd is the
    same two fp32 roundings in numpy and on the device), with planted rows / columns.  Returns S and
    the planted facts {name: (axis, line, expected first argmax, the later tied index)}."""
    rng = np.random.default_rng(100 + B)
    S = (rng.integers(-64, 65, (B, B)) / 64.0).astype(np.float32)
    ties, zero, hinge = {}, None, None
    if B >= 66:
        # tied maxima: (first, later) 65 apart in lanes 0 / 1; 64 apart in one lane (second stride of the
        # lane loop); and 59 apart with the first index in the HIGHER lane (5 against 64 -> lane 0)
        plan = {"row2": (1, 2, 0, 65), "row3": (1, 3, 1, 65), "row4": (1, 4, 5, 64), "col6": (0, 6, 0, 65),
                "col7": (0, 7, 5, 64)}
        zero, hinge = 8, (9, 10)
    elif B >= 5:
        plan = {"row0": (1, 0, 1, B - 1), "col2": (0, 2, 0, B - 1)}
        zero, hinge = 3, (1, 4)
    else:
        plan = {}
    for name, (axis, line, first, later) in plan.items():
        if axis == 1:
            S[line, :] = np.minimum(S[line, :], 0.5)
            S[line, first] = S[line, later] = 1.0
        else:
            S[:, line] = np.minimum(S[:, line], 0.5)
            S[first, line] = S[later, line] = 1.0
        S[line, line] = 0.0
        ties[name] = (axis, line, first, later)
    if zero is not None:  # a row and a column whose costs are all zero: margin + x - 1 <= -0.05
        S[zero, :] = np.minimum(S[zero, :], 0.75)
        S[:, zero] = np.minimum(S[:, zero], 0.75)
        S[zero, zero] = 1.0
    if hinge is not None:  # an exact hinge boundary: (margin + S_ij) - S_ii == 0, where clamp's gradient passes
        i, j = hinge
        S[i, i] = MARGIN + S[i, j]
    return S, ties, zero, hinge


def _triplet_ref(S, mv, mean, dr, g32):
    """loss.py:127-153 in numpy float32: ((margin + S) - d).clamp(0), zero diagonal, max (first index)
    or sum; the backward as autograd routes it (clamp passes where its argument >= 0)."""
    B = S.shape[0]
    d, eye, idx = np.diag(S).copy(), np.eye(B, dtype=bool), np.arange(B)
    pre = {1: (MARGIN + S) - d[:, None], 2: (MARGIN + S) - d[None, :]}
    cost = {k: np.where(eye, np.float32(0), np.maximum(p, np.float32(0))) for k, p in pre.items()}
    assert all(c.dtype == np.float32 for c in cost.values())
    axis = {1: 1, 2: 0}
    arg = {k: np.argmax(cost[k], axis=axis[k]) for k in (1, 2)}
    val = {k: cost[k].max(axis=axis[k]) for k in (1, 2)}
    rowsum = {k: cost[k].astype(np.float64).sum(axis=axis[k]) for k in (1, 2)}
    one = np.float32(1)
    wscale = (one / np.float32(B) if mv else one / (np.float32(B) * np.float32(B))) if mean else one
    scale = (1.0 / B if mv else 1.0 / (B * B)) if mean else 1.0
    total = sum((val[k].astype(np.float64).sum() if mv else rowsum[k].sum()) for k in (1, 2) if dr & k)
    off, diag = np.zeros((B, B), np.int64), np.zeros(B, np.int64)
    for k in (1, 2):
        if not dr & k:
            continue
        act = (pre[k] >= 0) & ~eye
        if mv:
            act &= (idx[None, :] == arg[1][:, None]) if k == 1 else (idx[:, None] == arg[2][None, :])
        off += act
        diag += act.sum(axis=axis[k])
    gr = g32 * wscale
    dS = gr * off.astype(np.float32)
    dS[idx, idx] = -(gr * diag.astype(np.float32))
    assert dS.dtype == np.float32
    return dict(pre=pre, cost=cost, arg=arg, val=val, rowsum=rowsum, loss=total * scale, dS=dS)


@pytest.mark.parametrize("B", [1, 5, 66, 130])
def test_triplet_ties_boundaries_and_strides(B):
    """cmve_triplet_fwd / _bwd, ld = B + 7, ldd = B + 1, margin 0.2, g = 0.7, every (max_violation,
    mean_style, dir).  One wave per row / column, lane loop k = lane, lane + 64, lane + 128: B = 1 and 5
    use one stride and part of a wave, B = 66 two lanes' second stride, B = 130 a third.  Required: arg
    and val element for element under max_violation (first index on ties, within a lane and across
    lanes), dS element for element in every mode (g w times small integers), the loss within
    B 2^-24 sum|c| (scaled as the loss is) of the fp64 sum of the fp32 costs; without max_violation
    val holds the row sums (fp32, any order: B 2^-24 sum|c|) and arg is -1."""
    engine, lib, check = _api()
    S, ties, zero, hinge = _triplet_scores(B)
    g32 = np.float32(0.7)
    # before any GPU call: the generator really holds what this test is about
    base = _triplet_ref(S, 1, 0, 3, g32)
    if B >= 5:
        assert ties and zero is not None and hinge is not None
        for name, (axis, line, first, later) in ties.items():
            c = base["cost"][1][line, :] if axis == 1 else base["cost"][2][:, line]
            k = 1 if axis == 1 else 2
            assert c[first] == c[later] == c.max() > 0 and base["arg"][k][line] == first, name
        assert not base["cost"][1][zero].any() and not base["cost"][2][:, zero].any()
        assert base["arg"][1][zero] == 0 and base["arg"][2][zero] == 0
        i, j = hinge
        assert base["pre"][1][i, j] == 0.0
    if B >= 66:  # a tie across the 64-column stride of one lane, and across lanes further than 64 apart
        assert any(l - f == 64 for _, _, f, l in ties.values()) and any(l - f > 64 for _, _, f, l in ties.values())
    Sd = Pad(B, B, ld=B + 7, data=S)
    g = torch.full((1,), 0.7, dtype=torch.float32, device="cuda")
    for mv in (1, 0):
        for mean in (0, 1):
            for dr in (1, 2, 3):
                tag = f"B={B} mv={mv} mean={mean} dir={dr}"
                ref = _triplet_ref(S, mv, mean, dr, g32)
                loss = Pad(1, 1)
                val = {1: Pad(1, B), 2: Pad(1, B)}
                arg = {1: Pad(1, B, dtype=torch.int32), 2: Pad(1, B, dtype=torch.int32)}
                check(lib.cmve_triplet_fwd(engine.handle(), Sd.ptr, Sd.ld, B, float(MARGIN), mv, dr, mean, loss.ptr,
                                           val[1].ptr, arg[1].ptr, val[2].ptr, arg[2].ptr), "cmve_triplet_fwd")
                got_loss = float(loss.numpy()[0, 0])
                for p in (loss, val[1], val[2], arg[1], arg[2]):
                    p.assert_canary(f"triplet_fwd {tag}")
                for k in (1, 2):
                    if not dr & k:
                        val[k].assert_untouched(f"val[{k}] {tag}")
                        arg[k].assert_untouched(f"arg[{k}] {tag}")
                    elif mv:
                        assert np.array_equal(arg[k].numpy()[0], ref["arg"][k]), f"arg[{k}] {tag}"
                        assert np.array_equal(val[k].numpy()[0], ref["val"][k]), f"val[{k}] {tag}"
                    else:
                        assert (arg[k].numpy() == -1).all(), f"arg[{k}] {tag}"
                        _within(val[k].numpy()[0], ref["rowsum"][k], B * U24 * ref["rowsum"][k], f"val[{k}] {tag}")
                _within(got_loss, ref["loss"], B * U24 * abs(ref["loss"]), f"loss {tag}")  # c >= 0: sum|c| scaled = loss

                dS = Pad(B, B, ld=B + 1)
                check(lib.cmve_triplet_bwd(engine.handle(), Sd.ptr, Sd.ld, B, float(MARGIN), mv, dr, mean,
                                           engine._ptr(g), arg[1].ptr if mv and dr & 1 else None,
                                           arg[2].ptr if mv and dr & 2 else None, dS.ptr, dS.ld), "cmve_triplet_bwd")
                got = dS.numpy()
                dS.assert_canary(f"triplet dS {tag}")
                assert np.array_equal(got, ref["dS"]), \
                    f"dS {tag}: {int((got != ref['dS']).sum())} differ, first at {np.argwhere(got != ref['dS'])[:3]}"


# ------------------------------------------------------------------ 5. K11 column and row kernels
ND = [(2, 1), (3, 15), (17, 16), (40, 33), (5, 200)]


def _nd_data(n, d, seed):
    rng = np.random.default_rng(seed * 1000 + n * 7 + d)
    return (3 * rng.standard_normal((n, d)) + 1).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)


@pytest.mark.parametrize("n,d", ND)
def test_col_sum_padded(n, d):
    """cmve_col_sum, ldx = d + 3: blocks of 16 columns x 16 row groups (rows grp, grp + 16, ...).  d = 1,
    15: one partly filled column block; 16: exactly one; 33: a third block with one column; n = 2, 3, 5:
    most row groups empty; n = 17, 40: a second and third row per group.  fp64 column sums rounded once:
    2^-23 |want| + n 2^-53 sum|x|."""
    engine, lib, check = _api()
    x, _ = _nd_data(n, d, 1)
    X, out = Pad(n, d, ld=d + 3, data=x), Pad(1, d)
    check(lib.cmve_col_sum(engine.handle(), X.ptr, X.ld, n, d, out.ptr), "cmve_col_sum")
    got = out.numpy()[0]
    out.assert_canary("col_sum out")
    x64 = x.astype(np.float64)
    want = x64.sum(0)
    _within(got, want, U23 * np.abs(want) + n * U53 * np.abs(x64).sum(0), f"col_sum ({n},{d})")


@pytest.mark.parametrize("n,d", ND)
def test_l2norm_bwd_padded(n, d):
    """cmve_l2norm_bwd, every leading dimension d + 3: one wave per row, 4 rows per block (n = 2, 3, 5,
    17: `r >= n` waves in the last block), lane loop k = lane, lane + 64: d = 1, 15, 16, 33 fill part of
    a wave once, d = 200 three strides and 8 lanes of a fourth.  Closed form in fp64, per element within
    2^-23 (|dy| / |x| + |x_k| |<x, dy>| / |x|^3)."""
    engine, lib, check = _api()
    x, dy = _nd_data(n, d, 2)
    X, DY, DX = Pad(n, d, ld=d + 3, data=x), Pad(n, d, ld=d + 3, data=dy), Pad(n, d, ld=d + 3)
    check(lib.cmve_l2norm_bwd(engine.handle(), X.ptr, X.ld, DY.ptr, DY.ld, n, d, DX.ptr, DX.ld), "cmve_l2norm_bwd")
    got = DX.numpy()
    DX.assert_canary("l2norm_bwd dx")
    x64, g64 = x.astype(np.float64), dy.astype(np.float64)
    nrm = np.sqrt((x64 * x64).sum(1, keepdims=True))
    xg = (x64 * g64).sum(1, keepdims=True)
    want = g64 / nrm - x64 * xg / nrm ** 3
    _within(got, want, U23 * (np.abs(g64) / nrm + np.abs(x64) * np.abs(xg) / nrm ** 3), f"l2norm_bwd ({n},{d})")


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("n,d", ND)
def test_bn_train_padded_and_null_arguments(n, d, given):
    """cmve_bn_train_fwd / _bwd, every leading dimension d + 3, the column-block / row-group cases of
    test_col_sum_padded; gamma, beta and the running statistics given, or all NULL (gamma 1, beta 0, no
    running update); the backward once with dx and once with dx NULL, where dgamma / dbeta are still
    written.  Reference: torch BatchNorm1d in double, with test_batchnorm_train_matches_torch's
    tolerances (y 1e-5 / 2e-5, dx 1e-4 / 2e-5, running 1e-5 / 1e-6, dgamma 1e-4 / 1e-4, dbeta 1e-5 / 1e-5);
    save_mean / save_invstd are fp64 values rounded once: 2^-23 |want| + 2^-53 sum|x|."""
    engine, lib, check = _api()
    eps, mom = 1e-5, 0.1
    x, dy = _nd_data(n, d, 3)
    rng = np.random.default_rng(n + d)
    gamma, beta = rng.uniform(0.5, 1.5, d).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    rm0, rv0 = rng.standard_normal(d).astype(np.float32), rng.uniform(0.5, 2.0, d).astype(np.float32)
    ref = torch.nn.BatchNorm1d(d, eps=eps, momentum=mom, affine=given).double().train()
    with torch.no_grad():
        if given:
            ref.weight.copy_(torch.from_numpy(gamma))
            ref.bias.copy_(torch.from_numpy(beta))
            ref.running_mean.copy_(torch.from_numpy(rm0))
            ref.running_var.copy_(torch.from_numpy(rv0))
    xr = torch.from_numpy(x).double().requires_grad_(True)
    yr = ref(xr)
    (yr * torch.from_numpy(dy).double()).sum().backward()

    X, Y = Pad(n, d, ld=d + 3, data=x), Pad(n, d, ld=d + 3)
    G, Bt = (Pad(1, d, data=gamma[None]), Pad(1, d, data=beta[None])) if given else (None, None)
    RM, RV = (Pad(1, d, data=rm0[None]), Pad(1, d, data=rv0[None])) if given else (None, None)
    SM, SI = Pad(1, d), Pad(1, d)
    ptr = lambda p: p.ptr if p is not None else None  # noqa: E731
    check(lib.cmve_bn_train_fwd(engine.handle(), X.ptr, X.ld, n, d, ptr(G), ptr(Bt), eps, mom, ptr(RM), ptr(RV),
                                Y.ptr, Y.ld, SM.ptr, SI.ptr), "cmve_bn_train_fwd")
    y = torch.from_numpy(Y.numpy()).double()
    for p in (Y, SM, SI) + ((RM, RV) if given else ()):
        p.assert_canary(f"bn fwd ({n},{d})")
    torch.testing.assert_close(y, yr.detach(), rtol=1e-5, atol=2e-5)
    x64 = x.astype(np.float64)
    mean, var = x64.mean(0), x64.var(0)
    noise = U53 * np.abs(x64).sum(0)
    _within(SM.numpy()[0], mean, U23 * np.abs(mean) + noise, "save_mean")
    inv = 1.0 / np.sqrt(var + eps)
    _within(SI.numpy()[0], inv, U23 * inv + noise, "save_invstd")
    if given:
        torch.testing.assert_close(torch.from_numpy(RM.numpy()[0]).double(), ref.running_mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(torch.from_numpy(RV.numpy()[0]).double(), ref.running_var, rtol=1e-5, atol=1e-6)

    DY = Pad(n, d, ld=d + 3, data=dy)
    want_dg = ref.weight.grad if given else (torch.from_numpy(dy).double() * (yr.detach())).sum(0)  # gamma 1, beta 0: y = xhat
    want_db = ref.bias.grad if given else torch.from_numpy(dy).double().sum(0)
    for with_dx in (True, False):
        DX, DG, DB = (Pad(n, d, ld=d + 3) if with_dx else None), Pad(1, d), Pad(1, d)
        check(lib.cmve_bn_train_bwd(engine.handle(), DY.ptr, DY.ld, X.ptr, X.ld, n, d, ptr(G), eps, ptr(DX),
                                    d + 3, DG.ptr, DB.ptr), "cmve_bn_train_bwd")
        dg, db = torch.from_numpy(DG.numpy()[0]).double(), torch.from_numpy(DB.numpy()[0]).double()
        DG.assert_canary("bn dgamma")
        DB.assert_canary("bn dbeta")
        torch.testing.assert_close(dg, want_dg, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(db, want_db, rtol=1e-5, atol=1e-5)
        if with_dx:
            dx = torch.from_numpy(DX.numpy()).double()
            DX.assert_canary("bn dx")
            torch.testing.assert_close(dx, xr.grad, rtol=1e-4, atol=2e-5)
