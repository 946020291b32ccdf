"""Edge shapes and strided operands of the MultiFusion Combiner's kernels, through the C ABI.

fusion.hip (K8 LayerNorm / one-query attention / fuse_combine, K9b absorbed attention, the block transposes
and fused packers) and ctrain.hip (K16: activations, training LayerNorm, attention backward, combine,
mean-pool backward) are otherwise reached only through Combiner and CombinerTrainer: contiguous tensors,
d = 640, H = 8, npix = 16, C = d, v_off = d.  Here every leading dimension, base offset and NULL-able
argument is the test's own, each operand is a window of a NaN-filled buffer (an operand read past its row
poisons the result; an output written past it breaks the canary, which is checked after every call that
writes), and every reference is a few lines of fp64 numpy / torch (fp32 where the kernel's own fp32 steps
are exact to restate).  Each docstring names the path its shapes take and where its bound comes from.
A rejected call must return its status, leave every output all-canary and be followed by a valid call.
"""
import ctypes

import numpy as np
import pytest
import torch

from _windows import Pad, _within

pytestmark = pytest.mark.gpu

U24, U53 = 2.0 ** -24, 2.0 ** -53
E_INVALID, E_UNSUPPORTED = -1, -3
F32 = np.float32


def _api():
    from cmve import engine
    from cmve._lib import lib, check
    return engine, lib, check


def _p(pad):
    return pad.ptr if pad is not None else None


def _rejected(status, code, rule, outs, what):
    """Nonzero status (the documented code), the rule named by cmve_last_error, every output all-canary."""
    _, lib, _ = _api()
    assert status != 0, f"{what}: accepted"
    assert code is None or status == code, f"{what}: status {status}, expected {code}"
    msg = lib.cmve_last_error().decode(errors="replace")
    assert rule in msg, f"{what}: cmve_last_error() = {msg!r} does not name {rule!r}"
    torch.cuda.synchronize()
    for o in outs:
        o.assert_untouched(f"{what}: an output")


def _one_rounding(want, rel=1e-9, abs_=1e-9):
    """An fp64 value rounded once to fp32: half an ulp, 2^-24 |want|, plus the fp64 chains' own slack."""
    return U24 * np.abs(want) + rel * np.abs(want) + abs_


# ------------------------------------------------------------------ 1. cmve_mha_1q / cmve_mha_1q_bwd
def _mha_path(d, H, dh, T):
    """cmve_mha_1q's dispatch restated."""
    E = d // 64
    lph = dh // E if (d % 64 == 0 and E > 0 and dh % E == 0) else 0
    if E in (4, 8, 10, 16) and lph in (1, 2, 4, 8, 16) and 4 * (H * T + 4 * d) <= 65536:
        return f"rows<{E}> lph {lph}"
    return "fallback"


def _mha_ref(q, k, v, B, T, H, dh, g=None, dtype=torch.float64):
    """test_mha_1q_backward_vs_torch's softmax attention: keys / values at rows t*B + b, scaling dh^-0.5.
    -> out [B, d] (and dq, dk, dv for an upstream gradient g), computed in `dtype` on the CPU."""
    d = H * dh
    grad = g is not None
    q_, k_, v_ = (torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(grad) for a in (q, k, v))
    kk = k_.reshape(T, B, H, dh).permute(1, 2, 0, 3)  # [B, H, T, dh]
    vv = v_.reshape(T, B, H, dh).permute(1, 2, 0, 3)
    qq = q_.reshape(B, H, 1, dh) / dh ** 0.5
    p = torch.softmax(qq @ kk.transpose(-1, -2), dim=-1)
    out = (p @ vv).reshape(B, d)
    if not grad:
        return out.double().numpy()
    out.backward(torch.from_numpy(g).to(dtype))
    return tuple(t.detach().double().numpy() for t in (out, q_.grad, k_.grad, v_.grad))


def _mha_data(B, T, d, seed):
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*s, generator=gen).numpy() for s in ((B, d), (T * B, d), (T * B, d), (B, d)))


def _mha_geom(d, strided, gap):
    """(ldq, ldo / lddo, v_off, ldkv, base offset, lddq): contiguous as the Combiner calls it, or every
    leading dimension padded, V `gap` columns after K and every base one float past a 16-byte boundary."""
    if not strided:
        return d, d, d, 2 * d, 0, d
    v_off = d + gap
    return d + 3, d + 5, v_off, v_off + d + 7, 1, d + 2


def _kv_window(k, v, d, v_off):
    w = np.full((k.shape[0], v_off + d), np.nan, F32)  # the gap between K and V stays NaN
    w[:, :d], w[:, v_off:] = k, v
    return w


def _mha_fwd(q, k, v, B, T, H, dh, strided=False, gap=4):
    engine, lib, check = _api()
    d = H * dh
    ldq, ldo, v_off, ldkv, off, _ = _mha_geom(d, strided, gap)
    Q, O = Pad(B, d, ld=ldq, off=off, data=q), Pad(B, d, ld=ldo, off=off)
    KV = Pad(T * B, v_off + d, ld=ldkv, off=off, data=_kv_window(k, v, d, v_off))
    check(lib.cmve_mha_1q(engine.handle(), Q.ptr, Q.ld, KV.ptr, KV.ld, v_off, B, T, H, dh, O.ptr, O.ld), "cmve_mha_1q")
    got = O.numpy()
    O.assert_canary(f"mha_1q out ({B},{T},{H},{dh}) strided={strided}")
    return got


# name: (d, H, dh, B, T, path).  atol 2e-5 is test_mha_1q_backward_vs_torch's (the same randn inputs; the
# scores q.k / sqrt(dh) are ~N(0, 1) at every dh); the shapes that test does not have were measured: the same
# formula in fp32 torch on the CPU against fp64 is off by at most 2.1e-7 (dh300), 3.0e-7 (lds_at_limit) and
# 2.3e-7 (lds_over_limit) -- four times that is below 2e-5, which therefore stands for all of them.
MHA_FWD = {
    "E4_lph16": (256, 4, 64, 3, 9, "rows<4> lph 16"),
    "E4_lph1": (256, 64, 4, 3, 9, "rows<4> lph 1"),
    "E8_lph4": (512, 16, 32, 3, 9, "rows<8> lph 4"),
    "E16_lph2": (1024, 32, 32, 3, 9, "rows<16> lph 2"),
    "E10_lph8": (640, 8, 80, 3, 9, "rows<10> lph 8"),
    "E10_lph2": (640, 32, 20, 3, 9, "rows<10> lph 2"),
    "lds_at_limit": (256, 64, 4, 2, 240, "rows<4> lph 1"),
    "lds_over_limit": (256, 64, 4, 2, 241, "fallback"),
    "dh300": (300, 1, 300, 3, 9, "fallback"),
    "dh33": (66, 2, 33, 3, 9, "fallback"),
    "dh33_T1": (66, 2, 33, 3, 1, "fallback"),
    "dh33_T2": (66, 2, 33, 3, 2, "fallback"),
    "dh33_T3": (66, 2, 33, 3, 3, "fallback"),
    "dh33_T65": (66, 2, 33, 3, 65, "fallback"),
    "dh33_B1": (66, 2, 33, 1, 9, "fallback"),
    "rows_T1": (640, 8, 80, 3, 1, "rows<10> lph 8"),
    "rows_T2": (640, 8, 80, 3, 2, "rows<10> lph 8"),
    "rows_T3": (640, 8, 80, 3, 3, "rows<10> lph 8"),
    "rows_T65_B1": (640, 8, 80, 1, 65, "rows<10> lph 8"),
}
MHA_ATOL = 2e-5


@pytest.mark.parametrize("name", sorted(MHA_FWD))
def test_mha_1q_paths_and_strides(name):
    """cmve_mha_1q against fp64 softmax attention, atol 2e-5 (see MHA_FWD), once as the Combiner calls it
    (contiguous, v_off = d, ldkv = 2d) and twice strided: ldq = d + 3, ldo = d + 5, ldkv = v_off + d + 7 with
    v_off = d + 4 and d + 1 (NaN between K and V), every base one float past a 16-byte boundary.  A strided
    call runs the same kernel in the same order: bit for bit the contiguous call's values.  Paths by the
    dispatch rule (rows kernel for E = d / 64 in {4, 8, 10, 16}, lph = dh / E in {1, 2, 4, 8, 16} and
    4 (H T + 4 d) <= 65536, else one block per (b, h)):
      E4_lph16 .. E10_lph2   mha_1q_rows_kernel<4 / 8 / 16 / 10>, every DPP stage count of group_sum_f32
                             (lph 1: none; 2; 4; 8; 16: all four), B = 3, T = 9 (wave 0 takes 3 keys, the others 2)
      lds_at_limit / over    (256, 64, 4): 64 T + 1024 floats is exactly 64 KiB at T = 240 (rows kernel) and past
                             it at 241 (fallback, 64 x 2 blocks)
      dh300                  fallback with dh > 256: the `tid` loops take a second trip
      dh33*                  fallback, d % 64 != 0; T = 1 (softmax of one key: the output is the value row,
                             bit for bit), T = 2, 3 (waves with no key), T = 65 (lane 0's second softmax
                             stride), B = 1
      rows_T*                the rows kernel at T = 1 (bit for bit the value row), 2, 3, and T = 65 with B = 1
    """
    d, H, dh, B, T, path = MHA_FWD[name]
    assert _mha_path(d, H, dh, T) == path
    q, k, v, _ = _mha_data(B, T, d, sum(map(ord, name)))
    want = _mha_ref(q, k, v, B, T, H, dh)
    got = _mha_fwd(q, k, v, B, T, H, dh)
    _within(got, want, MHA_ATOL, f"{name} contiguous")
    if T == 1:
        assert np.array_equal(got, v[:B]), f"{name}: one key, the output must be its value row"
    for gap in (4, 1):
        gs = _mha_fwd(q, k, v, B, T, H, dh, strided=True, gap=gap)
        assert np.array_equal(gs, got), f"{name}: strided (v_off = d + {gap}) differs from contiguous"


def test_mha_1q_rejects_v_inside_k_and_short_rows():
    """v_off < d (V would overlap K) and ldkv < v_off + d (a V row would run into the next row) are
    CMVE_E_INVALID, as in cmve_mha_1q_bwd; so is ldq < d.  Nothing is launched; a valid call follows."""
    engine, lib, check = _api()
    d, H, dh, B, T = 66, 2, 33, 3, 2
    q, k, v, _ = _mha_data(B, T, d, 7)
    Q, KV = Pad(B, d, data=q), Pad(T * B, 2 * d + 8, data=_kv_window(k, v, d, d + 8))
    for what, ldq, ldkv, v_off in (("v_off < d", d, KV.ld, d - 1), ("ldkv < v_off + d", d, 2 * d + 7, d + 8),
                                   ("ldkv < v_off + d at v_off = d", d, 2 * d - 1, d), ("ldq < d", d - 1, KV.ld, d)):
        O = Pad(B, d)
        st = lib.cmve_mha_1q(engine.handle(), Q.ptr, ldq, KV.ptr, ldkv, v_off, B, T, H, dh, O.ptr, O.ld)
        _rejected(st, E_INVALID, "cmve_mha_1q", [O], what)
    _within(_mha_fwd(q, k, v, B, T, H, dh), _mha_ref(q, k, v, B, T, H, dh), MHA_ATOL, "the valid call after")


def _mha_bwd(q, k, v, g, B, T, H, dh, strided=False, gap=4):
    engine, lib, check = _api()
    d = H * dh
    ldq, lddo, v_off, ldkv, off, lddq = _mha_geom(d, strided, gap)
    lddkv = v_off + d + (9 if strided else 0)
    Q, G = Pad(B, d, ld=ldq, off=off, data=q), Pad(B, d, ld=lddo, off=off, data=g)
    KV = Pad(T * B, v_off + d, ld=ldkv, off=off, data=_kv_window(k, v, d, v_off))
    DQ, DKV = Pad(B, d, ld=lddq, off=off), Pad(T * B, v_off + d, ld=lddkv, off=off)
    check(lib.cmve_mha_1q_bwd(engine.handle(), Q.ptr, Q.ld, KV.ptr, KV.ld, v_off, B, T, H, dh, G.ptr, G.ld, DQ.ptr,
                              DQ.ld, DKV.ptr, DKV.ld), "cmve_mha_1q_bwd")
    dq, dkv = DQ.numpy(), DKV.numpy()
    DQ.assert_canary("mha_1q_bwd dq")
    DKV.assert_canary("mha_1q_bwd dkv")
    assert np.isnan(dkv[:, d:v_off]).all(), "the columns of dkv between the K and V gradients were written"
    return dq, dkv[:, :d], dkv[:, v_off:]


def _close(got, want, rtol, atol, what):
    _within(got, want, atol + rtol * np.abs(want), what)


MHA_BWD = [(3, 1, 2, 33), (3, 2, 2, 33), (3, 3, 2, 33), (3, 9, 8, 80), (1, 65, 1, 300)]


@pytest.mark.parametrize("B,T,H,dh", MHA_BWD)
def test_mha_1q_bwd_small_t_and_strides(B, T, H, dh):
    """cmve_mha_1q_bwd (one block per (b, h), 4 waves over the keys) against fp64 autograd, rtol 1e-4, atol
    2e-5 (test_mha_1q_backward_vs_torch's, the same randn inputs; (1, 65, 1, 300) measured in fp32 torch on
    the CPU against fp64: dq 8.9e-8, dk 4.0e-8, dv 6.4e-8 absolute at worst, 0.3% of the bound, which stands).
    T = 1 (ds = 0: dq and dk are zero), 2, 3 (idle waves), 9, and T = 65 with dh = 300 (second trips of the
    `tid` and lane loops), B = 1.  Contiguous, and with ldq / lddo / lddq / ldkv / lddkv padded, v_off = d + 4
    and d + 1, bases one float off alignment: bit for bit the contiguous values, and the gap columns of dkv
    between the K and V gradients keep their canary."""
    d = H * dh
    q, k, v, g = _mha_data(B, T, d, B * 1000 + T * 10 + H)
    _, wq, wk, wv = _mha_ref(q, k, v, B, T, H, dh, g=g)
    dq, dk, dv = _mha_bwd(q, k, v, g, B, T, H, dh)
    for got, want, what in ((dq, wq, "dq"), (dk, wk, "dk"), (dv, wv, "dv")):
        _close(got, want, 1e-4, 2e-5, f"{what} ({B},{T},{H},{dh})")
    for gap in (4, 1):
        sq, sk, sv = _mha_bwd(q, k, v, g, B, T, H, dh, strided=True, gap=gap)
        assert np.array_equal(sq, dq) and np.array_equal(sk, dk) and np.array_equal(sv, dv), f"strided, gap {gap}"


def test_mha_1q_bwd_at_the_lds_limit():
    """H = 1, dh = 64, B = 1: T = 8000 is the largest accepted T (2T + 6dh = 16384 floats = 64 KiB of dynamic
    LDS, next to the kernel's static 8 bytes) and must launch and be right; T = 8001 is CMVE_E_INVALID.
    Bounds: rtol 1e-4, atol 2e-5 as above; measured at this shape (fp32 torch on the CPU against fp64):
    dq 3.3e-8, dk 6.3e-9, dv 4.0e-9 absolute at worst, so four times the fp32 error is inside the bound."""
    engine, lib, check = _api()
    B, T, H, dh = 1, 8000, 1, 64
    q, k, v, g = _mha_data(B, T + 1, dh, 8000)
    _, wq, wk, wv = _mha_ref(q, k[:T], v[:T], B, T, H, dh, g=g)
    dq, dk, dv = _mha_bwd(q, k[:T], v[:T], g, B, T, H, dh)
    for got, want, what in ((dq, wq, "dq"), (dk, wk, "dk"), (dv, wv, "dv")):
        _close(got, want, 1e-4, 2e-5, f"{what} at T = 8000")
    Q, G, KV = Pad(B, dh, data=q), Pad(B, dh, data=g), Pad(T + 1, 2 * dh, data=_kv_window(k, v, dh, dh))
    DQ, DKV = Pad(B, dh), Pad(T + 1, 2 * dh)
    st = lib.cmve_mha_1q_bwd(engine.handle(), Q.ptr, Q.ld, KV.ptr, KV.ld, dh, B, T + 1, H, dh, G.ptr, G.ld, DQ.ptr,
                             DQ.ld, DKV.ptr, DKV.ld)
    _rejected(st, E_INVALID, "LDS", [DQ, DKV], "T = 8001")
    check(lib.cmve_mha_1q_bwd(engine.handle(), Q.ptr, Q.ld, KV.ptr, KV.ld, dh, B, 5, H, dh, G.ptr, G.ld, DQ.ptr,
                              DQ.ld, DKV.ptr, DKV.ld), "the valid call after")


# ------------------------------------------------------------------ 2. cmve_mha_absorbed (K9b)
def _abs_key(qb, t, f, gs, L):
    """Key t of query qb = g gs + bb: run R % L of conv block g gs f + R / L, R = t gs + bb."""
    g, bb = divmod(qb, gs)
    R = t * gs + bb
    return g * gs * f + R // L, R % L


def _abs_ref(y, u, d, npix, C, f, gs, B, H, eps=1e-5):
    """test_gpu_mha_absorbed_against_fp64's restatement for any npix and C: z_h = sum_t softmax_t(u_h . n_t) n_t,
    n_t the un-affined LayerNorm of key t in the kernel's element order e = p cpr + c'; v.mean(0) in the
    original order c' npix + p."""
    cpr = d // npix
    L = C // cpr
    T = f * L
    yd, ud = torch.from_numpy(y).double(), torch.from_numpy(u).double()
    p_idx, c_idx = torch.meshgrid(torch.arange(npix), torch.arange(cpr), indexing="ij")
    perm = (c_idx * npix + p_idx).reshape(-1)  # kernel element e -> original element
    zr, vr = torch.empty(B, H, d, dtype=torch.float64), torch.empty(B, d, dtype=torch.float64)
    for qb in range(B):
        keys = []
        for t in range(T):
            bf, run = _abs_key(qb, t, f, gs, L)
            keys.append(yd[bf * npix:(bf + 1) * npix, run * cpr:(run + 1) * cpr].reshape(-1))
        X = torch.stack(keys)  # [T, d], kernel order
        n = (X - X.mean(1, keepdim=True)) / torch.sqrt(X.var(1, unbiased=False, keepdim=True) + eps)
        p = torch.softmax(n @ ud[qb].view(H, d).T, 0)  # [T, H]
        zr[qb] = p.T @ n
        orig = torch.empty_like(X)
        orig[:, perm] = X
        vr[qb] = orig.mean(0)
    return zr.reshape(B, H * d).numpy(), vr.numpy()


def _abs_call(y, u, d, npix, C, f, gs, B, H, strided):
    engine, lib, check = _api()
    ldy, ldu, ldz, ldv, o2, o1 = (C + 2, H * d + 2, H * d + 6, d + 3, 2, 1) if strided else (C, H * d, H * d, d, 0, 0)
    Y, U = Pad(B * f * npix, C, ld=ldy, off=o2, data=y), Pad(B, H * d, ld=ldu, off=o2, data=u)
    Z, V = Pad(B, H * d, ld=ldz, off=o2), Pad(B, d, ld=ldv, off=o1)
    assert not strided or not (Y.aligned16 or U.aligned16 or Z.aligned16 or V.aligned16)
    check(lib.cmve_mha_absorbed(engine.handle(), Y.ptr, Y.ld, C, npix, f, gs, B, H, d, U.ptr, U.ld, 1e-5, Z.ptr, Z.ld,
                                V.ptr, V.ld), "cmve_mha_absorbed")
    z, vm = Z.numpy(), V.numpy()
    Z.assert_canary("mha_absorbed z")
    V.assert_canary("mha_absorbed vmean")
    return z, vm


# name: (d, npix, C / cpr = L, f, gs, B)
ABS_CASES = {
    "npix1_L1_T3": (640, 1, 1, 3, 1, 1),
    "npix8_L8": (512, 8, 8, 1, 3, 9),
    "npix32_halfC": (640, 32, 16, 1, 5, 15),
    "npix64_2C": (640, 64, 128, 1, 3, 3),
    "npix_half_d_T5": (512, 256, 1, 5, 2, 2),
    "npix_half_d_640": (640, 320, 4, 1, 3, 9),
    "T1": (640, 16, 1, 1, 1, 1),
    "T2": (512, 16, 1, 2, 1, 9),
    "T3_gs2": (640, 16, 3, 1, 2, 6),
    "T5_f5": (640, 16, 1, 5, 3, 15),
    "C_eq_d_f2": (512, 16, 16, 2, 5, 15),
}
ABS_REF = {}


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("name", sorted(ABS_CASES))
def test_mha_absorbed_index_arithmetic(name, strided):
    """cmve_mha_absorbed (H = 8, d = 640: E 10, and d = 512: E 8; one key row per step, two waves per query)
    against the fp64 restatement, z 2e-5 and vmean 2e-6 as test_gpu_mha_absorbed_against_fp64 (the same
    relu(randn) keys and 0.05 randn queries).  cpr = d / npix channels per run, L = C / cpr runs per conv row
    group, T = f L keys; contiguous, and with ldy = C + 2, ldu = H d + 2, ldz = H d + 6 on bases 8 bytes past a
    16-byte boundary and ldv = d + 3 on a base 4 bytes past one.
      npix1_L1_T3       npix 1: cpr = d, one contiguous 2560-byte run per key; C = cpr (L = 1); T = 3: one
                        ping-pong trip and the odd tail
      npix8_L8          d 512, cpr 64, C = d, gs = 3 coprime to L = 8, B = 3 gs = 9 (9 % 8 != 0 for xcd_linear)
      npix32_halfC      cpr 20, C = d / 2 (L 16), gs = 5, B = 15
      npix64_2C         cpr 10, cpr2 5 (pieces of a lane straddle pixels), C = 2 d (L 128, T 128), gs = 3
      npix_half_d_T5    d 512, npix 256: cpr 2, cpr2 1; C = cpr: every key from another conv block; T = 5, gs = 2
      npix_half_d_640   d 640, npix 320, L 4, gs 3, B 9
      T1 / T2 / T3_gs2  T = 1 (the prologue alone), 2 (one loop trip, no tail), 3 (L = 3, gs = 2: runs cross
                        conv blocks and groups)
      T5_f5             L = 1, f = 5, gs = 3, B = 15
      C_eq_d_f2         d 512, C = d, f = 2, gs = 5 coprime to L = 16, B = 15
    """
    d, npix, L, f, gs, B = ABS_CASES[name]
    H, cpr = 8, d // npix
    C = L * cpr
    if name not in ABS_REF:
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        y = torch.relu(torch.randn(B * f * npix, C, generator=gen)).numpy()
        u = (torch.randn(B, H * d, generator=gen) * 0.05).numpy()
        ABS_REF[name] = (y, u) + _abs_ref(y, u, d, npix, C, f, gs, B, H)
    y, u, zr, vr = ABS_REF[name]
    z, vm = _abs_call(y, u, d, npix, C, f, gs, B, H, strided)
    _within(z, zr, 2e-5, f"z {name}")
    _within(vm, vr, 2e-6, f"vmean {name}")


def test_mha_absorbed_degenerate_keys():
    """d 640, npix 16, C = 3 cpr (T = 3), gs = 1, B = 3, strided.  Query 0's key 1 is all zero: mean 0, variance
    0, rstd = eps^-1/2, n = 0 -- a score of 0 and no contribution to z.  Query 1's three keys are identical:
    equal scores, the uniform softmax, z_h = n for every head.  Bounds as the other absorbed cases."""
    d, npix, L, f, gs, B, H = 640, 16, 3, 1, 1, 3, 8
    cpr = d // npix
    C = L * cpr
    gen = torch.Generator().manual_seed(99)
    y = torch.relu(torch.randn(B * f * npix, C, generator=gen)).numpy()
    u = (torch.randn(B, H * d, generator=gen) * 0.05).numpy()
    bf, run = _abs_key(0, 1, f, gs, L)
    y[bf * npix:(bf + 1) * npix, run * cpr:(run + 1) * cpr] = 0
    b0, r0 = _abs_key(1, 0, f, gs, L)
    for t in (1, 2):
        bf, run = _abs_key(1, t, f, gs, L)
        y[bf * npix:(bf + 1) * npix, run * cpr:(run + 1) * cpr] = y[b0 * npix:(b0 + 1) * npix, r0 * cpr:(r0 + 1) * cpr]
    zr, vr = _abs_ref(y, u, d, npix, C, f, gs, B, H)
    x = torch.from_numpy(y[b0 * npix:(b0 + 1) * npix, r0 * cpr:(r0 + 1) * cpr].reshape(-1)).double()
    n1 = ((x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-5)).numpy()
    assert np.abs(zr[1].reshape(H, d) - n1).max() < 1e-12  # the reference itself: uniform softmax
    z, vm = _abs_call(y, u, d, npix, C, f, gs, B, H, True)
    _within(z, zr, 2e-5, "z with a zero key and identical keys")
    _within(vm, vr, 2e-6, "vmean with a zero key and identical keys")


def test_mha_absorbed_rejections():
    """Each refused call: its status (CMVE_E_INVALID, or CMVE_E_UNSUPPORTED for a (d, H) without an
    instantiation), cmve_last_error naming the rule, z and vmean all-canary.  B = 0 is CMVE_OK and writes
    nothing.  Every pointer covers the nominal shape of its call.  A valid call follows."""
    engine, lib, check = _api()
    d, npix, f, gs, B, H = 640, 16, 1, 3, 3, 8
    C = d

    def call(d=d, npix=npix, C=C, f=f, gs=gs, B=B, H=H, ldy=None, yoff=0, ldv=None):
        rows, Hd = max(B, 1) * f * npix, H * d
        Y, U = Pad(rows, C, ld=C if ldy is None else ldy, off=yoff), Pad(max(B, 1), Hd)
        Y.t.fill_(1.0)
        U.t.fill_(0.0)
        Z, V = Pad(max(B, 1), Hd), Pad(max(B, 1), max(d, d if ldv is None else ldv))
        st = lib.cmve_mha_absorbed(engine.handle(), Y.ptr, Y.ld, C, npix, f, gs, B, H, d, U.ptr, U.ld, 1e-5, Z.ptr,
                                   Z.ld, V.ptr, d if ldv is None else ldv)
        return st, [Z, V]

    for what, kw, code, rule in (
            ("odd ldy", dict(ldy=C + 1), E_INVALID, "alignment"),
            ("y one float off", dict(yoff=1), E_INVALID, "alignment"),
            ("ldv < d", dict(ldv=d - 1), E_INVALID, "strides"),
            ("(d, H) = (256, 8)", dict(d=256, C=256), E_UNSUPPORTED, "instantiated"),
            ("(d, H) = (640, 4)", dict(H=4), E_UNSUPPORTED, "instantiated"),
            ("B % gs != 0", dict(B=4), E_INVALID, "multiple of gs"),
            ("d % npix != 0", dict(npix=7), E_INVALID, "d / npix"),
            ("odd d / npix", dict(npix=128), E_INVALID, "even")):
        st, outs = call(**kw)
        _rejected(st, code, rule, outs, what)
    st, outs = call(B=0)
    assert st == 0
    torch.cuda.synchronize()
    for o in outs:
        o.assert_untouched("an output of B = 0")
    st, outs = call()
    check(st, "the valid call after")
    assert np.isfinite(outs[0].numpy()).all() and np.allclose(outs[1].numpy(), 1.0)


# ------------------------------------------------------------------ 3. LayerNorm family
LN_EPS = 1e-5


def _ln_ref(x, gamma, beta, eps=LN_EPS):
    x64 = x.astype(np.float64)
    mean = x64.mean(1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    y = (x64 - mean) * rstd
    if gamma is not None:
        y = y * gamma.astype(np.float64)
    if beta is not None:
        y = y + beta.astype(np.float64)
    return y, mean[:, 0], rstd[:, 0]


def _ln_rows(n, d, seed):
    """Row 0: 3 randn + 1; row 1: constant 1.5; row 2: scaled by 1e4; row 3: by 1e-4 (eps-dominated); row 4: randn."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((max(n, 1), d))
    x[0] = 3 * x[0] + 1
    if n > 1:
        x[1], x[2], x[3] = 1.5, x[2] * 1e4, x[3] * 1e-4
    return x[:n].astype(F32), rng.uniform(0.5, 1.5, d).astype(F32), rng.standard_normal(d).astype(F32)


def _ln_call(x, gamma, beta, n, d, ldx=None, ldy=None, yoff=0, goff=0):
    engine, lib, check = _api()
    X = Pad(n, d, ld=ldx, data=x if n else None)
    G = Pad(1, d, off=goff, data=gamma[None]) if gamma is not None else None
    Bt = Pad(1, d, data=beta[None]) if beta is not None else None
    Y = Pad(n, d, ld=ldy, off=yoff)
    check(lib.cmve_layernorm(engine.handle(), X.ptr, X.ld, n, d, _p(G), _p(Bt), LN_EPS, Y.ptr, Y.ld), "cmve_layernorm")
    if n == 0:
        torch.cuda.synchronize()
        Y.assert_untouched("layernorm y with n = 0")
        return None
    got = Y.numpy()
    Y.assert_canary(f"layernorm y ({n},{d})")
    return got


@pytest.mark.parametrize("d", [1, 3, 4, 63, 64, 65, 1024, 1025, 1028])
def test_layernorm_paths_null_arguments_and_strides(d):
    """cmve_layernorm, n = 0 (no launch, y untouched), 1 and 5 (a second block of one wave), against fp64 within
    one rounding: the kernel holds fp64 until its single conversion, so 2^-24 |want| + 1e-9 (1 + |want|), the
    second term for the fp64 sums' order.  Rows: 3 randn + 1, a constant row (variance 0: the output is beta),
    a row scaled by 1e4 and one by 1e-4 (variance 1e-8 under eps = 1e-5).  Paths (ln_vec4_ok: d <= 1024,
    d % 4 == 0, ldx % 4 == 0, x / gamma / beta 16-byte aligned): d = 4, 64, 1024 float4 rows (1024: all four
    runs of every lane); d = 1, 3, 63, 65 the scalar register row (d <= 1024); d = 1025, 1028 the looping
    form.  Variants: gamma / beta NULL in turn and together; gamma one float off alignment (scalar path, equal
    to the aligned call within the bound); ldx = d + 4 (float4 where d allows) and d + 1 (scalar); ldy = d + 3
    with y one float off: the input side alone picks the path, so bit for bit the aligned output."""
    for n in (0, 1, 5):
        x, gamma, beta = _ln_rows(n, d, d * 10 + n)
        if n == 0:
            _ln_call(x, gamma, beta, 0, d)
            continue
        base = None
        for g, b in ((gamma, beta), (None, beta), (gamma, None), (None, None)):
            want, _, _ = _ln_ref(x, g, b)
            got = _ln_call(x, g, b, n, d)
            _within(got, want, _one_rounding(want), f"layernorm ({n},{d}) gamma={g is not None} beta={b is not None}")
            base = got if base is None else base
        want, _, _ = _ln_ref(x, gamma, beta)
        bound = _one_rounding(want)
        if n == 5:
            _within(base[1], beta.astype(np.float64), bound[1], "a constant row gives beta")
        mis = _ln_call(x, gamma, beta, n, d, goff=1)
        _within(mis, want, bound, f"layernorm ({n},{d}) gamma off alignment")
        _within(mis, base, bound, f"layernorm ({n},{d}) gamma off alignment against the aligned call")
        for dld in (4, 1):
            _within(_ln_call(x, gamma, beta, n, d, ldx=d + dld), want, bound, f"layernorm ({n},{d}) ldx = d + {dld}")
        assert np.array_equal(_ln_call(x, gamma, beta, n, d, ldy=d + 3, yoff=1), base), "padded, misaligned y"
        assert np.array_equal(_ln_call(x, gamma, beta, n, d, ldx=d + 4), _ln_call(x, gamma, beta, n, d, ldx=d + 4,
                                                                                 ldy=d + 3, yoff=1))


def _bf16_rne(y):
    """fp32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.ascontiguousarray(y, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf2f(h):
    return (h.astype(np.uint32) << 16).view(F32)


def _split_planes(y, n_pad, d_pad):
    """The CMVE_PACK_RAW split of fp32 rows: hi = bf16_rne(y), lo = bf16_rne(y - hi); zero padding."""
    n, d = y.shape
    hi, lo = np.zeros((n_pad, d_pad), np.uint16), np.zeros((n_pad, d_pad), np.uint16)
    hi[:n, :d] = _bf16_rne(y)
    lo[:n, :d] = _bf16_rne(y - _bf2f(hi[:n, :d]))
    return hi, lo


def _rows_struct(n, d, n_pad, d_pad, with_err=True, plane_off=0):
    from cmve._lib import Rows
    HI, LO = (Pad(n_pad, d_pad, off=plane_off, dtype=torch.int16) for _ in range(2))
    ERR = Pad(1, 3) if with_err else None
    r = Rows()
    r.n, r.d, r.n_pad, r.d_pad = n, d, n_pad, d_pad
    r.hi, r.lo = HI.ptr, LO.ptr
    r.err_max = ERR.ptr if with_err else None
    return r, HI, LO, ERR


def _check_planes(r, HI, LO, ERR, hi, lo, what):
    from cmve._lib import PACK_RAW
    ghi, glo = HI.numpy().view(np.uint16), LO.numpy().view(np.uint16)
    HI.assert_canary(f"{what} hi")
    LO.assert_canary(f"{what} lo")
    assert np.array_equal(ghi, hi), f"{what}: hi plane, {int((ghi != hi).sum())} differ"
    assert np.array_equal(glo, lo), f"{what}: lo plane, {int((glo != lo).sum())} differ"
    assert r.flags & PACK_RAW, f"{what}: CMVE_PACK_RAW not set"
    if ERR is not None:
        assert np.array_equal(ERR.numpy()[0], np.full(3, np.inf, F32)), f"{what}: err_max is not +inf"
        ERR.assert_canary(f"{what} err_max")


@pytest.mark.parametrize("d,d_pad,dld", [(3, 7, 1), (64, 128, 4), (65, 67, 4), (640, 704, 4), (640, 642, 4),
                                         (1024, 1088, 4), (1024, 1088, 1)])
def test_layernorm_pack_planes_and_padding(d, d_pad, dld):
    """cmve_layernorm_pack, n = 5 (the rows of the LayerNorm test), ldx = d + dld, n_pad = n + 7 (rows 5 .. 11
    zero: a block of pure padding and a partly padded one), d_pad > d (columns zero), err_max given (three +inf
    words) -- bit for bit the split of cmve_layernorm's fp32 output for the same x / ldx / gamma / beta, hi =
    bf16_rne(y), lo = bf16_rne(y - hi).  d = 64, 640, 1024 with ldx = d + 4: float4 rows, 8-byte plane stores for
    d_pad = 128 / 704 / 1088 and 2-byte ones for d_pad = 642; d = 3, 65 and ldx = d + 1: the scalar row."""
    engine, lib, check = _api()
    n, n_pad = 5, 12
    x, gamma, beta = _ln_rows(n, d, d)
    y = _ln_call(x, gamma, beta, n, d, ldx=d + dld)
    hi, lo = _split_planes(y, n_pad, d_pad)
    X, G, Bt = Pad(n, d, ld=d + dld, data=x), Pad(1, d, data=gamma[None]), Pad(1, d, data=beta[None])
    r, HI, LO, ERR = _rows_struct(n, d, n_pad, d_pad)
    check(lib.cmve_layernorm_pack(engine.handle(), X.ptr, X.ld, n, d, G.ptr, Bt.ptr, LN_EPS, ctypes.byref(r)),
          "cmve_layernorm_pack")
    _check_planes(r, HI, LO, ERR, hi, lo, f"layernorm_pack d={d} d_pad={d_pad}")


def test_layernorm_pack_rejections():
    """d = 1028 (> 1024: the register row does not hold it) and out->n != n are CMVE_E_INVALID, planes and err_max
    untouched, flags unchanged; a valid call follows."""
    engine, lib, check = _api()
    for what, d, n_out, rule in (("d = 1028", 1028, 5, "d <= 1024"), ("out->n != n", 64, 4, "bad out")):
        X = Pad(5, d, data=_ln_rows(5, d, 1)[0])
        r, HI, LO, ERR = _rows_struct(n_out, d, 8, d + 4)
        st = lib.cmve_layernorm_pack(engine.handle(), X.ptr, X.ld, 5, d, None, None, LN_EPS, ctypes.byref(r))
        _rejected(st, E_INVALID, rule, [HI, LO, ERR], what)
        assert r.flags == 0
    x = _ln_rows(5, 64, 1)[0]
    r, HI, LO, ERR = _rows_struct(5, 64, 8, 68)
    X = Pad(5, 64, data=x)
    check(lib.cmve_layernorm_pack(engine.handle(), X.ptr, X.ld, 5, 64, None, None, LN_EPS, ctypes.byref(r)), "valid")
    _check_planes(r, HI, LO, ERR, *_split_planes(_ln_call(x, None, None, 5, 64), 8, 68), "the valid call after")


LN_TRAIN = [(1, 1), (5, 3), (7, 300), (0, 8)]


@pytest.mark.parametrize("n,d", LN_TRAIN)
def test_layernorm_train_fwd_and_bwd(n, d):
    """cmve_layernorm_train_fwd / cmve_layernorm_bwd (one wave per row, lane loop k = lane, lane + 64, ...:
    d = 1 and 3 part of a wave, d = 300 four full strides and 44 lanes of a fifth; n = 1, 5, 7: `row >= n`
    waves in the last block; n = 0: no launch), ldx = d + 3, ldy = d + 2, lddy = d + 5, lddx = d + 1, gamma /
    beta given and NULL.  Forward: y within one rounding of fp64 (cmve_layernorm's bound); save_mean and
    save_rstd are fp64 values stored as fp32: 2^-24 |want| plus the fp64 sum's own 2^-53 sum|x| / d (mean) or
    1e-12 relative (rstd).  Backward: the reference takes the kernel's saved fp32 mean and rstd as given and
    evaluates dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)), dgamma = sum dy xhat, dbeta = sum dy in
    fp64, so each output is again one rounding: 2^-24 |want| + 1e-9 (1 + |want|).  dx, dgamma and dbeta are NULL
    in turn and all together (nothing launched)."""
    engine, lib, check = _api()
    rng = np.random.default_rng(n * 1000 + d)
    x = (3 * rng.standard_normal((max(n, 1), d)) + 1).astype(F32)[:n]
    dy = rng.standard_normal((max(n, 1), d)).astype(F32)[:n]
    gamma, beta = rng.uniform(0.5, 1.5, d).astype(F32), rng.standard_normal(d).astype(F32)
    for g, b in ((gamma, beta), (None, None)):
        X, DY = Pad(n, d, ld=d + 3, data=x if n else None), Pad(n, d, ld=d + 5, data=dy if n else None)
        G = Pad(1, d, data=g[None]) if g is not None else None
        Bt = Pad(1, d, data=b[None]) if b is not None else None
        Y, SM, SR = Pad(n, d, ld=d + 2), Pad(1, max(n, 1)), Pad(1, max(n, 1))
        check(lib.cmve_layernorm_train_fwd(engine.handle(), X.ptr, X.ld, n, d, _p(G), _p(Bt), LN_EPS, Y.ptr, Y.ld,
                                           SM.ptr, SR.ptr), "cmve_layernorm_train_fwd")
        if n == 0:
            torch.cuda.synchronize()
            for o in (Y, SM, SR):
                o.assert_untouched("layernorm_train_fwd with n = 0")
        else:
            want, mean, rstd = _ln_ref(x, g, b)
            y, sm, sr = Y.numpy(), SM.numpy()[0], SR.numpy()[0]
            for o in (Y, SM, SR):
                o.assert_canary(f"layernorm_train_fwd ({n},{d})")
            _within(y, want, _one_rounding(want), f"train y ({n},{d})")
            _within(sm, mean, U24 * np.abs(mean) + U53 * np.abs(x.astype(np.float64)).sum(1) / d, "save_mean")
            _within(sr, rstd, (U24 + 1e-12) * rstd, "save_rstd")
            x64, g64 = x.astype(np.float64), dy.astype(np.float64)
            xh = (x64 - sm.astype(np.float64)[:, None]) * sr.astype(np.float64)[:, None]
            gd = g64 * (g.astype(np.float64) if g is not None else 1.0)
            want_dx = sr.astype(np.float64)[:, None] * (gd - gd.mean(1, keepdims=True) - xh * (gd * xh).mean(1, keepdims=True))
            want_dg, want_db = (g64 * xh).sum(0), g64.sum(0)
        for with_dx, with_dg, with_db in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
            DX = Pad(n, d, ld=d + 1) if with_dx else None
            DG, DB = (Pad(1, d) if with_dg else None), (Pad(1, d) if with_db else None)
            check(lib.cmve_layernorm_bwd(engine.handle(), X.ptr, X.ld, DY.ptr, DY.ld, n, d, _p(G), SM.ptr, SR.ptr,
                                         _p(DX), d + 1, _p(DG), _p(DB)), "cmve_layernorm_bwd")
            tag = f"({n},{d}) dx={with_dx} dgamma={with_dg} dbeta={with_db}"
            if n == 0:
                torch.cuda.synchronize()
                for o in (DX, DG, DB):
                    if o is not None:
                        o.assert_untouched(f"layernorm_bwd with n = 0 {tag}")
                continue
            for o, w, what in ((DX, want_dx, "dx"), (DG, want_dg[None], "dgamma"), (DB, want_db[None], "dbeta")):
                if o is not None:
                    got = o.numpy()
                    o.assert_canary(f"layernorm_bwd {what} {tag}")
                    _within(got, w, _one_rounding(w), f"{what} {tag}")


# ------------------------------------------------------------------ 4. block transposes and packers
def _tb_vec4(R, C, ow, x_aligned):
    return C % 4 == 0 and ow % 4 == 0 and x_aligned


TB_CASES = {(8192, 1): False, (1, 12288): False, (16, 768): True, (3, 5): False, (4, 8): True, (8, 4): True}


@pytest.mark.parametrize("R,C", sorted(TB_CASES))
def test_transpose_blocks_shapes_at_the_limits(R, C):
    """cmve_transpose_blocks, nb = 0 (no launch, y untouched), 1 and 3, against torch's view / transpose,
    torch.equal.  (8192, 1): 4 R (C + 1) = 65536 exactly, the LDS limit; (1, 12288): R C = 12288 exactly, the
    staging limit; both scalar (R or C not a multiple of 4), as (3, 5).  (16, 768), (4, 8), (8, 4): float4 loads
    and stores; (4, 8) again with x one float off alignment: the scalar form of the same values."""
    engine, lib, check = _api()
    assert _tb_vec4(R, C, R, True) == TB_CASES[(R, C)]
    for nb in (0, 1, 3):
        for xoff in ((0, 1) if (R, C) == (4, 8) else (0,)):
            x = torch.randn(max(nb, 1) * R * C, generator=torch.Generator().manual_seed(R + C + nb))
            X, Y = Pad(1, max(nb, 1) * R * C, off=xoff, data=x.numpy()[None]), Pad(1, max(nb, 1) * R * C)
            check(lib.cmve_transpose_blocks(engine.handle(), X.ptr, nb, R, C, Y.ptr), "cmve_transpose_blocks")
            if nb == 0:
                torch.cuda.synchronize()
                Y.assert_untouched("transpose_blocks y with nb = 0")
                continue
            got = Y.t.cpu()[0]
            Y.assert_canary(f"transpose_blocks ({R},{C}) nb={nb}")
            assert torch.equal(got, x.view(nb, R, C).transpose(1, 2).reshape(-1)), f"({R},{C}) nb={nb} xoff={xoff}"


def test_transpose_blocks_rejections():
    """(8193, 1): 4 R (C + 1) > 65536; (1, 12289): R C > 12288; R = 0: CMVE_E_INVALID, y untouched."""
    engine, lib, check = _api()
    X = Pad(1, 12289)
    X.t.fill_(1.0)
    for R, C in ((8193, 1), (1, 12289), (0, 4)):
        Y = Pad(1, 12289)
        _rejected(lib.cmve_transpose_blocks(engine.handle(), X.ptr, 1, R, C, Y.ptr), E_INVALID, "bad block shape", [Y],
                  f"(R, C) = ({R}, {C})")
    Y = Pad(1, 12)
    check(lib.cmve_transpose_blocks(engine.handle(), X.ptr, 1, 3, 4, Y.ptr), "the valid call after")
    assert (Y.t == 1).all()


# (R, C, d, G, gs, T, float4?): nb = G gs T d / (R C)
KV_CASES = [(16, 8, 8, 1, 2, 8, True), (16, 8, 8, 3, 2, 8, True), (16, 8, 8, 3, 1, 16, True),
            (4, 12, 6, 1, 2, 4, False),  # float4-able blocks, but a run of 6 floats: scalar
            (5, 6, 10, 3, 1, 1, False), (5, 6, 10, 3, 2, 3, False), (5, 6, 10, 1, 2, 3, False)] + \
           [(3, 2, 6, G, gs, T, False) for G in (1, 3) for gs in (1, 2) for T in (1, 3)]


@pytest.mark.parametrize("R,C,d,G,gs,T,vec", KV_CASES)
def test_transpose_blocks_kv_remap(R, C, d, G, gs, T, vec):
    """cmve_transpose_blocks_kv against its rule: the transposed blocks, flat, are G x T x gs runs of d floats and
    run (g, t, bb) goes to row t B + g gs + bb (B = G gs), torch.equal.  float4 form: R = 16, C = 8, d = 8
    (G = 1 and 3, gs = 1 and 2); scalar form: d = 6 on float4-able (4, 12) blocks, R = 5, and (3, 2) blocks
    with d = 6 at every G in {1, 3} x gs in {1, 2} x T in {1, 3}; once more with x one float off (scalar)."""
    engine, lib, check = _api()
    B = G * gs
    nb, rem = divmod(B * T * d, R * C)
    assert rem == 0 and vec == (_tb_vec4(R, C, R, True) and d % 4 == 0)
    x = torch.randn(nb * R * C, generator=torch.Generator().manual_seed(R * C + G + gs + T))
    want = x.view(nb, R, C).transpose(1, 2).reshape(G, T, gs, d).permute(1, 0, 2, 3).reshape(T * B, d)
    for xoff in (0, 1):
        X, Y = Pad(1, nb * R * C, off=xoff, data=x.numpy()[None]), Pad(T * B, d)
        check(lib.cmve_transpose_blocks_kv(engine.handle(), X.ptr, nb, R, C, d, T, gs, B, Y.ptr), "transpose_blocks_kv")
        got = Y.t.cpu()
        Y.assert_canary("transpose_blocks_kv y")
        assert torch.equal(got, want), f"kv ({R},{C},{d}) G={G} gs={gs} T={T} xoff={xoff}"


def test_transpose_blocks_kv_rejections():
    """nb R C != B T d and B % gs != 0: CMVE_E_INVALID, y untouched; a valid call follows."""
    engine, lib, check = _api()
    X = Pad(1, 96)
    X.t.fill_(2.0)
    for what, nb, B, gs in (("nb R C != B T d", 3, 4, 2), ("B % gs != 0", 4, 4, 3)):
        Y = Pad(16, 6)
        st = lib.cmve_transpose_blocks_kv(engine.handle(), X.ptr, nb, 4, 6, 6, 4, gs, B, Y.ptr)
        _rejected(st, E_INVALID, "nb*R*C must equal B*T*d", [Y], what)
    Y = Pad(16, 6)
    check(lib.cmve_transpose_blocks_kv(engine.handle(), X.ptr, 4, 4, 6, 6, 4, 2, 4, Y.ptr), "the valid call after")
    assert (Y.t == 2).all()


@pytest.mark.parametrize("with_err", [True, False])
@pytest.mark.parametrize("R,C,d_pad", [(8, 4, 8), (8, 4, 12), (8, 4, 9), (5, 3, 5), (5, 3, 9), (640, 16, 704)])
def test_pack_tblocks_planes_and_padding(R, C, d_pad, with_err):
    """cmve_pack_tblocks through a hand-built cmve_rows_t over canary planes, nb = 3, n = nb C, n_pad = n + 2 C
    (two blocks past nb write zero rows), d_pad = R, R + 4 (zero columns, float4 form for (8, 4)), R + 1 (scalar
    form), and the Combiner's (640, 16) into d_pad 704.  Bit for bit the CMVE_PACK_RAW split of the torch
    transpose; CMVE_PACK_RAW set in flags; err_max, where given, three +inf words."""
    engine, lib, check = _api()
    nb = 3
    n, n_pad = nb * C, nb * C + 2 * C
    x = torch.randn(nb * R * C, generator=torch.Generator().manual_seed(R * C + d_pad))
    ref = x.view(nb, R, C).transpose(1, 2).reshape(n, R).numpy()
    hi, lo = _split_planes(ref, n_pad, d_pad)
    X = Pad(1, nb * R * C, data=x.numpy()[None])
    r, HI, LO, ERR = _rows_struct(n, R, n_pad, d_pad, with_err=with_err)
    check(lib.cmve_pack_tblocks(engine.handle(), X.ptr, nb, R, C, ctypes.byref(r)), "cmve_pack_tblocks")
    _check_planes(r, HI, LO, ERR, hi, lo, f"pack_tblocks ({R},{C}) d_pad={d_pad}")


# ------------------------------------------------------------------ 5. fuse_combine and the other K16 kernels
def _combine32(y, ds, text, ref, based):
    """((y + ds text) + (1 - ds) ref) + based, every product and sum rounded to fp32 on its own."""
    s = ds.astype(F32)[:, None]
    out = ((y + s * text) + (F32(1) - s) * ref) + based
    assert out.dtype == F32
    return out


@pytest.mark.parametrize("n,d", [(1, 1), (5, 63), (6, 640), (0, 8)])
def test_fuse_combine_rows(n, d):
    """cmve_fuse_combine (one wave per row, lane loop over d: d = 1, 63 part of a wave, 640 ten strides; n = 1,
    5, 6: `row >= n` waves).  The fp32 combine v = ((y + ds text) + (1 - ds) ref) + relu(based) is restated
    op for op (the parenthesisation is the contract: bit-exact), then out = fp32(v / max(||v||, eps)) from
    fp64: one rounding, (2^-24 + 1e-12) |want| + 2^-149 (1e-12: the fp64 sum's order over <= 640 terms).  Rows:
    0 ds = 0.3; 1 ds = 0; 2 ds = 1; 3 all zero with based <= 0 (sum exactly 0: the output is 0, not NaN); 4 norm
    1e-20 under eps = 1e-12 (divided by eps); 5 as row 0.  based is negative at half the elements (the ReLU).
    n = 0: nothing launched."""
    engine, lib, check = _api()
    eps = 1e-12
    rng = np.random.default_rng(n * 100 + d)
    m = max(n, 1)
    y, text, ref, based = (rng.standard_normal((m, d)).astype(F32) for _ in range(4))
    ds = np.array([0.3, 0.0, 1.0, 0.5, 0.7, 0.3], F32)[:m]
    if n >= 5:
        y[3] = text[3] = ref[3] = 0
        based[3] = -np.abs(based[3])
        y[4] = (1e-20 * y[4] / np.linalg.norm(y[4].astype(np.float64))).astype(F32)
        text[4] = ref[4] = 0
        based[4] = -1.0
    pads = [Pad(m, d, data=a) for a in (y, text, ref, based)]
    DS, OUT = Pad(1, m, data=ds[None]), Pad(n, d)
    check(lib.cmve_fuse_combine(engine.handle(), pads[0].ptr, DS.ptr, pads[1].ptr, pads[2].ptr, pads[3].ptr, n, d, eps,
                                OUT.ptr), "cmve_fuse_combine")
    if n == 0:
        torch.cuda.synchronize()
        OUT.assert_untouched("fuse_combine out with n = 0")
        return
    got = OUT.numpy()
    OUT.assert_canary(f"fuse_combine out ({n},{d})")
    v = _combine32(y[:n], ds[:n], text[:n], ref[:n], np.maximum(based[:n], F32(0))).astype(np.float64)
    nrm = np.sqrt((v * v).sum(1, keepdims=True))
    want = v / np.maximum(nrm, eps)
    _within(got, want, (U24 + 1e-12) * np.abs(want) + 2.0 ** -149, f"fuse_combine ({n},{d})")
    if n >= 5:
        assert not got[3].any() and 0 < nrm[4, 0] < 2e-20 and np.abs(got[4]).max() < 1e-7


def test_fuse_combine_rejects_bad_shapes():
    """n < 0 and d <= 0 are CMVE_E_INVALID before any launch (unchecked, (n + 3) / 4 cast to unsigned made n = -1 a
    grid of 0 blocks, a launch error, and n = -8 one of 2^32 - 1 empty blocks); out untouched; a valid call
    follows."""
    engine, lib, check = _api()
    A, DS = Pad(2, 8), Pad(1, 2)
    A.t.fill_(1.0)
    DS.t.fill_(0.5)
    for n, d in ((-1, 8), (-8, 8), (2, 0), (2, -8)):
        OUT = Pad(2, 8)
        st = lib.cmve_fuse_combine(engine.handle(), A.ptr, DS.ptr, A.ptr, A.ptr, A.ptr, n, d, 1e-12, OUT.ptr)
        _rejected(st, E_INVALID, "cmve_fuse_combine: bad shape", [OUT], f"(n, d) = ({n}, {d})")
    OUT = Pad(2, 8)
    check(lib.cmve_fuse_combine(engine.handle(), A.ptr, DS.ptr, A.ptr, A.ptr, A.ptr, 2, 8, 1e-12, OUT.ptr), "valid")
    _within(OUT.numpy(), np.full((2, 8), 8 ** -0.5), 1e-7, "the valid call after")


ACT_SPECIALS = [0.0, -0.0, np.inf, -np.inf, 88.0, -88.0, 104.0, -104.0, 1e-40, -1e-40, 1.4e-45, np.nan, 1.0, -1.0, 20.0,
                -20.0]


def _act_ref(x, g, kind):
    """torch in fp64 on the CPU (relu, sigmoid, x sigmoid(1.702 x)) and its autograd: NaN and the infinities
    follow torch."""
    xr = torch.from_numpy(x).double().requires_grad_(True)
    yr = (torch.relu, torch.sigmoid, lambda v: v * torch.sigmoid(1.702 * v))[kind](xr)
    yr.backward(torch.from_numpy(g).double())
    return yr.detach().numpy(), xr.grad.numpy()


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n", [0, 1, 255, 257, 8192 * 256 + 3])
def test_activations_edges(n, kind):
    """cmve_act_fwd / _bwd (ReLU, sigmoid, QuickGELU; 256 threads per block, grid-stride) against torch in fp64:
    forward rtol 1e-6, atol 1e-7 and backward rtol 1e-5, atol 1e-6 (test_activations_vs_torch's).  n = 0 (no
    launch), 1, 255, 257 (a second block of one thread) and 8192 x 256 + 3: the grid is capped at 8192 blocks, so
    three threads take a second stride.  The first elements are +-0, +-inf, +-88, +-104 (expf overflows to inf
    inside sigm: 1 / (1 + inf) = 0), subnormals and NaN (the same non-finite pattern as torch: a NaN passes
    through ReLU and through its backward); the upstream gradient is 1 there.  ReLU's backward is exactly 0 at
    v = +0 and v = -0."""
    engine, lib, check = _api()
    rng = np.random.default_rng(n % 1000 + kind)
    m = max(n, 1)
    x, g = (3 * rng.standard_normal(m)).astype(F32), rng.standard_normal(m).astype(F32)
    k = min(n, len(ACT_SPECIALS))
    x[:k], g[:k] = np.array(ACT_SPECIALS, F32)[:k], 1.0
    if n > 2 ** 21:
        x[-3:], g[-3:] = [0.5, -0.5, 2.0], [1.0, 2.0, -3.0]  # the elements of the second stride
    X, G, Y, DX = Pad(1, m, data=x[None]), Pad(1, m, data=g[None]), Pad(1, m), Pad(1, m)
    check(lib.cmve_act_fwd(engine.handle(), X.ptr, n, kind, Y.ptr), "cmve_act_fwd")
    check(lib.cmve_act_bwd(engine.handle(), X.ptr, G.ptr, n, kind, DX.ptr), "cmve_act_bwd")
    if n == 0:
        torch.cuda.synchronize()
        Y.assert_untouched("act_fwd y with n = 0")
        DX.assert_untouched("act_bwd dx with n = 0")
        return
    y, dx = Y.numpy()[0], DX.numpy()[0]
    Y.assert_canary("act_fwd y")
    DX.assert_canary("act_bwd dx")
    wy, wdx = _act_ref(x, g, kind)
    _close(y, wy, 1e-6, 1e-7, f"act_fwd kind {kind} n {n}")
    _close(dx, wdx, 1e-5, 1e-6, f"act_bwd kind {kind} n {n}")
    if kind == 0 and n >= 2:
        assert dx[0] == 0 and dx[1] == 0, "ReLU backward at +-0"


@pytest.mark.parametrize("B,d", [(1, 1), (5, 65), (0, 4)])
def test_combine_train_fwd_and_bwd(B, d):
    """cmve_combine_train_fwd (elementwise, grid-stride) is bit for bit the op-for-op fp32 restatement ((y + ds
    text) + (1 - ds) ref) + based; cmve_combine_train_bwd (one wave per row; d = 65: lane 0's second stride)
    gives dtext = g ds and dref = g (1 - ds) bit for bit, and dds = sum g (text - ref) from fp64: 2^-24 |want| +
    2^-24 sum|g (text - ref)| 2^-20 (one rounding plus the fp64 chain).  ds includes 0 and 1; dtext, dref and dds
    NULL in turn; B = 0: nothing launched."""
    engine, lib, check = _api()
    rng = np.random.default_rng(B * 10 + d)
    m = max(B, 1)
    y, text, ref, based, g = (rng.standard_normal((m, d)).astype(F32) for _ in range(5))
    ds = np.array([0.3, 0.0, 1.0, 0.9, 0.123], F32)[:m]
    P = [Pad(m, d, data=a) for a in (y, text, ref, based, g)]
    DS, OUT = Pad(1, m, data=ds[None]), Pad(B, d)
    check(lib.cmve_combine_train_fwd(engine.handle(), P[0].ptr, DS.ptr, P[1].ptr, P[2].ptr, P[3].ptr, B, d, OUT.ptr),
          "cmve_combine_train_fwd")
    if B == 0:
        torch.cuda.synchronize()
        OUT.assert_untouched("combine_train_fwd out with B = 0")
    else:
        got = OUT.numpy()
        OUT.assert_canary("combine_train_fwd out")
        want = _combine32(y, ds, text, ref, based)
        assert np.array_equal(got, want), f"combine_train_fwd: {int((got != want).sum())} of {got.size} differ"
    s = ds[:, None]
    want_dt, want_dr = g * s, g * (F32(1) - s)
    t64 = g.astype(np.float64) * (text.astype(np.float64) - ref.astype(np.float64))
    want_dds = t64.sum(1)
    for wt, wr, wd in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        DT, DR, DD = (Pad(B, d) if wt else None), (Pad(B, d) if wr else None), (Pad(1, m) if wd else None)
        check(lib.cmve_combine_train_bwd(engine.handle(), P[4].ptr, DS.ptr, P[1].ptr, P[2].ptr, B, d, _p(DT), _p(DR),
                                         _p(DD)), "cmve_combine_train_bwd")
        if B == 0:
            torch.cuda.synchronize()
            for o in (DT, DR, DD):
                if o is not None:
                    o.assert_untouched("combine_train_bwd with B = 0")
            continue
        for o, w, what in ((DT, want_dt, "dtext"), (DR, want_dr, "dref")):
            if o is not None:
                got = o.numpy()
                o.assert_canary(f"combine_train_bwd {what}")
                assert np.array_equal(got, w), f"{what} ({B},{d})"
        if DD is not None:
            got = DD.numpy()[0]
            DD.assert_canary("combine_train_bwd dds")
            _within(got, want_dds, U24 * np.abs(want_dds) + U24 * np.abs(t64).sum(1) * 2.0 ** -20, f"dds ({B},{d})")


@pytest.mark.parametrize("B,T,F", [(1, 1, 1), (3, 7, 5), (2, 3, 640)])
def test_pool_mean_bwd_exact(B, T, F):
    """cmve_pool_mean_bwd: dx[b, t, f] is exactly dy[b, f] * (1.f / T) in fp32 (T = 7 and 3: 1 / T is inexact, the
    product is one more rounding, not a division); (2, 3, 640): 15 blocks, the index split i / (T F), i % F."""
    engine, lib, check = _api()
    dy = np.random.default_rng(B + T + F).standard_normal((B, F)).astype(F32)
    DY, DX = Pad(B, F, data=dy), Pad(B, T * F)
    check(lib.cmve_pool_mean_bwd(engine.handle(), DY.ptr, B, T, F, DX.ptr), "cmve_pool_mean_bwd")
    got = DX.numpy().reshape(B, T, F)
    DX.assert_canary("pool_mean_bwd dx")
    want = np.broadcast_to((dy * (F32(1) / F32(T)))[:, None, :], (B, T, F))
    assert np.array_equal(got, want)
