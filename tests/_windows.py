"""Canary-buffer windows, the bound check and the restatements of score_error_bound, the directed fp32
roundings and the GEMM's geometry rule shared by the C-ABI edge tests (test_gpu_head_edges.py,
test_gpu_fusion_edges.py, test_gpu_pack_edges.py, test_gpu_topk_edges.py, test_gpu_gemm_edges.py).  A plain
module, not a test file."""
import numpy as np
import torch

GUARD = 8  # canary elements before and after a window: a multiple of 4 floats, so `off` alone sets the base alignment


class Pad:
    """A [rows, cols] window with leading dimension ld, `off` elements into a canary-filled device
    buffer (NaN; -77 for integers).  `t` is the window, `ptr` its base address."""

    def __init__(self, rows, cols, ld=None, off=0, dtype=torch.float32, data=None):
        import ctypes
        self.ld = cols if ld is None else ld
        assert self.ld >= cols
        self.isf = dtype.is_floating_point
        fill = float("nan") if self.isf else -77
        self.flat = torch.full((GUARD + off + max(rows, 1) * self.ld + GUARD,), fill, dtype=dtype, device="cuda")
        self.geom = ((rows, cols), (self.ld, 1), GUARD + off)
        self.t = torch.as_strided(self.flat, *self.geom)
        addr = self.flat.data_ptr() + (GUARD + off) * self.flat.element_size()
        assert self.flat.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(addr)
        self.aligned16 = addr % 16 == 0
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)).to(dtype))

    def numpy(self):
        return self.t.cpu().numpy()

    def assert_canary(self, what=""):
        keep = torch.ones(self.flat.shape, dtype=torch.bool, device="cuda")
        torch.as_strided(keep, *self.geom).fill_(False)
        rest = self.flat[keep]
        ok = rest.isnan().all() if self.isf else (rest == -77).all()
        assert bool(ok), f"canary overwritten around {what}"

    def assert_untouched(self, what=""):
        ok = self.flat.isnan().all() if self.isf else (self.flat == -77).all()
        assert bool(ok), f"{what} was written"


def _within(got, want, bound, what):
    """|got - want| <= bound where want is finite; the same inf / NaN where it is not."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), f"{what}: non-finite pattern differs"
    err = np.abs(got[fin] - want[fin])
    b = np.broadcast_to(bound, want.shape)[fin]
    bad = ~(err <= b)
    assert not bad.any(), f"{what}: {int(bad.sum())} outside the bound, worst err {err[bad].max():.3e} " \
                          f"against {b[bad][np.argmax(err[bad])]:.3e}"


def _f32_up(x):
    with np.errstate(over="ignore"):
        f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def _f32_down(x):
    with np.errstate(over="ignore"):
        f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def _E(ea, eb, d_pad, mode):
    """score_error_bound (cmve_internal.h:692) in fp64, operation for operation (mode 1 = CMVE_SIM_BF16X3)."""
    ea, eb = np.asarray(ea, np.float64), np.asarray(eb, np.float64)
    n = float(d_pad) * (33.0 / 32.0) * (3.0 if mode == 1 else 1.0)
    u = 1.0 / 8388608.0
    gamma = n * u / (1.0 - n * u)
    return ea + (1.0 + ea) * eb + gamma * (1.0 + ea) * (1.0 + eb) + 1e-12


def _phased(nq_pad, ng_pad):
    """sim_uses_phased (sim.hip): the persistent G256 kernel."""
    return nq_pad % 256 == 0 and ng_pad % 256 == 0 and (nq_pad // 256) * (ng_pad // 256) >= 512


def _g64(nq_pad, ng_pad):
    """sim_uses_g64 (sim.hip): the G64 ring kernel; neither: G128."""
    return not _phased(nq_pad, ng_pad) and (nq_pad // 128) * (ng_pad // 128) < 128 and nq_pad % 64 == 0 and \
        ng_pad % 64 == 0
