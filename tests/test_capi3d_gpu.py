"""The 3D entry points of the C ABI (csrc/include/rma/capi.h) on the GPU, driven
through ctypes the way a C / Julia host would: the one- and two-step kernels on
boxes, the device-side initial conditions and the native 3D time loop, bitwise
against the Python ops and ``Diffusion3D``."""
import ctypes
import os

import pytest
import torch

from helpers import ROOT
from rocm_mpi_amd import ops
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig

pytestmark = pytest.mark.gpu

P, I64, DBL = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double


def lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rocm_mpi_amd", "librma_core.so"))
    L.rma_last_error.restype = ctypes.c_char_p
    for f in ("rma_nx_g", "rma_ny_g", "rma_nz_g"):
        getattr(L, f).restype = ctypes.c_int64
    for f in ("rma_diffusion3d_step", "rma_diffusion3d_boxes", "rma_init_gaussian3d",
              "rma_init_random3d", "rma_executor3d_create", "rma_executor3d_run",
              "rma_executor3d_parity", "rma_executor3d_uniform", "rma_executor3d_rescan_factor",
              "rma_executor3d_destroy"):
        getattr(L, f)  # the first missing symbol fails here
    return L


def ck(L, rc):
    assert rc == 0, L.rma_last_error().decode()


def grid(L, n, K=1, periods=(0, 0, 0), ol=None):
    g = ctypes.c_void_p()
    ol = ol or (2 * K,) * 3
    ck(L, L.rma_init_global_grid(n[0], n[1], n[2], None, (ctypes.c_int * 3)(*periods),
                                 (ctypes.c_int * 3)(*ol), (ctypes.c_int * 3)(*(o // 2 for o in ol)),
                                 1, 0, None, 0, ctypes.byref(g), None, None, None))
    return g


def stream():
    return P(torch.cuda.current_stream().cuda_stream)


def eq(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


COEF = ops.StencilCoef3(-1.0, 25.8, 13.0, 7.0, 2.4e-4)


def fields(nz, ny, nx, seed=7):
    g = torch.Generator().manual_seed(seed)
    T = torch.rand((nz, ny, nx), generator=g, dtype=torch.float64).cuda()
    iCp = (0.5 + torch.rand((nz, ny, nx), generator=g, dtype=torch.float64)).cuda()
    return T, iCp


def test_step_equals_ops_stencil3d_step_bitwise():
    L = lib()
    nz, ny, nx = 7, 13, 258
    T, iCp = fields(nz, ny, nx)
    want, got = torch.full_like(T, -3.0), torch.full_like(T, -3.0)
    ops.stencil3d_step(want, T, iCp, COEF)
    ck(L, L.rma_diffusion3d_step(P(got.data_ptr()), P(T.data_ptr()), P(iCp.data_ptr()), I64(nx),
                                 I64(ny), I64(nz), (DBL * 5)(*COEF), stream()))
    assert eq(got, want)


@pytest.mark.parametrize("fast", [False, True], ids=["canonical", "fast7"])
@pytest.mark.parametrize("K", [1, 2])
def test_boxes_equal_ops_stencil3dk_step_bitwise(K, fast):
    L = lib()
    nz, ny, nx = 7, 13, 258
    T, iCp = fields(nz, ny, nx)
    boxes = [(1, 100, 1, 12, 1, 6), (131, 257, 2, 9, 2, 5)]  # a gap over the strip seam
    want, got = torch.full_like(T, -3.0), torch.full_like(T, -3.0)
    ops.stencil3dk_step(K, want, T, iCp, COEF, boxes, tuning=ops.Stencil3DTuning(fast_math=fast))
    flat = (I64 * 12)(*[v for b in boxes for v in b])
    ck(L, L.rma_diffusion3d_boxes(K, P(got.data_ptr()), P(T.data_ptr()), P(iCp.data_ptr()),
                                  I64(nx), I64(ny), I64(nz), flat, 2, (DBL * 5)(*COEF),
                                  int(fast), stream()))
    assert eq(got, want)
    assert bool((got[:, :, 100:131] == -3.0).all())  # the gap keeps T2's values
    rc = L.rma_diffusion3d_boxes(K, P(got.data_ptr()), P(T.data_ptr()), P(iCp.data_ptr()),
                                 I64(nx), I64(ny), I64(nz), flat, 9, (DBL * 5)(*COEF), 0, stream())
    assert rc != 0 and b"nboxes" in L.rma_last_error()


def test_initial_conditions_equal_ops_bitwise():
    L = lib()
    nz, ny, nx = 6, 7, 9
    periods = (1, 0, 1)
    g = grid(L, (nx, ny, nz), periods=periods)
    ng = (L.rma_nx_g(g), L.rma_ny_g(g), L.rma_nz_g(g))
    assert ng == (nx - 2, ny, nz - 2)
    d = [10.0 / v for v in ng]
    geom = ops.TileGeometry3(0, 0, 0, ng[0], ng[1], ng[2], d[0], d[1], d[2], periodx=periods[0],
                             periody=periods[1], periodz=periods[2])
    want = torch.empty((nz, ny, nx), dtype=torch.float64, device="cuda")
    got = torch.empty_like(want)
    ops.init_gaussian3d_(want, geom, 10.0, 10.0, 10.0)
    ck(L, L.rma_init_gaussian3d(g, P(got.data_ptr()), I64(nx), I64(ny), I64(nz), DBL(d[0]),
                                DBL(d[1]), DBL(d[2]), DBL(10.0), DBL(10.0), DBL(10.0), stream()))
    assert eq(got, want)
    ops.init_random3d_(want, geom, seed=99)
    ck(L, L.rma_init_random3d(g, P(got.data_ptr()), I64(nx), I64(ny), I64(nz), DBL(d[0]),
                              DBL(d[1]), DBL(d[2]), ctypes.c_uint64(99), stream()))
    assert eq(got, want)
    ck(L, L.rma_finalize_global_grid(g))


def create(L, g, mode, T, T2, iCp, n, coef, K, fast=0, xface=0, bw=(16, 2, 2)):
    ex = ctypes.c_void_p()
    rc = L.rma_executor3d_create(g, mode, P(T.data_ptr()), P(T2.data_ptr()), P(iCp.data_ptr()),
                                 I64(n[0]), I64(n[1]), I64(n[2]), (DBL * 5)(*coef),
                                 (I64 * 3)(*bw), K, fast, xface, ctypes.byref(ex))
    return rc, ex


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("mode", [0, 1], ids=["perf", "perf_hide"])
def test_executor_equals_diffusion3d_bitwise_and_outlives_its_grid(mode, K):
    L = lib()
    n, nt = (130, 13, 9), 7
    m = Diffusion3D(Diffusion3DConfig(variant=("perf", "perf_hide")[mode], nx=n[0], ny=n[1],
                                      nz=n[2], nt=nt, init="random", seed=5, periods=(1, 1, 1),
                                      quiet=True, temporal=K))
    assert m.device.type == "cuda"
    coef = tuple(m.coef)
    T = m.field.clone()
    m.step(nt)
    want = m.field.clone()
    m.close()

    g = grid(L, n, K, periods=(1, 1, 1))
    T2, iCp = T.clone(), torch.ones_like(T)
    torch.cuda.synchronize()
    rc, ex = create(L, g, mode, T, T2, iCp, n, coef, K)
    ck(L, rc)
    assert L.rma_executor3d_uniform(ex) == 1
    ck(L, L.rma_executor3d_run(ex, I64(nt), stream()))
    par = L.rma_executor3d_parity(ex)
    assert par == (nt // K + nt % K) % 2
    torch.cuda.synchronize()
    assert eq((T, T2)[par], want)
    # an edit of 1/Cp is seen by the rescan
    iCp[1, 2, 3] = 2.0
    u = ctypes.c_int(-1)
    ck(L, L.rma_executor3d_rescan_factor(ex, ctypes.byref(u)))
    assert u.value == 0 and L.rma_executor3d_uniform(ex) == 0
    # the executor pins its grid: finalize first, then run once more, then destroy
    ck(L, L.rma_finalize_global_grid(g))
    ck(L, L.rma_executor3d_run(ex, I64(1), stream()))
    torch.cuda.synchronize()
    ck(L, L.rma_executor3d_destroy(ex))


def test_create_refusals_name_the_argument():
    L = lib()
    n = (130, 13, 9)
    T = torch.zeros((n[2], n[1], n[0]), dtype=torch.float64, device="cuda")
    T2 = torch.full_like(T, 7.25)
    iCp = torch.ones_like(T)
    g = grid(L, n, 1, periods=(1, 1, 1))  # overlap 2
    rc, _ = create(L, g, 0, T, T2, iCp, n, COEF, 3)
    assert rc != 0 and b"steps_per_pass" in L.rma_last_error()
    rc, _ = create(L, g, 1, T, T2, iCp, n, COEF, 2)
    assert rc != 0 and b"overlap" in L.rma_last_error()
    torch.cuda.synchronize()
    assert bool((T2 == 7.25).all())
    ck(L, L.rma_finalize_global_grid(g))  # no executor was created: torn down here
