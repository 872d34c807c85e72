"""Exact model of the fast7 arithmetic of the 3D kernels (the 7-point sum with
the constants folded into one per-cell factor; csrc/include/rma/kernels.h).

Python floats; every fused multiply-add is evaluated exactly with
``fractions.Fraction`` and rounded once (``float(Fraction)`` is the
round-to-nearest-even of the exact value, i.e. what v_fma_f64 / std::fma
return), as ``golden.step5`` does for the 2D fast5 arithmetic. Shares no code
with the package: slow, for small grids only.
"""
from fractions import Fraction

import numpy as np


def fma(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fast7_constants(mlam, rdx, rdy, rdz, dt):
    """(mkc, ry, rz, gs), every product in this order, in double."""
    ax = (-mlam) * rdx * rdx
    ay = (-mlam) * rdy * rdy
    az = (-mlam) * rdz * rdz
    ry = ay / ax
    rz = az / ax
    mkc = -2.0 * ((1.0 + ry) + rz)
    gs = dt * ax
    return mkc, ry, rz, gs


def cell7(T, iCp, z, y, x, mkc, ry, rz, gs) -> float:
    c = float(T[z, y, x])
    sx = float(T[z, y, x + 1]) + float(T[z, y, x - 1])
    sy = float(T[z, y - 1, x]) + float(T[z, y + 1, x])
    sz = float(T[z - 1, y, x]) + float(T[z + 1, y, x])
    t = fma(mkc, c, sx)
    t = fma(ry, sy, t)
    t = fma(rz, sz, t)
    return fma(gs * float(iCp[z, y, x]), t, c)  # gs*iCp: one rounded multiply


def step7(T, iCp, mlam, rdx, rdy, rdz, dt):
    """One step on the interior [1,n-1)^3 of a (nz, ny, nx) array; the six faces keep T."""
    k = fast7_constants(mlam, rdx, rdy, rdz, dt)
    nz, ny, nx = T.shape
    out = np.array(T, dtype=np.float64)
    for z in range(1, nz - 1):
        for y in range(1, ny - 1):
            for x in range(1, nx - 1):
                out[z, y, x] = cell7(T, iCp, z, y, x, *k)
    return out


def pass7(K, T2, T, iCp, boxes, mlam, rdx, rdy, rdz, dt):
    """A K-step pass: K - 1 steps on the interior, then the last step written
    into T2 on the half-open boxes (x0, x1, y0, y1, z0, z1) only."""
    k = fast7_constants(mlam, rdx, rdy, rdz, dt)
    a = np.array(T, dtype=np.float64)
    for _ in range(K - 1):
        a = step7(a, iCp, mlam, rdx, rdy, rdz, dt)
    for x0, x1, y0, y1, z0, z1 in boxes:
        for z in range(z0, z1):
            for y in range(y0, y1):
                for x in range(x0, x1):
                    T2[z, y, x] = cell7(a, iCp, z, y, x, *k)
    return T2
