"""NumPy float64 golden model of 3D heat diffusion on the GLOBAL grid.

Independent of the package. Fields are (nz, ny, nx), x fastest. The per-cell
update is the 2D golden model's with the z flux difference subtracted last:

    qxR=(mlam*(T[z][y][x+1]-c))*rdx   qxL=(mlam*(c-T[z][y][x-1]))*rdx
    qyU=(mlam*(T[z][y+1][x]-c))*rdy   qyD=(mlam*(c-T[z][y-1][x]))*rdy
    qzF=(mlam*(T[z+1][y][x]-c))*rdz   qzB=(mlam*(c-T[z-1][y][x]))*rdz
    T2 = c + dt*( iCp*( ((-(qxR-qxL))*rdx - (qyU-qyD)*rdy) - (qzF-qzB)*rdz ) )

NumPy evaluates every operation in float64 with one rounding, in the order
written, so decomposed runs of the package must match it bitwise.
"""
import numpy as np

M64 = 2**64
GOLDEN = 0x9E3779B97F4A7C15
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB


def params3(nxg, nyg, nzg, lx=10.0, ly=10.0, lz=10.0, lam=1.0, Cp0=1.0):
    dx, dy, dz = lx / nxg, ly / nyg, lz / nzg
    dt = min(dx * dx, dy * dy, dz * dz) * Cp0 / lam / 6.1
    return dx, dy, dz, dt


def initial3(nxg, nyg, nzg, lx=10.0, ly=10.0, lz=10.0):
    dx, dy, dz, _ = params3(nxg, nyg, nzg, lx, ly, lz)
    a = (np.arange(nxg, dtype=np.float64) * dx + dx / 2) - lx / 2
    b = (np.arange(nyg, dtype=np.float64) * dy + dy / 2) - ly / 2
    c = (np.arange(nzg, dtype=np.float64) * dz + dz / 2) - lz / 2
    return np.exp(-(a * a)[None, None, :] - (b * b)[None, :, None] - (c * c)[:, None, None])


def step3(T, iCp, mlam, rdx, rdy, rdz, dt):
    c = T[1:-1, 1:-1, 1:-1]
    qxR = (mlam * (T[1:-1, 1:-1, 2:] - c)) * rdx
    qxL = (mlam * (c - T[1:-1, 1:-1, :-2])) * rdx
    qyU = (mlam * (T[1:-1, 2:, 1:-1] - c)) * rdy
    qyD = (mlam * (c - T[1:-1, :-2, 1:-1])) * rdy
    qzF = (mlam * (T[2:, 1:-1, 1:-1] - c)) * rdz
    qzB = (mlam * (c - T[:-2, 1:-1, 1:-1])) * rdz
    out = T.copy()
    out[1:-1, 1:-1, 1:-1] = c + dt * (iCp[1:-1, 1:-1, 1:-1] * (
        ((-(qxR - qxL)) * rdx - (qyU - qyD) * rdy) - (qzF - qzB) * rdz))
    return out


def run3(nxg, nyg, nzg, nt, lx=10.0, ly=10.0, lz=10.0, lam=1.0, Cp0=1.0, T0=None,
         periods=(0, 0, 0), iCp=None):
    """nt steps on the (nzg, nyg, nxg) array of the global grid.

    On a periodic dimension the array's first and last cells are ghosts of the
    cells one period away, so the grid has n - 2 distinct cells there (that is
    ImplicitGlobalGrid's n_g, which sets the spacing) and the ghosts are
    refreshed after every step, as a halo update does.

    ``iCp``: a (nzg, nyg, nxg) array of 1/Cp (ghosts included) instead of the
    constant 1/Cp0; dt keeps Cp0, as the model's does."""
    ng = [n - 2 if p else n for n, p in zip((nxg, nyg, nzg), periods)]
    dx, dy, dz, dt = params3(*ng, lx, ly, lz, lam, Cp0)
    T = initial3(nxg, nyg, nzg, lx, ly, lz) if T0 is None else np.array(T0, dtype=np.float64)
    iCp = np.full_like(T, 1.0 / Cp0) if iCp is None else np.array(iCp, dtype=np.float64)
    assert iCp.shape == T.shape
    for _ in range(nt):
        T = step3(T, iCp, -lam, 1.0 / dx, 1.0 / dy, 1.0 / dz, dt)
        for ax, per in zip((2, 1, 0), periods):
            if per:
                Tm = np.moveaxis(T, ax, 0)  # a view: writes go to T
                Tm[0] = Tm[-2]
                Tm[-1] = Tm[1]
    return T


# ---------------------------------------------------------------------------
# init_random3d in Python integers: splitmix64 finaliser of
# seed + (idx + 1) * GOLDEN, idx = (gz*nyg + gy)*nxg + gx over the wrapped
# global indices, top 53 bits scaled to [0, 1)
# ---------------------------------------------------------------------------
def mix64(z):
    z = ((z ^ (z >> 30)) * MIX1) % M64
    z = ((z ^ (z >> 27)) * MIX2) % M64
    return z ^ (z >> 31)


def uniform01(seed, idx):
    return (mix64((seed + (idx + 1) * GOLDEN) % M64) >> 11) * 2.0**-53


def wrap(g, n, periodic):
    """Global index of a local cell: on a periodic dimension the grid's first
    cell is a ghost, g -> (g - 1) mod n."""
    return (g - 1) % n if periodic else g


def random_field3(nx, ny, nz, geom, seed, lo=0.0, hi=1.0):
    """(nz, ny, nx) field of a tile; ``geom`` has g{x,y,z}0, n{x,y,z}g, period{x,y,z}."""
    out = np.empty((nz, ny, nx), dtype=np.float64)
    for iz in range(nz):
        gz = wrap(geom.gz0 + iz, geom.nzg, geom.periodz)
        for iy in range(ny):
            gy = wrap(geom.gy0 + iy, geom.nyg, geom.periody)
            for ix in range(nx):
                gx = wrap(geom.gx0 + ix, geom.nxg, geom.periodx)
                idx = ((gz * geom.nyg + gy) * geom.nxg + gx) % M64
                out[iz, iy, ix] = lo + (hi - lo) * uniform01(seed % M64, idx)
    return out


def random_field3_np(nx, ny, nz, geom, seed, lo=0.0, hi=1.0):
    """random_field3 for grids too large for its Python loop: the same integers
    in NumPy uint64 arrays, whose products and sums wrap mod 2**64."""
    u64 = np.uint64

    def axis(g0, n, ng, periodic):
        g = g0 + np.arange(n, dtype=np.int64)
        return ((g - 1) % ng if periodic else g).astype(u64)

    gx = axis(geom.gx0, nx, geom.nxg, geom.periodx)
    gy = axis(geom.gy0, ny, geom.nyg, geom.periody)
    gz = axis(geom.gz0, nz, geom.nzg, geom.periodz)
    idx = (gz[:, None, None] * u64(geom.nyg) + gy[None, :, None]) * u64(geom.nxg) \
        + gx[None, None, :]
    z = (idx + u64(1)) * u64(GOLDEN) + u64(seed % M64)
    z = (z ^ (z >> u64(30))) * u64(MIX1)
    z = (z ^ (z >> u64(27))) * u64(MIX2)
    z = z ^ (z >> u64(31))
    return lo + (hi - lo) * ((z >> u64(11)).astype(np.float64) * 2.0**-53)


# ---------------------------------------------------------------------------
# init_gaussian3d: exp(-(a*a) - (b*b) - (c*c)) against the separable product
# exp(-a^2) * exp(-b^2) * exp(-c^2) of exact 1-D arguments
# ---------------------------------------------------------------------------
def _dims(nx, ny, nz, geom, lx, ly, lz):
    return ((geom.gx0, nx, geom.dx, geom.xoff, geom.nxg, geom.periodx, lx),
            (geom.gy0, ny, geom.dy, geom.yoff, geom.nyg, geom.periody, ly),
            (geom.gz0, nz, geom.dz, geom.zoff, geom.nzg, geom.periodz, lz))


def gaussian_product3(nx, ny, nz, geom, lx, ly, lz):
    """(nz, ny, nx) product of three 1-D factors exp(-a_i^2): every centred
    coordinate an exact rational of the float64 inputs, its negated square
    rounded to float64 once (int / int is correctly rounded), then NumPy's exp
    and two float64 multiplications."""
    from misc_oracles import _centred_1d

    fx, fy, fz = (np.exp(np.array([float(-(a * a)) for a in _centred_1d(*d)]))
                  for d in _dims(nx, ny, nz, geom, lx, ly, lz))
    return (fx[None, None, :] * fy[None, :, None]) * fz[:, None, None]


def gaussian_tolerance3(nx, ny, nz, geom, lx, ly, lz):
    """Relative bound on |kernel - gaussian_product3|, to first order, extending
    misc_oracles.gaussian_tolerance (u = 2**-53 per rounding) to three dimensions.

    Kernel: per dimension the centred coordinate is off by |da| <= R*u*C (R = 4
    roundings on an open dimension, 9 on a periodic one, intermediates at most
    C = (max(g0 + n, n_g) + 1)*d + |off|), so a*a is off by 2*A*R*u*C plus u*A^2
    of its own rounding (A = max |a|). -(a*a) is exact; the first subtraction
    rounds a quantity of at most Ax^2 + Ay^2, the second one of at most S =
    Ax^2 + Ay^2 + Az^2. Its argument is off by at most
      u * [2*sum(R*A*C) + S + (Ax^2 + Ay^2) + S] <= u * [2*sum(R*A*C) + 3*S],
    which exp turns into the same relative error, plus one ulp (2u) of exp.
    Oracle: each of the three arguments is rounded once (u*A_d^2, together u*S),
    each exp is allowed one ulp (3 * 2u) and the two products round (2u).
    In all  tol = u * [2*sum(R*A*C) + 4*S + 10].
    The results stay normal: S <= 3*(lx/2 + 2*d)^2 ~ 80 in the tests, e^-80 ~ 1e-35.
    A cell shifted by one along any axis is off by exp(2*a*d) - 1 >= d^2 ~ 1e-3
    on the test grids, ten orders of magnitude above the bound."""
    from misc_oracles import _centred_1d

    u = 2.0**-53
    rac = s = 0.0
    for g0, n, d, off, ng, per, length in _dims(nx, ny, nz, geom, lx, ly, lz):
        A = float(max(abs(a) for a in _centred_1d(g0, n, d, off, ng, per, length)))
        C = (max(g0 + n, ng) + 1) * d + abs(off)
        rac += (9 if per else 4) * A * C
        s += A * A
    return u * (2 * rac + 4 * s + 10)
