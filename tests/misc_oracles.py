"""Independent oracles for the utility kernels of csrc/kernels/misc.hip, shared by
test_misc_kernels_cpu.py / test_misc_kernels_gpu.py: initial conditions, fill, plane
copies, reductions, field statistics and the roofline probes.

Every oracle is written from the definition of the operation, in NumPy / Python
integers and exact rationals; nothing here imports the package's own geometry or
ops code. ``geom`` is any object with the attributes gx0, gy0, nxg, nyg, dx, dy,
xoff, yoff, periodx, periody (placement of a local tile in the global grid).

All oracles but the Gaussian are exact and independent of the order in which a
kernel visits or combines the cells, so the tests compare with ``==`` on values
or bit patterns. The Gaussian has a derived bound (``gaussian_tolerance``).
"""
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np
import torch

M64 = 2**64
GOLDEN = 0x9E3779B97F4A7C15
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB


@dataclass
class Geom:
    """Placement of a local tile in the global grid (the fields of the kernels'
    TileGeom): pass to the ops as ``ops.TileGeometry(**dataclasses.asdict(g))``."""

    gx0: int
    gy0: int
    nxg: int
    nyg: int
    dx: float
    dy: float
    xoff: float = 0.0
    yoff: float = 0.0
    periodx: int = 0
    periody: int = 0


TILES = [(1, 1), (3, 5), (128, 128), (1025, 1031)]  # (ny, nx)
PERIODS = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (periodx, periody)
SEEDS = [0, 42, 2**63 + 5, 2**64 - 1]
LX, LY = 10.0, 7.0  # anisotropic: dx = LX / nxg != dy = LY / nyg


def init_geoms(ny, nx, periods, stagger=False):
    """Placements of an (ny, nx) tile in a global grid of (2*ny + 3, 2*nx + 5)
    cells that straddle the periodic wrap: g0 = 0 (the ghost cell maps to global
    n - 1) and g0 = n_g - 3 (the tile runs over the far edge into the next
    period; the grid is more than twice the tile, so one wrap brings every cell
    back). An open dimension takes the first and the last tile of the grid
    instead. With ``stagger`` each placement also comes with the offsets
    (+dx/2, -dy/2) and (-dx/2, +dy/2) of a staggered field."""
    px, py = periods
    nxg, nyg = 2 * nx + 5, 2 * ny + 3
    dx, dy = LX / nxg, LY / nyg
    out = []
    for far in (0, 1):
        gx0 = 0 if not far else (nxg - 3 if px else nxg - nx)
        gy0 = 0 if not far else (nyg - 3 if py else nyg - ny)
        for sx, sy in ((0, 0), (1, -1), (-1, 1)) if stagger else ((0, 0),):
            out.append(Geom(gx0, gy0, nxg, nyg, dx, dy, sx * dx / 2, sy * dy / 2, px, py))
    return out


# ---------------------------------------------------------------------------
# init_random: counter-based uniform field keyed by the global cell index
# ---------------------------------------------------------------------------
def global_index_1d(g0, n_local, n_global, periodic):
    """Global cell index of each local cell of one dimension. On a periodic
    dimension the first local cell of the grid is a ghost: g -> (g - 1) mod n;
    on an open dimension g is unchanged."""
    g = g0 + np.arange(n_local, dtype=np.int64)
    return (g - 1) % n_global if periodic else g  # NumPy's % is a floor modulo: >= 0


def uniform_field(nx, ny, geom, seed, lo, hi):
    """(ny, nx) float64 field: splitmix64 finaliser of seed + (idx + 1) * GOLDEN
    with idx = gy * nxg + gx, the top 53 bits scaled by 2**-53 to [0, 1), then
    lo + (hi - lo) * u in float64 (a multiply, then an add)."""
    gx = global_index_1d(geom.gx0, nx, geom.nxg, geom.periodx)
    gy = global_index_1d(geom.gy0, ny, geom.nyg, geom.periody)
    with np.errstate(over="ignore"):
        idx = (gy[:, None] * np.int64(geom.nxg) + gx[None, :]).astype(np.uint64)
        z = np.uint64(seed % M64) + (idx + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(11)).astype(np.float64) * 2.0**-53  # < 2**53: the conversion is exact
    return np.float64(lo) + (np.float64(hi) - np.float64(lo)) * u


def uniform_cell(ix, iy, geom, seed, lo, hi):
    """Scalar twin of ``uniform_field`` for one local cell, in Python ``int``
    arithmetic modulo 2**64: no NumPy, no wrapping types."""
    gx = geom.gx0 + ix
    gy = geom.gy0 + iy
    if geom.periodx:
        gx = (gx - 1) % geom.nxg
    if geom.periody:
        gy = (gy - 1) % geom.nyg
    idx = (gy * geom.nxg + gx) % M64
    z = (seed + (idx + 1) * GOLDEN) % M64
    z = ((z ^ (z >> 30)) * MIX1) % M64
    z = ((z ^ (z >> 27)) * MIX2) % M64
    z ^= z >> 31
    return lo + (hi - lo) * ((z >> 11) * 2.0**-53)


# ---------------------------------------------------------------------------
# init_gaussian: exp(-(x_g + dx/2 - lx/2)^2 - (y_g + dy/2 - ly/2)^2)
# ---------------------------------------------------------------------------
def _centred_1d(g0, n_local, d, off, n_global, periodic, length):
    """Exact a_i = x_i + d/2 - length/2 of one dimension, as Fractions.
    x = (g0 + i) * d + off; periodic: shift by -d, then wrap into [0, n*d)."""
    d, off, length = Fraction(d), Fraction(off), Fraction(length)
    out = []
    for i in range(n_local):
        x = (g0 + i) * d + off
        if periodic:
            x = (x - d) % (n_global * d)  # Fraction % is a floor modulo: in [0, n*d)
        out.append(x + d / 2 - length / 2)
    return out


def _dyadic_ints(fracs):
    """Fractions of float64 values have power-of-two denominators: return
    (numerators over the common denominator, that denominator)."""
    den = max(f.denominator for f in fracs)
    assert den & (den - 1) == 0
    return [f.numerator * (den // f.denominator) for f in fracs], den


def gaussian_args(nx, ny, geom, lx, ly):
    """(ny, nx) float64 array of the exponent -(a^2 + b^2) of
    scripts/diffusion_2D_ap.jl:28, every coordinate an exact rational of the
    float64 dx, dy, xoff, yoff, lx, ly; rounded to float64 once, at the end
    (Python's int / int is correctly rounded)."""
    a2, da = _dyadic_ints([a * a for a in _centred_1d(geom.gx0, nx, geom.dx, geom.xoff,
                                                      geom.nxg, geom.periodx, lx)])
    b2, db = _dyadic_ints([b * b for b in _centred_1d(geom.gy0, ny, geom.dy, geom.yoff,
                                                      geom.nyg, geom.periody, ly)])
    den = max(da, db)
    a2 = np.array([v * (den // da) for v in a2], dtype=object)
    b2 = np.array([v * (den // db) for v in b2], dtype=object)
    s = -(b2[:, None] + a2[None, :])  # exact Python integers
    return (s / den).astype(np.float64)


def gaussian_field(nx, ny, geom, lx, ly):
    return np.exp(gaussian_args(nx, ny, geom, lx, ly))


def gaussian_tolerance(nx, ny, geom, lx, ly):
    """Relative bound on |kernel - exp(gaussian_args)|, to first order, from the
    kernel's documented operation sequence (csrc/kernels/misc.hip, global_coord
    and init_gaussian_kernel; built without contraction, so each operation below
    rounds once, by at most u = 2**-53 relative to its result).

    Per dimension (x shown; y alike), the centred coordinate a is formed by
      g*dx, + xoff, [periodic: - dx, then either wrap: n*dx and - or + it, at
      worst both wraps one after the other], + dx/2, - lx/2
    (dx/2 and lx/2 are exact): R = 4 roundings on an open dimension, at most
    R = 9 on a periodic one. Every intermediate is at most
      C = (max(gx0 + nx, nxg) + 1) * dx + |xoff|
    in magnitude (the unwrapped coordinate, n*dx, or their sum/difference), so
      |da| <= R * u * C.
    With A = max |a| over the tile (from the exact rationals), a*a is off by
    2*A*|da| from the perturbed a plus u*A^2 from its own rounding. -(a*a) is
    exact; the subtraction of b*b rounds a quantity of at most Ax^2 + Ay^2. The
    oracle rounds its exact exponent once more, by u*(Ax^2 + Ay^2). In all
      |d arg| <= u * [2*(Rx*Ax*Cx + Ry*Ay*Cy) + 3*(Ax^2 + Ay^2)].
    exp turns an absolute error of its argument into the same relative error of
    its result (e^t - 1 ~ t). The device exp and NumPy's are each allowed one ulp
    of the result, 2**-52 = 2*u relative:
      tol = u * [2*(Rx*Ax*Cx + Ry*Ay*Cy) + 3*(Ax^2 + Ay^2) + 4].

    Scale: the 128 x 128 tile at gx0 = 126 of an open 254 x 254 grid with
    lx = ly = 10, dx = dy = 10/254 (the existing GPU test's) has A = 4.98,
    C = 10.04, R = 4: tol = 1.06e-13. The doubly periodic 1025 x 1031 tile of
    ``init_geoms`` that starts three cells before the far edges (lx = 10, ly = 7)
    reaches Cx = 15.0, R = 9: tol = 2.36e-13. A cell wrapped to the wrong period
    is off by a factor exp(2*a*n*dx -+ (n*dx)^2), a cell shifted by one by
    exp(2*a*dx) - 1 >= dx^2 ~ 2e-5: both orders of magnitude above the bound
    everywhere.
    """
    u = 2.0**-53

    def dim(g0, n_local, d, off, n_global, periodic, length):
        A = float(max(abs(a) for a in _centred_1d(g0, n_local, d, off, n_global, periodic,
                                                   length)))
        C = (max(g0 + n_local, n_global) + 1) * d + abs(off)
        return (9 if periodic else 4), A, C

    Rx, Ax, Cx = dim(geom.gx0, nx, geom.dx, geom.xoff, geom.nxg, geom.periodx, lx)
    Ry, Ay, Cy = dim(geom.gy0, ny, geom.dy, geom.yoff, geom.nyg, geom.periody, ly)
    return u * (2 * (Rx * Ax * Cx + Ry * Ay * Cy) + 3 * (Ax * Ax + Ay * Ay) + 4)


def max_rel_dev(got, want):
    """Largest |got - want| / |want| (want > 0 everywhere: it is an exp)."""
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs(got - want) / want))


# ---------------------------------------------------------------------------
# reductions / field statistics: exact, order-independent fields
# ---------------------------------------------------------------------------
def integer_field(n, seed):
    """float64 array of random integers in [-2**20, 2**20] and its exact sum.
    Any partial sum of up to 2**32 such cells is below 2**53: exact in any order."""
    v = np.random.default_rng(seed).integers(-2**20, 2**20, size=n, endpoint=True, dtype=np.int64)
    return v.astype(np.float64), int(v.sum())


def background(n, seed):
    """float64 values in (-1, 1), none of them a zero of either sign."""
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, size=n)
    v[v == 0.0] = 0.5
    return v


def planted_positions(n, stride, seed, extra=()):
    """Cells at which to plant an extreme: wave and block edges, the last thread
    of the first grid stride and the first of the second (``stride`` cells per
    sweep of the grid), the last two cells, three seeded random cells, and any
    ``extra`` positions; those inside [0, n), each once."""
    rng = np.random.default_rng(seed)
    cand = [0, 1, 63, 64, 255, 256, stride - 1, stride, n - 2, n - 1, *extra,
            *(int(p) for p in rng.integers(0, n, size=3))]
    return sorted({p for p in cand if 0 <= p < n})


def bits(a):
    """float64 array -> int64 bit patterns (NaN payloads and signed zeros count)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def reduce_expected(a):
    """The five reductions of a float64 array with the native semantics: ``sum``
    propagates NaN (and inf - inf); ``max``, ``min`` and ``maxabs`` ignore NaN
    (fmax / fmin) and return their identity (-inf, inf, 0) when nothing else is
    there; +-inf count for them; ``nonfinite`` counts NaN and +-inf. ``sum`` is
    None when it is not exact in every order (a finite non-integer field)."""
    nan, pinf, ninf = np.isnan(a).any(), (a == np.inf).any(), (a == -np.inf).any()
    if nan or (pinf and ninf):
        total = float("nan")
    elif pinf or ninf:
        total = float("inf") if pinf else float("-inf")
    elif (a == np.rint(a)).all() and np.abs(a).max(initial=0.0) <= 2**20:
        total = float(int(a.astype(np.int64).sum()))
    else:
        total = None
    return {"sum": total,
            "max": float(np.fmax.reduce(a, initial=-np.inf)),
            "min": float(np.fmin.reduce(a, initial=np.inf)),
            "maxabs": float(np.fmax.reduce(np.abs(a), initial=0.0)),
            "nonfinite": float(np.count_nonzero(~np.isfinite(a)))}


def stats_expected(a):
    """(non-finite count, min, max of the finite cells); (n, inf, -inf) if none is."""
    fin = np.isfinite(a)
    return (float(a.size - np.count_nonzero(fin)), float(np.min(a, where=fin, initial=np.inf)),
            float(np.max(a, where=fin, initial=-np.inf)))


def same(got, want):
    """Equality of two floats that treats NaN by mask, never with ``==``."""
    return math.isnan(got) if math.isnan(want) else got == want


# ---------------------------------------------------------------------------
# drivers shared by the CPU and the GPU file: ``red(field, op) -> float`` and
# ``stats(field) -> (bad, lo, hi)`` are the code under test, on torch tensors
# ---------------------------------------------------------------------------
def to_field(a, device, offset=0):
    """The array as a 1-D float64 tensor on ``device``, ``offset`` elements into
    its allocation (offset 1: 8 bytes off the 16-byte alignment)."""
    base = torch.empty(a.size + offset, dtype=torch.float64, device=device)
    f = base[offset:]
    f.copy_(torch.from_numpy(a))
    return f


def _check_red(red, f, a, what):
    for op, want in reduce_expected(a).items():
        if want is not None:
            got = float(red(f, op))
            assert same(got, want), f"{what}: reduce {op} of {a.size} cells gave {got!r}, want {want!r}"


def _check_stats(stats, f, a, what):
    got, want = tuple(float(v) for v in stats(f)), stats_expected(a)
    assert got == want, f"{what}: field_stats of {a.size} cells gave {got!r}, want {want!r}"


def _special_fields(n, seed, positions):
    """Special-value fields as (name, array): all ones, all NaN, one NaN, +inf,
    -inf, and NaN with both infinities, on a background in (-1, 1)."""
    bg = background(n, seed)
    yield "ones", np.ones(n)
    yield "all-NaN", np.full(n, np.nan)
    p = positions
    for name, vals in (("NaN", [np.nan]), ("+inf", [np.inf]), ("-inf", [-np.inf]),
                       ("NaN,+inf,-inf", [np.nan, np.inf, -np.inf])):
        if len(vals) <= len(p):
            a = bg.copy()
            for k, v in enumerate(vals):  # one value: a middle position; three: the last cells
                a[p[len(p) // 2] if len(vals) == 1 else p[-1 - k]] = v
            yield name, a


def check_reduce(red, device, n, offset, stride, seed):
    """Every reduce check of one (n, offset): exact integer sum and extremes,
    all-ones, all-NaN, NaN / inf semantics, and one planted +-7 per launch at
    each of ``planted_positions`` (``stride`` = cells per sweep of the grid)."""
    a, total = integer_field(n, seed)
    f = to_field(a, device, offset)
    got = float(red(f, "sum"))
    assert got == total, f"integer sum of {n} cells gave {got!r}, want {total}"
    _check_red(red, f, a, "integers")
    pos = planted_positions(n, stride, seed + 1)
    for name, a in _special_fields(n, seed + 2, pos):
        f.copy_(torch.from_numpy(a))
        _check_red(red, f, a, name)
    a = background(n, seed + 3)
    f.copy_(torch.from_numpy(a))
    for p in pos:
        for v, ops_ in ((7.0, ("max", "maxabs", "min")), (-7.0, ("min", "maxabs", "max"))):
            old, a[p] = a[p], v
            f[p] = v
            want = {"max": float(a.max()), "min": float(a.min()), "maxabs": float(np.abs(a).max())}
            assert want["maxabs"] == 7.0 and want[ops_[0]] == v
            for op in ops_:
                got = float(red(f, op))
                assert got == want[op], f"{v} planted at {p} of {n}: {op} gave {got!r}, want {want[op]!r}"
            a[p] = old
            f[p] = old


def check_field_stats(stats, device, n, offset, stride, seed, extra=()):
    """The same for field_stats: ``stride`` = cells per sweep of the grid on the
    16-byte path, ``extra`` further positions to plant at."""
    a, _ = integer_field(n, seed)
    f = to_field(a, device, offset)
    _check_stats(stats, f, a, "integers")
    pos = planted_positions(n, stride, seed + 1, extra)
    for name, a in _special_fields(n, seed + 2, pos):
        f.copy_(torch.from_numpy(a))
        _check_stats(stats, f, a, name)
    a = background(n, seed + 3)
    f.copy_(torch.from_numpy(a))
    for p in pos:
        for v in (7.0, -7.0, np.nan):
            old, a[p] = a[p], v
            f[p] = v
            _check_stats(stats, f, a, f"{v} planted at {p}")
            a[p] = old
            f[p] = old


# ---------------------------------------------------------------------------
# plane copies: bitwise against a torch slice assignment
# ---------------------------------------------------------------------------
def as_bits(t):
    """Any tensor as a contiguous integer tensor of its bit patterns."""
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def rand_field(shape, dtype, device, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(shape, generator=g, dtype=torch.float64) - 0.5
    if dtype == torch.complex128:
        r = torch.complex(r, torch.rand(shape, generator=g, dtype=torch.float64) - 0.5)
    return r.to(dtype).to(device)


def _sl(r0, r1, c0, c1):
    return (slice(r0, r1), slice(c0, c1))


def _tiny_copies(even):
    """Seven tiny planes "t_src" -> "t_dst" (9 x 13 or 10 x 14 fields) with
    disjoint destinations; ``even``: columns and widths even (16-byte elements)."""
    if even:
        planes = [(0, 10, 0, 2), (0, 1, 2, 6), (1, 9, 2, 4), (1, 10, 4, 6), (0, 3, 6, 14),
                  (3, 10, 6, 8), (3, 4, 8, 14)]
    else:
        planes = [(0, 9, 0, 1), (0, 1, 1, 4), (1, 9, 1, 2), (1, 8, 2, 5), (0, 3, 5, 13),
                  (3, 9, 5, 6), (3, 4, 6, 13)]
    return [("t_dst", _sl(*p), "t_src", _sl(*p)) for p in planes]


def copy_case(name, device):
    """(fields, copies) of one launch: ``fields`` name -> 2-D tensor, ``copies``
    [(dst name, dst slices, src name, src slices)]. Block counts follow
    copy2d_batch_gpu (csrc/kernels/misc.hip): 256-thread blocks, rows of
    n_k <= 128 elements take 256 // n_k rows per block, wider rows one block per
    (row, 256-element chunk); the grid is capped at 256 * 8 = 2048 blocks in x."""
    f64, c128, f16 = torch.float64, torch.complex128, torch.float16

    def two(shape, dtype=f64, shape_b=None):
        return {"a": rand_field(shape, dtype, device, 1),
                "b": rand_field(shape_b or shape, dtype, device, 2)}

    if name == "narrow_8B_beyond_cap":
        # odd leading dimension: 8-byte elements; n_k = 128: 2 rows per block, 2050 blocks
        return two((4100, 257)), [("b", _sl(0, 4100, 100, 228), "a", _sl(0, 4100, 3, 131))]
    if name == "narrow_16B_beyond_cap":
        # the K = 24 x-halo's shape class: 24 fp64 move as 12 16-byte elements, 21 rows per
        # block, ceil(43100 / 21) = 2053 blocks
        return (two((43100, 48), shape_b=(43100, 50)),
                [("b", _sl(0, 43100, 2, 26), "a", _sl(0, 43100, 24, 48))])
    if name == "wide_8B_beyond_cap":
        # odd offsets: 8-byte elements; 600 columns = 3 chunks per row, 700 * 3 = 2100 units
        return two((700, 1301)), [("b", _sl(0, 700, 7, 607), "a", _sl(0, 700, 501, 1101))]
    if name.startswith("edge_"):
        # the narrow/wide switch n_k * 2 <= 256 (8-byte elements: odd leading dimension);
        # at n_k = 100 a block holds 2 rows and 56 of its threads idle
        nk = int(name[5:])
        return (two((300, 2 * nk + 5)),
                [("b", _sl(0, 300, 1, 1 + nk), "a", _sl(0, 300, nk + 2, 2 * nk + 2))])
    if name == "complex128_narrow":  # elem_bytes = 16 asked for directly
        return two((301, 40), c128), [("b", _sl(0, 301, 25, 37), "a", _sl(0, 301, 3, 15))]
    if name == "complex128_wide":
        return two((67, 700), c128), [("b", _sl(0, 67, 391, 691), "a", _sl(0, 67, 5, 305))]
    if name == "float16_narrow":
        return two((301, 41), f16), [("b", _sl(0, 301, 30, 37), "a", _sl(0, 301, 3, 10))]
    if name == "float16_wide":
        return two((67, 1301), f16), [("b", _sl(0, 67, 650, 1251), "a", _sl(0, 67, 5, 606))]
    if name in ("batch_8B_one_beyond_cap", "batch_16B_one_beyond_cap"):
        even = "16B" in name  # the grid is sized by the big copy: the tiny ones see surplus blocks
        fields, copies = copy_case("narrow_16B_beyond_cap" if even else "narrow_8B_beyond_cap",
                                   device)
        shape = (10, 14) if even else (9, 13)
        fields["t_src"] = rand_field(shape, f64, device, 3)
        fields["t_dst"] = rand_field(shape, f64, device, 4)
        tiny = _tiny_copies(even)
        return fields, tiny[:3] + copies + tiny[3:]
    raise KeyError(name)


COPY_CASES = ["narrow_8B_beyond_cap", "narrow_16B_beyond_cap", "wide_8B_beyond_cap", "edge_100",
              "edge_128", "edge_129", "edge_257", "complex128_narrow", "complex128_wide",
              "float16_narrow", "float16_wide", "batch_8B_one_beyond_cap",
              "batch_16B_one_beyond_cap"]


def check_copy_case(copy, name, device):
    """Run one launch ``copy([(dst view, src view), ...])`` and compare every field
    bitwise with slice assignments on clones: the destination planes hold the
    source planes, every other cell (sources included) is unchanged."""
    fields, copies = copy_case(name, device)
    ref = {k: v.clone() for k, v in fields.items()}
    for d, dsl, s, ssl in copies:
        ref[d][dsl] = fields[s][ssl]
    copy([(fields[d][dsl], fields[s][ssl]) for d, dsl, s, ssl in copies])
    for k in fields:
        assert torch.equal(as_bits(fields[k]), as_bits(ref[k])), f"{name}: field {k!r} differs"
