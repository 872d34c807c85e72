"""Seeded cases of the 2D differential fuzz (test_fuzz2d_{cpu,gpu}.py) and their
package-independent references.

``kernel_case(seed)``: one launch of one core 2D kernel (march, the two-step kernel,
lds_dpp, pipec, pipe, piper, piper_nosb), everything drawn from
``random.Random(seed)`` and ``np.random.default_rng(seed)``: depth K, field or uniform
1/Cp, the cells per lane V (reached through nx and the base alignment, never forced),
an nx whose last strip holds 0, 1, 2 or V +- 1 columns, an ny around the chunk sizes,
coefficients and data over many orders of magnitude (finite and normal, with blocks
of equal values and of signed zeros), 1..8 disjoint rects cut at strip seams, lane
and 16-byte-pair boundaries and chunk boundaries, and a tuning. ``tiny_case(seed)``:
a whole field of at most 14 x 14 cells for a fast5 kernel. ``model_case(seed)``: one
``Diffusion2D`` run on tiles wider than one strip, on 1 or 2 loopback ranks. Every
case is valid: nothing is filtered at run time. Replay a failure with
``kernel_case(seed)`` / ``tiny_case(seed)`` / ``model_case(seed)``.

References: K applications of ``golden.step`` (NumPy) on the whole field for the
canonical kernels, bitwise on every cell; ``golden.run5`` (exact rationals) for the
fast5 kernels: on every cell of a tiny case (tier A) and, through the dependence
cone, on sampled cells of the seam-shaped cases with K <= 4 (tier B, CPU twin only;
the GPU is compared with the twin on every cell, bitwise). ``float(Fraction)`` loses
the sign of an exact zero, so the comparisons with the rational model are numeric
equality (``==``, every value finite); the sign of zero is pinned by the bitwise
GPU-versus-twin comparison of tier B.
"""
import random
from fractions import Fraction

import numpy as np

import golden
from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native

N_SEEDS = 240
N_TINY = 80
MAX_CELLS = 200_000
MAX_TINY_UPDATES = 3_500  # interior cells x K of a tiny case (14 x 14 at K = 24: 3 456)
MAX_SAMPLES = 16
MAX_RECTS = 8
SENTINEL, CANARY = -7.25, 1234.5

# kernel rows: name, share as drawn, entry point
ROWS = (("march", 0.08), ("tb2", 0.08), ("lds_dpp", 0.12), ("pipec", 0.16), ("pipe", 0.17),
        ("piper", 0.25), ("piper_nosb", 0.14))
FAST = ("pipe", "piper", "piper_nosb")
PIPE = ("pipec", "pipe", "piper", "piper_nosb")
ARITH = {"pipe": 0, "pipec": 1, "piper": 3, "piper_nosb": 13}  # kernel id - 9
CHUNKS = (1, 4, 7, 16, 37, 64)
NX_SMALL = tuple(range(3, 14))


def _depth(r, seed, kernel):
    """K of the row. The pipelined rows walk their depths with the seed, so that 240
    seeds meet every depth."""
    if kernel == "march":
        return 1
    if kernel == "tb2":
        return 2
    if kernel == "lds_dpp":
        return r.choice((2, 3, 4, 6, 8))
    if kernel == "piper_nosb":
        return 24
    if kernel == "pipe" and r.random() < 0.3:
        return r.randint(1, 4)  # the depths whose twin the exact model checks at the seams
    walk = seed + 3 * (seed // 24)  # shifted every 24 seeds: no depth tied to one residue
    if kernel == "piper":
        return 10 + walk % 15
    return 1 + walk % 24


def strip_geometry(kernel, K, V):
    """(halo, step): columns recomputed on each side of a strip and the output columns
    a strip advances. march and the two-step kernel: strips of 64 V columns on
    multiples of 64 V (plan_rects, halo 0: stencil.hip, stencil_tb.hip); lds_dpp and
    the pipelined kernels: windows of 64 V columns that output (64 V - 2 K) / V * V
    (plan_rects / plan_strip_tasks with halo K: stencil_kstep.hip, Geo::kStep in
    stencil_pipe.h)."""
    if kernel in ("march", "tb2"):
        return 0, 64 * V
    return K, (64 * V - 2 * K) // V * V


def first_column(kernel, K, V, x0):
    """First output column of the first strip of a rect starting at x0 (<= x0)."""
    halo, step = strip_geometry(kernel, K, V)
    if halo == 0:
        return x0 - x0 % step
    return (x0 - halo) // V * V + halo  # the lane-aligned start xa, plus the halo


def seams(kernel, K, V, x0, x1):
    """First columns of the second, third, ... strip of a rect [x0, x1)."""
    step = strip_geometry(kernel, K, V)[1]
    s = first_column(kernel, K, V, x0) + step
    out = []
    while s < x1:
        out.append(s)
        s += step
    return out


def _nx_seam(r, kernel, K, V, residues, mod):
    """An nx whose interior rect has 1, 2 or 3 strips, the last of them holding 0, 1,
    2, V - 1, V or V + 1 columns, with nx % mod in ``residues`` (the shape that gives
    V cells per lane)."""
    step = strip_geometry(kernel, K, V)[1]
    first = first_column(kernel, K, V, 1)
    pool = []
    for s in (1, 2, 3):
        start = max(1, first + (s - 1) * step)
        for e in sorted({0, 1, 2, V - 1, V, V + 1}):
            nx = start + e + 1
            if nx >= 3 and nx % mod in residues:
                pool.append(nx)
    return r.choice(pool)


def _cells_per_lane(kernel, K, nx, vec, aligned, uniform):
    """V the launch will run, from the launchers' host-side rules."""
    if kernel == "march":
        return ops.strip_cells(nx, vec) // 64 if aligned else 1
    if kernel == "tb2":  # stencil2_rects_gpu
        return 2 if aligned and nx % 2 == 0 else 1
    if kernel == "lds_dpp":  # kstep::check_launch
        if not (aligned and nx % 2 == 0):
            return 1
        return 4 if vec == 4 and nx % 4 == 0 else 2
    if uniform:
        return native().pipe_vec_uniform(K, 0, ARITH[kernel], nx, vec, aligned, True)
    return native().pipe_vec(K, 0, ARITH[kernel], nx, vec, aligned)


def _pick(r, pool, lo, hi):
    """A cut strictly inside (lo, hi) from the pool, else any; None where none fits."""
    inside = sorted({c for c in pool if lo < c < hi})
    if inside and r.random() < 0.85:
        return r.choice(inside)
    return r.randint(lo + 1, hi - 1) if hi - lo >= 2 else None


def _x_pool(r, kernel, K, V, root, lo, hi):
    """x cuts of a piece [lo, hi): the seams of the root rect and of the piece itself,
    lane and 16-byte-pair boundaries, each +- 1, and widths 1, 2, 3, V - 1, V, V + 1
    from either edge."""
    u = r.random()
    if u < 0.5:
        ss = seams(kernel, K, V, root[0], root[1]) + seams(kernel, K, V, lo, hi)
        pool = [s + d for s in ss for d in (-1, 0, 1)]
        if any(lo < c < hi for c in pool):
            return pool
    if u < 0.7 and hi - lo > 4:
        m = r.choice((V, 2))
        b = r.randint(lo + 1, hi - 1) // m * m
        return [b - 1, b, b + 1]
    ws = [w for w in (1, 2, 3, V - 1, V, V + 1) if w >= 1]
    return [lo + w for w in ws] + [hi - w for w in ws]


def _y_pool(K, chunk, root, lo, hi):
    """y cuts: chunk boundaries of the root rect and of the piece, +- 1, and rows
    K - 1, K, K + 1 from either edge."""
    pool = []
    for y0 in (root[2], lo):
        pool += [y0 + m * chunk + d for m in range(1, (hi - y0) // chunk + 2) for d in (-1, 0, 1)]
    pool += [lo + w for w in (K - 1, K, K + 1)] + [hi - w for w in (K - 1, K, K + 1)]
    return pool


def _rects(r, kernel, K, V, chunk, nx, ny):
    """1..8 disjoint rects: recursive cuts of the interior (or of the box K cells in),
    some pieces dropped so that gaps remain."""
    root = (1, nx - 1, 1, ny - 1)
    if r.random() < 0.3 and min(nx, ny) > 2 * K:
        root = (K, nx - K, K, ny - K)
    target = r.choice((1, 2, 3, 4, 5, 6, 6, 7, 7, 8, 8, 8))
    rects = [root]
    for _ in range(48):
        if len(rects) >= target:
            break
        i = r.randrange(len(rects))
        b = rects[i]
        w, h = b[1] - b[0], b[3] - b[2]
        axis = r.choices((0, 1), weights=(3 if w >= 2 else 0, 2 if h >= 2 else 0))[0] \
            if max(w, h) >= 2 else None
        if axis is None:
            continue
        lo, hi = b[2 * axis], b[2 * axis + 1]
        pool = _x_pool(r, kernel, K, V, root, lo, hi) if axis == 0 else _y_pool(K, chunk, root,
                                                                                  lo, hi)
        c = _pick(r, pool, lo, hi)
        if c is None:
            continue
        left, right = list(b), list(b)
        left[2 * axis + 1] = right[2 * axis] = c
        rects[i:i + 1] = [tuple(left), tuple(right)]
    kept = [b for b in rects if r.random() < 0.75]
    return kept or [r.choice(rects)]


def _coefficients(r, imax):
    lam = 10.0 ** r.uniform(-2, 2)
    dx = 10.0 ** r.uniform(-3, 1)
    u = r.random()
    if u < 0.2:
        dy = dx  # isotropic: ry == 1.0 exactly
    elif u < 0.3:
        dy = dx * 2.0 ** r.choice((-6, -5, -4, -3, -2, -1, 1, 2, 3, 4, 5, 6))
    else:
        dy = 10.0 ** r.uniform(-3, 1)
    limit = 1.0 / (2.0 * lam * imax * (1 / dx**2 + 1 / dy**2))
    dt = r.uniform(0.2, 1.0) * limit
    return (-lam, 1.0 / dx, 1.0 / dy, dt), limit


def _data(r, rng, shape):
    """T = off + scale U(-1, 1) with 2..5 blocks of one value each (a value in range,
    0.0 or -0.0), blocks on the array boundary included."""
    scale = 10.0 ** r.uniform(-6, 6)
    off = r.choice((0.0, scale, -3.0 * scale))
    T = off + scale * rng.uniform(-1.0, 1.0, shape)
    stamps = []
    for _ in range(r.randint(2, 5)):
        lo = [r.randrange(n) for n in shape]
        hi = [min(n, a + r.randint(1, 6)) for n, a in zip(shape, lo)]
        v = r.choice((off + scale * r.uniform(-1.0, 1.0), 0.0, -0.0))
        T[lo[0]:hi[0], lo[1]:hi[1]] = v
        stamps.append((tuple(lo), tuple(hi), v))
    return T, scale, off, stamps


def _samples(r, c):
    """Cells of the tier-B sample: rect corners, cells on both sides of every seam of
    a rect, then random cells inside rects; at most MAX_SAMPLES."""
    cells = []

    def add(y, x):
        if (y, x) not in cells:
            cells.append((y, x))

    for x0, x1, y0, y1 in c["rects"]:
        for y in (y0, y1 - 1):
            for x in (x0, x1 - 1):
                add(y, x)
    for x0, x1, y0, y1 in c["rects"]:
        for s in seams(c["kernel"], c["K"], c["V"], x0, x1):
            y = r.randrange(y0, y1)
            for x in (s - 1, s):
                if x0 <= x < x1:
                    add(y, x)
    cells = cells[:MAX_SAMPLES]
    for _ in range(MAX_SAMPLES - len(cells)):
        x0, x1, y0, y1 = r.choice(c["rects"])
        add(r.randrange(y0, y1), r.randrange(x0, x1))
    return cells


def kernel_case(seed):
    r = random.Random(seed)
    rng = np.random.default_rng(seed)
    kernel = r.choices([k for k, _ in ROWS], weights=[w for _, w in ROWS])[0]
    K = _depth(r, seed, kernel)
    uniform = kernel in ("piper", "piper_nosb") and r.random() < 0.5
    aligned = r.random() < 0.7
    six = (uniform and aligned and r.random() < 0.9 and
           native().pipe_vec_uniform(K, 0, ARITH[kernel], 1024, 6, True, True) == 6)
    # the cells per lane the shape shall give: 6 (any even nx), 4 (nx % 4 == 0), 2
    # (nx % 4 == 2), 1 (odd nx, or any nx on a base at 8 mod 16)
    if not aligned:
        want, residues, mod = 1, (0, 1), 2
    elif six:
        want, residues, mod = 6, (0, 2), 4
    else:
        top = 2 if kernel == "tb2" else 4
        want = r.choices((1, 2, top), weights=(1, 2, 3))[0]
        residues, mod = {1: ((1, 3), 4), 2: ((2,), 4), 4: ((0,), 4)}[want]
        if kernel == "tb2" and want == 2:
            residues = (0, 2)
    vec = 6 if six else 4
    if want == 2 and kernel != "tb2" and r.random() < 0.15:
        vec, residues = 2, (0, 2)  # two cells requested: any even nx
    if r.random() < 0.15:
        nx = r.choice([n for n in NX_SMALL if n % mod in residues])
    else:
        nx = _nx_seam(r, kernel, K, want, residues, mod)
    V = _cells_per_lane(kernel, K, nx, vec, aligned, uniform)

    chunk = r.choice(CHUNKS)
    pool = [K + 1, 3 * chunk + 1]
    pool += [K - 1] if K - 1 >= 3 else []
    pool += [r.randint(3, K - 1)] if K > 3 else []
    pool += [m * chunk + 2 + d for m in (1, 2, 3) for d in (-1, 1)]
    ny = r.choice(pool) if r.random() < 0.6 else r.randint(3, 40)
    ny = max(3, min(ny, MAX_CELLS // nx))
    shape = (ny, nx)

    value = r.uniform(0.5, 2.0)
    iCp = np.full(shape, value) if uniform else rng.uniform(0.5, 2.0, shape)
    coef, limit = _coefficients(r, float(iCp.max()))
    T, scale, off, stamps = _data(r, rng, shape)
    rects = _rects(r, kernel, K, V, chunk, nx, ny)
    tuning = dict(chunk_rows=chunk, xcd_remap=r.randint(0, 1))
    if kernel == "march":
        tuning.update(nontemporal=r.randint(0, 7), unroll=r.choice((2, 4, 8)), vec=vec)
    elif kernel == "tb2":
        tuning.update(nontemporal=r.randint(0, 3), unroll=r.choice((2, 4)))
    else:
        tuning.update(nontemporal=r.randint(0, 3), vec=vec, kernel=kernel)
    c = dict(seed=seed, kernel=kernel, K=K, uniform=uniform, value=value, aligned=aligned,
             want=want, V=V, shape=shape, coef=coef, limit=limit, scale=scale, off=off,
             stamps=stamps, rects=rects, tuning=tuning, T=T, iCp=iCp)
    c["samples"] = _samples(r, c)
    return c


def tiny_case(seed):
    """A whole field of at most 14 x 14 cells for a fast5 kernel at any depth it has:
    the interior rect, compared with the exact model on every cell."""
    r = random.Random(10_000 + seed)
    rng = np.random.default_rng(10_000 + seed)
    kernel = r.choice(FAST)
    K = 24 if kernel == "piper_nosb" else r.randint(10, 24) if kernel == "piper" else r.randint(1, 24)
    uniform = kernel != "pipe" and r.random() < 0.5
    ny, nx = r.randint(3, 14), r.randint(3, 14)
    assert (nx - 2) * (ny - 2) * K <= MAX_TINY_UPDATES
    aligned = r.random() < 0.7
    vec = 6 if uniform and r.random() < 0.5 else 4
    shape = (ny, nx)
    value = r.uniform(0.5, 2.0)
    iCp = np.full(shape, value) if uniform else rng.uniform(0.5, 2.0, shape)
    coef, limit = _coefficients(r, float(iCp.max()))
    T, scale, off, stamps = _data(r, rng, shape)
    tuning = dict(chunk_rows=r.choice(CHUNKS), xcd_remap=r.randint(0, 1),
                  nontemporal=r.randint(0, 3), vec=vec, kernel=kernel)
    return dict(seed=seed, kernel=kernel, K=K, uniform=uniform, value=value, aligned=aligned,
                V=_cells_per_lane(kernel, K, nx, vec, aligned, uniform), shape=shape, coef=coef,
                limit=limit, scale=scale, off=off, stamps=stamps,
                rects=[(1, nx - 1, 1, ny - 1)], tuning=tuning, T=T, iCp=iCp)


def describe(c):
    """The case without its arrays, for a failure message."""
    return {k: v for k, v in c.items() if k not in ("T", "iCp")}


def tuning_of(c, **over):
    """The case's launch tuning. The uniform variant gets its value as an argument."""
    kw = dict(c["tuning"])
    if c["kernel"] in PIPE:
        kw.update(uniform=c["uniform"], uniform_value=c["value"] if c["uniform"] else None)
    kw.update(over)
    return ops.StencilTuning(**kw)


def run_kernel(c, T2, T, iCp, tuning=None):
    """One launch of the case's kernel through its entry point, on the tensors'
    device (CPU tensors: the package's CPU twin of the arithmetic)."""
    coef = ops.StencilCoef(*c["coef"])
    tn = tuning or tuning_of(c)
    if c["kernel"] == "march":
        ops.stencil_step(T2, T, iCp, coef, c["rects"], tn)
    elif c["kernel"] == "tb2":
        ops.stencil2_step(T2, T, iCp, coef, c["rects"], tn)
    else:
        ops.stencilk_step(c["K"], T2, T, iCp, coef, c["rects"], tn)


def twin(c):
    """The package's CPU twin on CPU tensors, from a sentinel T2, fed the array."""
    import torch

    T2 = torch.full(c["shape"], SENTINEL, dtype=torch.float64)
    run_kernel(c, T2, torch.from_numpy(c["T"]), torch.from_numpy(c["iCp"]))
    return T2.numpy()


def inside_mask(c):
    m = np.zeros(c["shape"], dtype=bool)
    for x0, x1, y0, y1 in c["rects"]:
        assert not m[y0:y1, x0:x1].any(), "rects overlap"
        m[y0:y1, x0:x1] = True
    return m


def crop(c, full):
    """``full`` on the rects, the sentinel everywhere else."""
    want = np.full(c["shape"], SENTINEL)
    m = inside_mask(c)
    want[m] = full[m]
    return want


def canonical_reference(c):
    """K applications of golden.step on the whole field (the boundary keeps T),
    cropped to the rects."""
    a = c["T"]
    for _ in range(c["K"]):
        a = golden.step(a, c["iCp"], *c["coef"])
    return crop(c, a)


def exact_reference(c):
    """golden.run5 (exact rationals) on the whole field, cropped to the rects."""
    return crop(c, golden.run5(c["T"], c["iCp"], c["K"], *c["coef"]))


def fast5_sample_reference(c):
    """[(cell, value)]: the exact fast5 model on the sampled cells, through the
    dependence cone: level j of a cell is the rational fused update of the five
    level j - 1 values around it, a boundary cell keeps T at every level."""
    T, iCp = c["T"], c["iCp"]
    ny, nx = c["shape"]
    ry, mkc, gs = golden.fast5_constants(*c["coef"])
    fry, fmkc = Fraction(ry), Fraction(mkc)
    memo = {}

    def level(j, y, x):
        if j == 0 or y == 0 or x == 0 or y == ny - 1 or x == nx - 1:
            return float(T[y, x])
        key = (j, y, x)
        if key not in memo:
            cc = level(j - 1, y, x)
            sx = level(j - 1, y, x + 1) + level(j - 1, y, x - 1)
            sy = level(j - 1, y - 1, x) + level(j - 1, y + 1, x)
            t = float(fmkc * Fraction(cc) + Fraction(sx))
            t = float(fry * Fraction(sy) + Fraction(t))
            memo[key] = float(Fraction(gs * float(iCp[y, x])) * Fraction(t) + Fraction(cc))
        return memo[key]

    return [((y, x), level(c["K"], y, x)) for y, x in c["samples"]]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def first_difference(same):
    return tuple(int(v) for v in np.argwhere(~same)[0])


# ---------------------------------------------------------------------------
# model fuzz: Diffusion2D on tiles wider than one strip, 1 or 2 loopback ranks
# ---------------------------------------------------------------------------
MODEL_DIMS = ((1, 1), (2, 1), (1, 2))
ICP_SEED = 4321
N_MODEL_CPU, N_MODEL_GPU = 12, 12


def model_case(seed):
    r = random.Random(20_000 + seed)
    # half of the depths from the six-cell range: with a uniform 1/Cp and fast-math
    # arithmetic those passes run six cells per lane under RMA_DIAG=pipe_cells=6
    K = r.randint(17, 24) if r.random() < 0.5 else r.randint(1, 24)
    return dict(seed=seed, dims=r.choice(MODEL_DIMS), K=K, nx=r.randint(300, 1100),
                ny=4 * K + r.randint(6, 90), nt=r.randint(1, 2 * K + 3),
                variant=r.choice(("perf", "perf_hide")), fast=r.random() < 0.7,
                bw=(r.randint(1, 9), r.randint(1, 9)),
                periods=(int(r.random() < 0.3), int(r.random() < 0.3)),
                icp=r.choice(("uniform", "random")), cells=r.choice((4, 6, 6)))


def model_spmd(rank, hub, c, device):
    from rocm_mpi_amd.models import Diffusion2D, DiffusionConfig
    from rocm_mpi_amd.parallel import implicit_grid as gg

    K, dims, per = c["K"], c["dims"], c["periods"]
    gpu = device != "cpu"
    gg.init_global_grid(c["nx"], c["ny"], 1, dimx=dims[0], dimy=dims[1], periodx=per[0],
                        periody=per[1], overlaps=(2 * K, 2 * K, 2), halowidths=(K, K, 1),
                        quiet=True, loopback=(hub, rank), device=device)
    m = Diffusion2D(DiffusionConfig(variant=c["variant"], nx=c["nx"], ny=c["ny"], nt=c["nt"],
                                    init="random", quiet=True, dims=(*dims, 0), temporal=K,
                                    fast_math=c["fast"], b_width=c["bw"], device=device,
                                    periods=(*per, 0), executor="native" if gpu else "auto"))
    assert (m.executor is not None) == gpu
    if c["icp"] == "random":  # decomposition-invariant, below 1/Cp0 = 1: dt stays stable
        ops.init_random_(m.iCp, m.geometry(), seed=ICP_SEED, lo=0.5, hi=1.0)
        if gpu:  # a write torch does not see
            m.executor.rescan_factor()
    if gpu:  # only the fast-math passes have a uniform-factor kernel
        assert bool(m.executor.uniform_factor) == (c["icp"] == "uniform" and c["fast"])
        assert sum(m.plan(c["nt"])) == c["nt"]
    m.step(c["nt"])
    out = (tuple(m.g.coords), m.field.cpu().numpy().copy(), tuple(m.g.nxyz_g))
    m.close()
    gg.finalize_global_grid()
    return out


def model_check(seed, device):
    """Every rank's tile == the same window of a 1-rank CPU run of the global grid,
    bitwise."""
    from helpers import run_loopback

    c = model_case(seed)
    P = c["dims"][0] * c["dims"][1]
    res = run_loopback(P, model_spmd, c, device, timeout=180)
    nxg, nyg, _ = res[0][2]
    # the 1-rank grid with the same global size: a periodic dimension keeps its
    # overlap on top, so tile c's window starts at c * (nx - ol) in both cases
    K = c["K"]
    one = dict(c, nx=nxg + 2 * K * c["periods"][0], ny=nyg + 2 * K * c["periods"][1], dims=(1, 1))
    ref = run_loopback(1, model_spmd, one, "cpu", timeout=180)[0][1]
    assert len(res) == P and len({co for co, _, _ in res}) == P
    for coords, tile, _ in res:
        gx0, gy0 = coords[0] * (c["nx"] - 2 * K), coords[1] * (c["ny"] - 2 * K)
        want = ref[gy0:gy0 + c["ny"], gx0:gx0 + c["nx"]]
        same = bits(tile) == bits(want)
        assert same.all(), (f"seed {seed}: {int((~same).sum())} cells differ on rank {coords}, "
                            f"first (y, x) = {first_difference(same)}; case {c}")
