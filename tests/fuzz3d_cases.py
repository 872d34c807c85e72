"""Seeded cases of the 3D differential fuzz (test_fuzz3d_{cpu,gpu}.py and
test_fuzz3d_model_{cpu,gpu}.py) and their package-independent references.

``kernel_case(seed)``: one launch of the one- or two-step 3D kernel, everything
drawn from ``random.Random(seed)``: K, arithmetic, field or uniform 1/Cp, a shape
whose nx sits at a strip seam, base alignment, coefficients and data over many
orders of magnitude (finite and normal, with blocks of equal values and of signed
zeros), 1..8 disjoint boxes cut at the dispatch limits and at strip seams deep in
the array, and a tuning. ``model_case(seed)``: one multi-rank ``Diffusion3D`` run
on loopback rank threads. Every case is valid: nothing is filtered at run time.
Replay a failure with ``kernel_case(seed)`` / ``model_case(seed)``.

References: ``golden3d.step3`` / ``golden3d.run3`` (NumPy) for the canonical
arithmetic, ``golden3d_fast.cell7`` (exact rationals) for fast7.
"""
import random
from types import SimpleNamespace

import numpy as np

import golden3d
import golden3d_fast
from rocm_mpi_amd import ops

N_SEEDS = 240
MAX_CELLS = 250_000
MAX_SAMPLES = 64
MAX_BOXES = 8  # boxes a launch takes (ops.stencil3d.MAX_BOXES)
SENTINEL, CANARY = -7.25, 1234.5

# box widths on both sides of every dispatch limit (thin: 8; x-face classes: 8, 16,
# 32 lanes, two columns fewer in a two-step pass) and strip seams deep in the array
# (64 / 128 cells a strip, advance 62 / 126 in a two-step pass), each +- 1
WIDTHS = (1, 6, 7, 8, 9, 14, 15, 16, 17, 30, 31, 32, 33)
SEAMS = (62, 63, 64, 126, 127, 128, 129, 130, 252, 253, 254, 255, 256, 257, 258)
SEAM_CUTS = tuple(sorted({s + d for s in SEAMS for d in (-1, 0, 1)}))
NX_SMALL = tuple(range(3, 13))
NX_SEAM = tuple(sorted({s * m + d for m in (64, 126, 128) for s in (1, 2, 3)
                        for d in range(-2, 4)}))
# rows R = 2, 4, 8: R + 2, R + 3, 4R + 3; 3 and 4 leave fewer interior planes / rows
# than the two-step margin
N_SPECIAL = (3, 4, 5, 6, 7, 10, 11, 19, 35)
WIDTH_CLASSES = ((1, 6, 7, 8), (9, 14, 15, 16), (17, 30, 31, 32, 33))
CLASS_WEIGHTS = (2, 2, 3)  # as drawn: a wide slab fits least often
CHUNKS = (0, 1, 1, 2, 3, 5)  # as drawn: one plane per task twice as often
# x-face limits as drawn (K: cumulative probability, pool): off, each lanes class at
# and just under its widest box (a two-step box needs two more lanes than its width)
XFACE_DRAW = {1: ((0.27, (0,)), (0.67, (30, 32, 32)), (0.80, (14, 16, 16)), (0.90, (6, 8, 8))),
              2: ((0.12, (0,)), (0.55, (30, 30, 32)), (0.75, (14, 14, 16)), (0.90, (6, 6, 8)))}


def _extent(r):
    return r.choice(N_SPECIAL) if r.random() < 0.5 else r.randint(3, 40)


def _x_cut(r, lo, hi):
    """A cut strictly inside (lo, hi), from the seam and width pools where they reach."""
    seams = [c for c in SEAM_CUTS if lo < c < hi]
    widths = sorted({c for w in WIDTHS for c in (lo + w, hi - w) if lo < c < hi})
    u = r.random()
    if seams and u < 0.5:
        return r.choice(seams)
    if widths and u < 0.9:
        return r.choice(widths)
    return r.randint(lo + 1, hi - 1) if hi - lo >= 2 else None


def _slab(r, b):
    """Cut a slab of a pool width (its class drawn first: narrow, middle, wide) at a
    pool origin out of box b: [left, slab, right], or None where none fits."""
    lo, hi = b[0], b[1]
    o = _x_cut(r, lo, hi)
    ws = [w for w in r.choices(WIDTH_CLASSES, weights=CLASS_WEIGHTS)[0] if o is not None and o + w < hi]
    if not ws:
        return None
    w = r.choice(ws)
    return [(lo, o) + b[2:], (o, o + w) + b[2:], (o + w, hi) + b[2:]]


def _boxes(r, K, nx, ny, nz):
    """1..8 disjoint boxes: random recursive cuts of the interior (or of the box K
    cells in), some pieces dropped so that gaps remain."""
    root = (1, nx - 1, 1, ny - 1, 1, nz - 1)
    if r.random() < 0.3 and min(nx, ny, nz) > 2 * K:
        root = (K, nx - K, K, ny - K, K, nz - K)
    target = r.choice((1, 2, 3, 4, 5, 5, 6, 6, 7, 7, 8, 8))
    boxes = [root]
    for _ in range(48):
        if len(boxes) >= target:
            break
        i = r.randrange(len(boxes))
        b = boxes[i]
        # a box already at a pool width keeps it: cut it along y or z
        axis = r.choices((0, 1, 2), weights=(6, 1, 1) if b[1] - b[0] > max(WIDTHS) else (0, 1, 1))[0]
        lo, hi = b[2 * axis], b[2 * axis + 1]
        if axis == 0 and len(boxes) + 2 <= target and r.random() < 0.75:
            pieces = _slab(r, b)
            if pieces:
                boxes[i:i + 1] = pieces
                continue
        c = _x_cut(r, lo, hi) if axis == 0 else (r.randint(lo + 1, hi - 1) if hi - lo >= 2
                                                 else None)
        if c is None:
            continue
        left, right = list(b), list(b)
        left[2 * axis + 1] = right[2 * axis] = c
        boxes[i:i + 1] = [tuple(left), tuple(right)]
    kept = [b for b in boxes if r.random() < 0.75]
    return kept or [r.choice(boxes)]


def _samples(r, boxes):
    """Cells of the fast7 sample: every box's eight corners, then random cells
    inside boxes, at most MAX_SAMPLES."""
    cells = []
    for x0, x1, y0, y1, z0, z1 in boxes:
        for z in (z0, z1 - 1):
            for y in (y0, y1 - 1):
                for x in (x0, x1 - 1):
                    if (z, y, x) not in cells:
                        cells.append((z, y, x))
    cells = cells[:MAX_SAMPLES]
    for _ in range(MAX_SAMPLES - len(cells)):
        x0, x1, y0, y1, z0, z1 = r.choice(boxes)
        c = (r.randrange(z0, z1), r.randrange(y0, y1), r.randrange(x0, x1))
        if c not in cells:
            cells.append(c)
    return cells


def kernel_case(seed):
    r = random.Random(seed)
    rng = np.random.default_rng(seed)
    K = r.choice((1, 2))
    fast = r.random() < 0.5
    uniform = r.random() < 0.5
    nx = r.choice(NX_SMALL) if r.random() < 0.2 else r.choice(NX_SEAM)
    if nx % 2 and r.random() < 0.35:  # an odd nx always runs one cell per lane: lean to even
        nx = r.choice(NX_SMALL) if r.random() < 0.2 else r.choice(NX_SEAM)
    ny = _extent(r)
    nz = max(3, min(_extent(r), MAX_CELLS // (nx * ny)))
    aligned = r.random() < 0.7
    shape = (nz, ny, nx)

    value = r.uniform(0.5, 2.0)
    iCp = np.full(shape, value) if uniform else rng.uniform(0.5, 2.0, shape)
    lam = 10.0 ** r.uniform(-2, 2)
    dx, dy, dz = (10.0 ** r.uniform(-3, 1) for _ in range(3))
    limit = 1.0 / (2.0 * lam * float(iCp.max()) * (1 / dx**2 + 1 / dy**2 + 1 / dz**2))
    dt = r.uniform(0.2, 1.0) * limit
    coef = (-lam, 1.0 / dx, 1.0 / dy, 1.0 / dz, dt)

    scale = 10.0 ** r.uniform(-6, 6)
    off = r.choice((0.0, scale, -3.0 * scale))
    T = off + scale * rng.uniform(-1.0, 1.0, shape)
    stamps = []
    for _ in range(r.randint(2, 5)):  # equal neighbours and signed zeros, faces included
        lo = [r.randrange(n) for n in shape]
        hi = [min(n, a + r.randint(1, 6)) for n, a in zip(shape, lo)]
        v = r.choice((off + scale * r.uniform(-1.0, 1.0), 0.0, -0.0))
        T[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = v
        stamps.append((tuple(lo), tuple(hi), v))

    boxes = _boxes(r, K, nx, ny, nz)
    u = r.random()
    xface = next((r.choice(pool) for p, pool in XFACE_DRAW[K] if u < p), r.randint(1, 32))
    w = r.choice([b[1] - b[0] for b in boxes])
    if xface and w <= ops.XFACE_MAX and r.random() < 0.15:
        xface = w  # the limit right on a box's width
    rows, unroll = r.choice(ops.TUNINGS_3D)
    tuning = dict(rows=rows, unroll=unroll, tb_rows=r.choice((0,) + tuple(ops.TB_ROWS_3D)),
                  vec=2 if r.random() < 0.9 else 1, nontemporal=r.randint(0, 3),
                  tb_nontemporal=r.randint(0, 3), chunk_z=r.choice(CHUNKS),
                  tb_chunk_z=r.choice(CHUNKS), xcd_remap=r.randint(0, 1))
    tuning["xface"] = xface
    return dict(seed=seed, K=K, fast=fast, uniform=uniform, value=value, shape=shape,
                aligned=aligned, coef=coef, scale=scale, off=off, stamps=stamps, boxes=boxes,
                tuning=tuning, samples=_samples(r, boxes), T=T, iCp=iCp)


def describe(c):
    """The case without its arrays, for a failure message."""
    return {k: v for k, v in c.items() if k not in ("T", "iCp")}


def tuning_of(c, **over):
    """The case's launch tuning. The uniform variant gets its value as an argument."""
    kw = dict(c["tuning"], fast_math=c["fast"], uniform=c["uniform"],
              uniform_value=c["value"] if c["uniform"] else None)
    kw.update(over)
    return ops.Stencil3DTuning(**kw)


def inside_mask(c):
    m = np.zeros(c["shape"], dtype=bool)
    for x0, x1, y0, y1, z0, z1 in c["boxes"]:
        assert not m[z0:z1, y0:y1, x0:x1].any(), "boxes overlap"
        m[z0:z1, y0:y1, x0:x1] = True
    return m


def crop(c, full):
    """``full`` on the boxes, the sentinel everywhere else."""
    want = np.full(c["shape"], SENTINEL)
    m = inside_mask(c)
    want[m] = full[m]
    return want


def canonical_reference(c):
    """K applications of golden3d.step3 on the whole field (the faces keep T),
    cropped to the boxes."""
    a = c["T"]
    for _ in range(c["K"]):
        a = golden3d.step3(a, c["iCp"], *c["coef"])
    return crop(c, a)


def fast7_sample_reference(c):
    """[(cell, value)]: golden3d_fast.cell7 on the sampled cells; for K = 2 the
    seven level-1 inputs of a cell are themselves cell7 of T, a face cell keeps T."""
    T, iCp = c["T"], c["iCp"]
    nz, ny, nx = c["shape"]
    k = golden3d_fast.fast7_constants(*c["coef"])

    def level1(z, y, x):
        if min(z, y, x) == 0 or z == nz - 1 or y == ny - 1 or x == nx - 1:
            return float(T[z, y, x])
        return golden3d_fast.cell7(T, iCp, z, y, x, *k)

    out = []
    for z, y, x in c["samples"]:
        if c["K"] == 1:
            out.append(((z, y, x), golden3d_fast.cell7(T, iCp, z, y, x, *k)))
            continue
        L = np.zeros((3, 3, 3))
        for dz, dy, dx in ((0, 0, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0),
                           (-1, 0, 0)):
            L[1 + dz, 1 + dy, 1 + dx] = level1(z + dz, y + dy, x + dx)
        out.append(((z, y, x), golden3d_fast.cell7(L, np.full((3, 3, 3), iCp[z, y, x]),
                                                   1, 1, 1, *k)))
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def twin(c):
    """The package's CPU twin of the case's arithmetic on CPU tensors, from a
    sentinel T2 (the twins always read the 1/Cp array)."""
    import torch

    T2 = torch.full(c["shape"], SENTINEL, dtype=torch.float64)
    ops.stencil3dk_step(c["K"], T2, torch.from_numpy(c["T"]), torch.from_numpy(c["iCp"]),
                        ops.StencilCoef3(*c["coef"]), c["boxes"],
                        tuning=ops.Stencil3DTuning(fast_math=c["fast"]))
    return T2.numpy()


def march_strips(K, V, x0, x1):
    """Strips the launchers give a march box (plan_boxes in
    csrc/kernels/stencil3d_device.h); for the coverage counts only."""
    if K == 1:
        sw = 64 * V
        return -(-(x1 - (x0 - x0 % sw)) // sw)
    step = 64 * V - 2 * (K - 1)
    xs = max(x0 - (K - 1), 0)
    xa = xs - xs % V
    first = 0 if xa == 0 else xa + K - 1
    return max(1, -(-(x1 - first) // step))


# ---------------------------------------------------------------------------
# model fuzz: Diffusion3D on P <= 8 loopback rank threads
# ---------------------------------------------------------------------------
MODEL_DIMS = ((1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (3, 1, 1), (1, 3, 1), (2, 1, 2),
              (2, 2, 1), (1, 2, 2), (2, 2, 2))
MODEL_SEED, ICP_SEED = 1234, 4321
N_MODEL_CPU, N_MODEL_GPU = 24, 16


def model_case(seed):
    r = random.Random(seed)
    dims = r.choice(MODEL_DIMS)
    periods = tuple(int(r.random() < 0.3) for _ in range(3))
    variant = r.choice(("perf", "perf_hide", "perf_hide", "ap"))
    temporal = 1 if variant == "ap" else r.choice((1, 2))
    fast = variant != "ap" and r.random() < 0.5
    ol = 2 * temporal
    wide = r.random() < 0.25  # nx past 130: more than one strip; the other extents stay small
    n = (2 * ol + (r.randint(127, 140) if wide else r.randint(3, 40)),
         2 * ol + r.randint(3, 14 if wide else 40), 2 * ol + r.randint(3, 14 if wide else 40))
    b_width = (r.randint(1, 20), r.randint(1, 6), r.randint(1, 6))
    u = r.random()
    xface = 0 if u < 0.25 else None if u < 0.5 else r.randint(1, 32)
    native = variant != "ap" and r.random() < 0.5
    # plan(nt) of two-step passes ends on a one-step pass: odd nt >= 3
    nt = r.choice((3, 5, 7, 9)) if temporal == 2 else r.randint(1, 9)
    return dict(seed=seed, dims=dims, periods=periods, variant=variant, temporal=temporal,
                fast=fast, n=n, b_width=b_width, xface=xface, native=native, nt=nt,
                icp=r.choice(("uniform", "random")))


def expect_inner(c, coords):
    """Whether the rank at ``coords`` has an interior box in a perf_hide pass of
    ``temporal`` steps (ops.hide_boxes3d on the neighbours the topology gives it)."""
    K, ol = c["temporal"], 2 * c["temporal"]
    sides, owned = [], []
    for d in range(3):
        lo = bool(c["periods"][d]) or coords[d] > 0
        hi = bool(c["periods"][d]) or coords[d] < c["dims"][d] - 1
        sides.append((lo, hi))
        owned += [K if lo else 1, c["n"][d] - (K if hi else 1)]
    return ops.hide_boxes3d(c["n"], tuple(owned), sides, (ol, ol, ol), c["b_width"])[1] is not None


def model_spmd(rank, hub, c, device):
    from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig

    n = c["n"]
    gpu = device != "cpu"
    m = Diffusion3D(Diffusion3DConfig(variant=c["variant"], nx=n[0], ny=n[1], nz=n[2], nt=c["nt"],
                                      init="random", seed=MODEL_SEED, dims=c["dims"],
                                      periods=c["periods"], quiet=True, temporal=c["temporal"],
                                      fast_math=c["fast"], b_width=c["b_width"],
                                      xface=c["xface"], native=bool(c["native"] and gpu),
                                      device=device),
                    grid_kwargs=dict(loopback=(hub, rank)))
    g = m.g
    assert m.device.type == ("cuda" if gpu else "cpu")
    assert tuple(g.overlaps) == (2 * c["temporal"],) * 3
    assert m.native_loop == bool(c["native"] and gpu)
    if c["variant"] == "perf_hide":
        assert (m.hide_boxes(c["temporal"])[1] is not None) == expect_inner(c, tuple(g.coords))
    if c["icp"] == "random":  # decomposition-invariant, below 1/Cp0 = 1: dt stays stable
        ops.init_random3d_(m.iCp, m.geometry(), seed=ICP_SEED, lo=0.5, hi=1.0)
        assert m.rescan_factor() is False
    plan = m.plan(c["nt"])
    assert sum(plan) == c["nt"] and (c["temporal"] == 1 or set(plan) == {1, 2})
    m.step(c["nt"])
    assert m.steps_done == c["nt"]
    out = (tuple(g.coords), m.field.cpu().numpy().copy(), tuple(g.nxyz_g))
    m.close()
    return out


def _global_index(c, ng, d, coord):
    """Index into the reference array of every local cell of the tile at ``coord``
    along d: on a periodic dimension array cell a holds global cell (a - 1) mod ng."""
    g = coord * (c["n"][d] - 2 * c["temporal"]) + np.arange(c["n"][d])
    return (g - 1) % ng + 1 if c["periods"][d] else g


def model_reference(c, ng):
    """The field of the global grid after nt steps, as an array whose cell a holds
    global cell a (open dimension) or (a - 1) mod ng (periodic). Canonical:
    golden3d.run3 (NumPy); fast7: a one-rank CPU run of the package, whose twin
    test_fuzz3d_cpu.py and test_stencil3d_fast_cpu.py tie to the exact model."""
    per = c["periods"]
    if c["fast"]:
        from helpers import run_loopback

        ol = 2 * c["temporal"]
        one = dict(c, dims=(1, 1, 1), variant="perf", native=False,
                   n=tuple(g + ol * p for g, p in zip(ng, per)))
        return run_loopback(1, model_spmd, one, "cpu", timeout=180)[0][1]
    arr = [g + 2 if p else g for g, p in zip(ng, per)]
    geom = SimpleNamespace(gx0=0, gy0=0, gz0=0, nxg=ng[0], nyg=ng[1], nzg=ng[2],
                           periodx=per[0], periody=per[1], periodz=per[2])
    T0 = golden3d.random_field3_np(*arr, geom, MODEL_SEED)
    iCp = (golden3d.random_field3_np(*arr, geom, ICP_SEED, lo=0.5, hi=1.0)
           if c["icp"] == "random" else None)
    return golden3d.run3(*arr, c["nt"], T0=T0, periods=per, iCp=iCp)


def model_check(seed, device):
    """Every rank's tile == the same window of the global field, bitwise."""
    from helpers import run_loopback

    c = model_case(seed)
    P = c["dims"][0] * c["dims"][1] * c["dims"][2]
    res = run_loopback(P, model_spmd, c, device, timeout=180)
    ng = res[0][2]
    assert list(ng) == [d * (k - 2 * c["temporal"]) + (0 if p else 2 * c["temporal"])
                        for d, k, p in zip(c["dims"], c["n"], c["periods"])], (seed, c)
    ref = model_reference(c, ng)
    assert len(res) == P and len({co for co, _, _ in res}) == P
    for coords, tile, _ in res:
        ix, iy, iz = (_global_index(c, ng[d], d, coords[d]) for d in range(3))
        want = ref[np.ix_(iz, iy, ix)]
        same = bits(tile) == bits(want)
        assert same.all(), (f"seed {seed}: {int((~same).sum())} cells differ on rank {coords}, "
                            f"first (z, y, x) = {tuple(np.argwhere(~same)[0])}; case {c}")
