#!/usr/bin/env python
"""Sweep of the 3D z-march kernel (csrc/kernels/stencil3d.hip) on one GPU.

For every cube size the tunings (rows x unroll x vec x chunk_z), the same-box
roofline probes (stream_triad: 2 reads + 1 write, the stencil's mix; stream_copy)
and nothing else run in interleaved rounds on alternating buffers; the report
is the median over the rounds. T_eff = 3 * nx*ny*nz * 8 B / t. ``--ap N`` also
times Diffusion3D's ``perf`` and ``ap`` variants at N^3 (the kernel against the
torch expressions a user had before). ``--one`` runs a few launches of the
default tuning and of the probes only (for a counter-collection run).

``--temporal 2`` instead times one 2-step pass (csrc/kernels/stencil3d_tb.hip,
every tb_rows x tb_chunk_z) against two launches of the one-step kernel at its
shipped tuning, in the same interleaved rounds (profiles/diffusion3d_temporal.md).

``--uniform`` also times the uniform-1/Cp variant of every tuning (16 B per cell:
the factor is a kernel argument, the array is not read), each right after its
field-path twin in the same rounds, and reports ``vs_field`` = field median /
uniform median (profiles/diffusion3d_uniform.md); with ``--temporal 2`` the same
for the two-step pass. ``spread`` = (max - min) / median over the rounds.

``--fast-math`` times the shipped tuning only (one-step, or with ``--temporal 2``
the two-step pass next to two one-step launches), each canonical kernel followed
by its fast7 twin (``Stencil3DTuning.fast_math``; names ending in ``_f7``) in the
same rounds, and reports ``vs_canonical`` = canonical median / fast7 median
(profiles/diffusion3d_fastmath.md); with ``--uniform`` the same for the
uniform-1/Cp variants.

``--xface W[,W...]`` instead times a pair of x-face boxes of width W (at x0 = 1
and at x1 = n-1, the x slabs of a frame) through three dispatches in the same
interleaved rounds: today's (thin-box path up to width 8, else the strip march),
the x-face path (``Stencil3DTuning.xface``) and, as a reference point, the same
number of cells as a pair of z slabs. ``vs_today`` = today's median / the
variant's median. It combines with ``--uniform`` and ``--fast-math``. With
``--temporal 2`` the pair (at x0 = 2 and x1 = n-2, the x slabs of a two-step frame)
runs through the two-step kernel's two paths instead: the strip march (today's
dispatch) and its x-face path at rows per group 2 and 4 and every
``--face-chunk-z`` planes per task (``xface-rR-czC``); GB/s counts one pass.

``--hide`` instead times ``Diffusion3D`` steps with one rank: ``perf`` with periods
(0,0,0) (no exchange: the floor), ``perf`` with periods (1,1,1) (the rank is its own
neighbour on all six sides) and ``perf_hide`` with periods (1,1,1), with the x-face
path off and on (one- and two-step frames alike), every model rebuilt in every round
so the rounds interleave. ``--hide --fused`` adds ``perf_hide`` with frame-first
single-launch passes (``Diffusion3DConfig.fused``) as a fifth column and reports
``vs_split`` / ``vs_split_xface`` = the split column's median / the fused median
(profiles/diffusion3d_fused.md).
``recovered`` = (perf periodic - perf_hide) / (perf periodic - perf open). It
combines with ``--temporal 2``, ``--uniform`` (1/Cp one value: the model's scan
finds it; without the flag the scan is disabled) and ``--fast-math``
(profiles/diffusion3d_hide.md).

``--native`` instead times ``Diffusion3D`` steps issued pass by pass from Python
against the native time loop (``Diffusion3DConfig(native=True)``,
csrc/runtime/executor3d.cpp) of the same build: ``perf`` and ``perf_hide``, one rank
that is its own periodic neighbour on six sides, uniform 1/Cp, ``--iters`` passes of
``--temporal`` steps per timing, every model rebuilt in every round. ``median_ms`` is
GPU time per step, ``enqueue_ms`` host time per step until ``step`` returns;
``vs_python`` = Python median / native median (profiles/diffusion3d_native.md).

    python bench/stencil3d_sweep.py --sizes 512,1024,1536 --ap 1024 --out sweep3d.json
    python bench/stencil3d_sweep.py --sizes 128,256 --native --iters 200 --rounds 7
    python bench/stencil3d_sweep.py --sizes 256,512,1024 --xface 2,8,16 --out sweep3d_xface.json
    python bench/stencil3d_sweep.py --sizes 256,512,1024 --hide --out sweep3d_hide.json
    python bench/stencil3d_sweep.py --sizes 256,512,1024 --xface 2,6,14,30 --temporal 2 --uniform --fast-math
    python bench/stencil3d_sweep.py --sizes 256,512,1024 --hide --temporal 2 --uniform
    python bench/stencil3d_sweep.py --temporal 2 --out sweep3d_tb.json
    python bench/stencil3d_sweep.py --uniform --out sweep3d_uni.json
    python bench/stencil3d_sweep.py --fast-math --uniform --temporal 2 --out sweep3d_f7.json
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rocm_mpi_amd import ops  # noqa: E402
from rocm_mpi_amd._native import native  # noqa: E402


def sweep_size(n: int, a) -> dict:
    nat = native()
    dev = torch.device("cuda")
    s = torch.cuda.current_stream().cuda_stream
    bufs = [torch.empty((n, n, n), dtype=torch.float64, device=dev) for _ in range(2)]
    iCp = torch.empty((n, n, n), dtype=torch.float64, device=dev)
    geom = ops.TileGeometry3(0, 0, 0, n, n, n, 10.0 / n, 10.0 / n, 10.0 / n)
    ops.init_random3d_(bufs[0], geom, seed=1)
    bufs[1].copy_(bufs[0])
    ops.init_random3d_(iCp, geom, seed=2, lo=0.5, hi=2.0)
    d = 10.0 / n
    coef = ops.StencilCoef3.from_physics(1.0, d, d, d, d * d / 6.1)
    cells = float(n) ** 3
    flip = [0]

    def pair():
        flip[0] ^= 1
        return bufs[flip[0]], bufs[flip[0] ^ 1]

    variants = {}
    steps = {}  # time steps one call of a variant advances (default 1)

    def add(name, fn, tn, nbytes, nsteps=1):
        """The variant and, with --fast-math, its fast7 twin right after it."""
        arith = [("", tn)]
        if a.fast_math:
            arith.append(("_f7", dataclasses.replace(tn, fast_math=True)))
        for suffix, t in arith:
            variants[name + suffix] = ((lambda t=t: fn(t)), nbytes)
            steps[name + suffix] = nsteps

    if a.temporal > 1:
        K = a.temporal
        tunings = []

        def onestep_k(tn):  # K launches of the one-step kernel at its shipped tuning
            for _ in range(K):
                dst, src = pair()
                ops.stencil3d_step(dst, src, iCp, coef, tuning=tn)

        add("onestep_x%d" % K, onestep_k, ops.Stencil3DTuning(), 24.0 * cells * K, K)
        if a.fast_math:
            tbs = [ops.Stencil3DTuning()]
        else:
            tbs = [ops.Stencil3DTuning(tb_rows=r, tb_chunk_z=cz) for r in ops.TB_ROWS_3D
                   for cz in a.tb_chunk_z]
            tbs += [ops.Stencil3DTuning(tb_nontemporal=m) for m in (1, 2, 3)]
            tbs += [ops.Stencil3DTuning(xcd_remap=0)]

        def run_tb(tn):
            dst, src = pair()
            ops.stencil3dk_step(K, dst, src, iCp, coef, tuning=tn)

        for tn in tbs:
            name = (f"tb{K}_r{tn.tb_rows}_cz{tn.tb_chunk_z}_nt{tn.tb_nontemporal}"
                    f"_x{tn.xcd_remap}")
            add(name, run_tb, tn, 24.0 * cells, K)
            if a.uniform:
                add(name + "_uni", run_tb, dataclasses.replace(tn, uniform=True, uniform_value=1.0),
                    16.0 * cells, K)
    elif a.one or a.fast_math:
        tunings = [ops.Stencil3DTuning()]
    else:
        tunings = [ops.Stencil3DTuning(rows=r, unroll=u, vec=v, chunk_z=cz)
                   for r, u in ops.TUNINGS_3D for v in (2, 1) for cz in a.chunk_z
                   if v == 2 or (r, u, cz) == (4, 2, 0)]
        tunings += [ops.Stencil3DTuning(nontemporal=0), ops.Stencil3DTuning(xcd_remap=0)]
    for tn in tunings:
        name = (f"march_r{tn.rows}_u{tn.unroll}_v{tn.vec}_cz{tn.chunk_z}_nt{tn.nontemporal}"
                f"_x{tn.xcd_remap}")

        def run(tn):
            dst, src = pair()
            ops.stencil3d_step(dst, src, iCp, coef, tuning=tn)

        add(name, run, tn, 24.0 * cells)
        if a.uniform:
            add(name + "_uni", run, dataclasses.replace(tn, uniform=True, uniform_value=1.0),
                16.0 * cells)

    def triad():
        dst, src = pair()
        nat.stream_triad(dst.data_ptr(), src.data_ptr(), iCp.data_ptr(), 0.5, int(cells), s, 1, 0)

    def copy():
        dst, src = pair()
        nat.stream_copy(dst.data_ptr(), src.data_ptr(), int(cells), s, 1, 0)

    variants["roof_triad"] = (triad, 24.0 * cells)
    variants["roof_copy"] = (copy, 16.0 * cells)
    times = {k: [] for k in variants}
    for fn, _ in variants.values():  # warm every shape and code object
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for k, (fn, _) in variants.items():
            ev0.record()
            for _ in range(a.iters):
                fn()
            ev1.record()
            ev1.synchronize()
            times[k].append(ev0.elapsed_time(ev1) / a.iters)
    res = {}
    for k, (_, b) in variants.items():
        med = statistics.median(times[k])
        nst = steps.get(k, 1)
        res[k] = {"median_ms": med, "min_ms": min(times[k]), "max_ms": max(times[k]),
                  "GBps": b / med / 1e6, "T_eff_GBps": 24.0 * cells * nst / med / 1e6,
                  "spread": (max(times[k]) - min(times[k])) / med}
        if a.temporal > 1:
            res[k]["ms_per_step"] = med / nst
    tri, cp = res["roof_triad"]["median_ms"], res["roof_copy"]["GBps"]
    for k, r in res.items():
        if k.startswith("march"):
            r["vs_triad"] = tri / r["median_ms"]
            r["vs_copy_rate"] = r["GBps"] / cp
        if k.startswith("tb"):  # > 1: the K-step pass is ahead of K one-step launches
            one = "onestep_x%d" % a.temporal + ("_f7" if k.endswith("_f7") else "")  # same arithmetic
            r["vs_onestep"] = res[one]["median_ms"] / r["median_ms"]
            r["vs_triad"] = tri / r["median_ms"]  # the ceiling of a 24 B pass is 1
        base = k[:-3] if k.endswith("_f7") else k
        if base.endswith("_uni"):  # > 1: the uniform variant is ahead; the traffic model allows 1.5
            r["vs_field"] = res[base[:-4] + k[len(base):]]["median_ms"] / r["median_ms"]
        if k.endswith("_f7"):  # > 1: fast7 is ahead of the canonical kernel of the same rounds
            r["vs_canonical"] = res[base]["median_ms"] / r["median_ms"]
    del bufs, iCp
    torch.cuda.empty_cache()
    return res


def _summary(times: dict) -> dict:
    out = {}
    for k, t in times.items():
        med = statistics.median(t)
        out[k] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t),
                  "spread": (max(t) - min(t)) / med}
    return out


def sweep_xface(n: int, a) -> dict:
    """A pair of x-face boxes of every width through today's dispatch, the x-face
    path and as z slabs of the same cell count."""
    dev = torch.device("cuda")
    bufs = [torch.empty((n, n, n), dtype=torch.float64, device=dev) for _ in range(2)]
    iCp = torch.empty((n, n, n), dtype=torch.float64, device=dev)
    geom = ops.TileGeometry3(0, 0, 0, n, n, n, 10.0 / n, 10.0 / n, 10.0 / n)
    ops.init_random3d_(bufs[0], geom, seed=1)
    bufs[1].copy_(bufs[0])
    ops.init_random3d_(iCp, geom, seed=2, lo=0.5, hi=2.0)
    d = 10.0 / n
    coef = ops.StencilCoef3.from_physics(1.0, d, d, d, d * d / 6.1)
    flip = [0]
    variants, cells = {}, {}
    kinds = [("", ops.Stencil3DTuning())]
    if a.uniform:
        kinds.append(("_uni", ops.Stencil3DTuning(uniform=True, uniform_value=1.0)))
    if a.fast_math:
        kinds += [(s + "_f7", dataclasses.replace(t, fast_math=True)) for s, t in list(kinds)]
    K = a.temporal
    today = {}  # variant -> today's dispatch of the same boxes, arithmetic and 1/Cp path
    for w in a.xface:
        # one-step: the slabs start at the first interior cell; a K-step pass owns
        # [K, n-K) next to a neighbour (width-K halos)
        xb = [(K, K + w, K, n - K, K, n - K), (n - K - w, n - K, K, n - K, K, n - K)]
        zb = [(K, n - K, K, n - K, K, K + w), (K, n - K, K, n - K, n - K - w, n - K)]
        for suffix, tn in kinds:
            cases = [("today", xb, tn)]
            if K == 1:
                cases.append(("xface", xb, dataclasses.replace(tn, xface=w)))
            else:  # the two-step face path at every rows x planes-per-task
                cases += [(f"xface-r{r}-cz{cz}", xb,
                           dataclasses.replace(tn, xface=w, tb_rows=r, tb_chunk_z=cz))
                          for r in ops.TB_ROWS_3D for cz in a.face_chunk_z]
            cases.append(("zslab", zb, tn))
            for name, boxes, t in cases:
                def run(boxes=boxes, t=t):
                    flip[0] ^= 1
                    if K == 1:
                        ops.stencil3d_step(bufs[flip[0]], bufs[flip[0] ^ 1], iCp, coef, boxes, t)
                    else:
                        ops.stencil3dk_step(K, bufs[flip[0]], bufs[flip[0] ^ 1], iCp, coef, boxes,
                                            t)

                key = f"{name}_w{w}{suffix}"
                variants[key] = run
                today[key] = f"today_w{w}{suffix}"
                cells[key] = 2.0 * w * (n - 2 * K) * (n - 2 * K)
    times = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ev0.record()
            for _ in range(a.iters):
                fn()
            ev1.record()
            ev1.synchronize()
            times[k].append(ev0.elapsed_time(ev1) / a.iters)
    res = _summary(times)
    for k, r in res.items():
        per = 16.0 if "_uni" in k else 24.0
        r["GBps"] = per * cells[k] / r["median_ms"] / 1e6
        r["vs_today"] = res[today[k]]["median_ms"] / r["median_ms"]
    del bufs, iCp
    torch.cuda.empty_cache()
    return res


def sweep_hide(n: int, a) -> dict:
    """ms per step of perf (open), perf (periodic) and perf_hide (periodic, x-face
    path off and on) at n^3 with one rank, the models rebuilt in every round."""
    from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig

    cases = {"perf_open": ("perf", (0, 0, 0), 0), "perf_periodic": ("perf", (1, 1, 1), 0),
             "hide_periodic": ("perf_hide", (1, 1, 1), 0),
             "hide_periodic_xface": ("perf_hide", (1, 1, 1), None)}
    if a.fused:
        cases["hide_periodic_fused"] = ("perf_hide", (1, 1, 1), 0)
    steps = a.iters * a.temporal
    times = {k: [] for k in cases}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(a.rounds + 1):  # round 0 warms every shape and code object
        for k, (variant, periods, xface) in cases.items():
            m = Diffusion3D(Diffusion3DConfig(
                variant=variant, nx=n, ny=n, nz=n, nt=steps, init="random", periods=periods,
                quiet=True, temporal=a.temporal, fast_math=a.fast_math,
                uniform_factor=a.uniform, b_width=a.b_width, xface=xface,
                fused=k.endswith("_fused")))
            m.step(2 * a.temporal)
            m.synchronize()
            ev0.record()
            m.step(steps)
            ev1.record()
            ev1.synchronize()
            if rnd:
                times[k].append(ev0.elapsed_time(ev1) / steps)
            m.synchronize()  # raises if a fused pass's wait timed out
            m.close()
            del m
    torch.cuda.empty_cache()
    res = _summary(times)
    exposed = res["perf_periodic"]["median_ms"] - res["perf_open"]["median_ms"]
    for k in [c for c in cases if c.startswith("hide_")]:
        gain = res["perf_periodic"]["median_ms"] - res[k]["median_ms"]
        res[k]["gain_ms"] = gain
        res[k]["recovered"] = gain / exposed if exposed > 0 else float("nan")
    res["perf_periodic"]["exposed_ms"] = exposed
    if a.fused:
        f = res["hide_periodic_fused"]
        f["vs_split"] = res["hide_periodic"]["median_ms"] / f["median_ms"]
        f["vs_split_xface"] = res["hide_periodic_xface"]["median_ms"] / f["median_ms"]
    return res


def sweep_native(n: int, a) -> dict:
    """ms per step of the Python-issued loop and of the native loop
    (Diffusion3DConfig.native) at n^3: perf and perf_hide, one rank that is its own
    periodic neighbour on six sides, uniform 1/Cp, the models rebuilt in every round.
    ``median_ms``: GPU time per step between two events around step(n) (what a
    run delivers); ``enqueue_ms``: host time per step until step(n) returns,
    nothing synchronised (what the loop costs the host)."""
    import time

    from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig

    cases = {f"{v}_{loop}": (v, loop == "native") for v in ("perf", "perf_hide")
             for loop in ("python", "native")}
    steps = a.iters * a.temporal
    times = {k: [] for k in cases}
    host = {k: [] for k in cases}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(a.rounds + 1):  # round 0 warms every shape and code object
        for k, (variant, nat) in cases.items():
            m = Diffusion3D(Diffusion3DConfig(
                variant=variant, nx=n, ny=n, nz=n, nt=steps, init="random", periods=(1, 1, 1),
                quiet=True, temporal=a.temporal, fast_math=a.fast_math, uniform_factor=True,
                b_width=a.b_width, native=nat))
            assert m.native_loop == nat and m.uniform_factor
            m.step(2 * a.temporal)
            m.synchronize()
            ev0.record()
            t0 = time.perf_counter()
            m.step(steps)
            t1 = time.perf_counter()
            ev1.record()
            ev1.synchronize()
            if rnd:
                times[k].append(ev0.elapsed_time(ev1) / steps)
                host[k].append((t1 - t0) * 1e3 / steps)
            m.close()
            del m
    torch.cuda.empty_cache()
    res = _summary(times)
    for k, r in res.items():
        r["enqueue_ms"] = statistics.median(host[k])
        r["enqueue_spread"] = (max(host[k]) - min(host[k])) / r["enqueue_ms"]
    for v in ("perf", "perf_hide"):  # > 1: the native loop is ahead
        py, nat = res[v + "_python"], res[v + "_native"]
        nat["vs_python"] = py["median_ms"] / nat["median_ms"]
        nat["enqueue_vs_python"] = py["enqueue_ms"] / nat["enqueue_ms"]
    return res


def model_compare(n: int, steps: int) -> dict:
    """Seconds per step of Diffusion3D perf (the kernel) and ap (torch) at n^3."""
    from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig

    out = {}
    for variant in ("perf", "ap", "perf", "ap"):  # alternating: two timings each
        m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=n, ny=n, nz=n, nt=steps + 2,
                                          init="random", quiet=True))
        res = m.run(steps + 2, warmup=2)
        out.setdefault(variant, []).append(res.t_it * 1e3)
        m.close()
        del m
        torch.cuda.empty_cache()
    return {"n": n, "steps": steps, "perf_ms_per_step": out["perf"], "ap_ms_per_step": out["ap"],
            "speedup": min(out["ap"]) / max(out["perf"])}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="512,1024,1536")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--chunk-z", dest="chunk_z", default="0,32,128",
                    type=lambda v: [int(x) for x in v.split(",")])
    ap.add_argument("--temporal", type=int, default=1, choices=[1, 2],
                    help="2: the 2-step pass against two one-step launches")
    ap.add_argument("--tb-chunk-z", dest="tb_chunk_z", default="0,16,64",
                    type=lambda v: [int(x) for x in v.split(",")])
    ap.add_argument("--face-chunk-z", dest="face_chunk_z", default="16,32",
                    type=lambda v: [int(x) for x in v.split(",")],
                    help="--xface --temporal 2: planes per task of the two-step face path")
    ap.add_argument("--ap", type=int, default=0, help="cube size of the perf-versus-ap timing")
    ap.add_argument("--ap-steps", type=int, default=5)
    ap.add_argument("--one", action="store_true", help="default tuning and probes only")
    ap.add_argument("--uniform", action="store_true",
                    help="also the uniform-1/Cp variant of every tuning (vs_field)")
    ap.add_argument("--fast-math", dest="fast_math", action="store_true",
                    help="the shipped tuning only, each kernel next to its fast7 twin "
                         "(vs_canonical)")
    ap.add_argument("--xface", default=[], type=lambda v: [int(x) for x in v.split(",") if x],
                    help="widths of an x-face box pair: today's dispatch, the x-face path, z slabs")
    ap.add_argument("--hide", action="store_true",
                    help="Diffusion3D perf (open, periodic) against perf_hide (periodic)")
    ap.add_argument("--fused", action="store_true",
                    help="--hide: also perf_hide with frame-first single-launch passes")
    ap.add_argument("--native", action="store_true",
                    help="Diffusion3D's Python-issued loop against the native loop (perf, "
                         "perf_hide; periodic, uniform 1/Cp): ms per step and host enqueue time")
    ap.add_argument("--b-width", dest="b_width", default=(16, 2, 2),
                    type=lambda v: tuple(int(x) for x in v.split(",")))
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stencil3d_sweep needs a GPU")
    report = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters,
              "sizes": {}}
    for n in [int(v) for v in a.sizes.split(",") if v]:
        if a.xface or a.hide or a.native:
            r = report["sizes"][str(n)] = (sweep_xface(n, a) if a.xface else
                                           sweep_native(n, a) if a.native else sweep_hide(n, a))
            for k, v in r.items():
                print(f"{n:5d}^3 {k:28s} {v['median_ms']:9.4f} ms  spread {v['spread']:.3f}"
                      + (f"  {v['GBps']:8.1f} GB/s  {v['vs_today']:.3f} x today"
                         if "vs_today" in v else "")
                      + (f"  exposed exchange {v['exposed_ms']:.4f} ms" if "exposed_ms" in v else "")
                      + (f"  gain {v['gain_ms']:.4f} ms, recovered {v['recovered']:.2f}"
                         if "recovered" in v else "")
                      + (f"  {v['vs_split']:.3f} x split, {v['vs_split_xface']:.3f} x split+xface"
                         if "vs_split" in v else "")
                      + (f"  enqueue {v['enqueue_ms']:.4f} ms/step (spread "
                         f"{v['enqueue_spread']:.3f})" if "enqueue_ms" in v else "")
                      + (f"  {v['vs_python']:.3f} x python (enqueue "
                         f"{v['enqueue_vs_python']:.2f} x)" if "vs_python" in v else ""),
                      flush=True)
            continue
        report["sizes"][str(n)] = sweep_size(n, a)
        best = sorted((r["median_ms"], k) for k, r in report["sizes"][str(n)].items())
        for ms, k in best:
            r = report["sizes"][str(n)][k]
            print(f"{n:5d}^3 {k:40s} {ms:9.3f} ms  {r['GBps']:8.1f} GB/s"
                  + (f"  {r['vs_triad']:.3f} of triad" if "vs_triad" in r else "")
                  + (f"  {r['vs_onestep']:.3f} x one-step" if "vs_onestep" in r else "")
                  + (f"  {r['vs_field']:.3f} x field" if "vs_field" in r else "")
                  + (f"  {r['vs_canonical']:.3f} x canonical" if "vs_canonical" in r else "")
                  + f"  spread {r['spread']:.3f}",
                  flush=True)
    if a.ap:
        report["perf_vs_ap"] = model_compare(a.ap, a.ap_steps)
        print("perf_vs_ap", json.dumps(report["perf_vs_ap"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    print(json.dumps({"ok": True, "sizes": list(report["sizes"])}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
