"""Placement pass of the IGG-style gather on one GPU (a probe, not a gate).

Times ``ops.assemble_blocks`` (one launch of the strided block-copy kernel,
csrc/kernels/blocks.hip) for 4 rank-major blocks of 4096 x 4096 fp64 placed on
a 2 x 2 process grid, interleaved with the torch slice assignment the Python
``gather_`` performs today (one strided copy per block), and writes both
times and the fraction of the flat-copy roofline (README: 6.32 TB/s) to
``profiles/gather_blocks.md``::

    python bench/gather_probe.py [--out profiles/gather_blocks.md] [--n 4096] [--rounds 20]

Each round times ``--reps`` back-to-back calls of one method between device
events, then the same for the other; the report gives the median, the minimum
and the maximum over the rounds, per call. Bytes moved: every element is read
once and written once. The two results are compared bitwise before timing.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROOFLINE_TBPS = 6.32  # README: same-box flat copy probe (bench/stencil_sweep.py)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_blocks.md"))
    ap.add_argument("--n", type=int, default=4096, help="block edge (cells)")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    a = ap.parse_args(argv)

    import torch

    from rocm_mpi_amd import ops

    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = "cuda:0"
    dims, n = (2, 2, 1), a.n
    g = torch.Generator().manual_seed(11)
    staging = torch.rand((4, n, n), generator=g, dtype=torch.float64).to(dev)
    G_native = torch.empty((2 * n, 2 * n), dtype=torch.float64, device=dev)
    G_torch = torch.empty_like(G_native)
    # rank = c0 * 2 + c1 sits at (x, y) = (c0, c1): the ordering of gather_ (halo.py)
    slices = [(slice(c1 * n, (c1 + 1) * n), slice(c0 * n, (c0 + 1) * n))
              for c0 in range(2) for c1 in range(2)]

    def native():
        ops.assemble_blocks(staging, G_native, dims)

    def by_torch():
        for r, idx in enumerate(slices):
            G_torch[idx] = staging[r]

    native()
    by_torch()
    torch.cuda.synchronize()
    assert torch.equal(G_native, G_torch), "the two placements differ"

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps  # ms per call

    for _ in range(3):  # warm-up of both
        window(native)
        window(by_torch)
    t = {"native": [], "torch": []}
    for _ in range(a.rounds):  # interleaved: both see the same neighbours on the box
        t["native"].append(window(native))
        t["torch"].append(window(by_torch))

    nbytes = 2 * staging.numel() * 8  # one read + one write per element
    rows = []
    for k, label in (("native", "`ops.assemble_blocks` (1 launch)"),
                     ("torch", "torch slice assignment (4 copies)")):
        med, lo, hi = statistics.median(t[k]), min(t[k]), max(t[k])
        tbps = nbytes / (med * 1e-3) / 1e12
        rows.append((label, med, lo, hi, tbps, tbps / ROOFLINE_TBPS))
    ratio = rows[1][1] / rows[0][1]
    lines = [
        "# Placement pass of the C ABI gather (bench/gather_probe.py)",
        "",
        f"{torch.cuda.get_device_name(0)}; 4 blocks of {n} x {n} fp64 (rank-major staging) placed on a "
        f"2 x 2 process grid into a {2 * n} x {2 * n} array; {nbytes / 1e9:.3f} GB moved per call "
        "(every element read once, written once).",
        f"{a.rounds} interleaved rounds of {a.reps} back-to-back calls each, timed with device events; "
        "ms per call. Results compared bitwise before timing.",
        "",
        "| method | median ms | min ms | max ms | TB/s (median) | of the 6.32 TB/s flat-copy roofline |",
        "|---|---|---|---|---|---|",
    ]
    for label, med, lo, hi, tbps, frac in rows:
        lines.append(f"| {label} | {med:.4f} | {lo:.4f} | {hi:.4f} | {tbps:.2f} | {100 * frac:.1f} % |")
    lines += ["", f"torch / native (median): {ratio:.3f}x", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
