"""Two-step ``perf_hide`` passes whose frame runs the two-step kernel's x-face
path (``Diffusion3DConfig(temporal=2, xface=None)``) on one MI355X: one rank that
is its own periodic neighbour on six sides, the default boundary width (x slabs
14 wide, 16 lanes per segment) and one whose x slabs land in the 32-lane class,
canonical and fast7, uniform 1/Cp and the field path, the Python-issued loop and
the native one. Bitwise the ``perf`` field and the golden model of the global
grid; the launcher's own dispatch puts both x slabs on the face path and the y
and z slabs on the strip march."""
from types import SimpleNamespace

import numpy as np
import pytest

import golden3d
import golden3d_fast
from helpers import run_loopback
from rocm_mpi_amd import ops
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig
from test_diffusion3d_hide_gpu import perf_run
from test_diffusion3d_tb_cpu import SEED, bits, golden_global

pytestmark = pytest.mark.gpu

K, NT = 2, 8
DIMS, PERIODS = (1, 1, 1), (1, 1, 1)
# (b_width, local size, lanes per segment of the x slabs): the cubes are just
# large enough for an interior box at overlap 4
CASES = {"bw16": ((16, 2, 2), (34, 12, 10), 16), "bw20": ((20, 2, 2), (42, 12, 10), 32)}
_golden: dict = {}


def golden(n, fast):
    """The golden field of the global grid after NT steps, computed once."""
    key = (n, fast)
    if key not in _golden:
        if not fast:
            G, _ = golden_global(DIMS, PERIODS, 2 * K, n=n, nt=NT)
        else:  # golden_global's array and spacing, stepped by the exact fast7 model
            ng = [k - 2 * K for k in n]
            arr = [g + 2 for g in ng]
            geom = SimpleNamespace(gx0=0, gy0=0, gz0=0, nxg=ng[0], nyg=ng[1], nzg=ng[2],
                                   periodx=1, periody=1, periodz=1)
            G = golden3d.random_field3(arr[0], arr[1], arr[2], geom, SEED)
            dx, dy, dz, dt = golden3d.params3(*ng)
            iCp = np.full_like(G, 1.0)
            for _ in range(NT):
                G = golden3d_fast.step7(G, iCp, -1.0, 1.0 / dx, 1.0 / dy, 1.0 / dz, dt)
                for ax in (2, 1, 0):
                    Gm = np.moveaxis(G, ax, 0)
                    Gm[0] = Gm[-2]
                    Gm[-1] = Gm[1]
        _golden[key] = G[1:-1, 1:-1, 1:-1].copy()
    return _golden[key]


def hide_spmd(rank, hub, n, b_width, lanes, fast, uniform, nat):
    m = Diffusion3D(Diffusion3DConfig(variant="perf_hide", nx=n[0], ny=n[1], nz=n[2], nt=NT,
                                      init="random", seed=SEED, dims=DIMS, periods=PERIODS,
                                      quiet=True, temporal=K, fast_math=fast, b_width=b_width,
                                      xface=None, uniform_factor=uniform, native=nat),
                    grid_kwargs=dict(loopback=(hub, rank)))
    assert m.device.type == "cuda" and m.g.halo is not None and m.native_loop == nat
    assert m.uniform_factor == uniform and m.plan(NT) == [K] * (NT // K)
    frame, inner = m.hide_boxes(K)
    assert inner is not None and len(frame) == 6
    assert m.frame_xface(K) == b_width[0]
    if nat:
        assert m._exec.frame_xface == m.frame_xface(K)
    # what the frame launch runs: z and y slabs on the strip march, both x slabs
    # (the last two, b_width - 2 wide) on the face path
    plan = ops.stencil3d_dispatch(K, (n[2], n[1], n[0]), frame,
                                  ops.Stencil3DTuning(xface=m.frame_xface(K)))
    assert [(p, ln) for _, p, ln in plan] == [("march", 64)] * 4 + [("xface", lanes)] * 2
    assert [b[1] - b[0] for b, _, _ in plan[4:]] == [b_width[0] - K] * 2
    m.step(NT)
    Tv = m.gather_interior()
    out = None if Tv is None else Tv.numpy().copy()
    m.close()
    return out


@pytest.mark.parametrize("nat", [False, True], ids=["python", "native"])
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "field"])
@pytest.mark.parametrize("fast", [False, True], ids=["canonical", "fast7"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_two_step_frame_on_the_face_path_equals_perf_and_golden(case, fast, uniform, nat):
    b_width, n, lanes = CASES[case]
    hide = run_loopback(1, hide_spmd, n, b_width, lanes, fast, uniform, nat, timeout=120)[0]
    perf = perf_run(K, n, NT, DIMS, PERIODS, fast_math=fast)
    assert hide.shape == perf.shape
    assert np.array_equal(bits(hide), bits(perf))
    assert np.array_equal(bits(hide), bits(golden(n, fast)))
