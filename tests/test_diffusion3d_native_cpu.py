"""``Diffusion3DConfig(native=True)`` where the native time loop does not apply:
CPU tensors and ``variant="ap"`` keep the Python-issued loop, with the same field,
and the app says which loop runs. The default stays off."""
import pytest
import torch

from rocm_mpi_amd.apps import diffusion_3D_perf as app
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig


def test_native_defaults_to_off():
    assert Diffusion3DConfig().native is False
    assert app.build_parser().parse_args([]).native is False


@pytest.mark.parametrize("variant", ["perf", "perf_hide", "ap"])
def test_cpu_tensors_keep_the_python_loop_and_the_field(variant):
    out = []
    for nat in (False, True):
        m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=20, ny=9, nz=7, nt=5, init="random",
                                          periods=(1, 1, 1), device="cpu", quiet=True,
                                          native=nat))
        assert not m.native_loop and m._exec is None
        m.step(5)
        assert m.rescan_factor() == m.uniform_factor
        out.append(m.field.clone())
        m.close()
    assert torch.equal(out[0].view(torch.int64), out[1].view(torch.int64))


def test_app_prints_the_loop_line_on_cpu(capsys):
    args = ["--nx", "12", "--ny", "9", "--nz", "8", "--nt", "3", "--device", "cpu"]
    assert app.main(args + ["--native"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert [ln for ln in lines if ln.startswith("[loop]")] == [
        "[loop] python (--native does not apply: CPU tensors)"]
    assert app.main(args) == 0
    lines = capsys.readouterr().out.splitlines()
    assert [ln for ln in lines if ln.startswith("[loop] python")]
