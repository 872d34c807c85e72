"""Target of tests/test_gather_procs_gpu.py: one rank of a multi-process
rma_gather_igg, driving ONLY the C ABI through ctypes (what a C or Julia host
does). Every case is a grid of its own: rank 0 makes the RCCL unique id and
writes it atomically into the test's directory, the others poll for the file
(bounded)."""
import ctypes
import os
import time

import numpy as np

I64P = ctypes.POINTER(ctypes.c_int64)

# name -> (dims, root, source, A_global, dtype, block (nx, ny, nz), halo of the source field)
CASES = {
    "host_to_host": ((2, 2, 1), 0, "host", "host", "float64", (10, 7, 1), 0),
    "device_crop_to_host": ((2, 2, 1), 0, "device", "host", "float64", (8, 5, 1), 1),
    "device_to_device_in_place": ((1, 4, 1), 3, "device", "device", "float64", (10, 7, 1), 0),
    "device_to_device_3d_fp32": ((2, 1, 2), 0, "device", "device", "float32", (8, 6, 4), 0),
}


def expected(name):
    """A_global of a case: every cell holds its own global linear index."""
    dims, _, _, _, dtype, (nx, ny, nz), _ = CASES[name]
    shape = (dims[2] * nz, dims[1] * ny, dims[0] * nx)
    return np.arange(int(np.prod(shape))).reshape(shape).astype(dtype)


def _uid(L, rank, path, bound_s=60.0):
    if rank == 0:
        buf = ctypes.create_string_buffer(128)
        assert L.rma_unique_id(buf) == 0, L.rma_last_error().decode()
        with open(path + ".part", "wb") as f:
            f.write(buf.raw)
        os.replace(path + ".part", path)  # atomic: a reader sees all 128 bytes or no file
        return buf.raw
    t0 = time.monotonic()
    while not os.path.exists(path):
        if time.monotonic() - t0 > bound_s:
            raise TimeoutError(f"rank {rank}: no unique id at {path} after {bound_s} s")
        time.sleep(0.005)
    return open(path, "rb").read()


def igg_gather(rank, world, outdir, names):
    from rocm_mpi_amd.parallel import comm as C

    C.shared_gpu_rccl(rank, world)  # before the library's first RCCL call
    import torch

    from helpers import ROOT

    L = ctypes.CDLL(os.path.join(ROOT, "rocm_mpi_amd", "librma_core.so"))
    L.rma_last_error.restype = ctypes.c_char_p
    L.rma_gather_igg.argtypes = [ctypes.c_void_p, ctypes.c_void_p, I64P, I64P, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    for name in names:
        dims, root, src_kind, dst_kind, dtype, (nx, ny, nz), halo = CASES[name]
        uid = _uid(L, rank, os.path.join(outdir, f"uid_{name}.bin"))
        g = ctypes.c_void_p()
        coords = (ctypes.c_int * 3)()
        # the local field of the grid: the block plus the halo that the crop leaves out
        fx, fy, fz = nx + 2 * halo, ny + 2 * halo, nz
        rc = L.rma_init_global_grid(fx, fy, fz, (ctypes.c_int * 3)(*dims), None, None, None, world,
                                    rank, uid, 0, ctypes.byref(g), None, None, coords)
        assert rc == 0, L.rma_last_error().decode()
        c = tuple(coords)
        NXg, NYg = dims[0] * nx, dims[1] * ny
        gz = c[2] * nz + np.arange(nz)[:, None, None]
        gy = c[1] * ny + np.arange(ny)[None, :, None]
        gx = c[0] * nx + np.arange(nx)[None, None, :]
        block = ((gz * NYg + gy) * NXg + gx).astype(dtype)
        field = np.full((fz, fy, fx), -1.0, dtype=dtype)
        field[:, halo:fy - halo, halo:fx - halo] = block
        pitch = (ctypes.c_int64 * 2)(fx, fx * fy) if halo else None
        first = halo * fx + halo  # element offset of the interior's first cell
        eb = field.dtype.itemsize
        if src_kind == "device":
            src = torch.from_numpy(field).to("cuda:0")
            a = src.data_ptr() + first * eb
        else:
            a = field.ctypes.data + first * eb
        out = out_ptr = None
        if rank == root:
            shape = (dims[2] * nz, dims[1] * ny, dims[0] * nx)
            if dst_kind == "device":
                out = torch.full(shape, -1.0, dtype=getattr(torch, dtype), device="cuda:0")
                out_ptr = out.data_ptr()
            else:
                out = np.full(shape, -1.0, dtype=dtype)
                out_ptr = out.ctypes.data
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.rma_gather_igg(g, a, (ctypes.c_int64 * 3)(nx, ny, nz), pitch, eb, out_ptr, root,
                              stream)
        assert rc == 0, L.rma_last_error().decode()
        if rank == root:
            res = out.cpu().numpy() if dst_kind == "device" else out
            np.save(os.path.join(outdir, f"A_global_{name}.npy"), res)
        assert L.rma_finalize_global_grid(g) == 0, L.rma_last_error().decode()
