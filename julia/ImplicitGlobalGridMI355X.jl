# ImplicitGlobalGrid-compatible Julia front end over librma_core.so (C ABI,
# csrc/include/rma/capi.h). Keeps the call sites of the reference scripts
# (scripts/diffusion_2D_*.jl) source compatible:
#
#     using ImplicitGlobalGridMI355X
#     me, dims, nprocs, coords, comm = init_global_grid(nx, ny, 1)
#     update_halo!(T); nx_g(); x_g(ix, dx, T); tic(); toc(); finalize_global_grid()
#
# Device arrays are anything with a device pointer (AMDGPU.ROCArray); the halo
# exchange runs GPU-direct over RCCL. The RCCL unique id is broadcast with
# MPI.jl when it is loaded (the reference already uses MPI.jl), otherwise
# world size must be 1. NOTE: Julia is not installed in this repository's CI;
# this shim is untested here (the C ABI itself is exercised by
# examples/diffusion_2D_perf_hide.cpp and tests/test_capi_gpu.py).
#
# The native time loop is exposed too: `ex = DiffusionExecutor(T, T2, iCp,
# coef; mode=1, steps_per_pass=8)`, `run!(ex, n)` — K steps per kernel pass
# need init_global_grid(...; overlaps=(2K,2K,2), halowidths=(K,K,1)).
#
# 3D heat diffusion (diffusion3D, ImplicitGlobalGrid's flagship example):
#
#     init_global_grid(nx, ny, nz; periodx=1, periody=1, periodz=1)
#     init_gaussian3d!(T, dx, dy, dz, lx, ly, lz); T2 = copy(T)
#     ex = Diffusion3DExecutor(T, T2, iCp, (-lam, 1/dx, 1/dy, 1/dz, dt); mode=1,
#                              b_width=(16, 2, 2))
#     run!(ex, nt); T = current_field(ex)
#
# steps_per_pass=2 needs overlaps=(4,4,4), halowidths=(2,2,2). Single kernel
# calls: diffusion3d_step!(T2, T, iCp, coef), diffusion3d_boxes!(T2, T, iCp, coef,
# boxes; steps=K). After writing to iCp call rescan_factor!(ex).
module ImplicitGlobalGridMI355X

using Libdl

export init_global_grid, finalize_global_grid, update_halo!, gather!, gather_rankmajor!, nx_g, ny_g, nz_g,
       x_g, y_g, z_g, tic, toc, DiffusionExecutor, run!, current_field, check_executor,
       Diffusion3DExecutor, diffusion3d_step!, diffusion3d_boxes!, init_gaussian3d!,
       init_random3d!, uniform_factor, rescan_factor!

const LIB = Ref{Ptr{Cvoid}}(C_NULL)
const GRID = Ref{Ptr{Cvoid}}(C_NULL)
const NXYZ = Ref((1, 1, 1))

libpath() = get(ENV, "RMA_CORE_LIB", joinpath(@__DIR__, "..", "rocm_mpi_amd", "librma_core.so"))

function sym(name::Symbol)
    LIB[] == C_NULL && (LIB[] = Libdl.dlopen(libpath()))
    return Libdl.dlsym(LIB[], name)
end

check(rc) = rc == 0 || error("rocm_mpi_amd: " * unsafe_string(ccall(sym(:rma_last_error), Cstring, ())))

"""Node-local rank from the launcher (torchrun, SLURM, Open MPI, MPICH/Intel MPI), never
the global rank: on a second node the global rank names a GPU that does not exist there.
Without any of these variables the process is the node's only rank (device 0)."""
function launcher_local_rank()
    for name in ("LOCAL_RANK", "SLURM_LOCALID", "OMPI_COMM_WORLD_LOCAL_RANK", "MPI_LOCALRANKID")
        v = get(ENV, name, "")
        isempty(v) || return parse(Int, v)
    end
    return 0
end

"""init_global_grid(nx, ny, nz; dimx=0, dimy=0, dimz=0, periodx=0, periody=0, periodz=0,
overlaps=(2,2,2), halowidths=(1,1,1), comm=nothing, device=-1) -> (me, dims, nprocs, coords, comm)"""
function init_global_grid(nx::Integer, ny::Integer, nz::Integer; dimx=0, dimy=0, dimz=0,
                          periodx=0, periody=0, periodz=0, overlaps=(2, 2, 2),
                          halowidths=(1, 1, 1), comm=nothing, device::Integer=-1)
    nprocs, rank = 1, 0
    uid = zeros(UInt8, 128)
    local_rank = -1
    if comm !== nothing  # an MPI.Comm from MPI.jl
        MPI = Base.require(Base.PkgId(Base.UUID("da04e1cc-30fd-572f-bb4f-1f8673147195"), "MPI"))
        nprocs, rank = MPI.Comm_size(comm), MPI.Comm_rank(comm)
        rank == 0 && check(ccall(sym(:rma_unique_id), Cint, (Ptr{UInt8},), uid))
        MPI.Bcast!(uid, 0, comm)
        # node-local rank from the shared-memory split, as the reference does
        # (scripts/rocmaware_test_selectdevice.jl:7-9)
        comm_l = MPI.Comm_split_type(comm, MPI.COMM_TYPE_SHARED, rank)
        local_rank = MPI.Comm_rank(comm_l)
        MPI.free(comm_l)
    end
    dev = device >= 0 ? device : local_rank >= 0 ? local_rank : launcher_local_rank()
    g = Ref{Ptr{Cvoid}}(C_NULL)
    me = Ref{Cint}(0)
    dims = zeros(Cint, 3)
    coords = zeros(Cint, 3)
    check(ccall(sym(:rma_init_global_grid), Cint,
                (Cint, Cint, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Cint, Cint,
                 Ptr{UInt8}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}),
                nx, ny, nz, Cint[dimx, dimy, dimz], Cint[periodx, periody, periodz],
                Cint[overlaps...], Cint[halowidths...], nprocs, rank,
                nprocs > 1 ? uid : C_NULL, dev, g, me, dims, coords))
    GRID[] = g[]
    NXYZ[] = (nx, ny, nz)
    return Int(me[]), Tuple(Int.(dims)), nprocs, Tuple(Int.(coords)), comm
end

finalize_global_grid() = (check(ccall(sym(:rma_finalize_global_grid), Cint, (Ptr{Cvoid},), GRID[])); GRID[] = C_NULL; nothing)

nx_g() = Int(ccall(sym(:rma_nx_g), Int64, (Ptr{Cvoid},), GRID[]))
ny_g() = Int(ccall(sym(:rma_ny_g), Int64, (Ptr{Cvoid},), GRID[]))
nz_g() = Int(ccall(sym(:rma_nz_g), Int64, (Ptr{Cvoid},), GRID[]))
# IGG's indices are 1-based; the C ABI is 0-based
x_g(ix, dx, A) = ccall(sym(:rma_x_g), Float64, (Ptr{Cvoid}, Int64, Float64, Int64), GRID[], ix - 1, dx, size(A, 1))
y_g(iy, dy, A) = ccall(sym(:rma_y_g), Float64, (Ptr{Cvoid}, Int64, Float64, Int64), GRID[], iy - 1, dy, size(A, 2))
z_g(iz, dz, A) = ccall(sym(:rma_z_g), Float64, (Ptr{Cvoid}, Int64, Float64, Int64), GRID[], iz - 1, dz, size(A, 3))

"""update_halo!(A...): Julia column-major A[ix,iy,iz] is the row-major (nz,ny,nx) layout
of the native core, so sizes pass straight through."""
function update_halo!(A...; stream::Ptr{Cvoid}=C_NULL)
    ptrs = Ptr{Cvoid}[reinterpret(Ptr{Cvoid}, pointer(a)) for a in A]
    sizes = Int64[]
    for a in A
        append!(sizes, (size(a, 1), size(a, 2), size(a, 3)))
    end
    eb = Cint[sizeof(eltype(a)) for a in A]
    check(ccall(sym(:rma_update_halo), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Cint}, Ptr{Cvoid}),
                GRID[], length(A), ptrs, sizes, eb, stream))
    return nothing
end

"""gather!(A, A_global; root=0): IGG's gather!. `root` assembles every rank's `A` at its
Cartesian coordinates into `A_global` (size `dims .* size(A)`; `nothing` off-root). `A` and
`A_global` may each be a host `Array` or a device array: the pointers pass straight
through and the native side finds out which is which (rma_gather_igg). Blocking."""
function gather!(A, A_global; root::Integer=0, stream::Ptr{Cvoid}=C_NULL)
    sizes = Int64[size(A, 1), size(A, 2), size(A, 3)]
    check(ccall(sym(:rma_gather_igg), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                GRID[], devptr(A), sizes, C_NULL, sizeof(eltype(A)), devptr(A_global), root, stream))
    return nothing
end

"""gather_rankmajor!(A, A_global; root=0): the rank-major concatenation of device buffers
(rma_gather; what `gather!` did before it followed IGG's layout). Asynchronous on `stream`."""
function gather_rankmajor!(A, A_global; root::Integer=0, stream::Ptr{Cvoid}=C_NULL)
    check(ccall(sym(:rma_gather), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint, Ptr{Cvoid}),
                GRID[], pointer(A), A_global === nothing ? C_NULL : pointer(A_global),
                sizeof(A), root, stream))
    return nothing
end

const T0 = Ref(0.0)
tic(; stream::Ptr{Cvoid}=C_NULL) = check(ccall(sym(:rma_tic), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), GRID[], stream))
function toc(; stream::Ptr{Cvoid}=C_NULL)
    t = Ref{Float64}(0)
    check(ccall(sym(:rma_toc), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), GRID[], stream, t))
    return t[]
end

# Native executor (mode 0 perf, 1 perf_hide, 2 kp; coef = (-lam, 1/dx, 1/dy, dt)).
# The struct keeps every array the native executor reads or writes (T, T2,
# 1/Cp and the kp buffers) referenced for as long as it lives, so the GC cannot
# free one under a running executor (VERDICT r3: iCp was not kept).
mutable struct DiffusionExecutor
    ptr::Ptr{Cvoid}
    T::Any
    T2::Any
    iCp::Any
    qx::Any
    qy::Any
    dTdt::Any
end

devptr(a) = a === nothing ? C_NULL : reinterpret(Ptr{Cvoid}, pointer(a))

# steps_per_pass = K (1..24): at most K steps per kernel pass; run! plans the
# passes (csrc/runtime/plan.cpp). fast_math=true: every pass uses the
# 5-point-sum arithmetic (rounding-level difference from the canonical update,
# bitwise equal to its C++ CPU twin). graph_steps > 0: replay steps from a
# hipGraph of that many steps (rma_executor_create_g; needs a capturable halo
# transport). mode=2 (kp, the three kernels of diffusion_2D_kp.jl:88-91) needs
# qx, qy and dTdt: device arrays of size(T) (T-indexed flux / residual buffers,
# csrc/kernels/kp.hip); T2 is unused there and may be `nothing`.
function DiffusionExecutor(T, T2, iCp, coef::NTuple{4,Float64}; mode::Integer=1,
                           steps_per_pass::Integer=1, b_width=(1, 1), fast_math::Bool=false,
                           graph_steps::Integer=0, qx=nothing, qy=nothing, dTdt=nothing)
    if mode == 2
        (qx === nothing || qy === nothing || dTdt === nothing) &&
            error("DiffusionExecutor: kp mode (2) needs qx, qy and dTdt device arrays of size(T)")
        for (name, a) in (("qx", qx), ("qy", qy), ("dTdt", dTdt))
            size(a) == size(T) || error("DiffusionExecutor: $name must have size(T) = $(size(T)), got $(size(a))")
        end
    else
        T2 === nothing && error("DiffusionExecutor: modes 0/1 need T2")
    end
    out = Ref{Ptr{Cvoid}}(C_NULL)
    c = collect(coef)
    nx, ny = size(T, 1), size(T, 2)
    check(ccall(sym(:rma_executor_create_g), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64},
                 Int64, Int64, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
                 Ptr{Ptr{Cvoid}}),
                GRID[], mode, devptr(T), devptr(T2), devptr(iCp), nx, ny, c, b_width[1],
                b_width[2], steps_per_pass, Cint(fast_math), Cint(graph_steps), devptr(qx),
                devptr(qy), devptr(dTdt), out))
    ex = DiffusionExecutor(out[], T, T2, iCp, qx, qy, dTdt)
    # the native grid is pinned by its executors: finalize_global_grid before
    # this finalizer runs is safe (the teardown waits for the last destroy)
    finalizer(e -> ccall(sym(:rma_executor_destroy), Cint, (Ptr{Cvoid},), e.ptr), ex)
    return ex
end

run!(ex::DiffusionExecutor, n::Integer; stream::Ptr{Cvoid}=C_NULL) =
    check(ccall(sym(:rma_executor_run), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}), ex.ptr, n, stream))

current_field(ex::DiffusionExecutor) =
    ex.T2 === nothing || ccall(sym(:rma_executor_parity), Cint, (Ptr{Cvoid},), ex.ptr) == 0 ? ex.T : ex.T2

# after synchronising the stream: throws if a frame-first fused pass timed out
# waiting for its frame flag (rma_executor_check); returns the fused-pass count
function check_executor(ex::DiffusionExecutor)
    nf = Ref{Int64}(0)
    check(ccall(sym(:rma_executor_check), Cint, (Ptr{Cvoid}, Ref{Int64}), ex.ptr, nf))
    return nf[]
end

# ---------------- 3D heat diffusion ----------------
# Arrays are A[ix,iy,iz] (the native (nz,ny,nx) layout); coef = (-lam, 1/dx, 1/dy, 1/dz, dt).

"""diffusion3d_step!(T2, T, iCp, coef): one fused 7-point step on the whole interior."""
function diffusion3d_step!(T2, T, iCp, coef::NTuple{5,Float64}; stream::Ptr{Cvoid}=C_NULL)
    check(ccall(sym(:rma_diffusion3d_step), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}),
                devptr(T2), devptr(T), devptr(iCp), size(T, 1), size(T, 2), size(T, 3),
                collect(coef), stream))
    return nothing
end

"""diffusion3d_boxes!(T2, T, iCp, coef, boxes; steps=1, fast_math=false): `steps` (1 or 2)
time steps in one pass on at most 8 boxes. A box is (x0, x1, y0, y1, z0, z1), 1-based and
inclusive as Julia ranges x0:x1 (converted to the C ABI's 0-based half-open bounds)."""
function diffusion3d_boxes!(T2, T, iCp, coef::NTuple{5,Float64}, boxes; steps::Integer=1,
                            fast_math::Bool=false, stream::Ptr{Cvoid}=C_NULL)
    flat = Int64[]
    for b in boxes
        append!(flat, (b[1] - 1, b[2], b[3] - 1, b[4], b[5] - 1, b[6]))
    end
    check(ccall(sym(:rma_diffusion3d_boxes), Cint,
                (Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Cint,
                 Ptr{Float64}, Cint, Ptr{Cvoid}),
                steps, devptr(T2), devptr(T), devptr(iCp), size(T, 1), size(T, 2), size(T, 3),
                flat, length(boxes), collect(coef), Cint(fast_math), stream))
    return nothing
end

"""init_gaussian3d!(T, dx, dy, dz, lx, ly, lz): the reference's initial Gaussian on cell
centres, computed on the device for this rank's tile of the global grid."""
function init_gaussian3d!(T, dx, dy, dz, lx, ly, lz; stream::Ptr{Cvoid}=C_NULL)
    check(ccall(sym(:rma_init_gaussian3d), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Float64, Float64, Float64, Float64,
                 Float64, Float64, Ptr{Cvoid}),
                GRID[], devptr(T), size(T, 1), size(T, 2), size(T, 3), dx, dy, dz, lx, ly, lz,
                stream))
    return T
end

"""init_random3d!(A, dx, dy, dz; seed=0): uniform [0,1) keyed by the global cell index (the
same field for every decomposition)."""
function init_random3d!(A, dx, dy, dz; seed::Integer=0, stream::Ptr{Cvoid}=C_NULL)
    check(ccall(sym(:rma_init_random3d), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Float64, Float64, Float64, UInt64,
                 Ptr{Cvoid}),
                GRID[], devptr(A), size(A, 1), size(A, 2), size(A, 3), dx, dy, dz, UInt64(seed),
                stream))
    return A
end

# Native 3D time loop (mode 0 perf, 1 perf_hide). As DiffusionExecutor, the struct
# keeps T, T2 and 1/Cp referenced for as long as the native executor lives.
mutable struct Diffusion3DExecutor
    ptr::Ptr{Cvoid}
    T::Any
    T2::Any
    iCp::Any
end

# steps_per_pass = 1 or 2; b_width = perf_hide's boundary width per dimension from the
# array edge; xface = 0..32 (the widest frame box on the x-face path of the one- and
# two-step kernels, two-step frames up to width 30; -1: min(max(b_width[1], overlap_x), 32)).
# fused = true (mode 1): frame-first single-launch passes (rma_executor3d_create_f), the
# same field bit for bit; check_fused(ex) after synchronising throws if a wait timed out.
# T2 must hold a copy of T.
function Diffusion3DExecutor(T, T2, iCp, coef::NTuple{5,Float64}; mode::Integer=1,
                             steps_per_pass::Integer=1, b_width=(16, 2, 2),
                             fast_math::Bool=false, xface::Integer=0, fused::Bool=false)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall(sym(:rma_executor3d_create_f), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64,
                 Ptr{Float64}, Ptr{Int64}, Cint, Cint, Cint, Cint, Ptr{Ptr{Cvoid}}),
                GRID[], mode, devptr(T), devptr(T2), devptr(iCp), size(T, 1), size(T, 2),
                size(T, 3), collect(coef), Int64[b_width...], steps_per_pass, Cint(fast_math),
                xface, Cint(fused), out))
    ex = Diffusion3DExecutor(out[], T, T2, iCp)
    # pins the native grid like the 2D executor: any finalization order is safe
    finalizer(e -> ccall(sym(:rma_executor3d_destroy), Cint, (Ptr{Cvoid},), e.ptr), ex)
    return ex
end

run!(ex::Diffusion3DExecutor, n::Integer; stream::Ptr{Cvoid}=C_NULL) =
    check(ccall(sym(:rma_executor3d_run), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}), ex.ptr, n, stream))

# after synchronising the stream: throws if a fused pass timed out waiting for its frame
# flag (rma_executor3d_check); returns the fused-pass count
function check_fused(ex::Diffusion3DExecutor)
    check(ccall(sym(:rma_executor3d_check), Cint, (Ptr{Cvoid},), ex.ptr))
    return ccall(sym(:rma_executor3d_fused_passes), Int64, (Ptr{Cvoid},), ex.ptr)
end

current_field(ex::Diffusion3DExecutor) =
    ccall(sym(:rma_executor3d_parity), Cint, (Ptr{Cvoid},), ex.ptr) == 0 ? ex.T : ex.T2

"""uniform_factor(ex): the last scan found one value in every cell of 1/Cp (the passes
then take it as a kernel argument and do not read the array)."""
uniform_factor(ex::Diffusion3DExecutor) =
    ccall(sym(:rma_executor3d_uniform), Cint, (Ptr{Cvoid},), ex.ptr) != 0

"""rescan_factor!(ex): examine 1/Cp again after writing to it (synchronises the device)."""
function rescan_factor!(ex::Diffusion3DExecutor)
    u = Ref{Cint}(0)
    check(ccall(sym(:rma_executor3d_rescan_factor), Cint, (Ptr{Cvoid}, Ptr{Cint}), ex.ptr, u))
    return u[] != 0
end

end # module
