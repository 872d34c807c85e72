"""Hand-written HIP/CDNA4 kernels (gfx950) exposed on torch tensors."""
from .stencil import (FAST5, KERNELS, KSTEP_CORE, LAB_KERNELS, PIPE, PIPE_MAX_K, Rect, StencilCoef, StencilTuning,
                      TileGeometry, check_field, count_differing, fast5_constants, fast5_ok, field_stats, fill_, flux,
                      fma_exact, hide_rects, init_gaussian_, init_random_, interior_rect,
                      kernel_id, kernel_name, kp_views, reduce, residual, stencil2_step, stencil5_torch, stencil_step,
                      stencil_torch, stencilk_step, stream_handle, strip_cells, update,
                      validate_rects)
from .stencil3d import (TB_ROWS_3D, TEMPORAL_3D, TUNINGS_3D, XFACE_MAX, Box, Stencil3DTuning, StencilCoef3,
                        TileGeometry3, init_gaussian3d_, init_random3d_, interior_box,
                        fast7_ok, stencil3d_step, stencil3d_torch, stencil3dk_step, stencil3dk_torch,
                        hide_boxes3d, stencil3d_dispatch, validate_boxes, FusedPlan3D,
                        stencil3d_fused_plan)
from .halo_ops import copy_plane, copy_planes
from .block_ops import assemble_blocks, copy_blocks

__all__ = [
    "FAST5", "KERNELS", "KSTEP_CORE", "LAB_KERNELS", "PIPE", "PIPE_MAX_K", "Rect", "StencilCoef", "StencilTuning",
    "TileGeometry", "check_field", "count_differing", "fast5_constants", "fast5_ok", "field_stats", "fill_", "flux", "fma_exact",
    "hide_rects", "init_gaussian_", "init_random_", "interior_rect", "kernel_id", "kernel_name", "kp_views", "reduce",
    "residual", "stencil2_step", "stencil5_torch", "stencil_step", "stencil_torch",
    "stencilk_step", "stream_handle", "strip_cells", "update", "validate_rects", "copy_plane", "copy_planes",
    "assemble_blocks", "copy_blocks",
    "TUNINGS_3D", "Box", "Stencil3DTuning", "StencilCoef3", "TileGeometry3", "init_gaussian3d_",
    "init_random3d_", "interior_box", "stencil3d_step", "stencil3d_torch", "validate_boxes",
    "TB_ROWS_3D", "TEMPORAL_3D", "fast7_ok", "stencil3dk_step", "stencil3dk_torch",
    "XFACE_MAX", "hide_boxes3d", "stencil3d_dispatch", "FusedPlan3D", "stencil3d_fused_plan",
]
