"""Model family: the 2D diffusion variants of the reference (ap, kp, perf, perf_hide)
and the 3D diffusion model (perf, ap)."""
from .diffusion import VARIANTS, Diffusion2D, DiffusionConfig
from .diffusion3d import VARIANTS3D, Diffusion3D, Diffusion3DConfig

__all__ = ["VARIANTS", "Diffusion2D", "DiffusionConfig", "VARIANTS3D", "Diffusion3D",
           "Diffusion3DConfig"]
