"""flowfusion_amd: MI355X-native sampling / log-density path of Cosmo-Pop/flowfusion.

``flowfusion_amd.diffusion``, ``flowfusion_amd.flow`` and ``flowfusion_amd.symplectic`` mirror the reference modules
``flowfusion.diffusion`` / ``flowfusion.flow`` / ``flowfusion.symplectic``; the solves run in libflowfusion_amd.so
(hand-written HIP for gfx950, C ABI in include/flowfusion_amd.h).
"""
from . import diffusion, flow, symplectic  # noqa: F401

__all__ = ["diffusion", "flow", "symplectic"]
__version__ = "0.4.0"
