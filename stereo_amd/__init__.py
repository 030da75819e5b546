"""stereo_amd -- MI355X-native 3D-label stereo energy minimisation.

Host-side mirror (Python) of the reference's MATLAB solver surface
(`trws.m`, `rd.m`) over the C ABI of ``libstereo_hip.so``
(``include/stereo_hip.h``).  Names, argument meaning and error behaviour follow
the reference wrappers; arrays use MATLAB shapes (K x N, 2 x E, ...).
"""
from . import _lib
from ._lib import StereoHipError, device_count, LIB_PATH  # noqa: F401
from .trws import trws, TrwsPlan, TrwsState  # noqa: F401
from .rd import rd  # noqa: F401
from .dispmap import dispmap_super, dispmap_ncc, dispmap_globalstereo  # noqa: F401
from .fusion import PlaneProposal  # noqa: F401
from .segment import vgg_segment_ms, vgg_segment_gb  # noqa: F401
from .consistency import lr_check, lr_fill, lr_check_device, lr_fill_device, solve_pair_ncc  # noqa: F401
from .band import band_inputs, band_apply, band_inputs_device, band_apply_device, refine_band  # noqa: F401
from .pyramid import solve_pair_ncc_pyramid, solve_view_ncc_plane_pyramid  # noqa: F401
from .carry import carry_messages, carry_messages_device, scale_edge_map  # noqa: F401
from .plane_band import (plane_band_inputs, plane_band_apply, plane_band_inputs_device, plane_band_apply_device,  # noqa: F401
                         refine_plane_band, NccSource, GlobalstereoSource, PlaneBandProblem)
from .candidates import (candidates_inputs, candidates_apply, candidates_inputs_device, candidates_apply_device,  # noqa: F401
                         refine_candidates, CandidateProblem)
from . import candidates  # noqa: F401
from .plane_candidates import (plane_candidates_inputs, plane_candidates_apply, plane_candidates_inputs_device,  # noqa: F401
                               plane_candidates_apply_device, refine_plane_candidates, PlaneCandidateProblem)
from . import plane_candidates  # noqa: F401
from . import scanline  # noqa: F401
from .scanline import solve_pair_ncc_scanline  # noqa: F401
from . import contrast  # noqa: F401
from .contrast import Contrast  # noqa: F401
from . import mapfilter  # noqa: F401
from .mapfilter import MedianFilter  # noqa: F401

__all__ = ["contrast", "Contrast", "scanline", "solve_pair_ncc_scanline", "plane_candidates", "plane_candidates_inputs", "plane_candidates_apply", "plane_candidates_inputs_device", "plane_candidates_apply_device", "refine_plane_candidates", "PlaneCandidateProblem", "candidates", "candidates_inputs", "candidates_apply", "candidates_inputs_device", "candidates_apply_device", "refine_candidates", "CandidateProblem","trws", "rd", "dispmap_super", "dispmap_ncc", "dispmap_globalstereo", "TrwsPlan", "TrwsState", "PlaneProposal", "vgg_segment_ms", "vgg_segment_gb", "lr_check", "lr_fill", "lr_check_device", "lr_fill_device", "solve_pair_ncc", "solve_pair_ncc_pyramid", "solve_view_ncc_plane_pyramid", "band_inputs", "band_apply", "band_inputs_device", "band_apply_device", "refine_band", "carry_messages", "carry_messages_device", "scale_edge_map", "plane_band_inputs", "plane_band_apply", "plane_band_inputs_device", "plane_band_apply_device", "refine_plane_band", "NccSource", "GlobalstereoSource", "PlaneBandProblem", "StereoHipError", "device_count", "LIB_PATH"]

# Load the library (and let the HIP runtime finish its one-time initialisation, which draws from
# libc rand()) when the package is imported, not inside the first solver call: a caller that seeds
# rand() to reproduce the reference's QPBO Improve does so after the import.  Without a built
# library the import still succeeds; the first call then reports it.
try:
    _lib.lib()
except StereoHipError:
    pass
