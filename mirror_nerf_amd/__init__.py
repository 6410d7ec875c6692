"""mirror_nerf_amd -- MI355X-native (gfx950) implementation of Mirror-NeRF's volumetric
rendering hot path behind the reference's own Python interfaces.

    from mirror_nerf_amd import render_rays, MirrorNeRF, Embedding      # models/rendering.py, models/mirror_nerf.py
    from mirror_nerf_amd import NeRFSystem, batched_inference          # train.py:102-348, eval.py:114-740
    from mirror_nerf_amd import DirectTemporalNeRF, render_rays_dnerf  # models/d_nerf: the animated object of run.sh MODE 4
    from mirror_nerf_amd import ObjectBounds, estimate_object_bounds    # where a placed object is: batched_inference(object_bounds=)
    from mirror_nerf_amd import PlacedObject                            # several objects: batched_inference(placed_objects=[...])
    from mirror_nerf_amd import PlacedMirror                            # several mirrors on any plane: batched_inference(new_mirrors=[...])
    from mirror_nerf_amd import get_loss                                # losses.py:258 (TotalLoss, fused value + gradient)
    from mirror_nerf_amd import RayBank, read_blender                   # datasets/blender.py: training batches drawn on the device
    from mirror_nerf_amd import finish_frame, SplitExtrema, colormap_depth   # eval.py:743-978: the 8-bit images of a frame
    from mirror_nerf_amd import validation_step, validate, val_panel    # train.py:460-543, utils/visualization.py:26-184

All arithmetic runs in libmnrf_hip.so (include/mnrf.h).  There is no CPU fallback.
"""
from .mirror_nerf import Embedding, MirrorNeRF, check_guard, reset_guard, set_precision, verify_split  # noqa: F401
from .mirror_nerf_tcnn import MirrorNeRFTcnn  # noqa: F401
from .rendering import render_rays, sample_pdf  # noqa: F401
from .recursion import NeRFSystem, batched_inference, render_rays_chunk_recursively  # noqa: F401
from .dnerf import DirectTemporalNeRF, load_dnerf_object, render_rays_dnerf  # noqa: F401
from .object_bounds import ObjectBounds, estimate_object_bounds  # noqa: F401
from .placed_objects import PlacedObject  # noqa: F401
from .placed_mirrors import PlacedMirror  # noqa: F401
from .losses import TotalLoss, get_loss  # noqa: F401
from .data import RayBank, read_blender  # noqa: F401
from . import frames  # noqa: F401
from .frames import SplitExtrema, colormap_depth, finish_frame, jet_table, val_panel  # noqa: F401
from .validation import validate, validation_step  # noqa: F401
from . import _lib  # noqa: F401

__all__ = ["Embedding", "MirrorNeRF", "render_rays", "sample_pdf", "NeRFSystem", "batched_inference",
           "render_rays_chunk_recursively", "DirectTemporalNeRF", "load_dnerf_object", "render_rays_dnerf", "ObjectBounds", "estimate_object_bounds", "PlacedObject", "PlacedMirror", "TotalLoss", "get_loss", "RayBank", "read_blender", "frames", "finish_frame", "SplitExtrema",
           "colormap_depth", "jet_table", "val_panel", "validation_step", "validate"]
