"""fray_amd -- MI355X-native renderer for fray's per-pixel ray-trace hot path.

Python is only the plumbing above the C ABI (include/frayhip.h, fray_amd/libfrayhip.so): it mirrors
the reference's `Scene` interface (src/scene.h:280-299: parseScene / settings / camera /
beginRender) and `render()` (src/main.cpp:373).  All rendering happens in the HIP library; there is
no CPU fallback -- if the library is missing or no GPU is present the calls fail loudly.
"""
from .scene import (Scene, Accumulation, FrayError, lib, render_info, denoise, denoise_params, denoise_signal,  # noqa: F401
                    temporal_accumulate, temporal_params, view_from_camera, Transform, light_begin_frame, shader_begin_frame,
                    temporal_accumulate_split, split_history_parts, join_history_parts, change_frame, change_params, sample_map, sample_map_params,
                    history_map)
from . import abi  # noqa: F401

__all__ = ["Scene", "Accumulation", "FrayError", "lib", "abi", "render_info", "denoise", "denoise_params", "denoise_signal", "temporal_accumulate",
           "temporal_params", "view_from_camera", "Transform", "light_begin_frame", "shader_begin_frame", "temporal_accumulate_split",
           "split_history_parts", "join_history_parts", "change_frame", "change_params", "sample_map", "sample_map_params", "history_map"]
