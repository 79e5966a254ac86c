"""Host-side mirror of the reference's Scene / render() interface over the C ABI."""
import ctypes as C
import math
import os
import sys

import numpy as np

from . import abi

P = C.POINTER

_HERE = os.path.dirname(os.path.abspath(__file__))
# FRAYHIP_LIB: A/B-test another build of the same library (development only)
_LIB_PATH = os.environ.get("FRAYHIP_LIB") or os.path.join(_HERE, "libfrayhip.so")


class FrayError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("frayhip error %d: %s" % (code, msg))
        self.code = code


def _load():
    # PyTorch wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, no versioned SONAME).
    # A process must not end up with two HIP runtimes: whichever is loaded second finds no GPU and
    # stream handles do not carry over.  Loading torch first puts its runtime in the global symbol
    # scope, and libfrayhip.so then binds to that same runtime.  (Hosts that never use torch --
    # e.g. the reference's C++ main() -- just get /opt/rocm's runtime.)
    if "torch" not in sys.modules and not os.environ.get("FRAYHIP_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            "fray_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make`). There is no CPU fallback." % _LIB_PATH)
    return abi.bind(C.CDLL(_LIB_PATH))


lib = _load()


def _check(rc):
    if rc != 0:
        raise FrayError(rc, (lib.frayhip_last_error() or b"").decode("utf-8", "replace"))


def render_info():
    return {"library": _LIB_PATH, "abi_version": lib.frayhip_abi_version()}


class _ProgressRun:
    """The Python side of a progressive call: turns every callback into an info dict for `progress`, keeps an exception raised inside it
    (ctypes would print it and carry on) and cancels the frame instead, and re-raises it after the call."""

    def __init__(self, progress, frame_view):
        self.progress, self.frame_view = progress, frame_view
        self.error, self.samples_done = None, 0

    def __call__(self, _user, p):
        try:
            p = p.contents
            self.samples_done = p.samples_done
            info = p.as_dict()
            if p.preview and p.rgb:
                info.update(self.frame_view(p))
            return 1 if self.progress(info) else 0
        except BaseException as e:          # noqa: B902 -- KeyboardInterrupt too: it cancels the frame, then propagates
            if self.error is None:
                self.error = e
            return 1

    def finish(self, rc, st):
        if self.error is not None:
            raise self.error
        if rc not in (abi.OK, abi.E_CANCELLED):
            _check(rc)
        d = st.as_dict()
        d["samples_done"] = self.samples_done
        d["cancelled"] = rc == abi.E_CANCELLED
        return d


def _progress_request(progress, preview_ms, frame_view):
    run = _ProgressRun(progress, frame_view)
    req = abi.Progressive(fn=abi.PROGRESS_FN(run), user=None, preview_ms=float(preview_ms))
    req._run = run                          # the request keeps the ctypes callback object alive for the call
    return req, run


def _torch_tensor(x):
    t = sys.modules.get("torch")
    return t is not None and isinstance(x, t.Tensor)


def _query_inputs(named, width=3):
    """The inputs of a ray query, [(name, value)]: numpy arrays or device torch tensors (not a mix), float64, shaped [..., width], all of one
    shape.  Returns (contiguous inputs, leading shape, torch device or None)."""
    tensors = [_torch_tensor(v) for _, v in named]
    if any(tensors) and not all(tensors):
        raise TypeError("ray query: pass numpy arrays or torch tensors, not a mix")
    out, shape, device = [], None, None
    for name, v in named:
        if tensors[0]:
            import torch
            if not v.is_cuda:
                raise TypeError("ray query: %s is a CPU tensor; pass a tensor on the GPU (device entry) or a numpy array (host entry)" % name)
            if v.dtype != torch.float64:
                raise TypeError("ray query: %s must be float64, got %s" % (name, v.dtype))
            if device is not None and v.device != device:
                raise ValueError("ray query: the inputs are on different devices")
            device = v.device
        else:
            v = np.asarray(v)
            if v.dtype != np.float64:
                raise TypeError("ray query: %s must be float64, got %s" % (name, v.dtype))
        if v.ndim < 1 or v.shape[-1] != width:
            raise ValueError("ray query: %s must be shaped [..., %d], got %s" % (name, width, tuple(v.shape)))
        if shape is not None and tuple(v.shape[:-1]) != shape:
            raise ValueError("ray query: the inputs' shapes differ: %s and %s" % (shape, tuple(v.shape[:-1])))
        shape = tuple(v.shape[:-1])
        out.append(v)
    return out, shape, device


class _DeviceCall:
    """A device entry's call on a torch stream: inputs made contiguous and outputs allocated on that stream (the entry synchronises it)."""

    def __init__(self, device, stream):
        import torch
        self.torch = torch
        self.stream = stream if stream is not None else torch.cuda.current_stream(device)
        self.ctx = torch.cuda.stream(self.stream)

    def __enter__(self):
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)

    @property
    def handle(self):
        return C.c_void_p(self.stream.cuda_stream)


_DENOISE_FIELDS = ("levels", "demodulate", "sigma_luminance", "sigma_normal", "sigma_depth", "sigma_albedo")


def denoise_params(**params):
    """frayhip_denoise_defaults, with the named fields replaced (levels, demodulate, sigma_luminance, sigma_normal, sigma_depth, sigma_albedo)."""
    p = abi.Denoise()
    _check(lib.frayhip_denoise_defaults(C.byref(p)))
    for k, v in params.items():
        if k not in _DENOISE_FIELDS:
            raise TypeError("denoise: unknown parameter %r (known: %s)" % (k, ", ".join(_DENOISE_FIELDS)))
        setattr(p, k, v)
    return p


def _frame_inputs(who, named):
    """The per-pixel inputs of a scene-free entry, [(name, value, channels)] (channels 0: a plane shaped [H, W]): numpy arrays or device torch
    tensors (not a mix), float32, all of one size.  Returns (contiguous inputs, (H, W), whether they are tensors)."""
    tensors = [_torch_tensor(v) for _, v, _ in named]
    if any(tensors) and not all(tensors):
        raise TypeError("%s: pass numpy arrays or torch tensors, not a mix" % who)
    shape = None
    ins = []
    for name, v, width in named:
        if tensors[0]:
            import torch
            if not v.is_cuda:
                raise TypeError("%s: %s is a CPU tensor; pass a tensor on the GPU (device entry) or a numpy array (host entry)" % (who, name))
            if v.dtype != torch.float32:
                raise TypeError("%s: %s must be float32, got %s" % (who, name, v.dtype))
            if ins and v.device != ins[0].device:
                raise ValueError("%s: the inputs are on different devices" % who)
            v = v.contiguous()
        else:
            v = np.ascontiguousarray(v)
            if v.dtype != np.float32:
                raise TypeError("%s: %s must be float32, got %s" % (who, name, v.dtype))
        if width == 0:
            if v.ndim != 2:
                raise ValueError("%s: %s must be shaped [H, W], got %s" % (who, name, tuple(v.shape)))
        elif v.ndim != 3 or v.shape[2] != width:
            raise ValueError("%s: %s must be shaped [H, W, %d], got %s" % (who, name, width, tuple(v.shape)))
        if shape is not None and tuple(v.shape[:2]) != shape:
            raise ValueError("%s: the inputs' sizes differ: %s and %s" % (who, shape, tuple(v.shape[:2])))
        shape = tuple(v.shape[:2])
        ins.append(v)
    return ins, shape, tensors[0]


def _ptr(v):
    return None if v is None else v.data_ptr() if _torch_tensor(v) else v.ctypes.data


def denoise(rgb, feat, rgb_half=None, stats=False, stream=None, **params):
    """The edge-avoiding a-trous filter of include/frayhip.h (frayhip_denoise): rgb [H, W, 3] float32, feat [H, W, 10] float32 (render_features),
    rgb_half [H, W, 3] float32 or None (the frame of the first half of rgb's samples: the filter's noise estimate).  numpy arrays go through the
    host entry; torch tensors on the GPU through the device entry, on `stream` (None: the current stream).  params: see denoise_params.
    Returns the filtered frame (same kind as rgb), and with stats=True also the stats dict (ms_total, ms_kernels)."""
    p = denoise_params(**params)
    named = [("rgb", rgb, 3), ("feat", feat, abi.FEAT_CHANNELS)] + ([("rgb_half", rgb_half, 3)] if rgb_half is not None else [])
    ins, (H, W), tensors = _frame_inputs("denoise", named)
    half = ins[2] if rgb_half is not None else None
    st = abi.Stats()
    if not tensors:
        out = np.empty((H, W, 3), np.float32)
        _check(lib.frayhip_denoise(W, H, _ptr(ins[0]), _ptr(half), _ptr(ins[1]), C.byref(p), out.ctypes.data, C.byref(st)))
    else:
        with _DeviceCall(ins[0].device, stream) as call:
            out = call.torch.empty((H, W, 3), dtype=call.torch.float32, device=ins[0].device)
            _check(lib.frayhip_denoise_device(W, H, _ptr(ins[0]), _ptr(half), _ptr(ins[1]), C.byref(p), out.data_ptr(), call.handle, C.byref(st)))
    return (out, st.as_dict()) if stats else out


def denoise_signal(signal, variance, feat, stats=False, stream=None, **params):
    """The a-trous levels on a given signal and variance (frayhip_denoise_signal): signal [H, W, 3] and variance [H, W] as temporal_accumulate
    returns them, feat [H, W, 10]; float32.  With demodulate (the default) the signal is taken as already demodulated and the albedo is
    multiplied back.  numpy arrays or GPU torch tensors, `stream`, params and the return value as denoise()."""
    p = denoise_params(**params)
    ins, (H, W), tensors = _frame_inputs("denoise_signal", [("signal", signal, 3), ("variance", variance, 0), ("feat", feat, abi.FEAT_CHANNELS)])
    st = abi.Stats()
    if not tensors:
        out = np.empty((H, W, 3), np.float32)
        _check(lib.frayhip_denoise_signal(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), C.byref(p), out.ctypes.data, C.byref(st)))
    else:
        with _DeviceCall(ins[0].device, stream) as call:
            out = call.torch.empty((H, W, 3), dtype=call.torch.float32, device=ins[0].device)
            _check(lib.frayhip_denoise_signal_device(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), C.byref(p), out.data_ptr(), call.handle, C.byref(st)))
    return (out, st.as_dict()) if stats else out


_denoise_params = denoise_params         # Scene.render_sequence takes **denoise_params


def _sum_stats(a, b):
    """The stats dict of two calls that together are one step of a sequence: every figure is the sum of the two."""
    return {k: a[k] + b[k] for k in a}
_TEMPORAL_FIELDS = ("demodulate", "max_history", "variance_history", "alpha_min", "film_offset", "plane_tolerance", "normal_min_dot")


def temporal_params(**params):
    """frayhip_temporal_defaults, with the named fields replaced (demodulate, max_history, variance_history, alpha_min, film_offset,
    plane_tolerance, normal_min_dot)."""
    p = abi.Temporal()
    _check(lib.frayhip_temporal_defaults(C.byref(p)))
    for k, v in params.items():
        if k not in _TEMPORAL_FIELDS:
            raise TypeError("temporal: unknown parameter %r (known: %s)" % (k, ", ".join(_TEMPORAL_FIELDS)))
        setattr(p, k, v)
    return p


def view_from_camera(camera, width, height):
    """frayhip_view_from_camera: the abi.View of an abi.Camera (Scene.camera) on a width x height film -- the previous view that
    temporal_accumulate reprojects into."""
    if not isinstance(camera, abi.Camera):
        raise TypeError("view_from_camera: camera must be an abi.Camera, got %s" % type(camera).__name__)
    v = abi.View()
    _check(lib.frayhip_view_from_camera(C.byref(camera), int(width), int(height), C.byref(v)))
    return v


def change_params(radius=3, gain=1.0):
    """A frayhip_change with the given fields (the defaults are frayhip_change_defaults')."""
    p = abi.Change()
    _check(lib.frayhip_change_defaults(C.byref(p)))
    p.radius, p.gain = int(radius), float(gain)
    return p


def change_frame(before, after, motion=None, stats=False, stream=None, radius=3, gain=1.0):
    """The change frame of include/frayhip.h (frayhip_change_frame): before and after are two states [H, W, 4] float32 -- or the Accumulations
    that hold them (Scene.render_samples, or one component of Scene.render_components) -- of the SAME samples of one seed and view, rendered
    before and after an edit of the scene; motion [H, W, 8] or None masks the pixels of moved nodes.  numpy arrays go through the host entry;
    torch tensors on the GPU (storage 16-byte aligned) through the device entry, on `stream` (None: the current stream).  radius 0..3: the
    window is (2 radius + 1)^2 pixels; gain > 0.  Returns change [H, W] float32 of the inputs' kind, in [0, 1] and exactly 0 where no state in
    the window differs -- temporal_accumulate's change= -- and with stats=True also the stats dict (ms_total, ms_kernels)."""
    who = "change_frame"
    if isinstance(before, Accumulation) and isinstance(after, Accumulation) and before.samples_done != after.samples_done:
        raise ValueError("%s: before holds %d samples per pixel and after %d" % (who, before.samples_done, after.samples_done))
    before, after = (a.state if isinstance(a, Accumulation) else a for a in (before, after))
    p = change_params(radius, gain)
    named = [("before", before, abi.ACCUM_CHANNELS), ("after", after, abi.ACCUM_CHANNELS)]
    if motion is not None:
        named.append(("motion", motion, abi.MOTION_CHANNELS))
    ins, (H, W), tensors = _frame_inputs(who, named)
    mot = ins[2] if motion is not None else None
    st = abi.Stats()
    if not tensors:
        out = np.empty((H, W), np.float32)
        _check(lib.frayhip_change_frame(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(mot), C.byref(p), out.ctypes.data, C.byref(st)))
    else:
        with _DeviceCall(ins[0].device, stream) as call:
            out = call.torch.empty((H, W), dtype=call.torch.float32, device=ins[0].device)
            _check(lib.frayhip_change_frame_device(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(mot), C.byref(p), out.data_ptr(), call.handle, C.byref(st)))
    return (out, st.as_dict()) if stats else out


_SAMPLE_MAP_FIELDS = ("tolerance", "lum_floor", "min_count", "max_count", "max_add", "grow")
_MAX_COUNT = 1 << 24


def sample_map_params(**params):
    """frayhip_sample_map_defaults, with the named fields replaced (tolerance, lum_floor, min_count, max_count, max_add, grow), checked as the
    library checks them (ValueError).  max_count has no default: the caller sets it."""
    p = abi.SampleMap()
    _check(lib.frayhip_sample_map_defaults(C.byref(p)))
    for k, v in params.items():
        if k not in _SAMPLE_MAP_FIELDS:
            raise TypeError("sample_map: unknown parameter %r (known: %s)" % (k, ", ".join(_SAMPLE_MAP_FIELDS)))
        setattr(p, k, float(v) if k in ("tolerance", "lum_floor") else int(v))
    if "max_count" not in params:
        raise ValueError("sample_map: max_count must be given (it has no default)")
    for k in ("tolerance", "lum_floor"):
        v = float(params.get(k, getattr(p, k)))
        if not (math.isfinite(v) and v > 0):
            raise ValueError("sample_map: %s must be finite and > 0, got %r" % (k, v))
    if p.min_count < 1:
        raise ValueError("sample_map: min_count must be >= 1, got %d" % p.min_count)
    if not (p.min_count <= p.max_count <= _MAX_COUNT):
        raise ValueError("sample_map: max_count must be min_count .. 2^24, got %d (min_count %d)" % (p.max_count, p.min_count))
    if p.max_add < 1:
        raise ValueError("sample_map: max_add must be >= 1, got %d" % p.max_add)
    if not (2 <= p.grow <= 16):
        raise ValueError("sample_map: grow must be 2..16, got %d" % p.grow)
    return p


def _budget_of(who, budget):
    """A frame-wide sample budget as the library takes it: None, or an integer 0 .. 2^64 - 1 (bool and float are refused)."""
    if budget is None:
        return None
    if isinstance(budget, bool) or not isinstance(budget, (int, np.integer)):
        raise TypeError("%s: budget must be an integer or None, got %s" % (who, type(budget).__name__))
    if not (0 <= int(budget) < 1 << 64):
        raise ValueError("%s: budget must be 0 .. 2^64 - 1, got %d" % (who, int(budget)))
    return int(budget)


def _budget_info(info, b):
    info.update(budget=int(b.budget), demand=int(b.demand), tolerance_used=float(b.tolerance_used), cap_used=int(b.cap_used), stage=int(b.stage))


def sample_map(state, stats=False, stream=None, budget=None, **params):
    """The sample map of a state (frayhip_sample_map): how many more samples each pixel of the Accumulation `state` needs before the standard error
    of its mean's luminance is `tolerance` times that luminance, every pixel brought to min_count first and none past max_count (params: see
    sample_map_params; the formula is in include/frayhip.h "sample maps").  A numpy state goes through the host entry, a state on the GPU through
    the device entry, on `stream` (None: the current stream).  Returns (add, info): add int32 [H, W] of the state's kind -- what
    Scene.render_samples_map takes -- and info {"pixels": pixels with add > 0, "samples": the sum of add}, both over the whole frame, with
    "stats" (ms_total, ms_kernels) when stats=True.
    state may also be a pair (direct, indirect) of component states holding the same samples (Scene.render_components_map): the map then comes from
    frayhip_sample_map_pair, which adds the two components' mean luminances and their noise estimates, and is what render_components_map takes.
    budget: None, or the most samples the map may hand out over the whole frame, an int >= 0 (frayhip_sample_map_budget: the tolerance is raised
    until the frame can afford it, and where no tolerance is enough a per-pixel cap is lowered; include/frayhip.h has the three stages).  info then
    gains "budget", "demand" (what `tolerance` asked for), "tolerance_used", "cap_used" (-1: none) and "stage"; "samples" <= budget."""
    who = "sample_map"
    budget = _budget_of(who, budget)
    if isinstance(state, (tuple, list)):
        return _sample_map_pair(who, state, stats, stream, params, budget)
    if not isinstance(state, Accumulation):
        raise TypeError("%s: state must be an Accumulation, got %s" % (who, type(state).__name__))
    p = sample_map_params(**params)
    state.check(who, state.size, state.seed, state.bucket_first, state.bucket_stride)
    if budget is not None and state.bucket_stride != 1:
        raise ValueError("%s: budget with a bucket share (bucket_stride %d): the map's totals are frame-wide, so a share cannot own a budget" % (who, state.bucket_stride))
    W, H = state.size
    count = state.count_plane()
    st = abi.Stats()
    b = abi.SampleBudget(budget=budget or 0)
    if not state.on_device:
        add = np.zeros((H, W), np.int32)
        if budget is None:
            _check(lib.frayhip_sample_map(W, H, _ptr(state.state), _ptr(count), C.byref(p), _ptr(add), C.byref(st)))
        else:
            _check(lib.frayhip_sample_map_budget(W, H, _ptr(state.state), None, _ptr(count), C.byref(p), C.byref(b), _ptr(add), C.byref(st)))
    else:
        with _DeviceCall(state.state.device, stream) as call:
            add = call.torch.zeros((H, W), dtype=call.torch.int32, device=state.state.device)
            if budget is None:
                _check(lib.frayhip_sample_map_device(W, H, _ptr(state.state), _ptr(count), C.byref(p), _ptr(add), call.handle, C.byref(st)))
            else:
                _check(lib.frayhip_sample_map_budget_device(W, H, _ptr(state.state), None, _ptr(count), C.byref(p), C.byref(b), _ptr(add), call.handle,
                                                            C.byref(st)))
    info = {"pixels": int(p.pixels), "samples": int(p.samples)}
    if budget is not None:
        _budget_info(info, b)
    if stats:
        info["stats"] = st.as_dict()
    return add, info


def _component_pair(who, state, size, seed, bucket_first, bucket_stride):
    """The checks of a pair (direct, indirect) of component states whose pixels may hold different numbers of samples (render_components' checks,
    but instead of uniform counts the two count planes must be equal).  Returns (direct, indirect, count plane of the direct state)."""
    if not (isinstance(state, (tuple, list)) and len(state) == 2 and all(isinstance(a, Accumulation) for a in state)):
        raise TypeError("%s: state must be a pair (direct, indirect) of Accumulations" % who)
    sd, si = state
    for a in (sd, si):
        a.check(who, size, seed, bucket_first, bucket_stride)
    if sd is si or sd.state is si.state:
        raise ValueError("%s: the direct and the indirect state are the same object" % who)
    if sd.on_device != si.on_device:
        raise ValueError("%s: one state is a numpy array and the other a GPU tensor" % who)
    if sd.on_device and sd.state.device != si.state.device:
        raise ValueError("%s: the states are on different devices" % who)
    cd, ci = sd.count_plane(), si.count_plane()
    if not bool((cd == ci).all()):
        raise ValueError("%s: the direct and the indirect state hold different numbers of samples in some pixel (the two count planes must be equal)" % who)
    return sd, si, cd


def _sample_map_pair(who, state, stats, stream, params, budget=None):
    """sample_map of a pair of component states (frayhip_sample_map_pair; under a budget frayhip_sample_map_budget with both states)."""
    if not (len(state) == 2 and all(isinstance(a, Accumulation) for a in state)):
        raise TypeError("%s: state must be an Accumulation or a pair (direct, indirect) of Accumulations" % who)
    p = sample_map_params(**params)
    sd, si, count = _component_pair(who, state, state[0].size, state[0].seed, state[0].bucket_first, state[0].bucket_stride)
    if budget is not None and sd.bucket_stride != 1:
        raise ValueError("%s: budget with a bucket share (bucket_stride %d): the map's totals are frame-wide, so a share cannot own a budget" % (who, sd.bucket_stride))
    W, H = sd.size
    st = abi.Stats()
    b = abi.SampleBudget(budget=budget or 0)
    if not sd.on_device:
        add = np.zeros((H, W), np.int32)
        if budget is None:
            _check(lib.frayhip_sample_map_pair(W, H, _ptr(sd.state), _ptr(si.state), _ptr(count), C.byref(p), _ptr(add), C.byref(st)))
        else:
            _check(lib.frayhip_sample_map_budget(W, H, _ptr(sd.state), _ptr(si.state), _ptr(count), C.byref(p), C.byref(b), _ptr(add), C.byref(st)))
    else:
        with _DeviceCall(sd.state.device, stream) as call:
            add = call.torch.zeros((H, W), dtype=call.torch.int32, device=sd.state.device)
            if budget is None:
                _check(lib.frayhip_sample_map_pair_device(W, H, _ptr(sd.state), _ptr(si.state), _ptr(count), C.byref(p), _ptr(add), call.handle, C.byref(st)))
            else:
                _check(lib.frayhip_sample_map_budget_device(W, H, _ptr(sd.state), _ptr(si.state), _ptr(count), C.byref(p), C.byref(b), _ptr(add), call.handle,
                                                            C.byref(st)))
    info = {"pixels": int(p.pixels), "samples": int(p.samples)}
    if budget is not None:
        _budget_info(info, b)
    if stats:
        info["stats"] = st.as_dict()
    return add, info


def temporal_accumulate(rgb, feat, prev_view=None, hist_in=None, stats=False, stream=None, motion=None, change=None, weight=None, units_in=None,
                        **params):
    """The temporal stage of include/frayhip.h (frayhip_temporal_accumulate): rgb [H, W, 3] and feat [H, W, 10] of the current frame, prev_view
    (view_from_camera of the previous frame's camera) and hist_in [H, W, 12] (the previous call's history), both None for the first frame;
    float32.  numpy arrays go through the host entry; torch tensors on the GPU through the device entry, on `stream` (None: the current
    stream).  params: see temporal_params.  Returns (hist_out [H, W, 12], signal [H, W, 3], variance [H, W]) of the inputs' kind -- signal and
    variance are denoise_signal's inputs -- and with stats=True also the stats dict (ms_total, ms_kernels).
    motion: the motion frame [H, W, 8] of Scene.render_features_motion, of the inputs' kind (a tensor's storage 16-byte aligned): the history is
    fetched where the pixel's surface point was before the scene's nodes moved (frayhip_temporal_accumulate_motion).  None: exactly the call
    above.
    change: a change frame [H, W] of the inputs' kind (change_frame): the history is shortened per pixel -- dropped where change >= 1, blended
    with a larger factor where it is > 0, taken as it is where it is 0 (frayhip_temporal_accumulate_adaptive, with or without motion).  None:
    exactly the calls above.
    weight: a weight plane [H, W] of the inputs' kind -- the units of the sequence's base sample count this frame gave each pixel (history_map) --
    with units_in [H, W], the previous call's units plane, given exactly when hist_in is (frayhip_temporal_accumulate_weighted, with or without
    motion and change): the blend factor comes from sample weight, w / U, while N keeps counting frames.  The call then returns (hist_out, units_out
    [H, W], signal, variance[, stats]).  None: exactly the calls and returns above."""
    p = temporal_params(**params)
    if (prev_view is None) != (hist_in is None):
        raise ValueError("temporal_accumulate: prev_view and hist_in must both be given or both be None")
    if prev_view is not None and not isinstance(prev_view, abi.View):
        raise TypeError("temporal_accumulate: prev_view must be an abi.View (view_from_camera), got %s" % type(prev_view).__name__)
    if weight is None and units_in is not None:
        raise ValueError("temporal_accumulate: units_in needs weight=")
    if weight is not None and (units_in is None) != (hist_in is None):
        raise ValueError("temporal_accumulate: with weight=, units_in and hist_in must both be given or both be None")
    named = [("rgb", rgb, 3), ("feat", feat, abi.FEAT_CHANNELS)] + ([("hist_in", hist_in, abi.HISTORY_CHANNELS)] if hist_in is not None else [])
    if motion is not None:
        named.append(("motion", motion, abi.MOTION_CHANNELS))
    if change is not None:
        named.append(("change", change, 0))
    if weight is not None:
        named.append(("weight", weight, 0))
        if units_in is not None:
            named.append(("units_in", units_in, 0))
    ins, (H, W), tensors = _frame_inputs("temporal_accumulate", named)
    hin = ins[2] if hist_in is not None else None
    uin = ins.pop() if units_in is not None else None
    wgt = ins.pop() if weight is not None else None
    chg = ins.pop() if change is not None else None
    mot = ins[-1] if motion is not None else None
    view = C.byref(prev_view) if prev_view is not None else None
    st = abi.Stats()
    if wgt is not None:
        if not tensors:
            hist, units, signal, var = (np.empty((H, W, abi.HISTORY_CHANNELS), np.float32), np.empty((H, W), np.float32), np.empty((H, W, 3), np.float32),
                                        np.empty((H, W), np.float32))
            _check(lib.frayhip_temporal_accumulate_weighted(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(mot), _ptr(chg), _ptr(wgt), view, _ptr(hin), _ptr(uin),
                                                            C.byref(p), _ptr(hist), _ptr(units), _ptr(signal), _ptr(var), C.byref(st)))
        else:
            with _DeviceCall(ins[0].device, stream) as call:
                new = lambda *shape: call.torch.empty(shape, dtype=call.torch.float32, device=ins[0].device)
                hist, units, signal, var = new(H, W, abi.HISTORY_CHANNELS), new(H, W), new(H, W, 3), new(H, W)
                _check(lib.frayhip_temporal_accumulate_weighted_device(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(mot), _ptr(chg), _ptr(wgt), view, _ptr(hin),
                                                                       _ptr(uin), C.byref(p), _ptr(hist), _ptr(units), _ptr(signal), _ptr(var), call.handle,
                                                                       C.byref(st)))
        return (hist, units, signal, var, st.as_dict()) if stats else (hist, units, signal, var)
    if not tensors:
        hist, signal, var = (np.empty((H, W, abi.HISTORY_CHANNELS), np.float32), np.empty((H, W, 3), np.float32), np.empty((H, W), np.float32))
        if chg is not None:
            _check(lib.frayhip_temporal_accumulate_adaptive(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(mot), _ptr(chg), view, _ptr(hin), C.byref(p),
                                                            hist.ctypes.data, signal.ctypes.data, var.ctypes.data, C.byref(st)))
        elif mot is not None:
            _check(lib.frayhip_temporal_accumulate_motion(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(mot), view, _ptr(hin), C.byref(p), hist.ctypes.data,
                                                          signal.ctypes.data, var.ctypes.data, C.byref(st)))
        else:
            _check(lib.frayhip_temporal_accumulate(W, H, _ptr(ins[0]), _ptr(ins[1]), view, _ptr(hin), C.byref(p), hist.ctypes.data, signal.ctypes.data,
                                                   var.ctypes.data, C.byref(st)))
    else:
        with _DeviceCall(ins[0].device, stream) as call:
            new = lambda *shape: call.torch.empty(shape, dtype=call.torch.float32, device=ins[0].device)
            hist, signal, var = new(H, W, abi.HISTORY_CHANNELS), new(H, W, 3), new(H, W)
            if chg is not None:
                _check(lib.frayhip_temporal_accumulate_adaptive_device(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(mot), _ptr(chg), view, _ptr(hin), C.byref(p),
                                                                       hist.data_ptr(), signal.data_ptr(), var.data_ptr(), call.handle, C.byref(st)))
            elif mot is not None:
                _check(lib.frayhip_temporal_accumulate_motion_device(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(mot), view, _ptr(hin), C.byref(p),
                                                                     hist.data_ptr(), signal.data_ptr(), var.data_ptr(), call.handle, C.byref(st)))
            else:
                _check(lib.frayhip_temporal_accumulate_device(W, H, _ptr(ins[0]), _ptr(ins[1]), view, _ptr(hin), C.byref(p), hist.data_ptr(),
                                                              signal.data_ptr(), var.data_ptr(), call.handle, C.byref(st)))
    return (hist, signal, var, st.as_dict()) if stats else (hist, signal, var)


def history_map(feat, prev_view=None, hist_in=None, units_in=None, motion=None, change=None, base=None, target=8, max_units=8, budget=None,
                held=False, stats=False, stream=None, **temporal_params_):
    """The history map of include/frayhip.h (frayhip_history_map): from the history that temporal_accumulate(weight=) will fetch for this view,
    how many samples each pixel gets this frame.  feat [H, W, 10]; prev_view, hist_in [H, W, 12] and units_in [H, W] all None (first frame) or
    all given; motion [H, W, 8] and change [H, W] or None, as temporal_accumulate takes them; float32, numpy arrays (host entry) or GPU torch
    tensors (device entry, on `stream`).  base: the samples a pixel with a full history gets (required); target: the units a pixel's history
    should amount to after this frame; max_units: the most units one frame gives a pixel; budget: None, or the most samples the plane may hold
    (an int >= base * W * H; the target is lowered until the plane fits).  **temporal_params_: the temporal_params fields of the accumulation
    that follows -- the map fetches with its tap tests and counts against its max_history.
    Returns (add, weight, info): add int32 [H, W] -- what Scene.render_samples_map takes -- weight float32 [H, W] -- what
    temporal_accumulate(weight=) takes -- and info {"target_used", "samples", "boosted", "budget"}, with "held" (the units each pixel's
    reprojected history holds, float32 [H, W]) when held=True and "stats" (ms_total, ms_kernels) when stats=True."""
    who = "history_map"
    p = temporal_params(**temporal_params_)
    if base is None:
        raise ValueError("%s: base must be given (it has no default)" % who)
    budget = _budget_of(who, budget)
    given = [x is not None for x in (prev_view, hist_in, units_in)]
    if any(given) and not all(given):
        raise ValueError("%s: prev_view, hist_in and units_in must all be given or all be None" % who)
    if prev_view is not None and not isinstance(prev_view, abi.View):
        raise TypeError("%s: prev_view must be an abi.View (view_from_camera), got %s" % (who, type(prev_view).__name__))
    named = [("feat", feat, abi.FEAT_CHANNELS)]
    if hist_in is not None:
        named += [("hist_in", hist_in, abi.HISTORY_CHANNELS), ("units_in", units_in, 0)]
    if motion is not None:
        named.append(("motion", motion, abi.MOTION_CHANNELS))
    if change is not None:
        named.append(("change", change, 0))
    ins, (H, W), tensors = _frame_inputs(who, named)
    chg = ins.pop() if change is not None else None
    mot = ins.pop() if motion is not None else None
    hin, uin = (ins[1], ins[2]) if hist_in is not None else (None, None)
    view = C.byref(prev_view) if prev_view is not None else None
    m = abi.HistoryMap()
    _check(lib.frayhip_history_map_defaults(C.byref(m)))
    m.base, m.target, m.max_units = int(base), int(target), int(max_units)
    if budget is not None:
        m.budget = budget
    st = abi.Stats()
    if not tensors:
        add, weight = np.zeros((H, W), np.int32), np.zeros((H, W), np.float32)
        hld = np.zeros((H, W), np.float32) if held else None
        _check(lib.frayhip_history_map(W, H, _ptr(ins[0]), _ptr(mot), _ptr(chg), view, _ptr(hin), _ptr(uin), C.byref(p), C.byref(m), _ptr(add), _ptr(weight),
                                       _ptr(hld), C.byref(st)))
    else:
        with _DeviceCall(ins[0].device, stream) as call:
            add = call.torch.zeros((H, W), dtype=call.torch.int32, device=ins[0].device)
            weight = call.torch.zeros((H, W), dtype=call.torch.float32, device=ins[0].device)
            hld = call.torch.zeros((H, W), dtype=call.torch.float32, device=ins[0].device) if held else None
            _check(lib.frayhip_history_map_device(W, H, _ptr(ins[0]), _ptr(mot), _ptr(chg), view, _ptr(hin), _ptr(uin), C.byref(p), C.byref(m), _ptr(add),
                                                  _ptr(weight), _ptr(hld), call.handle, C.byref(st)))
    info = {"target_used": int(m.target_used), "samples": int(m.samples), "boosted": int(m.boosted), "budget": budget}
    if held:
        info["held"] = hld
    if stats:
        info["stats"] = st.as_dict()
    return add, weight, info


_TEMPORAL_SHARED = ("demodulate", "film_offset", "plane_tolerance", "normal_min_dot")     # the fields that decide which taps count


def _split_params(who, direct, indirect, shared):
    """The two abi.Temporal of a split call: `shared` applied to both, then each component's own dict; the fields of _TEMPORAL_SHARED must come
    out equal bit for bit (ValueError)."""
    pd, pi = temporal_params(**dict(shared, **(direct or {}))), temporal_params(**dict(shared, **(indirect or {})))
    for k in _TEMPORAL_SHARED:
        a, b = getattr(pd, k), getattr(pi, k)
        if np.asarray(a).tobytes() != np.asarray(b).tobytes():
            raise ValueError("%s: direct and indirect must agree on %s (%r and %r): it decides which taps count" % (who, k, a, b))
    return pd, pi


def split_history_parts(hist):
    """The two ordinary histories inside a split history [H, W, 20] (numpy or torch): (direct [H, W, 12], indirect [H, W, 12]), each what
    temporal_accumulate takes as hist_in for that component.  Copies."""
    if hist.ndim != 3 or hist.shape[2] != abi.HISTORY_SPLIT_CHANNELS:
        raise ValueError("split_history_parts: hist must be shaped [H, W, %d], got %s" % (abi.HISTORY_SPLIT_CHANNELS, tuple(hist.shape)))
    if _torch_tensor(hist):
        import torch
        return hist[..., 0:12].contiguous(), torch.cat([hist[..., 12:16], hist[..., 4:7], hist[..., 16:17], hist[..., 8:11], hist[..., 17:18]], dim=2)
    return (np.ascontiguousarray(hist[..., 0:12]),
            np.concatenate([hist[..., 12:16], hist[..., 4:7], hist[..., 16:17], hist[..., 8:11], hist[..., 17:18]], axis=2))


def join_history_parts(hist_direct, hist_indirect):
    """split_history_parts' inverse: the split history [H, W, 20] of two ordinary histories of one frame.  ValueError when their position or
    normal columns differ in any bit (they are not histories of the same surface points)."""
    who = "join_history_parts"
    tensors = _torch_tensor(hist_direct)
    if tensors != _torch_tensor(hist_indirect):
        raise TypeError("%s: pass numpy arrays or torch tensors, not a mix" % who)
    for name, h in (("hist_direct", hist_direct), ("hist_indirect", hist_indirect)):
        if h.ndim != 3 or h.shape[2] != abi.HISTORY_CHANNELS:
            raise ValueError("%s: %s must be shaped [H, W, %d], got %s" % (who, name, abi.HISTORY_CHANNELS, tuple(h.shape)))
    if tuple(hist_direct.shape) != tuple(hist_indirect.shape):
        raise ValueError("%s: the parts' sizes differ: %s and %s" % (who, tuple(hist_direct.shape), tuple(hist_indirect.shape)))
    if tensors:
        import torch
        bits = lambda a: a.contiguous().view(torch.int32)
        cat = lambda parts: torch.cat(parts, dim=2)
        zeros = torch.zeros_like(hist_indirect[..., 0:2])
    else:
        if hist_direct.dtype != np.float32 or hist_indirect.dtype != np.float32:
            raise TypeError("%s: the parts must be float32" % who)
        bits = lambda a: np.ascontiguousarray(a).view(np.int32)
        cat = lambda parts: np.concatenate(parts, axis=2)
        zeros = np.zeros_like(hist_indirect[..., 0:2])
    for lo in (4, 8):
        if not bool((bits(hist_direct[..., lo:lo + 3]) == bits(hist_indirect[..., lo:lo + 3])).all()):
            raise ValueError("%s: the parts' %s columns differ" % (who, "position" if lo == 4 else "normal"))
    return cat([hist_direct, hist_indirect[..., 0:4], hist_indirect[..., 7:8], hist_indirect[..., 11:12], zeros])


def temporal_accumulate_split(rgb_direct, rgb_indirect, feat, prev_view=None, hist_in=None, motion=None, direct=None, indirect=None, stats=False,
                              stream=None, change_direct=None, change_indirect=None, **shared):
    """temporal_accumulate for a frame's direct and indirect light in one call (frayhip_temporal_accumulate_split): rgb_direct and rgb_indirect
    [H, W, 3] (Scene.render_components), feat [H, W, 10], prev_view and hist_in [H, W, 20] (the previous call's split history) both None for the
    first frame, motion [H, W, 8] or None as temporal_accumulate takes it; float32, numpy arrays (host entry) or GPU torch tensors (device
    entry, on `stream`).  direct, indirect: dicts of temporal_params fields for that component; **shared is applied to both.  The components may
    differ in max_history, variance_history and alpha_min; demodulate, film_offset, plane_tolerance and normal_min_dot must agree (ValueError).
    Returns (hist_out [H, W, 20], signal_direct, signal_indirect, variance_direct, variance_indirect[, stats]); each component's outputs are
    temporal_accumulate's for that component and its part of the history (split_history_parts), bit for bit.
    change_direct, change_indirect: both None (exactly the call above), or one change frame [H, W] per component, of the inputs' kind
    (change_frame; the same array may be passed for both): each component's history is shortened per pixel as temporal_accumulate(change=)
    shortens it, in one call on the split history (frayhip_temporal_accumulate_split_adaptive), and each component's outputs are
    temporal_accumulate(change=)'s for that component, bit for bit.  One of the two alone is a ValueError."""
    who = "temporal_accumulate_split"
    pd, pi = _split_params(who, direct, indirect, shared)
    if (change_direct is None) != (change_indirect is None):
        raise ValueError("%s: change_direct and change_indirect must both be given or both be None" % who)
    if (prev_view is None) != (hist_in is None):
        raise ValueError("%s: prev_view and hist_in must both be given or both be None" % who)
    if prev_view is not None and not isinstance(prev_view, abi.View):
        raise TypeError("%s: prev_view must be an abi.View (view_from_camera), got %s" % (who, type(prev_view).__name__))
    named = [("rgb_direct", rgb_direct, 3), ("rgb_indirect", rgb_indirect, 3), ("feat", feat, abi.FEAT_CHANNELS)]
    if hist_in is not None:
        named.append(("hist_in", hist_in, abi.HISTORY_SPLIT_CHANNELS))
    if motion is not None:
        named.append(("motion", motion, abi.MOTION_CHANNELS))
    if change_direct is not None:
        named += [("change_direct", change_direct, 0), ("change_indirect", change_indirect, 0)]
    ins, (H, W), tensors = _frame_inputs(who, named)
    hin = ins[3] if hist_in is not None else None
    chg_i, chg_d = (ins.pop(), ins.pop()) if change_direct is not None else (None, None)
    mot = ins[-1] if motion is not None else None
    view = C.byref(prev_view) if prev_view is not None else None
    st = abi.Stats()
    shapes = ((H, W, abi.HISTORY_SPLIT_CHANNELS), (H, W, 3), (H, W, 3), (H, W), (H, W))
    if not tensors:
        outs = tuple(np.empty(shape, np.float32) for shape in shapes)
        if chg_d is not None:
            _check(lib.frayhip_temporal_accumulate_split_adaptive(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(mot), _ptr(chg_d), _ptr(chg_i), view,
                                                                  _ptr(hin), C.byref(pd), C.byref(pi), *[_ptr(o) for o in outs], C.byref(st)))
        else:
            _check(lib.frayhip_temporal_accumulate_split(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(mot), view, _ptr(hin), C.byref(pd),
                                                         C.byref(pi), *[_ptr(o) for o in outs], C.byref(st)))
    else:
        with _DeviceCall(ins[0].device, stream) as call:
            outs = tuple(call.torch.empty(shape, dtype=call.torch.float32, device=ins[0].device) for shape in shapes)
            if chg_d is not None:
                _check(lib.frayhip_temporal_accumulate_split_adaptive_device(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(mot), _ptr(chg_d), _ptr(chg_i),
                                                                             view, _ptr(hin), C.byref(pd), C.byref(pi), *[_ptr(o) for o in outs], call.handle,
                                                                             C.byref(st)))
            else:
                _check(lib.frayhip_temporal_accumulate_split_device(W, H, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(mot), view, _ptr(hin), C.byref(pd),
                                                                    C.byref(pi), *[_ptr(o) for o in outs], call.handle, C.byref(st)))
    return outs + ((st.as_dict(),) if stats else ())


class Transform:
    """The reference's Transform (matrix.h:72-98) over the C helpers frayhip_transform_*: the parser's own arithmetic, so that
    Transform().scale(...).rotate(...).translate(...) in the order of a block's lines gives the bytes parseScene stores.  Starts as the identity,
    or as a copy of `init` (an abi.Transform, or a node / light, whose T is taken).  store(target) writes it to a node's or a light's T (or to an
    abi.Transform); a rect light's center and area are then light_begin_frame's to refresh."""

    def __init__(self, init=None):
        self.T = abi.Transform()
        if init is None:
            _check(lib.frayhip_transform_identity(C.byref(self.T)))
        else:
            C.memmove(C.byref(self.T), C.byref(getattr(init, "T", init)), C.sizeof(abi.Transform))

    def scale(self, x, y, z):
        _check(lib.frayhip_transform_scale(C.byref(self.T), float(x), float(y), float(z)))
        return self

    def rotate(self, yaw, pitch, roll):
        _check(lib.frayhip_transform_rotate(C.byref(self.T), float(yaw), float(pitch), float(roll)))
        return self

    def translate(self, x, y, z):
        _check(lib.frayhip_transform_translate(C.byref(self.T), float(x), float(y), float(z)))
        return self

    def store(self, target):
        dst = target if isinstance(target, abi.Transform) else target.T
        C.memmove(C.byref(dst), C.byref(self.T), C.sizeof(abi.Transform))
        return target


def light_begin_frame(light):
    """RectLight::beginFrame on an abi.Light (Scene.lights[i]): center and area from its T (frayhip_light_begin_frame).  Returns the light."""
    _check(lib.frayhip_light_begin_frame(C.byref(light)))
    return light


def shader_begin_frame(shader):
    """Reflection::beginFrame on an abi.Shader (Scene.shaders[i]): deflectionScaling from its glossiness (frayhip_shader_begin_frame)."""
    _check(lib.frayhip_shader_begin_frame(C.byref(shader)))
    return shader


class Accumulation:
    """The state of a resumable frame (include/frayhip.h "resumable frames"): `state`, float32 [H, W, 4] -- per pixel the FP32 sum of its samples'
    colours and the second moment of their luminance -- as a numpy array (Scene.render_samples then goes through the host entry) or a torch tensor
    on the GPU (the device entry); `samples_done`, the samples per pixel it holds; and what it belongs to: `seed`, `size` (W, H) and the bucket
    share (`bucket_first`, `bucket_stride`) that was rendered into it.  The scene, its view and its settings are the caller's to keep unchanged.
    `counts`: None while every pixel holds `samples_done` samples; after Scene.render_samples_map has given the pixels different numbers, the int32
    [H, W] plane (of the state's kind) of how many each one holds, and samples_done is then the smallest of them."""

    def __init__(self, state, samples_done=0, seed=42, size=None, bucket_first=0, bucket_stride=1, counts=None):
        self.state = state
        self.counts = counts
        self.samples_done = int(samples_done)
        self.seed = int(seed) & 0xffffffff
        self.size = (int(size[0]), int(size[1])) if size is not None else (int(state.shape[1]), int(state.shape[0]))
        self.bucket_first, self.bucket_stride = int(bucket_first), int(bucket_stride)

    @classmethod
    def empty(cls, size, seed=42, bucket_first=0, bucket_stride=1, device=None):
        """A state of no samples for a W x H frame: a numpy array, or with `device` a torch tensor there."""
        W, H = int(size[0]), int(size[1])
        if device is None:
            state = np.zeros((H, W, abi.ACCUM_CHANNELS), np.float32)
        else:
            import torch
            state = torch.zeros((H, W, abi.ACCUM_CHANNELS), dtype=torch.float32, device=device)
        return cls(state, 0, seed, (W, H), bucket_first, bucket_stride)

    @property
    def on_device(self):
        return _torch_tensor(self.state)

    def check(self, who, size, seed, bucket_first, bucket_stride):
        """ValueError unless the state is a well-formed one of this size, seed and bucket share."""
        W, H = size
        if self.size != (W, H):
            raise ValueError("%s: the state belongs to a %d x %d frame, the scene renders %d x %d" % ((who,) + self.size + (W, H)))
        if self.seed != (int(seed) & 0xffffffff):
            raise ValueError("%s: the state was rendered with seed %d, the call asks for seed %d" % (who, self.seed, int(seed) & 0xffffffff))
        if (self.bucket_first, self.bucket_stride) != (int(bucket_first), int(bucket_stride)):
            raise ValueError("%s: the state holds the bucket share (first %d, stride %d), the call asks for (first %d, stride %d)"
                             % (who, self.bucket_first, self.bucket_stride, bucket_first, bucket_stride))
        if self.samples_done < 0:
            raise ValueError("%s: the state's samples_done is negative" % who)
        st = self.state
        if self.on_device:
            import torch
            ok = st.is_cuda and st.dtype == torch.float32 and st.is_contiguous()
        else:
            ok = isinstance(st, np.ndarray) and st.dtype == np.float32 and st.flags.c_contiguous and st.flags.writeable
        if not ok or tuple(st.shape) != (H, W, abi.ACCUM_CHANNELS):
            raise ValueError("%s: the state must be a contiguous float32 numpy array or GPU torch tensor shaped %s" % (who, (H, W, abi.ACCUM_CHANNELS)))
        ct = self.counts
        if ct is not None:
            if self.on_device:
                ok = _torch_tensor(ct) and ct.is_cuda and ct.dtype == torch.int32 and ct.is_contiguous() and ct.device == st.device
            else:
                ok = isinstance(ct, np.ndarray) and ct.dtype == np.int32 and ct.flags.c_contiguous and ct.flags.writeable
            if not ok or tuple(ct.shape) != (H, W):
                raise ValueError("%s: the state's counts must be a contiguous int32 plane of the state's kind shaped %s" % (who, (H, W)))

    def count_plane(self):
        """The per-pixel sample counts as an int32 [H, W] plane of the state's kind: `counts`, or a new plane of samples_done everywhere."""
        if self.counts is not None:
            return self.counts
        W, H = self.size
        if self.on_device:
            import torch
            return torch.full((H, W), self.samples_done, dtype=torch.int32, device=self.state.device)
        return np.full((H, W), self.samples_done, np.int32)

    def require_uniform(self, who):
        """For the calls that add the same number of samples to every pixel: a counts plane that holds one value collapses back to samples_done;
        one that does not is refused (ValueError)."""
        if self.counts is None:
            return
        lo, hi = int(self.counts.min()), int(self.counts.max())
        if lo != hi:
            raise ValueError("%s: the state's pixels hold different numbers of samples (%d .. %d, Scene.render_samples_map); only "
                             "render_samples_map can continue it" % (who, lo, hi))
        self.samples_done, self.counts = lo, None

    def save(self, path):
        """Writes the state in .npz format to `path` as it is given (a tensor is copied to the host); load() reads it back as a numpy state.
        Returns the path."""
        path = os.fspath(path)
        arr = self.state.cpu().numpy() if self.on_device else self.state
        extra = {}
        if self.counts is not None:          # only a state with per-pixel counts carries the plane: files of uniform states stay as they were
            extra["counts"] = self.counts.cpu().numpy() if self.on_device else self.counts
        with open(path, "wb") as f:
            np.savez(f, state=arr, samples_done=np.int64(self.samples_done), seed=np.uint32(self.seed), size=np.array(self.size, np.int64),
                     share=np.array([self.bucket_first, self.bucket_stride], np.int64), **extra)
        return path

    @classmethod
    def load(cls, path):
        with np.load(os.fspath(path)) as z:
            missing = [k for k in ("state", "samples_done", "seed", "size", "share") if k not in z.files]
            if missing:
                raise ValueError("Accumulation.load: %s is not a saved state (no %s)" % (path, ", ".join(missing)))
            state = np.ascontiguousarray(z["state"], dtype=np.float32)
            counts = np.ascontiguousarray(z["counts"], dtype=np.int32) if "counts" in z.files else None
            return cls(state, int(z["samples_done"]), int(z["seed"]), tuple(int(v) for v in z["size"]), int(z["share"][0]), int(z["share"][1]),
                       counts)


class Scene:
    """`Scene scene` of the reference (scene.h:280-299).

    parseScene()  -> Scene::parseScene + the beginRender work that needs no GPU (KD build)
    settings / camera -> mutable GlobalSettings / Camera records, edited before beginRender() the way
                     the reference's callers edit scene.settings.* after parsing
    beginRender() -> uploads the flattened scene to the current GPU
    render()      -> render() (main.cpp:373): returns vfb as float32 [H, W, 3]
    """

    def __init__(self):
        self._hs = C.c_void_p()
        self._dev = C.c_void_p()
        self.desc = None

    @classmethod
    def parseScene(cls, path):
        s = cls()
        _check(lib.frayhip_scene_parse(os.fspath(path).encode(), C.byref(s._hs)))
        s.desc = lib.frayhip_host_scene_desc(s._hs).contents
        return s

    @property
    def settings(self):
        return self.desc.settings

    @property
    def camera(self):
        return self.desc.camera

    def _table(self, name, rec):
        """A mutable ctypes view of one of the host scene's tables: edits land in self.desc's arrays, and update() pushes them."""
        n = getattr(self.desc, "n_" + name)
        return C.cast(getattr(self.desc, name), P(rec * n)).contents if n else (rec * 0)()

    nodes = property(lambda self: self._table("nodes", abi.Node), doc="desc.nodes[] as a mutable array of abi.Node")
    lights = property(lambda self: self._table("lights", abi.Light), doc="desc.lights[] (abi.Light)")
    shaders = property(lambda self: self._table("shaders", abi.Shader), doc="desc.shaders[] (abi.Shader)")
    layers = property(lambda self: self._table("layers", abi.Layer), doc="desc.layers[] (abi.Layer)")
    textures = property(lambda self: self._table("textures", abi.Texture), doc="desc.textures[] (abi.Texture): color1, color2, scaling, bumpIntensity and ior are editable")
    spheres = property(lambda self: self._table("spheres", abi.Sphere), doc="desc.spheres[] (abi.Sphere)")
    planes = property(lambda self: self._table("planes", abi.Plane), doc="desc.planes[] (abi.Plane)")
    cubes = property(lambda self: self._table("cubes", abi.Cube), doc="desc.cubes[] (abi.Cube)")

    @property
    def frame_size(self):
        return self.desc.settings.frameWidth, self.desc.settings.frameHeight

    def samples_per_pixel(self):
        """main.cpp:395-400"""
        spp = 5 if self.settings.wantAA else 1
        if self.camera.dof:
            spp = max(spp, self.camera.numDOFSamples)
        if self.settings.gi:
            spp = max(spp, self.settings.numPaths)
        return spp

    def beginRender(self, device=None):
        if device is not None:
            _check(lib.frayhip_init(int(device)))
        self.endRender()
        _check(lib.frayhip_scene_create(C.byref(self.desc), C.byref(self._dev)))
        return self

    def beginFrame(self):
        """Pushes the current settings / camera records to the uploaded scene (Scene::beginFrame: the
        reference re-derives the camera every frame, so callers may move it between render() calls)."""
        self._need_dev()
        _check(lib.frayhip_scene_set_view(self._dev, C.byref(self.desc.camera), C.byref(self.desc.settings)))
        return self

    def update(self):
        """Pushes the editable tables of self.desc -- nodes, planes, spheres, cubes, shaders, layers, lights and the textures' parameters, as edited
        through the views above -- to the uploaded scene (frayhip_scene_update): the handle then renders and answers queries exactly as one
        created from the edited description would, and keeps its workspace, options and seed table.  The camera and the settings stay
        beginFrame()'s."""
        self._need_dev()
        _check(lib.frayhip_scene_update(self._dev, C.byref(self.desc)))
        return self

    def endRender(self):
        if self._dev:
            lib.frayhip_scene_destroy(self._dev)
            self._dev = C.c_void_p()

    def set_option(self, name, value):
        """frayhip_scene_set_option: "pt_lanes" (1..4 batches in flight), "pt_budget_mib" (queue memory), "speculate_fans" (0 / 1), "fused_whitted_max" (0..1024: the light samples per hit
        up to which a Whitted frame without recursive shaders and KD meshes runs the fused shade kernel), "fp_contract" (0 / 1: relaxed arithmetic
        for path-traced rays after a sample's first closest hit, include/frayhip.h), "skip_null_segments" (0 / 1: next-event samples that are black by bit pattern are not traced),
        "segment_planes" (0 / 1: the path tracer's any-hit kernel skips, per wave, the small untransformed meshes whose triangles' planes no next-event segment of the wave crosses),
        "certified_segments" (0 / 1: in a scene of such meshes and exactly gated ones only, the bounce kernel stores the term of a next-event segment proven unoccluded itself, without a query),
        "seed_table_mib" (cap of the table that keeps the samples' seeding words across frames of one seed, size and bucket share; 0 = off)."""
        self._need_dev()
        _check(lib.frayhip_scene_set_option(self._dev, name.encode(), int(value)))
        return self

    def tight_gates(self, enable=None):
        """frayhip_scene_tight_gates: switches tight gates on or off (None leaves the switch alone) and returns (enabled, eligible gates): the path tracer
        tests a gated mesh that is eligible by the box of its own triangles and a guard against rays nearly parallel to a face, not by its bounding box."""
        self._need_dev()
        on, n = C.c_int64(0), C.c_int64(0)
        _check(lib.frayhip_scene_tight_gates(self._dev, -1 if enable is None else int(bool(enable)), C.byref(on), C.byref(n)))
        return int(on.value), int(n.value)

    def camera_skip(self, enable=None):
        """frayhip_scene_camera_skip: switches the first bounce's shortcut on or off (None leaves the switch alone) and returns (enabled, miss records, the last
        frame's skipped (wave, node) pairs, its first-bounce wave iterations): a wave of camera rays leaves out the eligible meshes all its rays provably miss."""
        self._need_dev()
        on, n, skipped, waves = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(lib.frayhip_scene_camera_skip(self._dev, -1 if enable is None else int(bool(enable)), C.byref(on), C.byref(n), C.byref(skipped), C.byref(waves)))
        return int(on.value), int(n.value), int(skipped.value), int(waves.value)

    def camera_tiles(self, enable=None):
        """frayhip_scene_camera_tiles: switches the first bounce's tile table on or off (None leaves the switch alone) and returns the switch: a first-bounce wave
        reads its tile's pixel origin and the meshes no camera ray of the tile can hit from a table made once per frame."""
        self._need_dev()
        on = C.c_int64(0)
        _check(lib.frayhip_scene_camera_tiles(self._dev, -1 if enable is None else int(bool(enable)), C.byref(on)))
        return int(on.value)

    def shade_shortcuts(self, enable=None):
        """frayhip_scene_shade_shortcuts: switches the shading shortcuts on or off (None leaves the switch alone) and returns (enabled, eligible): bit 0 of eligible --
        every node is an untransformed flat mesh, shaded without its transform and with a stored world normal; bit 1 -- every light is an axis-scaled RectLight."""
        self._need_dev()
        on, el = C.c_int64(0), C.c_int64(0)
        _check(lib.frayhip_scene_shade_shortcuts(self._dev, -1 if enable is None else int(bool(enable)), C.byref(on), C.byref(el)))
        return int(on.value), int(el.value)

    def get_option(self, name):
        """frayhip_scene_get_option: an option's value, or a figure of the last frame ("fans_filed", "fan_children", "fan_children_looked_up", "fans_given_up", "contracted_launches", "shadow_segments",
        "shadow_segments_certified", "certified_segments_eligible", "segment_plane_nodes", "shadow_nodes_skipped", "seed_table_bytes", "seed_launches", "seed_planes_reused", "batch_lanes")."""
        self._need_dev()
        v = C.c_int64(0)
        _check(lib.frayhip_scene_get_option(self._dev, name.encode(), C.byref(v)))
        return int(v.value)

    def _frame(self, mode, seed, bucket_first, bucket_stride, spp_chunk, stats):
        return abi.Frame(mode=mode, seed=seed, bucket_first=bucket_first, bucket_stride=bucket_stride,
                         spp_chunk=spp_chunk, flags=abi.FRAME_STATS if stats else 0)

    def _need_dev(self):
        if not self._dev:
            raise FrayError(abi.E_ARG, "Scene.beginRender() has not been called")

    def render(self, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, stats=False, out=None, progress=None, preview_ms=-1):
        """Full render; returns (vfb, stats dict).

        progress(info): called after batches of the frame (frayhip_render_progressive, include/frayhip.h): info holds samples_done,
        samples_total, batches_done, batches_total, ms_elapsed, preview and final; when info["preview"] is set, info["image"] is a
        float32 [H, W, 3] view of the frame's running mean, valid during the call only.  preview_ms < 0: no previews, 0: one per batch,
        > 0: at most one per that many milliseconds.  A truthy return cancels the frame; so does an exception, which is raised again
        once the call has returned.  With a progress callback the stats dict also holds "samples_done" and "cancelled": a cancelled
        frame is returned, not raised -- vfb is the exact frame of its samples_done samples per pixel."""
        self._need_dev()
        W, H = self.frame_size
        rgb = out if out is not None else np.zeros((H, W, 3), np.float32)
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, seed, bucket_first, bucket_stride, spp_chunk, stats)
        if progress is None:
            _check(lib.frayhip_render(self._dev, C.byref(fr), rgb.ctypes.data, None, None, C.byref(st)))
            return rgb, st.as_dict()
        req, run = _progress_request(progress, preview_ms, lambda p: {"image": np.ctypeslib.as_array(p.rgb, shape=(H, W, 3))})
        rc = lib.frayhip_render_progressive(self._dev, C.byref(fr), C.byref(req), rgb.ctypes.data, None, None, C.byref(st))
        return rgb, run.finish(rc, st)

    def primary_hits(self, bucket_first=0, bucket_stride=1, stats=False):
        """Closest hit of the camera ray through every integer pixel: (ids int32 [H,W], dist f64 [H,W], stats)."""
        self._need_dev()
        W, H = self.frame_size
        ids = np.full((H, W), -9, np.int32)
        dist = np.zeros((H, W), np.float64)
        st = abi.Stats()
        fr = self._frame(abi.MODE_PRIMARY_ID, 0, bucket_first, bucket_stride, 0, stats)
        _check(lib.frayhip_render(self._dev, C.byref(fr), None, ids.ctypes.data, dist.ctypes.data, C.byref(st)))
        return ids, dist, st.as_dict()

    def render_device(self, d_rgb_ptr, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, stats=False,
                      stream=None, mode=abi.MODE_RENDER, d_id_ptr=None, d_dist_ptr=None, progress=None, preview_ms=-1):
        """Render into caller-owned device memory (e.g. torch tensors' data_ptr()).  progress / preview_ms as in render(); a preview's
        info["d_rgb"] is the device address of the frame (d_rgb_ptr), complete when the callback runs."""
        self._need_dev()
        st = abi.Stats()
        fr = self._frame(mode, seed, bucket_first, bucket_stride, spp_chunk, stats)
        if progress is None:
            _check(lib.frayhip_render_device(self._dev, C.byref(fr), d_rgb_ptr, d_id_ptr, d_dist_ptr, stream, C.byref(st)))
            return st.as_dict()
        req, run = _progress_request(progress, preview_ms, lambda p: {"d_rgb": C.cast(p.rgb, C.c_void_p).value})
        rc = lib.frayhip_render_device_progressive(self._dev, C.byref(fr), C.byref(req), d_rgb_ptr, d_id_ptr, d_dist_ptr, stream, C.byref(st))
        return run.finish(rc, st)

    # ---- ray queries (include/frayhip.h): numpy arrays through the host entries, torch tensors on the GPU through the device entries ----
    def camera_rays(self, xy=None, eye=0, stream=None):
        """Camera::getScreenRay(x, y, eye) of the current view (eye 0 = CENTER, 1 = LEFT, 2 = RIGHT): (origin, dir).  xy None: every integer
        pixel, shaped [H, W, 3] (the rays of primary_hits(), bit for bit); else film positions [..., 2] float64 -> [..., 3]."""
        self._need_dev()
        if xy is None:
            W, H = self.frame_size
            org, dirs = np.empty((H, W, 3)), np.empty((H, W, 3))
            _check(lib.frayhip_camera_rays(self._dev, W * H, None, int(eye), org.ctypes.data, dirs.ctypes.data))
            return org, dirs
        (xy,), shape, device = _query_inputs([("xy", xy)], 2)
        n = int(np.prod(shape, dtype=np.int64))
        if device is None:
            xy = np.ascontiguousarray(xy)
            org, dirs = np.empty(shape + (3,)), np.empty(shape + (3,))
            _check(lib.frayhip_camera_rays(self._dev, n, xy.ctypes.data, int(eye), org.ctypes.data, dirs.ctypes.data))
            return org, dirs
        with _DeviceCall(device, stream) as call:
            torch = call.torch
            xy = xy.contiguous()
            org = torch.empty(shape + (3,), dtype=torch.float64, device=device)
            dirs = torch.empty(shape + (3,), dtype=torch.float64, device=device)
            if n:                                   # (an empty tensor's data_ptr() is 0: nothing to call)
                _check(lib.frayhip_camera_rays_device(self._dev, n, xy.data_ptr(), int(eye), org.data_ptr(), dirs.data_ptr(), call.handle))
        return org, dirs

    def trace_rays(self, origin, dir, record=False, stats=False, stream=None):
        """The reference's closestHit for rays origin / dir [..., 3] float64: {"hit_id" (int32, -1 miss, -2-i light i), "hit_dist" (1e99 on a miss),
        "hit_rec" (only with record: [..., 9] = dist, ip, norm, u, v), "stats"}."""
        self._need_dev()
        (o, d), shape, device = _query_inputs([("origin", origin), ("dir", dir)])
        n = int(np.prod(shape, dtype=np.int64))
        st = abi.Stats()
        flags = abi.FRAME_STATS if stats else 0
        if device is None:
            o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
            ids, dist = np.empty(shape, np.int32), np.empty(shape, np.float64)
            rec = np.empty(shape + (9,), np.float64) if record else None
            _check(lib.frayhip_trace_rays(self._dev, n, o.ctypes.data, d.ctypes.data, flags, ids.ctypes.data, dist.ctypes.data,
                                          rec.ctypes.data if record else None, C.byref(st)))
        else:
            with _DeviceCall(device, stream) as call:
                torch = call.torch
                o, d = o.contiguous(), d.contiguous()
                ids = torch.empty(shape, dtype=torch.int32, device=device)
                dist = torch.empty(shape, dtype=torch.float64, device=device)
                rec = torch.empty(shape + (9,), dtype=torch.float64, device=device) if record else None
                if n:                                   # (an empty tensor's data_ptr() is 0: nothing to call)
                    _check(lib.frayhip_trace_rays_device(self._dev, n, o.data_ptr(), d.data_ptr(), flags, ids.data_ptr(), dist.data_ptr(),
                                                         rec.data_ptr() if record else None, call.handle, C.byref(st)))
        out = {"hit_id": ids, "hit_dist": dist, "stats": st.as_dict()}
        if record:
            out["hit_rec"] = rec
        return out

    def visible(self, a, b, stats=False, stream=None):
        """visible(a, b) (main.cpp:64-80) for segments a -> b [..., 3] float64: (vis, stats), vis a bool array / tensor [...]."""
        self._need_dev()
        (a, b), shape, device = _query_inputs([("a", a), ("b", b)])
        n = int(np.prod(shape, dtype=np.int64))
        st = abi.Stats()
        flags = abi.FRAME_STATS if stats else 0
        if device is None:
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            vis = np.empty(shape, np.bool_)
            _check(lib.frayhip_visible(self._dev, n, a.ctypes.data, b.ctypes.data, flags, vis.ctypes.data, C.byref(st)))
        else:
            with _DeviceCall(device, stream) as call:
                torch = call.torch
                a, b = a.contiguous(), b.contiguous()
                vis = torch.empty(shape, dtype=torch.bool, device=device)       # one byte per element: the entry's uint8 output
                if n:                                   # (an empty tensor's data_ptr() is 0: nothing to call)
                    _check(lib.frayhip_visible_device(self._dev, n, a.data_ptr(), b.data_ptr(), flags, vis.data_ptr(), call.handle, C.byref(st)))
        return vis, st.as_dict()

    def shade_rays(self, origin, dir, spp=1, seed=42, sample_first=0, rng_skip=0, keys=None, stats=False, stream=None):
        """trace(ray, rnd) (main.cpp:286-293) for rays origin / dir [..., 3] float64: the mean colour of samples sample_first .. sample_first + spp - 1
        of each ray under the scene's integrator, float32 [..., 3] (include/frayhip.h, radiance queries).  keys: uint32 [...], the generator key of
        each ray (None: its flat index).  numpy arrays go through the host entry, GPU torch tensors through the device entry on `stream` (default:
        the current one).  With stats=True returns (rgb, stats)."""
        self._need_dev()
        (o, d), shape, device = _query_inputs([("origin", origin), ("dir", dir)])
        n = int(np.prod(shape, dtype=np.int64))
        st = abi.Stats()
        req = abi.ShadeRequest(seed=int(seed) & 0xffffffff, spp=int(spp), sample_first=int(sample_first), rng_skip=int(rng_skip),
                               flags=abi.FRAME_STATS if stats else 0, keys=None)
        if device is None:
            o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
            if keys is not None:
                keys = np.ascontiguousarray(keys, dtype=np.uint32)
                if keys.shape != shape:
                    raise ValueError("shade_rays: keys must be shaped %s, got %s" % (shape, keys.shape))
                req.keys = keys.ctypes.data
            rgb = np.empty(shape + (3,), np.float32)
            _check(lib.frayhip_shade_rays(self._dev, n, o.ctypes.data, d.ctypes.data, C.byref(req), rgb.ctypes.data, C.byref(st)))
        else:
            with _DeviceCall(device, stream) as call:
                torch = call.torch
                o, d = o.contiguous(), d.contiguous()
                if keys is not None:
                    if not _torch_tensor(keys) or keys.device != device:
                        raise TypeError("shade_rays: keys must be a tensor on the rays' device")
                    if tuple(keys.shape) != shape:
                        raise ValueError("shade_rays: keys must be shaped %s, got %s" % (shape, tuple(keys.shape)))
                    if keys.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                        raise TypeError("shade_rays: keys must be int32 / uint32, got %s" % keys.dtype)
                    keys = keys.contiguous()
                    req.keys = keys.data_ptr() if n else None
                rgb = torch.empty(shape + (3,), dtype=torch.float32, device=device)
                if n:                                   # (an empty tensor's data_ptr() is 0: nothing to call)
                    _check(lib.frayhip_shade_rays_device(self._dev, n, o.data_ptr(), d.data_ptr(), C.byref(req), rgb.data_ptr(), call.handle, C.byref(st)))
        return (rgb, st.as_dict()) if stats else rgb

    # ---- resumable frames (include/frayhip.h "resumable frames") ----
    def render_samples(self, count, state=None, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, stats=False, progress=None, preview_ms=-1,
                       noise=False, stream=None):
        """Adds `count` samples per pixel to a frame (frayhip_render_samples): samples state.samples_done .. state.samples_done + count - 1 of the
        call's buckets, under the scene's current view and settings; the frame's own sample count plays no part.  state: an Accumulation, or
        None to start one (a numpy state).  A numpy state goes through the host entry and a state on the GPU through the device entry, on
        `stream` (None: the current stream); rgb and noise are of the state's kind.

        Returns (rgb, state[, noise][, stats]): rgb float32 [H, W, 3] is the mean of all samples the state holds -- after samples 0 .. N-1 it is
        render() with N samples per pixel, bit for bit -- and `state` is the one given, updated in place.  noise=True adds the variance estimate
        of the mean's luminance, float32 [H, W] (denoise_signal's variance, with demodulate=0).  The stats dict follows with stats=True or a
        progress callback.  progress / preview_ms: as render(); previews show the running mean of all samples so far (info["image"], or
        info["d_rgb"] for a state on the GPU), and samples_done counts from sample 0.  A cancelled call returns normally, with
        stats["cancelled"] set and state.samples_done at the samples resolved; the next call continues from there.
        A state of another seed, size or bucket share is refused (ValueError)."""
        who = "render_samples"
        count = int(count)
        if count < 1:
            raise ValueError("%s: count must be >= 1, got %d" % (who, count))
        W, H = self.frame_size
        if state is None:
            state = Accumulation.empty((W, H), seed, bucket_first, bucket_stride)
        elif not isinstance(state, Accumulation):
            raise TypeError("%s: state must be an Accumulation, got %s" % (who, type(state).__name__))
        state.check(who, (W, H), seed, bucket_first, bucket_stride)
        state.require_uniform(who)
        self._need_dev()
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, state.seed, bucket_first, bucket_stride, spp_chunk, stats)
        req = abi.Samples(sample_first=state.samples_done, sample_count=count)
        preq, run = None, None
        if not state.on_device:
            rgb = np.zeros((H, W, 3), np.float32)
            var = np.zeros((H, W), np.float32) if noise else None
            if progress is not None:
                preq, run = _progress_request(progress, preview_ms, lambda p: {"image": np.ctypeslib.as_array(p.rgb, shape=(H, W, 3))})
            rc = lib.frayhip_render_samples(self._dev, C.byref(fr), C.byref(req), C.byref(preq) if preq is not None else None, _ptr(state.state),
                                            _ptr(rgb), _ptr(var), C.byref(st))
        else:
            with _DeviceCall(state.state.device, stream) as call:
                rgb = call.torch.zeros((H, W, 3), dtype=call.torch.float32, device=state.state.device)
                var = call.torch.zeros((H, W), dtype=call.torch.float32, device=state.state.device) if noise else None
                if progress is not None:
                    preq, run = _progress_request(progress, preview_ms, lambda p: {"d_rgb": C.cast(p.rgb, C.c_void_p).value})
                rc = lib.frayhip_render_samples_device(self._dev, C.byref(fr), C.byref(req), C.byref(preq) if preq is not None else None,
                                                       _ptr(state.state), _ptr(rgb), _ptr(var), call.handle, C.byref(st))
        if rc in (abi.OK, abi.E_CANCELLED):
            state.samples_done = req.samples_done
        if run is not None:
            info = run.finish(rc, st)
            info["samples_done"] = state.samples_done
        else:
            _check(rc)
            info = st.as_dict()
        out = (rgb, state) + ((var,) if noise else ())
        return out + ((info,) if (stats or progress is not None) else ())

    # ---- component frames (include/frayhip.h "component frames") ----
    def render_components(self, count, state=None, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, stats=False, progress=None, noise=False,
                          stream=None):
        """render_samples with direct and indirect light kept apart (frayhip_render_components; mono path-traced frames): `count` more samples per
        pixel into a pair of states, state = (direct, indirect), two Accumulations of one kind (numpy: the host entry; GPU tensors: the device
        entry, on `stream`), or None to start a numpy pair.  A sample's direct light is its path's first term, its indirect light the fold of the
        others, and direct + indirect is render_samples' sample colour in one FP32 addition, bit for bit.

        Returns (direct_rgb, indirect_rgb, state[, noise_direct, noise_indirect][, stats]): each rgb float32 [H, W, 3] is the mean of its
        component over all samples the states hold, `state` is the pair given, updated in place, and noise=True adds each component's variance
        estimate, float32 [H, W] (denoise_signal's variance, with demodulate=0).  The stats dict follows with stats=True or a progress callback.
        progress: as render_samples, but no previews are offered.  A cancelled call returns normally with stats["cancelled"] set and both states
        at the samples resolved.  ValueError when the two states disagree in seed, size, share, kind or samples_done, or belong to another
        frame."""
        who = "render_components"
        count = int(count)
        if count < 1:
            raise ValueError("%s: count must be >= 1, got %d" % (who, count))
        W, H = self.frame_size
        if state is None:
            state = (Accumulation.empty((W, H), seed, bucket_first, bucket_stride), Accumulation.empty((W, H), seed, bucket_first, bucket_stride))
        elif not (isinstance(state, (tuple, list)) and len(state) == 2 and all(isinstance(a, Accumulation) for a in state)):
            raise TypeError("%s: state must be a pair (direct, indirect) of Accumulations" % who)
        sd, si = state
        for a in (sd, si):
            a.check(who, (W, H), seed, bucket_first, bucket_stride)
            a.require_uniform(who)
        if sd is si or sd.state is si.state:
            raise ValueError("%s: the direct and the indirect state are the same object" % who)
        if sd.on_device != si.on_device:
            raise ValueError("%s: one state is a numpy array and the other a GPU tensor" % who)
        if sd.on_device and sd.state.device != si.state.device:
            raise ValueError("%s: the states are on different devices" % who)
        if sd.samples_done != si.samples_done:
            raise ValueError("%s: the direct state holds %d samples per pixel, the indirect state %d" % (who, sd.samples_done, si.samples_done))
        self._need_dev()
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, sd.seed, bucket_first, bucket_stride, spp_chunk, stats)
        req = abi.Samples(sample_first=sd.samples_done, sample_count=count)
        preq, run = None, None
        if progress is not None:
            preq, run = _progress_request(progress, -1, lambda p: {})
        pp = C.byref(preq) if preq is not None else None
        if not sd.on_device:
            rgb = [np.zeros((H, W, 3), np.float32) for _ in range(2)]
            var = [np.zeros((H, W), np.float32) if noise else None for _ in range(2)]
            rc = lib.frayhip_render_components(self._dev, C.byref(fr), C.byref(req), pp, _ptr(sd.state), _ptr(si.state), _ptr(rgb[0]), _ptr(rgb[1]),
                                               _ptr(var[0]), _ptr(var[1]), C.byref(st))
        else:
            with _DeviceCall(sd.state.device, stream) as call:
                rgb = [call.torch.zeros((H, W, 3), dtype=call.torch.float32, device=sd.state.device) for _ in range(2)]
                var = [call.torch.zeros((H, W), dtype=call.torch.float32, device=sd.state.device) if noise else None for _ in range(2)]
                rc = lib.frayhip_render_components_device(self._dev, C.byref(fr), C.byref(req), pp, _ptr(sd.state), _ptr(si.state), _ptr(rgb[0]),
                                                          _ptr(rgb[1]), _ptr(var[0]), _ptr(var[1]), call.handle, C.byref(st))
        if rc in (abi.OK, abi.E_CANCELLED):
            sd.samples_done = si.samples_done = req.samples_done
        if run is not None:
            info = run.finish(rc, st)
            info["samples_done"] = sd.samples_done
        else:
            _check(rc)
            info = st.as_dict()
        out = (rgb[0], rgb[1], state) + ((var[0], var[1]) if noise else ())
        return out + ((info,) if (stats or progress is not None) else ())

    # ---- sample maps (include/frayhip.h "sample maps") ----
    def _add_plane(self, who, add, state):
        """The add plane of a map call, checked against the state it goes with: int32 [H, W] of the state's kind, contiguous."""
        W, H = self.frame_size
        if _torch_tensor(add) != state.on_device:
            raise TypeError("%s: add must be of the state's kind (a numpy array for a numpy state, a GPU tensor for a state on the GPU)" % who)
        if state.on_device:
            import torch
            if not add.is_cuda or add.device != state.state.device or add.dtype != torch.int32:
                raise TypeError("%s: add must be an int32 tensor on the state's device" % who)
            add = add.contiguous()
        else:
            add = np.asarray(add)
            if add.dtype != np.int32:
                raise TypeError("%s: add must be int32, got %s" % (who, add.dtype))
            add = np.ascontiguousarray(add)
        if tuple(add.shape) != (H, W):
            raise ValueError("%s: add must be shaped %s, got %s" % (who, (H, W), tuple(add.shape)))
        return add

    def render_components_map(self, add, state=None, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, stats=False, noise=False, stream=None):
        """render_samples_map with direct and indirect light kept apart (frayhip_render_components_map): add[y, x] more samples to each pixel of a
        pair of component states, state = (direct, indirect) as render_components takes it, or None to start a numpy pair.  The two states must
        hold the same number of samples in every pixel (ValueError otherwise), but the pixels may differ among themselves.

        Returns (direct_rgb, indirect_rgb, state[, noise_direct, noise_indirect][, stats]) as render_components.  Every pixel of the call's buckets
        is, bit for bit, that pixel of render_components at the number of samples it now holds; one that holds none is (0, 0, 0) with noise 0.
        The states are updated in place: each carries its own `counts` plane and samples_done, and both collapse back to uniform states once all
        pixels agree.  stats["samples"] is the sum of add over the call's pixels."""
        who = "render_components_map"
        W, H = self.frame_size
        if state is None:
            state = (Accumulation.empty((W, H), seed, bucket_first, bucket_stride), Accumulation.empty((W, H), seed, bucket_first, bucket_stride))
        sd, si, count = _component_pair(who, state, (W, H), seed, bucket_first, bucket_stride)
        add = self._add_plane(who, add, sd)
        self._need_dev()
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, sd.seed, bucket_first, bucket_stride, spp_chunk, stats)
        req = abi.SamplesMap()
        if not sd.on_device:
            rgb = [np.zeros((H, W, 3), np.float32) for _ in range(2)]
            var = [np.zeros((H, W), np.float32) if noise else None for _ in range(2)]
            _check(lib.frayhip_render_components_map(self._dev, C.byref(fr), C.byref(req), _ptr(sd.state), _ptr(si.state), _ptr(count), _ptr(add),
                                                     _ptr(rgb[0]), _ptr(rgb[1]), _ptr(var[0]), _ptr(var[1]), C.byref(st)))
        else:
            with _DeviceCall(sd.state.device, stream) as call:
                rgb = [call.torch.zeros((H, W, 3), dtype=call.torch.float32, device=sd.state.device) for _ in range(2)]
                var = [call.torch.zeros((H, W), dtype=call.torch.float32, device=sd.state.device) if noise else None for _ in range(2)]
                _check(lib.frayhip_render_components_map_device(self._dev, C.byref(fr), C.byref(req), _ptr(sd.state), _ptr(si.state), _ptr(count),
                                                                _ptr(add), _ptr(rgb[0]), _ptr(rgb[1]), _ptr(var[0]), _ptr(var[1]), call.handle,
                                                                C.byref(st)))
        uniform = req.count_min == req.count_max
        sd.samples_done = si.samples_done = req.count_min
        sd.counts = None if uniform else count
        si.counts = None if uniform else (count.clone() if sd.on_device else count.copy())          # each state carries its own plane
        out = (rgb[0], rgb[1], state) + ((var[0], var[1]) if noise else ())
        return out + ((st.as_dict(),) if stats else ())

    def render_samples_map(self, add, state=None, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, stats=False, noise=False, stream=None):
        """Adds add[y, x] more samples to each pixel of a frame (frayhip_render_samples_map): pixel p's samples count[p] .. count[p] + add[p] - 1,
        where count is what the state holds of it.  add: int32 [H, W], >= 0, of the state's kind (numpy: the host entry; a GPU tensor: the device
        entry, on `stream`); state: an Accumulation, or None to start a numpy one.  Mono path-traced frames only.

        Returns (rgb, state[, noise][, stats]) as render_samples.  Every pixel of the call's buckets is, bit for bit, that pixel of render() at the
        number of samples it now holds; one that holds none is (0, 0, 0) with noise 0.  The state is updated in place: while its pixels hold
        different numbers, state.counts is their int32 plane and only this call can continue the state; once they agree again it collapses
        back to samples_done.  stats["samples"] is the sum of add over the call's pixels."""
        who = "render_samples_map"
        W, H = self.frame_size
        if state is None:
            state = Accumulation.empty((W, H), seed, bucket_first, bucket_stride)
        elif not isinstance(state, Accumulation):
            raise TypeError("%s: state must be an Accumulation, got %s" % (who, type(state).__name__))
        state.check(who, (W, H), seed, bucket_first, bucket_stride)
        add = self._add_plane(who, add, state)
        self._need_dev()
        count = state.count_plane()
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, state.seed, bucket_first, bucket_stride, spp_chunk, stats)
        req = abi.SamplesMap()
        if not state.on_device:
            rgb = np.zeros((H, W, 3), np.float32)
            var = np.zeros((H, W), np.float32) if noise else None
            _check(lib.frayhip_render_samples_map(self._dev, C.byref(fr), C.byref(req), _ptr(state.state), _ptr(count), _ptr(add), _ptr(rgb), _ptr(var),
                                                  C.byref(st)))
        else:
            with _DeviceCall(state.state.device, stream) as call:
                rgb = call.torch.zeros((H, W, 3), dtype=call.torch.float32, device=state.state.device)
                var = call.torch.zeros((H, W), dtype=call.torch.float32, device=state.state.device) if noise else None
                _check(lib.frayhip_render_samples_map_device(self._dev, C.byref(fr), C.byref(req), _ptr(state.state), _ptr(count), _ptr(add), _ptr(rgb),
                                                             _ptr(var), call.handle, C.byref(st)))
        state.samples_done = req.count_min
        state.counts = None if req.count_min == req.count_max else count
        out = (rgb, state) + ((var,) if noise else ())
        return out + ((st.as_dict(),) if stats else ())

    def refine(self, state, tolerance, max_count, passes=8, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, stream=None, split=False, budget=None,
               **params):
        """Spends samples where the frame needs them: up to `passes` times, sample_map(state, tolerance=..., max_count=..., **params) and
        render_samples_map of its map; stops when a map is empty.  state: an Accumulation (None starts a numpy one; the first pass then brings
        every pixel to min_count).  Returns (rgb, state, noise, info): the frame, the state, the variance estimate of the mean's luminance --
        denoise_signal's `variance` with demodulate=0 -- and info {"passes": passes that rendered, "samples": samples they added, "ms_kernels":
        their kernel time}.
        With a pair (direct, indirect) of component states, or split=True and state=None (a numpy pair is started), the loop runs the pair's
        sample_map and render_components_map and returns (direct_rgb, indirect_rgb, state, noise_direct, noise_indirect, info).
        budget: None, or the most samples the whole call may add, an int >= 0: each pass asks sample_map for a map under what is left of it, and
        the loop also ends when nothing is left.  info then gains "budget", "tolerance_reached" (the last map's tolerance_used; `tolerance` when no
        map was made) and "stage" (that map's).  A budget with bucket_stride != 1 is refused (ValueError): the map's totals are frame-wide."""
        W, H = self.frame_size
        budget = _budget_of("refine", budget)
        if budget is not None and bucket_stride != 1:
            raise ValueError("refine: budget with a bucket share (bucket_stride %d): the map's totals are frame-wide, so a share cannot own a budget" % bucket_stride)
        pair = isinstance(state, (tuple, list)) or (state is None and split)
        if split and not pair:
            raise TypeError("refine: split=True takes a pair (direct, indirect) of Accumulations, or None")
        if state is None:
            new = lambda: Accumulation.empty((W, H), seed, bucket_first, bucket_stride)
            state = (new(), new()) if pair else new()
        step = self.render_components_map if pair else self.render_samples_map
        done = {"passes": 0, "samples": 0, "ms_kernels": 0.0}
        if budget is not None:
            done.update(budget=budget, tolerance_reached=float(np.float32(tolerance)), stage=0)
        out = None
        for _ in range(int(passes)):
            left = None if budget is None else budget - done["samples"]
            if left == 0:
                break
            add, info = sample_map(state, stream=stream, tolerance=tolerance, max_count=max_count, budget=left, **params)
            if left is not None:
                done["tolerance_reached"], done["stage"] = info["tolerance_used"], info["stage"]
            if info["pixels"] == 0:
                break
            out = step(add, state, seed, bucket_first, bucket_stride, spp_chunk, stats=True, noise=True, stream=stream)
            st = out[-1]
            if st["samples"] == 0:          # the map's pixels all lie outside the call's buckets
                break
            done["passes"] += 1
            done["samples"] += int(st["samples"])
            done["ms_kernels"] += st["ms_kernels"]
        if out is None:                     # nothing to add: the frame of what the state holds
            held = (state[0] if pair else state).count_plane()
            out = step(held * 0, state, seed, bucket_first, bucket_stride, spp_chunk, noise=True, stream=stream) + (None,)
        return out[:-1] + (done,)

    # ---- adaptive frames (include/frayhip.h "adaptive frames") ----
    def _adaptive_request(self, threshold, min_spp, err_floor):
        """Checks the caller's values as the library does and clamps min_spp to the frame's spp."""
        threshold, err_floor, min_spp = float(threshold), float(err_floor), int(min_spp)
        if min_spp < 2:
            raise ValueError("render_adaptive: min_spp must be >= 2, got %d" % min_spp)
        if math.isnan(threshold) or threshold < 0:
            raise ValueError("render_adaptive: threshold must be >= 0 (inf allowed), got %r" % threshold)
        if not (math.isfinite(err_floor) and err_floor > 0):
            raise ValueError("render_adaptive: err_floor must be finite and > 0, got %r" % err_floor)
        return abi.Adaptive(min_spp=min(min_spp, self.samples_per_pixel()), threshold=threshold, err_floor=err_floor)

    def render_adaptive(self, threshold, min_spp=16, err_floor=0.01, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, stats=False, out=None):
        """An adaptive path-traced frame (frayhip_render_adaptive): every pixel climbs the sample ladder floor(min_spp / 2), min_spp, 2 min_spp, ...,
        spp and stops at the first rung from min_spp on whose noise estimate |m - h|_1 / (err_floor + sum(m)) is <= threshold (m, h: its mean at
        this rung and the one before).  Each pixel equals, bit for bit, that pixel of the frame rendered at its final sample count.

        Returns (rgb float32 [H, W, 3], spp int32 [H, W], err float32 [H, W], info); info holds "rungs" (ladder rungs run), "samples" (the sum
        of spp over the call's pixels) and "stats" (the stats dict).  min_spp is clamped to the frame's spp.  out: (rgb, spp, err) arrays to fill
        instead of new zeroed ones (pixels outside the call's buckets keep their values).  The defaults of min_spp and err_floor are starting
        values, not tuned ones."""
        a = self._adaptive_request(threshold, min_spp, err_floor)
        self._need_dev()
        W, H = self.frame_size
        if out is None:
            out = (np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.int32), np.zeros((H, W), np.float32))
        rgb, spp, err = out
        for arr, shape, dt in ((rgb, (H, W, 3), np.float32), (spp, (H, W), np.int32), (err, (H, W), np.float32)):
            if arr.shape != shape or arr.dtype != dt or not arr.flags.c_contiguous:
                raise ValueError("render_adaptive: out arrays must be C-contiguous %s %s" % (shape, np.dtype(dt).name))
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, seed, bucket_first, bucket_stride, spp_chunk, stats)
        _check(lib.frayhip_render_adaptive(self._dev, C.byref(fr), C.byref(a), rgb.ctypes.data, spp.ctypes.data, err.ctypes.data, C.byref(st)))
        return rgb, spp, err, {"rungs": a.rungs, "samples": a.samples, "stats": st.as_dict()}

    def render_adaptive_device(self, d_rgb_ptr, d_spp_ptr=None, d_err_ptr=None, *, threshold, min_spp=16, err_floor=0.01, seed=42,
                               bucket_first=0, bucket_stride=1, spp_chunk=0, stats=False, stream=None):
        """render_adaptive into caller-owned device memory (e.g. torch tensors' data_ptr(): rgb [H, W, 3] float32, spp [H, W] int32, err [H, W]
        float32; spp / err may be None), enqueued on `stream` (a torch stream or a hipStream_t handle; None = the default stream) as render_device.
        Returns the info dict of render_adaptive."""
        a = self._adaptive_request(threshold, min_spp, err_floor)
        self._need_dev()
        if stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, seed, bucket_first, bucket_stride, spp_chunk, stats)
        _check(lib.frayhip_render_device_adaptive(self._dev, C.byref(fr), C.byref(a), d_rgb_ptr, d_spp_ptr, d_err_ptr, stream, C.byref(st)))
        return {"rungs": a.rungs, "samples": a.samples, "stats": st.as_dict()}

    # ---- feature frames and denoising (include/frayhip.h "feature frames", "denoising") ----
    def render_features(self, n_samples=4, seed=42, bucket_first=0, bucket_stride=1, stats=False, out=None):
        """First-hit features of the frame's camera samples 0 .. n_samples-1 (frayhip_render_features): float32 [H, W, 10] -- position[3],
        normal[3] (after the bump), albedo[3], depth -- the FP32 mean in sample order.  out: an array to fill instead of a new zeroed one (pixels
        outside the call's buckets keep their values).  With stats=True returns (feat, stats dict)."""
        self._need_dev()
        W, H = self.frame_size
        feat = out if out is not None else np.zeros((H, W, abi.FEAT_CHANNELS), np.float32)
        if feat.shape != (H, W, abi.FEAT_CHANNELS) or feat.dtype != np.float32 or not feat.flags.c_contiguous:
            raise ValueError("render_features: out must be a C-contiguous float32 array shaped %s" % ((H, W, abi.FEAT_CHANNELS),))
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, seed, bucket_first, bucket_stride, 0, stats)
        _check(lib.frayhip_render_features(self._dev, C.byref(fr), int(n_samples), feat.ctypes.data, C.byref(st)))
        return (feat, st.as_dict()) if stats else feat

    def render_features_specular(self, max_bounces=4, n_samples=4, seed=42, bucket_first=0, bucket_stride=1, stats=False, out=None, bounces=False):
        """render_features with every camera sample followed through Refl / Refr nodes to the first hit that is neither, at most max_bounces
        (1 .. 8) steps (frayhip_render_features_specular, "specular feature frames"): float32 [H, W, 10] with the virtual hit's position (the
        point at the path's length along the primary ray: the mirror image for a planar mirror), the terminal normal unfolded through the
        mirrors, the product of the chain's mult and the terminal albedo, and the path's length as depth.  A sample whose first hit is not
        specular has render_features' row bit for bit.  Layered glass, glossy lobes and total internal reflection are not followed.
        bounces=True also returns the plane of steps taken, float32 [H, W] (the mean over the samples).  out: an array to fill instead of a new
        zeroed one, or with bounces=True a (feat, bounces) pair (pixels outside the call's buckets keep their values).
        Returns feat, then the plane with bounces=True, then the stats dict with stats=True."""
        self._need_dev()
        W, H = self.frame_size
        if bounces:
            feat, plane = out if out is not None else (np.zeros((H, W, abi.FEAT_CHANNELS), np.float32), np.zeros((H, W), np.float32))
        else:
            feat, plane = (out if out is not None else np.zeros((H, W, abi.FEAT_CHANNELS), np.float32)), None
        for a, shape in ((feat, (H, W, abi.FEAT_CHANNELS)), (plane, (H, W))):
            if a is not None and (not isinstance(a, np.ndarray) or a.shape != shape or a.dtype != np.float32 or not a.flags.c_contiguous):
                raise ValueError("render_features_specular: out must be C-contiguous float32, shaped %s (and %s for the bounces)"
                                 % ((H, W, abi.FEAT_CHANNELS), (H, W)))
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, seed, bucket_first, bucket_stride, 0, stats)
        _check(lib.frayhip_render_features_specular(self._dev, C.byref(fr), int(n_samples), int(max_bounces), feat.ctypes.data,
                                                    plane.ctypes.data if plane is not None else None, C.byref(st)))
        res = (feat,) + ((plane,) if bounces else ()) + ((st.as_dict(),) if stats else ())
        return res if len(res) > 1 else feat

    def _features_for(self, n_samples, seed, specular):
        """(feat, stats dict) of render_denoised / render_denoised_split: first-hit guides, or with specular=K > 0 the virtual-hit ones."""
        if specular:
            return self.render_features_specular(int(specular), n_samples, seed=seed, stats=True)
        return self.render_features(n_samples, seed=seed, stats=True)

    def node_transforms(self):
        """A copy of the current nodes' frayhip_transform records (self.desc's, as update() pushes them), as a ctypes array of abi.Transform: the
        snapshot a caller takes before editing the nodes, for render_features_motion."""
        nodes = self.nodes
        out = (abi.Transform * len(nodes))()
        for i, n in enumerate(nodes):
            C.memmove(C.byref(out[i]), C.byref(n.T), C.sizeof(abi.Transform))
        return out

    def _prev_transforms(self, who, prev_transforms):
        """prev_transforms as a ctypes array of abi.Transform (node_transforms()' kind, or a sequence of abi.Transform records)."""
        if isinstance(prev_transforms, C.Array) and prev_transforms._type_ is abi.Transform:
            return prev_transforms
        seq = list(prev_transforms)
        if not all(isinstance(t, abi.Transform) for t in seq):
            raise TypeError("%s: prev_transforms must be Scene.node_transforms() or a sequence of abi.Transform" % who)
        out = (abi.Transform * len(seq))()
        for i, t in enumerate(seq):
            C.memmove(C.byref(out[i]), C.byref(t), C.sizeof(abi.Transform))
        return out

    def render_features_motion(self, prev_transforms, n_samples=4, seed=42, bucket_first=0, bucket_stride=1, stats=False, out=None):
        """The feature frame and the motion frame of one traced pass (frayhip_render_features_motion): (feat [H, W, 10], motion [H, W, 8]), float32.
        prev_transforms: the nodes' transforms when the previous frame was rendered -- node_transforms() taken before the edit.  feat is
        render_features(...), bit for bit; motion holds per pixel {P'.xyz, moved}, {n'.xyz, 0}: where the first hit and its normal were in that
        previous state (the hit itself for a node that did not move), and the share of the pixel's samples that hit a moved node.
        out: a (feat, motion) pair of arrays to fill instead of new zeroed ones.  With stats=True returns (feat, motion, stats dict)."""
        self._need_dev()
        W, H = self.frame_size
        prev = self._prev_transforms("render_features_motion", prev_transforms)
        feat, motion = out if out is not None else (np.zeros((H, W, abi.FEAT_CHANNELS), np.float32), np.zeros((H, W, abi.MOTION_CHANNELS), np.float32))
        for a, ch in ((feat, abi.FEAT_CHANNELS), (motion, abi.MOTION_CHANNELS)):
            if a.shape != (H, W, ch) or a.dtype != np.float32 or not a.flags.c_contiguous:
                raise ValueError("render_features_motion: out must be C-contiguous float32 arrays shaped %s and %s"
                                 % ((H, W, abi.FEAT_CHANNELS), (H, W, abi.MOTION_CHANNELS)))
        st = abi.Stats()
        fr = self._frame(abi.MODE_RENDER, seed, bucket_first, bucket_stride, 0, stats)
        _check(lib.frayhip_render_features_motion(self._dev, C.byref(fr), int(n_samples), prev, len(prev), feat.ctypes.data, motion.ctypes.data,
                                                  C.byref(st)))
        return (feat, motion, st.as_dict()) if stats else (feat, motion)

    def render_denoised(self, seed=42, feature_samples=4, specular=0, **params):
        """A denoised frame: (denoised, raw, stats).  raw is the ordinary frame (= render(seed), bit for bit), rendered progressively; with an even
        spp >= 2 its preview at spp / 2 samples is the filter's rgb_half (the exact spp/2 frame, no second render), otherwise the filter runs without
        it.  The features take min(feature_samples, spp) samples.  params: denoise_params.  stats: the "render", "features" and "denoise" stats dicts,
        and the filter's inputs "rgb_half" (None without it) and "features_frame".
        specular=K > 0: the guides are render_features_specular(K, ...) instead (what mirrors and glass show, followed through at most K
        steps); 0 is render_features."""
        self._need_dev()
        W, H = self.frame_size
        spp = self.samples_per_pixel()
        half = None
        chunk = 0
        if spp >= 2 and spp % 2 == 0:
            hs = spp // 2
            chunk = max(d for d in range(1, min(hs, 8) + 1) if hs % d == 0)     # batches end at spp / 2; at most 8 spp per batch
        half_wanted = chunk > 0
        keep = {}

        def progress(info):
            if half_wanted and info["preview"] and info["samples_done"] == spp // 2:
                keep["half"] = info["image"].copy()
            return False
        raw, rst = self.render(seed=seed, spp_chunk=chunk, progress=progress, preview_ms=0 if half_wanted else -1)
        if half_wanted:
            half = keep.get("half")
            if half is None:
                raise FrayError(abi.E_HIP, "render_denoised: no preview at spp / 2 = %d samples" % (spp // 2))
        feat, fst = self._features_for(min(int(feature_samples), spp), seed, specular)
        out, dst = denoise(raw, feat, half, stats=True, **params)
        return out, raw, {"render": rst, "features": fst, "denoise": dst, "rgb_half": half, "features_frame": feat}

    def render_denoised_split(self, seed=42, feature_samples=4, refine=None, max_count=None, passes=8, budget=None, specular=0, **params):
        """A frame whose direct and indirect light are filtered apart: (denoised, raw, info).  The components of the frame's spp samples come from
        render_components with their noise estimates, each goes through denoise_signal with the feature frame (demodulate=0: the states' noise is
        in rgb's domain) and the two results are added in FP32.  raw = direct_rgb + indirect_rgb.  params: denoise_params, but demodulate=1 is
        refused (ValueError).  info: the "render", "features", "denoise_direct" and "denoise_indirect" stats dicts, the filtered components
        "direct" and "indirect", and their inputs "direct_rgb", "indirect_rgb", "noise_direct", "noise_indirect" and "features_frame".
        refine=TOL: the components come from Scene.refine on a new pair of states instead (tolerance TOL, at most max_count samples in a pixel --
        required -- and at most `passes` passes); "render" is then refine's info, info gains "refine" (that info with "counts", the int32 [H, W]
        plane of samples held) and the features take min(feature_samples, the largest count) samples.  budget: refine's frame-wide sample
        budget (it needs refine).  specular=K > 0: the guides are render_features_specular(K, ...), as in render_denoised."""
        if refine is None and max_count is not None:
            raise ValueError("render_denoised_split: max_count needs refine")
        if refine is None and budget is not None:
            raise ValueError("render_denoised_split: budget needs refine")
        if refine is not None and max_count is None:
            raise ValueError("render_denoised_split: refine needs max_count")
        if params.get("demodulate", 0):
            raise ValueError("render_denoised_split: demodulate=1 is not offered: the components' noise is in rgb's domain, not demodulated")
        params = dict(params, demodulate=0)
        denoise_params(**params)                # unknown names are refused before anything is rendered
        self._need_dev()
        extra = {}
        if refine is None:
            spp = self.samples_per_pixel()
            d_rgb, i_rgb, _state, d_noise, i_noise, rst = self.render_components(spp, seed=seed, noise=True, stats=True)
        else:
            d_rgb, i_rgb, state, d_noise, i_noise, rst = self.refine(None, refine, max_count, passes=passes, seed=seed, split=True, budget=budget)
            held = state[0].count_plane()
            spp = max(int(held.max()), 1)
            extra["refine"] = dict(rst, counts=held)
        feat, fst = self._features_for(min(int(feature_samples), spp), seed, specular)
        d_out, dst = denoise_signal(d_rgb, d_noise, feat, stats=True, **params)
        i_out, ist = denoise_signal(i_rgb, i_noise, feat, stats=True, **params)
        return d_out + i_out, d_rgb + i_rgb, dict({"render": rst, "features": fst, "denoise_direct": dst, "denoise_indirect": ist, "direct": d_out,
                                                   "indirect": i_out, "direct_rgb": d_rgb, "indirect_rgb": i_rgb, "noise_direct": d_noise,
                                                   "noise_indirect": i_noise, "features_frame": feat}, **extra)

    def _sequence_samples(self, fr, count, state, stream):
        """render_sequence's own call of frayhip_render_samples_device (state: an Accumulation) or frayhip_render_components_device (a pair of
        them) for `count` more samples of frame record `fr`, without the counting kernels that stats=True asks for: (rgb or (direct_rgb,
        indirect_rgb), stats dict).  The states are fresh device states of the record's seed."""
        import torch
        W, H = self.frame_size
        pair = isinstance(state, tuple)
        first = state[0] if pair else state
        st = abi.Stats()
        req = abi.Samples(sample_first=first.samples_done, sample_count=int(count))
        with torch.cuda.stream(stream):
            rgb = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2 if pair else 1)]
        handle = C.c_void_p(stream.cuda_stream)
        if pair:
            _check(lib.frayhip_render_components_device(self._dev, C.byref(fr), C.byref(req), None, _ptr(state[0].state), _ptr(state[1].state),
                                                        _ptr(rgb[0]), _ptr(rgb[1]), None, None, handle, C.byref(st)))
        else:
            _check(lib.frayhip_render_samples_device(self._dev, C.byref(fr), C.byref(req), None, _ptr(state.state), _ptr(rgb[0]), None, handle,
                                                     C.byref(st)))
        for a in (state if pair else (state,)):
            a.samples_done = req.samples_done
        return (tuple(rgb) if pair else rgb[0]), st.as_dict()

    def _sequence_samples_map(self, fr, add, state, stream):
        """render_sequence's own call of frayhip_render_samples_map_device: add[y, x] more samples of frame record `fr` on the device state
        `state`, without the counting kernels that stats=True asks for: (rgb, stats dict)."""
        import torch
        W, H = self.frame_size
        st = abi.Stats()
        req = abi.SamplesMap()
        with torch.cuda.stream(stream):
            count = state.count_plane()
            rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        _check(lib.frayhip_render_samples_map_device(self._dev, C.byref(fr), C.byref(req), _ptr(state.state), _ptr(count), _ptr(add), _ptr(rgb), None,
                                                     C.c_void_p(stream.cuda_stream), C.byref(st)))
        state.samples_done = req.count_min
        state.counts = None if req.count_min == req.count_max else count
        return rgb, st.as_dict()

    def render_sequence(self, cameras, seed=42, feature_samples=4, temporal=None, edit=None, split=False, temporal_direct=None, temporal_indirect=None,
                        change_samples=0, change=None, boost=None, specular=0, **denoise_params):
        """A generator over a fly-through of a static scene with temporal accumulation (include/frayhip.h "temporal accumulation"): for the k-th
        abi.Camera of `cameras` it sets the view, renders the feature frame and the frame with seed + k (equal seeds would accumulate the same
        noise every frame), accumulates onto the previous frame's history reprojected into this view, runs the a-trous levels on the accumulated
        signal and its variance, and yields (denoised, raw, info): torch tensors on the GPU, float32 [H, W, 3]; raw is render(seed + k) of that
        view, bit for bit.  Every buffer stays on the device.  info: "features_frame", "history" [H, W, 12], "signal", "variance", "view"
        (this frame's abi.View), "film_offset", and the "render", "features", "temporal" and "denoise" stats dicts.
        temporal: a dict of temporal_params fields.  film_offset defaults to where a pixel's samples lie on average: 0.5 for gi and DOF frames
        (uniform jitter), 0.3 for a Whitted frame with wantAA (the mean of the five AA offsets), 0 for a plain Whitted frame.  The filter and
        the accumulation share `demodulate` (denoise_params; default 1).  Stereo frames and long generators are refused (FrayError) as
        render_features refuses them.  The scene's camera is restored when the generator ends or is closed.
        edit: None (a static scene: exactly the launches above), or a callable edit(k, scene) that is called before frame k >= 1, after the
        snapshot of node_transforms(); it may edit the description's tables and must call scene.update() itself if it does.  With edit given,
        every frame renders the features and the motion frame in one pass (frayhip_render_features_motion; frame 0 against its own transforms),
        accumulates through the motion frame, and info also holds "motion" [H, W, 8].  What was edited stays edited when the generator ends.
        split: False runs exactly the launches above.  True (mono path-traced frames; a Whitted or a stereo frame is refused with FrayError before
        anything is rendered) keeps one history per light component (include/frayhip.h "split temporal accumulation"): after the feature pass the
        frame's samples are rendered as components (render_components into two fresh device states, seed + k), one temporal_accumulate_split
        accumulates both, denoise_signal runs on each component with the sequence's `demodulate` (1 is fine here: the variance comes from the
        moments of the demodulated signal), and the yielded picture is the FP32 sum of the two results.  raw is direct_rgb + indirect_rgb, which
        is NOT render(seed + k) bit for bit: two sums of samples are added.  info then holds "direct", "indirect" (the filtered components),
        "direct_rgb", "indirect_rgb", "signal_direct", "signal_indirect", "variance_direct", "variance_indirect", "history" [H, W, 20],
        "params_direct" and "params_indirect" (the temporal_params fields in force), and "denoise_direct", "denoise_indirect" in place of
        "denoise".  temporal= still sets both components; temporal_direct / temporal_indirect (dicts of temporal_params fields; split only)
        override it per component, and demodulate, film_offset, plane_tolerance and normal_min_dot must stay equal.  Where the caller names no
        max_history the direct component's is 8 and the indirect one's the default 32: a shadow that moves over a static surface lives in the
        direct component, and its residue after j frames is (1 - 1/8)^j of the step instead of (1 - 1/32)^j, while direct light at one
        next-event sample per path sample is the less noisy component.  The 8 is a choice, not a measurement.
        change_samples: 0 runs exactly the launches above.  n > 0 (needs edit=, ValueError otherwise; n = min(change_samples, spp)) detects what
        the edit changed in the light a pixel receives -- moved lights, the shadows and reflections of moved objects -- and shortens the history
        there (include/frayhip.h "change frames").  Frame 0 is as above.  Frame k >= 1: after the snapshot of node_transforms() and BEFORE
        edit(k, scene), samples [0, n) of this frame's view and seed are rendered into a fresh device state (the probe: render_samples, or
        render_components with split) while the scene is still in frame k - 1's state; after the edit and the feature / motion pass the frame
        itself is rendered as those n samples into a fresh state, the state is cloned, and the remaining spp - n samples follow, so raw is still
        render(seed + k) bit for bit (resumable frames) and the frame costs n / spp more rays (info["render"] then holds the sum of its two
        calls' figures).  change_frame(probe, clone, motion) then gives the
        change frame, and the accumulation takes it (temporal_accumulate(change=)).  A pixel none of whose n paths met anything the edit changed
        has change 0 where its whole window has, and is accumulated exactly as without change_samples.  With split there is one change frame
        per component, from that component's pair of states, and frames k >= 1 make one temporal_accumulate_split(change_direct=,
        change_indirect=) on the 20-channel history, whose outputs are those two temporal_accumulate(change=) calls' bit for bit.  info then also
        holds "change" (or "change_direct" and "change_indirect") and the "probe" stats dict; they are None in frame 0.
        change: a dict of change_frame's radius and gain (needs change_samples > 0).  radius 3 and gain 1 are a choice, not a measurement.
        boost: None runs exactly the launches above.  A dict of history_map's target (default 8), max_units (8) and budget (None) spends samples
        where the reprojected history is short (include/frayhip.h "weighted accumulation and history maps"): mono path-traced frames only (a
        Whitted or stereo frame and a long generator are refused with FrayError before anything is rendered; with split=True it is a ValueError:
        not offered yet; unknown keys are a TypeError).  Frame k then runs the feature (and motion) pass as above; with change_samples, after
        the edit the frame's first n samples go into a fresh device state, which is cloned for change_frame; history_map(feat, view, history,
        units, motion, change, base=spp, ...) with the sequence's temporal parameters gives add and weight; render_samples_map renders add (add - n
        on the state that holds n; n <= spp <= add always), so that every pixel of raw is that pixel of render(seed + k) at add[pixel] samples bit for
        bit; temporal_accumulate(weight=, units_in=) accumulates raw.  info gains "counts" (int32 [H, W]: the samples each pixel of raw holds),
        "weight", "units" (the units plane that goes with "history") and "boost" (history_map's info).  target=1, max_units=1 gives every output bit
        of the boost=None sequence.  target 8 and max_units 8 are a choice, not a measurement.
        specular: 0 runs exactly the launches above.  K > 0 (1 .. 8) renders every frame's guides with frayhip_render_features_specular_device
        (max_bounces = K) in place of the first-hit pass and changes nothing else, with split= and boost= too: what a static mirror or pane of
        glass shows is then reprojected as the geometry it is, under a moving camera.  With edit= it raises ValueError: motion frames carry
        first hits only, so a moved object seen in a mirror cannot be followed (and change_samples=, which needs edit=, goes with it)."""
        specular = int(specular)
        if specular < 0 or specular > abi.SPECULAR_MAX_BOUNCES:
            raise ValueError("render_sequence: specular must be 0 .. %d, got %d" % (abi.SPECULAR_MAX_BOUNCES, specular))
        if specular and edit is not None:
            raise ValueError("render_sequence: specular= is not offered with edit=: motion frames carry first hits only")
        bparams = None
        if boost is not None:                   # what the arguments alone decide, before the device is asked for
            if split:
                raise ValueError("render_sequence: boost with split=True is not offered yet")
            bparams = dict(boost)
            if set(bparams) - {"target", "max_units", "budget"}:
                raise TypeError("render_sequence: boost= takes target, max_units and budget, got %s" % ", ".join(sorted(set(bparams) - {"target", "max_units", "budget"})))
        self._need_dev()
        import torch
        W, H = self.frame_size
        spp = self.samples_per_pixel()
        if boost is not None:
            if not self.settings.gi:
                raise FrayError(abi.E_UNSUPPORTED, "render_sequence: boost needs a path-traced frame (settings.gi): sample maps are not offered for Whitted frames")
            if self.camera.stereoSeparation > 0:
                raise FrayError(abi.E_UNSUPPORTED, "render_sequence: boost is not offered for stereo frames")
            if 8 + 10 * (int(self.settings.maxTraceDepth) + 2) > 227:
                raise FrayError(abi.E_UNSUPPORTED, "render_sequence: boost is not offered for long generators (maxTraceDepth %d)" % self.settings.maxTraceDepth)
        change_samples = int(change_samples)
        if change_samples < 0:
            raise ValueError("render_sequence: change_samples must be >= 0, got %d" % change_samples)
        if change_samples > 0 and edit is None:
            raise ValueError("render_sequence: change_samples needs edit=: without an edit nothing changes between the probe and the frame")
        if change is not None and change_samples == 0:
            raise ValueError("render_sequence: change= needs change_samples > 0")
        cparams = dict(change or {})
        if set(cparams) - {"radius", "gain"}:
            raise TypeError("render_sequence: change= takes radius and gain, got %s" % ", ".join(sorted(set(cparams) - {"radius", "gain"})))
        cp = change_params(**cparams)
        if not 0 <= cp.radius <= 3:
            raise ValueError("render_sequence: change=: radius must be 0..3, got %d" % cp.radius)
        if not (np.isfinite(cp.gain) and cp.gain > 0):
            raise ValueError("render_sequence: change=: gain must be finite and > 0, got %r" % cp.gain)
        n_probe = min(change_samples, spp)
        if not split and (temporal_direct is not None or temporal_indirect is not None):
            raise ValueError("render_sequence: temporal_direct and temporal_indirect need split=True")
        if split:
            if not self.settings.gi:
                raise FrayError(abi.E_UNSUPPORTED, "render_sequence: component frames need a path-traced frame (settings.gi)")
            if self.camera.stereoSeparation > 0:
                raise FrayError(abi.E_UNSUPPORTED, "render_sequence: component frames are not offered for stereo frames")
        tparams = dict(temporal or {})
        if "film_offset" not in tparams:
            tparams["film_offset"] = 0.5 if (self.settings.gi or self.camera.dof) else 0.3 if self.settings.wantAA else 0.0
        dparams = _denoise_params(**denoise_params)
        if tparams.setdefault("demodulate", dparams.demodulate) != dparams.demodulate:
            raise ValueError("render_sequence: the accumulation and the filter must agree on demodulate")
        temporal_params(**tparams)                      # unknown fields are refused before anything is rendered
        if split:
            tdirect, tindirect = dict(tparams, **(temporal_direct or {})), dict(tparams, **(temporal_indirect or {}))
            tdirect.setdefault("max_history", 8)
            for t in (tdirect, tindirect):
                if t["demodulate"] != dparams.demodulate:
                    raise ValueError("render_sequence: the accumulation and the filter must agree on demodulate")
            pd, pi = _split_params("render_sequence", tdirect, tindirect, {})
            fields = lambda p: {k: getattr(p, k) for k in _TEMPORAL_FIELDS}
        n_feat = min(int(feature_samples), spp)
        saved = abi.Camera.from_buffer_copy(self.desc.camera)
        stream = torch.cuda.current_stream()
        handle = C.c_void_p(stream.cuda_stream)
        hist, view, units = None, None, None
        try:
            for k, cam in enumerate(cameras):
                if not isinstance(cam, abi.Camera):
                    raise TypeError("render_sequence: cameras must yield abi.Camera records, got %s" % type(cam).__name__)
                C.memmove(C.byref(self.desc.camera), C.byref(cam), C.sizeof(abi.Camera))
                self.beginFrame()
                motion = None
                fr = self._frame(abi.MODE_RENDER, (seed + k) & 0xFFFFFFFF, 0, 1, 0, False)
                fresh = lambda: Accumulation.empty((W, H), fr.seed, device="cuda")
                probing = n_probe > 0 and k > 0
                probe, pst = None, None
                if edit is not None:
                    prev = self.node_transforms()
                    if probing:                 # samples [0, n) of this frame, in the scene as the previous frame saw it
                        probe = (fresh(), fresh()) if split else fresh()
                        _, pst = self._sequence_samples(fr, n_probe, probe, stream)
                    if k:
                        edit(k, self)
                feat = torch.empty((H, W, abi.FEAT_CHANNELS), dtype=torch.float32, device="cuda")
                fst, rst = abi.Stats(), abi.Stats()
                if edit is not None:
                    motion = torch.empty((H, W, abi.MOTION_CHANNELS), dtype=torch.float32, device="cuda")
                    _check(lib.frayhip_render_features_motion_device(self._dev, C.byref(fr), n_feat, prev, len(prev), feat.data_ptr(),
                                                                     motion.data_ptr(), handle, C.byref(fst)))
                elif specular:
                    _check(lib.frayhip_render_features_specular_device(self._dev, C.byref(fr), n_feat, specular, feat.data_ptr(), None, handle,
                                                                       C.byref(fst)))
                else:
                    _check(lib.frayhip_render_features_device(self._dev, C.byref(fr), n_feat, feat.data_ptr(), handle, C.byref(fst)))
                if split:
                    state = (fresh(), fresh())
                    chg_d = chg_i = None
                    if probing:
                        (d_rgb, i_rgb), rst = self._sequence_samples(fr, n_probe, state, stream)
                        first = [a.state.clone() for a in state]
                        if spp > n_probe:
                            (d_rgb, i_rgb), rst2 = self._sequence_samples(fr, spp - n_probe, state, stream)
                            rst = _sum_stats(rst, rst2)
                        chg_d = change_frame(probe[0], first[0], motion, stream=stream, **cparams)
                        chg_i = change_frame(probe[1], first[1], motion, stream=stream, **cparams)
                    else:
                        d_rgb, i_rgb, _state, rst = self.render_components(spp, state, seed=fr.seed, stats=True, stream=stream)
                    hist, sig_d, sig_i, var_d, var_i, tst = temporal_accumulate_split(d_rgb, i_rgb, feat, view, hist, motion=motion, direct=tdirect,
                                                                                      indirect=tindirect, stats=True, stream=stream, change_direct=chg_d,
                                                                                      change_indirect=chg_i)
                    d_out, dst = denoise_signal(sig_d, var_d, feat, stats=True, stream=stream, **denoise_params)
                    i_out, ist = denoise_signal(sig_i, var_i, feat, stats=True, stream=stream, **denoise_params)
                    view = view_from_camera(self.desc.camera, W, H)
                    info = {"features_frame": feat, "history": hist, "direct": d_out, "indirect": i_out, "direct_rgb": d_rgb, "indirect_rgb": i_rgb,
                            "signal_direct": sig_d, "signal_indirect": sig_i, "variance_direct": var_d, "variance_indirect": var_i, "view": view,
                            "film_offset": tdirect["film_offset"], "params_direct": fields(pd), "params_indirect": fields(pi), "render": rst,
                            "features": fst.as_dict(), "temporal": tst, "denoise_direct": dst, "denoise_indirect": ist}
                    if edit is not None:
                        info["motion"] = motion
                    if n_probe > 0:
                        info.update(change_direct=chg_d, change_indirect=chg_i, probe=pst)
                    yield d_out + i_out, d_rgb + i_rgb, info
                    continue
                chg = None
                if bparams is not None:
                    state = fresh()
                    rdict = None
                    if probing:
                        _, rdict = self._sequence_samples(fr, n_probe, state, stream)
                        chg = change_frame(probe, state.state.clone(), motion, stream=stream, **cparams)
                    add, weight, binfo = history_map(feat, view, hist, units, motion=motion, change=chg, base=spp, stream=stream,
                                                     **dict(bparams, **tparams))
                    raw, rdict2 = self._sequence_samples_map(fr, add - n_probe if probing else add, state, stream)
                    rdict = _sum_stats(rdict, rdict2) if rdict else rdict2
                    hist, units, signal, var, tst = temporal_accumulate(raw, feat, view, hist, stats=True, stream=stream, motion=motion, change=chg,
                                                                        weight=weight, units_in=units, **tparams)
                    out, dst = denoise_signal(signal, var, feat, stats=True, stream=stream, **denoise_params)
                    view = view_from_camera(self.desc.camera, W, H)
                    info = {"features_frame": feat, "history": hist, "signal": signal, "variance": var, "view": view,
                            "film_offset": tparams["film_offset"], "render": rdict, "features": fst.as_dict(), "temporal": tst,
                            "denoise": dst, "counts": add, "weight": weight, "units": units, "boost": binfo}
                    if edit is not None:
                        info["motion"] = motion
                    if n_probe > 0:
                        info.update(change=chg, probe=pst)
                    yield out, raw, info
                    continue
                if probing:
                    state = fresh()
                    raw, rdict = self._sequence_samples(fr, n_probe, state, stream)
                    first = state.state.clone()
                    if spp > n_probe:
                        raw, rdict2 = self._sequence_samples(fr, spp - n_probe, state, stream)
                        rdict = _sum_stats(rdict, rdict2)
                    chg = change_frame(probe, first, motion, stream=stream, **cparams)
                else:
                    raw = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
                    _check(lib.frayhip_render_device(self._dev, C.byref(fr), raw.data_ptr(), None, None, handle, C.byref(rst)))
                    rdict = rst.as_dict()
                hist, signal, var, tst = temporal_accumulate(raw, feat, view, hist, stats=True, stream=stream, motion=motion, change=chg, **tparams)
                out, dst = denoise_signal(signal, var, feat, stats=True, stream=stream, **denoise_params)
                view = view_from_camera(self.desc.camera, W, H)
                info = {"features_frame": feat, "history": hist, "signal": signal, "variance": var, "view": view,
                        "film_offset": tparams["film_offset"], "render": rdict, "features": fst.as_dict(), "temporal": tst,
                        "denoise": dst}
                if edit is not None:
                    info["motion"] = motion
                if n_probe > 0:
                    info.update(change=chg, probe=pst)
                yield out, raw, info
        finally:
            if self.desc is not None:
                C.memmove(C.byref(self.desc.camera), C.byref(saved), C.sizeof(abi.Camera))
                if self._dev:
                    self.beginFrame()

    def close(self):
        self.endRender()
        if self._hs:
            lib.frayhip_host_scene_free(self._hs)
            self._hs = C.c_void_p()
            self.desc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
