"""Sample maps (include/frayhip.h "sample maps": frayhip_render_samples_map), what can be checked without a GPU: both entry points are exported and
mirrored, the request struct's layout matches the library's, every argument check that needs no uploaded scene answers FRAYHIP_E_ARG before the
device is touched with the entry's name in the message, the Python side refuses bad values and keeps a state with per-pixel counts out of the
uniform calls, an Accumulation with and without counts survives save / load, and the CLI lists its flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES
from test_abi import header_functions

ENTRIES = ["frayhip_render_samples_map", "frayhip_render_samples_map_device"]


def test_samples_map_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n


def test_samples_map_struct_layout(fray, abi):
    assert fray.lib.frayhip_sizeof(b"frayhip_samples_map") == C.sizeof(abi.SamplesMap) == 16
    assert abi.STRUCTS["frayhip_samples_map"] is abi.SamplesMap
    assert abi.SamplesMap.samples.offset == 0 and abi.SamplesMap.count_min.offset == 8 and abi.SamplesMap.count_max.offset == 12
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning


@pytest.mark.parametrize("dev", [False, True])
def test_samples_map_argument_checks(fray, abi, dev):
    L = fray.lib
    buf = (C.c_float * 64)()                    # 16-byte aligned by ctypes' allocator for an array this size; carved below
    base = (C.addressof(buf) + 15) & ~15
    accum, count, add, rgb, noise = base, base + 16, base + 32, base + 48, base + 64
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)
    who = ENTRIES[1] if dev else ENTRIES[0]

    def call(f, m, accum=accum, count=count, add=add, rgb=rgb, noise=noise):
        fp = C.byref(f) if f is not None else None
        mp = C.byref(m) if m is not None else None
        if dev:
            return L.frayhip_render_samples_map_device(None, fp, mp, accum, count, add, rgb, noise, None, None)
        return L.frayhip_render_samples_map(None, fp, mp, accum, count, add, rgb, noise, None)

    def expect(rc, words):
        assert rc == abi.E_ARG
        msg = L.frayhip_last_error().decode()
        assert words in msg and msg.startswith(who + ":"), msg

    m = abi.SamplesMap()
    expect(call(None, m), "null frame")
    expect(call(fr, None), "null request")
    expect(call(fr, m, accum=None), "null accum")
    expect(call(fr, m, count=None), "null count")
    expect(call(fr, m, add=None), "null add")
    expect(call(abi.Frame(mode=abi.MODE_PRIMARY_ID, seed=42), m), "mode must be")
    # two buffers at one address overlap whatever the frame's size
    expect(call(fr, m, count=accum), "count must not overlap accum")
    expect(call(fr, m, add=count), "add must not overlap count")
    expect(call(fr, m, rgb=accum), "rgb must not overlap accum")
    expect(call(fr, m, noise=add), "noise must not overlap add")
    expect(call(fr, m, noise=rgb), "noise must not overlap rgb")
    if dev:
        expect(call(fr, m, accum=accum + 4), "16-byte aligned")
        for name, ptr in (("count", count), ("add", add), ("rgb", rgb), ("noise", noise)):
            expect(call(fr, m, **{name: ptr + 2}), "4-byte aligned")
    # good arguments, and the optional outputs left out, get as far as the missing scene
    expect(call(fr, m), "null scene")
    expect(call(fr, m, rgb=None, noise=None), "null scene")


def test_python_refuses_bad_values_without_a_gpu(fray):
    s = fray.Scene.parseScene(os.path.join(SCENES, "cornell_box.fray"))       # parsed, not uploaded
    W, H = s.frame_size
    add = np.ones((H, W), np.int32)
    with pytest.raises(TypeError):
        s.render_samples_map(add.astype(np.int64))
    with pytest.raises(TypeError):
        s.render_samples_map(add.astype(np.float32))
    with pytest.raises(ValueError):
        s.render_samples_map(add[:-1])
    with pytest.raises(TypeError):
        s.render_samples_map(add, state=np.zeros((H, W, 4), np.float32))
    st = fray.Accumulation.empty((W, H), seed=7)
    with pytest.raises(ValueError, match="seed"):
        s.render_samples_map(add, st, seed=8)
    st.counts = np.zeros((H, W), np.int64)
    with pytest.raises(ValueError, match="counts"):
        s.render_samples_map(add, st, seed=7)
    # good values get as far as the missing upload
    with pytest.raises(fray.FrayError, match="beginRender"):
        s.render_samples_map(add)
    s.close()


def test_uniform_calls_refuse_per_pixel_counts(fray):
    s = fray.Scene.parseScene(os.path.join(SCENES, "cornell_box.fray"))
    W, H = s.frame_size
    st = fray.Accumulation.empty((W, H))
    st.counts = np.full((H, W), 3, np.int32)
    st.counts[0, 0] = 5
    st.samples_done = 3
    with pytest.raises(ValueError, match="different numbers of samples"):
        s.render_samples(1, st)
    with pytest.raises(ValueError, match="different numbers of samples"):
        s.render_components(1, (st, fray.Accumulation.empty((W, H))))
    # a plane that holds one value collapses back to samples_done, and the call goes on to the missing upload
    st.counts[0, 0] = 3
    st.samples_done = 0
    with pytest.raises(fray.FrayError, match="beginRender"):
        s.render_samples(1, st)
    assert st.counts is None and st.samples_done == 3
    s.close()


def test_accumulation_round_trip_with_and_without_counts(fray, tmp_path):
    rng = np.random.default_rng(5)
    state = rng.random((6, 9, 4), dtype=np.float32)
    plain = fray.Accumulation(state.copy(), 7, seed=11, bucket_first=1, bucket_stride=2)
    back = fray.Accumulation.load(plain.save(tmp_path / "plain.npz"))
    assert back.counts is None and back.samples_done == 7 and back.seed == 11 and back.size == (9, 6)
    assert (back.bucket_first, back.bucket_stride) == (1, 2) and np.array_equal(back.state, state)
    with np.load(tmp_path / "plain.npz") as z:
        assert "counts" not in z.files                       # files of uniform states stay as they were
    counts = rng.integers(0, 40, (6, 9)).astype(np.int32)
    held = fray.Accumulation(state.copy(), int(counts.min()), seed=11, counts=counts.copy())
    back = fray.Accumulation.load(held.save(tmp_path / "counts.npz"))
    assert back.counts.dtype == np.int32 and np.array_equal(back.counts, counts) and back.samples_done == int(counts.min())
    assert np.array_equal(back.state, state) and np.array_equal(back.count_plane(), counts)
    back.check("test", (9, 6), 11, 0, 1)
    assert np.array_equal(plain.count_plane(), np.full((6, 9), 7, np.int32))


def test_cli_lists_the_refine_flags():
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, FRAYHIP_NO_TORCH="1"))
    assert out.returncode == 0, out.stderr
    for flag in ("--refine", "--max-spp", "--refine-passes"):
        assert flag in out.stdout, flag
    from fray_amd.__main__ import build_parser, check_args
    ap = build_parser()
    a = ap.parse_args(["scene.fray", "--refine", "0.05", "--max-spp", "64", "--accumulate", "s.npz", "--noise-out", "n.npy", "--denoise"])
    assert (a.refine, a.max_spp) == (0.05, 64)
    check_args(ap, a)                                        # --refine is what lets --accumulate and --noise-out meet --denoise
    assert ap.parse_args(["scene.fray"]).refine is None
    for argv in (["scene.fray", "--refine", "0.05"], ["scene.fray", "--max-spp", "8"], ["scene.fray", "--refine", "0", "--max-spp", "8"],
                 ["scene.fray", "--refine", "0.05", "--max-spp", "8", "--adaptive", "0.1"]):
        with pytest.raises(SystemExit):
            check_args(ap, ap.parse_args(argv))
