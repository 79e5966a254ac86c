"""Resumable frames (include/frayhip.h "resumable frames"), what can be checked without a GPU: both entry points are exported and mirrored, the request
struct's layout matches the library's, every argument check that needs no uploaded scene answers FRAYHIP_E_ARG with the entry's name before the
device is touched, the Python side refuses states that belong to another frame, the CLI lists its flags and refuses a foreign state before the
scene is uploaded, Accumulation.save / load round-trip, and the numpy restatement of the state (tests/samples_ref.py) behaves as the header says
on synthetic colours."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES
from samples_ref import accumulate, luminance, mean_and_noise
from test_abi import header_functions

ENTRIES = ["frayhip_render_samples", "frayhip_render_samples_device"]
F32 = np.float32


def test_samples_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n


def test_samples_struct_layout(fray, abi):
    assert fray.lib.frayhip_sizeof(b"frayhip_samples") == C.sizeof(abi.Samples) == 16
    assert abi.STRUCTS["frayhip_samples"] is abi.Samples
    assert [getattr(abi.Samples, f).offset for f in ("sample_first", "sample_count", "samples_done", "_pad")] == [0, 4, 8, 12]
    header = open(os.path.join(ROOT, "include", "frayhip.h")).read()
    assert int(re.search(r"#define FRAYHIP_ACCUM_CHANNELS (\d+)", header).group(1)) == abi.ACCUM_CHANNELS == 4
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning


@pytest.mark.parametrize("dev", [False, True])
def test_samples_argument_checks(fray, abi, dev):
    L = fray.lib
    name = ENTRIES[1] if dev else ENTRIES[0]
    acc = 1 << 20                                # an address, 16-byte aligned; never dereferenced: every call below ends before the device is touched
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)

    def req(first=0, count=4):
        return abi.Samples(sample_first=first, sample_count=count)

    def call(f=fr, r=None, p=None, accum=acc, rgb=None, noise=None):
        fp = C.byref(f) if f is not None else None
        rp = C.byref(r) if r is not None else None
        pp = C.byref(p) if p is not None else None
        if dev:
            return L.frayhip_render_samples_device(None, fp, rp, pp, accum, rgb, noise, None, None)
        return L.frayhip_render_samples(None, fp, rp, pp, accum, rgb, noise, None)

    def expect(rc, words):
        assert rc == abi.E_ARG
        msg = L.frayhip_last_error().decode()
        assert words in msg and msg.startswith(name + ":"), msg

    expect(call(f=None, r=req()), "null frame")
    expect(call(r=None), "null request")
    expect(call(r=req(), accum=None), "null accum")
    expect(call(f=abi.Frame(mode=abi.MODE_PRIMARY_ID, seed=42), r=req()), "mode must be")
    for first in (-1, -2 ** 31):
        expect(call(r=req(first=first)), "sample_first must be >= 0")
    for count in (0, -3):
        expect(call(r=req(count=count)), "sample_count must be >= 1")
    for first, count in ((2 ** 24, 1), (1, 2 ** 24), (2 ** 31 - 1, 2 ** 31 - 1)):
        expect(call(r=req(first, count)), "2^24")
    expect(call(r=req(), p=abi.Progressive(preview_ms=math.nan)), "preview_ms")
    if dev:
        expect(call(r=req(), accum=acc + 4), "16-byte aligned")
        expect(call(r=req(), accum=acc + 8), "16-byte aligned")
        expect(call(r=req(), rgb=acc + 2), "4-byte aligned")
        expect(call(r=req(), noise=acc + 1), "4-byte aligned")
    # the extreme legal values pass every check that needs no scene
    expect(call(r=req(0, 2 ** 24)), "null scene")
    expect(call(r=req(2 ** 24 - 1, 1), p=abi.Progressive(preview_ms=0.0)), "null scene")
    expect(call(r=req(), rgb=acc, noise=acc), "null scene")          # overlaps need the frame's size: checked with the scene


def test_python_refuses_foreign_states_without_a_gpu(fray):
    s = fray.Scene.parseScene(os.path.join(SCENES, "cornell_box.fray"))       # parsed, not uploaded
    s.settings.frameWidth, s.settings.frameHeight = 40, 30
    A = fray.Accumulation
    good = A.empty((40, 30), seed=42)
    for state, kw in ((A.empty((30, 40), seed=42), {}),                                    # another size
                      (A.empty((40, 30), seed=7), {}),                                     # another seed
                      (good, dict(seed=43)),
                      (good, dict(bucket_first=1, bucket_stride=2)),                       # another share
                      (A.empty((40, 30), seed=42, bucket_first=1, bucket_stride=2), {}),
                      (A(np.zeros((30, 40, 3), np.float32), 0, 42, (40, 30)), {}),         # not a state array
                      (A(np.zeros((30, 40, 4), np.float64), 0, 42, (40, 30)), {}),
                      (A(np.zeros((30, 40, 4), np.float32), -1, 42, (40, 30)), {})):
        with pytest.raises(ValueError):
            s.render_samples(4, state, **kw)
    with pytest.raises(ValueError):
        s.render_samples(0)
    with pytest.raises(TypeError):
        s.render_samples(4, np.zeros((30, 40, 4), np.float32))
    # good ones get as far as the missing upload
    for state, kw in ((None, {}), (good, {}), (A.empty((40, 30), seed=7, bucket_first=1, bucket_stride=3), dict(seed=7, bucket_first=1, bucket_stride=3))):
        with pytest.raises(fray.FrayError, match="beginRender"):
            s.render_samples(4, state, **kw)
    assert good.samples_done == 0
    s.close()


def test_cli_lists_the_accumulate_flags():
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, FRAYHIP_NO_TORCH="1"))
    assert out.returncode == 0, out.stderr
    for flag in ("--accumulate", "--noise-out"):
        assert flag in out.stdout, flag
    from fray_amd.__main__ import build_parser
    a = build_parser().parse_args(["scene.fray", "--accumulate", "s.npz", "--noise-out", "n.npy", "--spp", "4"])
    assert (a.accumulate, a.noise_out, a.spp) == ("s.npz", "n.npy", 4)
    assert build_parser().parse_args(["scene.fray"]).accumulate is None


def test_cli_refuses_a_state_of_another_size_before_the_upload(fray, tmp_path, capsys):
    from fray_amd.__main__ import main
    path = str(tmp_path / "state.npz")
    fray.Accumulation.empty((64, 48), seed=42).save(path)
    before = open(path, "rb").read()
    scene = os.path.join(SCENES, "cornell_box.fray")
    # device 99 does not exist: reaching beginRender would fail with another message and exit code
    with pytest.raises(SystemExit) as e:
        main([scene, "--width", "32", "--height", "24", "--accumulate", path, "--spp", "4", "--device", "99", "-o", str(tmp_path / "o.bmp")])
    assert e.value.code == 2
    assert "64 x 48" in capsys.readouterr().err
    assert open(path, "rb").read() == before and not os.path.exists(str(tmp_path / "o.bmp"))
    with pytest.raises(SystemExit):
        main([scene, "--noise-out", str(tmp_path / "n.npy")])                  # needs --accumulate


def test_accumulation_save_load_round_trip(fray, tmp_path):
    rng = np.random.default_rng(5)
    st = fray.Accumulation(rng.standard_normal((7, 9, 4)).astype(np.float32), samples_done=11, seed=2 ** 32 - 3, size=(9, 7), bucket_first=2, bucket_stride=5)
    path = st.save(tmp_path / "a.npz")
    back = fray.Accumulation.load(path)
    assert np.array_equal(back.state, st.state) and back.state.dtype == np.float32 and back.state.flags.c_contiguous
    assert (back.samples_done, back.seed, back.size, back.bucket_first, back.bucket_stride) == (11, 2 ** 32 - 3, (9, 7), 2, 5)
    back.check("test", (9, 7), 2 ** 32 - 3, 2, 5)
    np.savez(tmp_path / "other.npz", x=np.zeros(3))
    with pytest.raises(ValueError):
        fray.Accumulation.load(tmp_path / "other.npz")


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------

def test_constant_image_has_no_noise_and_a_flat_mean():
    # 0.375 and its multiples up to 16 are exact in FP32, so are their squares' sums: the variance is exactly 0
    c = np.full((16, 3, 4, 3), 0.375, F32)
    st = accumulate(c)
    assert np.all(st[..., :3] == F32(6.0)) and np.all(st[..., 3] == F32(16 * 0.375 * 0.375))
    rgb, noise = mean_and_noise(st, 16)
    assert np.all(rgb == F32(0.375)) and np.all(noise == 0)
    assert rgb.dtype == noise.dtype == st.dtype == F32


def test_variance_of_a_known_population_within_fp32_rounding():
    rng = np.random.default_rng(11)
    N = 64
    c = rng.uniform(0.0, 2.0, (N, 5, 6, 3)).astype(F32)
    rgb, noise = mean_and_noise(accumulate(c), N)
    l = ((c[..., 0].astype(np.float64) + c[..., 1]) + c[..., 2]) / 3.0
    want = l.var(axis=0) / (N - 1)                     # the population variance of the samples' luminance, over N - 1: the variance of the mean
    # Worst-case FP32 rounding, u = 2^-24, colours <= 2 so l <= 2 and l^2 <= 4:
    #   m2: N additions with partial sums <= 4N, each off by <= 4N u, plus the l_i^2 themselves (four operations, <= 32 u each): m2 / N is off by
    #       <= (4N + 33) u;
    #   a channel's sum: N additions with partial sums <= 2N: the mean is off by <= (2N + 2) u, so is lbar (plus 3 u), and lbar^2 by
    #       <= 2 * 2 * (2N + 5) u + 4 u;
    #   their difference (one more rounding of a value <= 4) is off by <= (12N + 61) u, and is divided by N - 1.
    u = 2.0 ** -24
    assert np.max(np.abs(noise.astype(np.float64) - want)) <= (12 * N + 61) * u / (N - 1) * (1 + u)
    assert np.max(np.abs(rgb.astype(np.float64) - c.astype(np.float64).mean(axis=0))) <= (2 * N + 2) * u
    assert np.all(noise > 0)


def test_any_split_into_prefixes_gives_the_same_state():
    rng = np.random.default_rng(12)
    c = (rng.standard_normal((12, 4, 5, 3)) * 3).astype(F32)
    whole = accumulate(c)
    for cuts in ((1,), (5,), (11,), (1, 2), (3, 5), (2, 4, 6, 8, 10), tuple(range(1, 12))):
        st = None
        for a, b in zip((0,) + cuts, cuts + (12,)):
            before = None if st is None else st.copy()
            new = accumulate(c[a:b], st)
            assert st is None or np.array_equal(st, before)          # the input state is left as it is
            st = new
        assert st.tobytes() == whole.tobytes(), cuts
    # the order of the samples matters in FP32, which is why the state is defined in sample order
    assert accumulate(c[::-1]).tobytes() != whole.tobytes()


def test_one_sample_is_as_uncertain_as_its_value():
    c = np.array([[[[0.5, 0.25, 1.5]], [[0.0, 0.0, 0.0]]]], F32)          # [1, 2, 1, 3]
    st = accumulate(c)
    rgb, noise = mean_and_noise(st, 1)
    assert np.array_equal(rgb, c[0])
    l = luminance(c[0])
    assert np.array_equal(noise, l * l) and noise[0, 0] == F32(0.75) * F32(0.75) and noise[1, 0] == 0
    assert np.array_equal(st[..., 3], l * l)
    # two equal samples: N = 2 takes the other branch and finds no spread
    _, n2 = mean_and_noise(accumulate(np.concatenate([c, c])), 2)
    assert np.all(n2 == 0)
    # a negative rounding residue is clamped, never reported as a negative variance
    bad = np.array([[[3.0, 3.0, 3.0, 2.9999998]]], F32)                  # m2 / 3 < lbar^2 = 1
    assert mean_and_noise(bad, 3)[1][0, 0] == 0
