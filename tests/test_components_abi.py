"""Component frames (include/frayhip.h "component frames"), what can be checked without a GPU: both entry points are exported, declared and
mirrored and the ABI version has not moved; every argument check that needs no uploaded scene answers FRAYHIP_E_ARG with the entry's name before
the device is touched; the Python side refuses pairs of states that disagree or belong to another frame; the CLI lists its flags and refuses what
it does not render; and the numpy restatement of the split (tests/components_ref.py) behaves as the header says on synthetic term lists."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from components_ref import accumulate, fold, mean_and_noise, split
from conftest import ROOT, SCENES
from test_abi import header_functions

ENTRIES = ["frayhip_render_components", "frayhip_render_components_device"]
F32 = np.float32


def test_components_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n
    host, dev = (abi.SYMBOLS[n][1] for n in ENTRIES)
    samples, samples_dev = (abi.SYMBOLS[n][1] for n in ("frayhip_render_samples", "frayhip_render_samples_device"))
    # frayhip_render_samples' arguments with six buffers in place of three; the device entry has the stream before the stats
    assert len(host) == len(samples) + 3 == 11 and len(dev) == len(samples_dev) + 3 == 12
    assert host[:4] == samples[:4] and host[-1] is samples[-1] and dev[:4] == samples_dev[:4] and dev[-2:] == samples_dev[-2:]
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning
    header = open(os.path.join(ROOT, "include", "frayhip.h")).read()
    assert "component frames" in header and "#define FRAYHIP_ABI_VERSION 3" in header


@pytest.mark.parametrize("dev", [False, True])
def test_components_argument_checks(fray, abi, dev):
    L = fray.lib
    name = ENTRIES[1] if dev else ENTRIES[0]
    # addresses, 16-byte aligned and far apart; never dereferenced: every call below ends before the device is touched
    D, I = 1 << 20, 1 << 24
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)

    def req(first=0, count=4):
        return abi.Samples(sample_first=first, sample_count=count)

    def call(f=fr, r=None, p=None, d=D, i=I, rgb_d=None, rgb_i=None, noise_d=None, noise_i=None):
        fp = C.byref(f) if f is not None else None
        rp = C.byref(r) if r is not None else None
        pp = C.byref(p) if p is not None else None
        if dev:
            return L.frayhip_render_components_device(None, fp, rp, pp, d, i, rgb_d, rgb_i, noise_d, noise_i, None, None)
        return L.frayhip_render_components(None, fp, rp, pp, d, i, rgb_d, rgb_i, noise_d, noise_i, None)

    def expect(rc, words):
        assert rc == abi.E_ARG
        msg = L.frayhip_last_error().decode()
        assert words in msg and msg.startswith(name + ":"), msg

    expect(call(f=None, r=req()), "null frame")
    expect(call(r=None), "null request")
    expect(call(r=req(), d=None), "null accum_direct")
    expect(call(r=req(), i=None), "null accum_indirect")
    expect(call(f=abi.Frame(mode=abi.MODE_PRIMARY_ID, seed=42), r=req()), "mode must be")
    for first in (-1, -2 ** 31):
        expect(call(r=req(first=first)), "sample_first must be >= 0")
    for count in (0, -3):
        expect(call(r=req(count=count)), "sample_count must be >= 1")
    for first, count in ((2 ** 24, 1), (1, 2 ** 24), (2 ** 31 - 1, 2 ** 31 - 1)):
        expect(call(r=req(first, count)), "2^24")
    expect(call(r=req(), p=abi.Progressive(preview_ms=math.nan)), "preview_ms")
    # previews are not offered
    for ms in (0.0, 1.0, math.inf):
        expect(call(r=req(), p=abi.Progressive(preview_ms=ms)), "previews are not offered")
    if dev:
        expect(call(r=req(), d=D + 4), "16-byte aligned")
        expect(call(r=req(), i=I + 8), "16-byte aligned")
        for kw in (dict(rgb_d=D + 2), dict(rgb_i=I + 2), dict(noise_d=D + 1), dict(noise_i=I + 3)):
            expect(call(r=req(), **kw), "4-byte aligned")
    # two buffers at one address overlap whatever the frame's size (ranges that merely intersect need the size: checked with the scene)
    expect(call(r=req(), i=D), "accum_indirect must not overlap accum_direct")
    expect(call(r=req(), rgb_d=I), "rgb_direct must not overlap accum_indirect")
    expect(call(r=req(), rgb_d=1 << 26, rgb_i=1 << 26), "rgb_indirect must not overlap rgb_direct")
    expect(call(r=req(), noise_i=D), "noise_indirect must not overlap accum_direct")
    expect(call(r=req(), noise_d=1 << 26, noise_i=1 << 26), "noise_indirect must not overlap noise_direct")
    # the extreme legal values pass every check that needs no scene
    expect(call(r=req(0, 2 ** 24)), "null scene")
    expect(call(r=req(2 ** 24 - 1, 1), p=abi.Progressive(preview_ms=-1.0)), "null scene")
    expect(call(r=req(), rgb_d=1 << 26, rgb_i=1 << 27, noise_d=1 << 28, noise_i=1 << 29), "null scene")


def test_python_refuses_states_that_disagree_without_a_gpu(fray):
    s = fray.Scene.parseScene(os.path.join(SCENES, "cornell_box.fray"))       # parsed, not uploaded
    s.settings.frameWidth, s.settings.frameHeight = 40, 30
    A = fray.Accumulation

    def good(**kw):
        return A.empty((40, 30), **dict(dict(seed=42), **kw))
    one = good()
    for state, kw in (((good(), A.empty((30, 40), seed=42)), {}),                               # sizes
                      ((A.empty((30, 40), seed=42), A.empty((30, 40), seed=42)), {}),           # both of another frame
                      ((good(), good(seed=7)), {}),                                             # seeds
                      ((good(seed=7), good(seed=7)), {}),
                      ((good(), good()), dict(seed=43)),
                      ((good(), good(bucket_first=1, bucket_stride=2)), {}),                    # shares
                      ((good(), good()), dict(bucket_first=1, bucket_stride=2)),
                      ((good(), A(np.zeros((30, 40, 4), np.float32), 3, 42, (40, 30))), {}),    # samples_done
                      ((good(), A(np.zeros((30, 40, 3), np.float32), 0, 42, (40, 30))), {}),    # not a state array
                      ((A(np.zeros((30, 40, 4), np.float64), 0, 42, (40, 30)), good()), {}),
                      ((one, one), {}),                                                         # one state twice
                      ((one, A(one.state, 0, 42, (40, 30))), {})):
        with pytest.raises(ValueError):
            s.render_components(4, state, **kw)
    with pytest.raises(ValueError):
        s.render_components(0)
    for state in (good(), (good(),), (good(), good(), good()), (good(), np.zeros((30, 40, 4), np.float32))):
        with pytest.raises(TypeError):
            s.render_components(4, state)
    # good ones get as far as the missing upload
    for state, kw in ((None, {}), ((good(), good()), {}), ([good(seed=7, bucket_first=1, bucket_stride=3), good(seed=7, bucket_first=1, bucket_stride=3)],
                                                           dict(seed=7, bucket_first=1, bucket_stride=3))):
        with pytest.raises(fray.FrayError, match="beginRender"):
            s.render_components(4, state, **kw)
    # the split filter takes the states' noise as it is: demodulate=1 is refused before anything is rendered, and so is an unknown parameter
    with pytest.raises(ValueError, match="demodulate"):
        s.render_denoised_split(demodulate=1)
    with pytest.raises(TypeError):
        s.render_denoised_split(sigma_colour=1.0)
    with pytest.raises(fray.FrayError, match="beginRender"):
        s.render_denoised_split(demodulate=0)
    s.close()


def test_cli_lists_the_component_flags_and_refuses_what_it_does_not_render(capsys):
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, FRAYHIP_NO_TORCH="1"))
    assert out.returncode == 0, out.stderr
    for flag in ("--components-out", "--split"):
        assert flag in out.stdout, flag
    from fray_amd.__main__ import build_parser, main
    a = build_parser().parse_args(["scene.fray", "--denoise", "--split", "--components-out", "c.npz"])
    assert (a.denoise, a.split, a.components_out) == (True, True, "c.npz")
    a = build_parser().parse_args(["scene.fray"])
    assert a.split is False and a.components_out is None
    cornell, boxed = os.path.join(SCENES, "cornell_box.fray"), os.path.join(SCENES, "boxed.fray")

    def refused(argv, words):
        # device 99 does not exist: reaching beginRender would fail with another message and exit code
        with pytest.raises(SystemExit) as e:
            main(argv + ["--device", "99"])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert words in err, err
    refused([cornell, "--denoise", "--split", "--adaptive", "0.05"], "--adaptive")
    refused([cornell, "--split"], "--split needs --denoise")
    refused([boxed, "--denoise", "--split"], "path-traced")                                   # gi off
    refused([boxed, "--components-out", "c.npz"], "path-traced")


def test_cli_refuses_a_stereo_scene_before_the_upload(fray, capsys):
    from fray_amd.__main__ import build_parser, check_components
    s = fray.Scene.parseScene(os.path.join(SCENES, "cornell_box.fray"))
    ap = build_parser()
    for argv in (["--denoise", "--split"], ["--components-out", "c.npz"]):
        a = ap.parse_args(["scene.fray"] + argv)
        s.camera.stereoSeparation = 0.0
        check_components(ap, a, s)                                  # a mono path-traced scene passes
        s.camera.stereoSeparation = 12.0
        with pytest.raises(SystemExit) as e:
            check_components(ap, a, s)
        assert e.value.code == 2 and "stereo" in capsys.readouterr().err
    check_components(ap, ap.parse_args(["scene.fray"]), s)          # without the flags nothing is asked of the scene
    s.close()


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------

def term_lists(n, rng, shape=(5, 7)):
    """n terms per pixel with magnitudes spread over many binades, so that every addition rounds; some exact zeros of both signs."""
    t = (rng.standard_normal((n,) + shape + (3,)) * np.exp2(rng.integers(-12, 6, (n,) + shape + (1,)))).astype(F32)
    t[rng.random(t.shape) < 0.1] = F32(0.0)
    t[rng.random(t.shape) < 0.1] = F32(-0.0)
    return t


@pytest.mark.parametrize("n", [1, 2, 8, 9, 23])
def test_direct_plus_indirect_is_the_fold_bit_for_bit(n):
    rng = np.random.default_rng(100 + n)
    t = term_lists(n, rng)
    before = t.copy()
    d, ind = split(t)
    assert d.dtype == ind.dtype == F32 and t.tobytes() == before.tobytes()
    assert (d + ind).tobytes() == fold(t).tobytes()
    assert d.tobytes() == t[0].tobytes()                       # stored as it is, the sign of a zero included
    if n == 1:
        assert ind.tobytes() == np.zeros_like(d).tobytes()     # +0
    else:
        assert ind.tobytes() == fold(t[1:]).tobytes()
        assert np.any(ind != 0)


@pytest.mark.parametrize("n", [1, 2, 8, 9, 23])
def test_negative_zero_terms(n):
    t = np.full((n, 2, 2, 3), -0.0, F32)
    d, ind = split(t)
    assert np.all(np.signbit(d))                               # d keeps the sign
    assert np.all(ind == 0) and not np.any(np.signbit(ind))    # n is +0: the fold starts at +0, and -0 + +0 = +0
    c = fold(t)
    assert (d + ind).tobytes() == c.tobytes() and not np.any(np.signbit(c))
    # in a state the sign is gone: the sum starts at +0
    st = accumulate(d[None])
    assert st.tobytes() == np.zeros((2, 2, 4), F32).tobytes()


def test_states_of_the_components_add_up_only_per_sample():
    """The per-sample identity is exact; the sums of N samples are not d-sum + n-sum = c-sum in FP32, which is why it is stated per sample."""
    rng = np.random.default_rng(7)
    N = 12
    terms = [term_lists(int(n), rng) for n in rng.integers(1, 10, N)]
    d, ind = (np.stack(x) for x in zip(*(split(t) for t in terms)))
    c = np.stack([fold(t) for t in terms])
    assert (d + ind).tobytes() == c.tobytes()
    sd, si, sc = accumulate(d), accumulate(ind), accumulate(c)
    assert np.allclose(sd[..., :3] + si[..., :3], sc[..., :3], rtol=1e-4, atol=1e-4)
    rgb_d, noise_d = mean_and_noise(sd, N)
    assert rgb_d.dtype == noise_d.dtype == F32 and np.all(noise_d >= 0)
    # cut anywhere, the states are the same
    assert accumulate(d[5:], accumulate(d[:5])).tobytes() == sd.tobytes()
