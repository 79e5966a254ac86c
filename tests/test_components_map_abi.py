"""Component states under a sample map (include/frayhip.h "sample maps": frayhip_render_components_map, frayhip_sample_map_pair), what can be
checked without a GPU: the four entries are exported and mirrored and the ABI version has not moved; every argument check that needs no uploaded
scene answers FRAYHIP_E_ARG before the device is touched, with the entry's name in the message -- the second state's null, alignment and overlap
messages included; the Python side refuses bad values, mismatched pairs and unequal count planes; the CLI takes --refine with --denoise --split
and still refuses what it refused; and the numpy restatement of the pair map (tests/sample_map_pair_ref.py) reduces to the single-state one when
the indirect state is empty of light, and is symmetric in its two states."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import SCENES
from sample_map_pair_ref import sample_map_pair_ref
from sample_map_ref import sample_map_ref
from test_abi import header_functions

RENDER = ["frayhip_render_components_map", "frayhip_render_components_map_device"]
MAP = ["frayhip_sample_map_pair", "frayhip_sample_map_pair_device"]


def test_pair_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in RENDER + MAP:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n
    host, dev = (abi.SYMBOLS[n][1] for n in RENDER)
    one, one_dev = (abi.SYMBOLS[n][1] for n in ("frayhip_render_samples_map", "frayhip_render_samples_map_device"))
    # frayhip_render_samples_map's arguments with three more buffers (the second state and its two outputs); the stream before the stats
    assert len(host) == len(one) + 3 == 12 and len(dev) == len(one_dev) + 3 == 13
    assert host[:3] == one[:3] and host[-1] is one[-1] and dev[:3] == one_dev[:3] and dev[-2:] == one_dev[-2:]
    m, m_dev = (abi.SYMBOLS[n][1] for n in MAP)
    s, s_dev = (abi.SYMBOLS[n][1] for n in ("frayhip_sample_map", "frayhip_sample_map_device"))
    assert len(m) == len(s) + 1 and len(m_dev) == len(s_dev) + 1 and m[:2] == s[:2] and m[-3:] == s[-3:] and m_dev[-4:] == s_dev[-4:]
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning
    assert fray.lib.frayhip_sizeof(b"frayhip_samples_map") == C.sizeof(abi.SamplesMap) == 16          # no new struct: the single-state calls' own
    assert fray.lib.frayhip_sizeof(b"frayhip_sample_map") == C.sizeof(abi.SampleMap) == 40


@pytest.mark.parametrize("dev", [False, True])
def test_components_map_argument_checks(fray, abi, dev):
    L = fray.lib
    buf = (C.c_float * 96)()                    # carved into eight 16-byte aligned addresses; never dereferenced: every call ends before the device
    base = (C.addressof(buf) + 15) & ~15
    names = ("accum_direct", "accum_indirect", "count", "add", "rgb_direct", "rgb_indirect", "noise_direct", "noise_indirect")
    good = {n: base + 16 * k for k, n in enumerate(names)}
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)
    who = RENDER[1] if dev else RENDER[0]

    def call(f, m, **over):
        a = dict(good, **over)
        fp = C.byref(f) if f is not None else None
        mp = C.byref(m) if m is not None else None
        args = [a[n] for n in names]
        if dev:
            return L.frayhip_render_components_map_device(None, fp, mp, *args, None, None)
        return L.frayhip_render_components_map(None, fp, mp, *args, None)

    def expect(rc, words):
        assert rc == abi.E_ARG
        msg = L.frayhip_last_error().decode()
        assert words in msg and msg.startswith(who + ":"), msg

    m = abi.SamplesMap()
    expect(call(None, m), "null frame")
    expect(call(fr, None), "null request")
    expect(call(fr, m, accum_direct=None), "null accum_direct")
    expect(call(fr, m, accum_indirect=None), "null accum_indirect")
    expect(call(fr, m, count=None), "null count")
    expect(call(fr, m, add=None), "null add")
    expect(call(abi.Frame(mode=abi.MODE_PRIMARY_ID, seed=42), m), "mode must be")
    # two buffers at one address overlap whatever the frame's size: every pair of the eight, named as the header names the arguments
    for j in range(1, 8):
        for i in range(j):
            expect(call(fr, m, **{names[j]: good[names[i]]}), "%s must not overlap %s" % (names[j], names[i]))
    if dev:
        expect(call(fr, m, accum_direct=good["accum_direct"] + 4), "16-byte aligned")
        expect(call(fr, m, accum_indirect=good["accum_indirect"] + 8), "16-byte aligned")
        for n in names[2:]:
            expect(call(fr, m, **{n: good[n] + 2}), "4-byte aligned")
    # good arguments, and the optional outputs left out, get as far as the missing scene
    expect(call(fr, m), "null scene")
    expect(call(fr, m, rgb_direct=None, rgb_indirect=None, noise_direct=None, noise_indirect=None), "null scene")
    expect(call(fr, m, rgb_indirect=None, noise_direct=None), "null scene")


@pytest.mark.parametrize("dev", [False, True])
def test_sample_map_pair_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 2
    n = W * H
    buf = (C.c_float * (n * 10 + 8))()
    direct = (C.addressof(buf) + 15) & ~15
    indirect, count, add = direct + n * 16, direct + n * 32, direct + n * 36
    who = MAP[1] if dev else MAP[0]

    def params(**kw):
        p = abi.SampleMap(tolerance=0.05, lum_floor=0.01, min_count=4, max_count=64, max_add=1 << 24, grow=2)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(p, W=W, H=H, direct=direct, indirect=indirect, count=count, add=add):
        pp = C.byref(p) if p is not None else None
        if dev:
            return L.frayhip_sample_map_pair_device(W, H, direct, indirect, count, pp, add, None, None)
        return L.frayhip_sample_map_pair(W, H, direct, indirect, count, pp, add, None)

    def expect(rc, words):
        assert rc == abi.E_ARG
        msg = L.frayhip_last_error().decode()
        assert words in msg and msg.startswith(who + ":"), msg

    ok = params()
    expect(call(ok, W=0), "width and height")
    expect(call(ok, H=-1), "width and height")
    expect(call(ok, W=1 << 16, H=(1 << 14) + 1), "2^30")
    expect(call(ok, direct=None), "null accum_direct")
    expect(call(ok, indirect=None), "null accum_indirect")
    expect(call(ok, count=None), "null count")
    expect(call(None), "null parameters")
    expect(call(ok, add=None), "null add")
    for t in (0.0, -0.05, math.inf, math.nan):
        expect(call(params(tolerance=t)), "tolerance must be")
        expect(call(params(lum_floor=t)), "lum_floor must be")
    expect(call(params(min_count=0)), "min_count must be")
    expect(call(params(min_count=8, max_count=7)), "max_count must be >= min_count")
    expect(call(params(max_count=(1 << 24) + 1)), "2^24")
    expect(call(params(max_add=0)), "max_add must be")
    for g in (1, 17):
        expect(call(params(grow=g)), "grow must be")
    # the overlaps among the four buffers
    expect(call(ok, add=direct), "add must not overlap")
    expect(call(ok, add=indirect + 16), "add must not overlap")
    expect(call(ok, add=count + 4), "add must not overlap")
    expect(call(ok, indirect=direct + 16), "accum_indirect must not overlap accum_direct")
    expect(call(ok, count=direct + 16), "count must not overlap accum_direct")
    expect(call(ok, count=indirect + 16), "count must not overlap accum_indirect")
    if dev:
        expect(call(ok, direct=direct + 8), "16-byte aligned")
        expect(call(ok, indirect=indirect + 8), "16-byte aligned")
        expect(call(ok, count=count + 2), "4-byte aligned")
        expect(call(ok, add=add + 2), "4-byte aligned")


def test_python_refuses_bad_values_and_mismatched_pairs(fray):
    s = fray.Scene.parseScene(os.path.join(SCENES, "cornell_box.fray"))       # parsed, not uploaded
    W, H = s.frame_size
    add = np.ones((H, W), np.int32)
    pair = lambda **kw: (fray.Accumulation.empty((W, H), **kw), fray.Accumulation.empty((W, H), **kw))
    with pytest.raises(TypeError):
        s.render_components_map(add.astype(np.int64))
    with pytest.raises(TypeError):
        s.render_components_map(add.astype(np.float32))
    with pytest.raises(ValueError):
        s.render_components_map(add[:-1])
    with pytest.raises(TypeError, match="pair"):
        s.render_components_map(add, state=fray.Accumulation.empty((W, H)))
    with pytest.raises(TypeError, match="pair"):
        s.render_components_map(add, state=(fray.Accumulation.empty((W, H)), np.zeros((H, W, 4), np.float32)))
    with pytest.raises(ValueError, match="seed"):
        s.render_components_map(add, pair(seed=7), seed=8)
    d, i = pair()
    with pytest.raises(ValueError, match="same object"):
        s.render_components_map(add, (d, d))
    i.state = np.zeros((H + 1, W, 4), np.float32)
    with pytest.raises(ValueError, match="shaped"):
        s.render_components_map(add, (d, i))
    d, i = pair()
    i.counts = np.zeros((H, W), np.int64)
    with pytest.raises(ValueError, match="counts"):
        s.render_components_map(add, (d, i))
    # unequal count planes: uniform against uniform, and a plane against a uniform state
    d, i = pair()
    i.samples_done = 2
    with pytest.raises(ValueError, match="count planes must be equal"):
        s.render_components_map(add, (d, i))
    d, i = pair()
    d.counts = np.zeros((H, W), np.int32)
    d.counts[3, 5] = 1
    with pytest.raises(ValueError, match="count planes must be equal"):
        s.render_components_map(add, (d, i))
    with pytest.raises(ValueError, match="count planes must be equal"):
        fray.sample_map((d, i), max_count=8)
    # equal non-uniform planes are what this call is for: they get as far as the missing upload (render_components still refuses them)
    i.counts = d.counts.copy()
    with pytest.raises(fray.FrayError, match="beginRender"):
        s.render_components_map(add, (d, i))
    with pytest.raises(ValueError, match="different numbers of samples"):
        s.render_components(1, (d, i))
    with pytest.raises(fray.FrayError, match="beginRender"):
        s.render_components_map(add)
    # sample_map and refine with a pair
    with pytest.raises(TypeError):
        fray.sample_map((d, np.zeros((H, W, 4), np.float32)), max_count=8)
    with pytest.raises(ValueError, match="max_count"):
        fray.sample_map((d, i))
    with pytest.raises(TypeError, match="split"):
        s.refine(fray.Accumulation.empty((W, H)), 0.1, 8, split=True)
    with pytest.raises(ValueError, match="max_count"):
        s.render_denoised_split(refine=0.1)
    with pytest.raises(ValueError, match="refine"):
        s.render_denoised_split(max_count=8)
    s.close()


def test_cli_takes_refine_with_split_and_still_refuses_the_rest(capsys):
    from fray_amd.__main__ import build_parser, check_args
    ap = build_parser()
    for extra in ([], ["--components-out", "c.npz"], ["--features-out", "f.npy"]):
        a = ap.parse_args(["scene.fray", "--refine", "0.1", "--max-spp", "32", "--denoise", "--split"] + extra)
        assert (a.refine, a.max_spp, a.denoise, a.split) == (0.1, 32, True, True)
        check_args(ap, a)
    base = ["scene.fray", "--refine", "0.1", "--max-spp", "32"]
    for argv, words in ((base + ["--split"], "--split needs --denoise"),
                        (base + ["--components-out", "c.npz"], "--components-out"),
                        (base + ["--denoise", "--components-out", "c.npz"], "--components-out"),
                        (base + ["--denoise", "--split", "--accumulate", "a.npz"], "--accumulate"),
                        (base + ["--denoise", "--split", "--noise-out", "n.npy"], "--noise-out"),
                        (base + ["--denoise", "--split", "--adaptive", "0.1"], "--adaptive"),
                        (base + ["--denoise", "--split", "--frames", "3"], "--frames"),
                        (base + ["--denoise", "--split", "--time-limit", "1"], "--time-limit"),
                        (base + ["--denoise", "--split", "--progress"], "--progress"),
                        (base + ["--denoise", "--split", "--probe", "1", "1"], "--probe"),
                        (["scene.fray", "--refine", "0.1", "--denoise", "--split"], "--max-spp"),
                        (["scene.fray", "--max-spp", "8", "--denoise", "--split"], "--max-spp needs --refine")):
        with pytest.raises(SystemExit) as e:
            check_args(ap, ap.parse_args(argv))
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert words in err, (argv, err)


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------

def states(seed, H=23, W=31):
    """A state with counts 0 .. 69 and every kind of row: quiet, noisy, dark, NaN, infinite second moment."""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, 70, (H, W)).astype(np.int32)
    lum = rng.random((H, W), dtype=np.float32) * np.float32(2.0)
    var = rng.random((H, W), dtype=np.float32) ** 4
    n = count.astype(np.float32)
    state = np.stack([n * lum, n * lum * np.float32(0.5), n * lum * np.float32(1.5), n * (var + lum * lum)], axis=-1).astype(np.float32)
    state[1, :, 3] = state[1, :, 0] * state[1, :, 0] / np.maximum(n[1], 1)
    state[2, :, :3] *= np.float32(1e-4)
    state[3, ::2] = np.float32(np.nan)
    state[4, :, 3] = np.float32(1e30)
    state[5, :, 3] = np.inf
    return state, count


PARAMS = [dict(tolerance=0.05, max_count=64), dict(tolerance=0.2, max_count=64, grow=16, max_add=5),
          dict(tolerance=0.5, lum_floor=0.5, min_count=1, max_count=48, grow=3)]


@pytest.mark.parametrize("params", PARAMS, ids=["defaults", "caps", "floor"])
def test_pair_ref_with_an_empty_indirect_state_is_the_single_state_map(params):
    state, count = states(3)
    count[0, :8] = [0, 1, 4, 64, 65, 2, 3, 63]
    want = sample_map_ref(state, count, **params)
    got = sample_map_pair_ref(state, np.zeros_like(state), count, **params)
    assert got[0].dtype == np.int32 and got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:]
    assert len(np.unique(want[0])) >= 4


@pytest.mark.parametrize("params", PARAMS, ids=["defaults", "caps", "floor"])
def test_pair_ref_is_symmetric_and_differs_from_either_state_alone(params):
    a, count = states(4)
    b, _ = states(5)
    b[..., :] *= np.float32(0.37)
    ab = sample_map_pair_ref(a, b, count, **params)
    ba = sample_map_pair_ref(b, a, count, **params)
    assert ab[0].tobytes() == ba[0].tobytes() and ab[1:] == ba[1:]
    assert (ab[0] != sample_map_ref(a, count, **params)[0]).any() and (ab[0] != sample_map_ref(b, count, **params)[0]).any()


def test_pair_ref_worked_case():
    # N = 8; direct: grey 1.0 with v = 0.5, indirect: grey 0.5 with v = 0.25.  lbar = 1.5, noise = 0.5 / 7 + 0.25 / 7 = 0.75 / 7;
    # t = 0.25 * 1.5 = 0.375, need = ceil(8 * (0.75 / 7) / 0.140625) = ceil(6.095...) = 7 -> target max(8, 7) = 8 -> add 0
    row = lambda lum, N, var: [N * lum, N * lum, N * lum, N * (var + lum * lum)]
    d = np.array([[row(1.0, 8, 0.5)]], np.float32)
    i = np.array([[row(0.5, 8, 0.25)]], np.float32)
    c = np.array([[8]], np.int32)
    assert sample_map_pair_ref(d, i, c, tolerance=0.25, min_count=4, max_count=64)[0][0, 0] == 0
    # tolerance 0.125: t = 0.1875, need = ceil(8 * (0.75 / 7) / 0.03515625) = ceil(24.38) = 25 > 2 * 8 -> 16 -> add 8; grow 4 -> 25 -> add 17
    assert sample_map_pair_ref(d, i, c, tolerance=0.125, min_count=4, max_count=64)[0][0, 0] == 8
    assert sample_map_pair_ref(d, i, c, tolerance=0.125, min_count=4, max_count=64, grow=4)[0][0, 0] == 17
