"""CPU: the definition of the step's input noise (tests/noise_restatement.py) -- Random123's known answers, the moments and the
independence of its streams -- and the host side of the feature: NoiseSpec, DeviceClipStore.field_std() on a CPU store, the signatures."""
import dataclasses
import inspect
import os

import numpy as np
import pytest
import torch

from tests import noise_restatement as NR

SAMPLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")
FILES = [os.path.join(SAMPLES, "sample_1.hdf5"), os.path.join(SAMPLES, "sample_2.hdf5")]
N = 1 << 20
BOUND = 5.0            # standard errors: the condition, not a measurement


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_reproduces_the_known_answers(counter, key, want):
    got = NR.philox4x32_10(counter, key)
    assert " ".join("%08x" % int(v) for v in got) == want


def test_counter_words_and_word_use():
    """Element 4g + j of a sample comes from the Philox call with counter {g, sample, draw, pass} and the seed's two words as the key:
    words (0, 1) serve j = 0, 1 and words (2, 3) serve j = 2, 3; a size that is no multiple of 4 uses the leading words of its last group."""
    seed, sample, draw, pas = (7 << 32) | 9, 2 ** 31 + 3, 2 ** 32 - 1, 3
    z, r = NR.normals(seed, sample, draw, pas, 10)
    w = NR.philox4x32_10((2, sample, draw, pas), (9, 7))
    z0, z1, ra = NR.box_muller(w[0], w[1])
    assert z[8] == z0 and z[9] == z1 and r[8] == r[9] == ra
    full, _ = NR.normals(seed, sample, draw, pas, 12)
    assert np.array_equal(full[:10], z)
    assert np.array_equal(NR.normals(seed, sample + 2 ** 32, draw, pas, 12)[0], full)      # ids count modulo 2^32


@pytest.mark.parametrize("sample,draw,pas", [(0, 1, 0), (5, 1, 0), (5, 2, 0), (5, 1, 1)])
def test_moments_of_a_stream(sample, draw, pas):
    z, _ = NR.normals(42, sample, draw, pas, N)
    st = NR.moment_statistics(z)
    print({k: round(float(v), 3) for k, v in st.items()}, "max |z| %.4f" % np.abs(z).max())
    assert all(abs(v) <= BOUND for v in st.values()), st
    assert np.abs(z).max() <= NR.Z_MAX


def test_streams_are_uncorrelated():
    a, _ = NR.normals(42, 5, 1, 0, N)
    for what, (seed, sample) in {"sample 6": (42, 6), "seed 43": (43, 5)}.items():
        b, _ = NR.normals(seed, sample, 1, 0, N)
        c = float((a * b).mean() * np.sqrt(N))
        print(what, round(c, 3))
        assert abs(c) <= BOUND, (what, c)
        assert not np.array_equal(a, b)


def test_noise_spec_validation():
    from bubbleformer_amd.utils import NoiseSpec
    s = NoiseSpec(0.1)
    assert s.active and not s.relative and s.seed == 0 and s.passes == "all" and s.sigma(3) == [0.1] * 3
    assert [s.perturbs(j) for j in range(3)] == [True, True, True]
    assert [NoiseSpec(0.1, passes="input").perturbs(j) for j in range(3)] == [True, False, False]
    assert [NoiseSpec(0.1, passes="fed_back").perturbs(j) for j in range(3)] == [False, True, True]
    off = NoiseSpec(std=0.0)
    assert not off.active and not any(off.perturbs(j) for j in range(3)) and not NoiseSpec([0.0, 0]).active
    per = NoiseSpec([0.5, 0.0, 2.0], relative=True, seed=2 ** 63 + 42)
    assert per.std == (0.5, 0.0, 2.0) and per.active
    assert per.sigma(3, [2.0, 3.0, 0.25]) == [1.0, 0.0, 0.5]
    with pytest.raises(ValueError, match="fit"):
        per.sigma(3)
    with pytest.raises(ValueError):
        per.sigma(4, [1.0] * 4)
    with pytest.raises(ValueError):
        per.sigma(3, [1.0, float("nan"), 1.0])
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.seed = 1
    for bad in (dict(std=-0.1), dict(std=float("nan")), dict(std=float("inf")), dict(std=[0.1, -1.0]), dict(std=[]), dict(std="0.1"), dict(std=None),
                dict(std=True), dict(std=0.1, passes="both"), dict(std=0.1, seed=1.5), dict(std=0.1, seed=None), dict(std=0.1, relative=1)):
        with pytest.raises(ValueError):
            NoiseSpec(**bad)


@pytest.mark.parametrize("norm", ["none", "std"])
def test_field_std_of_a_cpu_store_is_numpys_pooled_deviation(norm):
    from bubbleformer_amd.data import BubbleForecast
    from bubbleformer_amd.data import hdf5_lite
    d = BubbleForecast(FILES, norm=norm, time_window=4, start_time=5)
    d.normalize()
    got = d.device_store("cpu").field_std()
    assert sorted(got) == sorted(d.fields)
    for name in d.fields:
        pooled = np.concatenate([np.asarray(hdf5_lite.File(f, "r")[name][...], dtype=np.float32).astype(np.float64).reshape(-1) for f in FILES])
        want = pooled.std() / float(d.div_terms[name])      # norm="none": 1 + 1e-8, the constant the gather divides by
        assert abs(got[name] - want) <= 1e-12 * abs(want), (name, got[name], want)
        if norm == "std":
            assert 0.5 < got[name] < 2.0        # the pooled deviation over the mean of the files' deviations


def test_signatures_accept_the_new_keywords():
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import NoiseSpec, add_gaussian_noise
    from bubbleformer_amd.utils.noise import add_gaussian_noise as direct
    assert add_gaussian_noise is direct
    p = inspect.signature(TrainStep.__init__).parameters
    assert p["input_noise"].default is None and p["field_std"].default is None
    assert inspect.signature(TrainStep.__call__).parameters["sample_ids"].default is None
    assert inspect.signature(fit).parameters["input_noise"].default is None
    assert list(inspect.signature(add_gaussian_noise).parameters) == ["clip", "sigma", "sample_ids", "draw", "pass_index", "seed", "out"]
    assert [f.name for f in dataclasses.fields(NoiseSpec)] == ["std", "relative", "seed", "passes"]


def test_relative_noise_needs_the_field_deviations_and_cpu_clips_are_refused():
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils import NoiseSpec, add_gaussian_noise
    with pytest.raises(ValueError, match="fit"):
        TrainStep(torch.nn.Linear(2, 2), input_noise=NoiseSpec(0.1, relative=True))
    with pytest.raises(ValueError, match="NoiseSpec"):
        TrainStep(torch.nn.Linear(2, 2), input_noise=0.1)
    with pytest.raises(L.BubbleformerHipError, match="no CPU fallback"):
        add_gaussian_noise(torch.zeros(1, 1, 1, 2, 2), 0.1)
