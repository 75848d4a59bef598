"""bench.py --dump-outputs: the sample of the last step's ciphertexts (torus_sample) is fixed, within its budget, exact where it
converts and keeps every ciphertext's body word"""
import importlib.util
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _words(shape, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 64, shape, dtype=np.uint64)


def test_small_output_is_written_whole_as_torus_fractions():
    words = _words((2, 16, 8, 513))
    got = _bench().torus_sample(words, 1 << 20)
    assert got.dtype == np.float64 and got.shape == words.shape
    assert np.array_equal(got, words.astype(np.float64) * 2.0 ** -64)
    assert np.all((got >= 0) & (got <= 1))


def test_large_output_keeps_every_body_and_a_fixed_choice_of_mask_words():
    bench = _bench()
    words = _words((3, 16, 8, 2049))
    budget = 3 * 128 * 100
    got = bench.torus_sample(words, budget)
    assert got.shape == (3, 16, 8, 100) and got.size <= budget
    assert np.array_equal(got[..., -1], words[..., -1].astype(np.float64) * 2.0 ** -64)
    # the same columns for every ciphertext, the same columns on every call
    row = words[0, 0, 0].astype(np.float64) * 2.0 ** -64
    cols = [int(np.flatnonzero(row == v)[0]) for v in got[0, 0, 0]]
    assert cols == sorted(set(cols)) and cols[-1] == 2048
    assert np.array_equal(got[2, 15, 7], words[2, 15, 7, cols].astype(np.float64) * 2.0 ** -64)
    assert np.array_equal(got, bench.torus_sample(words.copy(), budget))
    assert bench.DUMP_BYTES <= 64_000_000


def test_more_ciphertexts_than_budget_gives_one_body_word_each_of_a_fixed_choice():
    bench = _bench()
    words = _words((4, 16, 8, 17))
    got = bench.torus_sample(words, 100)
    assert got.shape == (100, 1)
    bodies = words.reshape(-1, 17)[:, -1].astype(np.float64) * 2.0 ** -64
    assert np.isin(got[:, 0], bodies).all()
    assert np.array_equal(got, bench.torus_sample(words, 100))
