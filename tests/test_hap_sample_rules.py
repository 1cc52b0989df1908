"""The rules of the training sample list (tests/hap_sample_rules.py) held against their sources: Philox4x32-10 against known answers - in
numpy and in nanosnp_amd/csrc/nsnp_philox.hpp compiled for the host under the address and undefined-behaviour sanitizers - and the block
rules against TrainingDataset.__init__ (HaplotypeModel/dataset_dev.py:190-230) as include/nanosnp.h states them."""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import hap_sample_rules as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PN_VALUES = (0.0, 0.7, 1.0, 2.5)
FLOAT_TRAPS = (90, 170, 180, 330, 340, 350, 360, 650, 660, 670)          # int(len * 0.7) is one less than len * 7 // 10


def test_philox_known_answers():
    for counter, key, want in sr.KNOWN_ANSWERS:
        assert tuple(int(v) for v in sr.philox4x32_10(counter, key)) == want
    many = sr.philox4x32_10((np.arange(5), 3, 9, 0), (17, 1))              # arrays give what scalars give
    for j in range(5):
        assert [int(w[j]) for w in many] == [int(v) for v in sr.philox4x32_10((j, 3, 9, 0), (17, 1))]


def test_philox_header_on_the_host_under_sanitizers(tmp_path):
    """nsnp_philox.hpp is plain C++: built here by the host compiler with -fsanitize=address,undefined as a program of its own"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "philox_kat")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []      # the runtimes inside the program itself
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                   + static + ["-I", os.path.join(ROOT, "nanosnp_amd", "csrc"),
                               os.path.join(ROOT, "tests", "helpers_native", "philox_kat.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    rng = np.random.default_rng(32)
    cases = [(c, k) for c, k, _ in sr.KNOWN_ANSWERS] + [(tuple(int(v) for v in rng.integers(0, 1 << 32, 4)),
                                                        tuple(int(v) for v in rng.integers(0, 1 << 32, 2))) for _ in range(5)]
    args = [f"{w:x}" for c, k in cases for w in c + k]
    run = subprocess.run([exe] + args, check=True, capture_output=True, text=True)
    assert run.stderr == ""
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for line, (c, k) in zip(lines, cases):
        want = [int(v) for v in sr.philox4x32_10(c, k)]
        got = line.split()
        assert [int(v, 16) for v in got[:4]] == want
        assert int(got[4]) == (want[0] * 0x9e3779b1) >> 32
    for line, (_, _, want) in zip(lines, sr.KNOWN_ANSWERS):
        assert line.split()[:4] == [f"{v:08x}" for v in want]


@pytest.mark.parametrize("n_ref,want", [(0, []), (1, [1]), (999, [999]), (1000, [1000]), (1001, [1000, 1]), (2000, [1000, 1000]),
                                         (2001, [1000, 1000, 1])])
def test_block_cut(n_ref, want):
    assert sr.block_lengths(n_ref) == want
    assert len(want) == -(-n_ref // 1000)


def test_draws_per_tail_length_are_pythons_int_of_the_float_product():
    from nanosnp_amd import train
    for pn in PN_VALUES:
        for length in range(1, 1001):
            q = sr.draws_per_block(length, 5, pn)
            assert q == [int(length * pn)]
            assert train.pn_sample_count(length, 5, pn) == length + q[0] == sr.sample_count(length, 5, pn)
            assert train.pn_sample_count(2000 + length, 5, pn) == 2000 + length + 2 * int(1000 * pn) + q[0] == sr.sample_count(2000 + length, 5, pn)
    for length in FLOAT_TRAPS:
        assert sr.draws_per_block(length, 5, 0.7) == [length * 7 // 10 - 1]
    assert sr.draws_per_block(90, 5, 0.7) == [62]


def test_sample_count_without_refcalls_or_variants():
    from nanosnp_amd import train
    for pn in PN_VALUES:
        assert train.pn_sample_count(0, 40, pn) == 0 == sr.sample_count(0, 40, pn)
        assert train.pn_sample_count(2090, 0, pn) == 2090 == sr.sample_count(2090, 0, pn)
        assert train.pn_sample_count(0, 0, pn) == 0


@pytest.mark.parametrize("kept,n_ref", [(1, 1), (5, 3), (1025, 999), (1400, 1000), (1400, 1001), (5000, 2090)])
@pytest.mark.parametrize("pn", PN_VALUES)
def test_list_layout(kept, n_ref, pn):
    from nanosnp_amd import train
    cls = sr.flags(kept, n_ref, np.random.default_rng(kept + n_ref))
    samples, meta = sr.train_samples(cls, pn, 2021, 0)
    refs, var = np.flatnonzero(cls[:, 1] == 0), np.flatnonzero(cls[:, 1] != 0)
    assert meta.tolist() == [train.pn_sample_count(n_ref, kept - n_ref, pn), n_ref, kept - n_ref, -(-n_ref // 1000)]
    assert samples.size == meta[0]
    got_refs = samples[cls[samples, 1] == 0]
    assert np.array_equal(got_refs, refs)                                 # every refcall once, in order
    stride = 1000 + (int(1000.0 * pn) if var.size else 0)
    for b, length in enumerate(sr.block_lengths(n_ref)):                 # a block: its refcalls, then its draws
        blk = samples[b * stride:(b + 1) * stride]
        assert np.array_equal(blk[:length], refs[b * 1000:b * 1000 + length])
        assert (cls[blk[length:], 1] != 0).all() and blk.size == length + (int(length * pn) if var.size else 0)


def test_no_variants_gives_the_refcalls_and_no_refcalls_gives_nothing():
    cls = np.zeros((2500, 2), np.uint8)
    samples, meta = sr.train_samples(cls, 0.7, 1, 0)
    assert np.array_equal(samples, np.arange(2500)) and meta.tolist() == [2500, 2500, 0, 3]
    cls[:, 1] = 1
    samples, meta = sr.train_samples(cls, 0.7, 1, 0)
    assert samples.size == 0 and meta.tolist() == [0, 0, 2500, 0]
    samples, meta = sr.train_samples(np.zeros((0, 2), np.uint8), 0.7, 1, 0)
    assert samples.size == 0 and meta.tolist() == [0, 0, 0, 0]


def test_draw_and_seed_each_change_the_draws():
    cls = sr.flags(3000, 1500, np.random.default_rng(4))
    base = sr.train_samples(cls, 0.7, (5 << 32) | 9, 0)[0]
    assert np.array_equal(base, sr.train_samples(cls, 0.7, (5 << 32) | 9, 0)[0])
    for seed, draw in (((5 << 32) | 9, 1), ((5 << 32) | 10, 0), ((6 << 32) | 9, 0)):        # the draw, the low key word, the high key word
        other = sr.train_samples(cls, 0.7, seed, draw)[0]
        assert other.shape == base.shape and not np.array_equal(other, base)
        assert np.array_equal(other[cls[other, 1] == 0], base[cls[base, 1] == 0])


def test_draws_are_uniform_over_the_variants():
    """8 variants, 10 blocks of 1,000 refcalls at pn_value 0.7: 7,000 draws, 875 per variant expected, standard deviation
    sqrt(7000 * 1/8 * 7/8) = 27.7; every count within five of them.  The seed is fixed: the list is a pure function of it."""
    cls = np.zeros((10008, 2), np.uint8)
    var = np.array([3, 1000, 2500, 2501, 6000, 7777, 9000, 10007])
    cls[var, 1] = 1
    samples, meta = sr.train_samples(cls, 0.7, 2021, 0)
    assert meta.tolist() == [17000, 10000, 8, 10]
    drawn = samples[cls[samples, 1] != 0]
    counts = np.array([(drawn == v).sum() for v in var])
    print("draws per variant:", counts.tolist())
    assert counts.sum() == 7000 and (counts > 0).all()
    assert np.abs(counts - 875).max() <= 5 * np.sqrt(7000 * (1 / 8) * (7 / 8))
