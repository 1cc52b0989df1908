"""The training sample list of a HaplotypeModel pass under pn_value upsampling, restated in numpy: Philox4x32-10 and the rules of
nsnp_hap_train_samples (include/nanosnp.h), which follow TrainingDataset.__init__ (HaplotypeModel/dataset_dev.py:190-230).

Refcalls, in order, are cut into blocks of 1,000 (the last holds the remaining 1..1,000); block b of len_b refcalls contributes its refcalls
and then int(len_b * pn_value) variant draws - Python's float product, truncated; draw j of block b is variant (r * n_var) >> 32 with r =
word 0 of Philox at counter {j, b, draw, 0} under the key {seed low, seed high}.  No variant: no draws.  No refcall: an empty list."""
from __future__ import annotations

import numpy as np

BLOCK = 1000
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# counter, key -> output (the first is the Random123 distribution's own vector)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two -> four uint64 arrays holding the 32-bit output words"""
    c = [np.asarray(v, np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]              # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def block_lengths(n_ref):
    """the cut of n_ref refcalls: dataset_dev.py:210-230 (`i + 1000 < len` sends a remainder of exactly 1,000 to the tail branch: the same cut)"""
    out, i = [], 0
    while i < n_ref:
        if i + BLOCK < n_ref:
            out.append(BLOCK); i += BLOCK
        else:
            out.append(n_ref - i); i = n_ref
    return out


def draws_per_block(n_ref, n_var, pn_value):
    return [int(l * pn_value) if n_var > 0 else 0 for l in block_lengths(n_ref)]


def sample_count(n_ref, n_var, pn_value):
    return n_ref + sum(draws_per_block(n_ref, n_var, pn_value))


def block_start(b, pn_value, n_var=1):
    return b * (BLOCK + (int(float(BLOCK) * pn_value) if n_var > 0 else 0))


def train_samples(cls, pn_value, seed, draw):
    """cls uint8 [kept,2] -> (samples int64 [M], meta int64 [4] = {M, refcalls, variants, blocks})"""
    cls = np.asarray(cls, np.uint8).reshape(-1, 2)
    refs, var = np.flatnonzero(cls[:, 1] == 0), np.flatnonzero(cls[:, 1] != 0)
    out, i = [], 0
    lens = block_lengths(refs.size)
    for b, (l, q) in enumerate(zip(lens, draws_per_block(refs.size, var.size, pn_value))):
        assert sum(len(o) for o in out) == block_start(b, pn_value, var.size)
        out.append(refs[i:i + l]); i += l
        if q:
            r = philox4x32_10((np.arange(q), b, draw, 0), (seed & MASK, seed >> 32))[0]
            out.append(var[((r * np.uint64(var.size)) >> np.uint64(32)).astype(np.int64)])
    samples = np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)
    return samples, np.array([samples.size, refs.size, var.size, len(lens)], np.int64)


def flags(kept, n_ref, rng):
    """cls [kept,2] with n_ref refcalls at seeded places; a variant's zygosity byte is 1 or 2, genotypes are arbitrary"""
    cls = np.zeros((kept, 2), np.uint8)
    cls[:, 0] = rng.integers(0, 10, kept)
    cls[:, 1] = rng.integers(1, 3, kept)
    cls[rng.permutation(kept)[:n_ref], 1] = 0
    return cls
