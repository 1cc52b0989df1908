"""Records tests/golden/l0_rsx_parent.npz: the float32 gt / zy of the default fp32 PileupModel forward for the seeded inputs of
tests/test_gpu_l0_lean_step.py, with a sha256 of every input.  The fixture pins the bits of the forward as it was BEFORE the layer-0
step loop lost its bookkeeping (docs/rounds/r13.md), so it is recorded with the parent commit's library on an MI355X:

    git archive <parent> | tar -x -C DIR && cp tests/manual/record_l0_parent.py DIR/tests/manual/
    cd DIR && python __graft_entry__.py && python -m tests.manual.record_l0_parent OUT.npz

cases() is also what the test regenerates its inputs from."""
import hashlib
import sys

import numpy as np

SIZES = (1, 15, 16, 17, 33, 200)        # ragged last workgroups of 16 sites, nrows < 16
BIG = (257, 65536, 2**24 + 3)           # two bf16 terms, two, three: split levels 1, 1, 2


def _counts(rng, shape):
    return rng.integers(-15, 61, shape).astype(np.int32)


def cases():
    """name -> (x int32 [n, 33, 18], None) for nsnp_pileup_forward or (counts int32 [L, 18], center_idx int64 [n]) for the in-place
    windows entry"""
    out = {}
    for n in SIZES:
        out[f"n{n}"] = (_counts(np.random.default_rng(1300 + n), (n, 33, 18)), None)
    # overlapping windows read in place, in no order: 64-bit offsets of either sign between the sites of a workgroup
    rng = np.random.default_rng(1350)
    counts = _counts(rng, (120, 18))
    out["windows50"] = (counts, rng.permutation(np.arange(16, 104, dtype=np.int64))[:50].copy())
    # three workgroups; in each, one count per staging wave (wave 0 stages channels 0..7, wave 1 channels 8..15, wave 2 channels
    # 16, 17), the three values rotated over the waves from group to group, at different steps and beside small-count sites; steps
    # 5 and 7 share a staging buffer, so the second must find the first's planes 1 and 2 rewritten
    x = _counts(np.random.default_rng(1348), (48, 33, 18))
    for g in range(3):
        v = BIG[g:] + BIG[:g]
        x[16 * g + 3, 5, 2] = v[0]
        x[16 * g + 9, 8, 11] = v[1]
        x[16 * g + 14, 12, 17] = v[2]
        x[16 * g + 6, 7, 13] = 257
        x[16 * g + 12, 20, 16] = -v[2]
    out["big48"] = (x, None)
    return out


def digest(a, b):
    h = hashlib.sha256(np.ascontiguousarray(a).tobytes())
    if b is not None:
        h.update(np.ascontiguousarray(b).tobytes())
    return h.hexdigest()


def forward(ctx, a, b):
    import torch
    at = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g, z = ctx.pileup_forward(at) if b is None else ctx.pileup_forward_windows(at, torch.from_numpy(b).cuda())
    torch.cuda.synchronize()
    return g.cpu().numpy(), z.cpu().numpy()


def main(path):
    from nanosnp_amd import _lib
    from nanosnp_amd.fixtures import load_pileup_weights
    ctx = _lib.Context(0)
    ctx.pileup_load_weights(load_pileup_weights())
    rec = {}
    for name, (a, b) in cases().items():
        g, z = forward(ctx, a, b)
        assert g.dtype == np.float32 and z.dtype == np.float32 and np.isfinite(g).all() and np.isfinite(z).all()
        rec[name + "_gt"], rec[name + "_zy"], rec[name + "_sha256"] = g, z, np.array(digest(a, b))
    ctx.close()
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {len(rec) // 3} cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "tests/golden/l0_rsx_parent.npz")
